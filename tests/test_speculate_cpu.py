"""Speculative greedy decoding without a GPU: the rule in plain Python (speculate.py), the host loop's truncation arithmetic
against a pure-Python model of the plain loop, the fixture's stored statistics recomputed from its stored tokens, and the
server's parsing of "speculate" with a stub engine."""
import json
import os
import sys
import threading
import urllib.error
import urllib.request

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def spec():
    from phi_3_vision_mlx_amd import speculate
    return speculate


# ----------------------------------------------------------------------------- propose
def test_propose_most_recent_occurrence_wins():
    s = spec()
    #      0  1  2  3  4  5  6  7  8
    ctx = [5, 6, 7, 1, 5, 6, 8, 2, 5, 6]
    assert s.propose(ctx, 2, n_max=2, n_min=1) == [8, 2]                  # (5, 6) at 0 and at 4: the later one
    assert s.propose(ctx, 4, n_max=2, n_min=1) == [8, 2, 5, 6]
    assert s.propose([1, 2, 1, 3, 1], 3, n_max=1, n_min=1) == [3, 1]       # 1 at 0 and 2: position 2 wins


def test_propose_longer_ngram_wins_over_a_more_recent_shorter_one():
    s = spec()
    ctx = [1, 2, 3, 9, 9, 3, 7, 1, 2, 3]
    # the 3-gram (1, 2, 3) occurs at 0 -> draft 9 9 3; the 1-gram (3) occurs more recently at 5 -> would give 7
    assert s.propose(ctx, 3, n_max=3, n_min=1) == [9, 9, 3]
    assert s.propose(ctx, 3, n_max=1, n_min=1) == [7, 1, 2]
    # no 3-gram or 2-gram match: falls through to the 1-gram
    assert s.propose([4, 5, 6, 4], 2, n_max=3, n_min=1) == [5, 6]
    # n_min = 2: the 1-gram is never tried
    assert s.propose([4, 5, 6, 4], 2, n_max=3, n_min=2) == []


def test_propose_short_draft_at_the_end_and_tiny_contexts():
    s = spec()
    assert s.propose([7, 7], 4, n_max=3, n_min=1) == [7]                    # continuation runs into the end: one token
    assert s.propose([1, 2, 3, 1, 2], 4, n_max=2, n_min=1) == [3, 1, 2]     # min(p + m + K, n) cuts at n
    assert s.propose([], 4) == []
    assert s.propose([3], 4) == []                                          # n <= m for every m
    assert s.propose([3, 3], 4, n_max=3, n_min=2) == []                     # m = 2 >= n = 2 is skipped, m = 3 too
    assert s.propose([3, 4], 4) == []                                       # no match at any m
    assert s.propose([1, 2, 1, 2], 0) == []                                 # K = 0


def test_propose_cuts_at_out_of_vocabulary_ids():
    s = spec()
    ctx = [1, 2, 50, -3, 4, 1, 2]
    assert s.propose(ctx, 4, n_max=2, n_min=1, vocab=100) == [50]           # the image-slot id -3 is never proposed
    assert s.propose(ctx, 4, n_max=2, n_min=1, vocab=50) == []              # 50 is outside [0, 50): empty draft, search over
    assert s.propose([1, -1, 9, 1], 4, n_max=1, n_min=1, vocab=100) == []   # the match exists, its draft is cut to nothing
    # a negative id inside the SUFFIX still matches as an id
    assert s.propose([-5, 8, 9, -5], 2, n_max=1, n_min=1, vocab=100) == [8, 9]


def test_propose_brute_force_agreement():
    s = spec()
    rng = np.random.default_rng(0)

    def brute(ctx, K, n_max, n_min, vocab):
        n = len(ctx)
        for m in range(n_max, n_min - 1, -1):
            if m >= n:
                continue
            cands = [p for p in range(n - m) if ctx[p:p + m] == ctx[n - m:]]
            if cands:
                p = max(cands)
                d = ctx[p + m:min(p + m + K, n)]
                for i, t in enumerate(d):
                    if not 0 <= t < vocab:
                        return d[:i]
                return d
        return []
    for _ in range(300):
        n = int(rng.integers(0, 40))
        ctx = rng.integers(-1, 4, n).tolist()
        K, n_max = int(rng.integers(0, 8)), int(rng.integers(1, 5))
        n_min = int(rng.integers(1, n_max + 1))
        assert s.propose(ctx, K, n_max, n_min, vocab=3) == brute(ctx, K, n_max, n_min, 3), (ctx, K, n_max, n_min)


# ----------------------------------------------------------------------------- accept
def test_accept_none_partial_full():
    s = spec()
    assert s.accept([], [9]) == (0, [9])
    assert s.accept([1, 2, 3], [5, 2, 3, 4]) == (0, [5])
    assert s.accept([1, 2, 3], [1, 2, 7, 4]) == (2, [1, 2, 7])
    assert s.accept([1, 2, 3], [1, 2, 3, 4]) == (3, [1, 2, 3, 4])
    assert s.accept([1, 2], [1, -1, 5]) == (1, [1, -1])                     # a NaN row inside the run ends it
    assert s.accept([1, 2], [7, -1, 5]) == (0, [7])                         # ... behind the run: not looked at
    assert s.step([0] * 5, [1, 2], [1, -1, 5]) == [1, -1]
    assert s.step([0] * 5, [1, 2, 3], [1, 2, 3, 4], n_limit=7) == [1, 2]    # the budget cuts the emitted run
    assert s.step([0] * 5, [1, 2, 3], [1, 2, 3, 4], n_limit=5) == []


# ----------------------------------------------------------------------------- the loop's truncation arithmetic
def scripted(seq):
    """A "model" that continues any context with a fixed periodic sequence, by position."""
    def next_token(ctx):
        return seq[len(ctx) % len(seq)]
    return next_token


def plain_loop(prompt, first, next_token, max_tokens, stop_id):
    """The plain greedy loop (api._generate + greedy_loop): the prefill token, then max_tokens - 1 steps, stopping behind a stop
    token (the prefill token is not checked)."""
    ctx, out = list(prompt) + [first], [first]
    for _ in range(max_tokens - 1):
        t = next_token(ctx)
        ctx.append(t)
        out.append(t)
        if t == stop_id:
            break
    return out


@pytest.mark.parametrize("K", [1, 4, 7])
@pytest.mark.parametrize("max_tokens", [1, 2, 3, "K+2", 23])
def test_loop_truncation_matches_the_plain_loop(K, max_tokens):
    s = spec()
    mt = K + 2 if max_tokens == "K+2" else max_tokens
    seq = [3, 4, 5, 3, 4, 6]
    prompt = [seq[i % len(seq)] for i in range(18)]
    nt = scripted(seq)
    first = nt(prompt)
    for stop in (None, 6, 5):
        stats = {}
        got = s.run(prompt, first, nt, mt, K, stop_id=stop, stats=stats)
        want = plain_loop(prompt, first, nt, mt, stop)
        assert got[:len(want)] == want
        assert s.truncate(got, mt, stop) == want
        assert len(s.truncate(got, mt, None)) == mt if stop is None else True
        assert stats["emitted"] == stats["steps"] + stats["accepted"]
        if mt > 3 and stop is None:
            assert stats["accepted"] > 0                                    # the periodic script is drafted and accepted


def test_stop_token_in_the_middle_of_an_accepted_run():
    s = spec()
    seq = [10, 11, 12, 13]
    prompt = seq * 4
    nt = scripted(seq)
    got = s.run(prompt, nt(prompt), nt, 12, 4, stop_id=12)
    # the run [11, 12, 13, 10, ...] is accepted whole; the output is cut behind the stop token 12
    assert got == [10, 11, 12] == plain_loop(prompt, nt(prompt), nt, 12, 12)


# ----------------------------------------------------------------------------- fixture
def test_fixture_statistics_reproduce_from_its_tokens():
    sys.path.insert(0, GOLDEN)
    try:
        import gen_golden_spec as gs
    finally:
        sys.path.remove(GOLDEN)
    fx = np.load(os.path.join(GOLDEN, "tiny_spec_oracle.npz"))
    toks, mg = fx["tokens"].reshape(-1), fx["margins"].reshape(-1)
    assert toks.size == gs.STEPS
    unclear = np.nonzero(mg <= 1.0)[0]
    first_unclear = int(unclear[0]) if unclear.size else gs.STEPS
    assert first_unclear == int(fx["first_unclear"][0]) >= gs.NEED_CLEAR
    assert len(set(toks.tolist())) >= gs.MIN_DISTINCT
    from phi_3_vision_mlx_amd.config import make_config, tiny_config_dict
    vocab = make_config(tiny_config_dict(vision=False)).vocab_size
    sim = gs.simulate(fx["ids"], toks.tolist(), int(fx["sim_k"][0]), vocab)
    assert list(sim) == fx["sim"].tolist()
    assert sim[2] >= gs.MIN_ACCEPTED and sim[3] >= gs.MIN_REJECT
    from phi_3_vision_mlx_amd.processor import Phi3VProcessor
    ids = np.asarray(Phi3VProcessor(None)(gs.chat_text())["input_ids"]).reshape(-1)
    assert np.array_equal(ids, fx["ids"])


# ----------------------------------------------------------------------------- API surface
def test_surface_and_refusals_without_a_gpu():
    import inspect
    import phi_3_vision_mlx_amd as pkg
    from phi_3_vision_mlx_amd import api, _lib
    assert inspect.signature(api.generate).parameters["speculate"].default == 0
    assert inspect.signature(api._generate).parameters["speculate"].default == 0
    assert inspect.signature(api._generate).parameters["spec_info"].default is None
    assert "speculate" not in inspect.signature(pkg.generate).parameters        # the reference's exact signature
    assert spec().MAX_K == _lib.DECODE_MAX_L - 1
    h = open(os.path.join(ROOT, "include", "p3v.h")).read()
    assert f"#define P3V_SPEC_DEFAULT_K {spec().DEFAULT_K}\n" in h
    assert f"#define P3V_SPEC_NGRAM_MAX {spec().N_MAX}\n" in h and f"#define P3V_SPEC_NGRAM_MIN {spec().N_MIN}\n" in h
    assert f"#define P3V_SPEC_REC_INTS {_lib.SPEC_REC_INTS}\n" in h and f"#define P3V_SPEC_CTL_INTS {_lib.SPEC_CTL_INTS}\n" in h
    for i, name in enumerate(("N", "NDRAFT", "FORCED", "REPLAY", "NLIMIT", "ACC")):
        assert f"#define P3V_SPEC_CTL_{name} {i}\n" in h and getattr(_lib, "SPEC_CTL_" + name) == i
    # struct layout == header field order
    body = h[h.rindex("typedef struct {", 0, h.index("} p3v_spec_state_t")):h.index("} p3v_spec_state_t")]
    import re
    names = re.findall(r"\b(\w+)\s*[;,]", body)
    assert names == [f for f, _ in _lib.SpecState._fields_]

    class Stub:
        def spec_refusal(self, st=None, K=None):
            return None if K <= 15 else "speculate must be 1 .. 15 (P3V_DECODE_MAX_L - 1 draft rows)"
    with pytest.raises(ValueError, match="B = 1"):
        api._check_speculate(Stub(), 4, True, False, False)
    with pytest.raises(ValueError, match="temperature"):
        api._check_speculate(Stub(), 4, False, True, False)
    with pytest.raises(ValueError, match="early_stop"):
        api._check_speculate(Stub(), 4, False, False, True)
    with pytest.raises(ValueError, match="15"):
        api._check_speculate(Stub(), 16, False, False, False)
    with pytest.raises(ValueError, match=">= 0"):
        api._check_speculate(Stub(), -1, False, False, False)
    assert api._check_speculate(Stub(), 4, False, False, False) == 4


# ----------------------------------------------------------------------------- server
def _post(port, payload):
    req = urllib.request.Request(f"http://127.0.0.1:{port}/v1/completions", data=json.dumps(payload).encode(),
                                 headers={"Content-Type": "application/json"})
    with urllib.request.urlopen(req, timeout=10) as r:
        return r.status, json.loads(r.read())


def _serve(**kw):
    from phi_3_vision_mlx_amd.server import serve
    calls = []

    def fake_generate(prompts, max_tokens, images=None, sampling=None, adapter=None, speculate=0, spec_info=None):
        calls.append((list(prompts), max_tokens, speculate))
        if spec_info is not None:
            spec_info.update(steps=3, drafted=8, accepted=5, emitted=8)
        out = [f"{p}|{max_tokens}|{speculate}" for p in prompts]
        return out[0] if len(out) == 1 else out
    httpd, engine = serve(fake_generate, port=0, host="127.0.0.1", **kw)
    threading.Thread(target=httpd.serve_forever, daemon=True).start()
    return httpd, engine, calls


def _expect_400(port, payload, word):
    with pytest.raises(urllib.error.HTTPError) as e:
        _post(port, payload)
    assert e.value.code == 400
    assert word in json.loads(e.value.read())["error"]


def test_server_speculate_field():
    httpd, engine, calls = _serve(speculate=True)
    port = httpd.server_address[1]
    try:
        code, out = _post(port, {"prompt": "hi", "max_tokens": 9, "speculate": 4})
        assert code == 200 and out["responses"] == ["hi|9|4"]
        assert out["speculation"] == {"steps": 3, "drafted": 8, "accepted": 5}
        code, out = _post(port, {"prompt": "hi", "max_tokens": 9})
        assert out == {"model": "phi-3-vision", "responses": ["hi|9|0"]}                     # absent: off, no new field
        assert _post(port, {"prompt": "hi", "speculate": 0})[1] == {"model": "phi-3-vision", "responses": ["hi|512|0"]}
        assert _post(port, {"prompt": "hi", "speculate": 15})[1]["responses"] == ["hi|512|15"]
        _expect_400(port, {"prompt": "hi", "speculate": 16}, "0 .. 15")
        _expect_400(port, {"prompt": "hi", "speculate": -1}, "0 .. 15")
        _expect_400(port, {"prompt": "hi", "speculate": "4"}, "integer")
        _expect_400(port, {"prompt": "hi", "speculate": True}, "integer")
        _expect_400(port, {"prompt": "hi", "speculate": 2.0}, "integer")
        _expect_400(port, {"prompt": ["a", "b"], "speculate": 4}, "one prompt")
        _expect_400(port, {"prompt": "hi", "speculate": 4, "temperature": 0.7}, "greedy")
        assert _post(port, {"prompt": "hi", "speculate": 4, "temperature": 0.0, "seed": 1})[0] == 200
    finally:
        httpd.shutdown()
        engine.close()


def test_server_speculate_default_flag_and_unsupported_backends():
    httpd, engine, calls = _serve(speculate=True, speculate_default=3)
    port = httpd.server_address[1]
    try:
        code, out = _post(port, {"prompt": "hi", "max_tokens": 5})
        assert out["responses"] == ["hi|5|3"] and "speculation" in out                      # the flag's default applies
        assert _post(port, {"prompt": "hi", "max_tokens": 5, "speculate": 0})[1]["responses"] == ["hi|5|0"]
        assert _post(port, {"prompt": ["a", "b"], "max_tokens": 5})[1]["responses"] == ["a|5|0", "b|5|0"]   # default only where it can run
    finally:
        httpd.shutdown()
        engine.close()
    httpd, engine, calls = _serve(speculate=True, merge=True)                              # --merge: B > 1 batches
    port = httpd.server_address[1]
    try:
        _expect_400(port, {"prompt": "hi", "speculate": 4}, "--merge")
        assert _post(port, {"prompt": "hi"})[0] == 200
    finally:
        httpd.shutdown()
        engine.close()
    from http.server import ThreadingHTTPServer
    from phi_3_vision_mlx_amd.server import make_handler

    class Continuous:                                                                      # what ContinuousBackend offers the handler
        def submit(self, prompts, max_tokens, images=None, **kw):
            return [p + "!" for p in prompts]
    httpd = ThreadingHTTPServer(("127.0.0.1", 0), make_handler(Continuous()))
    threading.Thread(target=httpd.serve_forever, daemon=True).start()
    try:
        _expect_400(httpd.server_address[1], {"prompt": "hi", "speculate": 4}, "--continuous")
        assert _post(httpd.server_address[1], {"prompt": "hi"})[1]["responses"] == ["hi!"]
    finally:
        httpd.shutdown()
