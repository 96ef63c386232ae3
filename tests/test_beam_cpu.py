"""Beam search without a GPU: the rule (beam.reference_step) on hand-made rows, the host search (beam.Search) against a
full-width enumeration and against itself without the DONE test, the record layout against the header, and every refusal
of the public surface before any model call."""
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NINF = float("-inf")


def to_bits(x):
    return torch.as_tensor(np.asarray(x, dtype=np.float32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16).copy()


def f32(bits):
    return np.asarray(bits, dtype=np.int32).view(np.float32)


def _step(x, cum, W, eos):
    from phi_3_vision_mlx_amd import beam
    rec = beam.reference_step(to_bits(np.atleast_2d(x)), np.asarray(cum, dtype=np.float32), W, eos)
    return rec, beam.unpack(rec, W)


# ---------------------------------------------------------------------------------------------------- the rule
def test_record_layout_matches_the_header():
    from phi_3_vision_mlx_amd import _lib, beam
    src = open(os.path.join(ROOT, "include", "p3v.h")).read()
    assert int(re.search(r"#define P3V_BEAM_MAX (\d+)", src).group(1)) == beam.MAX == _lib.BEAM_MAX == 8
    assert "#define P3V_BEAM_REC_INTS (2 + 5 * P3V_BEAM_MAX)" in src and beam.REC_INTS == _lib.BEAM_REC_INTS == 42
    body = re.search(r"typedef struct \{([^}]*)\} p3v_beam_state_t;", src).group(1)
    names = re.findall(r"\*?\s*(\w+);", body)
    assert names == [f for f, _ in _lib.BeamState._fields_]


def test_ties_go_to_the_lower_row_then_the_lower_index():
    W = 3
    rec, u = _step(np.ones((W, 8)), [0.0, 0.0, 0.0], W, eos=7)
    assert u["status"] == 0 and u["tok"] == [0, 1, 2] and u["parent"] == [0, 0, 0] and u["fin"] == []
    assert len({c for c in u["cum"]}) == 1 and abs(u["cum"][0] - math.log(1 / 8)) < 1e-6
    assert (rec[2 + W:10] == -1).all() and (rec[10 + W:18] == -1).all() and (rec[26:] == -1).all()      # unused entries
    # the better cum wins whatever the row index; equal cum and equal logits: the lower row first
    _, u = _step(np.ones((W, 8)), [-1.0, 0.0, 0.0], W, eos=7)
    assert u["parent"] == [1, 1, 1] and u["tok"] == [0, 1, 2]
    x = np.zeros((2, 6))
    x[:, 4] = 1.0
    _, u = _step(x, [0.0, 0.0], 2, eos=5)
    assert list(zip(u["parent"], u["tok"])) == [(0, 4), (1, 4)]


def test_eos_is_recorded_below_order_index_w_and_ignored_from_it():
    W = 4
    x = np.full((1, 16), -30.0)
    ids = [9, 3, 12, 0, 7, 5, 1, 14]
    x[0, ids] = 8.0 - 0.5 * np.arange(8)
    _, u = _step(x, [0.0], W, eos=ids[W - 1])                            # order index W - 1: recorded
    assert u["tok"] == [9, 3, 12, 7] and len(u["fin"]) == 1 and u["fin"][0][0] == 0
    lp = u["fin"][0][1]
    assert u["cum"][2] > lp > u["cum"][3]
    _, u = _step(x, [0.0], W, eos=ids[W])                                # order index W: ignored
    assert u["tok"] == [9, 3, 12, 0] and u["fin"] == []
    _, u = _step(x, [0.0], W, eos=ids[0])                                # first of all: recorded, W beams follow
    assert u["tok"] == [3, 12, 0, 7] and len(u["fin"]) == 1


def test_one_prefill_row_and_minus_inf_candidates_fill_the_beams():
    W = 4
    x = np.full((1, 9), NINF)
    x[0, [6, 2, 4]] = [1.0, 0.5, 0.0]
    rec, u = _step(x, [0.0], W, eos=2)
    assert u["tok"] == [6, 4, 0, 1] and u["parent"] == [0] * W           # two finite beams, then -inf ones in index order
    assert u["cum"][2:] == [NINF, NINF] and u["cum"][0] > u["cum"][1] > NINF
    assert [p for p, _ in u["fin"]] == [0] and u["cum"][0] > u["fin"][0][1] > u["cum"][1]
    # a beam whose sum is -inf keeps -inf (an ordinary value), behind every finite candidate
    y = np.zeros((W, 9))
    _, u = _step(y, [NINF, -5.0, NINF, -1.0], W, eos=8)
    assert u["parent"] == [3, 3, 3, 3] and not any(math.isnan(c) for c in u["cum"])


def test_undefined_rows_fail_the_step():
    from phi_3_vision_mlx_amd import beam
    W = 2
    for bad in (float("nan"), float("inf")):
        x = np.zeros((W, 8))
        x[1, 3] = bad
        rec, u = _step(x, [0.0, 0.0], W, eos=0)
        assert rec[0] == 1 and rec[1] == 0 and (rec[2:] == -1).all() and u["tok"] == [-1, -1]
        with pytest.raises(RuntimeError, match="failed"):
            beam.Search(W, 4, 0).add(rec)
    rec, _ = _step(np.full((1, 8), NINF), [0.0], W, eos=0)               # no finite logit
    assert rec[0] == 1
    for args in ((np.zeros((3, 8)), [0, 0, 0], 2), (np.zeros((1, 3)), [0], 2), (np.zeros((1, 40)), [0], 9), (np.zeros((1, 40)), [0], 1)):
        with pytest.raises(ValueError):
            beam.reference_step(to_bits(args[0]), np.asarray(args[1], np.float32), args[2], 0)


# ---------------------------------------------------------------------------------------------------- the host search
class Scripted:
    """A model whose logits depend on the token sequence alone: a seeded table per (depth, last token)."""

    def __init__(self, n, seed, finite=None, scale=2.0, boost=None):
        self.n, self.seed, self.finite, self.scale, self.boost = n, seed, finite, scale, boost

    def row(self, seq):
        rng = np.random.default_rng([self.seed, len(seq)] + [int(t) for t in seq[-2:]])
        x = (rng.standard_normal(self.n) * self.scale).astype(np.float32)
        if self.boost is not None:
            x[self.boost[0]] += self.boost[1]                             # an EOS likely enough for hypotheses to finish
        if self.finite is not None:
            y = np.full(self.n, NINF, np.float32)
            y[self.finite] = x[self.finite]
            x = y
        return x


def run_search(model, W, max_tokens, eos, length_penalty, prune=True):
    """beam.Search driven by beam.reference_step: what the device loop does, one record per step."""
    from phi_3_vision_mlx_amd import beam
    s = beam.Search(W, max_tokens, eos, length_penalty, prune=prune)
    seqs, cum = [[]], np.zeros(1, np.float32)
    while True:
        rec = beam.reference_step(to_bits(np.stack([model.row(q) for q in seqs])), cum, W, eos)
        u = beam.unpack(rec, W)
        seqs = [seqs[p] + [t] for p, t in zip(u["parent"], u["tok"])]
        cum = f32(rec[18:18 + W]).copy()
        if s.add(rec):
            return s


def full_width(model, W, max_tokens, eos, length_penalty, finite):
    """Every sequence over the finite ids, depth by depth, nothing pruned among the live prefixes: all their children are
    ordered at once and point 4 of the rule is applied to that order (an EOS counts iff fewer than W entries precede it;
    at the budget the W best live children enter unfinished).  Scores are summed prefix by prefix in fp32, as the rule does."""
    from phi_3_vision_mlx_amd import beam
    live, pool = [([], np.float32(0))], []
    for t in range(max_tokens):
        kids = []
        for r, (seq, c) in enumerate(live):
            lp = beam.row_logprobs(to_bits(model.row(seq)))
            x = beam.bf16_values(to_bits(model.row(seq)))
            order = sorted(finite, key=lambda i: (-x[i], i))
            kids += [(np.float32(c + lp[i]), r, place, seq + [int(i)]) for place, i in enumerate(order)]
        kids.sort(key=lambda k: (-float(k[0]), k[1], k[2]))
        nxt = []
        for j, (s, _, _, seq) in enumerate(kids):
            if seq[-1] == eos:
                if j < W:
                    pool.append((-(float(s) / (t + 1) ** length_penalty), t, j, seq, float(s), True))
            else:
                nxt.append((seq, s))
        assert len(nxt) <= W or t == max_tokens - 1                     # no live finite prefix is ever pruned before the budget
        if t == max_tokens - 1:
            pool += [(-(float(s) / max_tokens ** length_penalty), t, 8 + k, seq, float(s), False) for k, (seq, s) in enumerate(nxt[:W])]
        live = nxt
    pool.sort(key=lambda e: e[:3])
    return [dict(token_ids=e[3], score=-e[0], sum_logprob=e[4], finished=e[5]) for e in pool[:W]]


@pytest.mark.parametrize("length_penalty", [0, 0.5, 1, 2])
def test_search_equals_the_full_width_enumeration(length_penalty):
    """16 ids, 3 finite (one the EOS), max_tokens = 4, W = 8: 2^d <= 8 live finite prefixes at every depth d <= 3, so the
    beam prunes none of them and the pool must be the enumeration's."""
    finite, eos, W = [2, 7, 11], 7, 8
    for seed in range(6):
        model = Scripted(16, seed, finite=finite, scale=1.0)
        got = run_search(model, W, 4, eos, length_penalty, prune=False).result()
        want = full_width(model, W, 4, eos, length_penalty, finite)
        assert got == want, (seed, got, want)
        assert all(set(h["token_ids"]) <= set(finite) and math.isfinite(h["score"]) for h in got)
        pruned = run_search(model, W, 4, eos, length_penalty).result()
        assert pruned == got


def test_pruning_is_exact_on_random_models():
    """The DONE test is a bound, not a heuristic: with it the search returns what it returns when run to the budget."""
    rng = np.random.default_rng(2024)
    stopped_early = 0
    for case in range(200):
        n, W = int(rng.integers(16, 41)), int(rng.integers(2, 9))
        max_tokens, lp = int(rng.integers(2, 13)), float(rng.choice([0.0, 0.5, 1.0, 2.0]))
        eos = int(rng.integers(0, n))
        model = Scripted(n, case, scale=float(rng.choice([0.5, 2.0, 4.0])), boost=(eos, float(rng.choice([0.0, 2.0, 4.0]))))
        a, b = run_search(model, W, max_tokens, eos, lp), run_search(model, W, max_tokens, eos, lp, prune=False)
        assert a.result() == b.result(), (case, n, W, max_tokens, lp)
        assert len(a.steps) <= len(b.steps) == max_tokens
        stopped_early += len(a.steps) < max_tokens
    assert stopped_early > 10                                            # the property was exercised


def test_search_arguments():
    from phi_3_vision_mlx_amd import beam
    for W in (1, 9, 0, -2, 2.0, True, "4", None):
        with pytest.raises(ValueError, match="2..8"):
            beam.Search(W, 4, 0)
    for lp in (-0.1, float("nan"), float("inf"), "1", None, True):
        with pytest.raises(ValueError, match="length_penalty"):
            beam.Search(2, 4, 0, lp)
    for mt in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="max_tokens"):
            beam.Search(2, mt, 0)
    assert beam.Search(2, 4, 0).lp == 1.0


# ---------------------------------------------------------------------------------------------------- the public surface
def test_defaults_and_signatures():
    import phi_3_vision_mlx_amd as pkg
    from phi_3_vision_mlx_amd import api, server
    for fn in (api.generate, api._generate):
        p = inspect.signature(fn).parameters
        assert (p["num_beams"].default, p["length_penalty"].default, p["beam_info"].default) == (1, 1.0, None)
    assert not {"num_beams", "length_penalty", "beam_info"} & set(inspect.signature(pkg.generate).parameters)   # the reference's signature
    assert inspect.signature(server.in_use).parameters["beam"].default is None
    assert server.in_use() == {} and server.in_use(beam={"num_beams": 2, "length_penalty": 1.0}) == {"beam": {"num_beams": 2, "length_penalty": 1.0}}
    assert "P3V_BEAM_MAX" in open(os.path.join(ROOT, "include", "p3v.h")).read()


API_REFUSALS = [
    (dict(num_beams=9), "2..8"), (dict(num_beams=0), "2..8"), (dict(num_beams=-3), "2..8"), (dict(num_beams=2.0), "2..8"),
    (dict(num_beams=True), "2..8"), (dict(num_beams="4"), "2..8"),
    (dict(num_beams=2, length_penalty=-0.5), "length_penalty"), (dict(num_beams=2, length_penalty=float("nan")), "length_penalty"),
    (dict(num_beams=2, length_penalty=float("inf")), "length_penalty"), (dict(num_beams=1, length_penalty=-1), "length_penalty"),
    (dict(num_beams=2, temperature=0.7), "temperature"), (dict(num_beams=2, speculate=4), "speculate"),
    (dict(num_beams=2, n=2), "best_of"), (dict(num_beams=2, best_of=3), "best_of"), (dict(num_beams=2, logprobs=0), "logprobs"),
    (dict(num_beams=2, repetition_penalty=1.2), "penalties"), (dict(num_beams=2, presence_penalty=0.5), "penalties"),
    (dict(num_beams=2, frequency_penalty=0.5), "penalties"), (dict(num_beams=2, logit_bias={5: -1.0}), "logit_bias"),
    (dict(num_beams=2, guided_regex="a+"), "guided"), (dict(num_beams=2, guided_choice=["a", "b"]), "guided"),
    (dict(num_beams=2, guided_json={"type": "boolean"}), "guided"), (dict(num_beams=2, early_stop=True), "early_stop"),
    (dict(num_beams=2, adapter="x"), "adapter"),
]


@pytest.mark.parametrize("kw,word", API_REFUSALS, ids=[f"{i}-{w}" for i, (_, w) in enumerate(API_REFUSALS)])
def test_generate_refuses_before_any_model_call(kw, word):
    """A ValueError that names the limit; the preload is never touched (it is a pair of Nones)."""
    from phi_3_vision_mlx_amd import api
    with pytest.raises(ValueError, match=re.escape(word)):
        api.generate("hi", preload=(None, None), verbose=False, **kw)
    with pytest.raises(ValueError, match=re.escape(word)):
        api._generate(None, None, "hi", verbose=False, **kw)


def test_generate_refuses_a_list_of_prompts_and_models_without_the_step():
    from phi_3_vision_mlx_amd import api
    with pytest.raises(ValueError, match="one prompt"):
        api.generate(["a", "b"], preload=(None, None), num_beams=2)

    class Plain:                                                          # a model class without the captured beam step
        pass
    with pytest.raises(ValueError, match="captured step"):
        api._generate(Plain(), None, "hi", num_beams=2)

    class Int8:
        def beam_refusal(self, st=None, W=None):
            return "beam search needs the bf16 KV cache: the reorder has no int8 form"

        def family_refusal(self, st=None):
            return None
    with pytest.raises(ValueError, match="int8"):
        api._generate(Int8(), None, "hi", num_beams=2)


# ---------------------------------------------------------------------------------------------------- the server
def _post(port, payload):
    import json
    import urllib.request
    req = urllib.request.Request(f"http://127.0.0.1:{port}/v1/completions", data=json.dumps(payload).encode(),
                                 headers={"Content-Type": "application/json"})
    with urllib.request.urlopen(req, timeout=10) as r:
        return r.status, json.loads(r.read())


def _expect_400(port, payload, word):
    import json
    import urllib.error
    with pytest.raises(urllib.error.HTTPError) as e:
        _post(port, payload)
    assert e.value.code == 400
    assert word in json.loads(e.value.read())["error"], word


def _serve(**kw):
    import threading
    from phi_3_vision_mlx_amd.server import serve
    calls = []

    def fake_generate(prompts, max_tokens, images=None, beam=None, beam_info=None, **rest):
        calls.append((list(prompts), max_tokens, beam, sorted(rest)))
        if beam_info is not None:
            beam_info.update(hypotheses=[dict(token_ids=[1, 2], score=-0.75, sum_logprob=-1.5, finished=True)], steps=5)
        out = [f"{p}|{max_tokens}|{(beam or {}).get('num_beams', 1)}" for p in prompts]
        return out[0] if len(out) == 1 else out
    httpd, engine = serve(fake_generate, port=0, host="127.0.0.1", **kw)
    threading.Thread(target=httpd.serve_forever, daemon=True).start()
    return httpd, engine, calls


def test_server_fields_response_and_refusals():
    httpd, engine, calls = _serve(beam=True, speculate=True, speculate_default=3, adapter_names=["x"], sharded_fn=lambda p, i: False)
    port = httpd.server_address[1]
    try:
        code, out = _post(port, {"prompt": "hi", "max_tokens": 9, "num_beams": 4, "length_penalty": 0.5})
        assert code == 200 and out["responses"] == ["hi|9|4"] and out["beam"] == {"score": -0.75, "steps": 5}
        assert calls[-1] == (["hi"], 9, {"num_beams": 4, "length_penalty": 0.5}, [])       # the --speculate default stepped aside
        assert "speculation" not in out and "cached_tokens" not in out
        assert _post(port, {"prompt": "hi", "num_beams": 2})[1]["beam"]["steps"] == 5 and calls[-1][2] == {"num_beams": 2, "length_penalty": 1.0}
        code, out = _post(port, {"prompt": "hi", "max_tokens": 9, "num_beams": 1, "speculate": 0})
        assert out == {"model": "phi-3-vision", "responses": ["hi|9|1"]} and calls[-1][2] is None      # 1: today's request
        assert _post(port, {"prompt": "hi", "num_beams": 2, "temperature": 0.0, "seed": 3})[0] == 200
        for body, word in (({"num_beams": 9}, "2..8"), ({"num_beams": 0}, "2..8"), ({"num_beams": "4"}, "2..8"), ({"num_beams": True}, "2..8"),
                           ({"num_beams": 2.5}, "2..8"), ({"num_beams": 2, "length_penalty": -1}, "length_penalty"),
                           ({"length_penalty": "x"}, "length_penalty"), ({"num_beams": 2, "temperature": 0.7}, "temperature"),
                           ({"num_beams": 2, "speculate": 4}, "speculate"), ({"num_beams": 2, "n": 2}, "best_of"),
                           ({"num_beams": 2, "best_of": 2}, "best_of"), ({"num_beams": 2, "logprobs": 1}, "logprobs"),
                           ({"num_beams": 2, "repetition_penalty": 1.3}, "penalties"), ({"num_beams": 2, "logit_bias": {"5": -1}}, "penalties"),
                           ({"num_beams": 2, "guided_regex": "a+"}, "guided"), ({"num_beams": 2, "guided_choice": ["a", "b"]}, "guided"),
                           ({"num_beams": 2, "adapter": "x"}, "adapter")):
            _expect_400(port, dict({"prompt": "hi"}, **body), word)
        _expect_400(port, {"prompt": ["a", "b"], "num_beams": 2}, "one prompt")
        _expect_400(port, {"prompt": ["a"], "num_beams": 2}, "one prompt")
    finally:
        httpd.shutdown()
        engine.close()


def test_server_backends_without_beams():
    import threading
    from http.server import ThreadingHTTPServer
    from phi_3_vision_mlx_amd.server import make_handler
    httpd, engine, calls = _serve(beam=True, merge=True)
    try:
        _expect_400(httpd.server_address[1], {"prompt": "hi", "num_beams": 2}, "--merge")
        assert _post(httpd.server_address[1], {"prompt": "hi"})[0] == 200
    finally:
        httpd.shutdown()
        engine.close()
    httpd, engine, calls = _serve(beam=True, sharded_fn=lambda p, i: True)                  # a process group: the batch-sharded path
    try:
        _expect_400(httpd.server_address[1], {"prompt": "hi", "num_beams": 2}, "batch-sharded")
    finally:
        httpd.shutdown()
        engine.close()
    httpd, engine, calls = _serve()                                                         # a generate_fn that knows no beams
    try:
        _expect_400(httpd.server_address[1], {"prompt": "hi", "num_beams": 2}, "one-request path")
    finally:
        httpd.shutdown()
        engine.close()

    class Continuous:                                                                      # what ContinuousBackend offers the handler
        def submit(self, prompts, max_tokens, images=None, **kw):
            return [p + "!" for p in prompts]
    httpd = ThreadingHTTPServer(("127.0.0.1", 0), make_handler(Continuous()))
    threading.Thread(target=httpd.serve_forever, daemon=True).start()
    try:
        _expect_400(httpd.server_address[1], {"prompt": "hi", "num_beams": 2}, "--continuous")
        assert _post(httpd.server_address[1], {"prompt": "hi", "num_beams": 1})[1]["responses"] == ["hi!"]
    finally:
        httpd.shutdown()
