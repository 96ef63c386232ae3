"""Token log-probabilities without a GPU: the NumPy restatement of the rule in include/p3v.h (p3v_logprob_t), which the GPU
tests hold the kernel to; the record layout against the header; argument checks of generate / score / submit before any model
call; the HTTP handler's "logprobs" field on a fake backend; the continuous engine's choice of replay and its want-table on a
stub that records its calls; the fleet's pass-through over gloo."""
import ctypes
import json
import math
import os
import re
import socket
import threading
import time
import urllib.error
import urllib.request

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EOS = 32007


# ---------------------------------------------------------------------------------------------------- the restatement
def bf16_values(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def to_bits(x):
    """float array -> bf16 bit patterns (round to nearest even)."""
    return torch.as_tensor(np.asarray(x, dtype=np.float32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def _row_logprobs(bits):
    """steps 2 - 6 for a defined row: the fp32 logprob of every token"""
    x = bf16_values(bits)
    m = np.float32(x.max())                                               # 2.
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        d = x.astype(np.float64) - np.float64(m)
        w = np.floor(np.exp(d) * 4294967296.0)                            # 3. (a -inf logit: exp(-inf) = 0)
    W = int(w.astype(np.uint64).sum())                                    # 4. an exact integer
    assert 1 << 32 <= W < 1 << 48
    lse = np.float64(m) + np.log(np.float64(W)) - 32.0 * np.log(2.0)      # 5.
    with np.errstate(invalid="ignore"):
        return (x.astype(np.float64) - lse).astype(np.float32)            # 6.


def logprobs_ref(bits, token, N):
    """The record of one row under the rule (include/p3v.h): dict(token, logprob, rank, top=[(id, logprob)] * n_top)."""
    x = bf16_values(bits)
    n, t = len(x), int(token)
    rec = dict(token=t, logprob=float("nan"), rank=0, top=[])
    if np.isnan(x).any() or np.isposinf(x).any() or not np.isfinite(x).any():
        return rec                                                        # 1. undefined
    lp = _row_logprobs(bits)                                              # 2. - 6.
    order = np.lexsort((np.arange(n), -x))                                # 8. larger value first, then the lower index
    rec["top"] = [(int(i), float(lp[i])) for i in order[:min(int(N), n)]]
    if 0 <= t < n:                                                        # 7. / 9.
        rec["rank"] = 1 + int((x > x[t]).sum()) + int((x[:t] == x[t]).sum())
        rec["logprob"] = float(lp[t])
    return rec


def f32_ulps_apart(a, b):
    """0 for equal values (two NaNs, equal infinities included), else the distance in fp32 steps (a large number across
    NaN / non-NaN)."""
    a, b = np.float32(a), np.float32(b)
    if np.isnan(a) or np.isnan(b):
        return 0 if np.isnan(a) and np.isnan(b) else 1 << 31

    def key(v):
        i = int(np.array(v, dtype=np.float32).view(np.int32))
        return i if i >= 0 else -(i & 0x7FFFFFFF)
    return abs(key(a) - key(b))


def assert_record(got, want, what=""):
    """Ids, ranks and n_top exact; every float within 1 fp32 ulp (device log and NumPy log may differ by one fp64 ulp)."""
    assert got["token"] == want["token"] and got["rank"] == want["rank"], (what, got, want)
    assert f32_ulps_apart(got["logprob"], want["logprob"]) <= 1, (what, got["logprob"], want["logprob"])
    assert [i for i, _ in got["top"]] == [i for i, _ in want["top"]], (what, got["top"], want["top"])
    for (_, a), (_, b) in zip(got["top"], want["top"]):
        assert f32_ulps_apart(a, b) <= 1, (what, got["top"], want["top"])


def pack_records(recs):
    """dicts as logprobs_ref makes them -> int32 [n, 20] in the p3v_logprob_t layout (stubs and fake backends)."""
    from phi_3_vision_mlx_amd import _lib
    arr = (_lib.LogprobRecord * len(recs))()
    for k, r in enumerate(recs):
        ids = [i for i, _ in r["top"]] + [-1] * (8 - len(r["top"]))
        lps = [v for _, v in r["top"]] + [float("nan")] * (8 - len(r["top"]))
        arr[k] = _lib.LogprobRecord(r["token"], r["logprob"], r["rank"], len(r["top"]), (ctypes.c_int32 * 8)(*ids), (ctypes.c_float * 8)(*lps))
    return torch.frombuffer(bytearray(arr), dtype=torch.int32).view(len(recs), 20).clone()


# ---------------------------------------------------------------------------------------------------- rule tests
def test_probabilities_sum_to_one():
    """exp(logprob) over a row sums to 1 within 1e-6 -- where the rule can promise it.  Step 3 floors every weight, so W falls
    short of the exact sum 2^32 * S (S = sum exp(l_i - m) >= 1) by less than one unit per non-zero weight: the probabilities
    sum to 1 + e with 0 <= e < n / (2^32 * S), plus the fp32 rounding of each logprob (relative 2^-24 * |logprob| per term,
    signs mixed).  n <= 4096 gives e < 9.6e-7 for ANY row; at the vocabulary's n = 32064 the promise needs S >= 7.5, which a
    row of sigma 1 has a hundred times over (S ~ n * e^0.5 / e^4) and a row whose top token holds most of the mass has not.
    Those rows are held to the bound the rule does give, n / (2^32 * S)."""
    rng = np.random.default_rng(0)
    for sigma, n in ((1.0, 32064), (1.0, 4096), (4.0, 4096), (2.0, 1025), (3.0, 5)):
        bits = to_bits(rng.normal(0, sigma, n))
        lp = _row_logprobs(bits)                                              # every token's fp32 logprob
        assert abs(np.exp(lp.astype(np.float64)).sum() - 1.0) < 1e-6, (sigma, n)
        # ... and a record carries its own token's, whichever token is asked about
        for t in (0, n // 2, n - 1):
            rec = logprobs_ref(bits, t, 8)
            assert rec["logprob"] == float(lp[t]) and all(v == float(lp[i]) for i, v in rec["top"])
    for sigma, n in ((4.0, 32064), (8.0, 32064)):                             # peaked rows of the full vocabulary
        bits = to_bits(rng.normal(0, sigma, n))
        x = bf16_values(bits).astype(np.float64)
        S = np.exp(x - x.max()).sum()
        e = np.exp(_row_logprobs(bits).astype(np.float64)).sum() - 1.0
        assert -2e-7 < e < n / (4294967296.0 * S) + 2e-7, (sigma, e, S)


def test_ties_go_to_the_lower_index_and_argmax_has_rank_one():
    bits = to_bits(np.r_[np.full(100, -3.0), [2.0, 5.0, 2.0, 5.0, 5.0, -0.0, 0.0]])
    rec = logprobs_ref(bits, 101, 8)
    assert rec["rank"] == 1 and int(np.argmax(bf16_values(bits))) == 101
    assert [i for i, _ in rec["top"]] == [101, 103, 104, 100, 102, 105, 106, 0]     # (-0 == +0: the lower index first)
    assert logprobs_ref(bits, 103, 0)["rank"] == 2 and logprobs_ref(bits, 104, 0)["rank"] == 3
    assert logprobs_ref(bits, 102, 0)["rank"] == 5 and logprobs_ref(bits, 106, 0)["rank"] == 7
    assert logprobs_ref(bits, 99, 0)["rank"] == 107
    lps = [v for _, v in rec["top"]]
    assert lps[0] == lps[1] == lps[2] and lps[3] == lps[4] and lps[5] == lps[6]


def test_minus_inf_entries():
    rng = np.random.default_rng(1)
    bits = to_bits(rng.normal(0, 2, 4096))
    clean = logprobs_ref(bits, 7, 3)
    masked = bits.copy()
    masked[1::2] = 0xFF80
    rec = logprobs_ref(masked, 7, 3)
    assert rec["logprob"] == -math.inf and rec["rank"] >= 2049               # a -inf token: -inf, behind every finite one
    assert all(i % 2 == 0 for i, _ in rec["top"])
    keep = logprobs_ref(masked, 6, 3)
    assert keep["logprob"] > logprobs_ref(bits, 6, 3)["logprob"]             # half of the mass is gone: the rest weighs more
    assert math.isfinite(clean["logprob"])
    # more top entries than finite logits: the list runs on into the -inf tokens, lower index first
    few = to_bits(np.r_[[-np.inf] * 6, [1.0, 2.0]])
    rec = logprobs_ref(few, 7, 5)
    assert [i for i, _ in rec["top"]] == [7, 6, 0, 1, 2] and [v for _, v in rec["top"]][2:] == [-math.inf] * 3


def test_undefined_rows():
    base = to_bits(np.linspace(-2, 2, 64))
    for poison in (0x7FC0, 0xFFC1, 0x7F80):                                   # NaN, a negative NaN, +inf
        row = base.copy()
        row[13] = poison
        rec = logprobs_ref(row, 3, 8)
        assert math.isnan(rec["logprob"]) and rec["rank"] == 0 and rec["top"] == [] and rec["token"] == 3
    rec = logprobs_ref(to_bits(np.full(64, -np.inf)), 0, 4)                   # no finite logit
    assert math.isnan(rec["logprob"]) and rec["rank"] == 0 and rec["top"] == []


def test_token_out_of_range_and_more_top_than_tokens():
    bits = to_bits([0.5, 3.0, -1.0, 3.0, 0.0])
    for t in (-1, 5, -32044, 1 << 20):
        rec = logprobs_ref(bits, t, 2)
        assert math.isnan(rec["logprob"]) and rec["rank"] == 0 and rec["token"] == t
        assert [i for i, _ in rec["top"]] == [1, 3]                           # the top list is still filled
    rec = logprobs_ref(bits, 4, 8)                                            # N > n: n_top = n
    assert [i for i, _ in rec["top"]] == [1, 3, 0, 4, 2] and rec["rank"] == 4
    assert logprobs_ref(bits, 2, 0)["top"] == []


# ---------------------------------------------------------------------------------------------------- layout and arguments
def test_logprob_record_layout_matches_header_field_order():
    from phi_3_vision_mlx_amd import _lib
    h = open(os.path.join(ROOT, "include", "p3v.h")).read()
    end = h.index("} p3v_logprob_t")
    body = h[h.rindex("typedef struct {", 0, end) + len("typedef struct {"):end]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if stmt:
            decl = re.sub(r"^(int32_t|float)\s+", "", stmt)
            names.append(re.sub(r"\[.*\]", "", decl).strip())
    assert names == [f for f, _ in _lib.LogprobRecord._fields_]
    assert ctypes.sizeof(_lib.LogprobRecord) == 80 and _lib.LOGPROB_WORDS == 20 and _lib.LOGPROBS_MAX == 8
    assert "#define P3V_LOGPROBS_MAX 8" in h
    assert {"p3v_logprobs", "p3v_logprobs_step"} <= set(_lib.SIGNATURES)
    for name in ("p3v_logprobs", "p3v_logprobs_step"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", h)
    # pack -> unpack round trip through the host module
    from phi_3_vision_mlx_amd import logprobs
    rec = dict(token=5, logprob=-0.25, rank=2, top=[(9, -0.125), (5, -0.25), (1, -math.inf)])
    assert logprobs.unpack(pack_records([rec, dict(token=-1, logprob=float("nan"), rank=0, top=[])]))[0] == rec


BAD_VALUES = (True, False, 1.0, "3", -1, 9, [1, 2, 3], [1, "a"], [True])


def test_generate_score_submit_reject_bad_values_before_any_model_call():
    from phi_3_vision_mlx_amd import api, logprobs
    from phi_3_vision_mlx_amd.engine import ContinuousEngine, logprob_args

    class NoModel:
        def __call__(self, *a, **kw):
            raise AssertionError("the model must not run")

        def __getattr__(self, name):
            raise AssertionError(f"the model must not be touched ({name})")

    class Proc:
        def __call__(self, *a, **kw):
            raise AssertionError("the processor must not run")

    assert logprobs.wants(None, 3) is None and logprobs.wants([None, None], 2) is None
    assert logprobs.wants(0, 2) == [0, 0] and logprobs.wants([8, None, 3], 3) == [8, -1, 3]
    for bad in BAD_VALUES:
        with pytest.raises(ValueError, match=r"0\.\.8|values for"):
            api._generate(NoModel(), Proc(), ["a", "b"] if isinstance(bad, list) and len(bad) == 2 else "hi", max_tokens=4,
                          verbose=False, stream=False, mute=True, logprobs=bad)
        with pytest.raises(ValueError, match=r"0\.\.8|values for"):
            api.generate("hi", preload=(NoModel(), Proc()), max_tokens=4, verbose=False, logprobs=bad)
    for bad in (True, 1.0, "3", -1, 9, None, [1]):
        with pytest.raises(ValueError, match=r"0\.\.8"):
            api.score("hi", preload=(NoModel(), Proc()), top=bad)
    # speculation + logprobs: refused by name, before the speculative checks touch the model
    with pytest.raises(ValueError, match="speculate: logprobs are not supported"):
        api._generate(NoModel(), Proc(), "hi", max_tokens=4, verbose=False, stream=False, mute=True, logprobs=2, speculate=4)
    with pytest.raises(ValueError, match="speculate: logprobs are not supported"):
        api.generate("hi", preload=(NoModel(), Proc()), max_tokens=4, verbose=False, logprobs=0, speculate=2)
    # the engine: the handle fails at submit, nothing is queued
    stub = LogprobStub()
    eng = ContinuousEngine(stub, None, slots=2, window=256)
    for bad in (True, 1.0, "3", -1, 9, [1]):
        h = eng.submit(logprob_args(_req(12, 4), bad), 3)
        assert h.done.is_set() and isinstance(h.error, ValueError) and "0..8" in str(h.error)
    assert not eng.waiting and stub.calls == []


def test_package_level_generate_keeps_the_reference_signature():
    import inspect

    import phi_3_vision_mlx_amd as pkg
    assert "logprobs" not in inspect.signature(pkg.generate).parameters
    assert {"logprobs", "logprob_info"} <= set(inspect.signature(pkg.api.generate).parameters)


# ---------------------------------------------------------------------------------------------------- HTTP handler
def _post(port, payload):
    req = urllib.request.Request(f"http://127.0.0.1:{port}/v1/completions", data=json.dumps(payload).encode(),
                                 headers={"Content-Type": "application/json"})
    with urllib.request.urlopen(req, timeout=10) as r:
        return r.status, json.loads(r.read())


def _fake_entry(prompt, n_top):
    """three tokens, then EOS, then one more (a batched row runs on until every row is done): ids derived from the prompt"""
    k = sum(prompt.encode()) % 1000
    ids = [k, k + 1, k + 2, EOS, k + 4]
    lps = [-0.5, -math.inf, float("nan"), -0.25, -1.0]
    return dict(token_ids=ids, token_logprobs=lps, ranks=[1, 7, 0, 1, 2],
                top_logprobs=[[(i + j, -0.5 - j if j else -math.inf) for j in range(n_top)] for i in ids])


@pytest.fixture(params=[True, False], ids=["merge", "solo"])
def queue_server(request):
    from phi_3_vision_mlx_amd.server import serve
    calls = []

    def fake_generate(prompts, max_tokens, images=None, sampling=None, logprobs=None, logprob_info=None):
        calls.append((list(prompts), max_tokens, sampling, None if logprobs is None else list(logprobs)))
        time.sleep(0.05)
        if logprobs is not None:
            assert len(logprobs) == len(prompts) and logprob_info == {}
            rows = [None if w is None else _fake_entry(p, w) for p, w in zip(prompts, logprobs)]
            for key in ("token_ids", "token_logprobs", "ranks", "top_logprobs"):
                logprob_info[key] = [None if r is None else r[key] for r in rows]
        return [f"{p}|{max_tokens}" for p in prompts]

    httpd, engine = serve(fake_generate, port=0, merge=request.param, sharded_fn=lambda prompts, images: images is not None,
                          decode_fn=lambda i: f"<{i}>")
    threading.Thread(target=httpd.serve_forever, daemon=True).start()
    yield httpd.server_address[1], calls
    httpd.shutdown()
    engine.close()


def test_http_logprobs_field(queue_server):
    port, calls = queue_server
    # absent or null: today's call, no "logprobs" in the response
    for body in ({"prompt": "a", "max_tokens": 3}, {"prompt": "a", "max_tokens": 3, "logprobs": None}):
        code, out = _post(port, body)
        assert code == 200 and out == {"model": "phi-3-vision", "responses": ["a|3"]}
        assert calls[-1] == (["a"], 3, None, None)
    # N = 2 on two prompts: one object per prompt, lists aligned and cut behind the EOS, null for non-finite values
    code, out = _post(port, {"prompt": ["x", "yy"], "max_tokens": 5, "logprobs": 2})
    assert code == 200 and out["responses"] == ["x|5", "yy|5"] and calls[-1][3] == [2, 2]
    assert set(out) == {"model", "responses", "logprobs"} and len(out["logprobs"]) == 2
    for p, obj in zip(("x", "yy"), out["logprobs"]):
        e = _fake_entry(p, 2)
        assert set(obj) == {"token_ids", "tokens", "token_logprobs", "ranks", "top_logprobs"}
        assert obj["token_ids"] == e["token_ids"][:4] and obj["token_ids"][-1] == EOS
        assert obj["tokens"] == [f"<{i}>" for i in obj["token_ids"]]
        assert obj["token_logprobs"] == [-0.5, None, None, -0.25] and obj["ranks"] == [1, 7, 0, 1]
        assert len(obj["top_logprobs"]) == 4 and all(len(t) == 2 for t in obj["top_logprobs"])
        first = obj["top_logprobs"][0]
        assert first[0] == {"id": e["token_ids"][0], "token": f"<{e['token_ids'][0]}>", "logprob": None}
        assert first[1] == {"id": e["token_ids"][0] + 1, "token": f"<{e['token_ids'][0] + 1}>", "logprob": -1.5}
    # N = 0: records without a top list
    code, out = _post(port, {"prompt": "z", "logprobs": 0})
    assert calls[-1][3] == [0] and all(t == [] for t in out["logprobs"][0]["top_logprobs"])
    # sampled + logprobs travel together
    code, out = _post(port, {"prompt": "z", "logprobs": 1, "temperature": 0.7, "seed": 3})
    assert out["seeds"] == [3] and calls[-1][2][0]["seed"] == 3 and calls[-1][3] == [1]
    # bad types / ranges: 400 naming the range, nothing reaches the backend
    n = len(calls)
    for bad in (True, False, "2", 2.5, -1, 9, [1], {"n": 1}):
        with pytest.raises(urllib.error.HTTPError) as e:
            _post(port, {"prompt": "q", "logprobs": bad})
        assert e.value.code == 400 and "0" in (msg := e.value.read().decode()) and "8" in msg, bad
    # speculation next to logprobs, and the batch-sharded path: 400 naming the limit
    with pytest.raises(urllib.error.HTTPError) as e:
        _post(port, {"prompt": "q", "logprobs": 1, "speculate": 4})
    assert e.value.code == 400 and "speculative" in e.value.read().decode()
    from test_server import _png_data_uri
    with pytest.raises(urllib.error.HTTPError) as e:
        _post(port, {"prompt": "q", "images": [_png_data_uri()], "logprobs": 1})
    assert e.value.code == 400 and "batch-sharded" in e.value.read().decode()
    assert len(calls) == n


def test_http_merged_requests_keep_their_own_n(queue_server):
    port, calls = queue_server
    results = {}

    def worker(i):
        body = {"prompt": [f"p{i}a", f"p{i}b"], "max_tokens": 6}
        if i % 3:
            body["logprobs"] = i
        results[i] = _post(port, body)[1]

    _post(port, {"prompt": "warm"})
    ths = [threading.Thread(target=worker, args=(i,)) for i in range(6)]
    [t.start() for t in ths]
    [t.join() for t in ths]
    for i in range(6):
        assert results[i]["responses"] == [f"p{i}a|6", f"p{i}b|6"]
        assert ("logprobs" in results[i]) == bool(i % 3)
        if i % 3:
            for p, obj in zip((f"p{i}a", f"p{i}b"), results[i]["logprobs"]):
                assert obj["token_ids"] == _fake_entry(p, i)["token_ids"][:4]
                assert all(len(t) == i for t in obj["top_logprobs"])
    for prompts, mt, sampling, wants in calls:
        if wants is None:
            assert all(int(p[1:-1]) % 3 == 0 for p in prompts if p != "warm")
            continue
        assert wants == [(int(p[1:-1]) if int(p[1:-1]) % 3 else None) for p in prompts]   # every row its own request's N


def test_http_continuous_backend_passes_logprobs_through():
    from http.server import ThreadingHTTPServer

    from phi_3_vision_mlx_amd.server import ContinuousBackend, make_handler
    seen = []

    class Tok:
        def decode(self, ids):
            return "".join(f"[{i}]" for i in ids)

    class Eng:
        processor = type("P", (), {"tokenizer": Tok()})()

        def serve_forever(self, stop, idle_sleep=0.002):
            stop.wait()

        def generate(self, prompts, images=None, max_tokens=512, timeout=600.0, sampling=None, info=None, logprobs=None):
            seen.append((sampling, logprobs, info is not None))
            if logprobs is not None:
                info["logprobs"] = [{k: v[:3] for k, v in _fake_entry(p, w).items()} for p, w in zip(prompts, logprobs)]
            return list(prompts)

    backend = ContinuousBackend(Eng())
    httpd = ThreadingHTTPServer(("127.0.0.1", 0), make_handler(backend))
    threading.Thread(target=httpd.serve_forever, daemon=True).start()
    port = httpd.server_address[1]
    try:
        code, out = _post(port, {"prompt": "a"})
        assert seen[-1] == (None, None, False) and set(out) == {"model", "responses"}
        code, out = _post(port, {"prompt": "a", "logprobs": 3})
        assert code == 200 and seen[-1] == (None, [3], True) and set(out) == {"model", "responses", "logprobs"}
        obj = out["logprobs"][0]
        assert obj["token_ids"] == _fake_entry("a", 3)["token_ids"][:3] and obj["tokens"] == [f"[{i}]" for i in obj["token_ids"]]
        assert all(len(t) == 3 for t in obj["top_logprobs"])
        with pytest.raises(urllib.error.HTTPError) as e:
            _post(port, {"prompt": "a", "logprobs": 99})
        assert e.value.code == 400
    finally:
        httpd.shutdown()
        backend.close()


# ---------------------------------------------------------------------------------------------------- engine host logic
class LogprobStub:
    """test_sampling_cpu.SamplingStub plus the log-probability methods, every model call recorded.  A record's rank field
    carries the stub's step counter of its row, its n_top the row's want: enough to see which record went where."""
    device = "cpu"
    RECORD_SLOTS = 4                                            # few on purpose: the engine must restart the step counter

    def __init__(self):
        from test_sampling_cpu import SamplingStub
        self.inner = SamplingStub()
        self.calls = self.inner.calls
        for name in ("new_slot_state", "prefill_slot", "set_sampling", "sample_logits"):
            setattr(self, name, getattr(self.inner, name))

    def decode_graph(self, st):
        g = self.inner.decode_graph(st)
        g.setdefault("n_replays", 0)
        g.setdefault("history", torch.zeros((len(st.pad_len), self.RECORD_SLOTS), dtype=torch.int32))
        return g

    def _plain(self, name, token, cache):
        """as the model's `_replay`: EVERY replay advances the capture's step counter, and one past the slots writes nothing"""
        out = getattr(self.inner, name)(token, cache)
        self.decode_graph(cache[0].state)["n_replays"] += 1
        return out

    def greedy_step(self, token, cache):
        return self._plain("greedy_step", token, cache)

    def sample_step(self, token, cache):
        return self._plain("sample_step", token, cache)

    def set_logprobs(self, st, wants, row0=0):
        self.calls.append(("set_logprobs", row0, list(wants)))
        if getattr(st, "logprob_want", None) is None:
            st.logprob_want = [-1] * len(st.pad_len)
        st.logprob_want[row0:row0 + len(wants)] = list(wants)

    def _records(self, st, tokens, rows):
        return pack_records([dict(token=int(t), logprob=-1.0 - b, rank=1 + int(st.step[b]),
                                  top=[(int(t) + j, -1.0 - j) for j in range(max(st.logprob_want[b], 0))])
                             for t, b in zip(tokens, rows)])

    def logprobs_of(self, st, logits, tokens, row0=0):
        self.calls.append(("logprobs_of", row0, tokens.reshape(-1).tolist()))
        return self._records(st, tokens.reshape(-1).tolist(), range(row0, row0 + tokens.numel()))

    def _scored(self, name, token, cache):
        st = cache[0].state
        self.calls.append((name,))
        out = self.inner.base.greedy_step(token, cache)
        g = self.decode_graph(st)
        g.setdefault("records", torch.full((len(st.pad_len), g["history"].shape[1], 20), -7, dtype=torch.int32))   # made on first use
        g["n_replays"] += 1
        assert g["n_replays"] <= self.RECORD_SLOTS, "the engine replayed past the record slots"
        g["records"][:, g["n_replays"] - 1] = self._records(st, out[1].reshape(-1).tolist(), range(len(st.pad_len)))
        return out

    def logprob_step(self, token, cache):
        return self._scored("logprob_step", token, cache)

    def sample_logprob_step(self, token, cache):
        return self._scored("sample_logprob_step", token, cache)

    def restart_history(self, st):
        self.calls.append(("restart_history",))
        self.decode_graph(st)["n_replays"] = 0


def _req(n, key):
    return {"input_ids": np.full((1, n), key, dtype=np.int64)}


def test_engine_traffic_without_logprobs_never_calls_the_new_methods():
    from phi_3_vision_mlx_amd.engine import ContinuousEngine
    stub = LogprobStub()
    eng = ContinuousEngine(stub, None, slots=3, window=256)
    hs = [eng.submit(_req(10 + i, 3 + i), 6, **({"sampling": {"temperature": 0.5, "seed": 1}} if i == 2 else {})) for i in range(4)]
    eng.run_until_idle()
    assert all(h.error is None and h.logprob_records == [] for h in hs)
    names = {c[0] for c in stub.calls}
    assert names == {"prefill_slot", "greedy_step", "set_sampling", "sample_logits", "sample_step"}
    greedy_only = LogprobStub()
    eng = ContinuousEngine(greedy_only, None, slots=3, window=256)
    hs = [eng.submit(_req(10 + i, 3 + i), 6) for i in range(4)]
    eng.run_until_idle()
    assert {c[0] for c in greedy_only.calls} == {"prefill_slot", "greedy_step"}
    assert all(c[2] == () for c in greedy_only.calls if c[0] == "prefill_slot")     # prefill_slot(st, row, inputs): as today


@pytest.mark.parametrize("plain_steps", [LogprobStub.RECORD_SLOTS - 1, LogprobStub.RECORD_SLOTS, LogprobStub.RECORD_SLOTS + 3])
def test_engine_first_scored_request_after_long_plain_traffic(plain_steps):
    """plain replays advance the step counter that indexes the records, and the record buffer does not exist before the first
    scored replay: an engine that has served more plain steps than there are slots must still restart the counter"""
    from phi_3_vision_mlx_amd.engine import ContinuousEngine, logprob_args
    stub = LogprobStub()
    eng = ContinuousEngine(stub, None, slots=2, window=256)
    g = eng.submit(_req(12, 29), plain_steps + 6)
    for _ in range(plain_steps):
        eng.step()
    assert stub.decode_graph(eng.st)["n_replays"] == plain_steps and "records" not in stub.decode_graph(eng.st)
    assert ("restart_history",) not in stub.calls
    s = eng.submit(logprob_args(_req(12, 5), 2), 4)
    eng.safe_step()                                                           # (a failed step would fail BOTH requests here)
    assert eng.failures == 0 and g.error is None and s.error is None
    assert (("restart_history",) in stub.calls) == (plain_steps >= LogprobStub.RECORD_SLOTS)
    eng.run_until_idle()
    assert eng.failures == 0 and g.error is None and s.error is None and g.logprob_records == []
    assert len(g.tokens) == plain_steps + 6 and [r["token"] for r in s.logprob_records] == s.tokens and len(s.tokens) == 4
    assert [r["rank"] for r in s.logprob_records] == [1, 2, 3, 4]


def test_engine_mixed_traffic_switches_captures_and_clears_the_want_table():
    from phi_3_vision_mlx_amd.engine import ContinuousEngine, logprob_args
    stub = LogprobStub()
    eng = ContinuousEngine(stub, None, slots=2, window=256)
    g = eng.submit(_req(12, 29), 12)                                          # (keys whose stub tokens meet no EOS this early)
    eng.step()
    eng.step()
    assert [c[0] for c in stub.calls] == ["prefill_slot", "greedy_step", "greedy_step"]
    s = eng.submit(logprob_args(_req(12, 5), 3), 9)
    eng.step()
    i = next(k for k, c in enumerate(stub.calls) if c[0] == "prefill_slot" and k > 0)
    # the same prefill with its logits kept, the row's want, the first record from the prefill logits, then the scored replay
    assert [c[0] for c in stub.calls[i:i + 4]] == ["prefill_slot", "set_logprobs", "logprobs_of", "logprob_step"]
    assert stub.calls[i][2] == ("return_logits",) and stub.calls[i + 1][1:] == (1, [3]) and stub.calls[i + 2][1] == 1
    assert eng.st.logprob_want == [-1, 3]
    eng.run_until_idle()
    assert g.error is None and s.error is None and g.logprob_records == []
    assert len(s.logprob_records) == len(s.tokens) == 9
    assert [r["token"] for r in s.logprob_records] == s.tokens                # every record is its own token's ...
    assert [r["rank"] for r in s.logprob_records] == list(range(1, 10))       # ... of its own step, in order,
    assert all(len(r["top"]) == 3 for r in s.logprob_records)                 # with its own N
    assert ("restart_history",) in stub.calls                                 # 8 scored replays on 4 record slots
    # released: the row's want is back at -1, and once the scored request has left the greedy capture replays again
    assert eng.st.logprob_want == [-1, -1]
    k = max(j for j, c in enumerate(stub.calls) if c[0] == "logprob_step")
    assert stub.calls[k + 1] == ("set_logprobs", 1, [-1])
    assert [c[0] for c in stub.calls[k + 2:]] == ["greedy_step"] * (len(stub.calls) - k - 2) and len(stub.calls) > k + 2
    # sampled + scored in one batch: the sampled capture with the extra launch; an unscored neighbour gets no records
    stub.calls.clear()
    a = eng.submit(logprob_args(_req(12, 4), 0), 3, sampling={"temperature": 0.7, "seed": 5})
    b = eng.submit(_req(12, 5), 3)
    eng.run_until_idle()
    assert a.error is None and b.error is None and b.logprob_records == []
    assert len(a.logprob_records) == 3 and all(r["top"] == [] for r in a.logprob_records)
    steps = [c[0] for c in stub.calls if c[0].endswith("_step")]
    assert steps == ["sample_logprob_step"] * 2
    sets = [c for c in stub.calls if c[0] == "set_logprobs"]
    assert sets[0][2] in ([0, -1], [0]) and sets[-1][2] == [-1] and eng.st.logprob_want == [-1, -1]
    # the router passes the field on
    from phi_3_vision_mlx_amd.engine import RegimeRouter
    router = RegimeRouter([eng])
    eng.processor = None
    r = router.submit(logprob_args(_req(12, 6), 8), 2)
    eng.run_until_idle()
    assert r.error is None and [len(x["top"]) for x in r.logprob_records] == [8, 8]


def test_generate_text_reports_entries_cut_at_the_eos():
    from phi_3_vision_mlx_amd.engine import Request, _generate_text, requested_logprobs

    class Tok:
        def decode(self, ids):
            return " ".join(map(str, ids))

    class Eng:
        def submit(self, inputs, max_tokens):
            logprobs = requested_logprobs(inputs)
            r = Request(inputs, max_tokens, logprobs=logprobs)
            r.tokens = [11, EOS] if logprobs is not None else [12, 13]
            r.logprob_records = [dict(token=t, logprob=-0.5, rank=1, top=[(t, -0.5)] * (logprobs or 0)) for t in r.tokens] \
                if logprobs is not None else []
            r.done.set()
            return r

    proc = type("P", (), {"tokenizer": Tok(), "__call__": lambda self, text, imgs=None: _req(4, 1)})()
    info = {}
    out = _generate_text(Eng(), proc, ["a", "b"], None, 4, 5.0, info=info, logprobs=[2, None])
    assert out == [f"11 {EOS}", "12 13"]
    assert info["logprobs"][1] is None and info["logprobs"][0]["token_ids"] == [11, EOS]
    assert info["logprobs"][0]["top_logprobs"] == [[(11, -0.5)] * 2, [(EOS, -0.5)] * 2]
    info = {}
    _generate_text(Eng(), proc, ["a"], None, 4, 5.0, info=info)
    assert "logprobs" not in info
    with pytest.raises(ValueError, match=r"0\.\.8"):
        _generate_text(Eng(), proc, ["a"], None, 4, 5.0, logprobs=True)


# ---------------------------------------------------------------------------------------------------- fleet pass-through
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _fleet_worker(rank, world, port, out_dir):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "tests")]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from test_logprobs_cpu import LogprobStub, _req
    from phi_3_vision_mlx_amd import fleet
    from phi_3_vision_mlx_amd.engine import ContinuousEngine, Request, logprob_args
    eng = ContinuousEngine(LogprobStub(), None, slots=2, window=4096)
    groups = fleet.make_groups()
    if rank:
        fleet.worker(eng, groups)
        open(os.path.join(out_dir, f"worker{rank}"), "w").write("ok")
        dist.destroy_process_group()
        return
    front = fleet.EngineFleet(eng, groups, world)
    stop = threading.Event()
    stepper = threading.Thread(target=front.serve_forever, args=(stop,), daemon=True)
    stepper.start()
    busy = [Request(_req(5, 0), 1) for _ in range(5)]
    # a local request and a remote one, with and without the field
    for steer_remote in (False, True):
        front.local = list(busy) if steer_remote else []
        hs = [front.submit(logprob_args(_req(20, 3), 4), 5), front.submit(_req(21, 4), 5), front.submit(logprob_args(_req(22, 5), 0), 5)]
        assert all(h.done.wait(60) for h in hs) and all(h.error is None for h in hs), [h.error for h in hs]
        if steer_remote:
            assert all(getattr(h, "rank", 0) == 1 for h in hs)
        ref_eng = ContinuousEngine(LogprobStub(), None, slots=2, window=4096)
        for h, (n, key, want) in zip(hs, ((20, 3, 4), (21, 4, None), (22, 5, 0))):
            r = ref_eng.submit(logprob_args(_req(n, key), want), 5)
            ref_eng.run_until_idle()
            assert r.tokens == h.tokens and len(h.tokens) >= 1
            assert [x["token"] for x in h.logprob_records] == (h.tokens if want is not None else [])
            assert all(len(x["top"]) == want for x in h.logprob_records)
            assert [(x["token"], x["rank"], x["top"]) for x in h.logprob_records] == \
                [(x["token"], x["rank"], x["top"]) for x in r.logprob_records]
    bad = front.submit(logprob_args(_req(20, 3), 9), 5)                            # a bad N never leaves rank 0
    assert bad.done.is_set() and isinstance(bad.error, ValueError) and not hasattr(bad, "rank")
    front.local = []
    front.close()
    stop.set()
    stepper.join(5)
    open(os.path.join(out_dir, "front"), "w").write("ok")
    dist.destroy_process_group()


def test_fleet_carries_the_field_out_and_the_records_back(tmp_path):
    import torch.multiprocessing as mp
    world, port = 2, _free_port()
    mp.spawn(_fleet_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    assert os.path.exists(tmp_path / "front") and os.path.exists(tmp_path / "worker1")
