"""Seeded sampling without a GPU: the NumPy / Python restatement of the rule in include/p3v.h (p3v_sample_row_t), which the GPU
tests hold the kernels to; the HTTP handler's sampling fields on fake backends; the continuous engine's choice of replay on a
stub that records its calls; the record layout against the header."""
import json
import math
import os
import re
import threading
import time
import urllib.error
import urllib.request

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK32 = 0xFFFFFFFF


# ---------------------------------------------------------------------------------------------------- the restatement
def philox4x32_10(ctr, key):
    """Philox4x32-10 (Random123): four 32-bit output words."""
    c, (k0, k1) = list(ctr), key
    for r in range(10):
        if r:
            k0, k1 = (k0 + 0x9E3779B9) & MASK32, (k1 + 0xBB67AE85) & MASK32
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & MASK32, (p0 >> 32) ^ c[3] ^ k1, p0 & MASK32]
    return c


def draw_word(seed, c):
    return philox4x32_10([c & MASK32, 0, 0, 0], [seed & MASK32, seed >> 32])[0]


def bf16_values(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def argmax_ref(x):
    """p3v_argmax: first maximum, -1 for a row holding a NaN."""
    return -1 if np.isnan(x).any() else int(np.argmax(x))


_MEMO = {}


def sample_probs(bits, temperature, top_k, top_p):
    """The integer weights (uint64) of a row after top-k / top-p, or None for an arg-max row.  (Memoised: the weights do not
    depend on the seed or the draw index.)"""
    bits = np.ascontiguousarray(bits, dtype=np.uint16)
    key = (bits.tobytes(), float(np.float32(temperature)), int(top_k), float(np.float32(top_p)))
    if key not in _MEMO:
        if len(_MEMO) > 256:
            _MEMO.clear()
        _MEMO[key] = _sample_probs(bits, temperature, top_k, top_p)
    return _MEMO[key]


def _sample_probs(bits, temperature, top_k, top_p):
    x = bf16_values(bits)
    T = np.float32(temperature)
    if np.isnan(x).any() or not T > 0:
        return None
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        m = np.float32(x.max()) / T
        if not np.isfinite(m):
            return None
        z = x / T
        d = z.astype(np.float64) - np.float64(m)
        w = np.floor(np.exp(d) * 4294967296.0)
    w = np.where(np.isfinite(w), w, 0).astype(np.uint64)
    n = len(x)
    kept = np.ones(n, dtype=bool)
    if 1 <= top_k < n:
        kth = np.sort(x)[::-1][top_k - 1]
        kept &= x >= kth
    w = np.where(kept, w, np.uint64(0))
    p = float(np.float32(top_p))
    if 0.0 < p < 1.0:
        Q = int(w.sum())
        P = math.ceil(p * float(Q))
        vals, inv = np.unique(x[kept], return_inverse=True)          # ascending distinct values of the kept tokens
        mass = np.zeros(len(vals), dtype=np.uint64)
        np.add.at(mass, inv, w[kept])
        above = np.cumsum(mass[::-1])                                 # mass of the tokens >= each value, largest value first
        kappa = vals[::-1][int(np.argmax(above >= np.uint64(P)))]
        w = np.where(x >= kappa, w, np.uint64(0))
    return w


def sample_ref(bits, temperature, top_k, top_p, seed, c):
    """The token of one row under the rule (include/p3v.h)."""
    w = sample_probs(bits, temperature, top_k, top_p)
    if w is None:
        return argmax_ref(bf16_values(bits))
    ckey = ("cum", id(w))
    if _MEMO.get(ckey, (None,))[0] is not w:
        _MEMO[ckey] = (w, np.cumsum(w))
    cum = _MEMO[ckey][1]
    t = (int(cum[-1]) * draw_word(seed, c)) >> 32
    return int(np.searchsorted(cum, np.uint64(t), side="right"))        # the first index whose inclusive prefix exceeds t


def to_bits(x):
    """float array -> bf16 bit patterns (round to nearest even)."""
    return torch.as_tensor(np.asarray(x, dtype=np.float32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


# ---------------------------------------------------------------------------------------------------- restatement checks
def test_philox_known_answers():
    assert philox4x32_10([0, 0, 0, 0], [0, 0]) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert philox4x32_10([MASK32] * 4, [MASK32, MASK32]) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    assert philox4x32_10([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0]) == \
        [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]


def test_flat_row_draws_floor_n_r():
    n = 32064
    bits = to_bits(np.zeros(n))
    for seed, c, want in ((0, 0, 12795), (1, 0, 28545), (0, 1, 31173), (0x0123456789ABCDEF, 7, 17858)):
        assert (n * draw_word(seed, c)) >> 32 == want
        assert sample_ref(bits, 1.0, 0, 1.0, seed, c) == want


def test_restatement_rules():
    rng = np.random.default_rng(0)
    bits = to_bits(rng.normal(0, 2, 4096))
    x = bf16_values(bits)
    top = int(np.argmax(x))
    for s in range(20):
        assert sample_ref(bits, 0.0, 0, 1.0, s, s) == top                 # T = 0: the arg-max
        assert sample_ref(bits, 0.7, 1, 1.0, s, s) == top                 # k = 1
        assert sample_ref(bits, 1.0, 0, 1e-4, s, s) == top                # tiny p: the top token alone
    # ties at the top-k cut are kept: 3 tokens at the 2nd largest value, k = 2 keeps all four
    tie = to_bits(np.r_[np.full(4092, -30.0), [5.0, 4.0, 4.0, 4.0]])
    w = sample_probs(tie, 1.0, 2, 1.0)
    assert (w[-4:] > 0).all() and (w[:-4] == 0).all()
    # -inf entries are never drawn
    ninf = bits.copy()
    ninf[::3] = 0xFF80
    draws = {sample_ref(ninf, 3.0, 0, 1.0, s, c) for s in range(8) for c in range(32)}
    assert all(d % 3 for d in draws)
    # a NaN row gives -1, sampled or not
    nan = bits.copy()
    nan[77] = 0x7FC0
    assert sample_ref(nan, 1.0, 0, 1.0, 0, 0) == -1 and sample_ref(nan, 0.0, 0, 1.0, 0, 0) == -1
    # no finite logit / an overflowing max z: the arg-max
    assert sample_ref(to_bits(np.full(64, -np.inf)), 1.0, 0, 1.0, 0, 0) == 0
    assert sample_ref(to_bits(np.r_[np.zeros(63), 1e30]), 1e-20, 0, 1.0, 0, 0) == 63


# ---------------------------------------------------------------------------------------------------- host arguments
def test_sampling_rows_validation_and_seeds():
    from phi_3_vision_mlx_amd import sampling
    assert sampling.rows(3, 0.5, 4, 0.9, 7) == [(0.5, 4, 0.9, 7), (0.5, 4, 0.9, 8), (0.5, 4, 0.9, 9)]
    assert [r[3] for r in sampling.rows(2, 1.0, seed=(1 << 64) - 1)] == [(1 << 64) - 1, 0]
    assert [r[3] for r in sampling.rows(2, 1.0, seed=[5, 3])] == [5, 3]
    a, b = sampling.rows(1, 1.0)[0][3], sampling.rows(1, 1.0)[0][3]
    assert a != b                                                         # None: fresh random bits per call
    assert sampling.greedy(sampling.rows(2, 0.0)) and not sampling.greedy(sampling.rows(2, [0.0, 1.0]))
    for bad in (dict(temperature=-1.0), dict(temperature=float("inf")), dict(temperature=float("nan")), dict(top_p=0.0),
                dict(top_p=1.5), dict(top_k=-1), dict(seed=-1), dict(seed=1 << 64), dict(temperature=[1.0]),
                dict(seed=[1, 2, 3]), dict(top_k=1.5), dict(temperature="1")):
        with pytest.raises(ValueError):
            sampling.rows(2, **{"temperature": 1.0, **bad})
    recs = sampling.pack(sampling.rows(2, [0.5, 2.0], [0, 40], [1.0, 0.25], [3, (1 << 64) - 2]), counter=9)
    assert recs.dtype == torch.int32 and tuple(recs.shape) == (2, 6)
    got = sampling.unpack(recs)
    assert got[1] == dict(temperature=2.0, top_k=40, top_p=0.25, seed=(1 << 64) - 2, counter=9)
    assert got[0]["temperature"] == 0.5 and got[0]["seed"] == 3


def test_generate_rejects_bad_sampling_arguments_before_the_model_runs():
    from phi_3_vision_mlx_amd import api

    class NoModel:
        def __call__(self, *a, **kw):
            raise AssertionError("the model must not run")

    class Proc:
        def __call__(self, *a, **kw):
            raise AssertionError("the processor must not run")

    for kw in (dict(temperature=-0.5), dict(top_p=0.0), dict(top_k=-3), dict(seed=1 << 64), dict(temperature=[1.0, 1.0])):
        with pytest.raises(ValueError):
            api._generate(NoModel(), Proc(), "hi", max_tokens=4, verbose=False, stream=False, mute=True, **kw)


def test_sample_record_layout_matches_header_field_order():
    from phi_3_vision_mlx_amd import _lib
    h = open(os.path.join(ROOT, "include", "p3v.h")).read()
    end = h.index("} p3v_sample_row_t")
    body = h[h.rindex("typedef struct {", 0, end) + len("typedef struct {"):end]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if stmt:
            decl = re.sub(r"^(const\s+)?(void|uint16_t|uint8_t|uint32_t|int32_t|int64_t|float|int)\s*\*?\s*", "", stmt)
            names += [n.strip() for n in decl.split(",")]
    assert names == [f for f, _ in _lib.SampleRow._fields_]
    import ctypes
    assert ctypes.sizeof(_lib.SampleRow) == 24
    assert {"p3v_sample", "p3v_sample_step_end"} <= set(_lib.SIGNATURES)


# ---------------------------------------------------------------------------------------------------- HTTP handler
def _post(port, payload):
    req = urllib.request.Request(f"http://127.0.0.1:{port}/v1/completions", data=json.dumps(payload).encode(),
                                 headers={"Content-Type": "application/json"})
    with urllib.request.urlopen(req, timeout=10) as r:
        return r.status, json.loads(r.read())


@pytest.fixture(params=[True, False], ids=["merge", "solo"])
def queue_server(request):
    from phi_3_vision_mlx_amd.server import serve
    calls = []

    def fake_generate(prompts, max_tokens, images=None, sampling=None):
        calls.append((list(prompts), max_tokens, images, sampling))
        time.sleep(0.05)
        return [f"{p}|{max_tokens}|{'s' if sampling else 'g'}" for p in prompts]

    httpd, engine = serve(fake_generate, port=0, merge=request.param, sharded_fn=lambda prompts, images: images is not None)
    threading.Thread(target=httpd.serve_forever, daemon=True).start()
    yield httpd.server_address[1], calls
    httpd.shutdown()
    engine.close()


def test_http_sampling_fields(queue_server):
    port, calls = queue_server
    # no sampling field, or temperature 0: today's call, no "seeds"
    for body in ({"prompt": "a", "max_tokens": 3}, {"prompt": "a", "max_tokens": 3, "temperature": 0, "top_p": 0.5, "seed": 4}):
        code, out = _post(port, body)
        assert code == 200 and out == {"model": "phi-3-vision", "responses": ["a|3|g"]}
        assert calls[-1] == (["a"], 3, None, None)
    # sampled: one record per row, the client's seed + row, echoed back
    code, out = _post(port, {"prompt": ["x", "y"], "max_tokens": 5, "temperature": 0.8, "top_k": 40, "top_p": 0.9, "seed": 11})
    assert code == 200 and out["responses"] == ["x|5|s", "y|5|s"] and out["seeds"] == [11, 12]
    recs = calls[-1][3]
    assert len(recs) == 2 and recs[1] == dict(temperature=0.8, top_k=40, top_p=0.9, seed=12)
    # no seed: the handler draws one before queueing, and it reproduces the request
    code, out = _post(port, {"prompt": "z", "temperature": 1})
    assert len(out["seeds"]) == 1 and calls[-1][3][0]["seed"] == out["seeds"][0]
    # bad types / ranges: 400, nothing reaches the backend
    n = len(calls)
    for bad in ({"temperature": -1}, {"temperature": "hot"}, {"temperature": True}, {"temperature": 1, "top_p": 0},
                {"temperature": 1, "top_p": 1.5}, {"top_k": -2}, {"top_k": 2.5}, {"seed": -1}, {"seed": 1 << 64},
                {"seed": "7"}, {"temperature": [1, 2]}, {"top_p": 2}):
        with pytest.raises(urllib.error.HTTPError) as e:
            _post(port, {"prompt": "q", **bad})
        assert e.value.code == 400, bad
    # a sampled request bound for the batch-sharded path (images on the queue server): 400 naming the limitation
    from test_server import _png_data_uri
    with pytest.raises(urllib.error.HTTPError) as e:
        _post(port, {"prompt": "q", "images": [_png_data_uri()], "temperature": 0.7})
    assert e.value.code == 400 and "batch-sharded" in e.value.read().decode()
    assert len(calls) == n
    assert _post(port, {"prompt": "q", "images": [_png_data_uri()]})[0] == 200          # greedy image requests still served


def test_http_merged_sampled_requests_keep_their_own_records(queue_server):
    port, calls = queue_server
    results = {}

    def worker(i, sampled):
        body = {"prompt": [f"p{i}a", f"p{i}b"], "max_tokens": 6}
        if sampled:
            body.update(temperature=0.5, seed=100 * i)
        results[i] = _post(port, body)[1]

    _post(port, {"prompt": "warm"})
    ths = [threading.Thread(target=worker, args=(i, i % 2 == 0)) for i in range(6)]
    [t.start() for t in ths]
    [t.join() for t in ths]
    for i in range(6):
        assert ("seeds" in results[i]) == (i % 2 == 0)
        if i % 2 == 0:
            assert results[i]["seeds"] == [100 * i, 100 * i + 1]
    for prompts, mt, images, recs in calls:
        if recs is None:
            continue
        assert len(recs) == len(prompts)                                  # one record per row, greedy rows never merged in
        for p, r in zip(prompts, recs):
            i, row = int(p[1:-1]), "ab".index(p[-1])
            assert i % 2 == 0 and r["seed"] == 100 * i + row


def test_http_continuous_backend_passes_sampling_through():
    from phi_3_vision_mlx_amd.server import make_handler, ContinuousBackend
    from http.server import ThreadingHTTPServer
    seen = []

    class Eng:
        def serve_forever(self, stop, idle_sleep=0.002):
            stop.wait()

        def generate(self, prompts, images=None, max_tokens=512, timeout=600.0, sampling=None):
            seen.append(sampling)
            return [f"{p}" for p in prompts]

    backend = ContinuousBackend(Eng())
    httpd = ThreadingHTTPServer(("127.0.0.1", 0), make_handler(backend))
    threading.Thread(target=httpd.serve_forever, daemon=True).start()
    port = httpd.server_address[1]
    try:
        from test_server import _png_data_uri
        code, out = _post(port, {"prompt": "a", "images": [_png_data_uri()], "temperature": 0.9, "seed": 1})
        assert code == 200 and out["seeds"] == [1] and seen[-1][0]["temperature"] == 0.9   # images sample on the engine
        _post(port, {"prompt": "a"})
        assert seen[-1] is None
    finally:
        httpd.shutdown()
        backend.close()


# ---------------------------------------------------------------------------------------------------- engine host logic
class SamplingStub:
    """test_engine_cpu.SlotStub plus the sampling methods, every model call recorded."""
    device = "cpu"

    def __init__(self):
        from test_engine_cpu import SlotStub
        self.base, self.calls = SlotStub(), []

    def new_slot_state(self, slots, window):
        return self.base.new_slot_state(slots, window)

    def decode_graph(self, st):
        return self.base.decode_graph(st)

    def prefill_slot(self, st, row, inputs, **kw):
        self.calls.append(("prefill_slot", row, tuple(kw)))
        tok = self.base.prefill_slot(st, row, inputs)
        if kw.get("return_logits"):
            return tok, torch.zeros((tok.shape[0], 1, 8))
        return tok

    def greedy_step(self, token, cache):
        self.calls.append(("greedy_step",))
        return self.base.greedy_step(token, cache)

    def set_sampling(self, st, records, row0=0):
        from phi_3_vision_mlx_amd import sampling
        self.calls.append(("set_sampling", row0, [(r["temperature"], r["counter"]) for r in sampling.unpack(records)]))
        st.sample_rows = True

    def sample_logits(self, st, logits, row0=0):
        self.calls.append(("sample_logits", row0))
        return torch.full((logits.shape[0], 1), 5, dtype=torch.int32)

    def sample_step(self, token, cache):
        self.calls.append(("sample_step",))
        return self.base.greedy_step(token, cache)


def _req(n, key):
    return {"input_ids": np.full((1, n), key, dtype=np.int64)}


def test_engine_greedy_traffic_never_touches_sampling():
    from phi_3_vision_mlx_amd.engine import ContinuousEngine
    stub = SamplingStub()
    eng = ContinuousEngine(stub, None, slots=3, window=256)
    hs = [eng.submit(_req(10 + i, 3 + i), 6) for i in range(4)]
    eng.run_until_idle()
    assert all(h.error is None for h in hs)
    names = {c[0] for c in stub.calls}
    assert names == {"prefill_slot", "greedy_step"}
    assert all(c[2] == () for c in stub.calls if c[0] == "prefill_slot")      # prefill_slot(st, row, inputs): as today


def test_engine_mixed_traffic_switches_variants_and_resets_counters():
    from phi_3_vision_mlx_amd.engine import ContinuousEngine
    stub = SamplingStub()
    eng = ContinuousEngine(stub, None, slots=2, window=256)
    g = eng.submit(_req(12, 7), 3)
    eng.step()
    eng.step()
    assert [c[0] for c in stub.calls] == ["prefill_slot", "greedy_step", "greedy_step"]
    s = eng.submit(_req(12, 9), 4, sampling={"temperature": 0.7, "top_p": 0.9, "seed": 5})
    eng.step()
    i = next(k for k, c in enumerate(stub.calls) if c[0] == "set_sampling")
    assert stub.calls[i][2] == [(pytest.approx(0.7), 0)]                      # the admitted row's record, counter reset
    assert [c[0] for c in stub.calls[i:i + 4]] == ["set_sampling", "prefill_slot", "sample_logits", "sample_step"]
    assert ("return_logits",) == stub.calls[i + 1][2]
    eng.run_until_idle()
    assert g.error is None and s.error is None and s.tokens[0] == 5 and len(s.tokens) == 4
    assert stub.calls[-1] == ("sample_step",) or stub.calls[-1] == ("greedy_step",)
    # once the sampled request has left, greedy traffic replays the greedy variant again -- and resets its rows' records
    stub.calls.clear()
    g2 = eng.submit(_req(12, 4), 3)
    eng.run_until_idle()
    assert g2.error is None
    assert [c[0] for c in stub.calls] == ["set_sampling", "prefill_slot", "greedy_step", "greedy_step"]
    assert stub.calls[0][2] == [(0.0, 0)]
    # a bad sampling setting fails the request at submit
    bad = eng.submit(_req(12, 4), 3, sampling={"temperature": -1})
    assert bad.done.is_set() and isinstance(bad.error, ValueError)
