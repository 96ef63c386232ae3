"""Host side of the repetition / presence / frequency penalties and logit_bias (penalties.py, and their way through api.generate,
the engine and the server): argument checking, the record layout, the NumPy restatement of the rule of include/p3v.h on
hand-computed rows, request parsing and the 400s, the refusal under speculation, and the engine's bookkeeping on a stub model.
The kernels are pinned against `reference_adjust` bit for bit in tests/test_penalties_gpu.py."""
import ctypes
import json
import math
import threading
import urllib.error
import urllib.request

import numpy as np
import pytest
import torch

from phi_3_vision_mlx_amd import _lib, penalties
from phi_3_vision_mlx_amd.engine import ContinuousEngine, penalty_args

INF = float("inf")


def bf16(x):
    """float -> bf16 bits (uint16), through the module's own rounding of an fp32 value"""
    return penalties.f32_to_bf16_bits(np.asarray(x, dtype=np.float32))


def f32(bits):
    return penalties.bf16_bits_to_f32(bits)


# ----------------------------------------------------------------------------- rows / pack / unpack / off
def test_rows_defaults_are_off_and_scalars_spread_over_rows():
    r = penalties.rows(3)
    assert r == [(1.0, 0.0, 0.0, None)] * 3 and penalties.off(r)
    r = penalties.rows(2, 1.3, 0.5, 0.25, {5: -1.0, "7": 2})
    assert r == [(1.3, 0.25, 0.5, {5: -1.0, 7: 2.0})] * 2 and not penalties.off(r)       # (repetition, frequency, presence, bias)
    r = penalties.rows(3, [1.0, 1.2, 1.0], 0.0, [0.0, 0.0, 0.5], [None, None, {}])
    assert [penalties.active(x) for x in r] == [False, True, True] and r[2][3] is None   # an empty mapping: no bias
    assert not penalties.off(r)
    assert penalties.rows(1, logit_bias={3: -INF})[0][3] == {3: -INF}                    # -inf is a ban, allowed
    assert penalties.rows(1, np.float32(1.5))[0][0] == 1.5


@pytest.mark.parametrize("kw", [
    dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(repetition_penalty=INF), dict(repetition_penalty=math.nan),
    dict(repetition_penalty="1.2"), dict(repetition_penalty=True), dict(repetition_penalty=None),
    dict(presence_penalty=INF), dict(presence_penalty=math.nan), dict(presence_penalty="x"),
    dict(frequency_penalty=-INF), dict(frequency_penalty=math.nan), dict(frequency_penalty=[0.1]),
    dict(repetition_penalty=[1.1, 1.2, 1.3]), dict(presence_penalty=[0.0]),
    dict(logit_bias={-1: 1.0}), dict(logit_bias={100: 1.0}), dict(logit_bias={"x": 1.0}), dict(logit_bias={"1.5": 1.0}),
    dict(logit_bias={1.5: 1.0}), dict(logit_bias={True: 1.0}), dict(logit_bias={"-3": 1.0}),
    dict(logit_bias={3: math.nan}), dict(logit_bias={3: INF}), dict(logit_bias={3: "1"}), dict(logit_bias={3: None}),
    dict(logit_bias=[{3: 1.0}]), dict(logit_bias="3:1"), dict(logit_bias=[{3: 1.0}, 7]),
])
def test_rows_refuses(kw):
    with pytest.raises(ValueError):
        penalties.rows(2, vocab=100, **kw)


def test_rows_key_bound_is_the_vocabulary():
    assert penalties.rows(1, logit_bias={"99": 1.0}, vocab=100)[0][3] == {99: 1.0}
    with pytest.raises(ValueError, match="vocabulary"):
        penalties.rows(1, logit_bias={"100": 1.0}, vocab=100)
    assert penalties.rows(1, logit_bias={100000: 1.0})[0][3] == {100000: 1.0}            # no bound given: only >= 0


def test_pack_unpack_round_trip_against_the_struct():
    assert ctypes.sizeof(_lib.PenaltyRow) == 16 and penalties.RECORD_WORDS == 4
    rows = penalties.rows(4, [1.0, 1.3, 1.0, 0.75], [0.0, 0.5, 0.0, -0.25], [0.0, 0.125, 0.0, 2.0], [None, None, {1: -INF}, {0: 3.0}])
    rec = penalties.pack(rows)
    assert rec.dtype == torch.int32 and tuple(rec.shape) == (4, 4)
    back = penalties.unpack(rec)
    assert [b["flags"] for b in back] == [0, 1, 3, 3]
    for b, r in zip(back, rows):
        assert (b["repetition"], b["frequency"], b["presence"]) == tuple(float(np.float32(v)) for v in r[:3])
    raw = rec.numpy().view(np.float32)
    assert raw[1, 0] == np.float32(1.3) and raw[1, 1] == np.float32(0.125) and raw[1, 2] == np.float32(0.5)   # field order
    t = penalties.bias_table(rows, 8)
    assert t.dtype == np.float32 and t.shape == (4, 8) and t[2, 1] == -INF and t[3, 0] == 3.0 and np.count_nonzero(t) == 2
    assert penalties.bias_table(rows[:2], 8) is None


def test_seen_table_marks_prompt_and_counts_output():
    seen = penalties.seen_table([3, 3, 5, -1, 99], [5, 5, 7, 8, -1, 42], 8)
    assert seen.dtype == np.uint32
    assert seen.tolist() == [0, 0, 0, 0x80000000, 0, 0x80000002, 0, 1]


# ----------------------------------------------------------------------------- the rule, by hand
def test_reference_repetition_divides_positive_and_multiplies_negative_logits():
    bits = bf16([2.0, -2.0, 2.0, -2.0, 0.0])
    seen = np.array([1, 1, 0, 0x80000000, 0x80000000], dtype=np.uint32)
    out = penalties.reference_adjust(bits, (1.3, 0.0, 0.0, 1), seen)
    rp = np.float32(1.3)
    want = bf16([np.float32(2.0) / rp, np.float32(-2.0) * rp, 2.0, np.float32(-2.0) * rp, 0.0])
    assert out.tolist() == want.tolist()
    assert f32(out)[0] == 1.5390625 and f32(out)[1] == -2.59375                          # bf16(1.53846..), bf16(-2.6)
    assert out[2] == bits[2]                                                             # unseen: untouched
    assert f32(out)[3] == -2.59375                                                       # prompt-only counts as seen
    # rp = 1 never touches a value, seen or not
    assert penalties.reference_adjust(bits, (1.0, 0.0, 0.0, 1), seen).tolist() == bits.tolist()


def test_reference_frequency_and_presence_count_output_only():
    bits = bf16([4.0, 4.0, 4.0, 4.0])
    seen = np.array([0, 1, 3, 0x80000000], dtype=np.uint32)                              # c = 0, 1, 3, and prompt-only (c = 0)
    out = f32(penalties.reference_adjust(bits, (1.0, 0.5, 0.25, 1), seen))
    assert out.tolist() == [4.0, 4.0 - 0.5 - 0.25, 4.0 - 1.5 - 0.25, 4.0]
    out = f32(penalties.reference_adjust(bits, (2.0, 0.5, 0.25, 1), seen))               # repetition first, then the other two
    assert out.tolist() == [4.0, 2.0 - 0.5 - 0.25, 2.0 - 1.5 - 0.25, 2.0]
    # the product is rounded on its own: 0.1f * 3 in fp32, then the subtraction
    got = penalties.reference_adjust(bf16([1.0]), (1.0, 0.1, 0.0, 1), np.array([3], dtype=np.uint32))
    prod = np.float32(np.float32(0.1) * np.float32(3.0))
    assert got.tolist() == bf16([np.float32(1.0) - prod]).tolist()
    # a count of 2^31 - 1 is converted like any other uint32
    big = penalties.reference_adjust(bf16([1.0]), (1.0, 1.0, 0.0, 1), np.array([0x7FFFFFFF], dtype=np.uint32))
    assert f32(big)[0] == -2147483648.0


def test_reference_bias_ban_and_nan():
    bits = bf16([1.0, 2.0, 3.0, math.nan])
    bias = np.array([-INF, 0.5, 0.0, 1.0], dtype=np.float32)
    seen = np.zeros(4, dtype=np.uint32)
    out = penalties.reference_adjust(bits, (1.0, 0.0, 0.0, 3), seen, bias)
    assert f32(out)[0] == -INF and f32(out)[1] == 2.5 and f32(out)[2] == 3.0 and math.isnan(f32(out)[3])
    # the bias bit off, or no table: step 5 is skipped
    assert penalties.reference_adjust(bits[:3], (1.0, 0.0, 0.0, 1), seen[:3], bias[:3]).tolist() == bits[:3].tolist()
    assert penalties.reference_adjust(bits[:3], (1.0, 0.0, 0.0, 3), seen[:3], None).tolist() == bits[:3].tolist()
    # +inf logit with a ban: inf - inf = NaN, and stays NaN
    assert math.isnan(f32(penalties.reference_adjust(bf16([INF]), (1.0, 0.0, 0.0, 3), seen[:1], bias[:1]))[0])
    # rounding to bf16 is to nearest even: 1 + 2^-8 is a tie and falls to 1.0, 1 + 3 * 2^-8 rises to 1 + 2^-6
    tie = penalties.reference_adjust(bf16([1.0, 1.0]), (1.0, 0.0, 0.0, 3), seen[:2], np.array([2.0 ** -8, 3 * 2.0 ** -8], np.float32))
    assert f32(tie).tolist() == [1.0, 1.0 + 2.0 ** -6]


def test_reference_inactive_row_is_a_byte_copy():
    bits = np.array([0x8000, 0x7FC1, 0xFFA5, 0x3F80, 0x7F80], dtype=np.uint16)           # -0, two NaN payloads, 1.0, +inf
    seen = np.full(5, 0x80000005, dtype=np.uint32)
    bias = np.full(5, -INF, dtype=np.float32)
    for flags in (0, 2):                                                                 # (the bias bit alone does not activate a row)
        out = penalties.reference_adjust(bits, (1.3, 0.5, 0.5, flags), seen, bias)
        assert out.tolist() == bits.tolist() and out is not bits
    # an active row keeps -0 as -0 when nothing applies to it
    assert penalties.reference_adjust(bits[:1], (1.3, 0.0, 0.0, 1), np.zeros(1, np.uint32)).tolist() == [0x8000]


# ----------------------------------------------------------------------------- api: refusals before anything runs
def test_generate_refuses_penalties_under_speculation_and_bad_values_before_loading_a_model():
    from phi_3_vision_mlx_amd import api
    with pytest.raises(ValueError, match="speculate"):
        api.generate("hi", preload=(None, None), speculate=4, repetition_penalty=1.3, verbose=False)
    with pytest.raises(ValueError, match="speculate"):
        api.generate("hi", preload=(None, None), speculate=4, logit_bias={3: -INF}, verbose=False)
    with pytest.raises(ValueError, match="repetition_penalty"):
        api.generate("hi", preload=(None, None), repetition_penalty=0.0, verbose=False)
    with pytest.raises(ValueError, match="logit_bias"):
        api.generate("hi", preload=(None, None), logit_bias={"a": 1.0}, verbose=False)
    import inspect
    import phi_3_vision_mlx_amd as pkg
    sig = inspect.signature(api.generate).parameters
    assert (sig["repetition_penalty"].default, sig["presence_penalty"].default, sig["frequency_penalty"].default,
            sig["logit_bias"].default) == (1.0, 0.0, 0.0, None)
    assert "repetition_penalty" not in inspect.signature(pkg.generate).parameters        # the package-level call keeps the reference's


# ----------------------------------------------------------------------------- server: parsing, 400s, plumbing
def test_parse_penalties():
    from phi_3_vision_mlx_amd.server import parse_penalties
    assert parse_penalties({}, 2) is None
    assert parse_penalties({"repetition_penalty": 1.0, "presence_penalty": 0, "frequency_penalty": None, "logit_bias": {}}, 1) is None
    d = parse_penalties({"repetition_penalty": 1.3, "logit_bias": {"17": -100, "3": -1e30}}, 2, vocab=32)
    assert len(d) == 2 and d[0] == {"repetition_penalty": 1.3, "logit_bias": {"17": -100, "3": -INF}}
    d = parse_penalties(json.loads('{"logit_bias": {"4": -Infinity}}'), 1, vocab=32)
    assert d == [{"logit_bias": {"4": -INF}}]
    for bad in ({"repetition_penalty": 0}, {"repetition_penalty": "1.3"}, {"repetition_penalty": [1.3]}, {"presence_penalty": True},
                {"frequency_penalty": "a"}, {"logit_bias": [1, 2]}, {"logit_bias": "x"}, {"logit_bias": {"x": 1}},
                {"logit_bias": {"32": 1}}, {"logit_bias": {"-1": 1}}, {"logit_bias": {"3": "1"}}, {"logit_bias": {"3": 1e999}},
                {"logit_bias": {"3": [1]}}):
        with pytest.raises(ValueError):
            parse_penalties(bad, 1, vocab=32)


def _post(port, payload):
    req = urllib.request.Request(f"http://127.0.0.1:{port}/v1/completions", data=json.dumps(payload).encode(),
                                 headers={"Content-Type": "application/json"})
    with urllib.request.urlopen(req, timeout=10) as r:
        return r.status, json.loads(r.read())


@pytest.fixture(params=[True, False], ids=["merge", "solo"])
def server(request):
    from phi_3_vision_mlx_amd.server import serve
    calls = []

    def fake_generate(prompts, max_tokens, images=None, sampling=None, adapter=None, speculate=0, spec_info=None, logprobs=None,
                      logprob_info=None, penalties=None):
        calls.append(dict(prompts=list(prompts), penalties=penalties, speculate=speculate, sampling=sampling))
        out = [f"{p}|{max_tokens}" for p in prompts]
        return out[0] if len(out) == 1 else out

    httpd, engine = serve(fake_generate, port=0, host="127.0.0.1", merge=request.param, max_tokens_cap=1000, vocab_size=64,
                          speculate=True, speculate_default=4)
    t = threading.Thread(target=httpd.serve_forever, daemon=True)
    t.start()
    yield httpd.server_address[1], calls
    httpd.shutdown()
    engine.close()


def test_server_carries_the_fields_and_answers_400(server):
    port, calls = server
    status, body = _post(port, {"prompt": ["a", "b"], "max_tokens": 5, "repetition_penalty": 1.2, "presence_penalty": 0.5,
                                "frequency_penalty": 0.25, "logit_bias": {"7": -100.0}})
    assert status == 200 and body["responses"] == ["a|5", "b|5"]
    want = {"repetition_penalty": 1.2, "presence_penalty": 0.5, "frequency_penalty": 0.25, "logit_bias": {"7": -100.0}}
    assert calls[-1]["penalties"] == [want, want] and calls[-1]["speculate"] == 0       # (the server-wide speculate default steps aside)
    # defaults: the call is today's (no keyword at all)
    assert _post(port, {"prompt": "c", "max_tokens": 5, "repetition_penalty": 1.0, "logit_bias": {}})[0] == 200
    assert calls[-1]["penalties"] is None
    for bad, word in (({"repetition_penalty": -1}, "repetition_penalty"), ({"presence_penalty": "x"}, "presence_penalty"),
                      ({"frequency_penalty": [1]}, "frequency_penalty"), ({"logit_bias": {"64": 1.0}}, "vocabulary"),
                      ({"logit_bias": {"tok": 1.0}}, "logit_bias"), ({"logit_bias": [1]}, "logit_bias"),
                      ({"logit_bias": {"3": 1.0}, "speculate": 4}, "speculative")):
        n = len(calls)
        with pytest.raises(urllib.error.HTTPError) as e:
            _post(port, dict({"prompt": "x", "max_tokens": 3}, **bad))
        assert e.value.code == 400 and word in json.loads(e.value.read())["error"]
        assert len(calls) == n                                                          # nothing reached the engine


def test_server_refuses_penalties_on_the_sharded_path():
    from phi_3_vision_mlx_amd.server import serve
    httpd, engine = serve(lambda prompts, max_tokens, *a, **k: [f"{p}" for p in prompts], port=0, host="127.0.0.1",
                          sharded_fn=lambda prompts, images: True)
    t = threading.Thread(target=httpd.serve_forever, daemon=True)
    t.start()
    try:
        with pytest.raises(urllib.error.HTTPError) as e:
            _post(httpd.server_address[1], {"prompt": "x", "presence_penalty": 1.0})
        assert e.value.code == 400 and "batch-sharded" in json.loads(e.value.read())["error"]
    finally:
        httpd.shutdown()
        engine.close()


def test_continuous_backend_hands_penalties_to_the_engine():
    from phi_3_vision_mlx_amd.server import ContinuousBackend
    seen = {}

    class Eng:
        def serve_forever(self, stop, idle_sleep=0.002):
            stop.wait()

        def generate(self, prompts, images, max_tokens, timeout, **kw):
            seen.update(kw)
            return ["t"] * len(prompts)
    b = ContinuousBackend(Eng())
    try:
        assert b.submit(["p"], 4, penalties=[{"presence_penalty": 1.0}]) == ["t"]
        assert seen == {"penalties": [{"presence_penalty": 1.0}]}
        seen.clear()
        b.submit(["p"], 4)
        assert seen == {}
    finally:
        b.close()


# ----------------------------------------------------------------------------- engine bookkeeping on a stub model
class _State:
    def __init__(self, slots, window):
        self.pad_len = torch.full((slots,), window, dtype=torch.int32)
        self.offset, self.T, self.graphs = 0, window, {}
        self.penalty, self.sample_rows = None, None


class PenaltyStub:
    """The slot interface of the model with its penalty calls recorded: tokens are 100 + row for plain steps and 200 + row for
    penalised ones, so a test can tell which replay ran."""
    device = "cpu"
    cfg = type("Cfg", (), {"vocab_size": 1000})()

    def __init__(self):
        self.log = []
        self.flags = None

    def new_slot_state(self, slots, window):
        self.flags = [0] * slots
        return _State(slots, window)

    def decode_graph(self, st):
        return st.graphs.setdefault("greedy", {"tok": torch.zeros(len(st.pad_len), dtype=torch.int32), "host_tok": None,
                                               "history": torch.zeros((len(st.pad_len), 64), dtype=torch.int32), "bufs": {}})

    def set_sampling(self, st, records, row0=0):
        st.sample_rows = True

    def set_penalties(self, st, records, prompt_ids, row0=0, bias=None, pad=None):
        st.penalty = True
        recs = penalties.unpack(records)
        for i, r in enumerate(recs):
            self.flags[row0 + i] = r["flags"]
        self.log.append(("set", row0, [r["flags"] for r in recs], np.asarray(prompt_ids).shape, None if bias is None else bias.shape,
                         None if pad is None else list(pad)))

    def clear_penalties(self, st, row0=0, n=None):
        for i in range(row0, len(self.flags) if n is None else row0 + n):
            self.flags[i] = 0
        self.log.append(("clear", row0, n))

    def penalized_logits(self, st, logits, row0=0):
        self.log.append(("adjust", row0))
        return logits

    def sample_logits(self, st, logits, row0=0):
        n = logits.shape[0]
        return torch.arange(200 + row0, 200 + row0 + n, dtype=torch.int32)[:, None]

    def prefill_slot(self, st, row, inputs, return_logits=False):
        ids = np.asarray(inputs["input_ids"])
        n = 1 if ids.ndim == 1 else ids.shape[0]
        toks = torch.arange(100 + row, 100 + row + n, dtype=torch.int32)[:, None]
        return (toks, torch.zeros((n, 1, 8))) if return_logits else toks

    def _step(self, cache, base, name):
        st = cache[0].state
        st.offset += 1
        self.log.append((name, list(self.flags)))
        g = self.decode_graph(st)
        g["host_tok"] = torch.arange(base, base + len(st.pad_len), dtype=torch.int32)[:, None]
        return None, g["host_tok"]

    def greedy_step(self, token, cache):
        return self._step(cache, 100, "greedy_step")

    def penal_step(self, token, cache):
        return self._step(cache, 200, "penal_step")


def _req(n, seed=0):
    return {"input_ids": np.random.default_rng(seed).integers(3, 600, (1, n)).astype(np.int64)}


def test_engine_sets_records_before_the_first_token_and_resets_a_refilled_row():
    m = PenaltyStub()
    e = ContinuousEngine(m, None, slots=1, window=4096)
    a = e.submit(penalty_args(_req(12, 1), repetition_penalty=1.3, logit_bias={"5": -INF}), 3)
    b = e.submit(_req(12, 2), 3)                                                      # takes over the one slot afterwards
    e.run_until_idle()
    assert a.error is None and b.error is None
    assert a.penalties == (1.3, 0.0, 0.0, {5: -INF}) and b.penalties is None
    assert a.tokens == [200, 200, 200]                                                   # first token from the adjusted prefill logits,
    assert b.tokens == [100, 100, 100]                                                   # ... then penalised replays; b: plain ones
    names = [x[0] for x in m.log]
    assert names.index("set") < names.index("adjust") < names.index("penal_step")
    assert m.log[names.index("set")][1:5] == (0, [3], (1, 12), (1, 1000))                 # active + bias, the prompt, a bias table
    # the row is inactive again before b's first step: cleared at a's release and again at b's prefill
    first_plain = names.index("greedy_step")
    assert "clear" in names[:first_plain] and m.log[first_plain][1] == [0]
    assert all(x[1] == [3] for x in m.log if x[0] == "penal_step")


def test_engine_picks_the_penalised_replay_while_any_active_row_is_penalised():
    m = PenaltyStub()
    e = ContinuousEngine(m, None, slots=2, window=4096)
    plain = e.submit(_req(10, 1), 6)
    pen = e.submit(penalty_args(_req(10, 2), presence_penalty=0.5), 3)
    e.run_until_idle()
    assert plain.error is None and pen.error is None
    # rows are prefilled as one group: both first tokens come from the sampled pick on adjusted logits
    steps = [x for x in m.log if x[0].endswith("_step")]
    assert [x[0] for x in steps] == ["penal_step"] * 2 + ["greedy_step"] * 3
    assert steps[0][1].count(1) == 1 and steps[-1][1] == [0, 0]                          # one active record, none once it left
    assert len(pen.tokens) == 3 and len(plain.tokens) == 6


def test_engine_refuses_bad_penalties_at_submit():
    m = PenaltyStub()
    e = ContinuousEngine(m, None, slots=1, window=4096)
    for bad in (dict(repetition_penalty=0.0), dict(frequency_penalty=INF), dict(logit_bias={"1000": 1.0}), dict(logit_bias={"a": 1})):
        r = e.submit(penalty_args(_req(8), **bad), 3)
        assert r.done.is_set() and isinstance(r.error, ValueError)
    assert not e.waiting
    r = e.submit(penalty_args(_req(8), repetition_penalty=1.0), 2)                    # all defaults: a plain request
    e.run_until_idle()
    assert r.penalties is None and r.tokens == [100, 100] and not any(x[0] == "set" for x in m.log)


def test_fleet_refuses_bad_penalties_on_rank_zero_and_local_requests_keep_theirs():
    """world = 1: the fleet's own engine serves everything; a bad value never reaches it."""
    from phi_3_vision_mlx_amd import fleet
    m = PenaltyStub()
    eng = ContinuousEngine(m, None, slots=1, window=4096)
    front = fleet.EngineFleet(eng, (None, None), 1)
    h = front.submit(penalty_args(_req(8), repetition_penalty=-2.0), 3)
    assert h.done.is_set() and isinstance(h.error, ValueError) and not eng.waiting
    h = front.submit(penalty_args(_req(8), frequency_penalty=0.5), 2)
    eng.run_until_idle()
    assert h.error is None and h.tokens == [200, 200] and h.penalties == (1.0, 0.5, 0.0, None)
