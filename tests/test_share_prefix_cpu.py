"""Host side of share_prefix: the family table as a pure function (parallel.family_table / families_without, model.set_families'
refusals), the engine's bookkeeping on the CPU stand-ins of tests/test_engine_cpu.py -- as a trace of table writes against
prefills --, and the server flag.  The device side is tests/test_attn_family_gpu.py and tests/test_share_prefix_gpu.py."""
import json
import threading
import urllib.error
import urllib.request

import numpy as np
import pytest

from test_engine_cpu import EOS, req
from test_parallel_sampling_cpu import ForkStub

from phi_3_vision_mlx_amd.parallel import FAMILY_INTS, families_without, family_pays, family_table


def _single(b):
    return [b, 0, b] + [-1] * 15


def test_table_of_several_families():
    t = family_table(8, [((5, 2, 7), 300), ((3, 0), 41), ((6,), 9)])
    assert t.shape == (8, FAMILY_INTS) and t.dtype == np.int32
    assert t[5].tolist() == [5, 300, 5, 2, 7] + [-1] * 13                       # the leader's row lists the family, itself first
    assert t[2].tolist() == [5, 300] + [-1] * 16 and t[7].tolist() == [5, 300] + [-1] * 16
    assert t[3].tolist() == [3, 41, 3, 0] + [-1] * 14 and t[0].tolist() == [3, 41] + [-1] * 16
    assert [t[b].tolist() for b in (1, 4, 6)] == [_single(b) for b in (1, 4, 6)]   # no family, and a family of one: single rows
    assert family_table(3, []).tolist() == [_single(b) for b in range(3)]


def test_table_of_a_family_of_16_and_the_refusals():
    rows = [9, 0, 15] + [r for r in range(16) if r not in (9, 0, 15)]
    t = family_table(16, [(rows, 1234)])
    assert t[9].tolist() == [9, 1234] + rows and all(t[r, :2].tolist() == [9, 1234] for r in range(16))
    with pytest.raises(ValueError, match="at most 16 rows"):
        family_table(17, [(list(range(17)), 10)])
    with pytest.raises(ValueError, match="one family, once"):                   # overlapping families
        family_table(8, [((0, 1, 2), 10), ((2, 3), 10)])
    with pytest.raises(ValueError, match="one family, once"):
        family_table(8, [((0, 1, 1), 10)])
    with pytest.raises(ValueError, match="rows of a state of 4"):
        family_table(4, [((0, 4), 10)])
    with pytest.raises(ValueError, match="negative"):
        family_table(4, [((0, 1), -1)])


def test_families_without():
    fams = [((5, 2, 7), 300), ((3, 0), 41)]
    assert families_without(fams, [2]) == [((5, 7), 300), ((3, 0), 41)]
    assert families_without(fams, [5]) == [((2, 7), 300), ((3, 0), 41)]           # the leader left: the next member leads
    assert families_without(fams, [0]) == [((5, 2, 7), 300)]                       # one member left of two: the family is cleared
    assert families_without(fams, [5, 2, 3]) == [] and families_without(fams, [1]) == fams


def test_break_even_rule():
    """(rows - 1) x shared keys >= 4096: the losing and the winning shapes of profiles/share_prefix_step_time.txt on their sides."""
    assert not family_pays(2, 512) and not family_pays(4, 512) and not family_pays(2, 2531) and not family_pays(1, 10 ** 6)
    assert family_pays(16, 512) and family_pays(4, 2531) and family_pays(8, 2531) and family_pays(2, 32768)


class _St:
    def __init__(self, quantized=False, mlx4=False):
        self.B, self.offset, self.quantized, self.mlx4, self.slots = 4, 100, quantized, mlx4, False
        self.family = self.family_host = None
        self.families = []


def test_set_families_refuses_a_quantised_state_before_it_touches_anything():
    from phi_3_vision_mlx_amd.model import Phi3VModel
    m = object.__new__(Phi3VModel)                                                # (no weights, no device: the checks come first)
    m.device = "cpu"
    for st, word in ((_St(quantized=True), "int8"), (_St(mlx4=True), "mlx4")):
        with pytest.raises(ValueError, match=f"share_prefix needs the bf16 KV cache.*{word}"):
            Phi3VModel.set_families.__wrapped__(m, st, [((0, 1), 50)])
        assert st.family is None and st.families == []
        Phi3VModel.set_families.__wrapped__(m, st, [])                            # nothing to clear: accepted, nothing made
        assert st.family is None
    st = _St()
    with pytest.raises(ValueError, match="one family, once"):
        Phi3VModel.set_families.__wrapped__(m, st, [((0, 1), 50), ((1, 2), 50)])
    with pytest.raises(ValueError, match="beyond the cache length"):
        Phi3VModel.set_families.__wrapped__(m, st, [((0, 1), 101)])
    assert st.family is None


# ----------------------------------------------------------------------------- engine: table writes against prefills
class ShareStub(ForkStub):
    """ForkStub plus the family table: every table write and every prefill goes to one trace."""

    def __init__(self):
        super().__init__()
        self.trace, self.table = [], None

    def family_refusal(self, st=None):
        return None

    def set_families(self, st, families, create=False):
        self.table = family_table(len(st.pad_len), families)                     # (raises what the model would raise)
        self.trace.append(("table", [(tuple(rows), se) for rows, se in families], bool(create)))

    def prefill_slot(self, st, row, inputs, return_logits=False):
        n = np.asarray(inputs["input_ids"]).reshape(-1, np.asarray(inputs["input_ids"]).shape[-1]).shape[0]
        if self.table is not None:                                               # THE invariant: nobody's `lead` is a row being refilled
            for b in range(len(st.pad_len)):
                assert b in range(row, row + n) or int(self.table[b, 0]) not in range(row, row + n), (row, n, self.table[:, 0].tolist())
            assert all(self.table[r, :3].tolist() == [r, 0, r] for r in range(row, row + n)), "a refilled row is still in a family"
        self.trace.append(("prefill", row, n))
        return super().prefill_slot(st, row, inputs, return_logits=return_logits)


def _engine(slots=4, **kw):
    from phi_3_vision_mlx_amd.engine import ContinuousEngine
    m = ShareStub()
    return m, ContinuousEngine(m, None, slots=slots, window=4096, **kw)


def _tables(m):
    return [t[1] for t in m.trace if t[0] == "table"]


def test_engine_registers_the_family_and_rewrites_the_table_as_members_leave():
    from phi_3_vision_mlx_amd.engine import n_args
    m, e = _engine(4, share_prefix=True)
    assert m.trace == [("table", [], True)]                                       # the table exists before any step is captured
    head = e.submit(n_args(req(20, 1), 3), 40, sampling={"temperature": 0.8, "seed": 41})
    late = [e.submit(req(12 + i, 50 + i), 5) for i in range(3)]                 # they refill the rows the members leave
    e.run_until_idle()
    assert m.forks == [(0, [1, 2], 20, 0)] and head.family_done.is_set()
    lens = {c.row: len(c.tokens) for c in head.members}
    assert len(set(lens.values())) > 1, lens                                     # the members left at different steps
    fams, want = [((0, 1, 2), 20)], [[], [((0, 1, 2), 20)]]
    for row in sorted(lens, key=lambda r: (lens[r], r)):                         # every leaving rewrites the table, in leaving order
        if any(row in rows for rows, _ in fams):
            fams = families_without(fams, [row])
            want.append(fams)
    assert _tables(m) == want and want[-1] == [] and len(want) == 4               # 3 rows -> 2 rows -> cleared (the last one: no write)
    assert e.families == [] and m.table[:, 0].tolist() == [0, 1, 2, 3]
    assert all(r.error is None and r.done.is_set() for r in late)
    assert {t[1] for t in m.trace if t[0] == "prefill"} >= {0, 3}                   # (rows were refilled: ShareStub.prefill_slot checked each)


def test_the_leader_leaving_re_elects_before_its_row_is_refilled():
    from phi_3_vision_mlx_amd.engine import n_args
    m, e = _engine(3, share_prefix=True)
    head = e.submit(n_args(req(20, 4), 3), 40)                                    # (greedy: the three rows run the same length)
    e.step()
    assert e.families == [((0, 1, 2), 20)] and m.table[0].tolist()[:5] == [0, 20, 0, 1, 2]
    waiting = e.submit(req(15, 9), 4)
    head.members[0].cancelled = True                                              # the leader alone goes first (head.cancel() would take the family)
    e.step()                                                                      # released; its row is free from the next admission on
    assert e.families == [((1, 2), 20)] and m.table[1].tolist()[:4] == [1, 20, 1, 2] and m.table[2, 0] == 1
    assert m.table[0].tolist() == [0, 0, 0] + [-1] * 15
    n_before = len(m.trace)
    e.run_until_idle()
    assert waiting.error is None and waiting.row == 0 and ("prefill", 0, 1) in m.trace[n_before - 1:]
    i_tab = m.trace.index(("table", [((1, 2), 20)], False))
    i_fill = max(i for i, t in enumerate(m.trace) if t == ("prefill", 0, 1))
    assert i_tab < i_fill                                                         # the table was rewritten BEFORE the row was refilled


def test_a_failed_family_prefill_leaves_no_family_behind():
    from phi_3_vision_mlx_amd.engine import n_args
    m, e = _engine(4, share_prefix=True)
    m.fail_fork = True
    head = e.submit(n_args(req(20, 1), 3), 10)
    e.step()
    assert head.error is not None and e.families == [] and all(t[1] == [] for t in m.trace if t[0] == "table")
    m.fail_fork = False
    ok = e.submit(n_args(req(20, 1), 2), 6)
    e.run_until_idle()
    assert ok.error is None and [((0, 1), 20)] in _tables(m) and e.families == []


def test_off_by_default_nothing_of_it_is_called():
    from phi_3_vision_mlx_amd.engine import n_args
    m, e = _engine(4)
    head = e.submit(n_args(req(20, 1), 3), 12)
    e.run_until_idle()
    assert head.family_done.is_set() and [t for t in m.trace if t[0] == "table"] == [] and e.families == [] and not e.share_prefix


def test_engine_refuses_share_prefix_on_a_quantised_model():
    from phi_3_vision_mlx_amd.engine import ContinuousEngine
    m = ShareStub()
    m.family_refusal = lambda st=None: "share_prefix needs the bf16 KV cache: the shared-prefix attention has no int8 form"
    with pytest.raises(ValueError, match="bf16 KV cache"):
        ContinuousEngine(m, None, slots=2, window=4096, share_prefix=True)


# ----------------------------------------------------------------------------- server
def test_share_prefix_flag_parses_and_reaches_the_engines(monkeypatch):
    from phi_3_vision_mlx_amd import api, engine, server
    ap = server.arg_parser()
    assert ap.parse_args(["--continuous"]).share_prefix is False and ap.parse_args([]).share_prefix is False
    assert ap.parse_args(["--share-prefix", "--continuous"]).share_prefix is True and ap.parse_args(["--share-prefix"]).share_prefix is True
    made = []

    class Eng:
        def __init__(self, model, processor, **kw):
            self.processor = processor
            made.append(kw)

    class Stop(Exception):
        pass

    def stop(*a, **kw):
        raise Stop
    model = type("M", (), {"serving": False, "device": "cpu", "family_refusal": lambda self: None})()
    monkeypatch.setattr(api, "load", lambda **kw: (model, None))
    monkeypatch.setattr(engine, "ContinuousEngine", Eng)
    monkeypatch.setattr(server, "serve_continuous", stop)
    for flag in (True, False):
        with pytest.raises(Stop):
            server.run(port=0, synthetic=True, continuous=True, long_window=8192, share_prefix=flag)
    assert made == [{"slots": 8, "share_prefix": True}, {"slots": 4, "window": 8192, "share_prefix": True}, {"slots": 8}, {"slots": 4, "window": 8192}]
    # the one-request path: generate gets share_prefix for a family, and only with the flag
    seen = []

    def serve(generate_fn, **kw):
        seen.append((generate_fn, kw.get("share_refusal", "absent")))
        raise Stop
    monkeypatch.setattr(server, "serve", serve)
    calls = []
    monkeypatch.setattr(api, "generate", lambda *a, **kw: calls.append(kw) or ["x"])
    for flag in (True, False):
        with pytest.raises(Stop):
            server.run(port=0, synthetic=True, share_prefix=flag)
        seen[-1][0](["p"], 4, n=3)
        seen[-1][0](["p"], 4)
    assert [c.get("share_prefix") for c in calls] == [True, None, None, None] and [s[1] for s in seen] == [None, "absent"]


def test_server_answers_400_where_a_family_cannot_share():
    from phi_3_vision_mlx_amd.server import serve
    why = "share_prefix needs the bf16 KV cache: the shared-prefix attention has no int8 form (quantize_cache=True)"
    httpd, queue = serve(lambda prompts, max_tokens, **kw: ["t"] * (kw.get("n") or len(prompts)), port=0, share_refusal=why)
    threading.Thread(target=httpd.serve_forever, daemon=True).start()

    def post(body):
        r = urllib.request.Request(f"http://127.0.0.1:{httpd.server_address[1]}/v1/completions", data=json.dumps(body).encode(),
                                   headers={"Content-Type": "application/json"})
        with urllib.request.urlopen(r, timeout=30) as resp:
            return json.loads(resp.read())
    try:
        with pytest.raises(urllib.error.HTTPError) as e:
            post({"prompt": "hi", "max_tokens": 4, "n": 3})
        assert e.value.code == 400 and "bf16 KV cache" in json.loads(e.value.read())["error"]
        assert post({"prompt": "hi", "max_tokens": 4})["responses"] == ["t"]        # a request without a family is served
    finally:
        httpd.shutdown()
        queue.close()
