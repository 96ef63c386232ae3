"""The decoder's projection layer tells the weight formats apart in one place (ops._weight_format) and still does what it did when every
caller worked the format out for itself: the ops `Phi3VModel._proj_frozen` chooses and the arguments the GEMV wrappers hand to the
library, against the recording in tests/golden/proj_calls.json (written by tests/golden/gen_golden_proj_calls.py from the code as it
stood before; no model, no GPU) -- and the helpers that state the format rules."""
import pytest
import torch

import gen_golden_proj_calls as gen

KEY = gen.KEY


@pytest.fixture(scope="module")
def got():
    """Recorded once from the code under test, shared by the tests below and left unchanged."""
    return gen.record_all()


def test_the_recording_is_byte_for_byte_what_the_generator_writes(got):
    with open(gen.PATH) as f:
        text = f.read()
    assert gen.dumps(got) == text
    assert len(text) < 64 * 1024


def test_the_chooser_grid_is_the_stated_one(got):
    ch = got["chooser"]
    n = len(gen.ROWS) * len(gen.KS) * len(gen.MS) * len(gen.EPILOGUES) * 2
    assert n == 1260 and len(gen.STATES) * n == 7560
    assert list(ch["cases"]) == list(gen.STATES) + [f"q4,{k}=0" for k in gen.KNOBS] and all(len(v) == n for v in ch["cases"].values())
    assert len({s for v in list(ch["cases"].values())[:len(gen.STATES)] for s in v}) == 21
    # each knob changes the 4-bit route somewhere
    assert all(ch["cases"][f"q4,{k}=0"] != ch["cases"]["q4"] for k in gen.KNOBS)
    # a packed copy whose bf16 matrix was replaced: the bf16 route, the copy dropped, the captured steps declared stale
    assert ch["stale_copy"] == {"sequence": "gemv+", "in_w13": False, "epoch": 1}


def test_the_launch_cases_cover_every_format_and_entry(got):
    cases = got["launch"]
    symbols = {c["calls"][0][0] for c in cases.values() if "calls" in c}
    assert symbols == {"p3v_gemv" + f + s for f in ("", "_fp8", "_q4", "_b13") for s in ("", "_step")}
    assert sum("raises" in c for c in cases.values()) == 4 + 3            # the workspace check per format, the packed format's K checks
    assert all(cases[f"{fmt},step_{end},unsupported"]["returns"] is False for fmt in ("bf16", "fp8", "q4", "b13") for end in ("begin", "end"))


# ------------------------------------------------------------------ the helpers (they did not exist before: plain assertions)
def _handles(rows=64, K=3072):
    return {fmt: gen.handles(rows=rows, K=K)[fmt][0] for fmt in ("bf16", "fp8", "q4", "b13")}


def test_weight_shape_and_format_of_the_four_handles():
    from phi_3_vision_mlx_amd import ops
    for fmt, h in _handles(rows=24, K=576).items():
        assert ops._weight_format(h).name == fmt
        assert ops.weight_shape(h) == (24, 576)
    w4, sb = _handles(rows=24, K=576)["q4"]
    assert w4.shape == (24, 72) and ops.weight_shape((w4, sb))[1] == 8 * w4.shape[1]


def _model(state):
    return gen.shell(state, 64, 3072, device="cpu")


@pytest.mark.parametrize("state,kind", [("bf16", "bf16"), ("fp8", "fp8"), ("q4", "q4")])
@pytest.mark.parametrize("rows", [0, 1, 2])
def test_weight_returns_the_dict_entry_where_there_is_no_packed_copy(state, kind, rows):
    from phi_3_vision_mlx_amd import ops
    m = _model(state)
    h = m._weight(KEY, rows)
    assert h is {"bf16": m.w, "fp8": m.w8, "q4": m.w4}[kind][KEY] and ops._weight_format(h).name == kind
    assert m._handle(KEY, rows) == (h, kind)                      # the dict names the format the classifier reads off the handle
    assert m._weight("no.such.weight", rows) is None and m._handle("no.such.weight", rows) == (None, None) and m.epoch == 0


def test_weight_returns_the_packed_copy_for_one_row_while_it_is_current():
    from phi_3_vision_mlx_amd import ops
    m = _model("b13")
    pk = m.w13[KEY]
    assert m._weight(KEY, 1) is pk and m._handle(KEY, 1) == (pk, "b13") and ops._weight_format(pk).name == "b13"
    assert m._weight(KEY, 0) is m.w[KEY] and m._weight(KEY, 2) is m.w[KEY]
    assert m.epoch == 0 and m.w13[KEY] is pk
    m.w[KEY].add_(1)                                              # written to in place: the copy no longer stands for it
    assert m._weight(KEY, 2) is m.w[KEY] and KEY in m.w13 and m.epoch == 0       # (only a one-row launch looks)
    assert m._weight(KEY, 1) is m.w[KEY] and KEY not in m.w13 and m.epoch == 1
    assert m._weight(KEY, 1) is m.w[KEY] and m.epoch == 1         # absent now: nothing more to drop


def test_weight_drops_a_copy_of_a_replaced_matrix():
    m = _model("b13_stale")
    assert m._weight(KEY, 1) is m.w[KEY] and KEY not in m.w13 and m.epoch == 1


@pytest.mark.parametrize("state", ["bf16", "b13", "fp8", "q4"])
@pytest.mark.parametrize("B", [1, 2])
def test_fold_weight(state, B, monkeypatch):
    monkeypatch.delenv("P3V_STEP_FOLD", raising=False)
    m = _model(state)
    assert m._fold_weight(KEY, B) is m._weight(KEY, B) is not None
    assert (m._fold_weight(KEY, B) is m.w13.get(KEY)) == (state == "b13" and B == 1)
    assert m._fold_weight("no.such.weight", B) is None
    m.adapters = {KEY: (None, None, 1.0)}                         # an adapter on the key: the projection runs through _proj
    assert m._fold_weight(KEY, B) is None
    m.adapters, m._bank = {}, {KEY: (None, 1)}                    # the key in the bank
    assert m._fold_weight(KEY, B) is None
    m._bank = {"model.layers.0.self_attn.o_proj.weight": (None, 1)}
    assert m._fold_weight(KEY, B) is m._weight(KEY, B)            # (another key's adapter does not matter)
    monkeypatch.setenv("P3V_STEP_FOLD", "0")
    assert m._fold_weight(KEY, B) is None


def test_fused_oproj_keywords():
    x, rearm = torch.zeros(1), torch.zeros(2)
    want = {"bf16": {"o_proj_w", "o_proj_x", "o_rearm"}, "q4": {"o_proj_w", "o_proj_sb", "o_proj_x", "o_rearm"},
            "fp8": {"o_proj_w8", "o_proj_scale", "o_proj_x", "o_rearm"}}
    for state, names in want.items():
        m = _model(state)
        kw = m._fused_oproj_kw(KEY, x, rearm)
        assert set(kw) == names and kw["o_proj_x"] is x and kw["o_rearm"] is rearm
        h = m._weight(KEY)
        if state == "bf16":
            assert kw["o_proj_w"] is h
        else:
            names = ("o_proj_w8", "o_proj_scale") if state == "fp8" else ("o_proj_w", "o_proj_sb")
            assert all(kw[k] is t for k, t in zip(names, h))
    m = _model("b13")                                             # the fused launch streams the bf16 matrix, never the packed copy
    assert m._fused_oproj_kw(KEY, x, rearm)["o_proj_w"] is m.w[KEY]
