"""The decode attention's plan is one record made by one planner (model.AttnPlan, Phi3VModel._plan) and still is what the four
planning functions over a dict made it: against the recording in tests/golden/attn_plans.json (written by
tests/golden/gen_golden_attn_plans.py from the code as it stood before; no GPU, no library) -- the plan of every case of the grid and
what Phi3VModel._layers hands the attention wrappers on every route."""
import dataclasses
import json
import os
import re

import pytest

import gen_golden_attn_plans as gen


@pytest.fixture(scope="module")
def got():
    """Recorded once from the code under test, shared by the tests below and left unchanged."""
    return gen.record_all()


def test_the_recording_is_byte_for_byte_what_the_generator_writes(got):
    with open(gen.PATH) as f:
        text = f.read()
    assert gen.dumps(got) == text
    assert len(text) < 64 * 1024


def test_the_plan_grid_is_the_stated_one(got):
    plans = got["plans"]
    n = len(gen.BS) * len(gen.LS) * len(gen.TS)
    assert (gen.BS, gen.LS) == ((1, 2, 8, 16), (1, 4, 16, 17)) and gen.TS == (64, 128, 1024, 1088, 1152, 2048, 2560, 6144, 6208, 8192, 32768)
    assert gen.STATES == ("bf16", "int8", "mlx4", "family", "slots", "serving") and gen.CUS == (256, 64) and len(gen.CAN) == 4
    assert n == 176 and len(plans["cases"]) == 6 * 4 * 2 + 6 * len(gen.VARIANTS) == 120
    assert all(len(v) == n * plans["width"] for v in plans["cases"].values())
    used = {v[i:i + plans["width"]] for v in plans["cases"].values() for i in range(0, len(v), plans["width"])}
    assert used == set(plans["outcomes"]) and len(set(plans["outcomes"].values())) == len(plans["outcomes"])


def test_every_knob_and_every_axis_changes_a_plan_somewhere(got):
    cases = got["plans"]["cases"]

    def base(kind, can="12", cus=256):
        return cases[f"{kind},can={can},cus={cus}"]

    assert {k.split("=")[0] for k in gen.VARIANTS if k.startswith("P3V_")} == set(gen.KNOBS)
    for name in gen.VARIANTS:
        assert any(cases[f"{kind},{name}"] != base(kind) for kind in gen.STATES), name
    assert base("mlx4") == base("bf16") and len({base(kind) for kind in gen.STATES}) == len(gen.STATES) - 1   # (mlx4: a bf16 cache to the plan)
    assert len({base("bf16", can) for can in ("00", "02", "10", "12")}) == 4 and len({base("int8", can) for can in ("00", "02", "10", "12")}) == 4
    # the library refusing the in-launch o_proj: a bf16-cache plan gives up its in-launch merge for the merge launch's o_proj, an int8 one never
    w, outcomes = got["plans"]["width"], {k: json.loads(v) for k, v in got["plans"]["outcomes"].items()}

    def gave_up_merge(kind):
        pairs = zip(*([outcomes[s[i:i + w]] for i in range(0, len(s), w)] for s in (base(kind, "00"), base(kind, "02"))))
        return sum(a[1] == 1 and b[1:3] == [0, 1] for a, b in pairs)

    assert gave_up_merge("bf16") > 0 and gave_up_merge("int8") == 0
    assert base("serving", cus=64) != base("serving") and base("bf16", cus=64) == base("bf16")
    assert base("family", "00") == base("family")                 # a family plan never asks for the fused o_proj


def test_layers_hands_the_plan_to_the_wrappers(got):
    layers = got["layers"]
    assert set(layers) == {f"{r},eager" for r in gen.ROUTES} | {f"{r},d_past" for r in gen.ROUTES if r not in ("beams", "prefill", "q8,prefill")}
    for name, rec in layers.items():
        n_split, merge, fuse_o, family = rec["plan"]
        attn = [c for c in rec["calls"] if c["op"].startswith("attention")]
        assert len(attn) == 2, name                                # one attention call per layer
        if name.split(",")[-2] in ("beams", "prefill"):
            continue
        assert {c["op"] for c in attn} == {"attention_decode_family" if family else "attention_decode_q8" if name.startswith("q8") else "attention_decode"}
        assert all(c["n_split"] == n_split and c["ws"] == "ws" for c in attn), name
        assert all(family or c["merge_in_launch"] == bool(merge) for c in attn), name
        assert all(c["rope_bstride"] == (int(name.split("L=")[1][0]) if "L=" in name else 1) for c in attn) or name.endswith("eager")
        if fuse_o:                                                 # the two all-ones buffers alternate, each launch re-arms the other
            assert [(c["out"], c["o_rearm"]) for c in attn] == [("o_f", "o_f2"), ("o_f2", "o_f")], name
            assert all("o_proj_x" in c["o_proj"] for c in attn)
        else:
            assert all(c["out"] == "o" and "o_proj" not in c and c.get("o_rearm") is None for c in attn), name
    assert layers["bf16,fused_in_merge,eager"]["plan"] == [2, 0, 1, 0] and layers["q8,fused_in_merge,eager"]["plan"][1:3] == [0, 1]
    assert layers["q4,fused_in_launch,d_past"]["calls"][0]["o_proj"] == ["o_proj_sb", "o_proj_w", "o_proj_x"]
    assert layers["q8,fused_in_launch,d_past"]["calls"][0]["o_proj"] == ["o_proj_scale", "o_proj_w8", "o_proj_x"]


def test_the_plan_is_a_record_with_defaults_and_the_rules_are_written_once():
    from phi_3_vision_mlx_amd import model
    p = model.AttnPlan()
    assert [f.name for f in dataclasses.fields(p)] == ["n_split", "ws", "attn_merge", "fuse_o", "family", "past_lb", "rope_cos", "rope_sin", "o_f", "o_f2"]
    assert (p.n_split, p.ws, p.attn_merge, p.fuse_o, p.family, p.past_lb, p.o_f) == (0, None, False, False, False, -1, None)
    with pytest.raises(AttributeError):
        p.no_such_field = 1
    with open(os.path.join(gen.ROOT, "phi-3-vision-mlx_amd", "model.py")) as f:
        src = f.read()
    for knob in gen.KNOBS:
        assert src.count(f'"{knob}"') == 1, knob
    planner = src[src.index("    def _plan("):src.index("    def _alloc_bufs(")]
    assert "self._plan(" not in planner and not re.search(r"def (_split_plan|_family_plan|_plan_fused_oproj)\b", src)
    assert not re.search(r'\["plan"\]\.\w+\s*=[^=]', src) and "os.environ" not in planner
