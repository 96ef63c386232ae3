"""p3v_attention_decode_route against the recorded launches (tests/golden/attn_decode_routes.json: one rocprofv3 --kernel-trace run of
tools/attn_decode_routes.py on an MI355X).  With the recorded capacity and CU count the route touches no device: no GPU here."""
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
O_PROJ = {None: 0, "bf16": 1, "e4m3": 2, "q4": 3}            # p3v_attn_oproj_t


@pytest.fixture(scope="module")
def recording():
    with open(os.path.join(ROOT, "tests", "golden", "attn_decode_routes.json")) as f:
        rows = json.load(f)
    device = next(v for k, v in rows if k == "device")
    return device, [v for k, v in rows if k == "case"]


def route(ops, device, c, **over):
    """The route of a recorded case on the recorded device, every knob given (the defaults of p3v_runtime.hip where the case names none)."""
    knobs = dict({"q8_old": 0, "attn_fo_map": 2, "attn_fo_map_q8": 0}, **c["knobs"])
    kw = dict(o_proj=O_PROJ[c["o_proj"]], o_n=3072 if c["o_proj"] else 0, capacity=device[c["kind"]]["capacity"], cu_count=device["cu_count"], **knobs)
    kw.update(over)
    return ops.attention_decode_route(c["kind"] == "q8", c["B"], 1, c["heads"], 96, c["n_split"], c["cache_t"], c["merge_in_launch"], **kw)


def test_recording_covers_the_stated_cases(recording):
    device, cases = recording
    assert len(cases) == 80 and len({c["id"] for c in cases}) == 80
    kernels = {l[0] for c in cases for l in c["launches"]}
    assert kernels == {"k_attn_decode", "k_attn_decode128", "k_attn_decode128_o", "k_attn_decode128_o4", "k_attn_decode_stream<64>",
                       "k_attn_decode_q8", "k_attn_decode_q8s", "k_attn_decode128_q8<false>", "k_attn_decode128_q8<true>", "k_attn_combine2",
                       "k_attn_combine_o<1>", "k_attn_combine_o<2>", "k_attn_combine_o<3>"}
    assert {c["status"] for c in cases} == {0, -95}
    assert {k for c in cases for k in c["knobs"].items()} == {("q8_old", 1), ("attn_fo_map", 0), ("attn_fo_map", 1), ("attn_fo_map", 2),
                                                               ("attn_fo_map_q8", 1)}
    for kind in ("bf16", "q8"):
        d = device[kind]
        assert d["capacity"] == d["workgroups_per_cu"] * (device["cu_count"] - 8)
        assert 32 * d["largest_n_split"] <= d["capacity"] < 32 * (d["largest_n_split"] + 1)


def test_route_answers_every_recorded_case(recording):
    """Kernel, grid, block, merge launch and status of every recorded call, from the route alone."""
    from phi_3_vision_mlx_amd import ops
    device, cases = recording
    for c in cases:
        r = route(ops, device, c)
        assert r.status == c["status"], c["id"]
        if c["status"]:
            assert r.fuse_form == 0 and c["launches"] == [], c["id"]
            continue
        got = [[r.kernel_name.decode(), list(r.grid), [r.block, 1, 1]]]
        if r.merge != ops.L.ATTN_MERGE_IN_LAUNCH:
            got.append([r.merge_name.decode(), [r.merge_grid, 1, 1], [r.merge_block, 1, 1]])
        assert got == c["launches"], (c["id"], got)
        assert (r.merge_name == b"") == (r.merge == ops.L.ATTN_MERGE_IN_LAUNCH) and r.merge_name.decode() in ("", got[-1][0])
        assert r.fuse_form == (0 if not c["o_proj"] else 1 if len(got) == 1 else 2), c["id"]
        assert r.fo_remap == (0 if r.grid[1] > 1 or r.fuse_form != 1 else dict(c["knobs"]).get("attn_fo_map_q8" if c["kind"] == "q8" else "attn_fo_map", 2))


def test_can_fuse_functions_are_the_routes_fused_form(recording):
    """p3v_attention_decode_can_fuse_oproj / _q8_can_fuse_oproj answer the route's fused form: asked here with the library's knobs and
    'ask the device', where no device answers -- a capacity of none, so every in-launch form is refused and so is the merge launch's."""
    from phi_3_vision_mlx_amd import ops
    device, cases = recording
    for c in cases:
        if not c["o_proj"]:
            continue
        can = ops.L.lib().p3v_attention_decode_q8_can_fuse_oproj if c["kind"] == "q8" else ops.L.lib().p3v_attention_decode_can_fuse_oproj
        olds = [(k, ops.set_tuning(k, v)) for k, v in c["knobs"].items()]
        try:
            r = ops.attention_decode_route(c["kind"] == "q8", c["B"], 1, c["heads"], 96, c["n_split"], c["cache_t"], c["merge_in_launch"],
                                           o_proj=O_PROJ[c["o_proj"]], o_n=3072)
            assert can(c["B"], 1, c["heads"], 96, c["n_split"], c["cache_t"], 3072, c["merge_in_launch"]) == r.fuse_form, c["id"]
        finally:
            for k, v in olds:
                ops.set_tuning(k, v)
        # ... and with the recorded device the fused form is what the recorded call did
        assert route(ops, device, c).fuse_form == (0 if c["status"] else 1 if len(c["launches"]) == 1 else 2), c["id"]


def test_route_rules(recording):
    """The rules the recording cannot separate: the capacity bound is exact, the head-room of the merge launch is 8 CUs, a knob left
    negative is the library's setting, and a format that does not go with the cache is an argument error."""
    from phi_3_vision_mlx_amd import ops
    device, cases = recording
    by_id = {c["id"]: c for c in cases}
    c = by_id["bf16,B=1,nh=32,n_split=13,T=1664,merge=1,o=bf16"]
    assert route(ops, device, c, capacity=13 * 32).fuse_form == 1 and route(ops, device, c, capacity=13 * 32 - 1).status == ops.L.ERR_UNSUPPORTED
    c = by_id["bf16,B=1,nh=32,n_split=13,T=1664,merge=0,o=bf16"]
    assert route(ops, device, c, cu_count=232).fuse_form == 2 and route(ops, device, c, cu_count=231).status == ops.L.ERR_UNSUPPORTED
    c = by_id["q8,B=1,nh=4,n_split=16,T=1024,merge=1,o=None"]
    assert route(ops, device, c, q8_old=-1).kernel_name == b"k_attn_decode_q8s"
    old = ops.set_tuning("q8_old", 1)
    try:
        assert route(ops, device, c, q8_old=-1).kernel_name == b"k_attn_decode_q8" and route(ops, device, c).kernel_name == b"k_attn_decode_q8s"
    finally:
        ops.set_tuning("q8_old", old)
    with pytest.raises(RuntimeError):
        route(ops, device, c, o_proj=O_PROJ["bf16"], o_n=3072)
