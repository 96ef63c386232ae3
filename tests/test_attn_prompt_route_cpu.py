"""p3v_attention_route against the recorded launches (tests/golden/attn_prompt_routes.json: one rocprofv3 --kernel-trace run of
tools/attn_prompt_routes.py on an MI355X, taken before the rules were gathered into the route).  The route asks no device: no GPU here."""
import itertools
import json
import math
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULTS = {"attn_old": 0, "attn_no_dma": 0, "attn_pp": -1, "attn_il": -1, "attn_il_waves": -1}     # p3v_runtime.hip (-1: by shape)
QUERIES_PER_WORKGROUP = {"ATTN": 64, "PREFILL": 128, "DMA": 128, "PP": 256, "IL4": 128, "IL8": 256}


@pytest.fixture(scope="module")
def ops():
    from phi_3_vision_mlx_amd import ops as o
    return o


@pytest.fixture(scope="module")
def cases():
    with open(os.path.join(ROOT, "tests", "golden", "attn_prompt_routes.json")) as f:
        return json.load(f)


def route(ops, c, **over):
    kw = dict(past=c["past"], past_t=c["past_t"], n_split=c["n_split"], new_is_cache=c["new_is_cache"], q_prescaled=c["q_prescaled"],
              has_ws=c["has_ws"], combine_g=-1, **dict(DEFAULTS, **c["knobs"]))
    kw.update(over)
    return ops.attention_route(c["B"], c["L"], c["heads"], c["kv_heads"], c["hd"], **kw)


def launches(r):
    got = [[r.kernel_name.decode(), list(r.grid), [r.block, 1, 1]]] if r.kernel >= 0 else []
    return got + ([[r.merge_name.decode(), [r.merge_grid, 1, 1], [r.merge_block, 1, 1]]] if r.merge else [])


def test_recording_covers_the_stated_cases(cases):
    assert len(cases) == 57 and len({c["id"] for c in cases}) == 57
    kernels = {l[0] for c in cases for l in c["launches"]}
    assert kernels == ({"k_attn<%d>" % hd for hd in (96, 64)} | {"k_attn_prefill<%d>" % hd for hd in (96, 64)}
                       | {"k_attn_prefill_%s<%d, %s>" % (k, hd, pre) for k in ("dma", "pp") for hd in (96, 64) for pre in ("true", "false")}
                       | {"k_attn_prefill_il<%d, %d>" % (hd, nw) for hd in (96, 64) for nw in (4, 8)} | {"k_attn_combine2"})
    assert {c["status"] for c in cases} == {0, -22, -95}
    assert {k for c in cases for k in c["knobs"].items()} == {("attn_old", 1), ("attn_no_dma", 1), ("attn_pp", 0), ("attn_pp", 1), ("attn_il", 0),
                                                               ("attn_il", 1), ("attn_il_waves", 4), ("attn_il_waves", 8)}
    shapes = {(c["B"], c["L"], c["q_prescaled"]) for c in cases if not c["knobs"] and c["hd"] == 96 and c["new_is_cache"]}
    assert {(1, L, 1) for L in (767, 768, 2815, 2816, 3071, 3072, 6143, 6144)} <= shapes             # every threshold, from both sides
    assert {(2, L, 1) for L in (3583, 3584, 6143, 6144)} | {(1, 3071, 0), (1, 3072, 0)} <= shapes
    assert {(c["L"], c["n_split"], c["has_ws"]) for c in cases if c["L"] in (16, 17) and not c["knobs"]} == set(itertools.product((16, 17), (1, 4), (0, 1)))
    assert any(c["B"] * c["L"] == 0 and c["status"] == 0 and not c["launches"] for c in cases)


def test_route_answers_every_recorded_case(ops, cases):
    """Status, kernel, grid, block and the merge launch of every recorded call, from the route alone."""
    for c in cases:
        r = route(ops, c)
        assert r.status == c["status"], c["id"]
        assert launches(r) == c["launches"], (c["id"], launches(r))
        assert (r.merge_name == b"") == (not r.merge) and (r.kernel_name == b"") == (r.kernel == ops.L.ATTN_PK_NONE)


def test_a_negative_knob_is_the_librarys_setting(ops, cases):
    c = next(c for c in cases if c["id"].startswith("B=1,L=6144,") and not c["knobs"])
    assert route(ops, c).kernel == ops.L.ATTN_PK_IL8 and route(ops, c, attn_il=0).kernel == ops.L.ATTN_PK_PP
    old = ops.set_tuning("attn_il", 0)
    try:
        assert route(ops, c).kernel == ops.L.ATTN_PK_PP and route(ops, c, attn_il=1).kernel == ops.L.ATTN_PK_IL8
    finally:
        ops.set_tuning("attn_il", old)
    c = next(c for c in cases if c["launches"] and c["launches"][-1][0] == "k_attn_combine2")
    assert [route(ops, c, combine_g=g).merge_block for g in (-1, 4, 8, 16)] == [256, 256, 512, 1024]
    assert route(ops, c, n_split=9).merge_block == 512                                               # by shape: 8 groups beyond 8 splits


@pytest.mark.parametrize("nh,hd,T,head_group", [(32, 96, 5461, 32), (32, 96, 5462, 8), (32, 96, 43690, 8), (32, 96, 43691, 4), (12, 96, 20000, 4),
                                                (6, 96, 40000, 6)])
def test_head_group(ops, nh, hd, T, head_group):
    """Literal values worked out by hand from the rule (one head's K + V^T: T * hd * 4 bytes; all heads while they fit 64 MiB, else 8
    heads while those fit 128 MiB, else 4; a head count the group does not divide stays whole): 5461 * 384 * 32 = 67,104,768 <= 64 MiB <
    5462 * 384 * 32; 43690 * 3072 = 134,215,680 <= 128 MiB < 43691 * 3072."""
    for past in (0, 1000):
        r = ops.attention_route(1, T - past, nh, nh, hd, past=past, past_t=(T + 63) // 64 * 64, new_is_cache=True, q_prescaled=True)
        assert r.status == 0 and r.head_group == head_group


def test_lds_bytes(ops):
    """Dynamic LDS per kernel, literal byte counts: k_attn_prefill two buffers of a padded K tile (64 rows of 2 hd + 16 bytes) and a padded
    V^T tile (hd rows of 144 bytes); dma two unpadded pairs (64 * hd * 2 + hd * 128); il rings of 3 + 3 tiles; pp rings of 4 K + 5 V^T tiles."""
    want = {"PREFILL": (54272, 36864), "DMA": (49152, 32768), "PP": (110592, 73728), "IL4": (73728, 49152), "IL8": (73728, 49152), "ATTN": (0, 0)}
    asks = {"PREFILL": dict(new_is_cache=False), "DMA": dict(attn_pp=0, attn_il=0), "PP": dict(attn_pp=1, attn_il=0),
            "IL4": dict(attn_il=1, attn_il_waves=4), "IL8": dict(attn_il=1, attn_il_waves=8), "ATTN": dict(attn_old=1)}
    for name, kw in asks.items():
        for hd, lds in zip((96, 64), want[name]):
            r = ops.attention_route(1, 300, 2, 2, hd, past_t=320, **dict(dict(new_is_cache=True, q_prescaled=True), **kw))
            assert (r.kernel, r.lds_bytes) == (getattr(ops.L, "ATTN_PK_" + name), lds), (name, hd)


def test_route_invariants(ops):
    """Over shapes x knob settings: a refused call launches nothing; grid x block covers the L queries of every (row, head) exactly;
    the merge launch goes with the split mode and nothing else; il never for plain Q; dma / pp / il only on a cache of whole tiles."""
    PK = {getattr(ops.L, "ATTN_PK_" + n): n for n in QUERIES_PER_WORKGROUP}
    shapes = itertools.product((0, 2), (0, 16, 17, 768, 6144), ((2, 2), (3, 2)), (96, 64, 80), (0, 40), (0, 4), (0, 1), (0, 1), (0, 1))
    knobs = [(0, 0) + k for k in itertools.product((-1, 0, 1), (-1, 0, 1), (-1, 4, 8))] + [(1, 0, -1, -1, -1), (0, 1, -1, -1, -1)]
    seen = set()
    for (B, L, (nh, nkv), hd, past, n_split, has_ws, cache, pre), (old, no_dma, pp, il, nw) in itertools.product(shapes, knobs):
        for past_t in ((past + L + 63) // 64 * 64, past + L + 8):
            r = ops.attention_route(B, L, nh, nkv, hd, past=past, past_t=past_t, n_split=n_split, new_is_cache=cache, q_prescaled=pre,
                                    has_ws=has_ws, attn_old=old, attn_no_dma=no_dma, attn_pp=pp, attn_il=il, attn_il_waves=nw)
            split = 0 < L <= 16 and n_split > 1
            want = -95 if hd == 80 else -22 if nh % nkv or (B and split and not has_ws) else 0
            assert r.status == want
            if r.status or B * L == 0:
                assert (r.kernel, list(r.grid), r.block, r.lds_bytes, r.merge, r.merge_grid, r.kernel_name, r.merge_name) == (-1, [0, 0, 0], 0, 0, 0, 0, b"", b"")
                continue
            name = PK[r.kernel]
            seen.add(name)
            per = QUERIES_PER_WORKGROUP[name]
            assert r.block == (256 if per <= 128 else 512)
            assert math.prod(r.grid) == B * nh * (n_split if split else -(-L // per))
            assert r.merge == int(split) and (name == "ATTN" if split else True)
            assert (r.merge_grid, r.merge_name) == ((B * nh * L, b"k_attn_combine2") if split else (0, b""))
            assert pre or name not in ("IL4", "IL8")
            assert (cache and past_t % 64 == 0) or name in ("ATTN", "PREFILL")
            assert (r.head_group > 0) == (name in ("DMA", "PP", "IL4", "IL8")) and (r.lds_bytes > 0) == (name != "ATTN")
    assert seen == set(QUERIES_PER_WORKGROUP)
