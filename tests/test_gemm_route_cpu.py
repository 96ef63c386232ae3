"""p3v_gemm_route against the launches recorded from a device (tests/golden/gemm_routes.json: kernel names, grids and blocks of the
cases of tools/gemm_routes.py, traced on the tree before the route existed), against the recorded host queries (tests/golden/gemm_plans.json: p3v_gemm_ws_bytes and p3v_gemm_rows_slices over a grid
of shapes, epilogues and knob settings, written by tests/golden/gen_golden_gemm_plans.py on the tree before the route existed) and
against its own invariants.  With a CU count given the route touches no device: no GPU here.

Two findings of the recording, kept as they were (neither is a shape the model runs):
  * a SiLU projection with 9 .. 32 rows whose rows rule says 4 slices (M = 16, N = 1024, K = 3072) is answered with a four-slice
    workspace by p3v_gemm_ws_bytes, but no rows kernel splits a SiLU shape: with that workspace it runs in ONE pass on the 64-row tiles;
  * where the rows rule says 4 slices and the 64-row tiles' own rule fewer (M = 16, N = 8192, K = 8192: 2), a workspace of
    ws_bytes - 16 does not give the one-pass form but the tiles' smaller split, which fits it.
`test_short_workspace` asserts the one-pass form everywhere else and exactly that second split there; `test_route_invariants` asserts
"ws_bytes > 0 iff S > 1" everywhere but at the first."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
CUS = 256
SILU = 6


@pytest.fixture(scope="module")
def plans():
    import gen_golden_gemm_plans as gen
    with open(gen.PATH) as f:
        text = f.read()
    rec = {"cases": {}}
    for row in json.loads(text):
        if row[0] == "case":
            rec["cases"][row[1]] = row[2]
        else:
            rec[row[0]] = row[1]
    return gen, text, rec


@pytest.fixture(scope="module")
def routes(plans):
    """(variant, M, N, K, epilogue, recorded [S, rows_slices], route with every workspace, route with none) for every grid row."""
    from phi_3_vision_mlx_amd import ops
    gen, _, rec = plans
    out = []
    for v in gen.VARIANTS:
        old = ops.set_tuning(*v) if v else None
        try:
            for (M, N, K, epi), sym in zip(gen.grid(), rec["cases"][gen.variant_name(v)]):
                out.append((v, M, N, K, epi, rec["outcomes"][sym], ops.gemm_route(M, N, K, epi, ws_bytes=1 << 62, cu_count=CUS),
                            ops.gemm_route(M, N, K, epi, cu_count=CUS)))
        finally:
            if v:
                ops.set_tuning(v[0], old)
    return out


def launches(r):
    return [r.launch[i] for i in range(r.n_launches)]


def test_recorded_launches_are_the_route():
    """Every case of the device recording: with the recorded CU count the route names the kernels, grids and blocks that ran, in order,
    and refuses what was refused."""
    from phi_3_vision_mlx_amd import ops
    with open(os.path.join(ROOT, "tests", "golden", "gemm_routes.json")) as f:
        rows = json.load(f)
    cus = rows[0][1]["cu_count"]
    cases = [c for kind, c in rows if kind == "case"]
    assert rows[0][0] == "device" and len(cases) >= 90
    entries = {"gemm": ops.L.GEMM_ENTRY_GEMM, "resid_norm": ops.L.GEMM_ENTRY_RESID_NORM, "qkv": ops.L.GEMM_ENTRY_QKV}
    for c in cases:
        old = [(name, ops.set_tuning(name, v)) for name, v in {"gemm_big_rows": -1, **c["knobs"]}.items()]   # (the suite pins 512 rows; the
        # recording ran on the library's own settings: the cost model)
        try:
            M, N, K, epi = c["M"], c["N"], c["K"], c["epilogue"]
            ws = ops.L.lib().p3v_gemm_ws_bytes(M, N, K, epi) if c["ws"] else 0
            r = ops.gemm_route(M, N, K, epi, entry=entries[c["entry"]], has_bias=epi in (1, 2, 3, 4, 7), ws_bytes=ws, n_heads=c.get("n_heads", 0),
                               n_kv=c.get("n_kv", 0), hd=c.get("hd", 0), dst_off=c.get("dst_off", 0), dst_t=c.get("dst_t", 0), cu_count=cus)
        finally:
            for name, v in old:
                ops.set_tuning(name, v)
        assert r.status == c["status"], c["id"]
        assert [[l.name.decode(), list(l.grid), [l.block, 1, 1]] for l in launches(r)] == c["launches"], c["id"]


def test_recording_is_reproduced_byte_for_byte(plans):
    gen, text, rec = plans
    assert gen.dumps(gen.record()) == text
    assert len(rec["cases"]) == len(gen.VARIANTS) and all(len(c) == 18 * 9 * 7 * 9 for c in rec["cases"].values())
    assert sorted(rec["outcomes"].values()) == [[1, 0], [1, 1], [2, 0], [4, 0], [4, 4], [8, 0]]


def test_queries_are_projections_of_the_route(routes):
    for v, M, N, K, epi, (S, rs), r, r0 in routes:                # (p3v_gemm_rows_slices: the recording's regeneration above)
        unit = M * (2 * N if epi == SILU else N) * 4
        assert r.ws_bytes == r0.ws_bytes == (S * unit if S > 1 else 0), (v, M, N, K, epi)


def test_route_invariants(routes):
    from phi_3_vision_mlx_amd import ops
    K_ = ops.L
    reduces = (K_.GEMM_K_REDUCE, K_.GEMM_K_REDUCE_NORM)
    for v, M, N, K, epi, (_, rs), r, r0 in routes:
        assert (r.ws_bytes > 0) == (r.S > 1) or (epi == SILU and rs > 1 and r.S == 1), (v, M, N, K, epi)      # (the first finding)
        for x in (r, r0):
            case = (v, M, N, K, epi)
            assert x.status in (0, K_.ERR_UNSUPPORTED) and (x.status == 0 or x.n_launches == 0), case
            if x.status:
                continue
            ls = launches(x)
            gemms = [l for l in ls if l.kernel not in reduces]
            row = 0
            for l in gemms:                                       # the GEMM launches tile [0, M) exactly once, in order
                assert l.row0 == row and l.rows > 0 and l.name, case
                row += l.rows
            assert row == M, case
            assert len(ls) - len(gemms) == (x.S > 1) and all(l.grid[2] == x.S for l in gemms if l.kernel != K_.GEMM_K_ROWS), case
            if x.S > 1:                                           # a split: one GEMM launch + the reduction of all its rows, last
                assert len(ls) == 2 and ls[1].kernel == K_.GEMM_K_REDUCE and (ls[1].row0, ls[1].rows) == (0, M), case
        assert r.ws_short == 0 and r0.ws_short == (r0.ws_bytes > 0) and r0.S == 1, (v, M, N, K, epi)


def test_short_workspace(routes):
    """ws_bytes - 16 offered: p3v_gemm_ws_bytes (the route's ws_bytes) is unchanged and the route is the one-pass form -- the route
    of no workspace at all.  The exception is the second finding above: the 64-row tiles' own, smaller split where it fits."""
    from phi_3_vision_mlx_amd import ops
    second = 0
    for v, M, N, K, epi, (_, rs), r, r0 in routes:
        if r.ws_bytes == 0 or v and v[0] not in ("gemm_skinny_s", "gemm_no_skinny", "gemm_no_splitk"):
            continue                                              # (the other knobs change no split: the default rows cover them)
        old = ops.set_tuning(*v) if v else None
        try:
            short = ops.gemm_route(M, N, K, epi, ws_bytes=r.ws_bytes - 16, cu_count=CUS)
            no_rows = ops.set_tuning("gemm_rows", 0)                # the tiles' own rule: the route of every workspace without the rows kernel
            try:
                own = ops.gemm_route(M, N, K, epi, ws_bytes=1 << 62, cu_count=CUS)
            finally:
                ops.set_tuning("gemm_rows", no_rows)
        finally:
            if v:
                ops.set_tuning(v[0], old)
        case = (v, M, N, K, epi)
        assert short.ws_bytes == r.ws_bytes and short.ws_short == 1 and short.status == 0, case
        if short.S == 1:
            assert [(l.name, list(l.grid)) for l in launches(short)] == [(l.name, list(l.grid)) for l in launches(r0)], case
        else:
            second += 1
            assert rs > 1 and 1 < short.S == own.S < rs and own.ws_bytes <= r.ws_bytes - 16, case
            assert [(l.name, list(l.grid)) for l in launches(short)] == [(l.name, list(l.grid)) for l in launches(own)], case
    assert second > 0


def test_route_rules():
    """What the grid does not separate: a bias keeps a call off the weight-streaming kernels, the 32-bit-offset bound, the persistent
    256 x 256 grid's CU count, the qkv and resid_norm entries."""
    from phi_3_vision_mlx_amd import ops
    K_ = ops.L
    big = 1 << 62
    model_rows = ops.set_tuning("gemm_big_rows", -1)              # (the suite pins 512 rows: the cost model here)
    try:
        r = ops.gemm_route(128, 3072, 8192, 0, has_bias=True, ws_bytes=big, cu_count=CUS)
        assert [l.name for l in launches(r)] == [b"k_gemm<8, 0>", b"k_splitk_reduce<0>"] and r.S == 8
        assert ops.gemm_route(16, 3072, 8192, 5, ldw=1 << 20, cu_count=CUS).status == K_.ERR_UNSUPPORTED
        r = ops.gemm_route(2531, 8192, 3072, SILU, cu_count=CUS)
        assert [(l.name, list(l.grid), l.block, l.row0, l.rows) for l in launches(r)] == [(b"k_gemm256<6, 80, 2>", [256, 1, 1], 512, 0, 2048),
                                                                                            (b"k_gemm<6, 0>", [128, 4, 1], 256, 2048, 483)]
        assert launches(ops.gemm_route(2531, 8192, 3072, SILU, cu_count=100))[0].grid[0] == 96
        r = ops.gemm_route(16, 1024, 3072, SILU, ws_bytes=big, cu_count=CUS)      # the first finding
        assert r.ws_bytes == 4 * 16 * 2048 * 4 and r.S == 1 and [l.name for l in launches(r)] == [b"k_gemm_skinny<6, false, 64, 64>"]
        r = ops.gemm_route(17, 3072, 3072, 5, entry=K_.GEMM_ENTRY_RESID_NORM, ws_bytes=big)
        assert [l.name for l in launches(r)] == [b"k_gemm_rows<false, 3, 1, 2, true>", b"k_splitk_reduce_norm"] and launches(r)[1].grid[0] == 17
        for kw in (dict(M=300), dict(N=4096), dict(ws_bytes=0), dict(has_bias=True)):
            q = dict(M=17, N=3072, K=3072, epilogue=5, entry=K_.GEMM_ENTRY_RESID_NORM, ws_bytes=big)
            q.update(kw)
            assert ops.gemm_route(**q).status == K_.ERR_UNSUPPORTED, kw
        qkv = dict(N=9216, K=256, entry=K_.GEMM_ENTRY_QKV, n_heads=32, n_kv=32, hd=96, dst_t=2560, cu_count=CUS)
        assert [l.name for l in launches(ops.gemm_route(M=128, **qkv))] == [b"k_gemm_skinny<100, false, 64, 128>"]
        assert ops.gemm_route(M=300, **qkv).status == K_.ERR_UNSUPPORTED and ops.gemm_route(M=128, dst_off=4, **qkv).status == K_.ERR_UNSUPPORTED
        old = ops.set_tuning("gemm_big_rows", 1024)
        try:
            r = ops.gemm_route(M=1300, **qkv)
            assert [(l.name, l.row0, l.rows) for l in launches(r)] == [(b"k_gemm256<100, 80, 2>", 0, 1024), (b"k_gemm<100, 0>", 1024, 276)]
            r = ops.gemm_route(M=1300, **dict(qkv, N=1152, n_heads=4, n_kv=4))     # 384-column regions: whole 128-column tiles only
            assert [l.name for l in launches(r)] == [b"k_gemm<100, 0>"]
        finally:
            ops.set_tuning("gemm_big_rows", old)
    finally:
        ops.set_tuning("gemm_big_rows", model_rows)
    with pytest.raises(RuntimeError):                            # P3V_ERR_ARG, the shape checks: N is not (n_heads + 2 n_kv) * hd ...
        ops.gemm_route(128, 9216, 256, 0, entry=K_.GEMM_ENTRY_QKV, n_heads=32, n_kv=32, hd=64)
    with pytest.raises(RuntimeError):                            # ... and K is no multiple of 64
        ops.gemm_route(128, 3072, 100, 0, cu_count=CUS)
