"""p3v_gemv_route against the launches recorded from a device (tests/golden/gemv_routes.json: kernel name, grid and block, or the
refusal code, of the cases of tools/gemv_routes.py, traced on the tree before the route existed), against p3v_gemv_b13_plan and against
its own invariants.  With a CU count given the route touches no device: no GPU here."""
import itertools
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = 256
NONE, BIAS, RESID, SILU, F32 = 0, 1, 5, 6, 8
FMTS = ("bf16", "fp8", "q4", "b13")
STEPS = {"none": 0, "begin": 1, "end": 2}
KNOBS = {"gemv_variant": (1, 3), "gemv_rows": (0, 1), "gemv8_min": (2, 5), "gemv_mfma8": (0, 1), "gemv_no_mfma": (0, 1), "gemv8_wgs": (64, 256),
         "gemv_wpc": (4, 8, 16), "gemv_wpw": (0, 3, 4), "gemv_no_mfma8": (0, 1), "gemv_f8_wpc": (8, 16), "gemv_q4_wpc": (4, 8),
         "gemv_q4_rows_wgs": (64, 256), "gemv_q4_rows8": (0, 1), "gemv_b13_wpc": (8, 16), "gemv_b13_wpc_end": (8, 16), "gemv_b13_xscale": (0, 1)}


@pytest.fixture()
def ops():
    from phi_3_vision_mlx_amd import ops as o
    o.L.lib()
    saved = {k: o.set_tuning(k, 0) for k in KNOBS}
    for k, v in saved.items():
        o.set_tuning(k, v)
    try:
        yield o
    finally:
        for k, v in saved.items():
            o.set_tuning(k, v)


def test_recorded_launches_are_the_route(ops):
    """Every case of the device recording: with the recorded CU count the route names the kernel, grid and block that ran and refuses
    what was refused, with the code the entry returned."""
    with open(os.path.join(ROOT, "tests", "golden", "gemv_routes.json")) as f:
        rows = json.load(f)
    cus = rows[0][1]["cu_count"]
    cases = [c for kind, c in rows if kind == "case"]
    assert rows[0][0] == "device" and len(cases) >= 120
    kernels = set()
    for c in cases:
        old = [(name, ops.set_tuning(name, v)) for name, v in c["knobs"].items()]
        try:
            r = ops.gemv_route(c["M"], c["N"], c["K"], c["epilogue"], fmt=c["fmt"], step=STEPS[c["step"]], has_norm=c["has_norm"],
                               exp_base=c["exp_base"], cu_count=cus)
        finally:
            for name, v in old:
                ops.set_tuning(name, v)
        assert r.status == c["status"], c["id"]
        assert ([[r.name.decode(), [r.grid, 1, 1], [r.block, 1, 1]]] if r.status == 0 else []) == c["launches"], c["id"]
        kernels.add(r.kernel)
    assert kernels == set(range(ops.L.GEMV_K_ROWS_Q4 + 1))        # every kernel family, and the refusals


def test_b13_plan_is_a_projection_of_the_route(ops):
    """p3v_gemv_b13_plan over the grid of tests/test_gemv_b13_plan_cpu.py."""
    import test_gemv_b13_plan_cpu as plan
    for wpc, wpw in itertools.product((1, 8, 12, 16), (0, 3, 4)):
        ops.set_tuning("gemv_b13_wpc", wpc), ops.set_tuning("gemv_wpw", wpw)
        for K, n_cu, N, epi in itertools.product((3072, 8192), (64, 256, 304), plan.NS, (NONE, SILU)):
            r = ops.gemv_route(1, N, K, epi, fmt="b13", exp_base=97, cu_count=n_cu)
            assert r.status == 0 and ops.gemv_b13_plan(N, K, epi, n_cu) == (r.upw, r.waves, r.wpw, r.grid), (wpc, wpw, K, n_cu, N, epi)


def grid():
    for fmt, M, N, K, epi in itertools.product(FMTS, (0, 1, 2, 4, 5, 8, 9, 16, 17), (16, 24, 100, 101, 272, 6200, 9216),
                                                (520, 1024, 3072, 4096, 8192, 10232), (NONE, BIAS, RESID, SILU, F32)):
        yield fmt, M, N, K, epi


def check(ops, L, fmt, M, N, K, epi, norm, base, what):
    r = ops.gemv_route(M, N, K, epi, fmt=fmt, has_norm=norm, exp_base=base, cu_count=CUS)
    assert (r.status != 0) == (r.kernel == L.GEMV_K_NONE) and r.status in (0, -22, -95), what
    assert bool(r.late) <= (r.status != 0), what
    if r.status == 0:
        assert r.grid >= 1 and r.block in (256, 512) and r.name, what
        # the LDS a launch asks for fits the limit the launcher sets: the raised cap, or the 64 KB every kernel has
        assert r.lds_bytes <= (r.lds_cap or 64 * 1024) and r.lds_cap in (0, 160 * 1024 - 256, 160 * 1024 - 512, 160 * 1024 - 8704), what
    if r.kernel == L.GEMV_K_GEMV3:
        units = N if epi == SILU else (N + 1) // 2
        assert r.grid * r.wpw >= r.waves and r.waves * r.upw >= units > (r.waves - 1) * r.upw and r.wpw in (3, 4), what
        assert r.NST * r.CH * 64 * (16 if fmt in ("fp8", "q4") else 8) == K, what
    if r.kernel in (L.GEMV_K_MFMA8, L.GEMV_K_GEMV8_Q4, L.GEMV_K_ROWS_Q4):
        assert r.n_sets == -(-N // (8 if epi == SILU else 16)) and r.grid * r.sets_per_wg >= r.n_sets > (r.grid - 1) * r.sets_per_wg, what
        assert r.NW * r.NST * 256 == K and r.block == 64 * r.NW, what
    if r.kernel == L.GEMV_K_GEMV:
        assert r.grid <= 2048 and r.MT >= M and r.lds_bytes == r.MT * K * 2, what
    one = r if (M, epi) == (1, NONE) else ops.gemv_route(1, N, K, NONE, fmt=fmt, has_norm=norm, exp_base=base, cu_count=CUS)
    for step in (L.GEMV_STEP_BEGIN, L.GEMV_STEP_END):
        s = ops.gemv_route(M, N, K, epi, fmt=fmt, step=step, has_norm=norm, exp_base=base, cu_count=CUS)
        assert (s.status != 0) == (s.kernel == L.GEMV_K_NONE), what
        if s.status == 0:                                         # a fold only where the plain entry streams that one row, and the same kernel
            assert (M, epi) == (1, NONE) and one.kernel == s.kernel == L.GEMV_K_GEMV3, what
            assert (s.MT, s.NST, s.CH, s.scaled) == (1, one.NST, one.CH, one.scaled) and s.grid <= 1024 and s.lds_cap == 0, what
        elif (M, epi) == (1, NONE) and one.kernel == L.GEMV_K_GEMV3:
            assert s.status == -95 and s.late == 1, what          # ... and there only a plan the fold's workspace does not hold is refused


def test_route_invariants(ops):
    L = ops.L
    for fmt, M, N, K, epi in grid():
        check(ops, L, fmt, M, N, K, epi, False, 97, (fmt, M, N, K, epi))
    for knob, values in KNOBS.items():                            # each knob at each of its values, the others at their defaults
        for v in values:
            old = ops.set_tuning(knob, v)
            try:
                for fmt, M, N, K, epi in grid():
                    if K in (1024, 3072, 8192) and N in (24, 101, 272, 9216) and epi in (NONE, SILU, F32):
                        for norm, base in ((False, 97), (True, 98)):
                            check(ops, L, fmt, M, N, K, epi, norm, base, (knob, v, fmt, M, N, K, epi, norm, base))
            finally:
                ops.set_tuning(knob, old)


def test_route_rules(ops):
    """What the recording does not hold: the side of k_gemv's LDS limit that is refused, the order of the refusal codes, a device's
    own CU count left alone where no plan is asked for."""
    L = ops.L
    assert ops.gemv_route(8, 16, 10224, cu_count=CUS).kernel == L.GEMV_K_GEMV and ops.gemv_route(8, 16, 10232, cu_count=CUS).status == -95
    assert ops.gemv_route(8, 16, 3072).name == b"k_gemv_mfma8<false, 4, 3>"                  # (no cu_count, no device: no plan in this route)
    # bf16: shape (ARG), epilogue (UNSUPPORTED), a missing residual (ARG), no kernel (UNSUPPORTED)
    assert ops.gemv_route(17, 16, 3072, BIAS, cu_count=CUS).status == -22 and ops.gemv_route(9, 16, 520, BIAS, cu_count=CUS).status == -95
    assert ops.gemv_route(9, 16, 520, RESID, has_resid=False, cu_count=CUS).status == -22 and ops.gemv_route(9, 16, 520, RESID, cu_count=CUS).status == -95
    # e4m3: shape and epilogue (UNSUPPORTED) before the missing residual
    assert ops.gemv_route(17, 16, 3072, RESID, fmt="fp8", has_resid=False, cu_count=CUS).status == -95
    assert ops.gemv_route(16, 16, 3072, RESID, fmt="fp8", has_resid=False, cu_count=CUS).status == -22
    # 4-bit: N % 16 (UNSUPPORTED), the missing residual (ARG), then -- after the entry's alignment checks -- the norm no rows kernel takes
    assert ops.gemv_route(2, 24, 3072, RESID, fmt="q4", has_resid=False, cu_count=CUS).status == -95
    assert ops.gemv_route(2, 32, 3072, RESID, fmt="q4", has_resid=False, cu_count=CUS).status == -22
    old = ops.set_tuning("gemv_q4_rows8", 0)
    try:
        r = ops.gemv_route(2, 32, 3072, fmt="q4", has_norm=True, cu_count=CUS)
        assert (r.status, r.late) == (-95, 1) and ops.gemv_route(2, 32, 3072, RESID, fmt="q4", has_norm=True, has_resid=False, cu_count=CUS).status == -22
    finally:
        ops.set_tuning("gemv_q4_rows8", old)
    # 13-bit codes: epilogue, residual, rows <= 0 (ARG), shape (UNSUPPORTED), exponent base (ARG)
    assert ops.gemv_route(0, 16, 3072, BIAS, fmt="b13", exp_base=97, cu_count=CUS).status == -95
    assert ops.gemv_route(0, 16, 3072, fmt="b13", exp_base=97, cu_count=CUS).status == -22
    assert ops.gemv_route(2, 16, 3072, fmt="b13", exp_base=0, cu_count=CUS).status == -95 and ops.gemv_route(1, 16, 3072, fmt="b13", exp_base=0, cu_count=CUS).status == -22
    # a step: rows <= 0 (ARG) before everything the caller keeps as separate launches (UNSUPPORTED)
    assert ops.gemv_route(0, 16, 4096, step=L.GEMV_STEP_END, cu_count=CUS).status == -22 and ops.gemv_route(1, 16, 4096, step=L.GEMV_STEP_END, cu_count=CUS).status == -95
    assert ops.gemv_route(1, 4102, 3072, fmt="b13", step=L.GEMV_STEP_END, exp_base=97, cu_count=CUS).name == b"k_gemv3_step<GemvB13<true>, 1, 1, 6, 2>"
    with pytest.raises(RuntimeError):
        ops.L.check(ops.L.lib().p3v_gemv_route(None, None), "gemv_route")
