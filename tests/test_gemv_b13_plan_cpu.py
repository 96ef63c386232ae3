"""p3v_gemv_b13_plan: how the packed decode GEMV cuts a launch into waves -- the launcher's own arithmetic (gemv_stream_plan,
p3v_gemv3_body.h), checked without a GPU: every row pair is streamed by exactly one wave at every knob setting, and the decode
shapes get the wave counts the defaults were measured at."""
import numpy as np
import pytest

NS = (2, 3072, 4102, 6144, 8198, 9216, 16384, 32064)
KNOBS = ("gemv_b13_wpc", "gemv_b13_wpc_end", "gemv_wpw")


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


def owners(units, upw, waves, wpw):
    """how many waves take each row pair, by the kernel's own indexing: wave w < wpw of workgroup b owns
    [min(units, (b * wpw + w) * upw), + upw)"""
    count = np.zeros(units, dtype=np.int64)
    n_wg = -(-waves // wpw)
    for i in range(n_wg * wpw):
        lo = min(units, i * upw)
        count[lo:min(units, lo + upw)] += 1
    return count, n_wg


def test_default(ops):
    assert ops.set_tuning("gemv_b13_wpc", 16) == 16


@pytest.mark.parametrize("K", [3072, 8192])
def test_every_row_pair_has_one_wave(ops, K):
    for wpc in (1, 8, 12, 16):
        ops.set_tuning("gemv_b13_wpc", wpc)
        for n_cu in (64, 256, 304):
            for N in NS:
                for epi in (ops.EPI_NONE, ops.EPI_SILU_MUL):
                    units = N if epi == ops.EPI_SILU_MUL else N // 2
                    upw, waves, wpw, n_wg = ops.gemv_b13_plan(N, K, epi, n_cu)
                    what = (N, K, epi, n_cu, wpc, upw, waves, wpw, n_wg)
                    assert upw == max(1, -(-units // (n_cu * wpc))) and waves == -(-units // upw) and wpw in (3, 4), what
                    count, wgs = owners(units, upw, waves, wpw)
                    assert (count == 1).all() and wgs == n_wg and n_wg * wpw >= waves, what


def test_forced_workgroup_shape(ops):
    for forced in (3, 4):
        ops.set_tuning("gemv_wpw", forced)
        assert ops.gemv_b13_plan(9216, 3072, ops.EPI_NONE, 256)[2] == forced


def test_decode_shapes_at_the_default_knobs(ops):
    # gate_up (SiLU pairs), qkv, down, vocabulary head on 256 compute units: (row pairs per wave, waves, waves per workgroup, workgroups)
    got = [ops.gemv_b13_plan(N, K, epi, 256) for N, K, epi in ((8192, 3072, ops.EPI_SILU_MUL), (9216, 3072, ops.EPI_NONE),
                                                                (3072, 8192, ops.EPI_RESID_BF16), (32064, 3072, ops.EPI_NONE))]
    assert got == [(2, 4096, 4, 1024), (2, 2304, 3, 768), (1, 1536, 3, 512), (4, 4008, 4, 1002)]
    assert got[1][3] <= 1024                                  # the begin fold: P3V_GEMV_STEP_MAX_WG (include/p3v.h)
    assert ops.set_tuning("gemv_b13_wpc_end", 8) == 8         # the end fold (the vocabulary head inside a step) keeps 2004 waves
    ops.set_tuning("gemv_b13_wpc", 8)
    assert ops.gemv_b13_plan(32064, 3072, ops.EPI_NONE, 256) == (8, 2004, 4, 501)


def test_bad_arguments(ops):
    import ctypes as C
    lib, out = ops.L.lib(), (C.c_int32 * 4)()
    assert lib.p3v_gemv_b13_plan(3072, 3072, 0, 256, None) == -22
    assert lib.p3v_gemv_b13_plan(0, 3072, 0, 256, out) == -22 and lib.p3v_gemv_b13_plan(3072, 3072, 0, 0, out) == -22
    assert lib.p3v_gemv_b13_plan(3073, 3072, 0, 256, out) != 0 and lib.p3v_gemv_b13_plan(3072, 4096, 0, 256, out) != 0
