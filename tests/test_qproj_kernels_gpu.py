"""The quantised projection kernels -- behind p3v_gemv_fp8: the e4m3 policy of the K = 3072 / 8192 streaming body, k_gemv_mfma_f8,
k_gemv_mfma8_f8; behind p3v_gemv_q4: the 4-bit policy of the streaming body, k_gemv8_q4, k_gemm_rows_q4; behind p3v_gemm_fp8:
k_gemm256_f8 with its wide and its narrow tile -- against plain fp64 on the input families of tests/qproj_probe.py, under the
acceptance rules of tests/proj_probe.py: on the exact-sum grid every output IS the fp64 value pushed through the roundings of
include/p3v.h (fp32 outputs equal as floats), everywhere else the rounding bracket, every element; outputs inside guarded buffers that
must come back bit-identical outside [M, N], the W8A8 operands inside padded buffers that hold 448, every operand untouched.  The path
is pinned with the launch-policy knobs of the case table.  tests/test_qproj_probe_cpu.py shows on the references alone that a kernel
with a dropped k, a neighbouring group's scale, swapped nibbles, an 8-bit dequantisation, a truncating store, ... cannot pass here."""
import ctypes as C

import pytest
import torch

import qproj_probe as qp

pytestmark = pytest.mark.gpu

ids = lambda c: c.id


@pytest.fixture(scope="module")
def ops():
    from phi_3_vision_mlx_amd import ops as o
    o.L.lib()
    return o


def _used(s):
    """For the record, not asserted: the smallest of the scales x E under which the rule still accepts the kernel's output."""
    return "outside E" if s is None else "bit-exact against the rounded fp64 reference" if s == 0 else f"inside its brackets at {s:g} x E"


def _pinned(ops, case, call):
    with qp.pinned(ops, case):
        return call()


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _report(case, pr, flat):
    msg = pr.verify(flat)
    print(f"{case.id} [{pr.label}]: {case.kernel}: {msg or _used(qp.needed_scale(lambda s: pr.verify(flat, s))) + ', nothing outside [M, N] touched'}")
    return msg


def _same_bits(dev, host):
    it = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[host.element_size()]
    return torch.equal(dev.cpu().contiguous().view(it), host.contiguous().view(it))


@pytest.mark.parametrize("family", qp.FAMILIES)
@pytest.mark.parametrize("case", qp.GEMV_CASES, ids=ids)
def test_gemv_against_fp64(ops, case, family):
    pr = qp.probe(case, family)
    L, lib, stream = ops.L, ops.L.lib(), torch.cuda.current_stream().cuda_stream
    host = (pr.A, pr.W8, pr.wscale) if case.fmt == "f8" else (pr.A, pr.W4, pr.SB)
    x, w, s = (t.cuda() for t in host)
    out = pr.out_buffer().cuda()
    res = pr.resid_buffer()
    res = out if pr.inplace else None if res is None else res.cuda()
    norm_w = None if pr.norm_w is None else pr.norm_w.cuda()
    esz = out.element_size()
    cls, fn, name = (L.GemvF8Args, lib.p3v_gemv_fp8, "gemv_fp8") if case.fmt == "f8" else (L.GemvQ4Args, lib.p3v_gemv_q4, "gemv_q4")
    args = cls(x.data_ptr(), w.data_ptr(), s.data_ptr(), out.data_ptr() + qp.GUARD * esz, 0 if res is None else res.data_ptr() + qp.GUARD * esz,
               _ptr(norm_w), qp.EPS if case.norm else 0.0, case.M, case.N, case.K, case.epi)
    _pinned(ops, case, lambda: L.check(fn(C.byref(args), stream), name))
    msg = _report(case, pr, out.cpu())
    assert msg == "", msg
    assert all(_same_bits(d, h) for d, h in zip((x, w, s), host))               # the operands (and a separate residual) are left alone
    assert norm_w is None or _same_bits(norm_w, pr.norm_w)
    if res is not None and not pr.inplace:
        assert torch.equal(res.cpu(), pr.resid_buffer())


@pytest.mark.parametrize("family", qp.FAMILIES)
@pytest.mark.parametrize("case", qp.GEMM_CASES, ids=ids)
def test_gemm_fp8_against_fp64(ops, case, family):
    pr = qp.probe(case, family)
    L, lib, stream = ops.L, ops.L.lib(), torch.cuda.current_stream().cuda_stream
    a_ref, w_ref = pr.operand_buffers()
    a_buf, w_buf, sa, sw = (t.cuda() for t in (a_ref, w_ref, pr.sa, pr.wscale))
    out = pr.out_buffer().cuda()
    res = pr.resid_buffer()
    res = out if pr.inplace else None if res is None else res.cuda()
    esz = out.element_size()
    args = L.GemmF8Args(a_buf.data_ptr(), sa.data_ptr(), w_buf.data_ptr(), sw.data_ptr(), out.data_ptr() + qp.GUARD * esz,
                        0 if res is None else res.data_ptr() + qp.GUARD * esz, case.M, case.N, case.K, pr.lda, pr.ldw, pr.ldo, case.epi)
    _pinned(ops, case, lambda: L.check(lib.p3v_gemm_fp8(C.byref(args), stream), "gemm_fp8"))
    msg = _report(case, pr, out.cpu())
    assert msg == "", msg
    assert all(_same_bits(d, h) for d, h in zip((a_buf, w_buf, sa, sw), (a_ref, w_ref, pr.sa, pr.wscale)))
    if res is not None and not pr.inplace:
        assert torch.equal(res.cpu(), pr.resid_buffer())
