"""The bf16 projection kernels -- behind p3v_gemm: k_gemm alone and as split-K partials with k_splitk_reduce, the 256 x 256 kernel,
k_gemm_skinny (64- and 128-row tiles, one pass or K slices, k_splitk_reduce_norm through p3v_gemm_resid_norm), k_gemm_rows; behind
p3v_gemv: k_gemv<MT>, the K = 3072 / 8192 streaming body at 1, 2 and 4 rows, k_gemv_mfma, k_gemv_mfma8 -- against plain fp64 on the
two input families of tests/proj_probe.py, under its acceptance rules: on the exact-sum grid every output IS the fp64 value pushed
through the roundings of include/p3v.h (fp32 outputs equal as floats), everywhere else the rounding bracket, every element;
operands inside padded buffers that hold 2^15, outputs inside guarded buffers that must come back bit-identical outside [M, N].
The path is pinned with the launch-policy knobs and, where a planning query exists, asserted.  tests/test_proj_probe_cpu.py shows on
the references alone that a kernel with a dropped k, a truncating store, a missed rounding, 16-bit partials, ... cannot pass here."""
import ctypes as C

import pytest
import torch

import proj_probe as pp

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
    with pp.pinned(ops, case):
        return call()


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _report(case, family, pr, flat, extra=""):
    msg = pr.verify(flat)
    print(f"{case.id} [{pr.label}]: {case.kernel}: {msg or _used(pp.needed_scale(lambda s: pr.verify(flat, s))) + ', nothing outside [M, N] touched'}{extra}")
    return msg


@pytest.mark.parametrize("family", pp.FAMILIES)
@pytest.mark.parametrize("case", pp.GEMM_CASES, ids=ids)
def test_gemm_against_fp64(ops, case, family):
    pr = pp.probe(case, family)
    L, lib, stream = ops.L, ops.L.lib(), torch.cuda.current_stream().cuda_stream
    a_buf, w_buf = (t.cuda() for t in pr.operand_buffers())
    out = pr.out_buffer().cuda()
    res = pr.resid_buffer()
    res = out if pr.inplace else None if res is None else res.cuda()
    bias = None if pr.bias is None else pr.bias.cuda()
    pos = None if pr.pos is None else pr.pos.cuda()
    esz = out.element_size()
    o_ptr = out.data_ptr() + pp.GUARD * esz
    r_ptr = 0 if res is None else res.data_ptr() + pp.GUARD * esz

    def call():
        if case.rows_slices >= 0:
            assert lib.p3v_gemm_rows_slices(case.M, case.N, case.K, case.epi) == case.rows_slices
        ws_bytes = lib.p3v_gemm_ws_bytes(case.M, case.N, case.K, case.epi)
        if case.slices >= 0:                                               # the plan the case is meant to hit
            want = 0 if case.slices == 1 else case.slices * case.M * case.w_rows * 4
            assert ws_bytes == want, f"p3v_gemm_ws_bytes says {ws_bytes}, the case is built for {case.slices} slices ({want})"
        ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device="cuda")
        args = L.GemmArgs(a_buf.data_ptr(), w_buf.data_ptr(), o_ptr, _ptr(bias), r_ptr, _ptr(pos), case.M, case.N, case.K, pr.lda, pr.ldw,
                          pr.ldo, case.epi, case.P, ws.data_ptr() if ws_bytes else 0, ws_bytes)
        if not case.norm:
            L.check(lib.p3v_gemm(C.byref(args), stream), "gemm")
            return None
        normed = torch.full((case.M, case.N), 777.0, dtype=pp.BF16, device="cuda")
        L.check(lib.p3v_gemm_resid_norm(C.byref(args), pr.norm_w.cuda().data_ptr(), pp.EPS, normed.data_ptr(), stream), "gemm_resid_norm")
        return normed

    normed = _pinned(ops, case, call)
    flat = out.cpu()
    extra, msg2 = "", ""
    if normed is not None:
        got, nrm = pr.window_get(flat), normed.cpu()
        msg2 = pr.verify_normed(got, nrm)
        extra = "; normed: " + (msg2 or _used(pp.needed_scale(lambda s: pr.verify_normed(got, nrm, s))))
    msg = _report(case, family, pr, flat, extra)
    assert msg == "", msg
    assert msg2 == "", msg2
    a_ref, w_ref = pr.operand_buffers()                                    # the operands (and a separate residual) are left alone
    assert torch.equal(a_buf.cpu().view(torch.int16), a_ref.view(torch.int16)) and torch.equal(w_buf.cpu().view(torch.int16), w_ref.view(torch.int16))
    if res is not None and not pr.inplace:
        assert torch.equal(res.cpu(), pr.resid_buffer())


@pytest.mark.parametrize("family", pp.FAMILIES)
@pytest.mark.parametrize("case", pp.GEMV_CASES, ids=ids)
def test_gemv_against_fp64(ops, case, family):
    pr = pp.probe(case, family)
    L, lib, stream = ops.L, ops.L.lib(), torch.cuda.current_stream().cuda_stream
    x, w = pr.A.cuda(), pr.W.cuda()
    out = pr.out_buffer().cuda()
    res = pr.resid_buffer()
    res = out if pr.inplace else None if res is None else res.cuda()
    norm_w = None if pr.norm_w is None else pr.norm_w.cuda()
    esz = out.element_size()
    args = L.GemvArgs(x.data_ptr(), w.data_ptr(), out.data_ptr() + pp.GUARD * esz, 0 if res is None else res.data_ptr() + pp.GUARD * esz,
                      _ptr(norm_w), pp.EPS if case.norm else 0.0, case.M, case.N, case.K, case.epi)
    _pinned(ops, case, lambda: L.check(lib.p3v_gemv(C.byref(args), stream), "gemv"))
    msg = _report(case, family, pr, out.cpu())
    assert msg == "", msg
    assert torch.equal(x.cpu().view(torch.int16), pr.A.view(torch.int16)) and torch.equal(w.cpu().view(torch.int16), pr.W.view(torch.int16))
    if res is not None and not pr.inplace:
        assert torch.equal(res.cpu(), pr.resid_buffer())
