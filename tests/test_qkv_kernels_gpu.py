"""p3v_gemm_qkv -- the qkv projection with the head split, the rotation and the KV append in its epilogue, as k_gemm_skinny<QKV>,
k_gemm<QKV> and k_gemm256<QKV> run it -- against plain fp64 on the two input families of tests/qkv_probe.py, under its acceptance rules:
V^T bit-equal to the exact sums on GRID and inside the accumulator bracket on SPIKES, rotated Q / K inside RopeProbe's bracket around
the fp64 rotation, every element; operands inside padded buffers that hold 2^15, destinations inside guarded sentinel buffers that must
come back bit-identical outside the windows.  The kernel is pinned with the launch-policy knobs and asserted through ops.gemm_route.
Then the header's contract on the same inputs: p3v_gemm + p3v_rope_kv_append into a second set of buffers, bit-identical.
tests/test_qkv_probe_cpu.py shows on the references alone that a kernel with a wrong pair partner, a wrong position, a dropped
m_base, a V^T run that wraps a batch row only once, ... cannot pass here."""
import ctypes as C

import pytest
import torch

import qkv_probe as qp

pytestmark = pytest.mark.gpu

ids = lambda c: c.id
EPI_NONE, EPI_BIAS = 0, 1
ERR_ARG = -22                           # P3V_ERR_ARG (include/p3v.h)


@pytest.fixture(scope="module")
def ops():
    from phi_3_vision_mlx_amd import ops as o
    o.L.lib()
    return o


def _used(s):
    """For the record, not asserted: the smallest of the scales x E under which the rule still accepts the kernel's output."""
    return "outside E" if s is None else "bit-exact against the rounded fp64 reference" if s == 0 else f"inside its brackets at {s:g} x E"


def _pinned(ops, knobs, call):
    old = []
    try:
        for name, value in knobs:
            old.append((name, ops.set_tuning(name, value)))
        return call()
    finally:
        for name, value in reversed(old):
            ops.set_tuning(name, value)


def _ptr(t, skip=0):
    return 0 if t is None else t.data_ptr() + skip * t.element_size()


def _split(L, case, cos, sin, flat):
    return L.QkvSplit(_ptr(cos), _ptr(sin), _ptr(flat["q"], qp.GUARD), _ptr(flat["k"], qp.GUARD), _ptr(flat["v"], qp.GUARD), case.B, case.L,
                      case.nh, case.nkv, case.hd, case.past, case.dst_t, int(case.off_is_past), case.tab_t, case.tab_div, case.q_scale)


@pytest.mark.parametrize("family", qp.FAMILIES)
@pytest.mark.parametrize("case", qp.CASES, ids=ids)
def test_gemm_qkv_against_fp64(ops, case, family):
    pr = qp.probe(case, family)
    L, lib, stream = ops.L, ops.L.lib(), torch.cuda.current_stream().cuda_stream
    a_buf, w_buf = (t.cuda() for t in pr.operand_buffers())
    bias = None if pr.lin.bias is None else pr.lin.bias.cuda()
    cos, sin = (None, None) if case.null else (pr.cos.cuda(), pr.sin.cuda())
    fused = {n: f.cuda() for n, f in pr.buffers().items()}
    two = {n: f.cuda() for n, f in pr.buffers().items()}
    scratch = torch.empty((case.M, case.N), dtype=qp.BF16, device="cuda")
    epi = EPI_BIAS if case.bias else EPI_NONE

    def call():
        route = qp.check_route(ops, case)
        g = L.GemmArgs(a_buf.data_ptr(), w_buf.data_ptr(), 0, _ptr(bias), 0, 0, case.M, case.N, case.K, pr.lin.lda, pr.lin.ldw, case.N, epi, 0, 0, 0)
        sp = _split(L, case, cos, sin, fused)
        L.check(lib.p3v_gemm_qkv(C.byref(g), C.byref(sp), stream), "gemm_qkv")
        # the two calls it stands for, on the same operands
        g2 = L.GemmArgs(a_buf.data_ptr(), w_buf.data_ptr(), scratch.data_ptr(), _ptr(bias), 0, 0, case.M, case.N, case.K, pr.lin.lda, pr.lin.ldw,
                        case.N, epi, 0, 0, 0)
        L.check(lib.p3v_gemm(C.byref(g2), stream), "gemm")
        rc = lib.p3v_rope_kv_append(scratch.data_ptr(), _ptr(cos), _ptr(sin), _ptr(two["q"], qp.GUARD), _ptr(two["k"], qp.GUARD),
                                    _ptr(two["v"], qp.GUARD), case.B, case.L, case.nh, case.nkv, case.hd, case.past, 0, case.dst_t,
                                    int(case.off_is_past), case.tab_t, case.tab_div, case.q_scale, stream)
        torch.cuda.synchronize()
        names = ", ".join(f"{route.launch[i].name.decode()} rows {route.launch[i].row0}+{route.launch[i].rows}" for i in range(route.n_launches))
        return names, rc

    names, rc = _pinned(ops, case.knobs, call)
    # p3v_rope_kv_append takes heads of up to 96 dimensions and answers P3V_ERR_ARG beyond: at hd = 128 the fused call has no two calls
    # to be compared with, and the fp64 reference below is all there is (and the stronger of the two)
    assert rc == (L.P3V_OK if case.hd <= 96 else ERR_ARG), f"p3v_rope_kv_append: {rc}"
    flat = {n: f.cpu() for n, f in fused.items()}
    msg = pr.verify(flat)
    print(f"{case.id} [{family}]: {names}: {msg or _used(qp.needed_scale(lambda s: pr.verify(flat, s))) + ', nothing outside the windows touched'}")
    assert msg == "", msg
    for n, f in two.items() if rc == L.P3V_OK else ():                     # include/p3v.h: the two calls, bit for bit
        diff = flat[n].view(torch.int16) != f.cpu().view(torch.int16)
        assert not bool(diff.any()), f"{n}: {int(diff.sum())} elements differ from p3v_gemm + p3v_rope_kv_append, first at flat index {int(diff.nonzero()[0]) - qp.GUARD}"
    a_ref, w_ref = pr.operand_buffers()                                    # the operands and the tables are left alone
    assert torch.equal(a_buf.cpu().view(torch.int16), a_ref.view(torch.int16)) and torch.equal(w_buf.cpu().view(torch.int16), w_ref.view(torch.int16))
    if bias is not None:
        assert torch.equal(bias.cpu().view(torch.int16), pr.lin.bias.view(torch.int16))
    if cos is not None:
        assert torch.equal(cos.cpu().view(torch.int32), pr.cos.view(torch.int32)) and torch.equal(sin.cpu().view(torch.int32), pr.sin.view(torch.int32))


# what the route refuses, line by line (gemm_route(), csrc/p3v_gemm.hip): B, L, (hd, nh, nkv), past, dst_t (0: the case's own), bias, knobs
H64 = (64, 2, 2)
REFUSALS = {
    "M<=8": (1, 8, H64, 0, 0, False, ()),
    "past%8-with-dst_off_is_past": (1, 16, H64, 3, 0, False, ()),
    "dst_t%8": (1, 16, H64, 0, 28, False, ()),
    "hd=48": (1, 16, (48, 8, 8), 0, 0, False, ()),
    "bias-below-1024-rows": (1, 16, H64, 0, 0, True, ()),
    "q-region-of-96-columns": (1, 16, (96, 1, 4), 0, 0, False, ()),
    "256<M<1024": (1, 300, H64, 0, 0, False, ()),
    "q-region-of-192-columns-at-1024-rows": (1, 1024, (96, 2, 4), 0, 0, False, ()),
    "gemm_128=1": (1, 1024, H64, 0, 0, False, (("gemm_128", 1),)),
    "gemm_no_qkv_fuse=1": (1, 16, H64, 0, 0, False, (("gemm_no_qkv_fuse", 1),)),
}


@pytest.mark.parametrize("line", REFUSALS, ids=str)
def test_gemm_qkv_refusals(ops, line):
    """P3V_ERR_UNSUPPORTED for each line of the route, the same answer from ops.gemm_route, and nothing written anywhere."""
    B, Lq, (hd, nh, nkv), past, dst_t, has_bias, knobs = REFUSALS[line]
    L, lib, stream = ops.L, ops.L.lib(), torch.cuda.current_stream().cuda_stream
    case = qp.QkvCase(qp.SKINNY, B, Lq, hd, nh, nkv, 64, past=past, null=True, bias=has_bias)
    dst_t = dst_t or case.dst_t
    a, w = qp.sentinel(case.M * case.K).cuda(), qp.sentinel(case.N * case.K).cuda()
    bias = qp.sentinel(case.N).cuda() if has_bias else None
    shapes = {"q": (B, nh, Lq, hd), "k": (B, nkv, dst_t, hd), "v": (B, nkv, hd, dst_t)}
    flat = {n: qp.sentinel(torch.Size(sh).numel() + 2 * qp.GUARD).cuda() for n, sh in shapes.items()}
    epi = EPI_BIAS if has_bias else EPI_NONE

    def call():
        g = L.GemmArgs(a.data_ptr(), w.data_ptr(), 0, _ptr(bias), 0, 0, case.M, case.N, case.K, case.K, case.K, case.N, epi, 0, 0, 0)
        sp = L.QkvSplit(0, 0, _ptr(flat["q"], qp.GUARD), _ptr(flat["k"], qp.GUARD), _ptr(flat["v"], qp.GUARD), B, Lq, nh, nkv, hd, past, dst_t, 1,
                        0, 1, 1.0)
        rc = lib.p3v_gemm_qkv(C.byref(g), C.byref(sp), stream)
        r = ops.gemm_route(case.M, case.N, case.K, epilogue=epi, entry=L.GEMM_ENTRY_QKV, has_bias=has_bias, n_heads=nh, n_kv=nkv, hd=hd,
                           dst_off=past, dst_t=dst_t)
        torch.cuda.synchronize()
        return rc, r

    rc, r = _pinned(ops, knobs, call)
    assert rc == L.ERR_UNSUPPORTED and r.status == L.ERR_UNSUPPORTED and r.n_launches == 0, (rc, r.status, r.n_launches)
    for n, f in flat.items():
        assert torch.equal(f.cpu().view(torch.int16), qp.sentinel(f.numel()).view(torch.int16)), f"{n} was written"
    assert torch.equal(a.cpu().view(torch.int16), qp.sentinel(a.numel()).view(torch.int16))
    assert torch.equal(w.cpu().view(torch.int16), qp.sentinel(w.numel()).view(torch.int16))
