"""The small kernels between the projections and at the end of a step -- p3v_rmsnorm (both kernels, partly filled passes),
p3v_layernorm (all four instantiations, in place), p3v_rope_table (positions up to 131071, long factors), p3v_rope_kv_append (both
paths, every mode), p3v_argmax / p3v_topk / p3v_log_softmax (scalar tail, unaligned rows, strided rows, ties, infinities, NaN),
p3v_clip_cls_rows -- against plain fp64 on the probing inputs of tests/glue_probe.py, under its acceptance rules: the rounding
bracket for every bf16 output (every element; bit-exact but for rounding ties of the reference), |got - ref| <= E for fp32 outputs,
exact indices, bit-identical memory outside the written window.  tests/test_glue_probe_cpu.py shows on the references alone that a
kernel with a dropped chunk, a shifted weight, a wrong table row, an fp32 range reduction, ... cannot pass here."""
import pytest
import torch

import glue_probe as gp

pytestmark = pytest.mark.gpu

ids = lambda c: c.id


@pytest.fixture(scope="module")
def ops():
    from phi_3_vision_mlx_amd import ops as o
    o.L.lib()
    return o


def _used(s):
    """For the record, not asserted: the smallest of gp.SCALES x E under which the rule still accepts the kernel's output."""
    return "outside E" if s is None else "bit-exact against the rounded fp64 reference" if s == 0 else f"inside its brackets at {s:g} x E"


@pytest.mark.parametrize("case", gp.RMS_CASES, ids=ids)
def test_rmsnorm_in_bracket(ops, case):
    pr = gp.probe(case)
    got = ops.rmsnorm(pr.x.cuda(), pr.w.cuda(), gp.EPS).cpu()
    msg = pr.verify(got)
    print(f"{case.id}: {'k_rmsnorm_r<6>' if case.hidden <= 3072 else 'k_rmsnorm'}: {msg or _used(gp.needed_scale(lambda s: pr.verify(got, s)))}")
    assert msg == "", msg


@pytest.mark.parametrize("case", gp.LN_CASES, ids=ids)
def test_layernorm_in_bound(ops, case):
    pr = gp.probe(case)
    x, w, b = pr.x.cuda(), pr.w.cuda(), pr.b.cuda()
    got = ops.layernorm(x, w, b, gp.EPS, out_f32=case.out_f32)
    msg, ratio = pr.verify(got.cpu(), case.out_f32)
    kernel = ("k_layernorm_r" if case.hidden <= 1024 else "k_layernorm") + ("<f32>" if case.out_f32 else "<bf16>")
    print(f"{case.id}: {kernel}: " + (f"worst |got - ref| / E {ratio:.3f}" if case.out_f32 else msg or _used(ratio)))
    assert msg == "", msg
    assert torch.equal(x.cpu(), pr.x)                                      # the input is left alone
    if case.out_f32:                                                       # in place (include/p3v.h): the same bits
        same = ops.layernorm(x, w, b, gp.EPS, out_f32=True, out=x)
        assert same.data_ptr() == x.data_ptr() and torch.equal(x.view(torch.int32), got.view(torch.int32))


@pytest.mark.parametrize("case", gp.TABLE_CASES, ids=ids)
def test_rope_table_in_bound(ops, case):
    pr = gp.probe(case)
    cos, sin = ops.rope_table(pr.pos.cuda(), pr.inv.cuda(), pr.scale)
    assert cos.shape == sin.shape == (pr.pos.numel(), case.half)
    msg, ratio = pr.verify(cos.cpu(), sin.cpu())
    print(f"{case.id}: worst |got - ref| / E {ratio:.3f}")
    assert msg == "", msg


@pytest.mark.parametrize("case", gp.ROPE_CASES, ids=ids)
def test_rope_kv_append_in_bracket(ops, case):
    pr = gp.probe(case)
    c = case
    flat = {name: f.cuda() for name, (f, _) in pr.buffers().items()}
    view = {name: flat[name][gp.GUARD:flat[name].numel() - gp.GUARD].view(pr.shapes[name]) for name in flat}
    cos, sin = (None, None) if c.null else (pr.cos.cuda(), pr.sin.cuda())
    d_past = torch.tensor([c.past], dtype=torch.int32).cuda() if c.dev_past else None
    ops.rope_kv_append(pr.qkv.cuda(), cos, sin, view["q"], view["k"], view["v"], c.B, c.L, c.nh, c.nkv, c.hd,
                       0 if c.dev_past else c.past, c.dst_t, c.off_is_past, tab_t=c.tab_t, tab_div=c.tab_div, d_past=d_past,
                       q_scale=c.q_scale)
    after = {name: f.cpu() for name, f in flat.items()}
    msg = pr.verify(after)
    print(f"{case.id}: {'k_rope_kv_vt' if c.L >= 32 else 'k_rope_kv_append'}: {msg or 'q, k ' + _used(gp.needed_scale(lambda s: pr.verify(after, s))) + ', v exact, nothing else touched'}")
    assert msg == "", msg


def _strided(x, pad_value=30000.0):
    """The rows of x inside a [rows, n + 3] buffer whose padding would win every comparison."""
    rows, n = x.shape
    buf = torch.full((rows, n + 3), pad_value, dtype=gp.BF16)
    buf[:, :n] = x
    return buf.cuda()


@pytest.mark.parametrize("case", gp.VOCAB_CASES, ids=ids)
def test_argmax_topk_exact(ops, case):
    pr = gp.probe(case)
    n, x = case.n, pr.x.cuda()
    lib, stream = ops.L.lib(), torch.cuda.current_stream().cuda_stream
    buf = _strided(pr.x)
    msgs = [pr.verify_argmax(ops.argmax(x).cpu())]
    out = torch.full((gp.VOCAB_ROWS,), -7, dtype=torch.int32).cuda()
    ops.L.check(lib.p3v_argmax(buf.data_ptr(), out.data_ptr(), gp.VOCAB_ROWS, n, n + 3, stream), "argmax")
    msgs.append(pr.verify_argmax(out.cpu()) and "row_stride n + 3: " + pr.verify_argmax(out.cpu()))
    for k in gp.topk_ks(n):
        msgs.append(pr.verify_topk(ops.topk(x, k).cpu(), k))
        out = torch.full((gp.VOCAB_ROWS, k), -7, dtype=torch.int32).cuda()
        ops.L.check(lib.p3v_topk(buf.data_ptr(), out.data_ptr(), gp.VOCAB_ROWS, n, k, n + 3, stream), "topk")
        msgs.append(pr.verify_topk(out.cpu(), k) and "row_stride n + 3: " + pr.verify_topk(out.cpu(), k))
    msg = "; ".join(m for m in msgs if m)
    assert msg == "", msg


@pytest.mark.parametrize("case", gp.LSM_CASES, ids=ids)
def test_log_softmax_in_bracket(ops, case):
    pr = gp.probe(case)
    got = ops.log_softmax(pr.x.cuda()).cpu()
    msg = pr.verify(got)
    print(f"{case.id}: {msg or _used(gp.needed_scale(lambda s: pr.verify(got, s)))}")
    assert msg == "", msg


@pytest.mark.parametrize("case", gp.CLS_CASES, ids=ids)
def test_clip_cls_rows_exact(ops, case):
    pr = gp.probe(case)
    x = pr.x.cuda()
    ops.clip_cls_rows(x, pr.cls.cuda(), pr.pos.cuda())
    msg = pr.verify(x.cpu())
    assert msg == "", msg
