"""The quantisers -- p3v_kv_quantize (k_kv_quantize_v with its byte-wise tail, the scalar k_kv_quantize at unaligned t0 and head sizes 64 /
32, the kvq_old path), p3v_kv_dequantize, the append sites of the three p3v_attention_decode_q8 kernels, and p3v_quant_fp8_rows on both
register layouts with partly filled passes and workgroups -- against plain fp64 on the probing inputs of tests/quant_probe.py, under its
rules: scales bit for bit one IEEE division, int8 codes inside the integer rounding bracket (the round-half-to-even code itself on the exact
GRID), e4m3 codes bit for bit (inside the code bracket under the fused norm), bit-identical memory outside the written window, sources
untouched.  tests/test_quant_probe_cpu.py shows on the references alone that a kernel that truncates, rounds half away, misses a lane of
the maximum, takes a neighbour's scale, leaks a token or writes one too many cannot pass here."""
import pytest
import torch

import glue_probe as gp
import quant_probe as qp

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


def _pinned(ops, case, call):
    old = []
    try:
        for name, value in case.knobs:
            old.append((name, ops.set_tuning(name, value)))
        return call()
    finally:
        for name, value in reversed(old):
            ops.set_tuning(name, value)


def _views(pr, dev):
    return {n: dev[n][qp.GUARD:dev[n].numel() - qp.GUARD].view(pr.shapes[n]) for n in dev}


def _same_bits(dev, host):
    it = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[host.element_size()]
    return torch.equal(dev.cpu().contiguous().view(it).flatten(), host.contiguous().view(it).flatten())


def _kv_quantize(ops, pr, case):
    c = case
    k, vt = pr.k.view(qp.BH, 1, c.src_t, c.hd).cuda(), pr.vt.view(qp.BH, 1, c.hd, c.src_t).cuda()
    dev = {n: f.cuda() for n, f in pr.buffers().items()}
    v = _views(pr, dev)
    _pinned(ops, c, lambda: ops.kv_quantize(k, vt, v["k8"].view(qp.BH, 1, c.dst_t, c.hd), v["v8"].view(qp.BH, 1, c.hd, c.dst_t), v["ksc"], v["vsc"],
                                            c.t0, c.n_tok))
    assert _same_bits(k, pr.k) and _same_bits(vt, pr.vt)                       # the sources are left alone
    return {n: f.cpu() for n, f in dev.items()}


@pytest.mark.parametrize("family", qp.FAMILIES)
@pytest.mark.parametrize("case", qp.KV_CASES, ids=ids)
def test_kv_quantize_against_fp64(ops, case, family):
    pr = qp.probe(case, family)
    after = _kv_quantize(ops, pr, case)
    msg = pr.verify(after)
    print(f"{case.id} [{family}]: {case.kernel}: {msg or 'scales exact, codes ' + _used(qp.needed_scale(lambda s: pr.verify(after, s))) + ', nothing outside the window touched'}")
    assert msg == "", msg
    if case.knobs:                                                           # "the same arithmetic": the bits of the vector kernel
        twin = next(c for c in qp.KV_CASES if not c.knobs and (c.hd, c.src_t, c.dst_t, c.t0, c.n_tok) == (case.hd, case.src_t, case.dst_t, case.t0, case.n_tok))
        assert twin.kernel == "k_kv_quantize_v"
        other = _kv_quantize(ops, pr, twin)
        assert all(_same_bits(other[n], after[n]) for n in after), "k_kv_quantize and k_kv_quantize_v differ"


@pytest.mark.parametrize("case", qp.DQ_CASES, ids=ids)
def test_kv_dequantize_against_fp64(ops, case):
    pr = qp.probe(case)
    c = case
    src = (pr.codes["k"].view(qp.BH, 1, c.src_t, c.hd), pr.v8t.view(qp.BH, 1, c.hd, c.src_t), pr.scales["k"], pr.scales["v"])
    k8, v8t, ksc, vsc = (t.cuda() for t in src)
    dev = {n: f.cuda() for n, f in pr.buffers().items()}
    v = _views(pr, dev)
    ops.kv_dequantize(k8, v8t, ksc, vsc, v["k"].view(qp.BH, 1, c.dst_t, c.hd), v["v"].view(qp.BH, 1, c.hd, c.dst_t), c.n_tok)
    after = {n: f.cpu() for n, f in dev.items()}
    msg = pr.verify(after)
    print(f"{c.id}: k_kv_dequantize: {msg or _used(qp.needed_scale(lambda s: pr.verify(after, s))) + ', nothing outside the window touched'}")
    assert msg == "", msg
    assert all(_same_bits(d, h) for d, h in zip((k8, v8t, ksc, vsc), src))


@pytest.mark.parametrize("case", qp.AP_CASES, ids=ids)
def test_q8_decode_append_against_fp64(ops, case):
    pr = qp.probe(case)
    c, B, nh, hd, T = case, qp.AP_B, qp.AP_NH, qp.AP_HD, qp.AP_T
    dev = {n: f.cuda() for n, f in pr.buffers().items()}
    v = _views(pr, dev)
    qkv, cos, sin = pr.qkv.cuda(), pr.cos.cuda(), pr.sin.cuda()
    out = torch.empty((B, c.L, nh * hd), dtype=gp.BF16, device="cuda")
    ws = ops.attention_ws(B, c.L, nh, hd, c.n_split, "cuda")
    _pinned(ops, c, lambda: ops.attention_decode_q8(qkv, cos, sin, c.L, v["k8"], v["v8"], v["ksc"], v["vsc"], out, B, c.L, nh, nh, hd, hd ** -0.5,
                                                     c.past, T, ws, c.n_split, merge_in_launch=c.fused))
    after = {n: f.cpu() for n, f in dev.items()}
    msg = pr.verify(after)
    print(f"{c.id}: {c.kernel}: {msg or 'scales exact, codes ' + _used(qp.needed_scale(lambda s: pr.verify(after, s))) + ', nothing outside [past, past + L) touched'}")
    assert msg == "", msg
    assert _same_bits(qkv, pr.qkv)


@pytest.mark.parametrize("case", qp.F8_CASES, ids=ids)
def test_quant_fp8_rows_against_reference(ops, case):
    pr = qp.probe(case)
    c = case
    x, w = pr.x.cuda(), pr.w.cuda() if c.norm else None
    dev = {n: f.cuda() for n, f in pr.buffers().items()}
    q = dev["q"][qp.GUARD:-qp.GUARD].view(c.rows, c.hidden)
    s = dev["scale"][qp.GUARD:-qp.GUARD]
    ops.quant_fp8_rows(x, w, gp.EPS if c.norm else 0.0, out=q, scale=s)
    after = {n: f.cpu() for n, f in dev.items()}
    msg = pr.verify(after)
    kept, uniq = pr.shares()
    rule = "bit-exact" if not c.norm else f"scales exact, codes inside their brackets ({100 * kept:.0f} % of rows judged, bracket one value on {100 * uniq:.2f} %)"
    print(f"{c.id}: {c.kernel}: {msg or rule + ', nothing outside touched'}")
    assert msg == "", msg
    assert _same_bits(x, pr.x)
    if c.norm:                                                               # "exactly the row p3v_rmsnorm would have written"
        q2, s2 = ops.quant_fp8_rows(ops.rmsnorm(x, w, gp.EPS))
        assert torch.equal(q2, q) and torch.equal(s2.view(torch.int32), s.view(torch.int32)), "quant(x, w) != quant(rmsnorm(x, w))"
