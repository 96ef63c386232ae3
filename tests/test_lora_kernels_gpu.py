"""The LoRA kernels -- p3v_lora_down / p3v_lora_up and the per-row forms p3v_lora_down_rows / p3v_lora_up_rows of the adapter bank -- against
plain fp64 of the rule in include/p3v.h on the input families of tests/lora_probe.py, under the acceptance rules of tests/proj_probe.py:
on the exact GRID t equals the reference as floats (every slice partial its own exact value) and `out` IS the fp64 value pushed through
the roundings of the epilogue; on SPIKES |t - T| <= E_t and the rounding bracket on every element of `out`.  Partial last slices (K = 192,
520), ranks on both sides of an 8-column chunk, r_max below an entry's rank, None entries, a null lora_b, slots -1 / -7 / n_slots; t starts
as a NaN pattern that rows without an adapter and columns >= r must keep; `out` sits in a guarded buffer.  tests/test_lora_probe_cpu.py shows
on the references alone that a kernel with a dropped element, slice or lora_b row, a bf16 t, a neighbour's slot, the clamped rank as
lora_a's row stride, ... cannot pass here."""
import pytest
import torch

import lora_probe as lp

pytestmark = pytest.mark.gpu

PAIRS = [(c, f) for c in lp.CASES for f in lp.families(c)]
IDS = [f"{c.id}-{f}" for c, f in PAIRS]


@pytest.fixture(scope="module")
def ops():
    from phi_3_vision_mlx_amd import ops as o
    o.L.lib()
    return o


def _used(s):
    """For the record, not asserted: the smallest of the scales x E under which the rule still accepts the kernel's output."""
    return "outside E" if s is None else "bit-exact against the rounded fp64 reference" if s == 0 else f"inside its brackets at {s:g} x E"


def _same_bits(dev, host):
    it = {2: torch.int16, 4: torch.int32}[host.element_size()]
    return torch.equal(dev.cpu().contiguous().view(it).flatten(), host.contiguous().view(it).flatten())


def _report(case, pr, out, t):
    msg_t, ratio = pr.verify_t(t)
    msg = pr.verify(out)
    t_says = "t exact" if pr.grid else f"t at {ratio:.3f} of E_t"
    print(f"{case.id} [{pr.family}]: {case.kernel}: " + ("; ".join(m for m in (msg_t, msg) if m) or
          f"{t_says}, unwritten t untouched; out {_used(lp.needed_scale(lambda s: pr.verify(out, s)))}, nothing outside [M, N] touched"))
    return "; ".join(m for m in (msg_t, msg) if m)


@pytest.mark.parametrize("case,family", PAIRS, ids=IDS)
def test_lora_against_fp64(ops, case, family):
    pr = lp.probe(case, family)
    c = case
    x, y = pr.x.cuda(), pr.y.cuda()
    resid = None if pr.resid is None else pr.resid.cuda()
    t = pr.t_buffer().cuda()
    tv = t[lp.GUARD:t.numel() - lp.GUARD]
    out = pr.out_buffer().cuda()
    ov = out[lp.GUARD:lp.GUARD + c.M * c.N].view(c.M, c.N)
    dev = [None if e is None else (e[0].cuda(), e[1].cuda()) for e in pr.entries]
    if not c.rows:
        (a, b), scale = dev[0], pr.scales[0]
        ops.lora_down(x, a, out=tv.view(c.M, c.r))
        ops.lora_up(y, tv.view(c.M, c.r), b, scale, c.epi, resid=resid, out=ov)
    else:
        norm_w = None if pr.norm_w is None else pr.norm_w.cuda()
        if c.norm:                                                           # the row as p3v_rmsnorm writes it is the reference's h
            pr.finish(ops.rmsnorm(x, norm_w, lp.EPS).cpu())
        table = ops.lora_table([None if e is None else (e[0], e[1], pr.scales[s]) for s, e in enumerate(dev)], "cuda")
        assert int(table[lp.NULL_B, 0]) != 0 and int(table[lp.NULL_B, 2]) & 0xFFFFFFFF == lp.TABLE_RANKS[lp.NULL_B]
        table[lp.NULL_B, 1] = 0                                              # an entry with a null lora_b
        ra = torch.tensor(pr.slots, dtype=torch.int32).cuda()
        assert ops.lora_slices(c.K) == c.S
        t3 = tv.view(c.M, c.S, c.r_max)
        ops.lora_down_rows(x, table, ra, c.r_max, norm_w=norm_w, norm_eps=lp.EPS if c.norm else 0.0, out=t3)
        ops.lora_up_rows(y, t3, table, ra, c.K, c.r_max, c.epi, resid=resid, out=ov)
    msg = _report(c, pr, out.cpu(), t.cpu())
    if c.norm:
        pr.finish(lp.rms_restate(pr.x, pr.norm_w))                           # (the cached probe goes back to its CPU reference)
    assert msg == "", msg
    assert _same_bits(x, pr.x) and _same_bits(y, pr.y) and (resid is None or _same_bits(resid, pr.resid))
    assert all(e is None or (_same_bits(d[0], e[0]) and _same_bits(d[1], e[1])) for d, e in zip(dev, pr.entries))
