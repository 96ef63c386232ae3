"""p3v_sample and p3v_sample_step_end (csrc/p3v_sample.hip) on the MI355X against the exact reference of tests/sample_probe.py,
on its cases: every width at which the kernel takes another path, unaligned and strided rows with NaN / +inf behind them, ties,
the 2^32 weights, the -22.25 cut, every arg-max fallback; random and aimed draws.  Every decided draw must equal the exact
reference, an undecided one must be one of its bracket's two tokens; the counters, the logits buffer and everything outside the
written window are checked bit for bit; every refusal of the two entry points goes through the raw entry.
tests/test_sample_probe_cpu.py shows on the references alone that a kernel with one of 21 planted defects cannot pass here."""
import numpy as np
import pytest
import torch

import sample_probe as sp

pytestmark = pytest.mark.gpu

ids = lambda c: c.id
SENT = -7
ERR_ARG = -22


@pytest.fixture(scope="module")
def ops():
    from phi_3_vision_mlx_amd import ops as o
    o.L.lib()
    return o


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _records(rows):
    """[(T, k, p, seed, counter)] -> device records, each row's own (seed, counter) packed with sampling.pack."""
    from phi_3_vision_mlx_amd import sampling
    return torch.cat([sampling.pack([(T, k, p, seed)], c) for T, k, p, seed, c in rows]).cuda()


def _counters(rec):
    return rec[:, 5].cpu().tolist()


def _launch(ops, case, si, first=0, count=None):
    """One p3v_sample launch of a case's draws first .. first + count under setting si: (tokens, message about everything else)."""
    img, dr = sp.image(case), sp.draws(case)
    count = len(dr) - first if count is None else count
    T, k, p = case.settings[si]
    buf = torch.from_numpy(img.view(np.int16).copy()).cuda()                 # 16-byte aligned; off1: the row starts one element in
    rec = _records([(T, k, p, seed, c) for seed, c in dr[first:first + count]])
    out = torch.full((count + 8,), SENT, dtype=torch.int32).cuda()
    ptr = buf.data_ptr() + 2 * (case.lead + first * case.stride)
    assert first >= 0 and count >= 1 and case.lead + (first + count - 1) * case.stride + case.n <= buf.numel()
    assert buf.data_ptr() % 16 == 0
    ops.L.check(ops.L.lib().p3v_sample(ptr, case.stride, rec.data_ptr(), out.data_ptr(), count, case.n, _stream()), "sample")
    torch.cuda.synchronize()
    msgs = []
    if _counters(rec) != [c + 1 for _, c in dr[first:first + count]]:
        msgs.append("a counter is not +1")
    if not np.array_equal(buf.cpu().numpy().view(np.uint16), img):
        msgs.append("the logits buffer changed")
    if out[count:].cpu().tolist() != [SENT] * 8:
        msgs.append("out beyond rows was written")
    return out[:count].cpu().numpy().astype(np.int64), "; ".join(msgs)


def _describe(case, si, L, got, a, b):
    """A mismatch in full: the setting, the draw, and d and the exact weights around the two tokens."""
    T, k, p = case.settings[si]
    seed, c = sp.draws(case)[L]
    ex = sp.exact_row(case.content, case.n, L % sp.ROWS, case.settings[si])
    msg = f"{case.id} T={T} k={k} p={p!r} row {L % sp.ROWS} seed={seed:#x} counter={c} r={sp.draw_word(seed, c)}: got {got}, want {a}" + (f"..{b}" if a != b else "")
    if ex.greedy is None:
        x = sp.bf16_values(sp.rows_of(case.content, case.n)[L % sp.ROWS])
        z = x / np.float32(T)
        for i in sorted({int(t) for t in (got, a, b) if 0 <= t < case.n}):
            msg += f"; [{i}] l={float(x[i])!r} d={float(np.float64(z[i]) - np.float64(z.max()))!r} w={int(ex.w_lo[i])}..{int(ex.w_hi[i])} cum={int(ex.cum_lo[i])}"
        msg += f"; Q'={ex.Q_lo}..{ex.Q_hi}"
    return msg


@pytest.mark.parametrize("case", sp.CASES, ids=ids)
def test_sample_equals_the_exact_reference(ops, case):
    n_draws = decided = 0
    bad, other = [], []
    for si in range(len(case.settings)):
        got, msg = _launch(ops, case, si)
        a, b = sp.expected(case, si)
        n_draws, decided = n_draws + len(a), decided + int((a == b).sum())
        bad += [_describe(case, si, L, int(got[L]), int(a[L]), int(b[L])) for L in np.flatnonzero((got != a) & (got != b))]
        if msg:
            other.append(f"{case.settings[si]}: {msg}")
    print(f"{case.id}: draws {n_draws}, decided {decided}, aimed {sp.n_aimed(case) * len(case.settings)}, mismatches {len(bad)}")
    assert not bad, bad[:5]
    assert not other, other


STEP_N, STEP_B, MAX_STEPS = (9, 1025, 8193, 32768), (1, 5, 300), 3          # 300: more workgroups than CUs
STEP_SETTINGS = ((0.7, 40, 0.9), (1.0, 0, 1.0), (3.0, 2, 0.3))


@pytest.mark.parametrize("B", STEP_B)
@pytest.mark.parametrize("n", STEP_N)
def test_step_end_tokens_and_books(ops, n, B):
    lib, rows = ops.L.lib(), sp.rows_of("gauss", n)
    logits = torch.from_numpy(rows[np.arange(B) % sp.ROWS].view(np.int16).copy()).cuda()
    rng = np.random.default_rng(sp._crc("step", n, B))
    seeds = [int(s) for s in rng.integers(0, 1 << 64, B, dtype=np.uint64)]
    c0 = [int(c) for c in rng.integers(0, 1 << 30, B)]
    sets = [(0.0, 40, 0.9) if b % 2 else STEP_SETTINGS[(b // 2) % 3] for b in range(B)]       # rows alternate T > 0 and T = 0
    rec = _records([(*sets[b], seeds[b], c0[b]) for b in range(B)])
    guarded = torch.full((B + 2, MAX_STEPS), SENT, dtype=torch.int32).cuda()                  # a guard row on either side
    history = guarded[1:B + 1]
    next_tok, tok = (torch.full((B + 8,), SENT, dtype=torch.int32).cuda() for _ in range(2))
    d_step, d_past, ticket = (torch.tensor([v], dtype=torch.int32).cuda() for v in (0, 100, 0))
    bad = []
    for step in range(MAX_STEPS + 1):                                                         # the last launch: *d_step == max_steps
        before = guarded.clone()
        ops.L.check(lib.p3v_sample_step_end(logits.data_ptr(), rec.data_ptr(), next_tok.data_ptr(), tok.data_ptr(), history.data_ptr(),
                                            d_step.data_ptr(), d_past.data_ptr(), ticket.data_ptr(), B, n, MAX_STEPS, _stream()),
                    "sample_step_end")
        torch.cuda.synchronize()
        got = tok[:B].cpu().tolist()
        for b in range(B):
            lo, hi = sp.exact_draw("gauss", n, b % sp.ROWS, sets[b], seeds[b], c0[b] + step)
            if got[b] not in (lo, hi):
                bad.append((step, b, sets[b], seeds[b], c0[b] + step, got[b], lo, hi))
        assert next_tok.cpu().tolist() == got + [SENT] * 8 and tok[B:].cpu().tolist() == [SENT] * 8
        assert (d_step.item(), d_past.item(), ticket.item()) == (step + 1, 101 + step, 0)
        assert _counters(rec) == [c + step + 1 for c in c0]
        want = before.clone()
        if step < MAX_STEPS:
            want[1:B + 1, step] = tok[:B]
        assert torch.equal(guarded, want)                                                     # history[:, step] alone, or nothing
    assert torch.equal(logits.cpu(), torch.from_numpy(rows[np.arange(B) % sp.ROWS].view(np.int16).copy()))
    assert not bad, bad[:5]


def test_refusals_write_nothing(ops):
    lib, s = ops.L.lib(), _stream()
    UNS = ops.L.ERR_UNSUPPORTED
    B = 1025
    logits = torch.zeros((B * 8 + 32769,), dtype=torch.bfloat16).cuda()                       # room for whatever a wrong launch reads
    rec = _records([(1.0, 0, 1.0, 5, 3)] * 4).repeat(257, 1)[:B].contiguous()
    rec0 = rec.clone()
    bufs = {name: torch.full((3 * B,), SENT, dtype=torch.int32).cuda() for name in ("out", "next_tok", "tok", "history")}
    d_step, d_past, ticket = (torch.tensor([v], dtype=torch.int32).cuda() for v in (0, 100, 0))
    lp, rp, op = logits.data_ptr(), rec.data_ptr(), bufs["out"].data_ptr()
    for args, want in (((None, 8, rp, op, 2, 8), ERR_ARG), ((lp, 8, None, op, 2, 8), ERR_ARG), ((lp, 8, rp, None, 2, 8), ERR_ARG),
                       ((lp, 8, rp, op, -1, 8), ERR_ARG), ((lp, 8, rp, op, 2, 0), ERR_ARG), ((lp, 7, rp, op, 2, 8), ERR_ARG),
                       ((lp, 32769, rp, op, 1, 32769), UNS), ((lp, 8, rp, op, 1025, 8), UNS), ((lp, 8, rp, op, 0, 8), 0)):
        assert lib.p3v_sample(*args, s) == want, args
    full = dict(logits=lp, rows_params=rp, next_tok=bufs["next_tok"].data_ptr(), tok=bufs["tok"].data_ptr(),
                history=bufs["history"].data_ptr(), d_step=d_step.data_ptr(), d_past=d_past.data_ptr(), ticket=ticket.data_ptr())
    call = lambda kw, B_, n_: lib.p3v_sample_step_end(*kw.values(), B_, n_, 2, s)
    for name in full:
        assert call({**full, name: None}, 2, 8) == ERR_ARG, name
    assert call(full, 0, 8) == ERR_ARG and call(full, 2, 0) == ERR_ARG and call(full, -1, 8) == ERR_ARG
    assert call(full, 1025, 8) == UNS and call(full, 1, 32769) == UNS
    torch.cuda.synchronize()
    assert torch.equal(rec, rec0) and all(bool((b == SENT).all()) for b in bufs.values())
    assert (d_step.item(), d_past.item(), ticket.item()) == (0, 100, 0)


def test_same_tokens_twice_and_alone(ops):
    for cid in ("gauss-n32767-contig", "gauss-n8193-pad3", "ties32-n32768-off1"):
        case = next(c for c in sp.CASES if c.id == cid)
        first, msg = _launch(ops, case, 1)
        again, _ = _launch(ops, case, 1)
        assert msg == "" and np.array_equal(first, again), cid
        for L in (0, 4, 9, 22):                                              # a row's token alone = among the other rows
            alone, msg = _launch(ops, case, 1, first=L, count=1)
            assert msg == "" and alone[0] == first[L], (cid, L)
        nine, _ = _launch(ops, case, 1, first=7, count=9)
        assert np.array_equal(nine, first[7:16]), cid
