"""The packed decode GEMV at every way its launcher cuts a matrix into waves (gemv_b13_wpc: 1 .. 16 waves per CU; 1 .. 9 row pairs
per wave, a ragged last wave, idle waves, three- and four-wave workgroups) against the bf16 kernel on the same rows: the same bits.
Shapes come from the device's CU count; what was reached is asserted from p3v_gemv_b13_plan.  Every comparison is torch.equal."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF16, F32, I16, I32 = torch.bfloat16, torch.float32, torch.int16, torch.int32
E_TOP = 127                                  # biased exponents 97 .. 127 (2^-30 .. 1): the 31 binades of the format


@pytest.fixture(scope="module")
def ops():
    from phi_3_vision_mlx_amd import ops as o
    o.L.lib()
    return o


@pytest.fixture()
def knobs(ops):
    """set(name, value); whatever was set is put back afterwards"""
    saved = {}

    def set_(name, value):
        old = ops.set_tuning(name, value)
        saved.setdefault(name, old)
    try:
        yield set_
    finally:
        for k, v in saved.items():
            ops.set_tuning(k, v)


def g(shape, seed, std=1.0):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=gen) * std).to(BF16)


def every_pattern():
    """The bit patterns the format claims, as int32: 31 binades x 128 mantissas x both signs, +0 and -0 (7938 values)."""
    e = torch.arange(E_TOP - 30, E_TOP + 1, dtype=I32)
    m = torch.arange(128, dtype=I32)
    mag = ((e[:, None] << 7) | m[None, :]).reshape(-1)
    return torch.cat([mag, mag | 0x8000, torch.tensor([0x0000, 0x8000], dtype=I32)])


def window_matrix(rows, K, seed):
    """bf16 [rows, K] (on the host): a block of 16 shuffles of every pattern of the format, less one element (127,007 values: coprime
    to both K, so no two rows of a test are equal), repeated to fill the matrix."""
    pats = every_pattern()
    gen = torch.Generator().manual_seed(seed)
    n = rows * K
    assert n >= pats.numel() and 16 * pats.numel() - 1 == 127007
    block = torch.cat([pats[torch.randperm(pats.numel(), generator=gen)] for _ in range(16)])[:-1].to(I16)
    return block.repeat(-(-n // block.numel()))[:n].view(BF16).reshape(rows, K).contiguous()


def same_bits(a, b):
    return torch.equal(a.view(I16), b.view(I16))


def units_for(n_cu, wpc, upw):
    """a row-pair count that gives `upw` row pairs per wave on n_cu * wpc waves, with a ragged last wave (upw > 1)"""
    return n_cu * wpc if upw == 1 else n_cu * wpc * (upw - 1) + 3


@pytest.mark.parametrize("K", [3072, 8192])
def test_every_cut_gives_the_bf16_bits(ops, knobs, K):
    n_cu = ops.device_props(0)["cu_count"]
    # (waves per CU, row pairs): one row pair (a single live wave), then 1 .. 3 row pairs per wave at 16 and 8 waves per CU, and
    # the larger counts on small matrices at one wave per CU
    cases = [(16, 1)] + [(wpc, units_for(n_cu, wpc, u)) for wpc in (16, 8) for u in (1, 2, 3)]
    cases += [(1, units_for(n_cu, 1, u)) for u in ((4, 5, 6, 7, 8, 9) if K == 3072 else (2, 3))]
    x, nw = g((1, K), 10 + K).cuda(), (1 + 0.1 * g((K,), 11 + K)).cuda()
    rows = window_matrix(2 * max(u for _, u in cases) + 2, K, 12 + K).cuda()
    resid = g((1, rows.shape[0]), 13).cuda()
    upws, wpws, ragged, idle = set(), set(), False, False
    for wpc, units in cases:
        for epi in ("none", "norm_silu", "resid"):
            if epi == "norm_silu":
                units += units & 1                                # (gate / up pairs: the output count itself must be even)
            w = rows[:2 * units].contiguous()
            N = units if epi == "norm_silu" else 2 * units
            if epi == "norm_silu":
                pk, kw = ops.pack_b13(w, silu_pairs=True), dict(epilogue=ops.EPI_SILU_MUL, norm_w=nw, norm_eps=1e-5)
            else:
                pk, kw = ops.pack_b13(w), (dict(epilogue=ops.EPI_RESID_BF16, resid=resid[:, :N].contiguous()) if epi == "resid" else {})
            assert pk is not None
            ref = ops.gemv(x, w, **kw)
            assert ref.shape == (1, N) and torch.isfinite(ref.float()).all() and ref.float().abs().max() > 0
            knobs("gemv_b13_wpc", wpc)
            upw, waves, wpw, n_wg = ops.gemv_b13_plan(N, K, kw.get("epilogue", ops.EPI_NONE), n_cu)
            out = ops.gemv_b13(x, pk, **kw)
            assert same_bits(out, ref), (K, wpc, units, epi, upw, waves, wpw)
            upws.add(upw)
            wpws.add(wpw)
            ragged |= units % upw != 0
            idle |= n_wg * 4 > waves
    assert upws >= ({1, 2, 3, 4, 5, 6, 7, 8, 9} if K == 3072 else {1, 2, 3}), upws
    assert ragged and idle and (wpws == {3, 4} if n_cu == 256 else wpws <= {3, 4}), wpws


@pytest.mark.parametrize("K", [3072, 8192])
def test_step_folds_at_every_wave_count_are_the_bf16_step_folds(ops, knobs, K):
    """p3v_gemv_b13_step, begin and end, at three wave counts, against p3v_gemv_step on the same weights: the same
    logits, token and bookkeeping outputs; steps 1 and 2 tie two vocabulary rows for the maximum, step 3 is a NaN row (-1)."""
    n_cu = ops.device_props(0)["cu_count"]
    B, V, T, half, steps, N1 = 1, 4102, 40, 48, 4, 1024
    table = g((V, K), 70).cuda()
    cos, sin = torch.rand((B, T, half), dtype=F32).cuda(), torch.rand((B, T, half), dtype=F32).cuda()
    w1, nw1 = window_matrix(N1, K, 71).cuda(), (1 + 0.1 * g((K,), 72)).cuda()
    p1 = ops.pack_b13(w1)
    tok = torch.tensor([V + 5 if K == 8192 else 4004], dtype=I32).cuda()
    d_past = torch.tensor([11], dtype=I32).cuda()
    wl, nwl = window_matrix(V, K, 73), (1 + 0.1 * g((K,), 74)).cuda()
    wl[3000] = wl[300]
    wl = wl.cuda()
    pl = ops.pack_b13(wl)
    xs = []
    for s in range(steps + 1):                                    # one step past the history capacity: must not write
        x = g((B, K), 90 + s).cuda()
        if s in (1, 2):
            x = (wl[300].float() * nwl.float().reciprocal()).to(BF16).view(B, K).contiguous()
        if s == 3:
            x[0, 5] = float("nan")
        xs.append(x)

    def run(w_first, w_last):
        x_o = torch.full((B, K), 7.0, dtype=BF16).cuda()
        c_o, s_o = torch.zeros((B, 1, half), dtype=F32).cuda(), torch.zeros((B, 1, half), dtype=F32).cuda()
        out = torch.full((B, N1), float("nan"), dtype=BF16).cuda()
        assert ops.gemv_step_begin(tok, table, x_o, cos, sin, d_past, c_o, s_o, w_first, nw1, 1e-5, out)
        ws = torch.zeros((ops.L.GEMV_STEP_WS_BYTES // 4,), dtype=F32).cuda()
        hist = torch.zeros((B, steps), dtype=I32).cuda()
        st, tk, past = torch.zeros(1, dtype=I32).cuda(), torch.zeros(1, dtype=I32).cuda(), d_past.clone()
        nx, to = torch.zeros(B, dtype=I32).cuda(), torch.zeros(B, dtype=I32).cuda()
        got = [out.view(I16), x_o.view(I16), c_o, s_o]
        for s, x in enumerate(xs):
            lg = torch.empty((B, V), dtype=BF16).cuda()
            assert ops.gemv_step_end(x, w_last, nwl, 1e-5, lg, nx, to, hist, st, past, tk, ws)
            got += [lg.view(I16), nx.clone(), to.clone(), st.clone(), past.clone()]
        return got + [hist]

    ref = run(w1, wl)
    assert ref[4 + 5 * 1 + 1].item() == 300 and ref[4 + 5 * 3 + 1].item() == -1 and ref[-2].item() == 11 + steps + 1
    cuts = set()
    for wpc in (16, 8, 2):
        knobs("gemv_b13_wpc", wpc)
        knobs("gemv_b13_wpc_end", wpc)                            # (the vocabulary head's fold has its own)
        cuts |= {ops.gemv_b13_plan(N, K, ops.EPI_NONE, n_cu)[0] for N in (N1, V)}
        got = run(p1, pl)
        assert len(got) == len(ref)
        for i, (a, b) in enumerate(zip(got, ref)):
            assert torch.equal(a, b), (K, wpc, i)
    assert len(cuts) >= 2, cuts
