"""The 13-bit packed GEMV with the exponent base carried by the staged activations (gemv_b13_xscale = 1, GemvB13<true> in
p3v_gemv_b13.hip) against the bf16 kernel on the bf16 matrix: torch.equal on the bits, at the eligibility edge
(shift 96), at a small shift, on activations that probe the scaling, on a matrix the scaled form does not serve, through the two
step folds and through a replayed decode.  Every case also runs with the knob at 0 (the exact decode everywhere).  The launcher keeps
the scaled form to K = 3072; the K = 8192 cases pin that whatever it chooses there, the bits are the bf16 kernel's."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF16, F32, I16, I32 = torch.bfloat16, torch.float32, torch.int16, torch.int32
MAX_SHIFT = 96


@pytest.fixture(scope="module")
def ops():
    from phi_3_vision_mlx_amd import ops as o
    o.L.lib()
    return o


@pytest.fixture
def xscale(ops):
    old = []

    def pin(v):
        old.append(ops.set_tuning("gemv_b13_xscale", v))
    yield pin
    if old:
        ops.set_tuning("gemv_b13_xscale", old[0])


def g(shape, seed, std=1.0):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=gen) * std).to(BF16)


def from_bits(b):
    return b.to(I16).view(BF16)


def window_matrix(rows, K, seed, e_top=127):
    """bf16 [rows, K] on the host: 16 shuffles of every pattern of the format under largest exponent e_top (31 binades x 128 mantissas
    x both signs, +0, -0), less one element (127,007 values: coprime to both K, so no two rows are equal), repeated."""
    e, m = torch.arange(e_top - 30, e_top + 1, dtype=I32), torch.arange(128, dtype=I32)
    mag = ((e[:, None] << 7) | m[None, :]).reshape(-1)
    pats = torch.cat([mag, mag | 0x8000, torch.tensor([0x0000, 0x8000], dtype=I32)])
    gen = torch.Generator().manual_seed(seed)
    n = rows * K
    block = torch.cat([pats[torch.randperm(pats.numel(), generator=gen)] for _ in range(16)])[:-1].to(I16)
    return block.repeat(-(-n // block.numel()))[:n].view(BF16).reshape(rows, K).contiguous()


def moved(w, e_top):
    """the window matrix under 127 moved to largest exponent e_top (zeros stay zeros), on the device"""
    b = w.view(I16).to(I32) & 0xffff
    return from_bits(torch.where((b & 0x7f80) != 0, b + ((e_top - 127) << 7), b)).reshape(w.shape).contiguous()


def same_bits(a, b):
    if a.dtype == F32:
        return torch.equal(a.view(I32), b.view(I32))
    return torch.equal(a.view(I16), b.view(I16))


def same_but_nan(a, b):
    """the same NaN mask, and the same bits everywhere else"""
    na, nb = torch.isnan(a.float()), torch.isnan(b.float())
    return torch.equal(na, nb) and same_bits(torch.where(na, torch.zeros_like(a), a), torch.where(nb, torch.zeros_like(b), b))


@pytest.fixture(scope="module")
def case():
    """K -> (x [1, K], norm weight, 8204 rows of the window under 127), on the device; built once, never written"""
    cache = {}

    def get(K):
        if K not in cache:
            cache[K] = (g((1, K), 10 + K).cuda(), (1 + 0.1 * g((K,), 11 + K)).cuda(), window_matrix(2 * 4102, K, 12 + K).cuda())
        return cache[K]
    yield get
    cache.clear()


def run_both(ops, x, w, epi, nw, N, knob, seed=13):
    """(the packing, p3v_gemv's output, p3v_gemv_b13's), the latter pinned: the library's route says that the call runs the form the
    test is about -- the scaled one exactly at knob = 1, K = 3072 and a base whose factor leaves the activations room."""
    if epi == "norm_silu":
        pk = ops.pack_b13(w, silu_pairs=True)
        kw = dict(epilogue=ops.EPI_SILU_MUL, norm_w=nw, norm_eps=1e-5)
    else:
        pk = ops.pack_b13(w)
        kw = {"none": {}, "norm": dict(norm_w=nw, norm_eps=1e-5), "f32": dict(epilogue=ops.EPI_F32),
              "resid": dict(epilogue=ops.EPI_RESID_BF16, resid=g((1, N), seed).cuda())}[epi]
    assert pk is not None
    r = ops.gemv_route(1, N, pk.K, kw.get("epilogue", ops.EPI_NONE), fmt="b13", has_norm="norm_w" in kw, exp_base=pk.base)
    scaled = knob == 1 and pk.K == 3072 and pk.base - 1 <= MAX_SHIFT
    want = "k_gemv3<GemvB13<%s>, 1, %s>" % ("true" if scaled else "false", "1, 6" if pk.K == 3072 else "4, 4")
    assert r.status == 0 and r.name.decode() == want, f"the call runs {r.name.decode()!r}, not {want}"
    return pk, ops.gemv(x, w, **kw), ops.gemv_b13(x, pk, **kw)


@pytest.mark.parametrize("knob", [1, 0])
@pytest.mark.parametrize("e_top", [127, 100])
@pytest.mark.parametrize("epi", ["none", "norm_silu", "resid", "f32"])
@pytest.mark.parametrize("N", [2, 66, 4102])
@pytest.mark.parametrize("K", [3072, 8192])
def test_scaled_gemv_is_the_bf16_gemv(ops, case, xscale, K, N, epi, e_top, knob):
    xscale(knob)
    x, nw, rows = case(K)
    w = moved(rows[:2 * N if epi == "norm_silu" else N], e_top)
    pk, ref, out = run_both(ops, x, w, epi, nw, N, knob)
    assert pk.base - 1 == e_top - 31 <= MAX_SHIFT                           # 96: the edge of the scaled form; 69: a small shift
    assert ref.shape == (1, N) and same_bits(out, ref)
    assert torch.isfinite(ref.float()).all() and ref.float().abs().max() > 0


def probe_x(kind, K, seed):
    """an activation row around the factor 2^96 of the window under 127"""
    x = g((1, K), seed)
    if kind == "zeros":
        x[0, ::5], x[0, 1::7] = 0.0, -0.0
    elif kind == "denormal":
        x.view(I16)[0, 9] = 0x0041                                           # a bf16 denormal
    elif kind == "largest":
        x[0, 3::11] = from_bits(torch.tensor([((127 + 31) << 7) | 0x40], dtype=I32))[0]       # 2^(127 - 96) * 1.5
        x[0, 4::11] = -x[0, 3::11]
    elif kind == "unfit":
        x[0, K - 3] = 2.0 ** 40                                              # times 2^96: not finite -- the exact decode inside the kernel
    elif kind == "inf":
        x[0, 17] = float("inf")
    elif kind == "nan":
        x[0, 17] = float("nan")
    return x.cuda()


@pytest.mark.parametrize("knob", [1, 0])
@pytest.mark.parametrize("epi", ["none", "norm"])
@pytest.mark.parametrize("kind", ["zeros", "denormal", "largest", "unfit", "inf", "nan"])
@pytest.mark.parametrize("K", [3072, 8192])
def test_activation_probes_on_an_eligible_matrix(ops, case, xscale, K, kind, epi, knob):
    xscale(knob)
    _, nw, rows = case(K)
    N = 66
    x = probe_x(kind, K, 20 + K)
    pk, ref, out = run_both(ops, x, rows[:N].contiguous(), epi, nw, N, knob)
    assert pk.base - 1 == MAX_SHIFT
    assert same_but_nan(out, ref)
    if kind in ("zeros", "denormal", "largest", "unfit"):
        assert torch.isfinite(ref.float()).all() and ref.float().abs().max() > 0
    elif epi == "none":
        assert not torch.isfinite(ref.float()).any()                         # Inf and NaN reach every output


@pytest.mark.parametrize("knob", [1, 0])
@pytest.mark.parametrize("epi", ["none", "norm_silu"])
@pytest.mark.parametrize("K", [3072, 8192])
def test_ineligible_matrix_keeps_the_exact_decode(ops, case, xscale, K, epi, knob):
    xscale(knob)
    x, nw, rows = case(K)
    N = 66
    w = moved(rows[:2 * N if epi == "norm_silu" else N], 130)
    pk, ref, out = run_both(ops, x, w, epi, nw, N, knob)
    assert pk.base - 1 == 99 > MAX_SHIFT
    assert same_bits(out, ref) and torch.isfinite(ref.float()).all()


@pytest.mark.parametrize("knob", [1, 0])
@pytest.mark.parametrize("K", [3072, 8192])
def test_step_folds_are_the_bf16_step_folds(ops, xscale, K, knob):
    """p3v_gemv_b13_step against p3v_gemv_step on the same weights (the shapes of test_gemv_b13_gpu.py): begin -- x_out is the
    embedding row as it is, not the scaled one -- and end with a tie for the first maximum and a NaN row reporting -1."""
    xscale(knob)
    B, V, T, half, steps, N1 = 1, 4102, 40, 48, 4, 1024
    table = g((V, K), 70).cuda()
    cos, sin = torch.rand((B, T, half), dtype=F32).cuda(), torch.rand((B, T, half), dtype=F32).cuda()
    w1, nw1 = window_matrix(N1, K, 71).cuda(), (1 + 0.1 * g((K,), 72)).cuda()
    p1 = ops.pack_b13(w1)
    assert p1.base - 1 == MAX_SHIFT
    tok = torch.tensor([V + 5 if K == 8192 else 4004], dtype=I32).cuda()
    d_past = torch.tensor([11], dtype=I32).cuda()
    x_a, x_b = torch.empty((B, K), dtype=BF16).cuda(), torch.full((B, K), 7.0, dtype=BF16).cuda()
    ca, sa = torch.empty((B, 1, half), dtype=F32).cuda(), torch.empty((B, 1, half), dtype=F32).cuda()
    cb, sb = torch.zeros_like(ca), torch.zeros_like(sa)
    out_a, out_b = (torch.full((B, N1), float("nan"), dtype=BF16).cuda() for _ in range(2))
    assert ops.gemv_step_begin(tok, table, x_a, cos, sin, d_past, ca, sa, w1, nw1, 1e-5, out_a)
    assert ops.gemv_step_begin(tok, table, x_b, cos, sin, d_past, cb, sb, p1, nw1, 1e-5, out_b)
    assert same_bits(out_a, out_b) and torch.equal(ca, cb) and torch.equal(sa, sb)
    assert same_bits(x_b, x_a) and same_bits(x_b, table[min(int(tok.item()), V - 1)].view(B, K))
    assert not torch.isnan(out_b.float()).any()

    wl, nwl = window_matrix(V, K, 73), (1 + 0.1 * g((K,), 74)).cuda()
    wl[3000] = wl[300]                                            # two equal vocabulary rows; steps 1 and 2 make them the maximum
    wl = wl.cuda()
    pl = ops.pack_b13(wl)
    ws_a, ws_b = (torch.zeros((ops.L.GEMV_STEP_WS_BYTES // 4,), dtype=F32).cuda() for _ in range(2))
    hist_a, hist_b = (torch.zeros((B, steps), dtype=I32).cuda() for _ in range(2))
    st_a, st_b, tk_a, tk_b = (torch.zeros(1, dtype=I32).cuda() for _ in range(4))
    pa, pb = d_past.clone(), d_past.clone()
    nx_a, nx_b, to_a, to_b = (torch.zeros(B, dtype=I32).cuda() for _ in range(4))
    for s in range(steps + 1):                                    # one step past the history capacity: must not write
        x = g((B, K), 90 + s).cuda()
        if s in (1, 2):                                           # x along the tied rows: rows 300 and 3000 carry the (equal) maximum
            x = (wl[300].float() * nwl.float().reciprocal()).to(BF16).view(B, K).contiguous()
        if s == 3:
            x[0, 5] = float("nan")                                # a poisoned row reports -1
        lg_a, lg_b = torch.empty((B, V), dtype=BF16).cuda(), torch.empty((B, V), dtype=BF16).cuda()
        assert ops.gemv_step_end(x, wl, nwl, 1e-5, lg_a, nx_a, to_a, hist_a, st_a, pa, tk_a, ws_a)
        assert ops.gemv_step_end(x, pl, nwl, 1e-5, lg_b, nx_b, to_b, hist_b, st_b, pb, tk_b, ws_b)
        assert same_but_nan(lg_a, lg_b)
        assert torch.equal(nx_a, nx_b) and torch.equal(to_a, to_b), (s, nx_a.tolist(), nx_b.tolist())
        assert st_b.item() == s + 1 and pb.item() == 12 + s
        if s in (1, 2):
            assert lg_b[0, 300].item() == lg_b[0, 3000].item() == lg_b.float().max().item() and nx_b[0].item() == 300
        if s == 3:
            assert nx_b[0].item() == -1
    assert torch.equal(hist_a, hist_b)


def _decode8(model, ids):
    logits, cache = model(input_ids=ids, max_tokens=16)
    token = logits[:, -1, :].float().argmax(dim=-1, keepdim=True)
    toks, last = [], None
    for _ in range(8):
        last, token = model.greedy_step(token, cache)
        toks.append(token.reshape(-1).tolist())
    torch.cuda.synchronize()
    assert "graph" in cache[0].state.graphs["greedy"]             # the steps above were graph replays
    return toks, last.detach().clone().view(-1)


def test_model_decodes_the_same_with_the_knob_at_0_and_1(ops, xscale):
    """Full hidden size, two layers, a 40-token prompt, 8 greedy tokens through the replayed graph (captured per prompt, so each
    run bakes in the knob it was captured under): tokens and last logits with gemv_b13_xscale = 0 and = 1."""
    from phi_3_vision_mlx_amd.api import load_synthetic
    ids = torch.randint(3, 32000, (1, 40), dtype=torch.int64, generator=torch.Generator().manual_seed(6))
    model, _ = load_synthetic(blind_model=True, tiny=False, seed=0, device="cuda:0", num_hidden_layers=2)
    assert len(model.w13) == 7 and all(pk.base - 1 <= MAX_SHIFT for pk in model.w13.values())   # every packed matrix is eligible
    xscale(0)
    toks0, logits0 = _decode8(model, ids)
    xscale(1)
    toks1, logits1 = _decode8(model, ids)
    assert toks1 == toks0 and same_bits(logits1, logits0)
    assert torch.isfinite(logits1.float()).all()
    del model
    torch.cuda.empty_cache()
