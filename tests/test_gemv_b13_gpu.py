"""bf16 weights as exact 13-bit codes (p3v_gemv_b13.hip): the packing is lossless or refused, and everything
computed from the packed copy is BIT-IDENTICAL to the same computation on the bf16 matrix.  Every comparison is torch.equal."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF16, F32, I16, I32 = torch.bfloat16, torch.float32, torch.int16, torch.int32
E_TOP = 127                                  # the window of these tests: biased exponents 97 .. 127 (2^-30 .. 1), 31 binades


@pytest.fixture(scope="module")
def ops():
    from phi_3_vision_mlx_amd import ops as o
    o.L.lib()
    return o


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
    block = torch.cat([pats[torch.randperm(pats.numel(), generator=gen)] for _ in range(16)])[:-1].to(I16)   # (0x8000.. wraps onto the sign)
    return block.repeat(-(-n // block.numel()))[:n].view(BF16).reshape(rows, K).contiguous()


def same_bits(a, b):
    return torch.equal(a.view(I16), b.view(I16))


@pytest.mark.parametrize("rows,K", [(8, 3072), (2, 8192)])
@pytest.mark.parametrize("silu_pairs", [False, True])
def test_round_trip_is_bit_exact(ops, rows, K, silu_pairs):
    w = window_matrix(rows, K, 1).cuda()
    assert set(every_pattern().tolist()) <= set((w.view(I16).to(I32) & 0xffff).reshape(-1).tolist())
    pk = ops.pack_b13(w, silu_pairs=silu_pairs)
    assert pk is not None and pk.base == E_TOP - 30
    assert pk.data.numel() == rows * K * 13 // 8
    assert same_bits(ops.unpack_b13(pk), w)


@pytest.mark.parametrize("rows,K", [(8, 3072), (2, 8192)])
def test_what_does_not_fit_is_refused(ops, rows, K):
    base = window_matrix(rows, K, 2)
    assert ops.pack_b13(base.cuda()) is not None
    below = (E_TOP - 31) << 7                                         # the 32nd binade under the largest exponent
    for name, bits in (("below the window", below), ("denormal", 0x0001), ("inf", 0x7f80), ("nan", 0x7fc0)):
        for pos in ((0, 0), (rows - 1, K - 1)):
            w = base.clone()
            w.view(I16)[pos] = bits
            assert ops.pack_b13(w.cuda()) is None, (name, pos)
    w = base.clone()                                                  # an all-zero matrix fits (every code 0)
    w.zero_()
    pk = ops.pack_b13(w.cuda())
    assert pk is not None and same_bits(ops.unpack_b13(pk), w.cuda())


@pytest.fixture(scope="module")
def gemv_case():
    """K -> (x [1, K], norm weight, 8204 weight rows spanning the whole window with zeros and both signs), on the device; built once."""
    cache = {}

    def get(K):
        if K not in cache:
            cache[K] = (g((1, K), 10 + K).cuda(), (1 + 0.1 * g((K,), 11 + K)).cuda(), window_matrix(2 * 4102, K, 12 + K).cuda())
        return cache[K]
    yield get
    cache.clear()


@pytest.mark.parametrize("epi", ["none", "norm_silu", "resid"])
@pytest.mark.parametrize("N", [2, 3072, 4102])
@pytest.mark.parametrize("K", [3072, 8192])
def test_gemv_is_the_bf16_gemv(ops, gemv_case, K, N, epi):
    x, nw, rows = gemv_case(K)
    if epi == "norm_silu":
        w = rows[:2 * N].contiguous()
        pk = ops.pack_b13(w, silu_pairs=True)
        kw = dict(epilogue=ops.EPI_SILU_MUL, norm_w=nw, norm_eps=1e-5)
    else:
        w = rows[:N].contiguous()
        pk = ops.pack_b13(w)
        kw = dict(epilogue=ops.EPI_RESID_BF16, resid=g((1, N), 13).cuda()) if epi == "resid" else {}
    assert pk is not None
    ref = ops.gemv(x, w, **kw)
    out = ops.gemv_b13(x, pk, **kw)
    assert ref.shape == (1, N) and same_bits(out, ref)
    assert torch.isfinite(ref.float()).all() and ref.float().abs().max() > 0


@pytest.mark.parametrize("K", [3072, 8192])
def test_step_folds_are_the_bf16_step_folds(ops, K):
    """p3v_gemv_b13_step against p3v_gemv_step on the same weights: begin (embedding gather + rotation rows in the first projection)
    and end (arg-max + bookkeeping in the vocabulary head, N = 4102: a tie for the first maximum, a NaN row reporting -1)."""
    B, V, T, half, steps, N1 = 1, 4102, 40, 48, 4, 1024
    table = g((V, K), 70).cuda()
    cos, sin = torch.rand((B, T, half), dtype=F32).cuda(), torch.rand((B, T, half), dtype=F32).cuda()
    w1, nw1 = window_matrix(N1, K, 71).cuda(), (1 + 0.1 * g((K,), 72)).cuda()
    p1 = ops.pack_b13(w1)
    tok = torch.tensor([V + 5 if K == 8192 else 4004], dtype=I32).cuda()
    d_past = torch.tensor([11], dtype=I32).cuda()
    x_a, x_b = torch.empty((B, K), dtype=BF16).cuda(), torch.full((B, K), 7.0, dtype=BF16).cuda()
    ca, sa = torch.empty((B, 1, half), dtype=F32).cuda(), torch.empty((B, 1, half), dtype=F32).cuda()
    cb, sb = torch.zeros_like(ca), torch.zeros_like(sa)
    out_a, out_b = (torch.full((B, N1), float("nan"), dtype=BF16).cuda() for _ in range(2))
    assert ops.gemv_step_begin(tok, table, x_a, cos, sin, d_past, ca, sa, w1, nw1, 1e-5, out_a)
    assert ops.gemv_step_begin(tok, table, x_b, cos, sin, d_past, cb, sb, p1, nw1, 1e-5, out_b)
    assert same_bits(out_a, out_b) and torch.equal(x_a, x_b) and torch.equal(ca, cb) and torch.equal(sa, sb)
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
        assert same_bits(lg_a, lg_b)
        assert torch.equal(nx_a, nx_b) and torch.equal(to_a, to_b), (s, nx_a.tolist(), nx_b.tolist())
        assert st_b.item() == s + 1 and pb.item() == 12 + s and st_a.item() == st_b.item() and pa.item() == pb.item()
        if s in (1, 2):
            assert lg_b[0, 300].item() == lg_b[0, 3000].item() == lg_b.float().max().item() and nx_b[0].item() == 300
        if s == 3:
            assert nx_b[0].item() == -1
    assert torch.equal(hist_a, hist_b)
    # more than one row is not the fold's shape: nothing launched, the caller keeps the bf16 launches
    assert not ops.gemv_step_end(g((2, K), 1).cuda(), pl, nwl, 1e-5, torch.empty((2, V), dtype=BF16).cuda(), nx_b, to_b, hist_b, st_b, pb, tk_b, ws_b)
    assert st_b.item() == steps + 1


def _decode8(model, ids):
    logits, cache = model(input_ids=ids, max_tokens=16)
    token = logits[:, -1, :].float().argmax(dim=-1, keepdim=True)
    toks, last = [], None
    for _ in range(8):
        last, token = model.greedy_step(token, cache)
        toks.append(token.reshape(-1).tolist())
    torch.cuda.synchronize()
    st = cache[0].state
    assert "graph" in st.graphs["greedy"]                         # the steps above were graph replays
    return toks, last.detach().clone().view(-1)


def test_model_decodes_the_same_tokens_and_logits(monkeypatch):
    """Full hidden size (3072 / 8192 / 32064), two layers, a text-only 40-token prompt, 8 greedy tokens through the replayed graph:
    P3V_PACK13=0 against the default, and the same again with a value far below its matrix's window planted in one matrix (that
    matrix is refused and stays bf16)."""
    from phi_3_vision_mlx_amd.api import load_synthetic
    ids = torch.randint(3, 32000, (1, 40), dtype=torch.int64, generator=torch.Generator().manual_seed(6))
    layers, k = 2, "model.layers.1.mlp.down_proj.weight"

    def plant(model):
        model.w[k].view(I16)[5, 7] = 40 << 7                     # 2^-87, written in place

    monkeypatch.setenv("P3V_PACK13", "0")
    model, _ = load_synthetic(blind_model=True, tiny=False, seed=0, device="cuda:0", num_hidden_layers=layers)
    assert model.w13 == {}
    ref = _decode8(model, ids)
    plant(model)
    ref_planted = _decode8(model, ids)
    del model
    torch.cuda.empty_cache()

    monkeypatch.delenv("P3V_PACK13")
    model, _ = load_synthetic(blind_model=True, tiny=False, seed=0, device="cuda:0", num_hidden_layers=layers)
    assert len(model.w13) == 3 * layers + 1 and not any("o_proj" in key for key in model.w13)
    toks, logits = _decode8(model, ids)
    assert len(model.w13) == 3 * layers + 1                       # (none was dropped on the way: the packed path ran)
    assert toks == ref[0] and same_bits(logits, ref[1])

    plant(model)
    model.repack_b13()                                            # what a caller does after writing to decoder weights
    assert k not in model.w13 and len(model.w13) == 3 * layers    # the planted matrix is refused, the others are packed again
    toks, logits = _decode8(model, ids)
    assert len(model.w13) == 3 * layers
    assert toks == ref_planted[0] and same_bits(logits, ref_planted[1])
    del model
    torch.cuda.empty_cache()
