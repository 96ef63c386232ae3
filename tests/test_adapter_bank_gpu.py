"""Adapter bank on the GPU: the per-row LoRA kernels (p3v_lora_down_rows / p3v_lora_up_rows) against the fp32 formula of
LoRALinear.__call__ (phi.py:129-133), their independence properties bit for bit, the model with a bank against the live CPU
oracle (every row against its own B = 1 oracle run), replays after a change of the row table without a recapture, the 4-bit
weight format, and the continuous engine + HTTP handler against tests/golden/tiny_adapters_oracle.npz."""
import json
import os
import threading

import numpy as np
import pytest
import torch

from gen_golden_adapters import ASSIGN, VARIANTS, fixture_adapter, synth_adapter, ALL_TARGETS

pytestmark = pytest.mark.gpu
BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
HERE = os.path.dirname(os.path.abspath(__file__))


def g(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(BF16)


def close(got, ref, rtol, atol):
    got, ref = got.float().cpu(), ref.float().cpu()
    err = (got - ref).abs()
    assert (err <= atol + rtol * ref.abs()).all(), f"max err {err.max():.5f} at |ref| {ref.abs().flatten()[err.argmax()]:.4f}"


def assert_logits(got, ref, what="", rel_atol=2e-2):
    """tests/test_model_gpu.py's logit bound, with the 2 % of its LoRA test (an adapted o_proj runs on the fp32 attention output in
    the reference; here the attention output and the frozen projection are already bf16 when the rank-r term is added)."""
    got, ref = got.float().cpu(), ref.float().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    atol = rel_atol * ref.abs().max().item()
    err = (got - ref).abs()
    tol = atol + 2e-2 * ref.abs()
    frac_bad = (err > tol).float().mean().item()
    assert frac_bad <= 1e-3 and (err <= 4 * tol).all(), \
        f"{what}: {frac_bad:.5f} outside tol; max err {err.max():.4f}, |ref|max {ref.abs().max():.3f}"
    return atol


def logits_differ(a, b, rel_atol=2e-2):
    """Fraction of entries of `a` outside assert_logits' tolerance around `b`."""
    a, b = a.float().cpu(), b.float().cpu()
    tol = rel_atol * b.abs().max().item() + 2e-2 * b.abs()
    return ((a - b).abs() > tol).float().mean().item()


# ------------------------------------------------------------------ kernels
RANKS = [1, 8, 64, 0]                                           # the four bank slots of the kernel tests


def make_bank(K, N, seed=0):
    """Four bank slots of ranks RANKS.  lora_b ~ N(0, 0.3 / sqrt(rank)): with unit-variance rows of x the rank-r term has a
    standard deviation of at most 0.5 at every rank, and v = bf16(y + term) with y ~ N(0, 0.5) stays below 4 in magnitude.  That is
    what makes test_lora_down_up's absolute bounds meaningful on millions of entries: the formula itself rounds v to bf16 before
    the residual is added, two correct fp32 evaluations of v may round to neighbouring bf16 values, and one bf16 step of |v| < 4
    (2^-6) is inside the 2e-2 the residual epilogue is given, whatever cancels in resid + v."""
    from phi_3_vision_mlx_amd import ops
    entries, host = [], []
    for s, r in enumerate(RANKS):
        if r == 0:
            entries.append(None), host.append(None)
            continue
        a = torch.randn((K, r), generator=torch.Generator().manual_seed(seed + 10 * s + 1)) * K ** -0.5
        b = torch.randn((r, N), generator=torch.Generator().manual_seed(seed + 10 * s + 2)) * 0.3 * r ** -0.5
        scale = 1.7 - 0.4 * s
        host.append((a, b, scale))
        entries.append((a.cuda(), b.cuda(), scale))
    return ops.lora_table(entries, "cuda:0"), host, entries     # (entries: keeps the device tensors alive)


def row_slots(M, seed=0):
    """Rows spread over all four slots and -1."""
    base = [0, 1, 2, 3, -1]
    perm = np.random.default_rng(seed).permutation(M)
    return [base[int(p) % 5] for p in perm]


def formula(x, y, host, slots, norm_w=None, eps=1e-5):
    """bf16(y + scale * ((h @ lora_a) @ lora_b)) in fp32 per row, h = x or ops.rmsnorm(x)."""
    h = x.float()
    v = y.float().clone()
    for m, s in enumerate(slots):
        if s >= 0 and host[s] is not None:
            a, b, scale = host[s]
            v[m] = y[m].float() + scale * ((h[m] @ a) @ b)
    return v.to(BF16)


def run_rows(ops, x, y, table, slots, K, epilogue, resid=None, norm_w=None, eps=1e-5):
    ra = torch.tensor(slots, dtype=I32, device="cuda:0")
    t = ops.lora_down_rows(x, table, ra, 64, norm_w=norm_w, norm_eps=eps)
    return ops.lora_up_rows(y, t, table, ra, K, 64, epilogue, resid=resid)


@pytest.mark.parametrize("K,N", [(3072, 9216), (3072, 3072), (3072, 16384), (8192, 3072)])
@pytest.mark.parametrize("M", [1, 5, 16, 32, 300])
def test_rows_kernels_match_formula(M, K, N):
    """Both launches against the fp32 formula on the real projections' shapes: three epilogues, a four-slot table with ranks
    {1, 8, 64, 0}, rows spread over all slots and -1, and the in-kernel norm against ops.rmsnorm followed by the formula.
    Tolerances: those of test_lora_down_up."""
    from phi_3_vision_mlx_amd import ops
    from phi_3_vision_mlx_amd.ops import EPI_NONE, EPI_RESID_BF16, EPI_SILU_MUL
    x, y, res = g((M, K), 100), g((M, N), 101, 0.5), g((M, N), 102)
    table, host, _keep = make_bank(K, N)
    slots = row_slots(M)
    xd, yd, rd = x.cuda(), y.cuda(), res.cuda()
    v = formula(x, y, host, slots)
    close(run_rows(ops, xd, yd, table, slots, K, EPI_NONE), v, rtol=2 ** -7, atol=1e-2)
    close(run_rows(ops, xd, yd, table, slots, K, EPI_RESID_BF16, resid=rd), (res.float() + v.float()).to(BF16), rtol=2 ** -7, atol=2e-2)
    gate, up = v[:, :N // 2], v[:, N // 2:]
    close(run_rows(ops, xd, yd, table, slots, K, EPI_SILU_MUL), gate * torch.sigmoid(gate) * up, rtol=2 ** -6, atol=2e-2)
    if K == 3072:                                               # the normed projections (qkv, gate_up) read the hidden state
        nw = (1 + 0.1 * torch.randn((K,), generator=torch.Generator().manual_seed(7))).to(BF16)
        h = ops.rmsnorm(xd, nw.cuda(), 1e-5)
        vn = formula(h.cpu(), y, host, slots)
        close(run_rows(ops, xd, yd, table, slots, K, EPI_NONE, norm_w=nw.cuda(), eps=1e-5), vn, rtol=2 ** -7, atol=1e-2)
        # and bit for bit what the un-normed launch gives on the materialised norm: the in-kernel norm IS p3v_rmsnorm's
        assert torch.equal(run_rows(ops, xd, yd, table, slots, K, EPI_NONE, norm_w=nw.cuda(), eps=1e-5),
                           run_rows(ops, h, yd, table, slots, K, EPI_NONE))


def test_rows_kernels_argument_checks():
    from phi_3_vision_mlx_amd import ops
    L = ops.L
    x, y = g((2, 256), 1).cuda(), g((2, 512), 2).cuda()
    table, _, _keep = make_bank(256, 512)
    ra = torch.tensor([0, -1], dtype=I32, device="cuda:0")
    t = torch.zeros((2, 1, 64), dtype=F32, device="cuda:0")
    out = torch.empty_like(y)
    p = lambda v: v.data_ptr()
    lib = L.lib()
    assert lib.p3v_lora_rows_slices(3072) == 12 and lib.p3v_lora_rows_slices(8192) == 32 and lib.p3v_lora_rows_slices(100) == 1
    for r_max in (0, 65):
        assert lib.p3v_lora_down_rows(p(x), 0, 0.0, p(table), p(ra), p(t), 2, 256, r_max, 4, 0) == -22
        assert lib.p3v_lora_up_rows(p(y), p(t), p(table), p(ra), 0, 0, p(out), 2, 512, 256, r_max, 4, 0) == -22
    assert lib.p3v_lora_down_rows(0, 0, 0.0, p(table), p(ra), p(t), 2, 256, 64, 4, 0) == -22
    assert lib.p3v_lora_down_rows(p(x), 0, 0.0, 0, p(ra), p(t), 2, 256, 64, 4, 0) == -22
    assert lib.p3v_lora_down_rows(p(x), 0, 0.0, p(table), 0, p(t), 2, 256, 64, 4, 0) == -22
    assert lib.p3v_lora_up_rows(p(y), p(t), p(table), 0, 0, 0, p(out), 2, 512, 256, 64, 4, 0) == -22
    assert lib.p3v_lora_up_rows(p(y), p(t), p(table), p(ra), ops.EPI_RESID_BF16, 0, p(out), 2, 512, 256, 64, 4, 0) == -22   # no resid
    assert lib.p3v_lora_down_rows(p(x), 0, 0.0, p(table), p(ra), p(t), 0, 256, 64, 4, 0) == 0                  # M = 0
    assert lib.p3v_lora_up_rows(p(y), p(t), p(table), p(ra), 0, 0, p(out), 0, 512, 256, 64, 4, 0) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("K,N,epi", [(3072, 9216, "none"), (8192, 3072, "resid"), (3072, 16384, "silu")])
def test_rows_kernels_independence_bit_exact(K, N, epi):
    """A row's output bits depend on its own input, its own entry and (K, N, epilogue) only: not on the other rows' slots, its
    position, M, or eager versus graph execution; a -1 row with the residual epilogue is bf16(resid + y)."""
    from phi_3_vision_mlx_amd import ops
    from phi_3_vision_mlx_amd.ops import EPI_NONE, EPI_RESID_BF16, EPI_SILU_MUL
    e = {"none": EPI_NONE, "resid": EPI_RESID_BF16, "silu": EPI_SILU_MUL}[epi]
    M = 300
    x, y, res = g((M, K), 200).cuda(), g((M, N), 201).cuda(), g((M, N), 202).cuda()
    nw = (1 + 0.1 * torch.randn((K,), generator=torch.Generator().manual_seed(8))).to(BF16).cuda() if K == 3072 else None
    table, host, _keep = make_bank(K, N, seed=50)
    slots = row_slots(M, seed=1)

    def run(xs, ys, rs, sl):
        return run_rows(ops, xs.contiguous(), ys.contiguous(), table, sl, K, e, resid=rs.contiguous() if e == EPI_RESID_BF16 else None, norm_w=nw)

    full = run(x, y, res, slots)
    probes = [slots.index(s) for s in (0, 1, 2, 3, -1)]         # one row per slot kind
    for m in probes:
        # other rows' slots permuted (this row keeps its own)
        other = list(np.random.default_rng(m).permutation(slots))
        other[m] = slots[m]
        assert torch.equal(run(x, y, res, other)[m], full[m])
        # the row on its own (M = 1), and at other positions of M = 5 / 32 calls
        assert torch.equal(run(x[m:m + 1], y[m:m + 1], res[m:m + 1], [slots[m]])[0], full[m])
        for M2, pos in ((5, 3), (32, 17)):
            idx = [(m + 1 + i) % M for i in range(M2)]
            idx[pos] = m
            sl = [slots[(i * 7) % M] for i in range(M2)]
            sl[pos] = slots[m]
            assert torch.equal(run(x[idx], y[idx], res[idx], sl)[pos], full[m]), (m, M2)
    if e == EPI_RESID_BF16:
        m = slots.index(-1)
        assert torch.equal(full[m], (res[m].float() + y[m].float()).to(BF16))
        m = slots.index(3)                                      # rank 0: the same
        assert torch.equal(full[m], (res[m].float() + y[m].float()).to(BF16))
    # eager versus a replayed capture; the replay follows the row table without a recapture
    xs, ys, rs = x[:16].contiguous(), y[:16].contiguous(), res[:16].contiguous()
    ra = torch.tensor(slots[:16], dtype=I32, device="cuda:0")
    t = torch.zeros((16, ops.lora_slices(K), 64), dtype=F32, device="cuda:0")
    out = torch.empty((16, N // 2 if e == EPI_SILU_MUL else N), dtype=BF16, device="cuda:0")

    def both():
        ops.lora_down_rows(xs, table, ra, 64, norm_w=nw, norm_eps=1e-5, out=t)
        ops.lora_up_rows(ys, t, table, ra, K, 64, e, resid=rs if e == EPI_RESID_BF16 else None, out=out)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        both()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            both()
    torch.cuda.current_stream().wait_stream(side)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, full[:16])
    new = list(reversed(slots[:16]))
    ra.copy_(torch.tensor(new, dtype=I32))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, run(xs, ys, rs, new))


# ------------------------------------------------------------------ model against the live oracle
def _tiny_bank_model(**kw):
    """The blind tiny model with the fixture adapters A and B in its bank, and one oracle per variant."""
    import phi3v_oracle as orc
    from phi_3_vision_mlx_amd.api import load_synthetic
    from phi_3_vision_mlx_amd.weights import resolve_adapter
    model, proc = load_synthetic(blind_model=True, tiny=True, seed=0, std_scale=4.0, device="cuda:0", **kw)
    ads = {n: resolve_adapter(model.cfg, *fixture_adapter(model.cfg, n)) for n in ("A", "B")}
    model.set_adapter_bank(ads)
    assert model.adapter_names == ["A", "B"]
    w = {k: v.cpu() for k, v in model.w.items()}
    oracles = {n: orc.OraclePhi3V(model.cfg, w, cache_fp32=True, adapters=ads.get(n)) for n in (None, "A", "B")}
    return model, proc, oracles


def test_bank_model_matches_oracle_rows_and_follows_row_table_without_recapture():
    """B = 4 batch with rows [A, none, B, A]: prefill, one eager cached call, graph-replayed steps, teacher-forced with the oracle's
    tokens; each row against its own B = 1 oracle run.  Then the row table changes to [none, B, A, none] between two replays: the
    same graph objects serve it, and the next step matches the oracle for the NEW assignment on the cache the old one built."""
    import phi3v_oracle as orc
    model, _, oracles = _tiny_bank_model()
    rows = ["A", None, "B", "A"]
    ids = np.random.default_rng(21).integers(3, 32000, (4, 33)).astype(np.int64)
    n = 5
    # every variant's own B = 1 oracle run of every row's prompt (rows 0 and 3 share an adapter, not a prompt)
    pre = {v: [oracles[v](input_ids=ids[r:r + 1], max_tokens=n + 2) for r in range(4)] for v in (None, "A", "B")}
    for r in range(4):                                          # the variants are far apart by this test's own yardstick:
        for a, b in ((None, "A"), (None, "B"), ("A", "B")):    # no pair passes assert_logits at the prefill step
            for u, v in ((a, b), (b, a)):
                frac = logits_differ(pre[u][r][0][:, -1], pre[v][r][0][:, -1])
                print(f"row {r}: oracle {u} vs {v}: {frac:.3f} of the prefill logits outside the tolerance")
                assert frac > 1e-3, (r, u, v, frac)
                with pytest.raises(AssertionError):
                    assert_logits(pre[u][r][0][:, -1], pre[v][r][0][:, -1])
    ref_lg = [[pre[rows[r]][r][0][:, -1]] for r in range(4)]   # per row: [step] -> logits [1, V]
    caches = [pre[rows[r]][r][1] for r in range(4)]
    ref_tok = [[] for _ in range(4)]
    for step in range(n - 1):
        for r in range(4):
            tok = torch.argmax(ref_lg[r][step].float(), dim=-1)[:, None]
            ref_tok[r].append(tok)
            lg, caches[r] = oracles[rows[r]](input_ids=tok, cache=caches[r])
            ref_lg[r].append(lg[:, -1])
    logits, cache = model(input_ids=ids, max_tokens=n + 2, row_adapters=rows)
    st = cache[0].state
    for step in range(n):
        for r in range(4):
            assert_logits(logits[r:r + 1, -1], ref_lg[r][step], f"bank row {r} ({rows[r]}) step {step}")
        if step + 1 < n:
            tok = torch.cat([ref_tok[r][step] for r in range(4)]).to("cuda:0", torch.int32)
            if step == 0:
                logits, cache = model(input_ids=tok, cache=cache)            # eager cached call
            else:
                logits, _ = model.greedy_step(tok, cache)                   # graph replay
    graphs = dict(st.graphs)
    graph_obj = st.graphs["greedy"]["graph"]
    # a new assignment on the caches the old one built: hand row r's oracle cache to the oracle that carries r's new adapter
    new_rows = [None, "B", "A", None]
    model.set_row_adapters(st, new_rows)
    tok = torch.cat([torch.argmax(ref_lg[r][n - 1].float(), dim=-1)[:, None] for r in range(4)])
    logits, _ = model.greedy_step(tok.to("cuda:0", torch.int32), cache)
    assert st.graphs["greedy"]["graph"] is graph_obj and all(st.graphs[k] is v for k, v in graphs.items()) and len(st.graphs) == len(graphs)
    told_apart = 0
    for r in range(4):
        lg_old, _ = oracles[rows[r]](input_ids=tok[r:r + 1], cache=caches[r])      # what the OLD adapter would give on this step
        for c in caches[r]:
            c.offset -= 1
        lg, _ = oracles[new_rows[r]](input_ids=tok[r:r + 1], cache=caches[r])
        assert_logits(logits[r:r + 1, -1], lg[:, -1], f"row {r} after {rows[r]} -> {new_rows[r]}")
        apart = logits_differ(lg[:, -1], lg_old[:, -1])
        print(f"row {r}: {rows[r]} -> {new_rows[r]}: oracle old vs new {apart:.3f} outside the tolerance")
        if apart > 1e-3:                                        # (the oracle alone says the two are distinguishable here)
            told_apart += 1
            assert logits_differ(logits[r:r + 1, -1], lg_old[:, -1]) > 1e-3, f"row {r} still runs its old adapter"
    assert told_apart >= 1


def test_bank_on_4bit_weights_matches_dequantised_model_with_set_adapters():
    """Format coverage (a cross-check between kernel families, not an oracle pin): a full-width 2-layer model on MLX 4-bit
    weights with a bank {A', B'} and a mixed B = 4 batch, against a bf16 model built from the dequantised weights that carries
    each row's adapter through the existing set_adapters path at B = 1.  Tolerances: those of
    test_int4_weights_full_size_decode_matches_dequantised_model."""
    from phi_3_vision_mlx_amd import ops
    from phi_3_vision_mlx_amd.api import load_synthetic
    from phi_3_vision_mlx_amd.model import Phi3VModel
    from phi_3_vision_mlx_amd.weights import resolve_adapter
    mq, _ = load_synthetic(blind_model=True, tiny=False, seed=0, device="cuda:0", num_hidden_layers=2, quantized_int4=True)
    assert mq.w4 and not any(k.endswith("_proj.weight") for k in mq.w)
    wd = dict(mq.w)
    for k, (w4, sb) in mq.w4.items():
        wd[k] = ops.dequant_q4(w4, sb)
    cfg = type(mq.cfg)(**{k: v for k, v in vars(mq.cfg).items() if k != "quantized_int4"})
    md = Phi3VModel(cfg, wd, device="cuda:0")
    ads = {n: resolve_adapter(mq.cfg, *fixture_adapter(mq.cfg, n)) for n in ("A", "B")}
    mq.set_adapter_bank(ads)
    rows = ["A", None, "B", "A"]
    ids = np.random.default_rng(5).integers(3, 32000, (4, 40)).astype(np.int64)
    n = 4
    ref_lg, ref_tok = [], []
    plain = None
    for r, name in enumerate(rows):                             # each row alone, its adapter attached the old way
        md.set_adapters(ads[name] if name else {})
        lg, cd = md(input_ids=ids[r:r + 1], max_tokens=n + 1)
        lgs, toks = [lg[:, -1].clone()], []
        for _ in range(n):
            tok = ops.argmax(lgs[-1].contiguous())[:, None]
            toks.append(tok.clone())
            lg, _ = md.greedy_step(tok, cd)
            lgs.append(lg[:, -1].clone())
        ref_lg.append(lgs), ref_tok.append(toks)
        if r == 0:
            md.set_adapters({})
            plain = md(input_ids=ids[:1], max_tokens=1)[0][:, -1]
    assert (ref_lg[0][0].float() - plain.float()).abs().max().item() > 0.05          # the adapter is live at this size
    lq, cq = mq(input_ids=ids, max_tokens=n + 1, row_adapters=rows)
    for r in range(4):
        assert_logits(lq[r:r + 1, -1], ref_lg[r][0], f"int4 bank prefill row {r}", rel_atol=1.5e-2)
    for step in range(n):
        tok = torch.cat([ref_tok[r][step] for r in range(4)])
        lq, _ = mq.greedy_step(tok, cq)
        for r in range(4):
            assert_logits(lq[r:r + 1, -1], ref_lg[r][step + 1], f"int4 bank decode step {step} row {r}", rel_atol=6e-2)
    del mq, md
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ engine and HTTP handler against the fixture
def _fixture():
    g = np.load(os.path.join(HERE, "golden", "tiny_adapters_oracle.npz"))
    assert [VARIANTS[i] for i in g["assign"]] == ASSIGN
    return g


def _serve_model():
    from golden_inputs import SERVE_TEXTS
    g = _fixture()
    model, proc, _ = _tiny_bank_model(lm_head_spread=float(g["spread"][0]), lm_head_seed=int(g["head_seed"][0]))
    reqs = [proc(t) for t in SERVE_TEXTS[1:]]
    names = [None if n == "none" else n for n in ASSIGN]
    return g, model, proc, reqs, names


def tokens_vs_assigned(got, g, what, budgets=None, min_first=1):
    """tests/test_serving_gpu.py's rule (tokens_vs_fixture) on each request's ASSIGNED run: token by token up to the run's first
    unclear step; then every stored witness inside the budget: the tokens differ from the OTHER variant's at the witness step."""
    n = 0
    for i, toks in enumerate(got):
        a = int(g["assign"][i])
        ref, clear = g["tokens"][i, a], g["margins"][i, a] > 1.0
        assert clear[:min_first].all(), f"{what}: fixture request {i} is not clear on its first step(s)"
        budget = len(ref) if budgets is None else budgets[i]
        assert len(toks) <= budget
        for step in range(min(len(ref), budget)):
            if not clear[step]:
                break
            assert step < len(toks), f"{what}: request {i} stopped after {len(toks)} tokens, oracle continues {ref.tolist()}"
            assert toks[step] == int(ref[step]), f"{what}: request {i} ({ASSIGN[i]}) step {step}: {toks} != oracle {ref.tolist()}"
            n += 1
            if toks[step] == 32007:
                break
    seen = 0
    for i, a, b, s_ in g["witnesses"].tolist():
        if i < len(got) and s_ < (len(g["tokens"][i, a]) if budgets is None else budgets[i]):
            assert got[i][s_] != int(g["tokens"][i, b, s_]), f"{what}: request {i} step {s_} equals the {VARIANTS[b]} run, not its own {VARIANTS[a]}"
            seen += 1
    return n, seen


def test_engine_rows_with_different_adapters_share_steps_and_match_the_fixture():
    """3 slots, the six requests with ASSIGN = [A, none, B, B, none, A]; the last three arrive mid-flight and two early ones have
    short budgets, so a row is refilled by a request with a different adapter and by one with none.  Free-running tokens ==
    each request's assigned B = 1 oracle run, and differ from the other variants' at the fixture's witness steps."""
    from golden_inputs import SERVE_STEPS
    from phi_3_vision_mlx_amd.engine import ContinuousEngine
    g, model, proc, reqs, names = _serve_model()
    writes = []
    real = model.set_row_adapters
    model.set_row_adapters = lambda st, ad, row0=0: (writes.append((row0, list(ad))), real(st, ad, row0))[1]
    eng = ContinuousEngine(model, proc, slots=3, window=4096)
    budgets = [2, SERVE_STEPS, 3, SERVE_STEPS, SERVE_STEPS, SERVE_STEPS]
    handles = [eng.submit(r, b, adapter=a) for r, b, a in zip(reqs[:3], budgets, names)]
    for _ in range(2):
        eng.step()
    graph = model.decode_graph(eng.st)["graph"]
    handles += [eng.submit(r, b, adapter=a) for r, b, a in zip(reqs[3:], budgets[3:], names[3:])]
    bad = eng.submit(reqs[0], 3, adapter="nope")               # unknown name: fails at once, nothing queued, nobody disturbed
    assert bad.done.is_set() and isinstance(bad.error, ValueError) and "A" in str(bad.error) and bad not in eng.waiting
    eng.run_until_idle()
    assert all(h.done.is_set() and h.error is None for h in handles)
    assert eng.joined_mid_flight >= 2 and eng.steps < sum(budgets) and eng.failures == 0
    assert model.decode_graph(eng.st)["graph"] is graph         # one captured step served every assignment
    history = {}
    for row0, ad in writes:
        for i, a in enumerate(ad):
            history.setdefault(row0 + i, []).append(a)
    swaps = [(h[i], h[i + 1]) for h in history.values() for i in range(len(h) - 1)]
    assert any(b is not None and a != b for a, b in swaps), history          # refilled with a different adapter
    assert any(a is not None and b is None for a, b in swaps), history       # and with none
    n, seen = tokens_vs_assigned([h.tokens for h in handles], g, "engine", budgets)
    assert n >= 12 and seen >= 6, (n, seen)
    print(f"adapter engine: {n} free-running tokens equal the assigned runs, {seen} witnesses told the variants apart; rows {history}")


def _http(port, path, body=None, timeout=300):
    import urllib.request
    req = urllib.request.Request(f"http://127.0.0.1:{port}{path}", data=None if body is None else json.dumps(body).encode(),
                                 headers={"Content-Type": "application/json"})
    with urllib.request.urlopen(req, timeout=timeout) as r:
        return json.loads(r.read())


class IdTokenizer:
    """Delegates encoding to the real tokenizer; decodes to the ids themselves so HTTP responses can be compared as tokens."""

    def __init__(self, real):
        self.real = real

    def __call__(self, *a, **kw):
        return self.real(*a, **kw)

    def encode(self, *a, **kw):
        return self.real.encode(*a, **kw)

    def decode(self, ids, **kw):
        return " ".join(str(int(i)) for i in ids)

    def batch_decode(self, seqs, **kw):
        return [self.decode(s) for s in seqs]


def test_http_handler_serves_the_adapter_field():
    """POST /v1/completions with "adapter" (a string, a list with nulls) from concurrent clients -> one engine, one bank: every
    response == its assigned oracle run; an unknown name is a 400 naming the known adapters; GET /v1/adapters lists them."""
    import urllib.error
    from golden_inputs import SERVE_PROMPTS, SERVE_STEPS
    from phi_3_vision_mlx_amd.engine import ContinuousEngine
    from phi_3_vision_mlx_amd.server import serve_continuous
    g, model, proc, _, names = _serve_model()
    proc.tokenizer = IdTokenizer(proc.tokenizer)
    httpd, backend = serve_continuous(ContinuousEngine(model, proc, slots=2, window=4096), port=0)
    threading.Thread(target=httpd.serve_forever, daemon=True).start()
    port, got = httpd.server_address[1], {}
    P = SERVE_PROMPTS[1:]
    bodies = [{"prompt": P[0:3], "adapter": names[0:3], "max_tokens": SERVE_STEPS},
              {"prompt": P[3], "adapter": names[3], "max_tokens": SERVE_STEPS},
              {"prompt": P[4:6], "adapter": names[4:6], "max_tokens": SERVE_STEPS}]
    try:
        ths = [threading.Thread(target=lambda i=i, b=b: got.__setitem__(i, _http(port, "/v1/completions", b))) for i, b in enumerate(bodies)]
        [t.start() for t in ths]
        [t.join() for t in ths]
        assert _http(port, "/v1/adapters")["adapters"] == ["A", "B"]
        for bad in ("C", 7, ["A"]):                            # unknown name, wrong type, wrong count (two prompts)
            with pytest.raises(urllib.error.HTTPError) as e:
                _http(port, "/v1/completions", {"prompt": P[0:2], "adapter": bad, "max_tokens": 2})
            assert e.value.code == 400 and "'A', 'B'" in json.loads(e.value.read())["error"]
        again = _http(port, "/v1/completions", {"prompt": P[0], "max_tokens": 2})         # the engine is still fine, base model
    finally:
        httpd.shutdown()
        backend.close()
    texts = got[0]["responses"] + got[1]["responses"] + got[2]["responses"]
    toks = [[int(t) for t in s.split()] for s in texts]
    n, seen = tokens_vs_assigned(toks, g, "HTTP")
    assert n >= 12 and seen == len(g["witnesses"]), (n, seen)
    assert int(again["responses"][0].split()[0]) == int(g["tokens"][0, 0, 0]) and g["margins"][0, 0, 0] > 1.0


def test_sampling_and_adapters_together():
    """One sampled request with adapter A next to a greedy one without: the sampled row reproduces under its returned seed (alone,
    beside a row that now carries adapter B), the greedy row still equals its fixture run."""
    from golden_inputs import SERVE_STEPS
    from phi_3_vision_mlx_amd.engine import ContinuousEngine
    g, model, proc, reqs, names = _serve_model()
    eng = ContinuousEngine(model, proc, slots=2, window=4096)
    hs = eng.submit(reqs[0], SERVE_STEPS, sampling={"temperature": 0.9, "top_k": 50, "top_p": 0.95}, adapter="A")
    hg = eng.submit(reqs[1], SERVE_STEPS)
    eng.run_until_idle()
    assert hs.error is None and hg.error is None and hs.adapter == "A"
    seed = hs.sampling[3]
    ref, clear = g["tokens"][1, 0], g["margins"][1, 0] > 1.0
    for step in range(SERVE_STEPS):
        if not clear[step]:
            break
        assert hg.tokens[step] == int(ref[step]), (step, hg.tokens, ref.tolist())
    again = eng.submit(reqs[0], SERVE_STEPS, sampling={"temperature": 0.9, "top_k": 50, "top_p": 0.95, "seed": seed}, adapter="A")
    other = eng.submit(reqs[1], SERVE_STEPS, adapter="B")      # (the same geometry as before, another adapter beside it)
    eng.run_until_idle()
    assert again.error is None and other.error is None
    assert again.tokens == hs.tokens, (again.tokens, hs.tokens)
    assert eng.failures == 0


def test_api_generate_takes_an_adapter_per_prompt():
    """api.generate on a left-padded batch of three prompts with adapter=[A, None, B], and on one prompt with adapter="B": each row's
    tokens == its assigned fixture run (and differ from the other variants' at the witness steps); an unknown name is refused
    before anything runs."""
    from golden_inputs import SERVE_PROMPTS, SERVE_STEPS
    from phi_3_vision_mlx_amd import api
    g, model, proc, _, names = _serve_model()
    proc.tokenizer = IdTokenizer(proc.tokenizer)
    texts = api.generate(SERVE_PROMPTS[1:4], preload=(model, proc), max_tokens=SERVE_STEPS, verbose=False, stream=False, adapter=names[:3])
    n, seen = tokens_vs_assigned([[int(t) for t in s.split()] for s in texts], g, "api.generate batch")
    assert n >= 6 and seen >= 3, (n, seen)
    one = api.generate(SERVE_PROMPTS[3], preload=(model, proc), max_tokens=SERVE_STEPS, verbose=False, stream=False, adapter="B")
    one = one[0] if isinstance(one, list) else one
    toks = [int(t) for t in one.split()]
    ref, clear = g["tokens"][2, 2], g["margins"][2, 2] > 1.0
    for step in range(SERVE_STEPS):
        if not clear[step]:
            break
        assert toks[step] == int(ref[step]), (step, toks, ref.tolist())
    with pytest.raises(ValueError, match="unknown adapter"):
        api.generate(SERVE_PROMPTS[1], preload=(model, proc), max_tokens=2, verbose=False, adapter="C")


def test_server_cli_with_two_adapter_flags_serves_interleaved_requests(tmp_path):
    """`python -m phi_3_vision_mlx_amd.server --continuous --adapter A=DIR --adapter B=DIR` on the tiny synthetic text model, the
    adapters read from files in the reference's format: GET /v1/adapters lists both; interleaved concurrent requests for A, B and
    the base model (every one twice) all come back 200 from the one engine, the same (prompt, adapter) gives the same text, an
    unknown name is a 400.  (What each variant must answer is pinned by the fixture tests above; here the CLI path is exercised.)"""
    import signal
    import socket
    import subprocess
    import sys
    import time
    import urllib.error
    from phi_3_vision_mlx_amd.config import make_config, tiny_config_dict
    from phi_3_vision_mlx_amd.weights import save_adapter
    root = os.path.dirname(HERE)
    cfg = make_config(tiny_config_dict(vision=False))
    for name in ("A", "B"):
        save_adapter(str(tmp_path / name), *fixture_adapter(cfg, name))
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    log = open(tmp_path / "server.log", "w")
    proc = subprocess.Popen([sys.executable, "-m", "phi_3_vision_mlx_amd.server", "--continuous", "--synthetic", "--tiny", "--blind",
                             "--port", str(port), "--slots", "3", "--adapter", f"A={tmp_path / 'A'}", "--adapter", f"B={tmp_path / 'B'}"],
                            cwd=root, stdout=log, stderr=subprocess.STDOUT, start_new_session=True)
    try:
        deadline = time.time() + 240
        while True:                                            # wait for the listener (the model and the bank load first)
            assert proc.poll() is None, open(tmp_path / "server.log").read()[-2000:]
            try:
                socket.create_connection(("127.0.0.1", port), timeout=1).close()
                break
            except OSError:
                assert time.time() < deadline, open(tmp_path / "server.log").read()[-2000:]
                time.sleep(0.5)
        assert _http(port, "/v1/adapters")["adapters"] == ["A", "B"]
        plan = [("A", "tell me about the weather"), (None, "tell me about the weather"), ("B", "tell me about the weather"),
                ("B", "and something else entirely, please"), (None, "hi"), ("A", "hi")] * 2
        out = [None] * len(plan)

        def one(i):
            body = {"prompt": plan[i][1], "max_tokens": 6}
            if plan[i][0] is not None:
                body["adapter"] = plan[i][0]
            out[i] = _http(port, "/v1/completions", body, timeout=120)
        threads = [threading.Thread(target=one, args=(i,)) for i in range(len(plan))]
        [t.start() for t in threads]
        [t.join(180) for t in threads]
        assert all(o is not None and isinstance(o["responses"][0], str) for o in out), out
        half = len(plan) // 2
        assert all(out[i]["responses"] == out[i + half]["responses"] for i in range(half)), out
        print("CLI server:", [(a, o["responses"][0]) for (a, _), o in zip(plan[:half], out)])
        with pytest.raises(urllib.error.HTTPError) as e:
            _http(port, "/v1/completions", {"prompt": "hi", "adapter": "C", "max_tokens": 2})
        assert e.value.code == 400 and "'A', 'B'" in json.loads(e.value.read())["error"]
    finally:
        os.killpg(proc.pid, signal.SIGTERM)
        try:
            proc.wait(30)
        except subprocess.TimeoutExpired:
            os.killpg(proc.pid, signal.SIGKILL)
        log.close()
