"""p3v_embed_pool and p3v_sim_topk (csrc/p3v_embed.hip) against plain fp64 on the probing inputs of tests/embed_probe.py, under its
acceptance rules: every element inside its interval, exact indices, memory outside the outputs bit-identical, a second launch
bit-identical, a row's bits independent of its batch, of N and of Q.  tests/test_embed_probe_cpu.py shows on the references alone
that a kernel with a leaking pad row, a dropped row, a wrong tie-break, ... cannot pass here.  Every case prints
`id [family]: kernel: result`; tools/proj_probe_parity.py turns those lines into profiles/embed_probe_parity.txt."""
import numpy as np
import pytest
import torch

import embed_probe as ep

pytestmark = pytest.mark.gpu

ids = lambda c: c.id
G = ep.GUARD


@pytest.fixture(scope="module")
def ops():
    from phi_3_vision_mlx_amd import ops as o
    o.L.lib()
    return o


def _guarded(shape, dtype, fill):
    """(flat buffer with GUARD sentinel elements either side, the view between them, a host copy of the buffer)."""
    n = int(np.prod(shape))
    flat = torch.full((n + 2 * G,), fill, dtype=dtype, device="cuda")
    flat[:G] = torch.arange(G, device="cuda").to(dtype) + 3
    flat[n + G:] = torch.arange(G, device="cuda").to(dtype) + 5
    return flat, flat[G:G + n].view(shape), flat.cpu().clone()


def _guards_intact(flat, before):
    now = flat.cpu()
    return torch.equal(now[:G], before[:G]) and torch.equal(now[-G:], before[-G:])


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("case", ep.POOL_CASES, ids=ids)
def test_embed_pool_in_rule(ops, case):
    pr = ep.pool_probe(case)
    x, w, start = pr.x.cuda(), pr.w.cuda(), pr.start.cuda()
    for mode in (ep.POOL_LAST, ep.POOL_MEAN):
        for nz in (False, True):
            flat, out, before = _guarded((case.B, case.H), torch.float32, -7.0)
            ops.embed_pool(x, w, ep.EPS, start, mode, nz, out=out)
            got = out.clone()
            msg, frac = pr.verify(got.cpu(), mode, nz)
            print(f"{case.id} [{mode}{'-norm' if nz else ''}]: k_pool_rstd + k_pool_sum{' + k_pool_l2' if nz else ''}: "
                  + (msg or f"worst excursion outside the bracket {frac:.3f} x E"))
            assert msg == "", msg
            assert _guards_intact(flat, before)
            ops.embed_pool(x, w, ep.EPS, start, mode, nz, out=out)
            assert torch.equal(_bits(out), _bits(got))                      # a second launch: the same bits
    assert torch.equal(x.cpu().view(torch.int16), pr.x.view(torch.int16))   # the input is left alone


@pytest.mark.parametrize("case", [c for c in ep.POOL_CASES if c.B == 16], ids=ids)
def test_embed_pool_row_is_a_function_of_its_own_input(ops, case):
    pr = ep.pool_probe(case)
    x, w, start = pr.x.cuda(), pr.w.cuda(), pr.start.cuda()
    for mode in (ep.POOL_LAST, ep.POOL_MEAN):
        full = ops.embed_pool(x, w, ep.EPS, start, mode, True)
        for b in (0, 1, 2, 7, 15):
            alone = ops.embed_pool(x[b:b + 1].contiguous(), w, ep.EPS, start[b:b + 1].contiguous(), mode, True)
            assert torch.equal(_bits(alone[0]), _bits(full[b])), (case.id, mode, b)


@pytest.mark.parametrize("case", [c for c in ep.POOL_CASES if c.H % 8 == 0 and c.B == 3], ids=ids)
def test_embed_pool_last_is_the_row_rmsnorm_writes(ops, case):
    pr = ep.pool_probe(case)
    x, w = pr.x.cuda(), pr.w.cuda()
    y = ops.rmsnorm(x[:, -1].contiguous(), w, ep.EPS).float()
    got = ops.embed_pool(x, w, ep.EPS, None, ep.POOL_LAST, False)
    live = ~torch.isnan(y)
    assert torch.equal(torch.isnan(got), ~live) and torch.equal(got[live], y[live])


def test_embed_pool_refuses_what_the_header_refuses(ops):
    x, w = torch.zeros((2, 3, 64), dtype=torch.bfloat16, device="cuda"), torch.ones((64,), dtype=torch.bfloat16, device="cuda")
    with pytest.raises(ValueError, match="'last' or 'mean'"):
        ops.embed_pool(x, w, ep.EPS, None, "max")
    with pytest.raises(RuntimeError):
        ops.embed_pool(x[:, :, :62].contiguous(), w[:62].contiguous(), ep.EPS)
    with pytest.raises(ValueError):
        ops.embed_pool(x, w, ep.EPS, torch.zeros((3,), dtype=torch.int32, device="cuda"), "mean")
    assert float(ops.embed_pool(x, w, ep.EPS, None, "mean", True).abs().max()) == 0.0       # zero rows stay zero


def _run_sim(ops, pr, n=None, queries=None, k=None):
    case = pr.case
    q = pr.queries if queries is None else queries
    k = case.k if k is None else k
    fi, idx, bi = _guarded((q.shape[0], k), torch.int32, -9)
    fs, score, bs = _guarded((q.shape[0], k), torch.float32, -9.0)
    index = pr.index.cuda() if pr.index.shape[0] else torch.zeros((0, case.D), dtype=torch.bfloat16, device="cuda")
    ops.sim_topk(index, q.cuda(), k, n=n, out=(idx, score))
    assert _guards_intact(fi, bi) and _guards_intact(fs, bs)
    return idx.clone(), score.clone()


@pytest.mark.parametrize("case", ep.SIM_CASES, ids=ids)
def test_sim_topk_in_rule(ops, case):
    pr = ep.sim_probe(case)
    idx, score = _run_sim(ops, pr)
    msg, frac = pr.verify(idx.cpu().numpy(), score.cpu().numpy())
    what = "indices and scores equal the reference" if case.family == ep.GRID else f"indices equal, worst |score - ref| {frac:.3f} x E"
    print(f"{case.id} [{case.family}]: k_sim_topk + k_sim_merge: {msg or what}")
    assert msg == "", msg
    idx2, score2 = _run_sim(ops, pr)
    assert torch.equal(idx, idx2) and torch.equal(_bits(score), _bits(score2))


def test_sim_topk_rows_beyond_n_are_not_read(ops):
    """N is a launch argument: rows past it hold NaN and a row that would win."""
    pr = ep.sim_probe(ep.SimCase(ep.GRID, 1000, 3, 8, 64))
    index = torch.cat([pr.index, torch.full((50, 64), float("nan"), dtype=torch.bfloat16), pr.index[:1] * 4]).cuda()
    idx, score = ops.sim_topk(index, pr.queries.cuda(), 8, n=1000)
    assert pr.verify(idx.cpu().numpy(), score.cpu().numpy())[0] == ""


def test_sim_topk_score_bits_do_not_depend_on_n_or_q(ops):
    pr = ep.sim_probe(ep.SimCase(ep.PLANTED, 4099, 16, 32, 3072))
    idx, score = _run_sim(ops, pr)
    for q in (0, 5, 15):                                                    # Q = 16 against Q = 1: the whole row of results
        i1, s1 = _run_sim(ops, pr, queries=pr.queries[q:q + 1].contiguous())
        assert torch.equal(i1[0], idx[q]) and torch.equal(_bits(s1[0]), _bits(score[q])), q
    for q, j in ((0, 0), (3, 17), (15, 31), (1, 31)):                       # N = 4099 against N = i + 1
        i = int(idx[q, j])
        i2, s2 = _run_sim(ops, pr, n=i + 1)
        at = (i2[q] == i).nonzero()
        assert at.numel() == 1, (q, j, i)
        assert int(_bits(s2[q])[int(at)]) == int(_bits(score[q])[j]), (q, j, i)


def test_sim_topk_nan_scores_sort_last_and_zero_signs_tie(ops):
    D = 64
    index = torch.zeros((6, D), dtype=torch.bfloat16)
    index[0, 0], index[1, 0], index[2, 0], index[4, 0] = -1.0, float("nan"), 2.0, float("-inf")
    index[3, 1] = -0.0
    q = torch.zeros((1, D), dtype=torch.bfloat16)
    q[0, 0] = 1.0
    idx, score = ops.sim_topk(index.cuda(), q.cuda(), 8)
    assert idx[0].tolist() == [2, 3, 5, 0, 4, 1, -1, -1]                   # rows 3 and 5 score -0 / +0: the lower index first
    s = score[0].cpu()
    assert s[:5].tolist() == [2.0, 0.0, 0.0, -1.0, float("-inf")] and bool(torch.isnan(s[5])) and s[6:].tolist() == [float("-inf")] * 2


def test_sim_topk_refuses_what_the_header_refuses(ops):
    index, q = torch.zeros((10, 64), dtype=torch.bfloat16, device="cuda"), torch.zeros((17, 64), dtype=torch.bfloat16, device="cuda")
    with pytest.raises(ValueError, match="P3V_SIM_TOPK_MAX"):
        ops.sim_topk(index, q[:1], 33)
    with pytest.raises(ValueError, match="1..16"):
        ops.sim_topk(index, q, 1)
    with pytest.raises(ValueError):
        ops.sim_topk(index, q[:1], 1, n=11)
    with pytest.raises(RuntimeError):
        ops.sim_topk(index[:, :60].contiguous(), q[:1, :60].contiguous(), 1)
