"""The probes of tests/qproj_probe.py, checked on the references alone (no GPU).  Three things:
  * the conditions the rules lean on hold for every case of every family: the builder's assertions (exact sums below 2^24, fp16-exact
    4-bit GRID weights, >= 1 % rounding ties, >= 50 % sums that are no bf16 value, one spike per 16-weight piece on the 4-bit stream, the
    fp16 rounding changing >= 25 % of the wide-bias weights), the bracket ONE value on >= 98 % of the elements, >= 3 of 4 rows kept under
    the norm fold; every hot K position is hit, every finite e4m3 code and every nibble value occurs;
  * a torch restatement of each kernel's documented arithmetic -- the 4-bit stream's per-piece scale (D - 128 X) + bias X in fp32, the
    rows kernels' fp16 fma dequantisation and exact products, e4m3's sum first and row scale afterwards, W8A8's acc (sa sw) -- passes
    every rule on every case in three summation orders;
  * every planted defect, applied to that restatement, fails the rule on the first case of every kernel group on which the defect
    exists at all, under the families named in DEFECTS; what a family cannot see is recorded at the end.
A kernel with such a defect therefore cannot pass tests/test_qproj_kernels_gpu.py."""
import pytest
import torch

import qproj_probe as qp
from qproj_probe import NONE, OUT_F32, RESID_BF16, SILU

ids = lambda c: c.id
PLAIN = lambda c: not c.norm and not c.range
BIG = lambda c: c.M * c.N >= 100
Q4 = lambda c: c.fmt == "q4"
E4 = lambda c: c.fmt in ("f8", "w8a8")
BOTH, GRID, SPIKES = ("grid", "spikes"), ("grid",), ("spikes",)

# the issue's defect -> (families it must fail on, the cases it exists on)
DEFECTS = {
    "drop_k0": (BOTH, lambda c: PLAIN(c) and BIG(c) and c.hot_rot == 0),           # (SPIKES: the row that carries positions 0 and K - 1)
    "drop_klast": (BOTH, lambda c: PLAIN(c) and BIG(c) and c.hot_rot == 0),
    "drop_piece": (GRID, lambda c: PLAIN(c) and BIG(c)),                           # a 16-weight piece (W8A8: a K-step) dropped ...
    "piece_twice": (GRID, lambda c: PLAIN(c) and BIG(c)),                          # ... or taken twice
    "neighbour_scale": (BOTH, lambda c: PLAIN(c) and BIG(c) and Q4(c)),            # a 64-weight group under the scale of the group before
    "neighbour_x": (BOTH, lambda c: PLAIN(c) and BIG(c) and Q4(c) and c.stream),   # a piece meeting the X of the piece before
    "no_bias": (BOTH, lambda c: PLAIN(c) and BIG(c) and Q4(c)),
    "keep_128": (BOTH, lambda c: PLAIN(c) and BIG(c) and Q4(c) and c.stream),      # scale D instead of scale (D - 128 X)
    "nibble_swap": (BOTH, lambda c: PLAIN(c) and BIG(c) and Q4(c)),
    "pair_swap": (BOTH, lambda c: PLAIN(c) and BIG(c) and E4(c)),                  # the two bytes of an e4m3 pair
    "flush_subnormal": (SPIKES, lambda c: PLAIN(c) and E4(c) and BIG(c) and (c.epi == OUT_F32 or c.M * c.N >= 60000)),   # (see test_what_a_family_cannot_see)
    "silu_scale_n": (BOTH, lambda c: PLAIN(c) and E4(c) and c.epi == SILU and BIG(c)),      # row n's scale on row n + N
    "scale_tile_local": (BOTH, lambda c: c.fmt == "w8a8" and (c.M > 256 or c.N > 256 or ("narrow" in c.kernel and c.N > 128))),
    "bf16_dequant": (SPIKES, lambda c: PLAIN(c) and BIG(c) and c.rows_q4),         # 8 bits where p3v.h promises fp16
    "x_trunc": (SPIKES, lambda c: PLAIN(c) and BIG(c) and c.rows_q4),
    "trunc_store": (GRID, lambda c: PLAIN(c) and BIG(c) and c.epi != OUT_F32),
    "resid_one_rounding": (GRID, lambda c: PLAIN(c) and BIG(c) and c.epi == RESID_BF16),
    "silu_no_inner": (GRID, lambda c: PLAIN(c) and c.epi == SILU and c.M * c.N >= 128),
    "row_m_twice": (BOTH, lambda c: True),
    "lda_as_k": (BOTH, lambda c: c.fmt == "w8a8" and c.M > 1),
}
# where a defect exists on no case of a group, this is why: it is none of that kernel's
ABSENT = {"neighbour_scale": E4, "no_bias": E4, "nibble_swap": E4, "neighbour_x": lambda c: not (Q4(c) and c.stream),
          "keep_128": lambda c: not (Q4(c) and c.stream), "pair_swap": Q4, "flush_subnormal": Q4, "silu_scale_n": Q4,
          "scale_tile_local": lambda c: c.fmt != "w8a8", "lda_as_k": lambda c: c.fmt != "w8a8", "bf16_dequant": lambda c: not c.rows_q4,
          "x_trunc": lambda c: not c.rows_q4}


def test_table_reaches_every_kernel_and_epilogue():
    assert set(qp.GROUPS) == {"k_gemv3<GemvF8>", "k_gemv3<GemvQ4>", "k_gemv_mfma_f8", "k_gemv_mfma8_f8", "k_gemv8_q4", "k_gemm_rows_q4", "k_gemm256_f8"}
    four = {NONE, RESID_BF16, SILU, OUT_F32}
    for g in qp.GROUPS:
        cases = [c for c in qp.CASES if qp.group(c) == g]
        if g == "k_gemm256_f8":                                               # its three epilogues, wide; the narrow tile has no SiLU form
            assert {c.epi for c in cases if "wide" in c.kernel} == {NONE, RESID_BF16, SILU}
            assert {c.epi for c in cases if "narrow" in c.kernel} == {NONE, RESID_BF16}
            assert {c.knobs[0][1] for c in cases} == {-1, 0, 1} and any(c.N == 384 for c in cases)
            assert {c.M for c in cases} >= {1, 255, 257, 300} and {c.K for c in cases} >= {128, 256, 384, 640}
            assert all(c.ld for c in cases) and any(c.inplace for c in cases)
            continue
        assert {c.epi for c in cases} == four, g
        assert {c.K for c in cases} == {3072, 8192}
        assert any(c.inplace for c in cases), g
        assert any(c.norm for c in cases) == (g != "k_gemm_rows_q4"), g      # (9 .. 16 rows on 4-bit weights: the caller normalises)
        for K in (3072, 8192):                                                # both instances of every kernel meet SiLU and a plain epilogue
            assert {c.epi == SILU for c in cases if c.K == K} == {False, True}, (g, K)
    assert {c.M for c in qp.CASES if c.kernel == "k_gemv_mfma_f8"} >= {2, 4, 5, 8, 9, 16}
    assert {c.M for c in qp.CASES if c.kernel == "k_gemv_mfma8_f8"} == {5, 8}
    assert {c.M for c in qp.CASES if c.kernel == "k_gemv8_q4"} == {2, 5, 8}
    assert {c.M for c in qp.CASES if c.kernel == "k_gemm_rows_q4"} == {2, 8, 9, 16}
    assert {c.kernel for c in qp.CASES if c.range} == {"k_gemv8_q4", "k_gemm_rows_q4"}
    for c in qp.CASES:                                                        # several row sets a workgroup on both 4-bit rows kernels
        assert not c.rows_q4 or ("gemv_q4_rows_wgs", 2) in c.knobs
    for c in qp.CASES:
        if c.stream:
            assert c.M == 1 and c.N in (2, 130, 4102)


def test_gemv_cases_reach_the_kernel_they_name():
    """The knobs of every GEMV case pin the kernel its `kernel` field claims: asked of the library's route on 256 CUs (no device)."""
    from phi_3_vision_mlx_amd import ops
    for case in qp.GEMV_CASES:
        with qp.pinned(ops, case, cu_count=256):
            pass


@pytest.mark.parametrize("family", qp.FAMILIES)
@pytest.mark.parametrize("case", qp.CASES, ids=ids)
def test_reference_passes_in_every_order(case, family):
    pr = qp.probe(case, family)                                                  # (the builder's assertions run here)
    unique, kept = pr.uniqueness()
    line = f"{case.id} [{pr.label}]: bracket is one value on {100 * unique:.2f} %"
    if pr.grid and not case.norm:
        line += f", {100 * pr.ties:.1f} % ties, {100 * pr.unrep:.0f} % sums that are no bf16 value"
    if hasattr(pr, "bites"):
        line += f", the fp16 rounding changes {100 * pr.bites:.0f} % of the wide-bias weights"
    print(line + (f", {100 * kept:.0f} % of the rows kept" if kept < 1 else ""))
    assert unique >= qp.MIN_UNIQUE and kept >= qp.MIN_KEPT
    if not pr.grid and not case.norm:
        hot = qp.hot_k(case)
        nz = pr.A != 0
        assert int(nz.sum(-1).max()) <= qp.NNZ and bool(nz.any(-1).all())
        assert int(nz.any(0).sum()) == min(qp.NNZ * case.M, len(hot)) == pr.hit
        assert set(nz.any(0).nonzero().flatten().tolist()) <= set(hot) and {0, case.K - 1} <= set(hot)
    for order in ("seq", "rev", "tiled"):
        msg = pr.verify(pr.restate(order))
        assert msg == "", f"{order}: {msg}"


def test_cases_share_out_the_hot_positions():
    """Over the plain cases of one kernel group and K every hot position is hit: the whole list where the cases have the rows for it, and
    on the streaming body (one row a case) 0, K - 1 and every 512-element edge."""
    for g in qp.GROUPS:
        for K in sorted({c.K for c in qp.CASES if qp.group(c) == g}):
            hit, want = set(), None
            for case in qp.CASES:
                if qp.group(case) == g and case.K == K and PLAIN(case):
                    pr = qp.probe(case, "spikes")
                    hit |= set((pr.A != 0).any(0).nonzero().flatten().tolist())
                    want = set(qp.hot_k(case))
            if g.startswith("k_gemv3"):
                want = {0, K - 1} | {512 * j + d for j in range(1, K // 512) for d in (-1, 0)}
            assert want <= hit, (g, K, sorted(want - hit))


def test_every_code_occurs():
    """SPIKES: every finite e4m3 byte in W (and every non-zero one in A8), every nibble value, on the first plain case of every group."""
    finite = set(range(256)) - {0x7F, 0xFF}
    for g in qp.GROUPS:
        case = next(c for c in qp.CASES if qp.group(c) == g and PLAIN(c) and BIG(c))
        pr = qp.probe(case, "spikes")
        if case.fmt == "q4":
            assert set(pr.q.unique().tolist()) == set(range(16)), g
            q = pr.q.to(torch.int64).view(pr.q.shape[0], -1, 8)                  # the packed words give the nibbles back in the device order
            for i, sh in enumerate(qp.NIB_POS):
                assert torch.equal((pr.W4.to(torch.int64).view(q.shape[0], -1) >> sh) & 15, q[..., i])
        else:
            assert set(pr.W8.unique().tolist()) == finite, g
    a8 = torch.cat([qp.probe(c, "spikes").A8.flatten() for c in qp.GEMM_CASES if c.M >= 255])
    assert set(a8.unique().tolist()) == finite - {0x80}                          # (0x00: the rows' zeros; -0 is never drawn)


def first_case(g, defect):
    return next((c for c in qp.CASES if qp.group(c) == g and DEFECTS[defect][1](c)), None)


@pytest.mark.parametrize("g", qp.GROUPS, ids=str)
@pytest.mark.parametrize("defect", DEFECTS, ids=str)
def test_defect_fails(g, defect):
    case = first_case(g, defect)
    if case is None:                                                           # the defect is none of this kernel's
        assert defect in ABSENT and all(ABSENT[defect](c) for c in qp.CASES if qp.group(c) == g), (g, defect)
        return
    for family in DEFECTS[defect][0]:
        pr = qp.probe(case, family)
        msg = pr.verify(pr.restate("tiled", defect))
        print(f"{case.id} [{family}] {defect}: {msg}")
        assert msg != "", f"{defect} goes unseen on {case.id} [{family}]"


@pytest.mark.parametrize("g", qp.GROUPS, ids=str)
def test_what_a_family_cannot_see(g):
    """Why there are two families.  GRID's operands are small integers: a dequantisation that keeps 8 bits, an x that loses its last bit
    on the way to fp16 and flushed e4m3 subnormals leave every GRID value as it is (and SPIKES cannot place a dropped piece or K-step that
    holds none of a row's four non-zeros: DEFECTS asks GRID alone for those).  (A flushed e4m3 subnormal is at most 2^-6 of a code: next to terms of up to 448 it moves a bf16
    output only where the other terms are as small, so that defect is held to the fp32 epilogue of the GEMVs and, on W8A8 -- bf16 out
    only -- to the cases of 60000 outputs and more.)"""
    for defect in ("bf16_dequant", "x_trunc", "flush_subnormal"):
        case = first_case(g, defect)
        if case is not None:
            pr = qp.probe(case, "grid")
            assert pr.verify(pr.restate("seq", defect)) == "", (defect, case.id)


def test_norm_fold_defects():
    """The norm fold: the norm weight left out, and the rows normalised with the next row's scale, on the first fold case of more than one
    row of each kernel (the streaming body has one row: the weight alone)."""
    for g in qp.GROUPS:
        case = next((c for c in qp.CASES if qp.group(c) == g and c.norm and (c.M > 1 or c.stream) and BIG(c)), None)
        if case is None:
            assert g in ("k_gemm_rows_q4", "k_gemm256_f8")
            continue
        pr = qp.probe(case, "grid")
        assert pr.verify(pr.restate()) == ""
        A = pr.A.float()
        r = (A * A).sum(-1, keepdim=True).mul(1.0 / case.K).add(qp.EPS).rsqrt()
        variants = [("no weight", (A * r).to(qp.BF16))]
        if case.M > 1:
            variants.append(("the next row's scale", ((A * r.roll(1, 0)).to(qp.BF16).float() * pr.norm_w.float()).to(qp.BF16)))
        for name, xn in variants:
            flat = pr.out_buffer()
            pr.window_put(flat, pr._epilogue(xn.float() @ pr.W.float().T, None))
            assert pr.verify(flat) != "", f"{name} goes unseen on {case.id}"
