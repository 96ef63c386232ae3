"""The probes of tests/proj_probe.py, checked on the references alone (no GPU).  Three things:
  * the conditions the rules lean on hold for every case of both families: exact sums below 2^24 units, >= 1 % rounding ties and
    >= 50 % sums that are no bf16 value (asserted by the builder), the bracket ONE value on >= 98 % of the elements, >= 3 of 4 rows
    kept under the norm fold, every hot K position hit;
  * a plain torch-fp32 restatement of the documented arithmetic passes every rule on every case in three summation orders
    (8-wide chunks in order, from the end, 64-wide tiles in halves inside 4 K slices): order is irrelevant, and no rule is so
    tight that a correct kernel fails it;
  * every planted defect, applied to that restatement, fails the rule on the first case of every (kernel, family) pair on which
    the defect exists at all (a SiLU defect needs a SiLU case, `lda taken as K` a case with lda > K, a rounding defect more than a
    handful of outputs).
A kernel with such a defect therefore cannot pass tests/test_proj_kernels_gpu.py."""
import pytest

import proj_probe as pp

ids = lambda c: c.id
BF16_OUT = lambda c: c.epi not in pp.F32_OUT
MANY = lambda c: c.M * c.N >= 256
PLAIN = lambda c: not (c.norm and c.entry == "gemv")

# defect -> (families it must fail on, the cases it exists on)
DEFECTS = {
    "drop_k0": (("grid", "spikes"), lambda c: PLAIN(c) and MANY(c)),
    "drop_klast": (("grid", "spikes"), lambda c: PLAIN(c) and MANY(c)),
    "drop_tile": (("grid",), lambda c: PLAIN(c) and MANY(c)),
    "tile_twice": (("grid",), lambda c: PLAIN(c) and MANY(c)),
    "shift_slice": (("grid",), lambda c: PLAIN(c) and MANY(c)),
    "cut_mantissa": (("spikes",), PLAIN),                      # operand mantissas cut to 4 bits: GRID cannot see it (recorded below)
    "trunc_store": (("grid",), lambda c: PLAIN(c) and BF16_OUT(c) and MANY(c)),
    "half_away": (("grid",), lambda c: PLAIN(c) and BF16_OUT(c) and MANY(c)),
    "resid_one_rounding": (("grid",), lambda c: PLAIN(c) and c.epi == pp.RESID_BF16 and MANY(c)),
    "bias_after_rounding": (("grid",), lambda c: c.epi == pp.BIAS and MANY(c)),
    "silu_no_inner": (("grid",), lambda c: PLAIN(c) and c.epi == pp.SILU and c.M * c.N >= 128),
    "up_from_gate": (("grid",), lambda c: PLAIN(c) and c.epi == pp.SILU),
    "bf16_partials": (("grid",), lambda c: PLAIN(c) and c.K >= 256 and MANY(c)),
    "fp16_partials": (("grid",), lambda c: PLAIN(c) and c.K >= 256 and MANY(c)),
    "row_m_twice": (("grid", "spikes"), lambda c: True),
    "lda_as_k": (("grid", "spikes"), lambda c: c.ld and c.M > 1),
    "patch_not_remapped": (("grid", "spikes"), lambda c: c.epi == pp.PATCH),
}


def group(case):
    """The kernel of a case without its template arguments and without a second launch (split-K on k_gemm is a path of its own)."""
    return "k_gemm+k_splitk_reduce" if case.kernel.startswith("k_gemm+") else case.kernel.split("<")[0].split("+")[0]


GROUPS = tuple(dict.fromkeys(group(c) for c in pp.CASES))


def test_table_reaches_every_kernel():
    assert set(GROUPS) == {"k_gemm", "k_gemm256", "k_gemm+k_splitk_reduce", "k_gemm_skinny", "k_gemm_rows", "k_gemv", "k_gemv3", "k_gemv_mfma8",
                           "k_gemv_mfma"}
    for g in GROUPS:                                                        # every p3v_gemm path has a strided case
        assert g.startswith("k_gemv") or any(c.ld for c in pp.CASES if group(c) == g), g
    assert any("k_splitk_reduce_norm" in c.kernel for c in pp.CASES)
    assert {c.epi for c in pp.CASES if group(c) == "k_gemm"} == set(range(9))
    for tag in ("pin", "all"):                                              # the 256 x 256 kernel: every epilogue it takes, both ways
        assert {c.epi for c in pp.CASES if group(c) == "k_gemm256" and c.tag == tag} == set(range(9)) - {pp.PATCH}


def test_gemv_cases_reach_the_kernel_they_name():
    """The knobs of every p3v_gemv case pin the kernel its `kernel` field claims: asked of the library's route on 256 CUs (no device)."""
    from phi_3_vision_mlx_amd import ops
    for case in pp.GEMV_CASES:
        with pp.pinned(ops, case, cu_count=256):
            pass


@pytest.mark.parametrize("family", pp.FAMILIES)
@pytest.mark.parametrize("case", pp.CASES, ids=ids)
def test_reference_passes_in_every_order(case, family):
    pr = pp.probe(case, family)                                            # (the builder's assertions run here)
    unique, kept = pr.uniqueness()
    line = f"{case.id} [{pr.label}]: bracket is one value on {100 * unique:.2f} %"
    if pr.grid and PLAIN(case):
        line += f", {100 * pr.ties:.1f} % ties, {100 * pr.unrep:.0f} % sums that are no bf16 value"
    print(line + (f", {100 * kept:.0f} % of the rows kept" if kept < 1 else ""))
    assert unique >= pp.MIN_UNIQUE and kept >= pp.MIN_KEPT
    if not pr.grid and PLAIN(case):
        hot = pp.hot_k(case)
        nz = (pr.A != 0)
        assert int(nz.sum(-1).max()) <= pp.NNZ and bool(nz.any(-1).all())          # at most 4 non-zeros, every row carries some
        assert int(nz.any(0).sum()) == min(pp.NNZ * case.M, len(hot)) == pr.hit    # the head of the list is hit, every position at most once per row
        assert set(nz.any(0).nonzero().flatten().tolist()) <= set(hot)
        assert {0, case.K - 1} <= set(hot)
    for order in ("seq", "rev", "tiled"):
        msg = pr.verify(pr.restate(order))
        assert msg == "", f"{order}: {msg}"
    if case.norm and case.entry == "gemm":                                 # the second output of p3v_gemm_resid_norm: glue_probe's restatement
        out = pr.window_get(pr.restate())
        x = out.float()
        r = (x * x).sum(-1, keepdim=True).mul(1.0 / case.N).add(pp.EPS).rsqrt()
        normed = ((x * r).to(pp.BF16).float() * pr.norm_w.float()).to(pp.BF16)
        assert pr.verify_normed(out, normed) == ""
        assert pr.verify_normed(out, (x * r * pr.norm_w.float()).to(pp.BF16)) != ""       # the first rounding skipped


def test_stream_cases_share_out_the_chunk_edges():
    """One streaming-GEMV case has at most 4 rows of 4 spikes: over the plain cases of one K, 0, K - 1 and every edge of the kernel's
    512-element lane chunks (which include its stage edges) are hit."""
    for K in (3072, 8192):
        hit = set()
        for case in pp.CASES:
            if group(case) == "k_gemv3" and case.K == K and PLAIN(case):
                hit |= set((pp.probe(case, "spikes").A != 0).any(0).nonzero().flatten().tolist())
        assert {0, K - 1} | {512 * j + d for j in range(1, K // 512) for d in (-1, 0)} <= hit, K


def first_case(g, defect):
    return next((c for c in pp.CASES if group(c) == g and DEFECTS[defect][1](c)), None)


@pytest.mark.parametrize("g", GROUPS, ids=str)
@pytest.mark.parametrize("defect", DEFECTS, ids=str)
def test_defect_fails(g, defect):
    case = first_case(g, defect)
    if case is None:                                                       # the defect does not exist on this kernel (no bias, no strides, ...)
        assert defect in ("bias_after_rounding", "lda_as_k", "patch_not_remapped") or (g == "k_gemm256" and defect.endswith("_partials")), (g, defect)
        return
    for family in DEFECTS[defect][0]:
        pr = pp.probe(case, family)
        msg = pr.verify(pr.restate("tiled", defect))
        print(f"{case.id} [{family}] {defect}: {msg}")
        assert msg != "", f"{defect} goes unseen on {case.id} [{family}]"


@pytest.mark.parametrize("g", GROUPS, ids=str)
def test_grid_cannot_see_lost_mantissa_bits(g):
    """Why the second family exists: operands cut to 4 mantissa bits leave every GRID value as it is."""
    case = first_case(g, "cut_mantissa")
    pr = pp.probe(case, "grid")
    assert pr.verify(pr.restate("seq", "cut_mantissa")) == ""


def test_norm_fold_defects():
    """The GEMV norm fold: the norm weight left out, and the rows normalised with the next row's scale, on the first fold case of each
    kernel.  (The fold's weights are powers of two, so its two roundings are one: that chain is p3v_rmsnorm's and pinned there.)"""
    for g in ("k_gemv", "k_gemv3", "k_gemv_mfma8", "k_gemv_mfma"):
        case = next(c for c in pp.CASES if group(c) == g and c.norm and c.M > 1)
        pr = pp.probe(case, "grid")
        assert pr.verify(pr.restate()) == ""
        A = pr.A.float()
        r = (A * A).sum(-1, keepdim=True).mul(1.0 / case.K).add(pp.EPS).rsqrt()
        for name, xn in (("no weight", (A * r).to(pp.BF16)), ("the next row's scale", ((A * r.roll(1, 0)).to(pp.BF16).float() * pr.norm_w.float()).to(pp.BF16))):
            flat = pr.out_buffer()
            pr.window_put(flat, pr._epilogue(xn.float() @ pr.W.float().T, None))
            assert pr.verify(flat) != "", f"{name} goes unseen on {case.id}"
