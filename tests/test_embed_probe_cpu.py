"""tests/embed_probe.py on the CPU: the documented arithmetic restated in torch passes every rule, and every defect the probe is
built for fails on the references alone -- so a GPU pass of tests/test_embed_kernels_gpu.py means what it says."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import embed_probe as ep  # noqa: E402

POOL_VARIANTS = tuple(itertools.product((ep.POOL_LAST, ep.POOL_MEAN), (False, True)))


def test_the_case_lists_cover_what_the_probe_promises():
    assert {c.L for c in ep.POOL_CASES} == set(ep.POOL_L) and {c.B for c in ep.POOL_CASES} == set(ep.POOL_B)
    assert {c.H for c in ep.POOL_CASES} == set(ep.POOL_H)
    for L in ep.POOL_L:
        st = ep.pool_starts(16, L).tolist()
        assert set(st) == {0, min(1, L - 1), L - 1} and all(0 <= s < L for s in st)
        assert L == 1 or all(a != b for a, b in zip(st, st[1:]))
    for fam in (ep.GRID, ep.PLANTED):
        cs = [c for c in ep.SIM_CASES if c.family == fam]
        assert {c.D for c in cs} == set(ep.SIM_D) and {c.Q for c in cs} == set(ep.SIM_Q) and {c.k for c in cs} == set(ep.SIM_K)
    ns = {c.N for c in ep.SIM_CASES if c.family == ep.GRID}
    assert {0, 1, 7, 1000, 4099, ep.ONE_ROW_N} <= ns and any(c.N == c.k - 1 and c.k > 2 for c in ep.SIM_CASES)
    rows_per_wg, n_wg, _ = ep.sim_plan(ep.ONE_ROW_N)
    assert ep.ONE_ROW_N - (n_wg - 1) * rows_per_wg == 1


def test_the_plan_the_probe_plants_on_is_the_librarys():
    from phi_3_vision_mlx_amd import ops
    for c in ep.SIM_CASES:
        assert ops.sim_topk_plan(c.N, c.Q, c.k, c.D) == ep.sim_plan(c.N), c.id
    assert ops.sim_topk_plan(1 << 20, 16, 32, 3072) == (2048, 512, 32)
    assert ops.sim_topk_plan(131072, 1, 1, 3072) == (256, 512, 32)
    with pytest.raises(RuntimeError):
        ops.sim_topk_plan(10, 17, 1, 64)
    with pytest.raises(RuntimeError):
        ops.sim_topk_plan(10, 1, 33, 64)
    with pytest.raises(RuntimeError):
        ops.sim_topk_plan(10, 1, 1, 68)


def test_pool_inputs_are_what_the_docstring_says():
    for c in ep.POOL_CASES:
        p = ep.pool_probe(c)
        x = p.x.float()
        for b in range(c.B):
            s = int(p.start[b])
            assert bool((x[b, :s] == 9984.0).all())                      # bf16(1e4)
        if c.B >= 3:
            assert bool((x[ep.ZERO_ROW, int(p.start[ep.ZERO_ROW]):] == 0).all()) and bool(x[ep.NAN_ROW, c.L - 1].isnan().any())
        lo, hi, nan = p.bounds(ep.POOL_LAST, False)
        assert bool(((lo == hi) | nan).double().mean() >= 0.98)        # the rule reads "bit-exact" almost everywhere


def test_pool_restated_arithmetic_passes_every_rule():
    for c in ep.POOL_CASES:
        p = ep.pool_probe(c)
        for mode, nz in POOL_VARIANTS:
            msg, frac = p.verify(p.restate(mode, nz), mode, nz)
            assert msg == "" and frac <= 1.0, (c.id, mode, nz, msg, frac)


@pytest.mark.parametrize("defect", ep.POOL_DEFECTS)
def test_pool_defect_fails_on_the_references_alone(defect):
    hit = [(c.id, mode, nz) for c in ep.POOL_CASES for mode, nz in POOL_VARIANTS
           if ep.pool_probe(c).verify(ep.pool_probe(c).restate(mode, nz, defect), mode, nz)[0]]
    assert hit, defect
    if defect == "lose_last8":
        assert any("h3080" in h[0] for h in hit)
    if defect == "mean_for_last":
        assert all(h[1] == ep.POOL_LAST for h in hit)
    if defect == "chunk_norm":
        assert all(h[2] for h in hit)


def test_sim_inputs_meet_the_conditions_the_rules_rest_on():
    for c in ep.SIM_CASES:
        ep.sim_probe(c).check_inputs()
    big = ep.sim_probe(ep.SimCase(ep.PLANTED, 4099, 16, 32, 3072))
    rows = set(big.winners.values())
    assert {0, 4098} <= rows and all({e - 1, e} <= rows for e in range(256, 4099, 256))
    assert big.winners[(0, 31)] == big.winners[(1, 31)] and len(rows) == 16 * 32 - 1
    grid = ep.sim_probe(ep.SimCase(ep.GRID, 4099, 16, 32, 3072))
    assert all({e - 1, e} <= set(grid.planted) for e in range(32, 4099, 32)) and {0, 4098} <= set(grid.planted)
    assert sorted(grid.planted.values()).count(0) == 16


def test_sim_restated_arithmetic_passes_every_rule():
    for c in ep.SIM_CASES:
        p = ep.sim_probe(c)
        msg, frac = p.verify(*p.restate())
        assert msg == "" and frac <= 1.0, (c.id, msg, frac)
        if c.N < c.k:
            assert np.all(p.ref_idx[:, c.N:] == -1) and np.all(p.ref_score[:, c.N:] == -np.inf)


@pytest.mark.parametrize("defect", ep.SIM_DEFECTS)
def test_sim_defect_fails_on_the_references_alone(defect):
    hit = [c for c in ep.SIM_CASES if ep.sim_probe(c).verify(*ep.sim_probe(c).restate(defect))[0]]
    assert hit, defect
    if defect in ("ties_high", "ties_wg_order", "lose_wg_first_row"):
        assert any(c.family == ep.GRID for c in hit)
    if defect == "pad_row0":
        assert all(c.N < c.k for c in hit)
