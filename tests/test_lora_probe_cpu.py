"""The probes of tests/lora_probe.py, checked on the references alone (no GPU).  Three things:
  * every cap holds on the references: the bracket is one value on >= 98 % of the elements of every case, the GRID builder's assertions
    (exact sums, ties, spread), the hot K positions hit by the rows that carry a live adapter;
  * a straightforward torch-fp32 restatement of the documented arithmetic (include/p3v.h) passes every rule, t included;
  * every planted defect, applied to that restatement, fails some element of some case.
A kernel with such a defect therefore cannot pass tests/test_lora_kernels_gpu.py."""
import pytest
import torch

import lora_probe as lp

ids = lambda c: c.id
PAIRS = [(c, f) for c in lp.CASES for f in lp.families(c)]


def _check(pr, out, t):
    """'' or what the rules say about (out, t)."""
    return "; ".join(m for m in (pr.verify(out), pr.verify_t(t)[0]) if m)


@pytest.mark.parametrize("case,family", PAIRS, ids=[f"{c.id}-{f}" for c, f in PAIRS])
def test_lora_probe(case, family):
    pr = lp.probe(case, family)
    uniq = pr.uniqueness()[0]
    out, t = pr.restate()
    msg, ratio = pr.verify_t(t)
    extra = f"ties {100 * pr.ties:.2f} %, no bf16 value {100 * pr.unrep:.1f} %" if pr.grid else f"t of the restatement at {ratio:.3f} of E_t, {len(pr.hit_live)} of {len(pr.hot)} hot positions on live rows"
    print(f"{case.id} [{family}] seed {pr.seed}: bracket is one value on {100 * uniq:.2f} %; {extra}")
    assert uniq >= lp.MIN_UNIQUE
    assert msg == "" and pr.verify(out) == "", _check(pr, out, t)
    assert any(pr.live) and (not case.rows or case.M < 5 or not all(pr.live))
    if not pr.grid:                                                        # the rows with a live adapter hit the head of the hot list, all of it where they can
        n_live = sum(pr.live)
        assert pr.hit_live == set(pr.hot[:lp.NNZ * n_live]) if lp.NNZ * n_live < len(pr.hot) else pr.hit_live == set(pr.hot)
        assert int((pr.x != 0).sum(-1).max()) <= lp.NNZ
    if case.rows:
        assert pr.slots[:8] == list(lp.FIRST_SLOTS)[:case.M] and lp.TABLE_RANKS == (64, 9, 1, None, 7)
        if case.r_max == 16:                                               # the rank-64 and the rank-9 entry are live and clamped / not
            assert {pr.r_of(0), pr.r_of(1), pr.r_of(2)} == {16, 9, 1} and {0, 1} <= set(pr.slots)


def test_hot_positions_are_all_hit_for_every_k():
    for K in (192, 520, 3072, 8192):
        hot = lp.hot_k(K)
        S = -(-K // 256)
        need = {0, K - 1, 63, 64, 255} | {256 * j + d for j in range(1, S) for d in (-1, 0)} | ({256 * (S - 1), K - 1} if K % 256 else set())
        assert {p for p in need if p < K} == set(hot)
        for group in (lp.PAIR_CASES, lp.ROWS_CASES):
            assert any(lp.probe(c, "spikes").hit_live == set(hot) for c in group if c.K == K), K


DEFECTS = ("drop_slice", "skip_partial", "t_bf16", "drop_b_last", "neighbour_slot", "a_stride", "scale_after", "dead_row_updated")


def test_every_defect_fails():
    seen = {(d, f): [] for d in DEFECTS + ("drop_k",) for f in lp.FAMILIES}
    for case, family in PAIRS:
        pr = lp.probe(case, family)
        for d in DEFECTS:
            if _check(pr, *pr.restate(d)):
                seen[d, family].append(case.id)
        if family == "spikes":                                             # an element dropped at each hot K position the live rows carry
            for p in sorted(pr.hit_live):
                assert _check(pr, *pr.restate("drop_k", p)), (case.id, f"k = {p} dropped goes unseen")
            seen["drop_k", family].append(case.id)
        else:
            seen["drop_k", family] += [case.id] if _check(pr, *pr.restate("drop_k", 0)) and _check(pr, *pr.restate("drop_k", case.K - 1)) else []
    for key, where in seen.items():
        print(key, len(where))
    of = lambda f, cond=lambda c: True: {c.id for c, g in PAIRS if g == f and cond(c)}
    full = {c.id for c, g in PAIRS if g == "spikes" and lp.probe(c, g).hit_live == set(lp.hot_k(c.K))}
    many = lambda c: c.rows and c.M > 1
    # SPIKES: every case the defect applies to sees it
    assert set(seen["drop_k", "spikes"]) == of("spikes")                                       # an element dropped at each hot K position
    assert set(seen["drop_slice", "spikes"]) >= of("spikes", lambda c: c.rows and c.K > 256) & full          # a dropped slice
    assert set(seen["skip_partial", "spikes"]) >= of("spikes", lambda c: c.K % 256 and (c.K > 256 or not c.rows))   # the last partial slice skipped
    assert set(seen["t_bf16", "spikes"]) == of("spikes")                                       # t rounded to bf16
    assert set(seen["drop_b_last", "spikes"]) == of("spikes")                                  # lora_b row r - 1 dropped
    assert set(seen["scale_after", "spikes"]) >= of("spikes", lambda c: c.M * c.N >= 256)      # scale applied after the rounding (moves 2^-9 of
    assert len(seen["scale_after", "spikes"]) >= len(of("spikes")) - 3                         # an update: a matter of elements in an 8-output case)
    # either family: the defects of the tables
    for f in lp.FAMILIES:
        assert set(seen["neighbour_slot", f]) >= of(f, many)                                   # the neighbour row's slot
        assert set(seen["dead_row_updated", f]) >= of(f, many)                                 # a rank-0 / null / out-of-range row given an update
        assert set(seen["a_stride", f]) == of(f, lambda c: c.rows and c.r_max < 64) != set()   # the wrong lora_a stride under r_max < rank
    # GRID (thinned operands: a single dropped element may meet a zero): most cases, and the exact ones always see a lost slice or row
    n_grid = len(of("grid"))
    for d in ("drop_k", "t_bf16", "scale_after"):
        assert len(seen[d, "grid"]) >= (2 * n_grid) // 3, (d, seen[d, "grid"])
    assert set(seen["drop_b_last", "grid"]) == of("grid")
    assert set(seen["drop_slice", "grid"]) >= of("grid", lambda c: c.rows and c.K > 256)
    assert set(seen["skip_partial", "grid"]) >= of("grid", lambda c: c.K % 256 and (c.K > 256 or not c.rows))
