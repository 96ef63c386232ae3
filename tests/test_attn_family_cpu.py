"""The probing inputs of tests/attn_family_probe.py, checked on the fp64 reference alone: every way in which a kernel that shares
a family's prefix can go wrong must move the reference by at least four tolerances, or the GPU tests that use these inputs could
not see it.  No GPU, no library."""
import math

import pytest
import torch

import attn_family_probe as fp
from attn_family_probe import CASES, GRP, HD, NH, NKV, POISON, probe, shared_splits, table, worst_ratio

MISS = 4.0                       # a mutant must miss `RTOL 2^-6, ATOL 2e-2` by this factor
FAMILY_CASES = [c for c in CASES if any(len(g) > 1 for g in c.groups)]


def _ratio_rows(pr, mut, rows):
    return {r: worst_ratio(mut[r], pr.ref[r]) for r in rows}


def _assert_missed(pr, mut, rows, what):
    bad = {r: round(v, 2) for r, v in _ratio_rows(pr, mut, rows).items() if v < MISS}
    assert not bad, f"{pr.case.id}: {what} stays within {MISS} tolerances on rows {bad}"


def _neighbours(g):
    return {r: g[(j + 1) % len(g)] for j, r in enumerate(g)}, {r: g[j - 1] for j, r in enumerate(g)}


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_inputs_are_what_the_docstring_says(case):
    pr = probe(case)
    for g in case.groups:
        lo = max(case.pad[r] for r in g)
        for r in g[1:]:                                                             # identical in [pad, share_end), different after
            assert torch.equal(pr.k[r, :, lo:case.share_end], pr.k[g[0], :, lo:case.share_end])
            assert torch.equal(pr.vt[r, :, :, lo:case.share_end], pr.vt[g[0], :, :, lo:case.share_end])
            if case.past > case.share_end:
                assert not torch.equal(pr.k[r, :, case.share_end:case.past], pr.k[g[0], :, case.share_end:case.past])
        for s in shared_splits(case, g):                                            # a planted key on both sides of every shared edge
            assert (s + 1) * case.chunk - 1 in pr.prefix[g[0]] or (s + 1) * case.chunk - 1 < lo
            assert (s + 1) * case.chunk in pr.prefix[g[0]] + pr.private[g[0]] or (s + 1) * case.chunk < lo
        assert case.share_end - 1 in pr.prefix[g[0]] and case.share_end in pr.private[g[0]]
    for b in range(case.B):                                                         # POISON in every dead position
        assert bool((pr.k[b, :, :case.pad[b]] == POISON).all()) and bool((pr.vt[b, :, :, :case.pad[b]] == POISON).all())
        assert bool((pr.k[b, :, case.past:] == POISON).all()) and bool((pr.vt[b, :, :, case.past:] == POISON).all())
    assert bool(torch.isfinite(pr.ref).all()) and 0.3 < float(pr.ref.abs().max()) < 8
    assert worst_ratio(pr.merge(*pr.partials()), pr.ref) < 1e-6                     # the split form of the reference is the reference


def test_tables():
    case = next(c for c in CASES if len(c.groups) == 4)
    t = table(case)
    assert t[:, 0].tolist() == [3, 1, 5, 3, 4, 5, 3, 5] and t[5, 2:5].tolist() == [5, 2, 7] and t[3, 2:5].tolist() == [3, 0, 6]
    assert t[2, 2:].tolist() == [-1] * 16 and t[1, 1:4].tolist() == [0, 1, -1] and t[5, 1] == case.share_end
    assert table(case, shared=False)[:, 0].tolist() == list(range(8))


@pytest.mark.parametrize("case", FAMILY_CASES, ids=lambda c: c.id)
def test_a_member_given_another_members_query_is_seen(case):
    pr = probe(case)
    for g in (g for g in case.groups if len(g) > 1):
        for nb in _neighbours(g):
            q_of = [nb.get(b, b) for b in range(case.B)]
            _assert_missed(pr, pr.attend(s=pr.scores(q_of=q_of)), g, "a neighbour's query")


@pytest.mark.parametrize("case", FAMILY_CASES, ids=lambda c: c.id)
def test_a_shared_split_stored_in_another_slot_doubled_or_dropped_is_seen(case):
    pr = probe(case)
    m, l, O = pr.partials()
    seen = 0
    for g in (g for g in case.groups if len(g) > 1):
        nxt = [_neighbours(g)[0].get(b, b) for b in range(case.B)]
        for s in pr.live_shared(g):
            seen += 1
            m2, l2, O2 = m.clone(), l.clone(), O.clone()                             # member j's record holds its neighbour's partial
            m2[..., s], l2[..., s], O2[..., s, :] = m[nxt][..., s], l[nxt][..., s], O[nxt][..., s, :]
            _assert_missed(pr, pr.merge(m2, l2, O2), g, f"split {s} in a neighbour's slot")
            l2, O2 = l.clone(), O.clone()                                            # counted twice: by the leader and by the row itself
            l2[..., s] *= 2
            O2[..., s, :] *= 2
            _assert_missed(pr, pr.merge(m, l2, O2), g, f"split {s} counted twice")
            m2, l2, O2 = m.clone(), l.clone(), O.clone()                             # dropped
            m2[..., s], l2[..., s], O2[..., s, :] = -math.inf, 0, 0
            _assert_missed(pr, pr.merge(m2, l2, O2), g, f"split {s} dropped")
    assert seen or case.share_end < case.chunk or max(case.pad) >= case.dead_end


@pytest.mark.parametrize("case", [c for c in FAMILY_CASES if c.dead_end != c.share_end], ids=lambda c: c.id)   # the others have none
def test_the_remainder_below_share_end_dropped_is_seen(case):
    pr = probe(case)
    vis = pr.visible()
    vis[:, case.dead_end:case.share_end] = False
    _assert_missed(pr, pr.attend(vis), [r for g in case.groups if len(g) > 1 for r in g], "the remainder dropped")


@pytest.mark.parametrize("case", FAMILY_CASES, ids=lambda c: c.id)
def test_a_private_key_leaking_to_another_member_is_seen(case):
    pr = probe(case)
    prev = {}
    for g in (g for g in case.groups if len(g) > 1):
        prev.update(_neighbours(g)[1])
    src = [prev.get(b, b) for b in range(case.B)]
    rows = sorted(prev)
    for i in range(len(pr.private[rows[0]])):                                        # one private key of the previous member at a time
        t = [pr.private[b][i] for b in range(case.B)]
        assert len(set(t)) == 1
        s_x = pr.scores(k_of=src)[..., t[0]:t[0] + 1]
        v_x = pr.vd[src][:, :, t[0]:t[0] + 1]
        _assert_missed(pr, pr.attend(extra=(s_x, v_x)), rows, f"the neighbour's key at {t[0]} leaking")
