"""The sampling probe (tests/sample_probe.py) judged without a GPU: the case table reaches every path of csrc/p3v_sample.hip that
the old suite never ran; every (row, setting) and every aimed literal is decided under the exact reference and at least 99 % of
each case's random draws are; the NumPy restatement the old GPU test uses (test_sampling_cpu.sample_ref) and the clean emulation
equal the exact reference on every decided draw; every planted defect changes a decided draw on every case where it exists."""
import numpy as np
import pytest

import sample_probe as sp
from test_sampling_cpu import sample_ref

ids = lambda c: c.id


def test_table_reaches_every_path():
    cs = sp.CASES
    by = lambda content: [c for c in cs if c.content == content]
    assert len({c.id for c in cs}) == len(cs)
    for layout in ("contig", "pad3"):                                        # every n in both layouts; off1 wherever n % 8 == 0
        assert {c.n for c in by("gauss") if c.layout == layout} == set(sp.NS)
    assert {c.n for c in by("gauss") if c.layout == "off1"} == {n for n in sp.NS if n % 8 == 0} >= {8, 32768}
    assert {c.groups for c in by("gauss")} == {1, 2, 3, 4} and {8191, 8192, 8193} <= set(sp.NS)   # a row ending in each chunk group
    assert any(c.n % 8 for c in cs if c.layout == "contig") and all(c.n % 8 == 0 for c in cs if c.layout == "off1")
    assert {c.content for c in cs} == {"gauss", "flat", "first", "last", "quarter", "ties32", "tail", "zeros", "overflow", "neginf",
                                       "posinf", "nan-last", "edgeP"}
    assert {c.layout for c in by("ties32")} == {"contig", "off1"} and {c.n for c in by("ties32")} == {32768}
    assert {8192, 32768} <= {c.n for c in by("flat")} and {c.groups for c in by("quarter")} == {2, 3, 4}
    for content in ("overflow", "neginf", "posinf", "nan-last", "zeros", "first", "last", "edgeP"):   # each fallback, with padding behind
        assert {"contig", "pad3"} <= {c.layout for c in by(content)}, content
    st = {s for c in cs for s in c.settings}
    assert {0.05, 0.7, 1.0, 3.0, 0.0} <= {T for T, _, _ in st}
    assert {1.0, 0.9, 0.3, 1e-4, sp.BELOW1} <= {p for _, _, p in st}
    for c in by("gauss"):
        if c.layout == "contig":
            assert {0, 1, 2, 40, c.n - 1, c.n, c.n + 5} <= {k for _, k, _ in c.settings}
    assert {1, 31, 32, 33, 71, 72, 73} <= {k for _, k, _ in by("ties32")[0].settings}
    # the planted rows are what the names say
    t = sp.bf16_values(sp.rows_of("ties32", 32768))
    for r in range(sp.ROWS):
        top = np.flatnonzero(t[r] == t[r].max())
        assert len(top) == 72 and sum((i // 8) % 1024 == 5 for i in top) == 32
    ex = sp.exact_row("tail", 32768, 0, (1.0, 0, 1.0))
    assert set(np.unique(ex.w_lo).tolist()) == {0, 1, sp.TWO32} and (ex.w_lo == 1).sum() > 8000
    ex = sp.exact_row("edgeP", 1025, 0, (1.0, 0, 1.0))
    assert ex.Q_lo == ex.Q_hi == 4 * sp.TWO32 + 2
    for name, exists in sp.DEFECTS.items():                                  # every defect exists on some case
        assert any(exists(c) for c in cs), name
    assert set(sp.DEFECTS) | set(sp.NO_OPS) == set(sp.WEIGHT_DEFECTS) | set(sp.DRAW_DEFECTS)
    for c in cs:
        assert len(sp.AIMED.get(c.id, ())) == len(sp.aim_plan(c)), c.id
        assert len(sp.draws(c)) <= 1024


def test_vector_philox_equals_the_scalar_one():
    c = np.array([0, 1, 7, 12345, (1 << 31) - 1, sp.MASK32], dtype=np.uint64)
    for seed in (0, 1, sp.AIM_SEED, (1 << 64) - 1):
        for swap in (False, True):
            assert sp.philox_words(seed, c, swap).tolist() == [sp.draw_word(seed, int(v), swap) for v in c]


@pytest.mark.parametrize("case", sp.CASES, ids=ids)
def test_case(case):
    dr, n = sp.draws(case), case.n
    rows = sp.rows_of(case.content, n)
    A, B, n_aimed = [], [], sp.n_aimed(case)
    for si, setting in enumerate(case.settings):
        for r in range(sp.ROWS):                                             # every (row, setting) is decided
            assert sp.exact_row(case.content, n, r, setting).decided, (case.id, setting, r)
        a, b = sp.expected(case, si)
        A.append(a), B.append(b)
        assert (a[:n_aimed] == b[:n_aimed]).all(), (case.id, setting, "an aimed draw is undecided")
        for L, (seed, c) in enumerate(dr):
            if a[L] != b[L]:
                continue
            assert sample_ref(rows[L % sp.ROWS], *setting, seed, c) == a[L], (case.id, setting, L, "sample_ref")
            assert sp.emulate(case, si, L) == a[L], (case.id, setting, L, "clean emulation")
    share = min(float((a[n_aimed:] == b[n_aimed:]).mean()) for a, b in zip(A, B))
    print(f"{case.id}: {len(case.settings)} settings x {len(dr)} draws ({n_aimed} aimed): least share of decided random draws {share:.4f}")
    assert share >= 0.99
    # every aimed literal lands where its target says
    words = sp.philox_words(sp.AIM_SEED, [c for _, c in sp.GENERIC])
    assert words[0] < (1 << 12) and words[1] >= sp.TWO32 - (1 << 12) and words[2] % (1 << 19) == 0 and (words[2] >> 17) % 8 and (words[2] >> 19) % 8
    if case.content == "flat":
        assert A[0][0] == 0 and A[0][1] == n - 1                            # index 0 and the last index of a flat row
        if n in (8192, 32768):
            assert sp.meets(case, "on_boundary", 0, 2, [sp.GENERIC[2][1]])[0]
    for i, (target, si, c) in enumerate(sp.AIMED.get(case.id, ())):
        assert sp.meets(case, target, si, len(sp.GENERIC) + i, [c])[0], (case.id, target)
    # every defect that exists here changes a decided draw
    for name, exists in sp.DEFECTS.items():
        if not exists(case):
            continue
        hit = any(A[si][L] == B[si][L] and sp.emulate(case, si, L, name) != A[si][L]
                  for si in range(len(case.settings)) for L in range(len(dr)))
        assert hit, (case.id, name, "changes no decided draw")
        if name in sp.FINE:                                                  # ... the fine ones on their aimed draws
            mine = [(len(sp.GENERIC) + i, si) for i, (t, si, _) in enumerate(sp.AIMED[case.id]) if t == name]
            assert mine and all(sp.emulate(case, si, L, name) != A[si][L] for L, si in mine)
    # k = n treated as a cut changes nothing: the n-th largest value is the minimum
    for name in sp.NO_OPS:
        for si, (T, k, p) in enumerate(case.settings):
            if k == n:
                assert all(sp.emulate(case, si, L, name) == sp.emulate(case, si, L) for L in range(len(dr)))


def test_aim_finds_the_committed_literals_again():
    case = next(c for c in sp.CASES if c.id == "gauss-n1025-contig")
    assert sp.aim_all(case, budget=1 << 20) == sp.AIMED[case.id]
    flat = next(c for c in sp.CASES if c.id == "flat-n9-contig")
    assert sp.aim(flat, "r_low", 0, 0, budget=1 << 20) == sp.GENERIC[0][1]
