"""Cases, an exact reference, an emulation and planted defects for seeded sampling: p3v_sample / p3v_sample_step_end
(csrc/p3v_sample.hip), the rule above p3v_sample_row_t in include/p3v.h.  Everything here is numpy / mpmath on the CPU;
tests/test_sample_probe_cpu.py judges the probe on the references alone, tests/test_sample_kernels_gpu.py runs the kernels.

THE EXACT REFERENCE.  The rule's step 3 takes w = floor(exp(d) * 2^32) "in fp64"; the last bit of an fp64 exp is not specified,
so the reference takes exp from mpmath at 128 bits, once per distinct d: W = floor(exp(d) * 2^32) is then the true integer (but
for |d| below 2^-90, where 128 bits round exp(d) to 1: there W = 2^32 - 1 is set by hand, and the element is near).  An element
is NEAR when the fractional part of exp(d) * 2^32 lies within 2^-16 of an integer and d != 0: assuming the fp64 exp is within
2 ulp, and the product being below 2^33, its absolute error is below 2^-18; the multiply's own rounding adds 2^-21; the sum is
below 2^-17, and 2^-16 doubles it.  (Change the 2-ulp assumption and NEAR_BITS changes with it.)  A near element gives a bracket
w_lo <= w <= w_hi, one apart.  A (row, setting) is DECIDED when the top-p cut kappa -- and so the kept set -- is the same under
w_lo and under w_hi (the top-k cut reads the bf16 values alone); a draw is decided when, in addition, the token is the same for
(cum_hi, t of Q_lo) and (cum_lo, t of Q_hi), the two ends of what any w inside the brackets can give.  z, m, the top-k cut,
P = ceil((double)p * (double)Q) and the Philox word are exactly as the header states them; a NaN row gives -1; the arg-max
fallbacks are those of step 0.  An undecided draw must still be one of the bracket's two tokens.

WHAT A TOKEN TEST CAN SEE.  A weight error shows only through a draw that lands next to a token boundary.  Random draws see a
relative 1e-7 (an fp32 exp, a reciprocal instead of the division) about once per few thousand draws of a wide row, so those draws
are AIMED: `aim` walks counters upwards for a fixed seed until a decided draw meets a target, and the counters it found are
committed below as literals (python tests/sample_probe.py prints them again; nothing is searched at import).  An error far below
1e-7 relative stays invisible to any token test: this probe does not claim bit-exact weights.

THE EMULATION restates the documented structure of the kernel (the header and the comment at the top of csrc/p3v_sample.hip):
16-bit order keys, index 8 (tid + 1024 j) + e in slot 8 j + e of thread tid, two 16-step key bisections, weights as a low word
plus a 2^32 flag, the 12-step chunk bisection and the walk.  Clean, it equals the exact reference on every decided draw; with
one of DEFECTS planted it changes a decided draw on every case where DEFECTS[name](case) says the defect exists.  One name of
the list is different: `topk_eq_n_on` (k = n treated as a cut) cannot change a token -- the n-th largest value is the minimum,
every token is >= it -- so it is listed in NO_OPS and the CPU test shows that it changes nothing: the rule's "k < n" is an
optimisation, not a behaviour.
"""
import math
import zlib
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from test_sampling_cpu import bf16_values, philox4x32_10, to_bits

MASK32 = 0xFFFFFFFF
TWO32 = 1 << 32
ROWS = 9                                  # distinct rows of a case; launch row L holds row L % 9, so the alignment varies
NS = (1, 7, 8, 9, 1023, 1024, 1025, 8191, 8192, 8193, 16391, 24577, 32064, 32767, 32768)
NAN, PINF, NINF = 0x7FC0, 0x7F80, 0xFF80
BELOW1 = float(np.nextafter(np.float32(1), np.float32(0)))      # the fp32 just below 1
NEAR_BITS = 16
N_RANDOM = 64
AIM_SEED = 0x0123456789ABCDEF             # seed_lo != seed_hi


def _crc(*key):
    return zlib.crc32(repr(key).encode())


# ---------------------------------------------------------------- Philox, vectorised
def philox_words(seed, counters, swap=False):
    """Word 0 of Philox4x32-10 for counter (c, 0, 0, 0) and key (seed_lo, seed_hi), c an array: uint64 values below 2^32."""
    k0, k1 = np.uint64(seed & MASK32), np.uint64(seed >> 32)
    if swap:
        k0, k1 = k1, k0
    m32 = np.uint64(MASK32)
    c0 = np.asarray(counters, dtype=np.uint64) & m32
    c1, c2, c3 = np.zeros_like(c0), np.zeros_like(c0), np.zeros_like(c0)
    s32 = np.uint64(32)
    for r in range(10):
        if r:
            k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & m32, (p0 >> s32) ^ c3 ^ k1, p0 & m32
    return c0


def draw_word(seed, c, swap=False):
    key = [seed >> 32, seed & MASK32] if swap else [seed & MASK32, seed >> 32]
    return philox4x32_10([c & MASK32, 0, 0, 0], key)[0]


def tokens_of(cum, Q, r):
    """Vectorised step 6: cum the inclusive prefix sums (uint64), Q the mass (below 2^48), r an array of words."""
    r = np.asarray(r, dtype=np.uint64)
    t = np.uint64(Q >> 32) * r + ((np.uint64(Q & MASK32) * r) >> np.uint64(32))
    return np.searchsorted(cum, t, side="right"), t


# ---------------------------------------------------------------- cases
def _settings(content, n):
    if content == "gauss":
        return ((3.0, 0, 1.0), (1.0, 0, 1.0), (0.7, 40, 0.9), (1.0, n - 1, 0.3), (0.05, 2, 1.0), (0.7, n, 1.0), (1.0, n + 5, 1e-4),
                (3.0, 1, BELOW1), (0.0, 40, 0.9))
    if content == "flat":
        return ((1.0, 0, 1.0), (0.7, 0, 0.9), (1.0, n, 1.0), (3.0, n + 5, 1.0), (1.0, 1, 1.0), (0.0, 0, 1.0))
    if content in ("first", "last"):
        return ((1.0, 0, 1.0), (0.05, 0, 1.0), (3.0, 1, 1.0), (1.0, 0, 1e-4), (0.7, 2, 0.9))
    if content == "quarter":
        return ((1.0, 0, 1.0), (3.0, 0, 1.0), (0.7, 40, 0.9), (1.0, 1, 0.3), (1.0, 2, 1.0))
    if content == "ties32":                # 72 tied maxima: k = 1 .. 71 cuts inside them; P of p = 0.8 falls inside them
        return ((1.0, 0, 1.0), (1.0, 0, 0.8)) + tuple((1.0, k, 1.0) for k in (1, 31, 32, 33, 71, 72, 73)) + ((1.0, 32, 0.8), (3.0, 72, 1.0))
    if content == "tail":
        return ((1.0, 0, 1.0), (1.0, n - 1, 1.0), (1.0, 1, 1.0), (1.0, 0, BELOW1))
    if content == "zeros":
        a, z = zeros_counts(n)
        return ((1.0, 0, 1.0), (0.7, a + 1, 1.0), (1.0, a + 2 * z, 1.0), (3.0, a, 0.9), (1.0, 1, 1.0))
    if content == "overflow":
        return ((0.5, 0, 1.0), (0.5, 2, 0.9), (0.5, 1, 1.0), (0.0, 40, 0.9))
    if content == "edgeP":
        return ((1.0, 0, 0.25), (1.0, 0, 1.0), (1.0, 1, 1.0))
    return ((1.0, 0, 1.0), (0.7, 40, 0.9), (0.0, 0, 1.0))            # neginf, posinf, nan-last


GAUSS_SUBSET = (0, 2, 3, 4, 7, 8)           # the settings of a gauss case in the pad3 / off1 layouts


@dataclass(frozen=True)
class Case:
    n: int
    layout: str                            # contig | pad3 | off1
    content: str

    @property
    def id(self):
        return f"{self.content}-n{self.n}-{self.layout}"

    @property
    def stride(self):
        return self.n + 3 if self.layout == "pad3" else self.n

    @property
    def lead(self):
        return 1 if self.layout == "off1" else 0

    @property
    def settings(self):
        s = _settings(self.content, self.n)
        return tuple(s[i] for i in GAUSS_SUBSET) if self.content == "gauss" and self.layout != "contig" else s

    @property
    def groups(self):
        return (self.n + 8191) // 8192


def _cases():
    cs = [Case(n, "contig", "gauss") for n in NS] + [Case(n, "pad3", "gauss") for n in NS]
    cs += [Case(n, "off1", "gauss") for n in NS if n % 8 == 0]
    table = {"flat": ((1, 9, 8192, 32768), (8193,), (8192,)), "first": ((7, 24577), (1025,), ()),
             "last": ((7, 24577, 32768), (1025, 8191), ()), "quarter": ((8193, 16391, 32768), (24577,), ()),
             "ties32": ((32768,), (), (32768,)), "tail": ((8193, 32768), (), ()), "zeros": ((9, 1025), (1025,), ()),
             "overflow": ((9, 1025), (1025,), ()), "neginf": ((7,), (8193,), ()), "posinf": ((7,), (8193,), ()),
             "nan-last": ((7,), (8193,), ()), "edgeP": ((1025,), (1025,), ())}
    for content, per in table.items():
        for layout, ns in zip(("contig", "pad3", "off1"), per):
            cs += [Case(n, layout, content) for n in ns]
    return tuple(cs)


CASES = _cases()
SAMPLED = ("gauss", "flat", "first", "last", "quarter", "ties32", "tail", "zeros", "overflow", "edgeP")


def zeros_counts(n):
    """(a, z): a positive subnormals (one of them the unique maximum), z of +0 and z of -0; the rest of the row are negative
    subnormals."""
    return (2, 2) if n == 9 else (n // 5, n // 5)


def _gauss(rng, n, top=8.0, clip=7.0):
    x = bf16_values(to_bits(np.minimum(rng.normal(0.0, 2.0, n), clip))).copy()
    x[int(rng.integers(n))] = top
    return x


@lru_cache(maxsize=None)
def edge_levels():
    """(d, count) of the tokens below the top one of an `edgeP` row: their exact weights sum to 3 * 2^32 + 2, so that
    Q = 4 * 2^32 + 2 and p = 0.25 give p * Q = 2^32 + 0.5: ceil takes the second value group, floor the top token alone."""
    rem, out = 3 * TWO32 + 2, []
    for i in range(1, 45):
        d = -0.5 * i
        W, lo, hi = exact_weight(d)
        assert lo == W == hi
        c = min(rem // W, 4)
        if c:
            out.append((d, int(c)))
            rem -= c * W
    assert rem == 0, rem
    return tuple(out)


@lru_cache(maxsize=64)
def rows_of(content, n):
    """The 9 rows of a content at width n: uint16 [9, n] (the layouts of one (content, n) share them)."""
    out = np.zeros((ROWS, n), dtype=np.uint16)
    for r in range(ROWS):
        rng = np.random.default_rng(_crc("row", content if content in ("zeros", "ties32") else "base", n, r))
        if content in ("gauss", "posinf", "nan-last"):
            x = _gauss(rng, n)
            if content == "posinf":
                x[((2 * r + 1) * n) // 18] = np.inf
            bits = to_bits(x)
            if content == "nan-last":
                bits[n - 1] = NAN
        elif content == "flat":
            bits = to_bits(np.zeros(n))
        elif content == "neginf":
            bits = np.full(n, NINF, dtype=np.uint16)
        elif content in ("first", "last"):                # rest: -inf (even rows), more than 22.25 * 3 below (odd rows)
            x = np.full(n, -np.inf) if r % 2 == 0 else rng.uniform(-90.0, -80.0, n)
            x[0 if content == "first" else n - 1] = 0.5
            bits = to_bits(x)
        elif content == "quarter":                        # all mass inside [8192 j, 8192 (j + 1))
            j = r % ((n + 8191) // 8192)
            lo, hi = 8192 * j, min(8192 * (j + 1), n)
            x = np.full(n, -np.inf) if r % 2 == 0 else rng.uniform(-100.0, -95.0, n)
            x[lo:hi] = _gauss(rng, hi - lo)
            bits = to_bits(x)
        elif content == "ties32":                         # 32 maxima in the slots of thread 5, 40 more in other threads
            x = _gauss(rng, n, top=7.0)
            own = np.array([8 * (5 + 1024 * j) + e for j in range(4) for e in range(8)])
            others = np.flatnonzero((np.arange(n) // 8) % 1024 != 5)
            x[rng.choice(others, 40, replace=False)] = 12.0
            x[own] = 12.0
            bits = to_bits(x)
        elif content == "tail":                           # T = 1: d = -22, -22.125, -22.25, -22.5: weights 1, 1, 0, 0
            x = rng.choice(np.array([8.0, 7.875, 7.75, 7.5]), n)
            x[((2 * r + 1) * n) // 18] = 30.0
            bits = to_bits(x)
        elif content == "zeros":
            a, z = zeros_counts(n)
            bits = np.concatenate([[0x007F], rng.integers(1, 0x7F, a - 1), np.full(z, 0x0000), np.full(z, 0x8000),
                                   0x8000 + rng.integers(1, 0x80, n - a - 2 * z)]).astype(np.uint16)
            bits = bits[rng.permutation(n)]
        elif content == "overflow":                       # even rows: max 3e38, m overflows at T = 0.5; odd: max 1.0 and a -3e38
            x = _gauss(rng, n, top=0.5, clip=0.5)
            i, i2 = rng.choice(n, 2, replace=False)
            if r % 2 == 0:
                x[i] = 3e38
            else:
                x[i], x[i2] = 1.0, -3e38
            bits = to_bits(x)
        elif content == "edgeP":
            vals = [30.0] + [30.0 + d for d, c in edge_levels() for _ in range(c)]
            x = np.full(n, -np.inf)
            x[rng.choice(n, len(vals), replace=False)] = vals
            bits = to_bits(x)
        else:
            raise ValueError(content)
        out[r] = bits
    out.setflags(write=False)
    return out


# aimed draws: (target, counter) under AIM_SEED.  GENERIC sits at launch rows 0 .. 2 of EVERY case and serves every setting:
# r below 2^12 (index 0 of a flat row), r above 2^32 - 2^12 (the last index of a flat row, and past it when padding counts),
# r a multiple of 2^19 (t exactly on a prefix boundary of a flat row at n = 8192 and 32768, and the token that boundary belongs to
# not the first of its chunk at either width: there `acc >= t` and `acc > t` walk to the same token).
GENERIC = (("r_low", 510587), ("r_high", 2755305), ("boundary", 8449173))
# per case, from launch row 3 on: (target, index of the setting it was found under, counter)
AIMED = {
    "gauss-n1-contig": (("first", 0, 0), ("last", 0, 0)),
    "gauss-n7-contig": (("first", 0, 5), ("last", 0, 58)),
    "gauss-n8-contig": (("first", 0, 12), ("last", 0, 2)),
    "gauss-n9-contig": (("first", 0, 12), ("last", 0, 2)),
    "gauss-n1023-contig": (("first", 0, 1193), ("last", 0, 475)),
    "gauss-n1024-contig": (("first", 0, 1193), ("last", 0, 475)),
    "gauss-n1025-contig": (("first", 0, 928), ("last", 0, 475)),
    "gauss-n8191-contig": (("first", 0, 1193), ("last", 0, 28476)),
    "gauss-n8192-contig": (("first", 0, 1193), ("last", 0, 28476)),
    "gauss-n8193-contig": (("first", 0, 1193), ("last", 0, 1872)),
    "gauss-n16391-contig": (("first", 0, 12063), ("last", 0, 1872)),
    "gauss-n24577-contig": (("first", 0, 1193), ("last", 0, 1872)),
    "gauss-n32064-contig": (("first", 0, 12063), ("last", 0, 28476)),
    "gauss-n32767-contig": (("first", 0, 12063), ("last", 0, 28476)),
    "gauss-n32768-contig": (("first", 0, 12063), ("last", 0, 28476), ("exp_f32", 1, 48383), ("exp_f32", 1, 16233),
                            ("recip_T", 5, 20496), ("recip_T", 5, 14602)),
    "tail-n8193-contig": (("weight1", 0, 1573788), ("weight1", 0, 1573788)),
    "tail-n32768-contig": (("weight1", 0, 223547), ("weight1", 0, 329162)),
}


def aim_plan(case):
    """The aimed targets of a case beyond GENERIC: (target, setting index)."""
    if case.content == "gauss" and case.layout == "contig":
        plan = [("first", 0), ("last", 0)]
        if case.n == 32768:
            plan += [("exp_f32", 1), ("exp_f32", 1), ("recip_T", 5), ("recip_T", 5)]
        return plan
    if case.content == "tail":
        return [("weight1", 0), ("weight1", 0)]
    return []


@lru_cache(maxsize=None)
def draws(case):
    """The draws of a case, in launch-row order: (seed, counter); launch row L reads row L % 9."""
    out = [(AIM_SEED, c) for _, c in GENERIC] + [(AIM_SEED, c) for _, _, c in AIMED.get(case.id, ())]
    rng = np.random.default_rng(_crc("draws", case.id))
    out += [(int(s), int(c)) for s, c in zip(rng.integers(0, 1 << 64, N_RANDOM, dtype=np.uint64), rng.integers(0, (1 << 31) - 1, N_RANDOM))]
    return tuple(out)


def n_aimed(case):
    return len(GENERIC) + len(AIMED.get(case.id, ()))


@lru_cache(maxsize=2)
def image(case):
    """The logits buffer of a case's launch as uint16: `lead` elements, then one row of `stride` elements per draw.  pad3: the
    three elements behind every row alternate NaN and +inf; off1: the element in front is +inf."""
    D, n = len(draws(case)), case.n
    rows = rows_of(case.content, n)
    buf = np.zeros((D, case.stride), dtype=np.uint16)
    for L in range(D):
        buf[L, :n] = rows[L % ROWS]
        if case.layout == "pad3":
            buf[L, n:] = [NAN, PINF, NAN] if L % 2 == 0 else [PINF, NAN, PINF]
    flat = np.concatenate([np.full(case.lead, PINF, dtype=np.uint16), buf.reshape(-1)])
    flat.setflags(write=False)
    return flat


# ---------------------------------------------------------------- the exact reference
_EXP = {}


def exact_weight(d):
    """(W, w_lo, w_hi) of one d = z - m <= 0 (a Python float)."""
    got = _EXP.get(d)
    if got is None:
        import mpmath
        if d == 0.0:
            got = (TWO32, TWO32, TWO32)
        elif not d >= -23.0:                              # exp(-22.25) * 2^32 = 0.93: below it the floor is 0 and nothing is near
            got = (0, 0, 0)
        else:
            with mpmath.workprec(128):
                v = mpmath.exp(mpmath.mpf(d)) * TWO32
                W = int(mpmath.floor(v))
                f = float(v - W)
            if W >= TWO32:                                # |d| so small that 128 bits round exp(d) to 1: the true floor
                got = (TWO32 - 1, TWO32 - 1, TWO32)
            else:
                eps = 2.0 ** -NEAR_BITS
                got = (W, W - 1 if f < eps else W, W + 1 if f > 1.0 - eps else W)
        _EXP[d] = got
    return got


class Exact:
    """One (row, setting) under the exact rule: `greedy` (the token of an arg-max row) or the kept weights at both ends."""
    greedy = None
    decided = True


_ROW_MEMO = {}


def _row_weights(content, n, row, T):
    key = (content, n, row, T)
    if key not in _ROW_MEMO:
        if len(_ROW_MEMO) > 40:
            _ROW_MEMO.clear()
        x = bf16_values(rows_of(content, n)[row])
        with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
            z = x / np.float32(T)
            d = z.astype(np.float64) - np.float64(z.max())
        ud, inv = np.unique(d, return_inverse=True)
        tab = np.array([exact_weight(float(v)) for v in ud], dtype=np.int64).reshape(-1, 3)
        _ROW_MEMO[key] = (x, tab[inv, 1], tab[inv, 2])
    return _ROW_MEMO[key]


def _top_p(x, w, p):
    Q = int(w.sum())
    P = math.ceil(float(np.float32(p)) * float(Q))
    live = w > 0                                          # a value without weight never decides kappa
    vals, inv = np.unique(x[live], return_inverse=True)
    mass = np.zeros(len(vals), dtype=np.int64)
    np.add.at(mass, inv, w[live])
    above = np.cumsum(mass[::-1])
    return vals[::-1][int(np.argmax(above >= P))]


_EXACT_MEMO = {}


def exact_row(content, n, row, setting):
    key = (content, n, row, setting)
    if key in _EXACT_MEMO:
        return _EXACT_MEMO[key]
    if len(_EXACT_MEMO) > 120:
        _EXACT_MEMO.clear()
    T, k, p = setting
    x = bf16_values(rows_of(content, n)[row])
    ex = Exact()
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        m = np.float32(x.max()) / np.float32(T) if np.float32(T) > 0 and not np.isnan(x).any() else np.float32(np.nan)
    if np.isnan(x).any():
        ex.greedy = -1
    elif not np.isfinite(m):                              # T <= 0, no finite logit, a +inf logit, or max z overflowed
        ex.greedy = int(np.argmax(x))
    else:
        x, lo, hi = _row_weights(content, n, row, T)
        kept = np.ones(n, dtype=bool)
        if 1 <= k < n:
            kept = x >= np.partition(x, n - k)[n - k]
        ends = []
        for w in ((lo,) if lo is hi or np.array_equal(lo, hi) else (lo, hi)):
            w = np.where(kept, w, 0)
            kappa = None
            if 0.0 < float(np.float32(p)) < 1.0:
                kappa = _top_p(x, w, p)
                w = np.where(x >= kappa, w, 0)
            ends.append((kappa, w))
        ex.decided = len(ends) == 1 or ends[0][0] == ends[1][0]
        ex.w_lo, ex.w_hi = ends[0][1], ends[-1][1]
        ex.cum_lo = np.cumsum(ex.w_lo).astype(np.uint64)
        ex.cum_hi = ex.cum_lo if len(ends) == 1 else np.cumsum(ex.w_hi).astype(np.uint64)
        ex.Q_lo, ex.Q_hi = int(ex.cum_lo[-1]), int(ex.cum_hi[-1])
    _EXACT_MEMO[key] = ex
    return ex


def exact_tokens(ex, r):
    """(first, last) token an in-bracket w can give for each word of r; the draw is decided where they agree."""
    r = np.atleast_1d(np.asarray(r, dtype=np.uint64))
    if ex.greedy is not None:
        g = np.full(len(r), ex.greedy, dtype=np.int64)
        return g, g
    a, _ = tokens_of(ex.cum_hi, ex.Q_lo, r)
    if ex.cum_hi is ex.cum_lo:
        return a, a
    b, _ = tokens_of(ex.cum_lo, ex.Q_hi, r)
    return a, b


def exact_draw(content, n, row, setting, seed, counter):
    a, b = exact_tokens(exact_row(content, n, row, setting), [draw_word(seed, counter)])
    return int(a[0]), int(b[0])


def expected(case, si):
    """(first, last) tokens of every draw of a case under setting si: int64 arrays in launch-row order."""
    dr = draws(case)
    a, b = np.zeros(len(dr), dtype=np.int64), np.zeros(len(dr), dtype=np.int64)
    for L, (seed, c) in enumerate(dr):
        a[L], b[L] = exact_draw(case.content, case.n, L % ROWS, case.settings[si], seed, c)
    return a, b


# ---------------------------------------------------------------- the emulation
def order_key(b, split=False):
    """16-bit key that orders the non-NaN bf16 values as floats do (-0 == +0); key 0, below -inf, is a padding slot."""
    b = np.asarray(b, dtype=np.uint32)
    if not split:
        b = np.where(b == 0x8000, 0, b)
    return np.where(b & 0x8000, ~b & 0xFFFF, b | 0x8000).astype(np.uint32)


def key_value(k):
    k = np.asarray(k, dtype=np.uint32)
    return bf16_values(np.where(k & 0x8000, k & 0x7FFF, ~k & 0xFFFF).astype(np.uint16))


_J, _TID, _E = np.meshgrid(np.arange(4), np.arange(1024), np.arange(8), indexing="ij")
_IDX = 8 * (_TID + 1024 * _J) + _E                        # the index held by slot 8 j + e of thread tid: [4, 1024, 8]
WEIGHT_DEFECTS = ("pad_counted", "read_past_n", "aligned_down", "slot_stride", "hi_bit_lost", "popc_one", "topk_strict",
                  "topk_off_by_one", "topk_eq_n_on", "zero_signs_split", "topp_floor", "topp_strict", "topp_mass_stale",
                  "topp_before_topk", "cut_at_22", "greedy_on_overflow_missing", "exp_f32", "recip_T")
DRAW_DEFECTS = ("chunk_bits_11", "walk_ge", "counter_plus_0", "seed_words_swapped")
_STAGE = {}


def _thread_sum(lo, hi, sel, defect):
    """Mass of the selected slots: the low words, plus 2^32 per selected flag -- counted per thread, as a popcount."""
    flags = (sel & hi).sum(axis=(0, 2))
    if defect == "popc_one":
        flags = np.minimum(flags, 1)
    return int(lo[sel].sum()) + (int(flags.sum()) << 32)


def stage(case, si, L, defect=None):
    """Everything of launch row L under setting si that does not depend on the draw: (greedy token, None, None, None) or
    (None, weights uint64 [4096, 8] in chunk order, mass, chunk prefix sums)."""
    if defect not in WEIGHT_DEFECTS:
        defect = None
    key = (case.id, si, L if defect in ("aligned_down", "read_past_n") else L % ROWS, defect)
    if key in _STAGE:
        return _STAGE[key]
    if len(_STAGE) > 150:
        _STAGE.clear()
    T, k, p = case.settings[si]
    n, img = case.n, image(case)
    start = case.lead + L * case.stride
    if defect == "aligned_down":
        start -= start % 8
    idx = 8 * (_TID + 1000 * _J) + _E if defect == "slot_stride" else _IDX
    valid = idx < n
    if defect == "read_past_n":
        valid = idx - _E < n
    pos = start + idx
    raw = np.where(valid & (pos < len(img)), img[np.minimum(pos, len(img) - 1)], 0).astype(np.uint32)
    if defect == "pad_counted":
        valid = np.ones_like(valid)
    nan = bool((((raw & 0x7FFF) > 0x7F80) & valid).any())
    keys = np.where(valid & ((raw & 0x7FFF) <= 0x7F80), order_key(raw, split=defect == "zero_signs_split"), 0)
    kmax = int(keys.max())
    T32 = np.float32(T)
    recip = np.float32(1.0) / T32 if T32 > 0 else T32
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        scale = (lambda v: v * recip) if defect == "recip_T" else (lambda v: v / T32)
        greedy = nan or not T32 > 0
        if not greedy:
            m = scale(key_value(kmax))
            greedy = not np.isfinite(m) and defect != "greedy_on_overflow_missing"
        if greedy:                                        # p3v_argmax: the first maximum, -1 for a NaN row
            out = (-1 if nan else int(_IDX[keys == kmax].min()), None, None, None)
            _STAGE[key] = out
            return out
        # top-k: the largest key kk with #{key >= kk} >= k
        kcut, active = 0, (1 <= k <= n) if defect == "topk_eq_n_on" else (1 <= k < n)
        if active:
            need = k + 1 if defect == "topk_off_by_one" else k
            for bit in range(15, -1, -1):
                cand = kcut | (1 << bit)
                if int((keys >= cand).sum()) >= need:
                    kcut = cand
        live = keys != 0
        kept = live & ((keys > kcut) if defect == "topk_strict" and active else (keys >= kcut))
        d = scale(key_value(keys)).astype(np.float64) - np.float64(m)
        e = np.exp(d.astype(np.float32)).astype(np.float64) if defect == "exp_f32" else np.exp(d)
        w_all = np.where(live & (d >= (-22.0 if defect == "cut_at_22" else -22.25)), np.floor(e * 4294967296.0), 0.0)
        w_all = np.where(np.isfinite(w_all), w_all, 0.0).astype(np.uint64)
    w = np.where(kept, w_all, np.uint64(0))
    lo, hi = w & np.uint64(MASK32), (w >> np.uint64(32)).astype(bool)
    if defect == "hi_bit_lost":
        hi = np.zeros_like(hi)
    everything = np.ones_like(kept)
    mass = _thread_sum(lo, hi, everything, defect)
    p32 = float(np.float32(p))
    if 0.0 < p32 < 1.0:
        Q = int(w_all.sum()) if defect == "topp_before_topk" else mass
        P = math.floor(p32 * float(Q)) if defect == "topp_floor" else math.ceil(p32 * float(Q))
        pcut, cut_mass = 0, mass
        for bit in range(15, -1, -1):
            cand = pcut | (1 << bit)
            tot = _thread_sum(lo, hi, keys >= cand, defect)
            if tot >= P:
                pcut, cut_mass = cand, tot
        drop = (keys <= pcut) if defect == "topp_strict" and pcut else (keys < pcut)
        lo, hi = np.where(drop, np.uint64(0), lo), hi & ~drop
        if defect == "topp_strict":
            cut_mass = _thread_sum(lo, hi, everything, defect)
        if defect != "topp_mass_stale":
            mass = cut_mass
    w = (lo + (hi.astype(np.uint64) << np.uint64(32))).reshape(4096, 8)
    out = (None, w, mass, np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(w.sum(axis=1))]))   # pre[C]: the mass before chunk C
    _STAGE[key] = out
    return out


def emulate(case, si, L, defect=None):
    """The token of launch row L of a case under setting si, as the documented structure computes it."""
    greedy, w, mass, pre = stage(case, si, L, defect)
    if greedy is not None:
        return greedy
    seed, c = draws(case)[L]
    r = draw_word(seed, c - 1 if defect == "counter_plus_0" else c, swap=defect == "seed_words_swapped")
    t = (mass * r) >> 32
    C, before = 0, 0
    for bit in range(10 if defect == "chunk_bits_11" else 11, -1, -1):
        cand = C | (1 << bit)
        if int(pre[cand]) <= t:
            C, before = cand, int(pre[cand])
    acc = before
    for e in range(8):
        acc += int(w[C, e])
        if (acc >= t) if defect == "walk_ge" else (acc > t):
            return 8 * C + e
    return -1


# ---------------------------------------------------------------- planted defects: where each exists
_MULTI = lambda c: (c.content in ("quarter", "ties32", "zeros", "edgeP") or (c.content in ("gauss", "overflow") and c.n >= 7)
                    or (c.content == "flat" and c.n >= 9))                      # more than one token is drawn
_UNALIGNED = lambda c: c.layout != "contig" or c.n % 8 != 0
DEFECTS = {
    # slots beyond n count, as +0.0, in the top-k and the mass (tail, edgeP: e^-30 of the top token, no weight)
    "pad_counted": lambda c: c.n < 32768 and c.content in SAMPLED and c.content not in ("tail", "edgeP"),
    # the last chunk is read whole (a NaN row stays -1 whatever else is read)
    "read_past_n": lambda c: c.layout == "pad3" and c.n % 8 != 0 and c.content != "nan-last",
    # an unaligned row is read from the 16-byte boundary below it (equal rows, and a NaN that stays in view, hide it)
    "aligned_down": lambda c: _UNALIGNED(c) and c.n >= 7 and c.content not in ("flat", "neginf", "nan-last"),
    # group j's indices start at 8 * 1000 * j
    "slot_stride": lambda c: c.n > 8192 and c.content in ("gauss", "last", "quarter", "ties32"),
    # the chunk bisection has 11 steps: C stays below 2048
    "chunk_bits_11": lambda c: c.n > 16384 and c.content in ("gauss", "flat", "last", "quarter", "ties32", "tail"),
    # acc >= t: only a t exactly on a prefix boundary shows it
    "walk_ge": lambda c: c.content == "flat" and c.n in (8192, 32768),
    # the weight is taken mod 2^32: the top token of every sampled row loses its weight
    "hi_bit_lost": lambda c: c.content in SAMPLED,
    # the tied-maxima count of the top-p bisection caps at 1 per thread
    "popc_one": lambda c: c.content == "ties32",
    # ties at the top-k cut are dropped
    "topk_strict": lambda c: c.content in SAMPLED and c.n >= 2,
    # the (k + 1)-th value
    "topk_off_by_one": lambda c: c.content in ("quarter", "ties32", "zeros") or (c.content == "gauss" and c.n >= 7),
    # -0 < +0
    "zero_signs_split": lambda c: c.content == "zeros",
    # P is floored
    "topp_floor": lambda c: c.content == "edgeP",
    # ties at kappa are dropped
    "topp_strict": lambda c: c.content in SAMPLED,
    # Q instead of Q' in step 6
    "topp_mass_stale": lambda c: c.content in ("quarter", "ties32", "edgeP") or (c.content == "gauss" and c.n >= 7),
    # Q is taken over all tokens, before the top-k cut
    "topp_before_topk": lambda c: c.content == "gauss" and c.n >= 1023,
    # weights below d = -22.0 are dropped
    "cut_at_22": lambda c: c.content == "tail",
    # an infinite m is sampled
    "greedy_on_overflow_missing": lambda c: c.content in ("overflow", "posinf"),
    # draw index c - 1
    "counter_plus_0": _MULTI,
    # key (seed_hi, seed_lo)
    "seed_words_swapped": _MULTI,
    # fine: weights from an fp32 exp; z = l * (1 / T).  Visible on their aimed draws alone
    "exp_f32": lambda c: c.id == "gauss-n32768-contig",
    "recip_T": lambda c: c.id == "gauss-n32768-contig",
}
NO_OPS = {"topk_eq_n_on": "k = n as a cut keeps l >= the minimum: every token"}
FINE = ("exp_f32", "recip_T")


# ---------------------------------------------------------------- aiming
def meets(case, target, si, L, counters):
    """Boolean array: which counters give, at launch row L under setting si and AIM_SEED, a decided draw that meets `target`."""
    r = philox_words(AIM_SEED, counters)
    if target == "r_low":
        return r < (1 << 12)
    if target == "r_high":
        return r >= TWO32 - (1 << 12)
    if target == "boundary":
        return (r % np.uint64(1 << 19) == 0) & ((r >> np.uint64(17)) % np.uint64(8) != 0) & ((r >> np.uint64(19)) % np.uint64(8) != 0)
    ex = exact_row(case.content, case.n, L % ROWS, case.settings[si])
    a, b = exact_tokens(ex, r)
    ok = a == b
    if target == "first":
        return ok & (a == 0)
    if target == "last":
        return ok & (a == case.n - 1)
    if target == "weight1":
        return ok & (ex.w_lo[a] == 1) & (ex.w_hi[a] == 1)
    if target == "on_boundary":                           # t equals a prefix sum
        _, t = tokens_of(ex.cum_lo, ex.Q_lo, r)
        return ok & (ex.cum_lo is ex.cum_hi) & np.isin(t, ex.cum_lo)
    assert target in FINE, target
    _, w, mass, _ = stage(case, si, L, target)
    got, _ = tokens_of(np.cumsum(w.reshape(-1)[:case.n]), mass, r)
    return ok & (got != a)


def aim(case, target, si, L, budget=1 << 22, block=1 << 18):
    """The first counter below `budget`, walking upwards from 0, that meets the target; None when there is none."""
    for base in range(0, budget, block):
        c = np.arange(base, min(base + block, budget), dtype=np.uint64)
        ok = meets(case, target, si, L, c)
        if ok.any():
            return int(c[int(np.argmax(ok))])
    return None


def aim_all(case, budget=1 << 22):
    """The AIMED entry of a case, searched afresh."""
    return tuple((target, si, aim(case, target, si, len(GENERIC) + i, budget)) for i, (target, si) in enumerate(aim_plan(case)))


if __name__ == "__main__":
    flat = next(c for c in CASES if c.content == "flat")
    print("GENERIC =", tuple((t, aim(flat, t, 0, i, budget=1 << 24)) for i, (t, _) in enumerate(GENERIC)))
    print("AIMED = {")
    for case in CASES:
        if aim_plan(case):
            print(f"    {case.id!r}: {aim_all(case)!r},")
    print("}")
