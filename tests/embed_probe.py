"""Probing inputs, fp64 references and acceptance rules for p3v_embed_pool and p3v_sim_topk (csrc/p3v_embed.hip), in the manner
of tests/glue_probe.py.  Everything here is torch / numpy on the CPU; tests/test_embed_probe_cpu.py shows on the references alone
that the inputs expose each defect, tests/test_embed_kernels_gpu.py runs the kernels.

POOL.  y_t is the bf16 row p3v_rmsnorm writes; its rounding bracket [y_lo, y_hi] is glue_probe's (r within relative 2^-16 of
the fp64 value, two roundings).  Pooling is monotone in every y_t, so the fp64 pooled value of the bracket ends encloses the exact
pooled value of whatever y_t the kernel holds: [P_lo, P_hi] = [mean_t y_lo, mean_t y_hi].  The result must lie in
[P_lo - E, P_hi + E], with E from the kernel's arithmetic alone (u = 2^-24, A_j = sum_t max|y_lo, y_hi|, n live rows):
  * LAST, not normalised: E = 0 -- the output is the fp32 of a bf16 value inside the RMSNorm bracket.
  * MEAN: an fp32 sum of n terms in any order is within (n - 1) u A_j of the exact sum, so within u A_j after the division by n;
    the one fp32 division adds u |p| <= u A_j / n.  E_j = 2 u A_j = 2^-23 A_j.
  * normalize: with p_j in [a_j, b_j] (the interval above), the norm S lies in [S_lo, S_hi] = [sqrt(sum min p^2), sqrt(sum max p^2)]
    and e_j in [a_j / (S_hi or S_lo), b_j / (S_lo or S_hi)] by sign.  The kernel's S carries H squarings and H - 1 adds on the
    sum of squares (relative (H + 1) u, halved by the square root), the square root and the division one u each:
    E_j = (H / 2 + 4) u max|a_j, b_j| / S_lo.  A row whose bracket is all zeros must come back all zeros; a row whose reference holds
    a NaN must come back NaN in every element.

SIM_TOPK.  Reference: fp64 dots, a stable sort by (-s, i) (-0 == +0, NaN last).  E(i, q) = D 2^-23 sum_j |index[i, j] queries[q, j]|:
the fp32 summation bound in any order, (D - 1) 2^-24 sum|terms|, with a factor of two in hand.  Two input families decide what is
compared, so that nothing is ever left out of a comparison:
  * GRID: both operands on a small integer grid, every partial sum an integer below 2^24: exact in every order.  Indices AND
    scores must equal the reference exactly.  Two classes of identical rows are planted on every plan edge: class 0 (k // 2
    copies) beats class 1 (the rest, at least a tenth of the rows), so the top k cuts through a class of exact ties.
  * PLANTED: random unit rows; for every query k winners on a ladder of cosines 0.008 apart (> 4 E: asserted), the lowest rung
    0.707, the crowd below; winners at row 0, row N - 1 and either side of the plan's edges, the last rung of queries 0 and 1 one
    shared row.  Gaps above 4 E make the fp64 ranking the only admissible one: indices must be equal, scores within E.
    (Needs N >= Q k rows; the smaller N run on GRID, where equality is exact.)
"""
import math
import zlib
from dataclasses import dataclass
from functools import lru_cache

import numpy as np
import torch

from glue_probe import BF16, F32, F64, EPS, bracket, to_bf16

GUARD = 64
U = 2.0 ** -24
POOL_LAST, POOL_MEAN = "last", "mean"


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


# ---------------------------------------------------------------- pool
POOL_L = (1, 2, 63, 64, 65, 257)
POOL_B = (1, 3, 16)
POOL_H = (3072, 3080, 1024, 1028)


@dataclass(frozen=True)
class PoolCase:
    B: int
    L: int
    H: int

    @property
    def id(self):
        return f"pool-b{self.B}-l{self.L}-h{self.H}"


def _pool_cases():
    """Every L, B and H; every (L, B) pair at one H (rotating), every H at B = 3 with the longest rows."""
    cases = []
    for i, L in enumerate(POOL_L):
        for j, B in enumerate(POOL_B):
            cases.append(PoolCase(B, L, POOL_H[(i + j) % 4]))
    for H in POOL_H:
        for L in (65, 257):
            c = PoolCase(3, L, H)
            if c not in cases:
                cases.append(c)
    return tuple(cases)


POOL_CASES = _pool_cases()
ZERO_ROW, NAN_ROW = 1, 2          # batch rows of every B >= 3 case: all-zero live rows; one NaN in the last row


def pool_starts(B, L):
    """start in {0, 1, L - 1}, differing between neighbouring batch rows."""
    opts = sorted({0, min(1, L - 1), L - 1})
    return torch.tensor([opts[b % len(opts)] for b in range(B)], dtype=torch.int32)


class PoolProbe:
    """Gaussian rows (std 3); 1e4 in every pad row; the first and the last live row HOT (background std 0.05, one 8-wide chunk
    8.0 / 16.0, a different chunk for each, so each carries columns nobody else reaches); for B >= 3, batch row 1 all zeros in its
    live rows and batch row 2 with one NaN in its last row.  Weights 1 + 0.1 N(0, 1), every 7th negated."""

    def __init__(self, case):
        self.case = case
        B, L, H = case.B, case.L, case.H
        gen = _gen("pool", B, L, H)
        self.start = pool_starts(B, L)
        x = torch.randn((B, L, H), generator=gen) * 3.0
        chunks = H // 8
        for b in range(B):
            s = int(self.start[b])
            for t, p in ((s, (3 + 5 * b) % chunks), (L - 1, (chunks - 1 - 7 * b) % chunks)):
                x[b, t] = torch.randn((H,), generator=gen) * 0.05
                x[b, t, 8 * p:8 * p + 4], x[b, t, 8 * p + 4:8 * p + 8] = 8.0, 16.0
            x[b, :s] = 1e4
        if B >= 3:
            x[ZERO_ROW, int(self.start[ZERO_ROW]):] = 0.0
            x[NAN_ROW, L - 1, 5] = math.nan
        w = 1 + 0.1 * torch.randn((H,), generator=gen)
        w[::7] *= -1
        self.x, self.w = to_bf16(x), to_bf16(w)
        x64 = self.x.to(F64)
        self.n = x64 * torch.rsqrt((x64 * x64).mean(-1, keepdim=True) + EPS)
        self.y_lo, self.y_hi = self._y_bracket(1.0)

    def _y_bracket(self, s):
        n_lo, n_hi = bracket(self.n, self.n.abs() * (s * 2.0 ** -16))
        w64 = self.w.to(F64)
        y1, y2 = to_bf16(n_lo.to(F64) * w64).to(F64), to_bf16(n_hi.to(F64) * w64).to(F64)
        return torch.minimum(y1, y2), torch.maximum(y1, y2)

    def live(self):
        t = torch.arange(self.case.L)[None, :]
        return t >= self.start[:, None].long()                     # [B, L]

    def bounds(self, mode, normalize, s=1.0):
        """(lo, hi, nan) fp64 [B, H]: the admissible interval under s x E, and where the reference is NaN."""
        L, H = self.case.L, self.case.H
        u = s * U
        if mode == POOL_LAST:
            lo, hi = self.y_lo[:, L - 1].clone(), self.y_hi[:, L - 1].clone()
        else:
            m = self.live()[:, :, None].to(F64)
            n = m.sum(1)
            ylo, yhi = torch.nan_to_num(self.y_lo) * m, torch.nan_to_num(self.y_hi) * m
            A = torch.maximum(ylo.abs(), yhi.abs()).sum(1)
            E = 2 * u * A
            lo, hi = ylo.sum(1) / n - E, yhi.sum(1) / n + E
            bad = (torch.isnan(self.y_lo) & (m > 0)).any(1)
            lo[bad], hi[bad] = math.nan, math.nan
        nan = torch.isnan(lo) | torch.isnan(hi)
        nan = nan | nan.any(-1, keepdim=True) if normalize else nan
        if normalize:
            a, b = torch.nan_to_num(lo), torch.nan_to_num(hi)
            big = torch.maximum(a.abs(), b.abs())
            small = torch.where((a <= 0) & (b >= 0), torch.zeros_like(a), torch.minimum(a.abs(), b.abs()))
            S_lo, S_hi = (small * small).sum(-1, keepdim=True).sqrt(), (big * big).sum(-1, keepdim=True).sqrt()
            zero = (S_hi == 0)
            S_lo_, S_hi_ = torch.where(S_lo == 0, torch.ones_like(S_lo), S_lo), torch.where(zero, torch.ones_like(S_hi), S_hi)
            assert bool(((S_lo > 0) | zero).all()), "a row whose norm bracket reaches zero without being zero"
            E = (H / 2 + 4) * u * big / S_lo_
            lo = torch.where(a >= 0, a / S_hi_, a / S_lo_) - E
            hi = torch.where(b >= 0, b / S_lo_, b / S_hi_) + E
        return lo, hi, nan

    def verify(self, got, mode, normalize):
        """('' or a description of the worst element, the worst distance outside the E-free interval as a fraction of E)."""
        lo, hi, nan = self.bounds(mode, normalize)
        g = got.to(F64)
        ok = torch.where(nan, torch.isnan(g), (lo <= g) & (g <= hi))
        msg = ""
        if not bool(ok.all()):
            i = int((~ok).flatten().nonzero()[0])
            idx = tuple(int(v) for v in np.unravel_index(i, tuple(g.shape)))
            msg = (f"{int((~ok).sum())} of {ok.numel()} outside; first at {idx}: got {float(g.flatten()[i])!r}, "
                   f"lo {float(lo.flatten()[i])!r}, hi {float(hi.flatten()[i])!r}, nan {bool(nan.flatten()[i])}")
        lo0, hi0, _ = self.bounds(mode, normalize, 0.0)
        E = torch.maximum(lo0 - lo, hi - hi0)
        out = torch.maximum(lo0 - g, g - hi0).clamp_min(0)
        frac = torch.where((E > 0) & ~nan, out / E, torch.zeros_like(out))
        return msg, float(torch.nan_to_num(frac).max())

    def restate(self, mode, normalize, defect=None):
        """The documented arithmetic in torch fp32, with one defect."""
        case, x, w = self.case, self.x.float(), self.w.float()
        B, L, H = case.B, case.L, case.H
        r = torch.rsqrt((x * x).sum(-1, keepdim=True) * (1.0 / H) + EPS)
        wv = torch.ones_like(w) if defect == "skip_weight" else w
        y = (x * r * wv).to(BF16).float() if defect == "skip_round" else ((x * r).to(BF16).float() * wv).to(BF16).float()
        start = self.start.long()
        if defect == "neighbour_start":
            start = torch.roll(start, -1)
        out = torch.empty((B, H), dtype=F32)
        for b in range(B):
            s = int(start[b])
            t0, t1 = s, L
            if defect == "pad_leak":
                t0 = max(s - 1, 0)
            if defect == "drop_first":
                t0 = min(s + 1, L - 1)
            if defect == "drop_last":
                t1 = max(L - 1, s + 1)
            eff = mode if defect != "mean_for_last" else POOL_MEAN
            if eff == POOL_LAST:
                out[b] = y[b, L - 1]
            else:
                out[b] = y[b, t0:t1].sum(0) / float(L if defect == "div_L" else L - s)
        if defect == "lose_last8":
            out[:, H - 8:] = 0
        if normalize:
            ss = (out[:, :512] ** 2).sum(-1, keepdim=True) if defect == "chunk_norm" else (out * out).sum(-1, keepdim=True)
            out = torch.where(ss == 0, out, out / ss.sqrt())
        return out


POOL_DEFECTS = ("pad_leak", "drop_first", "drop_last", "div_L", "neighbour_start", "skip_weight", "skip_round", "chunk_norm",
                "lose_last8", "mean_for_last")


@lru_cache(maxsize=None)
def pool_probe(case):
    return PoolProbe(case)


# ---------------------------------------------------------------- sim_topk
SIM_D = (64, 3072)
SIM_Q = (1, 3, 16)
SIM_K = (1, 8, 32)
GRID, PLANTED = "grid", "planted"
WG_ROWS, ROW_TILE = 256, 32               # the plan at these sizes (asserted against p3v_sim_topk_plan where the library is loaded)
ONE_ROW_N = 4097                          # leaves the last workgroup a single row


def sim_plan(N):
    """(rows_per_wg, n_wg, row_tile) as p3v_sim_topk_plan states it for N <= 131072."""
    assert N <= 512 * WG_ROWS
    return WG_ROWS, -(-N // WG_ROWS), ROW_TILE


@dataclass(frozen=True)
class SimCase:
    family: str
    N: int
    Q: int
    k: int
    D: int

    @property
    def id(self):
        return f"sim-{self.family}-n{self.N}-q{self.Q}-k{self.k}-d{self.D}"


def _sim_cases():
    """Every D, N, Q and k; (Q, k) rotates through its nine pairs along N, and at D = 64, N = 4099 all nine run."""
    qk = [(q, k) for q in SIM_Q for k in SIM_K]
    cases = []
    for D in SIM_D:
        for i, n in enumerate((0, 1, 7, "k-1", 1000, 4099, ONE_ROW_N)):
            Q, k = qk[(2 * i + (D == 64)) % 9] if n != "k-1" else (3, 8 if D == 64 else 32)
            N = k - 1 if n == "k-1" else n
            cases.append(SimCase(GRID, N, Q, k, D))
            if N >= 1000:
                cases.append(SimCase(PLANTED, N, Q, k, D))
    for Q, k in qk:
        for fam in (GRID, PLANTED):
            c = SimCase(fam, 4099, Q, k, 64)
            if c not in cases:
                cases.append(c)
    for c in (SimCase(GRID, 4099, 16, 32, 3072), SimCase(PLANTED, 4099, 16, 32, 3072)):
        if c not in cases:
            cases.append(c)
    return tuple(cases)


SIM_CASES = _sim_cases()


def plan_edges(N):
    """Rows on either side of every row_tile edge (the rows_per_wg edges are among them) below N, workgroup edges first."""
    out = []
    for step in (WG_ROWS, ROW_TILE):
        for e in range(step, N, step):
            for r in (e - 1, e):
                if r not in out:
                    out.append(r)
    return out


def stable_topk(s64, k):
    """First k of a stable sort by (-s, i), -0 == +0, NaN last: (idx [Q, k] int64 with -1 padding, score [Q, k] with -inf padding).
    s64: [N, Q]."""
    N, Q = s64.shape
    idx = np.full((Q, k), -1, dtype=np.int64)
    sc = np.full((Q, k), -np.inf)
    for q in range(Q):
        s = s64[:, q] + 0.0
        key = np.where(np.isnan(s), np.inf, -s)
        order = np.lexsort((np.arange(N), np.isnan(s), key))[:k]
        idx[q, :len(order)] = order
        sc[q, :len(order)] = s[order]
    return idx, sc


class SimProbe:
    def __init__(self, case):
        self.case = case
        N, Q, k, D = case.N, case.Q, case.k, case.D
        gen = _gen("sim", case.family, N, Q, k, D)
        if case.family == GRID:
            index, queries = self._grid(gen)
        else:
            index, queries = self._planted(gen)
        self.index, self.queries = to_bf16(index), to_bf16(queries)
        i64, q64 = self.index.to(F64), self.queries.to(F64)
        self.s64 = (i64 @ q64.T).numpy() if N else np.zeros((0, Q))
        self.E = (D * 2.0 ** -23 * (i64.abs() @ q64.abs().T)).numpy() if N else np.zeros((0, Q))
        self.ref_idx, self.ref_score = stable_topk(self.s64, k)

    # GRID: queries = a common +-1 pattern on the first half, integers of [-2, 2] on the second; crowd rows integers of [-1, 1] on
    # the second half only (|score| <= D); planted rows 4 x the pattern (class 1: the first column 3 x) and a fixed [-1, 1] tail
    # over the last 8 columns: scores 2 D - class +- 16, above every crowd row, different for every query
    def _grid(self, gen):
        N, Q, k, D = self.case.N, self.case.Q, self.case.k, self.case.D
        h = D // 2
        c = torch.randint(0, 2, (h,), generator=gen).float() * 2 - 1
        queries = torch.cat([c.expand(Q, h), torch.randint(-2, 3, (Q, h), generator=gen).float()], 1)
        index = torch.cat([torch.zeros((N, h)), torch.randint(-1, 2, (N, h), generator=gen).float()], 1)
        pos = [p for p in [0, N - 1] + plan_edges(N) if 0 <= p < N]
        extra = torch.randperm(max(N, 1), generator=gen).tolist()
        want = min(N, max(len(set(pos)), N // 8 + 2))
        for p in extra:
            if len(set(pos)) >= want:
                break
            pos.append(p)
        pos = sorted(set(pos))
        n0 = min(k // 2, len(pos) // 3)
        first = set(pos[(j * len(pos)) // n0] for j in range(n0)) if n0 else set()
        tail = torch.randint(-1, 2, (8,), generator=gen).float()
        tail[0] = 1.0
        self.planted = {}
        for p in pos:
            cls = 0 if p in first else 1
            row = torch.zeros(D)
            row[:h] = 4 * c
            if cls:
                row[0] = 3 * c[0]
            row[D - 8:] = tail
            index[p] = row
            self.planted[p] = cls
        return index, queries

    def _planted(self, gen):
        N, Q, k, D = self.case.N, self.case.Q, self.case.k, self.case.D
        assert N >= Q * k
        unit = lambda v: v / v.norm(dim=-1, keepdim=True)
        queries = unit(torch.randn((Q, D), generator=gen, dtype=F64))
        if Q >= 2 and float(queries[0] @ queries[1]) < 0:
            queries[1] = -queries[1]
        index = unit(torch.randn((N, D), generator=gen, dtype=F64))
        pos = [p for p in [0, N - 1] + plan_edges(N) if 0 <= p < N]
        pos += [p for p in torch.randperm(N, generator=gen).tolist() if p not in set(pos)]
        pos = pos[:Q * k]
        self.winners = {}
        shared = None
        for j, p in enumerate(pos):
            q, m = j % Q, j // Q                                   # rung m of query q: the edges go round the queries
            cos = 0.707 + 0.008 * (k - 1 - m)
            if Q >= 2 and m == k - 1 and q in (0, 1):
                if q == 1:
                    self.winners[(1, m)] = shared
                    continue
                shared = p
                c = float(queries[0] @ queries[1])                 # >= 0 (below): cos 0.707 with both queries exactly
                n = torch.randn((D,), generator=gen, dtype=F64)
                for v in (queries[0], unit(queries[1] - c * queries[0])):
                    n = n - (n @ v) * v
                index[p] = math.sqrt(0.5) / (1 + c) * (queries[0] + queries[1]) + math.sqrt(c / (1 + c)) * unit(n)
                self.winners[(0, m)] = p
                continue
            n = torch.randn((D,), generator=gen, dtype=F64)
            n = unit(n - (n @ queries[q]) * queries[q])
            index[p] = cos * queries[q] + math.sqrt(1 - cos * cos) * n
            self.winners[(q, m)] = p
        return index.float(), queries.float()

    def check_inputs(self):
        """The conditions the acceptance rule rests on, on the references alone.  GRID: exact sums; where N >= 20, at least a tenth
        of the rows tie exactly with a top-k member other than themselves, for every query.  PLANTED: every winner's gap to the next
        and to the crowd exceeds 4 E."""
        case, s, k = self.case, self.s64, self.case.k
        if case.family == GRID:
            assert float(np.abs(self.index.float().numpy()).max(initial=0)) <= 4 and np.all(s == np.round(s))
            assert float((self.index.to(F64).abs() @ self.queries.to(F64).abs().T).max()) < 2 ** 24 if case.N else True
            if case.N >= 20:
                for q in range(case.Q):
                    top = self.ref_idx[q][self.ref_idx[q] >= 0]
                    eq = s[:, q][:, None] == s[top, q][None, :]
                    eq[top, np.arange(len(top))] = False
                    tied = int(eq.any(1).sum())
                    assert tied * 10 >= case.N, (case.id, q, tied)
            return
        for q in range(case.Q):
            order = self.ref_idx[q]
            assert sorted(order) == sorted(self.winners[(q, m)] for m in range(k)), (case.id, q)
            sc = np.sort(s[:, q])[::-1][:k + 1]
            Emax = float(self.E[:, q].max())
            assert np.all(sc[:-1] - sc[1:] > 4 * Emax), (case.id, q, float((sc[:-1] - sc[1:]).min()), Emax)

    def verify(self, idx, score):
        """('' or the first violation, worst |score - ref| / E)."""
        case = self.case
        idx, score = np.asarray(idx, dtype=np.int64), np.asarray(score, dtype=np.float64)
        if idx.shape != self.ref_idx.shape or score.shape != self.ref_idx.shape:
            return f"shapes {idx.shape} {score.shape}", math.inf
        if not np.array_equal(idx, self.ref_idx):
            q, j = np.argwhere(idx != self.ref_idx)[0]
            return f"idx[{q}, {j}] = {idx[q, j]}, reference {self.ref_idx[q, j]}", math.inf
        frac, msg = 0.0, ""
        for q in range(case.Q):
            for j in range(case.k):
                i, g, r = idx[q, j], score[q, j], self.ref_score[q, j]
                if i < 0:
                    ok = g == -np.inf
                    e = 0.0
                else:
                    e = 0.0 if case.family == GRID else float(self.E[i, q])
                    ok = abs(g - r) <= e
                    if e > 0:
                        frac = max(frac, abs(g - r) / e)
                if not ok and not msg:
                    msg = f"score[{q}, {j}] (row {i}) = {g!r}, reference {r!r}, E {e!r}"
        return msg, (math.inf if msg else frac)

    def restate(self, defect=None):
        """Scores in torch fp32 (its own summation order), the rule's sort, with one defect: (idx, score)."""
        case = self.case
        N, Q, k, D = case.N, case.Q, case.k, case.D
        a, b = self.index.float(), self.queries.float()
        if defect == "drop_last8":
            a, b = a[:, :D - 8], b[:, :D - 8]
        s = (a @ b.T).double().numpy() if N else np.zeros((0, Q))
        if defect == "bf16_scores":
            s = torch.from_numpy(s).to(BF16).double().numpy()
        if defect == "next_query":
            s = np.roll(s, -1, axis=1)
        if defect == "lose_last_row" and N:
            s[N - 1] = -np.inf
        if defect == "lose_wg_first_row" and N > WG_ROWS:
            s[WG_ROWS] = -np.inf
        if defect in ("ties_high", "ties_wg_order"):
            grp = np.arange(N) if defect == "ties_high" else np.arange(N) // WG_ROWS
            idx = np.full((Q, k), -1, dtype=np.int64)
            sc = np.full((Q, k), -np.inf)
            for q in range(Q):
                order = np.lexsort((np.arange(N), -grp, -(s[:, q] + 0.0)))[:k]
                idx[q, :len(order)], sc[q, :len(order)] = order, s[order, q]
        else:
            idx, sc = stable_topk(s, k)
        if defect in ("lose_last_row", "lose_wg_first_row"):
            gone = sc == -np.inf
            idx[gone & (idx >= 0)] = -1
        if defect == "k_minus_1":
            idx[:, k - 1], sc[:, k - 1] = -1, -np.inf
        if defect == "duplicate" and k >= 2:
            idx[:, k - 1], sc[:, k - 1] = idx[:, 0], sc[:, 0]
        if defect == "pad_row0":
            sc[idx < 0] = s[0, 0] if N else 0.0
            idx[idx < 0] = 0
        return idx, sc


SIM_DEFECTS = ("lose_last_row", "lose_wg_first_row", "ties_high", "ties_wg_order", "next_query", "k_minus_1", "duplicate",
               "bf16_scores", "drop_last8", "pad_row0")


@lru_cache(maxsize=None)
def sim_probe(case):
    return SimProbe(case)
