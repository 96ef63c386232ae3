"""Probing inputs, fp64 references and acceptance rules for the LoRA kernels: p3v_lora_down / p3v_lora_up (k_lora_down, k_lora_up<MODE>) and the
per-row forms of the adapter bank p3v_lora_down_rows / p3v_lora_up_rows (k_lora_down_rows<NORM>, k_lora_up_rows<MODE>), csrc/p3v_lora.hip.
Layout and vocabulary of tests/proj_probe.py: LProbe IS a proj_probe.Probe whose accumulator is y + scale (h lora_a) lora_b -- reference(),
verify(), the brackets, the epilogue rules (NONE: the bracket; RESID_BF16: one monotonic fp32 add; SILU_MUL: the 2 x 2 x 2 ends with E_s) and
the guarded output buffer are that class's and are not repeated here.  Everything is torch on the CPU: tests/test_lora_probe_cpu.py shows on
the references alone that the inputs expose each defect, tests/test_lora_kernels_gpu.py runs the kernels.  Nothing here ever looks at what a
kernel produced.

THE REFERENCE is plain fp64 of the rule in include/p3v.h, for row m with entry e = table[row_adapter[m]] and r = min(e.rank, r_max) (the
plain pair: one entry for all rows, r its rank):
    h = x[m], or with norm_w the RMSNorm row AS p3v_rmsnorm WRITES IT (glue_probe pins that kernel, and k_lora_down_rows is already held
        bit-identical to it: the GPU test hands the row over with finish(); the CPU tests use the documented arithmetic in torch fp32);
    T = h @ lora_a[:, :r]   (lora_a is [K, e.rank]: the FIRST r columns of rows of e.rank floats)
    v = bf16(y + scale (T @ lora_b[:r])),   out = epilogue(v).
A row without an adapter -- slot -1, any other value outside 0 .. n_slots - 1, a None entry, an entry with a null pointer -- has v = y and
E = 0: out = epilogue(y) bit for bit, and its part of t is never written (nor read).

TWO INPUT FAMILIES (proj_probe's).
  * GRID, E = 0.  x = i / 8 with |i| <= 15, lora_a = ja 2^-4 and lora_b = jb 2^sb with |ja|, |jb| <= 3, scale in {1.5, 0.75, 2} (by slot), y
    and the residual i / 8: T is an integer of 2^-7, z = T @ lora_b an integer of 2^p (p = sb - 7, chosen per entry so that scale z has
    std <= 1), scale z and y integers of u = 2^(p - 2).  The builder asserts with int64 arithmetic on the actual data that every
    sum_k |x a| stays below 2^24 units of 2^-7 and every |scale| sum_j |T_j b_j| + |y| below 2^24 units u -- so every order of summation,
    every slice split and a fused multiply-add are exact --, that nothing is subnormal, that the std of v is in [0.3, 2], |gate| <= 8 for
    SiLU, and that >= 1 % of the v are bf16 rounding ties and >= 50 % are not bf16 values.  A tie needs the bits below the bf16 step to
    read 100..0, so u may be at most some 2^6 times finer than that step and z an integer of rms about 2000 at most: where dense
    ja, jb would give more (rms 35.6 sqrt(r K)), both are thinned out to a share 2000 / (35.6 sqrt(r K)) of non-zeros (no column of
    lora_a and no row of lora_b left empty) -- dense operands with full mantissas are the SPIKES family's business.  Then t (fp32)
    equals the reference as floats -- in the rows form every slice partial equals its own exact value -- and `out` is bit-exact through
    the epilogue rules.  The fused norm has no exact grid (h is whatever the norm rounds to): norm cases run on SPIKES only.
  * SPIKES.  lora_a and lora_b dense fp32 with all 24 mantissa bits drawn and column exponents in [-3, 3] (a column of lora_b is scaled by a
    power of two until |scale z| <= 1 in every row: with x up to 2^6 and both factors up to 2^3 the update would otherwise dwarf y), y = +-m
    with 8-bit mantissas m in [1, 2) -- E_v grows with sum_j |T_j b_j|, some 6 |z| at r = 64, while a bf16 step shrinks with |v|: under a
    Gaussian y the elements near zero alone put 2 .. 5 % of the brackets of a rank-64 case on two values, with |y| >= 1 it is below 1 %;
    the residual is N(0, 1); a row of x has at most 4 non-zeros (8-bit mantissas, exponents in [-6, 6]; under the fused norm h has the
    same non-zeros, 8-bit values again) at the case's HOT K positions hot_k(K): 0 and K - 1, 255 / 256 and every later slice edge, the
    first and last element of a partial last slice, positions tid = 63 / 64 / 255 of the first slice.  Rows take the
    positions cyclically, rows with a live adapter first; where 4 x (live rows) reaches the list they hit them all (asserted on the CPU,
    and for every K some case of each pair does).
        E_t = 8 2^-24 sum_k |h a|: four rounded products (an fma rounds less), the adds of the wave tree and of the four waves -- adds of
              zero are exact, so at most three adds round, in any order and any slice split: 7 roundings, each at most 2^-24 of the sum of
              magnitudes.  The same bound with the sums over one slice holds each slice partial.
        E_z = (2 r + 2 S) 2^-24 sum_j |T_j b_j| + sum_j E_t[j] |b_j|,  S the slice count: r products and r adds of k_lora_up(_rows), the
              S adds of the slice sum with margin, and what T brings along.
        E_v = |scale| E_z + 2^-23 (|y| + |scale z|): the product scale z and the add each round by 2^-24 of at most |y| + |scale z|.
    Then the bracket, every element.  It is one value on >= 98 % of the elements of every case (asserted on the CPU; a case of fewer than
    4096 outputs takes the first seed at which the conditions on the REFERENCE hold, as proj_probe.probe does).

CASES (M <= 33).  K 192 (one partial slice), 520 (two slices and 8 elements; K % 8 == 0: the norm is allowed), 3072, 8192; lora_b width 8,
576 (SILU_MUL: 288 outputs, no multiple of 256), 1024; M 1, 5, 33; plain pair r in 1, 7, 9, 64 (both sides of an 8-column chunk edge of the
down kernel).  Rows pair: a five-slot table -- ranks 64, 9, 1, a None entry, an entry with a null lora_b (written into the table tensor by
hand) -- row slots 0 .. 4, -1, -7, n_slots on the first eight rows and the live slots cyclically from there on; r_max = 64, and once
r_max = 16 with the rank-64 and rank-9 entries clamped: the rule then uses the first 16 columns of lora_a [K, 64] and the first 16 rows of
lora_b.  All three epilogues, the norm on and off at K = 520 and 3072.

MEMORY.  t is filled with a position-dependent NaN pattern before the down launch: rows without an adapter and columns >= r must keep it
bit for bit.  `out` sits in a guarded [M + 3, N] buffer (contiguous: the entry points take no strides); everything outside [M, N] must come
back bit-identical.
"""
import math
from dataclasses import dataclass
from functools import lru_cache

import torch

import proj_probe as pp
from glue_probe import BF16, F32, F64, GUARD, _gen, bracket, inside, needed_scale, sentinel, to_bf16, unique_share, worst, worst_abs  # noqa: F401
from proj_probe import EPS, MIN_UNIQUE, NNZ, NONE, RESID_BF16, SILU
from qproj_probe import _full_f32

SLICE_K = 256                            # include/p3v.h: P3V_LORA_SLICE_K
FAMILIES = pp.FAMILIES
TABLE_RANKS = (64, 9, 1, None, 7)        # slot 3: a None entry; slot 4: rank 7 with a null lora_b
NULL_B = 4
SCALES = (1.5, 0.75, 2.0, 1.0, 1.5)      # by slot (the plain pair: slot 0 .. 2 by case)
FIRST_SLOTS = (0, 1, 2, 3, 4, -1, -7, len(TABLE_RANKS))
SA = -4                                  # GRID: lora_a = ja 2^SA
TOP_Z = 1.0                              # SPIKES: the largest |scale z| of a column of lora_b (module docstring)


@dataclass(frozen=True)
class LCase(pp.Case):
    """N is the number of outputs (SILU_MUL: half of lora_b's width w_rows)."""
    r: int = 0                   # plain pair: the rank
    rows: bool = False           # the per-row pair
    r_max: int = 64

    @property
    def id(self):
        s = f"lora-{'rows' if self.rows else 'pair'}-{pp.EPI_NAMES[self.epi]}-M{self.M}-N{self.w_rows}-K{self.K}"
        s += f"-rmax{self.r_max}" if self.rows else f"-r{self.r}"
        return s + ("-norm" if self.norm else "")

    @property
    def S(self):
        return -(-self.K // SLICE_K) if self.rows else 1

    @property
    def t_cols(self):
        return self.r_max if self.rows else self.r


def _pair(M, Nb, K, r, epi):
    return LCase("k_lora_down + k_lora_up<%d>" % {NONE: 0, RESID_BF16: 1, SILU: 2}[epi], M, Nb // 2 if epi == SILU else Nb, K, epi, entry="lora", r=r)


def _rows(M, Nb, K, epi, norm=False, r_max=64):
    k = f"k_lora_down_rows<{'true' if norm else 'false'}> + k_lora_up_rows<{ {NONE: 0, RESID_BF16: 1, SILU: 2}[epi]}>"
    return LCase(k, M, Nb // 2 if epi == SILU else Nb, K, epi, entry="lora", norm=norm, rows=True, r_max=r_max)


PAIR_CASES = (_pair(1, 8, 192, 1, NONE), _pair(5, 576, 520, 7, SILU), _pair(33, 1024, 3072, 9, RESID_BF16), _pair(33, 576, 8192, 64, SILU),
              _pair(5, 1024, 192, 64, NONE), _pair(33, 8, 520, 9, RESID_BF16), _pair(1, 576, 3072, 7, NONE), _pair(5, 8, 8192, 1, RESID_BF16))
ROWS_CASES = (_rows(33, 1024, 3072, SILU), _rows(33, 576, 3072, RESID_BF16, norm=True), _rows(5, 576, 520, SILU, norm=True),
              _rows(33, 8, 520, NONE), _rows(1, 1024, 192, RESID_BF16), _rows(33, 576, 8192, NONE), _rows(5, 8, 192, SILU),
              _rows(33, 1024, 520, NONE, norm=True), _rows(5, 8, 3072, RESID_BF16),
              _rows(33, 576, 3072, RESID_BF16, r_max=16))
CASES = PAIR_CASES + ROWS_CASES
assert len({c.id for c in CASES}) == len(CASES)
assert {c.K for c in CASES} == {192, 520, 3072, 8192} and {c.w_rows for c in CASES} == {8, 576, 1024} and {c.M for c in CASES} == {1, 5, 33}
assert {c.r for c in PAIR_CASES} == {1, 7, 9, 64} and all({c.epi for c in g} == {NONE, RESID_BF16, SILU} for g in (PAIR_CASES, ROWS_CASES))
assert {(c.K, c.norm) for c in ROWS_CASES} >= {(520, True), (520, False), (3072, True), (3072, False)} and all(c.K % 8 == 0 for c in CASES if c.norm)


def families(case):
    """The families a case runs on: the fused norm has no exact grid."""
    return ("spikes",) if case.norm else FAMILIES


def hot_k(K):
    """The hot K positions, in order of priority."""
    S = -(-K // SLICE_K)
    pos = [0, K - 1]
    for j in range(1, S):
        pos += [SLICE_K * j - 1, SLICE_K * j]
    if K % SLICE_K:
        pos += [SLICE_K * (S - 1), K - 1]
    pos += [63, 64, 255]
    seen = []
    for p in pos:
        if 0 <= p < K and p not in seen:
            seen.append(p)
    return seen


def row_slots(case):
    """row_adapter of a rows case: slots 0 .. 4, -1, -7, n_slots on the first eight rows, then the live slots 0, 1, 2 in turn."""
    return [FIRST_SLOTS[m] if m < len(FIRST_SLOTS) else (m - len(FIRST_SLOTS)) % 3 for m in range(case.M)]


def t_sentinel(n):
    """Quiet NaNs with the index in the mantissa, as fp32."""
    return (0x7FC00000 + torch.arange(n, dtype=torch.int64) % 251 + 1).to(torch.int32).view(F32)


def rms_restate(x, w):
    """p3v_rmsnorm's documented arithmetic in torch fp32 (glue_probe.RmsProbe.restate)."""
    xf = x.float()
    r = torch.rsqrt((xf * xf).sum(-1, keepdim=True) * (1.0 / x.shape[-1]) + EPS)
    return ((xf * r).to(BF16).float() * w.float()).to(BF16)


class LProbe(pp.Probe):
    def __init__(self, case, family, seed=0):
        self.case, self.family, c = case, family, case
        assert family in families(case)
        self.grid = family == "grid"
        M, K, Nt = c.M, c.K, c.w_rows
        gen = _gen("lora", c.id, family, seed)
        self.bias = self.pos = self.norm_w = None
        # ---- the table and the rows' slots
        if c.rows:
            self.ranks, self.slots = list(TABLE_RANKS), row_slots(c)
            self.scales = list(SCALES)
        else:
            self.ranks, self.slots = [c.r], [0] * M
            self.scales = [SCALES[CASES.index(c) % 3]]
        self.live_slot = [rk is not None and not (c.rows and s == NULL_B) for s, rk in enumerate(self.ranks)]
        self.live = [0 <= s < len(self.ranks) and self.live_slot[s] for s in self.slots]
        # ---- x
        if self.grid:
            a = pp._rand_int(gen, (M, K), 15)
            a[(a == 0).all(-1), 0] = 1.0
            self.x = to_bf16(a / 8)
        else:
            hot = hot_k(K)
            assert len(hot) >= NNZ
            order = [m for m in range(M) if self.live[m]] + [m for m in range(M) if not self.live[m]]
            turn = torch.empty(M, dtype=torch.int64)
            turn[torch.tensor(order)] = torch.arange(M)
            at = torch.tensor(hot)[(NNZ * turn[:, None] + torch.arange(NNZ)[None]) % len(hot)]
            mant = (128 + torch.randint(0, 128, (M, NNZ), generator=gen)).to(F64) / 128
            e = torch.randint(-6, 7, (M, NNZ), generator=gen).to(F64)
            sign = torch.randint(0, 2, (M, NNZ), generator=gen).to(F64) * 2 - 1
            x = torch.zeros((M, K), dtype=F64)
            x[torch.arange(M)[:, None], at] = sign * mant * 2.0 ** e
            self.x = to_bf16(x)
            self.hot, self.hit_live = hot, {int(p) for m in range(M) if self.live[m] for p in at[m]}
        if c.norm:
            nw = 1 + 0.1 * torch.randn((K,), generator=gen)
            nw[::7] *= -1
            self.norm_w = to_bf16(nw)
        # ---- y, the residual
        small = (lambda shape: to_bf16(pp._rand_int(gen, shape, 15) / 8)) if self.grid else (lambda shape: to_bf16(torch.randn(shape, generator=gen)))
        if self.grid:
            self.y = small((M, Nt))
        else:                                                        # +-m with m in [1, 2): no v near zero, where a bf16 step is smaller than E
            sg = torch.randint(0, 2, (M, Nt), generator=gen).to(F64) * 2 - 1
            self.y = to_bf16(sg * (128 + torch.randint(0, 128, (M, Nt), generator=gen)).to(F64) / 128)
        self.resid = small((M, c.N)) if c.epi == RESID_BF16 else None
        # ---- the entries: (lora_a [K, rank], lora_b [rank, Nt]) fp32 per slot, None where the table holds nothing
        self.entries = []
        for s, rk in enumerate(self.ranks):
            if rk is None:
                self.entries.append(None)
            elif self.grid:
                ja, jb = pp._rand_int(gen, (K, rk), 3), pp._rand_int(gen, (rk, Nt), 3)
                q = 2000.0 / (35.6 * math.sqrt(min(rk, c.r_max) * K))                 # dense, z has an rms of 8.9 x 2 x 2 sqrt(r K) units: thinned out
                if q < 1:                                                            # until it is about 2000 (the ties: see the module docstring)
                    ja, jb = ja * (torch.rand((K, rk), generator=gen) < q), jb * (torch.rand((rk, Nt), generator=gen) < q)
                ja[0, (ja == 0).all(0)] = 1.0
                jb[(jb == 0).all(-1), 0] = 1.0
                self.entries.append([ja * 2.0 ** SA, jb, None])                      # (lora_b's exponent: _finish_grid_entry)
            else:
                sg = lambda shape: torch.randint(0, 2, shape, generator=gen).to(F32) * 2 - 1
                a = sg((K, rk)) * _full_f32(gen, (K, rk), 0, 0) * 2.0 ** torch.randint(-3, 4, (1, rk), generator=gen).to(F32)
                b = sg((rk, Nt)) * _full_f32(gen, (rk, Nt), 0, 0) * 2.0 ** torch.randint(-3, 4, (1, Nt), generator=gen).to(F32)
                self.entries.append([a, b, None])
        self.out_rows, self.row_map = M, torch.arange(M)
        self.rows_buf, self.ldo = M + 3, c.N
        self.out_dtype, self.inplace = BF16, False
        self.finish(self.x if not c.norm else rms_restate(self.x, self.norm_w), first=True)
        if self.grid:
            self._assert_grid()
        if c.epi == SILU:
            assert float(self.acc[:, :c.N].abs().max()) <= (8.0 if self.grid else 32.5)
        self._assert_normal()

    # ---- per row: the entry and the clamped rank
    def r_of(self, slot):
        return min(self.ranks[slot], self.case.r_max) if self.case.rows else self.ranks[slot]

    def groups(self, slots=None):
        """(slot, rows) for every live slot that some row names."""
        slots = self.slots if slots is None else slots
        out = []
        for s in range(len(self.ranks)):
            rows = [m for m in range(self.case.M) if slots[m] == s]
            if rows and self.live_slot[s]:
                out.append((s, torch.tensor(rows)))
        return out

    def _tame(self, h64):
        """First call: fix every entry's lora_b -- GRID: the exponent that brings scale z to std <= 1; SPIKES: columns scaled by powers of two
        until |scale z| <= TOP_Z in every row of the case (whatever its slot: the defects move rows between slots)."""
        self.p = {}
        for s, e in enumerate(self.entries):
            if e is None:
                continue
            a, b, _ = e
            r, sc = self.r_of(s), self.scales[s]
            z = (h64 @ a.to(F64)[:, :r]) @ b.to(F64)[:r]
            if self.grid:
                rms = float((z * z).mean().sqrt()) or 1.0
                p = math.floor(math.log2(1.0 / (sc * rms))) + SA - 3          # z is in units 2^(SA - 3) so far
                e[1] = (b * 2.0 ** (p - SA + 3)).to(F32)
                self.p[s] = p
            else:
                top = (sc * z).abs().amax(0)
                e[1] = (b * 2.0 ** -torch.ceil(torch.log2(top / TOP_Z).clamp_min(0))[None].to(F32)).to(F32)

    def finish(self, h, first=False):
        """The reference on the rows h (bf16 [M, K]): x itself, or the RMSNorm rows a test hands over."""
        c = self.case
        M, Nt, S = c.M, c.w_rows, c.S
        self.h = h
        h64 = h.to(F64)
        if first:
            self._tame(h64)
        y64 = self.y.to(F64)
        self.acc, self.Eacc = y64.clone(), torch.zeros_like(y64)
        self.T = torch.zeros((M, c.t_cols), dtype=F64)
        self.Tsl, self.Et, self.Etsl = torch.zeros((M, S, c.t_cols), dtype=F64), torch.zeros((M, c.t_cols), dtype=F64), torch.zeros((M, S, c.t_cols), dtype=F64)
        self.written = torch.zeros((M, c.t_cols), dtype=torch.bool)
        self.abs_in = torch.zeros((M,), dtype=F64)
        self.abs_z = torch.zeros((M, Nt), dtype=F64)
        for s, rows in self.groups():
            a, b, _ = self.entries[s]
            r, sc = self.r_of(s), self.scales[s]
            a64, b64, hg = a.to(F64)[:, :r], b.to(F64)[:r], h64[rows]
            T, absT = hg @ a64, hg.abs() @ a64.abs()
            for i in range(S):
                sl = slice(i * SLICE_K, min((i + 1) * SLICE_K, c.K)) if c.rows else slice(0, c.K)
                self.Tsl[rows, i, :r] = hg[:, sl] @ a64[sl]
                self.Etsl[rows, i, :r] = 8 * 2.0 ** -24 * (hg[:, sl].abs() @ a64[sl].abs())
            Et = 8 * 2.0 ** -24 * absT
            z, absz = T @ b64, T.abs() @ b64.abs()
            Ez = (2 * r + 2 * S) * 2.0 ** -24 * absz + Et @ b64.abs()
            self.T[rows, :r], self.Et[rows, :r] = T, Et
            self.written[rows, :r] = True
            self.acc[rows] = y64[rows] + sc * z
            self.Eacc[rows] = abs(sc) * Ez + 2.0 ** -23 * (y64[rows].abs() + (sc * z).abs())
            self.abs_in[rows], self.abs_z[rows] = absT.amax(-1), absz
        self.absacc = self.Eacc

    def _acc_E(self, s):
        return torch.zeros_like(self.acc) if self.grid or s == 0 else self.Eacc * s

    # ---- the builder's assertions (GRID)
    def _assert_grid(self):
        c = self.case
        xi = (self.x.to(F64) * 8).to(torch.int64)
        yi = self.y.to(F64)
        for s, rows in self.groups():
            a, b, _ = self.entries[s]
            r, sc, p = self.r_of(s), self.scales[s], self.p[s]
            ja, jb = (a.to(F64) * 2.0 ** -SA).to(torch.int64)[:, :r], (b.to(F64) * 2.0 ** (SA - 3 - p)).to(torch.int64)[:r]
            assert torch.equal(ja.to(F64) * 2.0 ** SA, a.to(F64)[:, :r]) and torch.equal(jb.to(F64) * 2.0 ** (p - SA + 3), b.to(F64)[:r])
            Ti = xi[rows] @ ja
            assert int((xi[rows].abs() @ ja.abs()).max()) < 2 ** 24, "sum_k |x a| leaves the exact range of fp32"
            u = 2.0 ** (p - 2)
            top = (int(sc * 4) * (Ti.abs() @ jb.abs())).to(F64) + yi[rows].abs() / u
            assert float(top.max()) < 2 ** 24, "|scale| sum_j |T_j b_j| + |y| leaves the exact range of fp32"
            assert torch.equal(Ti.to(F64) * 2.0 ** (SA - 3), self.T[rows, :r]), "the fp64 T is not exact"
            assert torch.equal(yi[rows] + (int(sc * 4) * (Ti @ jb)).to(F64) * u, self.acc[rows]), "the fp64 reference is not exact"
        live = torch.tensor(self.live)
        f = self.acc[live].to(F32)
        assert torch.equal(f.to(F64), self.acc[live])
        b = f.view(torch.int32)
        self.ties = float(((b & 0xFFFF) == 0x8000).double().mean())
        self.unrep = float((f.to(BF16).to(F64) != f.to(F64)).double().mean())
        std = float(self.acc[live].std()) if f.numel() > 1 else 1.0
        assert self.ties >= 0.01 and self.unrep >= 0.5, f"{c.id}: {self.ties:.3%} rounding ties, {self.unrep:.1%} sums that are no bf16 value"
        assert 0.3 <= std <= 2.0, f"{c.id}: std of v {std:.3f}"

    def _assert_normal(self):
        tiny = 2.0 ** -126
        ts = [self.x, self.y, self.resid, self.acc, self.T] + [t for e in self.entries if e is not None for t in e[:2]]
        for t in ts:
            if t is not None:
                v = t.abs()
                assert not bool(((v > 0) & (v < tiny)).any()), "a subnormal operand or sum"

    # ---- t
    def t_buffer(self):
        c = self.case
        return t_sentinel(c.M * c.S * c.t_cols + 2 * GUARD)

    def t_view(self, flat):
        c = self.case
        return flat[GUARD:flat.numel() - GUARD].view(c.M, c.S, c.t_cols)

    def verify_t(self, flat, s=1.0):
        """flat: the t buffer after the down launch -> ('' or what is wrong, the largest |got - ref| / E; 0 where t must be exact)."""
        got, msgs, top = self.t_view(flat), [], 0.0
        w = self.written
        wsl = w[:, None, :].expand_as(got)
        clean = self.t_buffer()
        keep = torch.ones(clean.numel(), dtype=torch.bool)
        self.t_view(keep)[wsl] = False
        bad = keep & (flat.view(torch.int32) != clean.view(torch.int32))
        if bool(bad.any()):
            msgs.append(f"t: {int(bad.sum())} elements of rows without an adapter, columns >= r or the guards changed, first at flat index {int(bad.nonzero()[0]) - GUARD}")
        g64 = torch.where(wsl, got.to(F64), torch.zeros_like(self.Tsl))
        if self.grid or s == 0:
            ne = (g64 != self.Tsl) & wsl
            if bool(ne.any()):
                msgs.append(f"t: {int(ne.sum())} of {int(wsl.sum())} slice partials differ from the exact value, first at {tuple(ne.nonzero()[0].tolist())}")
        else:
            tiny = 2.0 ** -140
            for name, g, ref, E in (("slice partial", g64, self.Tsl, self.Etsl), ("sum over slices", g64.sum(1), self.T, self.Et)):
                m, ratio = worst_abs(g, ref, E * s + tiny)
                top = max(top, ratio)
                if m:
                    msgs.append(f"t ({name}): {m}")
        return "; ".join(msgs), top

    # ---- the documented arithmetic in torch fp32, with defects
    def restate(self, defect=None, arg=None):
        """(flat out buffer, flat t buffer) as kernels leave them that compute in fp32 what include/p3v.h documents.  `defect`: see
        tests/test_lora_probe_cpu.py."""
        c, d = self.case, defect
        M, K, Nt, S = c.M, c.K, c.w_rows, c.S
        h = self.h.float().clone()
        if d == "drop_k":
            h[:, arg] = 0
        slots = list(self.slots)
        if d == "neighbour_slot":
            slots = slots[1:] + slots[:1]
        if d == "dead_row_updated":
            slots = [s if self.live[m] else 0 for m, s in enumerate(slots)]
        acc = self.y.float().clone()
        tflat = self.t_buffer()
        tv = self.t_view(tflat)
        for s, rows in self.groups(slots):
            a, b, _ = self.entries[s]
            r, sc = self.r_of(s), self.scales[s]
            a_use = a.flatten()[:K * r].view(K, r) if d == "a_stride" else a[:, :r]
            b_use = b[:r]
            skip = {"drop_slice": S // 2 if S > 1 else None, "skip_partial": S - 1 if K % SLICE_K and c.rows and S > 1 else None}.get(d)
            T = torch.zeros((len(rows), r), dtype=F32)
            for i in range(S):
                sl = slice(i * SLICE_K, min((i + 1) * SLICE_K, K)) if c.rows else slice(0, K)
                part = h[rows][:, sl] @ a_use[sl]
                if d == "skip_partial" and not c.rows and K % SLICE_K:
                    part = h[rows][:, :K - K % SLICE_K] @ a_use[:K - K % SLICE_K]
                if i == skip:
                    part = torch.zeros_like(part)
                if d == "t_bf16":
                    part = part.to(BF16).float()
                tv[rows, i, :r] = part
                T = T + part
            z = torch.zeros((len(rows), Nt), dtype=F32)
            for j in range(r - 1 if d == "drop_b_last" else r):
                z = z + T[:, j:j + 1] * b_use[j][None]
            if d == "scale_after":
                acc[rows] = self.y.float()[rows] + sc * z.to(BF16).float()
            else:
                acc[rows] = self.y.float()[rows] + sc * z
        out = self._epilogue(acc, None)
        flat = self.out_buffer()
        self.window_put(flat, out)
        return flat, tflat


@lru_cache(maxsize=2)
def probe(case, family):
    """The probe of a case, as proj_probe.probe: a case of fewer than 4096 outputs takes the first seed at which the conditions on the
    REFERENCE hold.  Nothing here looks at a kernel's output."""
    small = case.M * case.N < 4096
    for seed in range(256 if small else 1):
        try:
            pr = LProbe(case, family, seed)
        except AssertionError:
            if seed == 255 or not small:
                raise
            continue
        if pr.uniqueness()[0] >= MIN_UNIQUE or not small:
            break
    pr.seed = seed
    return pr
