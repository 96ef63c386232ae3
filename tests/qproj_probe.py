"""Probing inputs, fp64 references and acceptance rules for the QUANTISED projection kernels: behind p3v_gemv_fp8 the e4m3 policy of the
K = 3072 / 8192 streaming body (GemvF8), k_gemv_mfma_f8 and k_gemv_mfma8_f8; behind p3v_gemv_q4 the 4-bit policy of the streaming body
(GemvQ4), k_gemv8_q4 and k_gemm_rows_q4; behind p3v_gemm_fp8 the W8A8 kernel k_gemm256_f8 with its wide and its narrow tile.  The
vocabulary is tests/proj_probe.py's (and through it tests/glue_probe.py's): QProbe IS a proj_probe.Probe whose operands are quantised --
reference(), verify(), the brackets, the epilogue rules (RESID_BF16, SILU_MUL, F32), the norm fold and the guarded buffers are that
class's and are not repeated here.  Everything is torch on the CPU: tests/test_qproj_probe_cpu.py shows on the references alone that the
inputs expose each defect, tests/test_qproj_kernels_gpu.py runs the kernels.  Nothing here ever looks at what a kernel produced.

WHAT A WEIGHT IS.  The reference is x . w in fp64 with w the value the kernel's documented arithmetic gives a weight (include/p3v.h):
  * e4m3 GEMVs and the W8A8 GEMM: w = code (x) scale[n] -- the kernels sum x . code first and scale the sum (W8A8: by fl(sa[m] sw[n])).
  * 4-bit, M = 1 (streaming body): per 16-weight piece scale (D - 128 X) + bias X with D = sum x (128 + q), X = sum x: w = q scale + bias
    exactly.
  * 4-bit, 2 .. 16 rows (k_gemv8_q4, k_gemm_rows_q4): w = fp16(q scale + bias), ONE rounding (a packed fp16 fma after an exact
    (1024 + q) - 1024), x converted to fp16, products on the fp16 matrix cores.  q scale + bias is exact in fp32 at every input here
    (asserted), so torch's fp32 -> fp16 conversion is that single rounding.

THE INPUT FAMILIES (proj_probe's, rebuilt on codes).
  * GRID, E = 0: every partial sum in every order is exact in fp32, so `got ==` the fp64 value pushed through the roundings of p3v.h.
      e4m3 GEMVs: x = i / 8 with |i| <= 15, codes the integers |j| <= 15 (exact e4m3 values), row scales c 2^s with c in {4, 5, 6, 7} / 4
        and s = -10: sums are integers of 1 / 8 below 225 K, and 225 K 7 < 2^24 keeps acc x scale exact too.  Products have std
        1.118 x 8.94 x 1.40 (rms c) = 14.0: output std 0.76 (K = 3072) and 1.24 (K = 8192).
      4-bit: q in 0 .. 15, per group scale = +-{1, 2, 3} 2^t and bias = jb 2^t with |jb| <= 31, t = -11: a weight is an integer of at most
        76 units 2^t -- 7 bits, exact in fp16 as in fp32 -- and so is every piece of the streaming form: D <= 16 x 15 x 143 and
        |scale (D - 128 X)| + |bias X| <= 16 x 15 x 15 x 3 + 31 x 16 x 15 units of 2^(t - 3) per piece, (that) K / 16 < 2^24 in all (0.21 /
        0.56 of 2^24).  Weights have std 26.3 units: output std 0.80 and 1.30.
      W8A8: integer codes |i| <= 15 on both sides, sa and sw = c 2^e with c in {4, 5, 6, 7} / 4 (3 significant bits): sa sw has at most 6
        bits and acc at most 225 K < 2^18 (K <= 640): fl(sa sw) = sa sw and acc (sa sw) are exact (49 x 225 K < 2^24, asserted).
    The builder asserts the bounds by arithmetic, the fp64 product against an int64 product, fp16 exactness of 4-bit weights and scales,
    that nothing is subnormal, >= 1 % rounding ties and >= 50 % sums that are no bf16 value.  Scales and biases are drawn per group and
    per row: a wrong group or row index changes the value.
  * SPIKES: rows of x (W8A8: of A8) carry at most 4 non-zeros at the case's hot K positions: 0 and K - 1; for the streaming body right
    behind them the 512-element edges (every lane-load and stage edge of the e4m3 and 4-bit policies -- 1024 elements a lane load -- is
    one of them), shared out over the cases of one K by Case.hot_rot; the first and last 16-, 32-, 64-, 128- and 256-element edges (the
    e4m3 16-byte loads, the 4-bit pieces, groups and 256-weight blocks, the W8A8 K-step), the K / 8 wave slices.  x: 8-bit mantissas,
    exponents in [-6, 6]; A8: any non-zero finite code, subnormals and +-448 included.  W is dense: e4m3 bytes uniform over the 254
    finite patterns (0x7F / 0xFF excluded) with full-mantissa fp32 row scales; 4-bit random codes and full-mantissa bf16 scales, half the
    groups with bias = bf16(-7.5 scale) (what mlx_quantize produces: q scale + bias needs <= 11 bits), the other half |bias| up to
    64 |scale| with a mantissa of its own -- only those need more than 11 bits, so only on them the fp16 rounding bites (asserted: it
    changes >= 25 % of those weights).  For the 4-bit streaming form a row has at most one spike per 16-weight piece (asserted): D, X
    and D - 128 X are then exact and a piece contributes one rounding.
    E = (nnz + 8) 2^-23 sum_k |x_k w_k| (+ |resid|) as proj_probe derives it (w carries the scales), then the bracket on every element.
  * Fused RMSNorm: proj_probe's fold scheme -- rows +-c_m, norm weights 2^0 / 2^-1, weights j 2^s with |j| <= 3: e4m3 codes j under a
    power-of-two row scale, 4-bit q = 3 +- j in 0 .. 6 with bias = -3 scale.  k_gemv_mfma_f8 multiplies the dot product of bf16(x w) by r
    afterwards (k_gemv_mfma's rule, smaller c_m); the streaming body, k_gemv_mfma8_f8 and k_gemv8_q4 normalise every element to
    bf16(bf16(x r) w) first.  >= 3 of 4 rows are kept.
  * RANGE (k_gemv8_q4 and k_gemm_rows_q4 only, tag "range"): SPIKES with group scales in [2^-17, 2^-14) -- fp16 subnormals, still exact
    with their 8 bits -- biases in [2^-17, 2^-11) and activations in [2^-14, 2^15]: inside what fp16 holds, and the bracket holds.

MEMORY.  The GEMVs have no strides: their outputs sit between GUARD sentinel elements.  p3v_gemm_fp8 always runs with lda = K + 16,
ldw = K + 48 (padding 0x7E = 448), the output and the in-place residual in a [M + 3, N + 8] buffer inside the guards; everything outside
[M, N] and every operand must come back bit-identical.
"""
import math
from dataclasses import dataclass
from functools import lru_cache

import torch

import proj_probe as pp
from glue_probe import BF16, F32, F64, GUARD, _gen, bracket, needed_scale, to_bf16, unique_share, worst, worst_abs  # noqa: F401 (re-exported for the tests)
from proj_probe import EPS, MIN_KEPT, MIN_UNIQUE, NNZ, NONE, OUT_F32, RESID_BF16, SILU, pinned, sentinel  # noqa: F401 (pinned: a QCase's `fmt` names its entry)

F16, F8, U8 = torch.float16, torch.float8_e4m3fn, torch.uint8
FAMILIES = pp.FAMILIES
PAD8 = 0x7E                              # what the padding of A8 and W8 holds (448)
S_F8, T_Q4 = -10, -11                    # GRID: e4m3 row scales c 2^s, 4-bit scales / biases in units 2^t (module docstring)
NIB_POS = (0, 16, 4, 20, 8, 24, 12, 28)  # include/p3v.h: weights 8d .. 8d + 7 in dword d


@dataclass(frozen=True)
class QCase(pp.Case):
    fmt: str = "f8"              # "f8" (p3v_gemv_fp8) | "q4" (p3v_gemv_q4) | "w8a8" (p3v_gemm_fp8)

    @property
    def id(self):
        return f"{self.fmt}-{super().id}"

    @property
    def stream(self):
        return self.kernel.startswith("k_gemv3")

    @property
    def rows_q4(self):
        return self.kernel in ("k_gemv8_q4", "k_gemm_rows_q4")

    @property
    def range(self):
        return self.tag == "range"


# ---------------------------------------------------------------- the table, derived from the dispatch code
def _cases():
    c = []
    rot = {}                                   # (kernel, K) -> where the next plain case of that kernel and K goes on in the hot list

    def gv(kernel, fmt, M, N, K, epi, knobs=(), **kw):
        at = rot.get((kernel, K), 0)
        if not kw.get("norm") and not kw.get("tag"):
            rot[kernel, K] = at + NNZ * M
            kw["hot_rot"] = at
        return QCase(kernel, M, N, K, epi, knobs=knobs, entry="gemv", fmt=fmt, **kw)

    # the streaming body, M = 1: N = 2 (one row pair), 130, 4102 (several stages a wave, the last wave short); K = 3072 (1 stage x 3 lane
    # loads) and 8192 (2 x 4).  A case has one row of 4 spikes: the plain cases of one kernel and K walk the hot list
    # on from one another (every GEMV group: gv)
    for fmt, pol in (("f8", "GemvF8"), ("q4", "GemvQ4")):
        for N, K, epi, kw in ((4102, 3072, NONE, {}), (130, 3072, RESID_BF16, {}), (2, 3072, NONE, {}), (130, 3072, SILU, {}), (2, 3072, OUT_F32, {}),
                              (4102, 3072, RESID_BF16, {"inplace": True}),
                              (130, 8192, RESID_BF16, {"inplace": True}), (2, 8192, SILU, {}), (4102, 8192, RESID_BF16, {}), (130, 8192, OUT_F32, {}),
                              (2, 8192, NONE, {}), (130, 8192, NONE, {}), (130, 8192, SILU, {}), (2, 8192, RESID_BF16, {}),
                              (130, 3072, NONE, {"norm": True}), (130, 8192, RESID_BF16, {"norm": True}), (2, 3072, SILU, {"norm": True}),
                              (2, 8192, NONE, {"norm": True})):
            c.append(gv(f"k_gemv3<{pol}>", fmt, 1, N, K, epi, **kw))
    # k_gemv_mfma_f8: 2 .. 4 and 9 .. 16 rows, and 5 .. 8 rows when k_gemv_mfma8_f8 is switched off; N = 24, 100, 264: a ragged last 16-row block
    on, off = (("gemv_no_mfma8", 0),), (("gemv_no_mfma8", 1),)
    for M, N, K, epi, knobs, kw in ((2, 24, 3072, NONE, on, {}), (4, 100, 8192, RESID_BF16, on, {}), (9, 264, 3072, SILU, on, {}), (16, 100, 3072, OUT_F32, on, {}),
                                    (5, 24, 8192, SILU, off, {}), (8, 264, 8192, RESID_BF16, off, {"inplace": True}), (16, 24, 8192, NONE, on, {}),
                                    (9, 100, 3072, RESID_BF16, on, {}), (4, 100, 3072, NONE, on, {"norm": True}), (8, 24, 8192, RESID_BF16, off, {"norm": True}),
                                    (9, 264, 3072, SILU, on, {"norm": True})):
        c.append(gv("k_gemv_mfma_f8", "f8", M, N, K, epi, knobs, **kw))
    # k_gemv_mfma8_f8: 5 .. 8 rows, the <4, 6> (K = 3072) and <8, 8> (K = 8192) instances, SiLU and plain
    for M, N, K, epi, kw in ((5, 24, 3072, NONE, {}), (8, 100, 8192, SILU, {}), (8, 264, 3072, RESID_BF16, {}), (5, 264, 8192, OUT_F32, {}),
                             (5, 100, 3072, SILU, {}), (8, 24, 8192, RESID_BF16, {"inplace": True}), (5, 100, 3072, NONE, {"norm": True}),
                             (8, 24, 8192, SILU, {"norm": True})):
        c.append(gv("k_gemv_mfma8_f8", "f8", M, N, K, epi, on, **kw))
    # k_gemv8_q4: 2 .. 8 rows; N = 16, 80, 272 (SiLU: 8, 40, 136): 1, 5 and 17 row sets.  gemv_q4_rows_wgs = 2: two workgroups walk them -- one
    # set (the last-set copy alone), 3 + 2 and 9 + 8 (the refill copy, both parities of cpart, then the last-set copy)
    r8 = (("gemv_q4_rows8", 1), ("gemv_q4_rows_wgs", 2))
    for M, N, K, epi, kw in ((2, 16, 3072, NONE, {}), (5, 80, 8192, RESID_BF16, {}), (8, 272, 3072, OUT_F32, {}), (8, 136, 8192, SILU, {}),
                             (5, 40, 3072, SILU, {}), (2, 272, 8192, NONE, {}), (8, 80, 3072, RESID_BF16, {"inplace": True}), (5, 8, 8192, SILU, {}),
                             (5, 80, 3072, NONE, {"norm": True}), (8, 272, 8192, RESID_BF16, {"norm": True}), (2, 40, 3072, SILU, {"norm": True}),
                             (8, 80, 3072, NONE, {"tag": "range"}), (5, 272, 8192, RESID_BF16, {"tag": "range"})):
        c.append(gv("k_gemv8_q4", "q4", M, N, K, epi, r8, **kw))
    # k_gemm_rows_q4: 9 .. 16 rows, and 2 .. 8 rows when k_gemv8_q4 is switched off; no fused norm
    hi, lo = (("gemv_q4_rows8", 1), ("gemv_q4_rows_wgs", 2)), (("gemv_q4_rows8", 0), ("gemv_q4_rows_wgs", 2))
    for M, N, K, epi, knobs, kw in ((9, 16, 3072, NONE, hi, {}), (16, 80, 8192, RESID_BF16, hi, {}), (2, 272, 3072, OUT_F32, lo, {}), (8, 136, 8192, SILU, lo, {}),
                                    (16, 40, 3072, SILU, hi, {}), (9, 272, 8192, NONE, hi, {}), (8, 80, 3072, RESID_BF16, lo, {"inplace": True}),
                                    (16, 80, 8192, OUT_F32, hi, {}), (16, 80, 8192, NONE, hi, {"tag": "range"}), (2, 272, 3072, RESID_BF16, lo, {"tag": "range"})):
        c.append(gv("k_gemm_rows_q4", "q4", M, N, K, epi, knobs, **kw))

    # k_gemm256_f8: M = 1, 255, 257, 300 (one row, a tile less one, a tile plus one, ragged second tile); K = 128 (one step), 256, 384, 640 (both
    # parities of the double buffer); gemm_f8_narrow 0 / 1 pins the tile, N = 384 (no multiple of 256) takes the narrow one whatever the knob
    # says and SILU_MUL always the wide one
    def mm(M, N, K, epi, narrow, **kw):
        wide = epi == SILU or (N % 256 == 0 and narrow == 0)
        return QCase("k_gemm256_f8<wide>" if wide else "k_gemm256_f8<narrow>", M, N, K, epi, knobs=(("gemm_f8_narrow", narrow),), ld=True, entry="gemm",
                     fmt="w8a8", **kw)
    c += [mm(1, 256, 128, NONE, 0), mm(255, 256, 256, RESID_BF16, 0), mm(257, 256, 384, NONE, 0), mm(300, 256, 640, RESID_BF16, 0, inplace=True),
          mm(300, 128, 256, SILU, 0), mm(1, 128, 640, SILU, 1), mm(257, 256, 128, SILU, 0), mm(255, 384, 384, SILU, 1),
          mm(1, 256, 640, RESID_BF16, 1), mm(255, 256, 128, NONE, 1), mm(257, 256, 256, RESID_BF16, 1, inplace=True), mm(300, 256, 384, NONE, 1),
          mm(300, 384, 256, NONE, 0), mm(257, 384, 640, RESID_BF16, 1), mm(1, 384, 128, NONE, 0)]
    # tile order: 5 x 3 = 15 narrow workgroups = 1 per XCD + a remainder of 7, two bands (4 + 1 rows of tiles), the launcher's own choice of tile
    c.append(mm(1100, 384, 128, NONE, -1, tag="order"))
    c.append(mm(1100, 384, 128, RESID_BF16, -1, tag="order"))
    return tuple(c)


CASES = _cases()
GEMV_CASES = tuple(c for c in CASES if c.entry == "gemv")
GEMM_CASES = tuple(c for c in CASES if c.entry == "gemm")
assert len({c.id for c in CASES}) == len(CASES)


def group(case):
    """The kernel group of a case: the seven of the issue."""
    return f"k_gemv3<{'GemvF8' if case.fmt == 'f8' else 'GemvQ4'}>" if case.stream else case.kernel.split("<")[0]


GROUPS = tuple(dict.fromkeys(group(c) for c in CASES))


def hot_k(case):
    """The hot K positions of a case, in order of priority.  Edge pairs (e - 1, e) only, and position 0 not next to 15: four consecutive
    entries never share a 16-weight piece (asserted by the 4-bit builder)."""
    K = case.K
    pos = [0, K - 1]
    if case.stream:
        pos += [512 * j + d for j in range(1, K // 512) for d in (-1, 0)]
    for e in (32, 64, 128, 256, 16):
        pos += [e - 1, e]
    for e in (16, 32, 64, 128, 256):
        pos += [K - e, K - e - 1]
    pos += [j * (K // 8) + d for j in range(1, 8) for d in (-1, 0)]
    seen = []
    for p in pos:
        if 0 <= p < K and p not in seen:
            seen.append(p)
    return seen


def f8_decode(b):
    """e4m3 bytes -> fp32 values (exact)."""
    return b.contiguous().view(F8).float()


def f8_encode(v):
    """Values that ARE e4m3 numbers -> their bytes (asserted exact)."""
    b = v.to(F32).to(F8)
    assert torch.equal(b.float(), v.to(F32))
    return b.view(U8)


def q4_pack(q, scale, bias):
    """q [rows, K] in 0 .. 15, bf16 scale / bias [rows, K / 64] -> the device layout of include/p3v.h: W4 [rows, K / 8] and SB [rows, K / 64] int32."""
    w = (q.to(torch.int64).view(q.shape[0], -1, 8) << torch.tensor(NIB_POS)).sum(-1)
    s16 = scale.view(torch.int16).to(torch.int64) & 0xFFFF
    b16 = bias.view(torch.int16).to(torch.int64) & 0xFFFF
    sb = s16 | (b16 << 16)
    i32 = lambda t: torch.where(t >= 2 ** 31, t - 2 ** 32, t).to(torch.int32).contiguous()
    return i32(w), i32(sb)


def _finite_bytes(gen, shape, nonzero=False):
    """e4m3 bytes uniformly over the finite patterns (0x7F and 0xFF excluded; nonzero: 0x00 and 0x80 too)."""
    if nonzero:
        v = torch.randint(0, 252, shape, generator=gen)
        return torch.where(v < 126, v + 1, v - 126 + 0x81).to(U8)
    v = torch.randint(0, 254, shape, generator=gen)
    return torch.where(v < 127, v, v - 127 + 0x80).to(U8)


def _full_f32(gen, shape, e_lo, e_hi):
    """Positive fp32 values with all 24 mantissa bits drawn, exponents in [e_lo, e_hi]."""
    m = 1.0 + torch.randint(0, 2 ** 23, shape, generator=gen).to(F64) * 2.0 ** -23
    return (m * 2.0 ** torch.randint(e_lo, e_hi + 1, shape, generator=gen).to(F64)).to(F32)


def _full_bf16(gen, shape, e_lo, e_hi):
    """bf16 values of either sign with all 8 mantissa bits drawn."""
    m = (128 + torch.randint(0, 128, shape, generator=gen)).to(F64) / 128
    sign = torch.randint(0, 2, shape, generator=gen).to(F64) * 2 - 1
    return to_bf16(sign * m * 2.0 ** torch.randint(e_lo, e_hi + 1, shape, generator=gen).to(F64))


class QProbe(pp.Probe):
    """proj_probe.Probe on quantised operands: self.W is the fp64 weight the kernel's arithmetic defines (scales included), self.A the bf16
    activations (W8A8: the decoded codes of A8, self.sa the row scales); codes, scales and packed words are kept for the kernel and the
    restatement."""

    def __init__(self, case, family, seed=0):
        self.case, self.family, c = case, family, case
        assert family in FAMILIES
        self.grid = family == "grid"
        M, N, K = c.M, c.N, c.K
        self.bias = self.resid = self.pos = self.norm_w = None
        gen = _gen("qproj", c.id, family, seed)
        if c.fmt == "w8a8":
            self._inputs_w8a8(gen)
        elif c.norm:
            self._inputs_norm(gen)
        elif c.fmt == "f8":
            self._inputs_f8(gen)
        else:
            self._inputs_q4(gen)
        if c.epi == RESID_BF16 and self.resid is None:
            self.resid = to_bf16(pp._rand_int(gen, (M, N), 15) / 8) if self.grid else to_bf16(torch.randn((M, N), generator=gen))
        A64 = self.A.to(F64) * (self.sa.to(F64)[:, None] if c.fmt == "w8a8" else 1.0)
        self.acc = A64 @ self.W.T                                       # [M, Nw] fp64; GRID: exact (asserted below)
        self.absacc = None if self.grid else A64.abs() @ self.W.abs().T
        self.out_rows, self.row_map = M, torch.arange(M)
        self.rows_buf, self.ldo = M + (3 if c.ld else 0), N + (8 if c.ld else 0)
        self.lda, self.ldw = K + (16 if c.ld else 0), K + (48 if c.ld else 0)
        self.out_dtype = F32 if c.epi == OUT_F32 else BF16
        self.inplace = c.inplace and self.resid is not None
        if self.grid and not c.norm:
            self._assert_grid()
        elif c.norm:
            assert 2 * 3 * K < 2 ** 16
        if c.epi == SILU:                                               # (E_s is derived for an exponential far from the flush-to-zero range)
            gate = self.acc[:, :N].abs() / (self.A[:, :1].to(F64).abs() if c.norm else 1.0)
            assert float(gate.max()) <= (8.0 if self.grid or c.norm else 32.5)
        self._assert_normal()

    @property
    def scale_after(self):
        return self.case.kernel == "k_gemv_mfma_f8"

    @property
    def label(self):
        return "range" if self.case.range and not self.grid else "grid-sparse" if self.case.norm and not self.grid else self.family

    # ---- activations
    def _x_grid(self, gen):
        a = pp._rand_int(gen, (self.case.M, self.case.K), 15)
        a[(a == 0).all(-1), 0] = 1.0
        return to_bf16(a / 8)

    def _spike_at(self):
        c = self.case
        hot = hot_k(c)
        assert len(hot) >= NNZ
        self.hot, self.hit = hot, min(NNZ * c.M, len(hot))
        return torch.tensor(hot)[(c.hot_rot + NNZ * torch.arange(c.M)[:, None] + torch.arange(NNZ)[None]) % len(hot)]

    def _x_spikes(self, gen, e_lo=-6, e_hi=6):
        c = self.case
        at = self._spike_at()
        mant = (128 + torch.randint(0, 128, (c.M, NNZ), generator=gen)).to(F64) / 128
        e = torch.randint(e_lo, e_hi + 1, (c.M, NNZ), generator=gen).to(F64)
        sign = torch.randint(0, 2, (c.M, NNZ), generator=gen).to(F64) * 2 - 1
        a = torch.zeros((c.M, c.K), dtype=F64)
        a[torch.arange(c.M)[:, None], at] = sign * mant * 2.0 ** e
        return to_bf16(a)

    def _tame_gate(self, x64, w64):
        """SPIKES under SILU_MUL: the power of two (<= 1) per gate row that keeps |gate| <= 32 (proj_probe scales such a row of W down)."""
        g = (x64 @ w64[:self.case.N].T).abs().amax(0)
        return 2.0 ** -torch.ceil(torch.log2(g / 32.0).clamp_min(0))

    # ---- e4m3 GEMVs
    def _inputs_f8(self, gen):
        c = self.case
        Nw, K = c.w_rows, c.K
        if self.grid:
            self.A = self._x_grid(gen)
            j = pp._rand_int(gen, (Nw, K), 15)
            j[(j == 0).all(-1), 0] = 1.0
            self.W8 = f8_encode(j)
            self.wscale = (torch.randint(4, 8, (Nw,), generator=gen).to(F64) / 4 * 2.0 ** S_F8).to(F32)
        else:
            self.A = self._x_spikes(gen)
            self.W8 = _finite_bytes(gen, (Nw, K))
            self.wscale = _full_f32(gen, (Nw,), -10, -6)
        self._finish_f8()

    def _finish_f8(self):
        c = self.case
        codes = f8_decode(self.W8).to(F64)
        if c.epi == SILU and not self.grid and not c.norm:
            self.wscale[:c.N] = (self.wscale[:c.N].to(F64) * self._tame_gate(self.A.to(F64), codes * self.wscale.to(F64)[:, None])).to(F32)
        self.W = codes * self.wscale.to(F64)[:, None]

    # ---- 4-bit
    def _inputs_q4(self, gen):
        c = self.case
        Nw, K, G = c.w_rows, c.K, c.K // 64
        self.q = torch.randint(0, 16, (Nw, K), generator=gen, dtype=torch.int16)
        if self.grid:
            self.A = self._x_grid(gen)
            sc = (torch.randint(1, 4, (Nw, G), generator=gen) * (torch.randint(0, 2, (Nw, G), generator=gen) * 2 - 1)).to(F64)
            bi = torch.randint(-31, 32, (Nw, G), generator=gen).to(F64)
            self.scale, self.qbias = to_bf16(sc * 2.0 ** T_Q4), to_bf16(bi * 2.0 ** T_Q4)
            # the streaming form, piece by piece and in all: (module docstring)
            assert 16 * 15 * (128 + 15) < 2 ** 24 and (16 * 15 * 15 * 3 + 31 * 16 * 15) * K // 16 < 2 ** 24
        elif c.range:
            self.A = self._x_spikes(gen, -14, 14)
            self.scale, self.qbias = _full_bf16(gen, (Nw, G), -17, -15), _full_bf16(gen, (Nw, G), -17, -12)
            assert float(self.scale.to(F64).abs().max()) < 2.0 ** -14 and float(self.A.to(F64).abs().max()) <= 2.0 ** 15
        else:
            self.A = self._x_spikes(gen)
            self.scale = _full_bf16(gen, (Nw, G), -7, -3)
            far = torch.rand((Nw, G), generator=gen) < 0.5               # |bias| = |scale| m 2^u, u in -2 .. 5: up to 64 |scale|, a mantissa of its own
            m = (128 + torch.randint(0, 128, (Nw, G), generator=gen)).to(F64) / 128
            sg = torch.randint(0, 2, (Nw, G), generator=gen).to(F64) * 2 - 1
            u = torch.randint(-2, 6, (Nw, G), generator=gen).to(F64)
            s64 = self.scale.to(F64)
            self.qbias = to_bf16(torch.where(far, sg * m * 2.0 ** (torch.floor(torch.log2(s64.abs())) + u), -7.5 * s64))
            self.far = far
        if c.stream and not self.grid:                                 # at most one spike per 16-weight piece: D, X, D - 128 X exact
            assert int((self.A != 0).view(c.M, K // 16, 16).sum(-1).max()) <= 1
        self._finish_q4()

    def _weights_q4(self, scale, qbias):
        """(the exact q scale + bias, the weight of this case's kernel) in fp64."""
        exact = self.q.to(F64) * scale.to(F64).repeat_interleave(64, 1) + qbias.to(F64).repeat_interleave(64, 1)
        if not self.case.rows_q4:
            return exact, exact
        assert torch.equal(exact.to(F32).to(F64), exact), "q scale + bias is not exact in fp32: the fp16 conversion would round twice"
        return exact, exact.to(F32).to(F16).to(F64)

    def _finish_q4(self):
        c = self.case
        if c.epi == SILU and not self.grid and not c.norm:
            t = self._tame_gate(self.A.to(F64), self._weights_q4(self.scale, self.qbias)[1])[:, None]
            self.scale[:c.N], self.qbias[:c.N] = to_bf16(self.scale[:c.N].to(F64) * t), to_bf16(self.qbias[:c.N].to(F64) * t)
        for t in (self.scale, self.qbias):                             # what the 2 .. 16 row kernels convert to fp16 is an fp16 value (GRID: everywhere)
            assert not (c.rows_q4 or self.grid) or torch.equal(t.to(F16).to(F64), t.to(F64)), "a scale or bias that fp16 does not hold"
        assert not c.rows_q4 or torch.equal(self.A.to(F16).to(F64), self.A.to(F64))
        exact, self.W = self._weights_q4(self.scale, self.qbias)
        if self.grid or c.norm:
            assert torch.equal(exact.to(F16).to(F64), exact), "a GRID weight that fp16 does not hold"
        elif c.rows_q4 and not c.range:
            far = self.far.repeat_interleave(64, 1)
            self.bites = float((self.W != exact)[far].double().mean())
            assert self.bites >= 0.25, f"{c.id}: the fp16 rounding changes only {self.bites:.1%} of the wide-bias weights"
        self.W4, self.SB = q4_pack(self.q, self.scale, self.qbias)

    # ---- the norm fold (proj_probe._inputs_norm on codes)
    def _inputs_norm(self, gen):
        c = self.case
        M, K, Nw = c.M, c.K, c.w_rows
        self.s = s = math.floor(math.log2(1.3 / (2.2 * 0.8 * math.sqrt(K))))
        cm = to_bf16(0.5 + 3.0 * torch.rand((M, 1), generator=gen)).to(F64)
        if self.scale_after:
            cm = cm * 2.0 ** -7
        sign = torch.randint(0, 2, (M, K), generator=gen).to(F64) * 2 - 1
        self.A = to_bf16(sign * cm)
        self.norm_w = to_bf16(2.0 ** -torch.randint(0, 2, (K,), generator=gen).to(F64))
        j = pp._rand_int(gen, (Nw, K), 3)
        if not self.grid:
            j = j * (torch.rand((Nw, K), generator=gen) < 0.25)
            self.s = s = s + 1
        j[(j == 0).all(-1), 0] = 1.0
        if c.epi == RESID_BF16:
            self.resid = to_bf16(pp._rand_int(gen, (M, c.N), 15) / 8)
        if c.fmt == "f8":
            self.W8 = f8_encode(j)
            self.wscale = (2.0 ** (s - torch.arange(Nw) % 2).to(F64)).to(F32)          # powers of two, not the same on neighbouring rows
            self._finish_f8()
        else:
            sg = (torch.randint(0, 2, (Nw, K // 64), generator=gen) * 2 - 1).to(F64)
            self.q = (sg.repeat_interleave(64, 1) * j + 3).to(torch.int16)             # in 0 .. 6; scale (q - 3) = j 2^s
            self.scale, self.qbias = to_bf16(sg * 2.0 ** s), to_bf16(-3 * sg * 2.0 ** s)
            self._finish_q4()
            assert torch.equal(self.W, j.to(F64) * 2.0 ** s)

    # ---- W8A8
    def _inputs_w8a8(self, gen):
        c = self.case
        M, N, K, Nw = c.M, c.N, c.K, c.w_rows
        if self.grid:
            a, w = pp._rand_int(gen, (M, K), 15), pp._rand_int(gen, (Nw, K), 15)
            a[(a == 0).all(-1), 0] = 1.0
            w[(w == 0).all(-1), 0] = 1.0
            self.A8, self.W8 = f8_encode(a), f8_encode(w)
            st = math.floor(math.log2(1.3 / (80.0 * 1.97 * math.sqrt(K))))          # products 8.94^2, rms c^2 = 1.97: output std <= 1.3
            c4 = lambda n: torch.randint(4, 8, (n,), generator=gen).to(F64) / 4
            self.sa, self.wscale = (c4(M) * 2.0 ** (st // 2)).to(F32), (c4(Nw) * 2.0 ** (st - st // 2)).to(F32)
            assert 49 * 225 * K < 2 ** 24                                        # acc (sa sw) is exact, and sa sw has 6 bits
        else:
            at = self._spike_at()
            self.A8 = torch.zeros((M, K), dtype=U8)
            self.A8[torch.arange(M)[:, None], at] = _finite_bytes(gen, (M, NNZ), nonzero=True)
            self.W8 = _finite_bytes(gen, (Nw, K))
            self.sa, self.wscale = _full_f32(gen, (M,), -8, -4), _full_f32(gen, (Nw,), -8, -4)
        self.A = f8_decode(self.A8)                                              # [M, K] fp32: the codes' values
        codes = f8_decode(self.W8).to(F64)
        if c.epi == SILU and not self.grid:
            x64 = self.A.to(F64) * self.sa.to(F64)[:, None]
            self.wscale[:N] = (self.wscale[:N].to(F64) * self._tame_gate(x64, codes * self.wscale.to(F64)[:, None])).to(F32)
        self.W = codes * self.wscale.to(F64)[:, None]

    # ---- the builder's assertions
    def _assert_grid(self):
        c = self.case
        M, N, K = c.M, c.N, c.K
        if c.fmt == "q4":
            unit, top = 2.0 ** (T_Q4 - 3), 15 * 76 * K
            ai, wi = (self.A.to(F64) * 8).to(torch.int64), (self.W * 2.0 ** -T_Q4).to(torch.int64)
        elif c.fmt == "f8":
            unit, top = 2.0 ** (S_F8 - 5), 225 * K * 7                # (scales: integers 4 .. 7 of 2^(s - 2))
            ai, wi = (self.A.to(F64) * 8).to(torch.int64), (self.W * 2.0 ** (2 - S_F8)).to(torch.int64)
        else:
            ea, ew = (math.floor(math.log2(float(t.min()))) for t in (self.sa, self.wscale))
            unit, top = 2.0 ** (ea + ew - 4), 49 * 225 * K
            ai = (self.A.to(F64) * self.sa.to(F64)[:, None] * 2.0 ** (2 - ea)).to(torch.int64)
            wi = (self.W * 2.0 ** (2 - ew)).to(torch.int64)
        assert top < 2 ** 24, "partial sums leave the exact range of fp32"
        rows = torch.arange(M) if M * c.w_rows * K <= 2 ** 23 else torch.tensor(sorted({0, M // 2, M - 1}))
        cols = torch.arange(0, c.w_rows, -(-len(rows) * c.w_rows * K // 2 ** 23))
        assert torch.equal((ai[rows] @ wi[cols].T).to(F64) * unit, self.acc[rows][:, cols]), "the fp64 reference is not exact"
        f = self.acc[:, :N].to(F32)
        assert torch.equal(f.to(F64), self.acc[:, :N])
        ties = self._tie_share()
        unrep = float((f.to(BF16).to(F64) != f.to(F64)).double().mean())
        assert ties >= 0.01 and unrep >= 0.5, f"{c.id}: {ties:.3%} rounding ties, {unrep:.1%} sums that are no bf16 value"
        self.ties, self.unrep = ties, unrep

    def _assert_normal(self):
        tiny = 2.0 ** -126
        for t in (self.A, self.W, self.resid, self.acc, getattr(self, "sa", None), getattr(self, "wscale", None)):
            if t is not None:
                v = t.abs()
                assert not bool(((v > 0) & (v < tiny)).any()), "a subnormal operand or sum"

    # ---- buffers (the W8A8 operands; the GEMVs pass their tensors as they are)
    def operand_buffers(self):
        c = self.case
        a = torch.full((c.M, self.lda), PAD8, dtype=U8)
        w = torch.full((c.w_rows, self.ldw), PAD8, dtype=U8)
        a[:, :c.K], w[:, :c.K] = self.A8, self.W8
        return a, w

    # ---- the documented arithmetic in torch fp32, with defects
    def _slices(self, order):
        """The K slices a restatement adds up, in `order` -- "seq": in order; "rev": from the end; "tiled": as four K quarters, each
        summed on its own and the four added in order (the waves of the MFMA kernels)."""
        K = self.case.K
        w = 32 if K <= 1024 else 256
        sl = [(k, k + w) for k in range(0, K, w)]
        if order == "rev":
            return [sl[::-1]]
        if order == "tiled":
            per = max(1, len(sl) // 4)
            return [sl[i:i + per] for i in range(0, len(sl), per)]
        return [sl]

    def restate(self, order="seq", defect=None):
        """The flat output buffer as a kernel leaves it that computes in fp32 what include/p3v.h and the kernel sources document, summing
        in `order`; `defect`: see tests/test_qproj_probe_cpu.py."""
        c, d = self.case, defect
        M, N, K = c.M, c.N, c.K
        x = self.A.float().clone()
        if d == "lda_as_k":
            x = f8_decode(self.operand_buffers()[0].flatten()[:M * K].view(M, K))
        r_after = None
        if c.norm:
            x, r_after = self._restate_norm(x)
        if d == "drop_k0":
            x[:, 0] = 0
        if d == "drop_klast":
            x[:, K - 1] = 0
        mid = (K // 32) * 16                                             # a 16-weight piece / the K-step in the middle
        span = slice(K // 256 * 128, K // 256 * 128 + 128) if c.fmt == "w8a8" else slice(mid, mid + 16)
        if d == "drop_piece":
            x[:, span] = 0
        if d == "piece_twice":
            x[:, span] *= 2
        if d == "x_trunc":                                               # the lowest mantissa bit lost on the way to fp16
            x = (x.to(BF16).view(torch.int16) & -2).view(BF16).float()
        if c.fmt == "q4":
            acc = self._restate_q4(x, order, d)
        else:
            acc = self._restate_f8(x, order, d)
        if r_after is not None:
            acc = acc * r_after
        out = self._epilogue(acc, d)
        flat = self.out_buffer()
        self.window_put(flat, out)
        if d == "row_m_twice":
            at = GUARD + M * self.ldo
            n = min(N, flat.numel() - at)
            flat[at:at + n] = out[-1, :n].to(self.out_dtype)
        return flat

    def _ksum(self, f, order):
        acc = None
        for part in self._slices(order):
            t = None
            for k0, k1 in part:
                v = f(k0, k1)
                t = v if t is None else t + v
            acc = t if acc is None else acc + t
        return acc

    def _restate_f8(self, x, order, d):
        """e4m3: the sum of x . code first, the scale afterwards (W8A8: acc (sa sw), one fp32 product of the two scales)."""
        c = self.case
        b = self.W8
        if d == "pair_swap":                                             # the two bytes of every 16-bit pair
            b = b.view(c.w_rows, -1, 2).flip(-1).reshape(c.w_rows, c.K)
        codes = f8_decode(b)
        if d == "flush_subnormal":
            codes = torch.where(codes.abs() < 2.0 ** -6, torch.zeros_like(codes), codes)
            if c.fmt == "w8a8":
                x = torch.where(x.abs() < 2.0 ** -6, torch.zeros_like(x), x)
        acc = self._ksum(lambda k0, k1: x[:, k0:k1] @ codes[:, k0:k1].T, order)
        sw = self.wscale.clone()
        if d == "silu_scale_n":
            sw[c.N:] = sw[:c.N]
        if c.fmt != "w8a8":
            return acc * sw
        sa = self.sa
        if d == "scale_tile_local":
            tile = 128 if "narrow" in c.kernel or c.epi == SILU else 256
            sa, sw = sa[torch.arange(c.M) % 256], torch.cat([sw[:c.N][torch.arange(c.N) % tile], sw[c.N:]])
        return acc * (sa[:, None] * sw[None])

    def _restate_q4(self, x, order, d):
        c = self.case
        Nw, K = c.w_rows, c.K
        q = self.q.float()
        if d == "nibble_swap":                                           # weights 0 and 1 of every dword
            q = q.view(Nw, -1, 8)[..., [1, 0, 2, 3, 4, 5, 6, 7]].reshape(Nw, K)
        s, b = self.scale.float(), self.qbias.float()
        if d == "neighbour_scale":
            s = s.roll(1, 1)
        if d == "no_bias":
            b = torch.zeros_like(b)
        if c.rows_q4:
            # the fp16 fma of the packed dequantisation (ONE rounding of q scale + bias), x as fp16, exact products, fp32 sums
            w64 = q.to(F64) * s.to(F64).repeat_interleave(64, 1) + b.to(F64).repeat_interleave(64, 1)
            w = (w64.to(BF16) if d == "bf16_dequant" else w64.to(F32).to(F16)).float()
            x16 = x.to(F16).float()
            return self._ksum(lambda k0, k1: x16[:, k0:k1] @ w[:, k0:k1].T, order)
        # the streaming form: per 16-weight piece scale (D - 128 X) + bias X, every step one fp32 operation
        assert c.M == 1
        P = K // 16
        xp = x.view(P, 16)
        X = xp.sum(-1)                                                   # [P]
        D = torch.einsum("pj,npj->np", xp, (128.0 + q).view(Nw, P, 16))  # [Nw, P]
        Xs = X.roll(1, 0) if d == "neighbour_x" else X
        core = D if d == "keep_128" else D - 128.0 * Xs
        cpp = s.repeat_interleave(4, 1) * core + b.repeat_interleave(4, 1) * Xs
        return self._ksum(lambda k0, k1: cpp[:, k0 // 16:k1 // 16].sum(-1)[None], order)


@lru_cache(maxsize=2)
def probe(case, family):
    """The probe of a case, as proj_probe.probe: a case of fewer than 4096 outputs takes the first seed at which the conditions on the
    REFERENCE hold (of up to 256: with two outputs "a rounding tie among them" is a matter of 4 % per element).  Nothing here looks at a kernel's output."""
    small = case.M * case.N < 4096
    for seed in range(256 if small else 1):
        try:
            pr = QProbe(case, family, seed)
        except AssertionError:
            if seed == 255 or not small:
                raise
            continue
        u, k = pr.uniqueness()
        if (u >= MIN_UNIQUE and k >= MIN_KEPT) or not small:
            break
    return pr
