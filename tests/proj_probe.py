"""Probing inputs, fp64 references and acceptance rules for the bf16 projection kernels: p3v_gemm (k_gemm alone and as split-K partials
with k_splitk_reduce / k_splitk_reduce_norm, the 256 x 256 kernel, k_gemm_skinny, k_gemm_rows) and p3v_gemv (k_gemv<MT>, the K = 3072 /
8192 streaming body, k_gemv_mfma, k_gemv_mfma8).  Layout and vocabulary of tests/glue_probe.py, whose bracket / inside / worst /
needed_scale are used as they are.  Everything here is torch on the CPU: tests/test_proj_probe_cpu.py shows on the references alone that
the inputs expose each defect, tests/test_proj_kernels_gpu.py runs the kernels.

TWO INPUT FAMILIES.
  * GRID (exact sums).  A[m, k] = i 2^-3 with |i| <= 15, W[n, k] = j 2^s with |j| <= 31: every product is an integer number of UNITS
    u = 2^(s - 3), every partial sum in every order an integer below 15 * 31 * K + (added terms) < 2^24 units, hence exact in fp32.  Tile
    order, wave split, K slices and MFMA block order do not matter and the accumulator is known exactly.  Bias, bf16 residual, fp32
    residual and position table are multiples of u too (bias, residual, pos: i 2^-3, |i| <= 15; fp32 residual: i 2^-6, |i| <= 255), so
    r32 + acc + bias is exact in any order.  s per K: the largest power of two with output std <= about 1.3 (and |gate| <= 8 for
    SiLU).  The builder asserts the bound by arithmetic, the fp64 product against an int64 product, that nothing is subnormal, and
    that >= 1 % of the sums are exact bf16 rounding ties and >= 50 % are not bf16 values (K = 8, k_gemv<MT>'s one-chunk cases: 25 %
    -- eight products of at most 9 bits seldom need more than the 8 + 1 bits that decide it; measured on the reference, 33 %).
  * SPIKES (few terms, full mantissas).  Every row of A has at most 4 non-zeros (8-bit mantissas, exponents in [-6, 6]) at the
    case's HOT K positions (0, K - 1, 63 / 64, the 64-element tile edges next to every slice edge K / S - 1, K / S for S in 2, 4, 8,
    the last tile; for the GEMV stream, right behind 0 and K - 1, the edges of its 512-element lane chunks -- a stage is 6 (K = 3072)
    or 4 (K = 8192) chunks, so every stage edge is one of them); W is dense, N(0, 1) 2^e per row with e in [-3, 3].  An integer grid cannot see a
    kernel that loses operand mantissa bits; these rows do.  Row r takes hot positions 4 r .. 4 r + 3 (cyclically), so every row
    carries spikes -- row M - 1 and the last row of every 64 / 128 / 256-row tile among them -- and min(4 M, #hot) positions are hit
    (a case with fewer than #hot / 4 rows takes the head of the list, which is in order of priority).  The stream has at most 4 rows
    and so at most 16 positions a case: its plain cases of one K start where the one before stopped (Case.hot_rot), and TOGETHER
    they hit 0, K - 1 and every chunk edge (asserted on the CPU) -- with nnz <= 4 a one-row case cannot do that alone.

ONE ACCEPTANCE RULE: THE ROUNDING BRACKET (glue_probe).  The fp32 value a kernel holds before a rounding is within E of the fp64
value; rounding is monotonic, so what it stores lies in [bf16(v - E), bf16(v + E)].  Every element is checked, no shares, no atol.
E never comes from an output:
  * accumulator.  GRID: E = 0 -- `got ==` the fp64 value pushed through the roundings of include/p3v.h; fp32 outputs are equal as
    floats.  SPIKES: E = (nnz + 8) 2^-23 (sum_k |a_k w_k| + |bias| + |resid|), nnz = 4: each of the <= 4 non-zero products is exact,
    every add rounds by <= 2^-24 of a partial sum that is <= the sum of magnitudes, 8 more such steps cover the adds of zeros
    between slices and the epilogue's adds, and 2^-23 instead of 2^-24 leaves room for a truncating adder inside the matrix core.
  * NONE / BIAS / F32 / BIAS_RESID_F32 / PATCH: one rounding (or none, fp32 outputs: |got - ref| <= E) of acc (+ bias) (+ resid | pos).
  * RESID_BF16: out = bf16(r + bf16(acc)).  t = bf16(acc) lies in its bracket; r + t is ONE IEEE fp32 add of two bf16 values, which
    torch fp32 reproduces bit for bit and which is monotonic in t: the bracket is [bf16(r + t_lo), bf16(r + t_hi)].
  * SILU_MUL: out = bf16(bf16(g bf16(sigmoid(g))) u), g and u the bf16-rounded sums.  g and u each lie in a bracket whose ends are
    equal or adjacent bf16 values; for each end, sigmoid64(g) +- E_s is pushed through the three roundings (a product of two bf16
    values is exact in fp32: one rounding each) and the smallest / largest result of the 2 x 2 x 2 ends taken (glue_probe's
    RMSNorm bracket, ends ordered as floats).  E_s = (|g| + 4) 2^-22 sigmoid(g) from 1.f / (1.f + __expf(-g)): the product
    -g log2 e rounds by 2^-24 |g| log2 e, which the exponential turns into a relative 2^-24 |g|; v_exp_f32 is documented at 1 ulp
    (relative 2^-23); both act on e = exp(-g) and reach d = 1 + e scaled by e / d = 1 - sigmoid <= 1; the add rounds by 2^-24, the
    division (correctly rounded, or v_rcp_f32 at 1 ulp) by <= 2^-23: relative (|g| + 5) 2^-24 in all, taken 4 x larger.  |g| <= 8
    (GRID; SPIKES: 32, a gate row that exceeds it is scaled down by a power of two) is asserted, so neither e nor a product of the chain
    comes near the flush-to-zero range.
  * BIAS_QGELU: out = bf16(x sigmoid(1.702f x)), x = acc + bias, one rounding.  t = 1.702f x rounds by 2^-24 |t| and the sigmoid
    is the expression above (with v_rcp_f32): E = |x| (|t| + 4) 2^-22 sigmoid(t) + 2^-23 |ref| (the last multiply), + 1.2 E_acc
    (|d/dx| <= 1.1).
  * BIAS_GELU: out = bf16(0.5f x (1 + erff(x 0.70710678f))).  z rounds by 2^-24 |z| (x erf'(z) <= 1.13 exp(-z^2)); erff is bounded
    by 16 ulp (the OpenCL bound the device library is built to), 2^-20 |erf z|; the add 1 + erf rounds by <= 2^-23 ABSOLUTE, and
    for negative x, where 1 + erf cancels, that and the erff term stay absolute while the result shrinks (the LayerNorm rule's
    absolute term); two multiplies, 2^-23 |ref|:  E = 0.5 |x| (2^-20 |erf z| + 2^-24 1.13 |z| exp(-z^2) + 2^-23) + 2^-23 |ref| + 1.2 E_acc.
  * p3v_gemm_resid_norm: `out` as RESID_BF16; `normed` under glue_probe's RMSNorm bracket (relative 2^-16 on r) of the `out` the
    kernel stored (which the first rule has already pinned).
  * GEMV norm fold (k_gemv<MT> and the stream: bf16(bf16(x r) w) per element, then the dot product).  Rows x[m, k] = +-c_m: every
    normalised element is +-v_m, v = bf16(c r) one value per row under the RMSNorm bracket (relative 2^-16 on r); rows whose bracket
    holds two values are not judged (>= 3 of 4 rows are kept, asserted).  Norm weights 2^0 / 2^-1 and W = j 2^s with |j| <= 3: every
    product is v j 2^(s - 1) times 1 or 2 and every partial sum v times an integer below 6 K < 2^16, exact in fp32 with v's 8
    bits -- the accumulator is v (integer) 2^(s - 1) exactly and the epilogues follow as on GRID.  (k_gemv_mfma / k_gemv_mfma8 scale
    the dot product of bf16(x w) by r afterwards, one fp32 rounding more: acc = r64 c (integer) 2^(s - 1) under relative 2^-16; their
    c_m are 2^-7 times smaller, so that c r is percents below 1 and the many rounding ties of the integer are none of acc.)  Few-term
    rows have no meaning under a fold of whole rows: the second family of these cases is a W three quarters zero at twice the step.
On >= 98 % of the elements of every case lo == hi (asserted on the CPU).  A case of fewer than 4096 outputs cannot hold "1 % ties" or
"98 %" by the law of large numbers (M = 1, N = 8: one element is 12.5 %): it takes the first seed at which the conditions on the
REFERENCE hold (probe()); nothing here ever looks at what a kernel produced.

MEMORY.  A and W live in buffers with lda = K + 8, ldw = K + 24 in the `ld` cases, the padding holding 2^15; the output (and the
in-place residual) in a [rows + 3, ldo = N + 8] buffer; a position-dependent sentinel fills padding and GUARD elements in front and
behind (every case); everything outside [M, N] -- for PATCH: outside the remapped rows, the CLS rows (m / P) (P + 1) included -- must come
back bit-identical.  p3v_gemv has no strides: its cases are guarded only.
"""
import math
from contextlib import contextmanager
from dataclasses import dataclass
from functools import lru_cache

import torch

from glue_probe import BF16, F32, F64, GUARD, _gen, bracket, needed_scale, to_bf16, unique_share, worst, worst_abs  # noqa: F401 (needed_scale: for the tests)

NONE, BIAS, QGELU, GELU, BIAS_RESID_F32, RESID_BF16, SILU, PATCH, OUT_F32 = range(9)       # include/p3v.h: P3V_EPI_*
EPI_NAMES = ("none", "bias", "qgelu", "gelu", "biasresf32", "resid", "silu", "patch", "f32")
F32_OUT = (BIAS_RESID_F32, PATCH, OUT_F32)
FAMILIES = ("grid", "spikes")
NNZ = 4                                  # non-zeros of a SPIKES row
EPS = 1e-5
PAD = 32768.0                            # what the padding of A and W holds
C_QGELU = float(torch.tensor(1.702, dtype=F32))
C_RSQRT2 = float(torch.tensor(0.70710678118654752, dtype=F32))


@dataclass(frozen=True)
class Case:
    kernel: str                  # the kernel the knobs pin (printed with the result)
    M: int
    N: int
    K: int
    epi: int = NONE
    knobs: tuple = ()            # ((knob, value), ...) for ops.set_tuning
    ld: bool = False             # lda = K + 8, ldw = K + 24, out [rows + 3, N + 8], residual in place
    P: int = 0                   # PATCH: patches per image
    bias: bool = False           # OUT_F32 with a bias
    norm: bool = False           # p3v_gemm: through p3v_gemm_resid_norm; p3v_gemv: fused RMSNorm (constant-magnitude rows)
    inplace: bool = False        # residual aliases the output (always with ld)
    entry: str = "gemm"          # "gemm" | "gemv"
    slices: int = -1             # gemm: the plan p3v_gemm_ws_bytes must report (S; 1 = no workspace); -1 = not asserted
    rows_slices: int = -1        # gemm: what p3v_gemm_rows_slices must report; -1 = not asserted
    hot_rot: int = 0             # SPIKES: row r takes hot positions hot_rot + 4 r .. + 3 (the stream's few-row cases share the list out)
    tag: str = ""

    @property
    def id(self):
        s = f"{self.kernel}-{EPI_NAMES[self.epi]}-M{self.M}-N{self.N}-K{self.K}"
        s += "-bias" if self.bias else ""
        s += "-norm" if self.norm else ""
        s += "-ld" if self.ld else "-inplace" if self.inplace else ""
        s += f"-P{self.P}" if self.P else ""
        return s + (f"-{self.tag}" if self.tag else "")

    @property
    def w_rows(self):
        return 2 * self.N if self.epi == SILU else self.N

    @property
    def has_bias(self):
        return self.bias or self.epi in (BIAS, QGELU, GELU, BIAS_RESID_F32)


# ---------------------------------------------------------------- the table, derived from the dispatch code
def _k128(M, N, K, epi, **kw):
    return Case("k_gemm", M, N, K, epi, knobs=(("gemm_no_skinny", 1), ("gemm_no_splitk", 1), ("gemm_128", 1)), slices=1, **kw)


def _gemm_cases():
    c = []
    # k_gemm in one pass: M 1 / 127 / 129 / 200 (one row, a tile less one, a tile plus one, two tiles), N % 8 only (8, 72, 136, 264: the
    # clamped column tail), K 64 .. 704 (1 .. 11 K-tiles); every epilogue
    shapes = ((1, 8, 64), (127, 72, 128), (129, 136, 192), (200, 264, 704), (129, 128, 64), (1, 264, 192), (200, 8, 128), (127, 136, 704))
    for e, epi in enumerate((NONE, BIAS, QGELU, GELU, BIAS_RESID_F32, RESID_BF16, OUT_F32)):
        for t in range(3):
            M, N, K = shapes[(3 * e + t) % len(shapes)]
            c.append(_k128(M, N, K, epi, ld=t == 1, inplace=t == 2 and epi in (RESID_BF16, BIAS_RESID_F32)))
    c.append(_k128(129, 72, 128, OUT_F32, bias=True, ld=True))
    c += [_k128(129, 40, 128, SILU), _k128(200, 192, 704, SILU, ld=True), _k128(1, 40, 64, SILU)]
    c += [_k128(12, 72, 128, PATCH, P=5, ld=True), _k128(12, 8, 64, PATCH, P=5), _k128(200, 136, 192, PATCH, P=5)]
    # tile order: 9 x 3 = 27 workgroups = 3 per XCD + a remainder of 3, the last band one row of tiles (N = 384 is no multiple of 256:
    # no big tiles; M > gemm_splitk_max_m, gemm_skinny_max_m)
    for epi in (NONE, RESID_BF16):
        c.append(Case("k_gemm", 1100, 384, 128, epi, knobs=(("gemm_big_rows", 0),), slices=1, ld=epi == RESID_BF16, tag="order"))
    # the 256 x 256 kernel: M = 1030 as the suite pins it (512 rows big + 518 on k_gemm) and with all rows big (ragged last tile of 6 rows).
    # The third way, gemm_big_rows = -1 (the launcher's own cost model), does NOT reach it at these shapes: 9 x 2 .. 9 x 4 small workgroups
    # are one partial round (0.42) against >= 1.45 for any split with a big tile at K <= 192 (gemm_big_rows(), p3v_gemm.hip), so all
    # 1030 rows run on k_gemm -- nine tiles of rows, the last of 6.  The model picks big rows from about 1030 x 8192 x 2048 on, beyond what
    # a test of a few seconds holds in fp64; the run stays, named for the kernel it reaches.
    ways = (("pin", 512), ("all", 1000000), ("auto", -1))
    nk = ((256, 64), (512, 192), (256, 192), (512, 64))
    for e, epi in enumerate((NONE, BIAS, QGELU, GELU, BIAS_RESID_F32, RESID_BF16, SILU, OUT_F32)):      # every epilogue it takes, each three ways
        for t, (name, rows) in enumerate(ways):
            N, K = nk[(e + t) % 4]
            N = N // 2 if epi == SILU and N == 256 else N
            c.append(Case("k_gemm" if rows < 0 else "k_gemm256" if rows > 512 else "k_gemm256+k_gemm", 1030, N, K, epi,
                          knobs=(("gemm_big_rows", rows), ("gemm_128", 0)), slices=1, ld=(e + t) % 3 == 1, tag=name))
    # split-K on k_gemm + k_splitk_reduce: S = 4 at K = 512, 8 at K = 1024 and 1536 (gemm_slices)
    sk = (("gemm_no_skinny", 1), ("gemm_no_splitk", 0), ("gemm_128", 1))
    for M, N, K, epi, S, ld in ((17, 128, 512, NONE, 4, False), (129, 256, 1024, RESID_BF16, 8, True), (300, 128, 1536, SILU, 8, False),
                                (129, 128, 512, SILU, 4, True), (300, 256, 512, RESID_BF16, 4, False), (17, 256, 1536, NONE, 8, True)):
        c.append(Case("k_gemm+k_splitk_reduce", M, N, K, epi, knobs=sk, slices=S, ld=ld))
    # k_gemm_skinny: 64-row tiles up to M = 64 (gemm_skinny_tm128 = 1: 128-row tiles there too), one pass or K slices
    def skinny(M, N, K, epi, s, tm128, S, **kw):
        knobs = (("gemm_no_skinny", 0), ("gemm_skinny_s", s), ("gemm_skinny_tm128", tm128), ("gemm_rows", 1))
        return Case("k_gemm_skinny" + ("<64>" if M <= 64 and not tm128 else "<128>") + ("+k_splitk_reduce" if S > 1 and not kw.get("norm") else
                    "+k_splitk_reduce_norm" if S > 1 else ""), M, N, K, epi, knobs=knobs, slices=S, **kw)
    c += [skinny(33, 64, 64, NONE, 0, 0, 1), skinny(64, 192, 384, RESID_BF16, 0, 0, 1, ld=True), skinny(64, 96, 768, SILU, 0, 1, 2),
          skinny(65, 64, 768, NONE, 0, 0, 2, ld=True), skinny(128, 192, 384, NONE, 2, 0, 2), skinny(129, 32, 384, SILU, 1, 0, 1, ld=True),
          skinny(250, 192, 768, RESID_BF16, 0, 0, 2, ld=True), skinny(256, 64, 768, SILU, 1, 0, 1), skinny(33, 192, 768, RESID_BF16, 2, 1, 2),
          skinny(64, 64, 384, NONE, 2, 0, 2, ld=True), skinny(256, 192, 64, RESID_BF16, 0, 0, 1, inplace=True),
          skinny(33, 64, 768, RESID_BF16, 0, 0, 2, norm=True), skinny(129, 192, 384, RESID_BF16, 2, 0, 2, norm=True, ld=True),
          skinny(250, 64, 768, RESID_BF16, 0, 1, 2, norm=True, inplace=True)]
    # k_gemm_rows: 9 .. 32 rows (MT = 1 up to 16 rows, 2 above); one pass at >= 512 column sets, else four K slices
    def rows(M, N, K, epi, S, **kw):
        return Case("k_gemm_rows" + ("+k_splitk_reduce" if S > 1 else ""), M, N, K, epi, knobs=(("gemm_no_skinny", 0), ("gemm_rows", 1), ("gemm_skinny_s", 0)),
                    slices=S, rows_slices=S, **kw)
    c += [rows(9, 48, 3072, RESID_BF16, 4, ld=True), rows(32, 48, 3072, RESID_BF16, 4), rows(16, 32, 8192, RESID_BF16, 4, inplace=True),
          rows(17, 32, 8192, NONE, 4, ld=True), rows(32, 32, 8192, NONE, 4),
          rows(9, 8192, 3072, NONE, 1), rows(17, 8192, 3072, NONE, 1, ld=True), rows(16, 4096, 3072, SILU, 1), rows(32, 4096, 3072, SILU, 1, ld=True)]
    return tuple(c)


def _gemv_cases():
    c = []
    def gv(kernel, M, N, K, epi, knobs, **kw):
        return Case(kernel, M, N, K, epi, knobs=knobs, entry="gemv", **kw)
    # k_gemv<MT>: MT = 1, 2, 4, 8; odd N (a last row pair of one row), K = 8 (one chunk), 200 (25 chunks), 1000 (125: both loops)
    gen = (("gemv_variant", 1), ("gemv_no_mfma", 1), ("gemv_mfma8", 0))
    for M, N, K, epi, kw in ((1, 1, 8, NONE, {}), (2, 37, 200, RESID_BF16, {}), (3, 101, 1000, SILU, {}), (5, 37, 1000, OUT_F32, {}),
                             (8, 101, 200, NONE, {}), (1, 101, 1000, RESID_BF16, {"inplace": True}), (5, 1, 200, SILU, {}), (8, 37, 8, RESID_BF16, {}),
                             (3, 37, 1000, NONE, {"norm": True}), (1, 101, 200, RESID_BF16, {"norm": True}), (8, 37, 1000, SILU, {"norm": True})):
        c.append(gv(f"k_gemv<{1 if M <= 1 else 2 if M <= 2 else 4 if M <= 4 else 8}>", M, N, K, epi, gen, **kw))
    # the streaming body: K = 3072 (1 stage x 6 chunks) and 8192 (4 x 4), 1 / 2 / 4 x rows (gemv8_min = 5 keeps 2 .. 4 rows off k_gemv_mfma8)
    st = (("gemv_variant", 3), ("gemv_rows", 1), ("gemv8_min", 5))
    rot = {3072: 0, 8192: 0}                             # the rows of all plain cases of one K walk the hot list on from one another
    for M, N, K, epi, kw in ((1, 2, 3072, NONE, {}), (2, 130, 8192, RESID_BF16, {}), (4, 4102, 3072, NONE, {}), (1, 130, 8192, SILU, {}),
                             (2, 2, 3072, SILU, {}), (4, 130, 3072, RESID_BF16, {"inplace": True}), (1, 4102, 8192, RESID_BF16, {}), (4, 2, 8192, NONE, {}),
                             (1, 130, 3072, NONE, {"norm": True}), (2, 130, 8192, RESID_BF16, {"norm": True}), (4, 2, 3072, SILU, {"norm": True}),
                             (1, 2, 8192, NONE, {"norm": True})):
        c.append(gv(f"k_gemv3<{1 if M <= 1 else 2 if M <= 2 else 4}>", M, N, K, epi, st, hot_rot=rot[K], **kw))
        rot[K] += 0 if kw.get("norm") else NNZ * M
    # k_gemv_mfma8: 2 .. 8 rows at K = NW x NST x 256
    m8 = (("gemv_mfma8", 1), ("gemv8_min", 2), ("gemv_variant", 3))
    for M, N, K, epi, kw in ((2, 24, 1024, NONE, {}), (5, 100, 2048, RESID_BF16, {}), (8, 264, 3072, SILU, {}), (8, 100, 4096, OUT_F32, {}),
                             (5, 24, 8192, SILU, {}), (2, 264, 8192, RESID_BF16, {"inplace": True}), (8, 24, 3072, NONE, {}), (5, 264, 1024, RESID_BF16, {}),
                             (5, 100, 3072, NONE, {"norm": True}), (8, 24, 8192, SILU, {"norm": True})):
        c.append(gv("k_gemv_mfma8", M, N, K, epi, m8, **kw))
    # k_gemv_mfma: more than 8 rows at any K % 1024 == 0; up to 8 rows at the smallest such K k_gemv_mfma8 has no instance for (5120)
    mf = (("gemv_mfma8", 1), ("gemv8_min", 2), ("gemv_no_mfma", 0), ("gemv_variant", 3))
    for M, N, K, epi, kw in ((9, 24, 1024, NONE, {}), (16, 100, 2048, RESID_BF16, {}), (2, 264, 5120, SILU, {}), (5, 100, 5120, OUT_F32, {}),
                             (16, 24, 1024, SILU, {}), (9, 264, 3072, RESID_BF16, {"inplace": True}), (8, 24, 5120, NONE, {}),
                             (9, 100, 2048, RESID_BF16, {"norm": True})):
        c.append(gv("k_gemv_mfma", M, N, K, epi, mf, **kw))
    return tuple(c)


def gemv_claim(r, fmt="bf16"):
    """The kernel of an ops.gemv_route answer in the shorthand of a case's `kernel` field: k_gemv<MT>, k_gemv3<MT> (bf16) or
    k_gemv3<policy> (the other formats), and the bare template name of every other kernel."""
    name = r.name.decode()
    base = name.split("<")[0]
    if base == "k_gemv3":
        return f"k_gemv3<{r.MT}>" if fmt == "bf16" else f"k_gemv3<{name[len('k_gemv3<'):].split(',')[0].split('<')[0]}>"
    return name if base == "k_gemv" else base


@contextmanager
def pinned(ops, case, cu_count=0):
    """Pin the kernel of `case` for the call about to be made: sets the case's knobs, for a GEMV case asserts from the library's route
    (ops.gemv_route, the library's own settings; cu_count = 0: this device) that the call runs the kernel the case's `kernel` field
    claims, and restores the knobs."""
    old = [(name, ops.set_tuning(name, value)) for name, value in case.knobs]
    try:
        if case.entry == "gemv":
            fmt = {"bf16": "bf16", "f8": "fp8", "q4": "q4"}[getattr(case, "fmt", "bf16")]
            r = ops.gemv_route(case.M, case.N, case.K, case.epi, fmt=fmt, has_norm=case.norm, cu_count=cu_count)
            got = gemv_claim(r, fmt) if r.status == 0 else f"refused: {r.status}"
            assert got == case.kernel, f"pinned {case.id}: the call runs {r.name.decode() or got!r}, not {case.kernel}"
        yield
    finally:
        for name, value in reversed(old):
            ops.set_tuning(name, value)


GEMM_CASES, GEMV_CASES = _gemm_cases(), _gemv_cases()
CASES = GEMM_CASES + GEMV_CASES
assert len({c.id for c in CASES}) == len(CASES)


# ---------------------------------------------------------------- inputs
def grid_shift(K, epi=NONE):
    """s of W = j 2^s: products a w have std 1.118 x 17.9 x 2^s, a sum of K of them sqrt(K) times that; the largest s with std <= 1.3.
    The two GELUs take one step less (std <= 0.65): below x = -2.5 their results shrink faster than E (its absolute terms), and the
    brackets there hold more than one value."""
    return math.floor(math.log2(1.3 / (20.0 * math.sqrt(K)))) - (1 if epi in (QGELU, GELU) else 0)


def hot_k(case):
    """The hot K positions of a case, in order of priority."""
    K = case.K
    stream = case.kernel.startswith("k_gemv3")
    pos = [0, K - 1]
    if stream:                                           # what means most to the kernel first: its lane-chunk (and stage) edges
        pos += [512 * j + d for j in range(1, K // 512) for d in (-1, 0)]
    pos += [63, 64]
    for S in (2, 4, 8):
        if K % S == 0:
            pos += [K // S - 1, K // S]
            pos += [j * (K // S) + d for j in range(2, S) for d in (-1, 0)]
    pos += [K - 64, K - 65]
    seen = []
    for p in pos:
        if 0 <= p < K and p not in seen:
            seen.append(p)
    return seen


def sentinel(n, dtype):
    """(index % 251) + 300 in `dtype` (bf16 rounds it to steps of 2 and 4): a pattern that repeats every 251 elements, no multiple of a row
    or tile, and nothing a kernel would write; the check compares every position with this clean buffer bit for bit."""
    return (torch.arange(n) % 251 + 300).float().to(dtype)


def _rand_int(gen, shape, top):
    return torch.randint(-top, top + 1, shape, generator=gen, dtype=torch.int16).to(F32)     # (small integers: exact in fp32)


class Probe:
    """Inputs, fp64 reference, brackets, buffers and a torch restatement (with defects) of one case under one family."""

    def __init__(self, case, family, seed=0):
        self.case, self.family, c = case, family, case
        assert family in FAMILIES
        self.grid = family == "grid"
        M, N, K = c.M, c.N, c.K
        self._inputs(_gen("proj", c.id, family, seed))
        A64, W64 = self.A.to(F64), self.W.to(F64)
        self.acc = A64 @ W64.T                                       # [M, Nw] fp64; GRID: exact (asserted below)
        self.absacc = None if self.grid else A64.abs() @ W64.abs_().T          # (SPIKES' E; W64 is spent)
        self.out_rows = -(-M // c.P) * (c.P + 1) if c.epi == PATCH else M
        m = torch.arange(M)
        self.row_map = (m // c.P) * (c.P + 1) + 1 + m % c.P if c.epi == PATCH else m
        self.rows_buf, self.ldo = self.out_rows + (3 if c.ld else 0), N + (8 if c.ld else 0)
        self.lda, self.ldw = K + (8 if c.ld else 0), K + (24 if c.ld else 0)
        self.out_dtype = F32 if c.epi in F32_OUT else BF16
        self.inplace = (c.ld or c.inplace) and self.resid is not None
        if self.grid:
            self._assert_grid(W64)
        if c.epi == SILU:                                            # E_s is derived for an exponential far from the flush-to-zero range
            gate = self.acc[:, :N].abs() / (self.A[:, :1].to(F64).abs() if c.norm and c.entry == "gemv" else 1.0)
            assert float(gate.max()) <= (8.0 if self.grid or c.norm else 32.5)
        self._assert_normal()

    @property
    def label(self):
        """The family as printed: under the GEMV norm fold the second family is not SPIKES but a sparse integer W (_inputs_norm)."""
        return "grid-sparse" if self.case.norm and self.case.entry == "gemv" and not self.grid else self.family

    @property
    def scale_after(self):
        """Norm fold: the kernel scales the dot product of bf16(x w) by r afterwards (k_gemv_mfma, k_gemv_mfma8), where the others
        normalise every element to bf16(bf16(x r) w) first."""
        return self.case.kernel.startswith("k_gemv_mfma")

    # ---- inputs
    def _inputs(self, gen):
        c = self.case
        M, N, K, Nw = c.M, c.N, c.K, c.w_rows
        self.bias = self.resid = self.pos = self.norm_w = None
        if c.norm and c.entry == "gemv":
            return self._inputs_norm(gen)
        if self.grid:
            self.s = s = grid_shift(K, c.epi)
            a, w = _rand_int(gen, (M, K), 15), _rand_int(gen, (Nw, K), 31)
            a[(a == 0).all(-1), 0] = 1.0
            w[(w == 0).all(-1), 0] = 1.0
            self.A, self.W = to_bf16(a / 8), to_bf16(w * 2.0 ** s)
            small = lambda shape: to_bf16(_rand_int(gen, shape, 15) / 8)
            r32 = lambda shape: (_rand_int(gen, shape, 255) / 64).to(F32)
        else:
            hot = hot_k(c)
            assert len(hot) >= NNZ                                   # (so the NNZ positions of a row are distinct)
            at = torch.tensor(hot)[(c.hot_rot + NNZ * torch.arange(M)[:, None] + torch.arange(NNZ)[None]) % len(hot)]
            mant = (128 + torch.randint(0, 128, (M, NNZ), generator=gen)).to(F64) / 128
            e = torch.randint(-6, 7, (M, NNZ), generator=gen).to(F64)
            sign = torch.randint(0, 2, (M, NNZ), generator=gen).to(F64) * 2 - 1
            a = torch.zeros((M, K), dtype=F64)
            a[torch.arange(M)[:, None], at] = sign * mant * 2.0 ** e
            self.hot, self.hit = hot, min(NNZ * M, len(hot))
            w = torch.randn((Nw, K), generator=gen, dtype=F32) * 2.0 ** torch.randint(-3, 4, (Nw, 1), generator=gen).to(F32)
            self.A, self.W = to_bf16(a), to_bf16(w)
            top = {SILU: 32.0, QGELU: 1.0, GELU: 1.0}.get(c.epi)      # keep |gate| <= 32 and the GELUs' |acc| <= 1 (grid_shift): a row of W
            if top is not None:                                      # that exceeds it is scaled by a power of two
                g = (self.A.to(F64) @ self.W[:N].to(F64).T).abs().amax(0)
                self.W[:N] = to_bf16(self.W[:N].to(F64) * 2.0 ** -torch.ceil(torch.log2(g / top).clamp_min(0))[:, None])
            half = 0.5 if c.epi in (QGELU, GELU) else 1.0
            small = lambda shape: to_bf16(torch.randn(shape, generator=gen) * half)
            r32 = lambda shape: torch.randn(shape, generator=gen).to(F32)
        if c.has_bias:
            self.bias = small((N,))
        if c.epi == RESID_BF16:
            self.resid = small((M, N))
        elif c.epi == BIAS_RESID_F32:
            self.resid = r32((M, N))
        elif c.epi == PATCH:
            self.pos = small((c.P + 1, N))
        if c.norm:                                                   # p3v_gemm_resid_norm's weight
            nw = 1 + 0.1 * torch.randn((N,), generator=gen)
            nw[::7] *= -1
            self.norm_w = to_bf16(nw)

    def _inputs_norm(self, gen):
        """The GEMV norm fold (module docstring): rows +-c_m, norm weights 2^0 / 2^-1, W = j 2^s with |j| <= 3."""
        c = self.case
        M, K, Nw = c.M, c.K, c.w_rows
        self.s = s = math.floor(math.log2(1.3 / (2.2 * 0.8 * math.sqrt(K))))      # |normalised x| ~ 1, |j| std 2.0 (spikes: see below), weights 0.79 rms
        cm = to_bf16(0.5 + 3.0 * torch.rand((M, 1), generator=gen)).to(F64)
        if self.scale_after:                                         # there acc = (c r) t with c r = (1 + eps / c^2)^-1/2: a small c keeps it
            cm = cm * 2.0 ** -7                                      # percents away from 1, so that t's many rounding ties are none of acc
        sign = torch.randint(0, 2, (M, K), generator=gen).to(F64) * 2 - 1
        self.A = to_bf16(sign * cm)
        self.norm_w = to_bf16(2.0 ** -torch.randint(0, 2, (K,), generator=gen).to(F64))
        j = _rand_int(gen, (Nw, K), 3)
        if not self.grid:                                            # SPIKES has no meaning under a fold of whole rows: the second family
            j = j * (torch.rand((Nw, K), generator=gen) < 0.25)      # of these cases is a sparse W (three quarters zero) at twice the step
            self.s = s = s + 1
        j[(j == 0).all(-1), 0] = 1.0
        self.W = to_bf16(j * 2.0 ** s)
        if c.epi == RESID_BF16:
            self.resid = to_bf16(_rand_int(gen, (M, c.N), 15) / 8)

    # ---- the builder's assertions
    def _tie_share(self):
        b = self.acc[:, :self.case.N].to(F32).view(torch.int32)     # (exact: < 2^24 units) a tie: the 16 dropped bits are 0x8000
        return float(((b & 0xFFFF) == 0x8000).double().mean())

    def _assert_grid(self, W64):
        c = self.case
        if c.norm and c.entry == "gemv":
            assert 2 * 3 * c.K < 2 ** 16
            return
        u = 2.0 ** (self.s - 3)
        extra = (15 * 2.0 ** -3 + 255 * 2.0 ** -6 + 15 * 2.0 ** -3) / u           # bias, fp32 residual, bf16 residual / pos: in units
        assert 15 * 31 * c.K + extra < 2 ** 24, "partial sums leave the exact range of fp32"
        # against an int64 product: all of it up to 2^23 multiply-adds (an integer matmul is slow), else rows 0, M / 2, M - 1 and
        # so many evenly spaced columns that 2^23 are not exceeded
        rows = torch.arange(c.M) if c.M * c.w_rows * c.K <= 2 ** 23 else torch.tensor(sorted({0, c.M // 2, c.M - 1}))
        cols = torch.arange(0, c.w_rows, -(-len(rows) * c.w_rows * c.K // 2 ** 23))
        ai = (self.A.to(F64)[rows] * 8).to(torch.int64)
        wi = (W64[cols] * 2.0 ** -self.s).to(torch.int64)
        assert torch.equal((ai @ wi.T).to(F64) * u, self.acc[rows][:, cols]), "the fp64 reference is not exact"
        f = self.acc[:, :c.N].to(F32)
        assert torch.equal(f.to(F64), self.acc[:, :c.N])
        ties = self._tie_share()
        unrep = float((f.to(BF16).to(F64) != f.to(F64)).double().mean())
        assert ties >= 0.01 and unrep >= (0.5 if c.K >= 64 else 0.25), f"{c.id}: {ties:.3%} rounding ties, {unrep:.1%} sums that are no bf16 value"
        self.ties, self.unrep = ties, unrep

    def _assert_normal(self):
        tiny = 2.0 ** -126
        for t in (self.A, self.W, self.bias, self.resid, self.pos, self.acc):
            if t is not None:
                v = t.abs()                                          # (in its own type: a bf16 / fp32 subnormal is below 2^-126 too)
                assert not bool(((v > 0) & (v < tiny)).any()), "a subnormal operand or sum"

    # ---- the reference: brackets (bf16 outputs) or (ref, E) (fp32 outputs) under s x E
    def _acc_E(self, s):
        c = self.case
        if self.grid or s == 0:
            return torch.zeros_like(self.acc)
        E = self.absacc.clone()
        if self.bias is not None:
            E[:, :c.N] += self.bias.to(F64).abs()
        if self.resid is not None:
            E[:, :c.N] += self.resid.to(F64).abs()
        if self.pos is not None:
            E[:, :c.N] += self.pos.to(F64)[1 + torch.arange(c.M) % c.P].abs()
        return E * ((NNZ + 8) * 2.0 ** -23 * s)

    def _norm_acc(self, s):
        """GEMV norm fold: (acc_lo, acc_hi, kept rows) -- the exact accumulator at the two ends of v's bracket."""
        c = self.case
        x64 = self.A.to(F64)
        cm = x64[:, :1].abs()
        r = torch.rsqrt((x64 * x64).mean(-1, keepdim=True) + EPS)
        t = (x64.sign() * self.norm_w.to(F64)) @ self.W.to(F64).T                  # integer 2^(s - 1): exact
        if self.scale_after:
            v = cm * r
            return v * (1 - s * 2.0 ** -16) * t, v * (1 + s * 2.0 ** -16) * t, torch.ones(c.M, dtype=torch.bool)
        v_lo, v_hi = bracket(cm * r, cm * r * (s * 2.0 ** -16))
        a1, a2 = v_lo.to(F64) * t, v_hi.to(F64) * t
        return torch.minimum(a1, a2), torch.maximum(a1, a2), (v_lo.to(F64) == v_hi.to(F64)).flatten()

    def reference(self, s=1.0):
        """-> ("bf16", lo, hi) or ("f32", ref64, E); both over [M, N]."""
        c, N = self.case, self.case.N
        kept = None
        if c.norm and c.entry == "gemv":
            a_lo, a_hi, kept = self._norm_acc(s)
            if self.scale_after:
                mid, E = (a_lo + a_hi) / 2, (a_hi - a_lo).abs() / 2
            else:
                mid, E = None, None
        else:
            mid, E = self.acc, self._acc_E(s)
        def ends(cols):
            if mid is not None:
                return bracket(mid[:, cols], E[:, cols])
            return to_bf16(a_lo[:, cols]), to_bf16(a_hi[:, cols])                  # exact sums: one rounding each
        full = slice(0, N)
        if c.epi == SILU:
            g_ends, u_ends = ends(slice(0, N)), ends(slice(N, 2 * N))
            outs = []
            for g in g_ends:
                g64 = g.to(F64)
                sg = torch.sigmoid(g64)
                for sb in bracket(sg, s * (g64.abs() + 4) * 2.0 ** -22 * sg):
                    p = to_bf16(g.float() * sb.float())
                    outs += [to_bf16(p.float() * u.float()).float() for u in u_ends]
            st = torch.stack(outs)
            return "bf16", st.amin(0).to(BF16), st.amax(0).to(BF16), kept
        if c.epi == RESID_BF16:
            t_lo, t_hi = ends(full)
            r = self.resid.float()
            return "bf16", (r + t_lo.float()).to(BF16), (r + t_hi.float()).to(BF16), kept
        if mid is None:                                              # norm fold, NONE
            return ("bf16",) + ends(full) + (kept,)
        x = mid[:, full] + (self.bias.to(F64) if self.bias is not None else 0.0)
        Ex = E[:, full]
        if c.epi in (NONE, BIAS):
            return ("bf16",) + bracket(x, Ex) + (kept,)
        if c.epi == QGELU:
            t = C_QGELU * x
            ref = x * torch.sigmoid(t)
            Ef = x.abs() * (t.abs() + 4) * 2.0 ** -22 * torch.sigmoid(t) + 2.0 ** -23 * ref.abs()
            return ("bf16",) + bracket(ref, s * Ef + 1.2 * Ex) + (kept,)
        if c.epi == GELU:
            z = C_RSQRT2 * x
            ref = 0.5 * x * (1 + torch.erf(z))
            Ef = 0.5 * x.abs() * (2.0 ** -20 * torch.erf(z).abs() + 2.0 ** -24 * 1.13 * z.abs() * torch.exp(-z * z) + 2.0 ** -23) + 2.0 ** -23 * ref.abs()
            return ("bf16",) + bracket(ref, s * Ef + 1.2 * Ex) + (kept,)
        if c.epi == BIAS_RESID_F32:
            x = x + self.resid.to(F64)
        elif c.epi == PATCH:
            x = x + self.pos.to(F64)[1 + torch.arange(c.M) % c.P]
        return "f32", x, Ex, kept

    def uniqueness(self):
        """Share of the judged elements whose bracket is one value (fp32 outputs: 1), and the share of rows judged."""
        kind, a, b, kept = self.reference()
        rows = slice(None) if kept is None else kept
        return (1.0 if kind == "f32" else unique_share(a[rows], b[rows])), (1.0 if kept is None else float(kept.double().mean()))

    # ---- buffers
    def operand_buffers(self):
        """A and W inside their [rows, ld] buffers (padding PAD), flat."""
        c = self.case
        a = torch.full((c.M, self.lda), PAD, dtype=BF16)
        w = torch.full((c.w_rows, self.ldw), PAD, dtype=BF16)
        a[:, :c.K], w[:, :c.K] = self.A, self.W
        return a, w

    def out_buffer(self):
        """The flat output buffer before the call: sentinel everywhere, the residual in the window when it is updated in place."""
        flat = sentinel(2 * GUARD + self.rows_buf * self.ldo, self.out_dtype)
        if self.inplace:
            self.window(flat)[:] = self.resid
        return flat

    def resid_buffer(self):
        """The residual in a buffer of the output's geometry (a separate one: the cases that are not in place), or None."""
        if self.resid is None or self.inplace:
            return None
        flat = sentinel(2 * GUARD + self.rows_buf * self.ldo, self.out_dtype)
        self.window(flat)[:] = self.resid
        return flat

    def body(self, flat):
        return flat[GUARD:GUARD + self.rows_buf * self.ldo].view(self.rows_buf, self.ldo)

    def window(self, flat):
        """The [M, N] elements of the buffer the call writes (a view for plain rows, PATCH: use window_get / window_put)."""
        assert self.case.epi != PATCH
        return self.body(flat)[:self.case.M, :self.case.N]

    def window_get(self, flat):
        return self.body(flat)[self.row_map][:, :self.case.N]

    def window_put(self, flat, v, row_map=None):
        self.body(flat)[self.row_map if row_map is None else row_map, :self.case.N] = v.to(self.out_dtype)

    # ---- acceptance
    def verify(self, flat, s=1.0):
        """flat: the output buffer after the call -> '' or what is wrong (s: the rule under s x E)."""
        c, msgs = self.case, []
        got = self.window_get(flat)
        kind, a, b, kept = self.reference(s)
        rows = slice(None) if kept is None else kept
        if kind == "bf16":
            m = worst(got[rows], a[rows], b[rows])
        elif self.grid or s == 0:
            bad = got.to(F64) != a
            m = "" if not bool(bad.any()) else f"{int(bad.sum())} of {bad.numel()} fp32 outputs differ from the exact value, first at {tuple(bad.nonzero()[0].tolist())}"
        else:
            m = worst_abs(got, a, b)[0]
        if m:
            msgs.append(m)
        clean = self.out_buffer()
        mask = torch.ones(clean.numel(), dtype=torch.bool)
        self.body(mask)[self.row_map, :c.N] = False
        it = torch.int32 if self.out_dtype == F32 else torch.int16
        bad = mask & (flat.view(it) != clean.view(it))
        if bool(bad.any()):
            i = int(bad.nonzero()[0]) - GUARD
            msgs.append(f"{int(bad.sum())} elements outside [M, N] changed, first at row {i // self.ldo} column {i % self.ldo} of the [{self.rows_buf}, {self.ldo}] buffer")
        return "; ".join(msgs)

    def verify_normed(self, out, normed, s=1.0):
        """p3v_gemm_resid_norm's second output under the RMSNorm bracket of the `out` it stored."""
        x64, w64 = out.to(F64), self.norm_w.to(F64)
        n = x64 * torch.rsqrt((x64 * x64).mean(-1, keepdim=True) + EPS)
        n_lo, n_hi = bracket(n, n.abs() * (s * 2.0 ** -16))
        y1, y2 = to_bf16(n_lo.to(F64) * w64).float(), to_bf16(n_hi.to(F64) * w64).float()
        return worst(normed, torch.minimum(y1, y2).to(BF16), torch.maximum(y1, y2).to(BF16))

    # ---- the documented arithmetic in torch fp32, with defects
    def restate(self, order="seq", defect=None):
        """The flat output buffer as a kernel leaves it that sums in fp32 in `order` -- "seq": 8-wide chunks in order; "rev": from the
        end; "tiled": 64-wide tiles summed as two halves, the tiles of each of 4 K slices in order, then the slices in order -- and
        applies the epilogue as include/p3v.h states it (K > 1024: 32-wide chunks).  `defect`: see tests/test_proj_probe_cpu.py."""
        c, d = self.case, defect
        M, N, K = c.M, c.N, c.K
        if d == "lda_as_k":                                          # (the padded buffer read with the wrong stride)
            A = self.operand_buffers()[0].flatten()[:M * K].view(M, K).float()
        else:
            A = self.A.float()
        W = self.W.float()                                           # (copies: the defects below write into them)
        if c.norm and c.entry == "gemv":
            A, r_after = self._restate_norm(A)
        if d == "up_from_gate":
            W[N:] = W[:N]
        if d == "cut_mantissa":
            cut = lambda t: (t.to(BF16).view(torch.int16) & -8).view(BF16).float()
            A, W = cut(A), cut(W)
        if d == "drop_k0":
            A[:, 0] = 0
        if d == "drop_klast":
            A[:, K - 1] = 0
        tiles = [(k, min(k + 64, K)) for k in range(0, K, 64)]
        if d == "shift_slice" :
            e = (len(tiles) // 4 or 1) * 64
            A[:, min(e, K - 8):min(e, K - 8) + 8] = 0                 # slice 1 starts 8 elements late
        if d == "drop_tile":
            tiles.pop(len(tiles) // 2)
        if d == "tile_twice":
            tiles.insert(len(tiles) // 2, tiles[len(tiles) // 2])
        part = {"bf16_partials": BF16, "fp16_partials": torch.float16}.get(d)
        if order == "tiled" or part is not None:
            per = max(1, -(-len(tiles) // 4))
            acc = torch.zeros((M, W.shape[0]), dtype=F32)
            for s0 in range(0, len(tiles), per):
                sl = torch.zeros_like(acc)
                for k0, k1 in tiles[s0:s0 + per]:
                    h = (k0 + k1) // 2
                    sl += A[:, k0:h] @ W[:, k0:h].T + A[:, h:k1] @ W[:, h:k1].T
                acc += sl if part is None else sl.to(part).float()
        else:
            w = 8 if K <= 1024 else 32                               # (K = 3072 / 8192: a quarter of the steps, still not the tiled order)
            chunks = [(k, min(k + w, k1)) for k0, k1 in tiles for k in range(k0, k1, w)]
            acc = torch.zeros((M, W.shape[0]), dtype=F32)
            for k0, k1 in (chunks if order == "seq" else chunks[::-1]):
                acc += A[:, k0:k1] @ W[:, k0:k1].T
        if c.norm and c.entry == "gemv" and r_after is not None:
            acc = acc * r_after
        out = self._epilogue(acc, d)
        flat = self.out_buffer()
        self.window_put(flat, out, torch.arange(M) if d == "patch_not_remapped" else None)
        if d == "row_m_twice":                                       # (without spare rows it lands in the guard band)
            at = GUARD + (int(self.row_map[-1]) + 1) * self.ldo
            n = min(N, flat.numel() - at)
            flat[at:at + n] = out[-1, :n].to(self.out_dtype)
        return flat

    def _restate_norm(self, A):
        nw = self.norm_w.float()
        r = torch.rsqrt((A * A).sum(-1, keepdim=True) * (1.0 / self.case.K) + EPS)
        if self.scale_after:
            return (A * nw).to(BF16).float(), r
        return ((A * r).to(BF16).float() * nw).to(BF16).float(), None

    def _epilogue(self, acc, d):
        c, N = self.case, self.case.N
        if d == "trunc_store":
            rnd = lambda t: (t.float().view(torch.int32) & -65536).view(F32)
        elif d == "half_away":
            rnd = lambda t: ((t.float().view(torch.int32) + 0x8000) & -65536).view(F32)
        else:
            rnd = lambda t: t.to(BF16).float()
        bias = self.bias.float() if self.bias is not None else 0.0
        if c.epi == SILU:
            if d == "silu_no_inner":
                g, u = acc[:, :N], acc[:, N:]
                return rnd(g * torch.sigmoid(g) * u)
            g, u = rnd(acc[:, :N]), rnd(acc[:, N:])
            return rnd(rnd(g * rnd(torch.sigmoid(g))) * u)
        if c.epi == RESID_BF16:
            r = self.resid.float()
            return rnd(r + acc) if d == "resid_one_rounding" else rnd(r + rnd(acc))
        if d == "bias_after_rounding" and c.epi == BIAS:
            return rnd(rnd(acc) + bias)
        x = acc + bias
        if c.epi in (NONE, BIAS):
            return rnd(x)
        if c.epi == QGELU:
            return rnd(x * torch.sigmoid(torch.tensor(C_QGELU, dtype=F32) * x))
        if c.epi == GELU:
            return rnd(0.5 * x * (1 + torch.erf(x * torch.tensor(C_RSQRT2, dtype=F32))))
        if c.epi == BIAS_RESID_F32:
            return x + self.resid
        if c.epi == PATCH:
            return x + self.pos.float()[1 + torch.arange(c.M) % c.P]
        return x


MIN_UNIQUE, MIN_KEPT = 0.98, 0.75


@lru_cache(maxsize=2)
def probe(case, family):
    """The probe of a case.  The conditions on the reference -- the builder's assertions, lo == hi on >= 98 % of the elements, >= 3 of 4
    rows kept -- hold at seed 0 for every case of a few thousand elements; a case of fewer (8 outputs cannot hold "1 % ties" by
    the law of large numbers) takes the first seed at which they do.  Nothing here looks at a kernel's output."""
    for seed in range(64 if case.M * case.N < 4096 else 1):
        try:
            pr = Probe(case, family, seed)
        except AssertionError:
            if seed == 63 or case.M * case.N >= 4096:
                raise
            continue
        u, k = pr.uniqueness()
        if (u >= MIN_UNIQUE and k >= MIN_KEPT) or case.M * case.N >= 4096:
            break
    return pr
