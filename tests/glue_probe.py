"""Probing inputs, fp64 references and acceptance rules for the small kernels between the projections and at the end of a step:
p3v_rmsnorm, p3v_layernorm, p3v_rope_table, p3v_rope_kv_append, p3v_argmax / p3v_topk / p3v_log_softmax, p3v_clip_cls_rows
(csrc/p3v_elementwise.hip, csrc/p3v_argmax.h).  Everything here is torch / numpy on the CPU; tests/test_glue_probe_cpu.py shows
on the references alone that the inputs expose each defect, tests/test_glue_kernels_gpu.py runs the kernels.

ONE ACCEPTANCE RULE FOR EVERY bf16 OUTPUT: THE ROUNDING BRACKET.  Rounding to bf16 is monotonic, so a kernel whose fp32 value
is within E of the fp64 value v stores a bf16 inside [bf16(v - E), bf16(v + E)].  `bracket(v, E)` gives the two ends (the
fp64 -> fp32 step rounds outwards, so the double rounding of the ends can only widen it), `inside(got, lo, hi)` compares as
floats (-0 == +0).  A test asserts `inside` for EVERY element: no shares, no atol.  On >= 98 % of the elements of every case
lo == hi (asserted on the CPU), so the rule reads "bit-exact, except where the reference itself sits on a rounding tie".
E comes from the arithmetic of each kernel and never from what a kernel produced:

  * RMSNorm, y = bf16(bf16(x r) w) (include/p3v.h).  r64 from fp64 statistics; the kernel's r is within relative 2^-16 of it:
    at most 128 sequential fp32 adds per lane at hidden 8192 plus the wave tree is 2^-16.9 on the sum of squares at worst, the
    square root halves that, rsqrtf and the two scalar operations add ~2^-22; rounded up to 2^-16.  A product of two bf16
    values is exact in fp32, so the second rounding adds no term: the bracket is
    [bf16(bf16(x r64 (1 - 2^-16)) w), bf16(bf16(x r64 (1 + 2^-16)) w)], the ends ordered as floats (a negative w swaps them).
  * LayerNorm, reference fp64.  E = 2^-20 r |w_j| (mean_row |x| + |x_j - mu|) + 2^-22 |ref_j|: the first term is the error of the
    fp32 mean (relative to the row's mean |x|) and of the fp32 variance (relative, through r, to |x_j - mu|), the second the
    roundings of the output expression.  fp32 output: |got - ref| <= E; bf16 output: bracket(ref, E).
  * RoPE table.  The header defines the table on the fp32 product float32(pos) * float32(inv_freq): the reference is fp64 cos / sin
    of THAT product, times the fp32 scale.  |got - ref| <= 2^-21 scale: the device library documents cosf / sinf at 2 ulp, the
    scale multiply adds half an ulp, <= 3 ulp at magnitudes below 2; 8 ulp carries the margin.
  * Split + rotation + append.  fp64 a cos - b sin and b cos + a sin on the bf16 inputs and the fp32 tables the kernel was given,
    queries times float32(q_scale) before the one rounding.  E = 2^-21 (|a cos| + |b sin|) q_scale: four fp32 roundings (two
    products, the sum, the scale) with a 2x margin.  V is a copy: bit-exact.  Destinations start as a position-dependent
    sentinel inside guard bands; everything outside the written window must come back bit-identical.
  * log-softmax, y = bf16(x - bf16(lse)).  lse64 in fp64, E = 2^-16 + 2^-22 |lse| (2-ulp expf, the fp32 sums, logf).  bf16 - bf16
    is exact in fp32 at these magnitudes: the bracket is [bf16(x - bf16(lse + E)), bf16(x - bf16(lse - E))].
  * arg-max / top-k: exact indices of a stable sort by (-value, index), -0 == +0; a row with a NaN reports arg-max -1.
  * CLS rows: row 0 of every image is float(cls) + float(pos[0]) exactly, every other element untouched.
"""
import math
import zlib
from dataclasses import dataclass
from functools import lru_cache

import numpy as np
import torch

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
EPS = 1e-5
Q_PRESCALE = 1.4426950408889634          # ops.Q_PRESCALE (log2 e)
GUARD = 64                               # sentinel elements in front of and behind every destination buffer


# ---------------------------------------------------------------- the rounding bracket
def f32_down(v):
    """fp64 -> the largest fp32 <= v."""
    f = v.to(F32)
    return torch.where(f.to(F64) > v, torch.nextafter(f, torch.full_like(f, -math.inf)), f)


def f32_up(v):
    """fp64 -> the smallest fp32 >= v."""
    f = v.to(F32)
    return torch.where(f.to(F64) < v, torch.nextafter(f, torch.full_like(f, math.inf)), f)


def bracket(v64, E):
    """The bf16 values a kernel may store when its fp32 value is within E of v64: (lo, hi), both bf16."""
    v64 = v64.to(F64)
    return f32_down(v64 - E).to(BF16), f32_up(v64 + E).to(BF16)


def inside(got, lo, hi):
    """Elementwise lo <= got <= hi, compared as floats (-0 == +0; a NaN is outside)."""
    g = got.to(F64)
    return (lo.to(F64) <= g) & (g <= hi.to(F64))


def unique_share(lo, hi):
    """Share of the elements whose bracket is one value."""
    return float((lo.to(F64) == hi.to(F64)).double().mean())


def worst(got, lo, hi):
    """'' when every element is inside, else the element furthest outside: its index, got, lo, hi."""
    ok = inside(got, lo, hi)
    if bool(ok.all()):
        return ""
    g, l, h = got.to(F64), lo.to(F64), hi.to(F64)
    out = torch.where(ok, torch.zeros_like(g), torch.maximum(l - g, g - h))
    out = torch.where(torch.isnan(out), torch.full_like(out, math.inf), out)
    i = int(out.argmax())
    idx = tuple(int(v) for v in np.unravel_index(i, tuple(g.shape)))
    return (f"{int((~ok).sum())} of {ok.numel()} outside; worst at {idx}: got {float(g.flatten()[i])!r}, "
            f"lo {float(l.flatten()[i])!r}, hi {float(h.flatten()[i])!r}")


def worst_abs(got, ref, E):
    """The same for an fp32 output under |got - ref| <= E; also the largest |got - ref| / E."""
    g, r = got.to(F64), ref.to(F64)
    err = (g - r).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / E)
    i = int(ratio.argmax())
    idx = tuple(int(v) for v in np.unravel_index(i, tuple(g.shape)))
    top = float(ratio.flatten()[i])
    msg = "" if top <= 1.0 else (f"{int((ratio > 1).sum())} of {ratio.numel()} outside; worst at {idx}: got {float(g.flatten()[i])!r}, "
                                 f"ref {float(r.flatten()[i])!r}, E {float(torch.as_tensor(E).expand_as(g).flatten()[i])!r}")
    return msg, top


SCALES = (0.0, 1 / 64, 1 / 16, 1 / 4, 1.0)


def needed_scale(verify):
    """The smallest s of SCALES at which verify(s) -- the rule under s x E -- accepts (for the record: how much of E a kernel uses;
    0: bit-exact against the rounded fp64 reference).  None when it fails at 1."""
    return next((s for s in SCALES if verify(s) == ""), None)


def to_bf16(x):
    return x.to(F32).to(BF16)


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def hot_positions(chunks):
    """The chunk positions a hot-chunk row is built for: 0, 63, 64, chunks - 1, chunks - 2 and the first and last chunk of every
    64-chunk pass, in that order of priority."""
    pos = [0, chunks - 1, chunks - 2, 63, 64]
    for p in range(0, chunks, 64):
        pos += [p, min(p + 63, chunks - 1)]
    seen = []
    for p in pos:
        if 0 <= p < chunks and p not in seen:
            seen.append(p)
    return seen


# ---------------------------------------------------------------- RMSNorm
RMS_HIDDEN = (8, 520, 3064, 3072, 3080, 8192)        # 1 / 65 / 383 / 384 chunks: the register kernel; 385 / 1024: the fallback
RMS_ROWS = (1, 6, 33)                                # rows % 4 != 0; 33 rows hold every hot position (33 of them at 8192)


@dataclass(frozen=True)
class RmsCase:
    hidden: int
    rows: int

    @property
    def id(self):
        return f"rms-h{self.hidden}-r{self.rows}"


RMS_CASES = tuple(RmsCase(h, r) for h in RMS_HIDDEN for r in RMS_ROWS)


class RmsProbe:
    """Gaussian rows (std 3) and HOT-CHUNK rows: background std 0.05, one 8-wide chunk 8.0 (low half) / 16.0 (high half), so the
    chunk carries almost the whole sum of squares and a swapped pair shows.  Weights 1 + 0.1 N(0, 1), every 7th negated."""

    def __init__(self, case, seed=0):
        self.case = case
        H, R = case.hidden, case.rows
        gen = _gen("rms", H, R) if seed == 0 else _gen("rms", H, R, seed)        # (seed > 0: other draws, for tests/quant_probe.py)
        hot = hot_positions(H // 8)
        hot = hot[:{1: 0, 6: 3, 33: 33}[R]]
        x = torch.randn((R, H), generator=gen) * 3.0
        self.hot = []                                            # (row, chunk)
        for i, p in enumerate(hot):
            row = R - len(hot) + i
            x[row] = torch.randn((H,), generator=gen) * 0.05
            x[row, 8 * p:8 * p + 4], x[row, 8 * p + 4:8 * p + 8] = 8.0, 16.0
            self.hot.append((row, p))
        w = 1 + 0.1 * torch.randn((H,), generator=gen)
        w[::7] *= -1
        self.x, self.w = to_bf16(x), to_bf16(w)
        x64, w64 = self.x.to(F64), self.w.to(F64)
        self.n = x64 * torch.rsqrt((x64 * x64).mean(-1, keepdim=True) + EPS)
        self.lo, self.hi = self.bracket_at(1.0)

    def bracket_at(self, s):
        """The bracket with s x 2^-16 on r."""
        n_lo, n_hi = bracket(self.n, self.n.abs() * (s * 2.0 ** -16))
        w64 = self.w.to(F64)
        y1, y2 = to_bf16(n_lo.to(F64) * w64).float(), to_bf16(n_hi.to(F64) * w64).float()      # bf16 x bf16: exact in fp32
        return torch.minimum(y1, y2).to(BF16), torch.maximum(y1, y2).to(BF16)

    def restate(self, drop=None, shift_w=False, skip_round=False):
        """The documented arithmetic in torch fp32.  Defects: chunk `drop` left out of the sum of squares, the weights shifted by
        one chunk, the first rounding skipped."""
        x, w, H = self.x.float(), self.w.float(), self.case.hidden
        sq = x * x
        if drop is not None:
            sq[:, 8 * drop:8 * drop + 8] = 0
        r = torch.rsqrt(sq.sum(-1, keepdim=True) * (1.0 / H) + EPS)
        if shift_w:
            w = torch.roll(w, 8)
        if skip_round:
            return (x * r * w).to(BF16)
        return ((x * r).to(BF16).float() * w).to(BF16)

    def verify(self, got, s=1.0):
        return worst(got, *self.bracket_at(s))


# ---------------------------------------------------------------- LayerNorm
LN_HIDDEN = (4, 1020, 1024, 1028, 4096)              # 1 / 255 / 256 chunks: the register kernels; 257 / 1024: the fallback
LN_ROWS = 101                                        # one LARGE-MEAN row in 101: its bf16 brackets are wide (E ~ 1e-3), see LnProbe


@dataclass(frozen=True)
class LnCase:
    hidden: int
    out_f32: bool

    @property
    def id(self):
        return f"ln-h{self.hidden}-{'f32' if self.out_f32 else 'bf16'}"


LN_CASES = tuple(LnCase(h, f) for h in LN_HIDDEN for f in (False, True))


class LnProbe:
    """fp32 rows: row 0 LARGE-MEAN (1000 + N(0, 1): the mean's fp32 error is 1e-4 of the spread, and a one-pass variance loses
    it whole), row 1 OUTLIER (Gaussian, every (hidden // 3)-th channel 80; at hidden 4 every 2nd, where every channel would make
    the row constant), then one HOT-CHUNK row per position of hot_positions over 4-wide chunks (background std 0.05, the chunk
    8, 8, 16, 16), then Gaussian rows 2 N + 0.5.  The inputs are shared by the two output types.
    The bf16 bracket of the LARGE-MEAN row is wide -- E there is 2^-20 x 1000, a quarter of a bf16 ulp at 1 -- so its share of a case
    is kept at one row in 101 (the fp32 output holds that row to E itself)."""

    def __init__(self, hidden):
        self.hidden = H = hidden
        gen = _gen("ln", H)
        x = torch.randn((LN_ROWS, H), generator=gen) * 2.0 + 0.5
        x[0] = 1000.0 + torch.randn((H,), generator=gen)
        x[1, ::max(2, H // 3)] = 80.0
        self.hot = []
        for i, p in enumerate(hot_positions(H // 4)):
            row = 2 + i
            x[row] = torch.randn((H,), generator=gen) * 0.05
            x[row, 4 * p:4 * p + 2], x[row, 4 * p + 2:4 * p + 4] = 8.0, 16.0
            self.hot.append((row, p))
        assert 2 + len(self.hot) < LN_ROWS
        self.x = x.to(F32)
        self.w = to_bf16(1 + 0.1 * torch.randn((H,), generator=gen))
        self.b = to_bf16(0.1 * torch.randn((H,), generator=gen))
        x64, w64, b64 = self.x.to(F64), self.w.to(F64), self.b.to(F64)
        mu = x64.mean(-1, keepdim=True)
        d = x64 - mu
        r = torch.rsqrt((d * d).mean(-1, keepdim=True) + EPS)
        self.ref = d * r * w64 + b64
        self.E = 2.0 ** -20 * r * w64.abs() * (x64.abs().mean(-1, keepdim=True) + d.abs()) + 2.0 ** -22 * self.ref.abs()
        self.lo, self.hi = bracket(self.ref, self.E)

    def restate(self, drop_mean=None, drop_var=None, one_pass=False):
        """Two-pass fp32 LayerNorm.  Defects: a chunk left out of the mean, out of the variance, a one-pass fp32 variance."""
        x, H = self.x, self.hidden
        s = x.clone()
        if drop_mean is not None:
            s[:, 4 * drop_mean:4 * drop_mean + 4] = 0
        mu = s.sum(-1, keepdim=True) * (1.0 / H)
        d = x - mu
        if one_pass:
            var = (x * x).sum(-1, keepdim=True) * (1.0 / H) - mu * mu
        else:
            q = d * d
            if drop_var is not None:
                q[:, 4 * drop_var:4 * drop_var + 4] = 0
            var = q.sum(-1, keepdim=True) * (1.0 / H)
        return d * torch.rsqrt(var + EPS) * self.w.float() + self.b.float()           # fp32; the bf16 output rounds it

    def verify(self, got, out_f32):
        """-> (message, largest |got - ref| / E for the fp32 output; for bf16 the needed_scale)."""
        if out_f32:
            return worst_abs(got, self.ref, self.E)
        return worst(got, self.lo, self.hi), needed_scale(lambda s: worst(got, *bracket(self.ref, self.E * s)))


@lru_cache(maxsize=None)
def ln_probe(hidden):
    return LnProbe(hidden)


# ---------------------------------------------------------------- RoPE table
ROPE_HALF = (16, 32, 48)
ROPE_GROUPS = ("dense", "edges", "seeded", "leftpad", "extended")


@dataclass(frozen=True)
class TableCase:
    half: int
    factors: str                 # "short" | "long"
    group: str

    @property
    def id(self):
        return f"table-half{self.half}-{self.factors}-{self.group}"


TABLE_CASES = tuple(TableCase(h, f, g) for h in ROPE_HALF for f in ("short", "long") for g in ROPE_GROUPS)


def table_positions(group):
    """fp32 positions of a group.  dense: 0..255 (n_pos * half a multiple of 256: full blocks); edges: every 4096 k +- 1 up to
    131071 (63 positions: never a multiple of 256); seeded: 32 positions in [4096, 131072); leftpad: a left-padded row as
    prefill_slot builds it; extended: explicit position ids continued as _new_state does."""
    if group == "dense":
        return torch.arange(256, dtype=F32)
    if group == "edges":
        p = [4096 * k + s for k in range(1, 33) for s in (-1, 1)]
        return torch.tensor([v for v in p if v <= 131071], dtype=F32)
    if group == "seeded":
        return torch.randint(4096, 131072, (32,), generator=_gen("table", "seeded")).to(F32)
    if group == "leftpad":
        return (torch.arange(520, dtype=F32) - float(200)).clamp_min(0)
    p = torch.cat([torch.ones(3), torch.arange(9.0)]).to(F32)
    return torch.cat([p, p[-1:] + 1 + torch.arange(40 - p.numel(), dtype=F32)])


def su_inv_freq(cfg, half, factors):
    """model._inv_freq for head dim 2 * half, on the first `half` factors."""
    f = torch.tensor(cfg.rope_scaling[factors + "_factor"][:half], dtype=F32)
    return 1.0 / (f * (torch.tensor(float(cfg.rope_theta), dtype=F32) ** (torch.arange(0, 2 * half, 2, dtype=F32) / (2 * half))))


class TableProbe:
    def __init__(self, case):
        from phi_3_vision_mlx_amd.config import make_config, rope_scaling_factor
        self.case, self.cfg = case, make_config()
        self.pos = table_positions(case.group)
        self.inv = su_inv_freq(self.cfg, case.half, case.factors)
        self.scale = float(np.float32(rope_scaling_factor(self.cfg)))                 # what the C ABI receives
        e = (self.pos[:, None] * self.inv[None, :]).to(F64)                          # the fp32 product, exactly
        self.cos, self.sin = torch.cos(e) * self.scale, torch.sin(e) * self.scale
        self.E = 2.0 ** -21 * self.scale

    def restate(self, wrong_factors=False, pos_shift=0, reduce_f32=False):
        """fp32 cos / sin of the fp32 product.  Defects: the other factor set, position + 1, an fp32 range reduction."""
        inv = self.inv
        if wrong_factors:
            inv = su_inv_freq(self.cfg, self.case.half, "short" if self.case.factors == "long" else "long")
        e = (self.pos + pos_shift)[:, None] * inv[None, :]
        if reduce_f32:
            two_pi = torch.tensor(2 * math.pi, dtype=F32)
            e = e - two_pi * torch.round(e / two_pi)
        s = torch.tensor(self.scale, dtype=F32)
        return torch.cos(e) * s, torch.sin(e) * s

    def verify(self, cos, sin):
        (m1, r1), (m2, r2) = worst_abs(cos, self.cos, self.E), worst_abs(sin, self.sin, self.E)
        return "; ".join(f"{n}: {m}" for n, m in (("cos", m1), ("sin", m2)) if m), max(r1, r2)


# ---------------------------------------------------------------- split + rotation + append
@dataclass(frozen=True)
class RopeCase:
    L: int
    past: int
    hd: int = 96
    nh: int = 4
    nkv: int = 4
    B: int = 1
    dev_past: bool = False       # d_past holds `past`, the host argument is 0
    tab_div: int = 1
    off_is_past: bool = True     # False: rows go to [0, L) of a scratch with dst_t = 8 ceil(L / 8)
    prescale: bool = False       # q_scale = hd^-0.5 * Q_PRESCALE
    null: bool = False           # null tables: a plain head split
    base: int = 0                # position of table row 0 (table g holds base + 1000 g + t)

    @property
    def q_scale(self):
        return float(np.float32(self.hd ** -0.5 * Q_PRESCALE)) if self.prescale else 1.0

    @property
    def dst_t(self):
        return 8 * -(-self.L // 8) if not self.off_is_past else 8 * -(-(self.past + self.L) // 8) + 8

    @property
    def dpos0(self):
        return self.past if self.off_is_past else 0

    @property
    def tab_t(self):
        return self.past + self.L + 1

    @property
    def id(self):
        s = f"rope-L{self.L}-past{self.past}-hd{self.hd}-h{self.nh}x{self.nkv}-B{self.B}-base{self.base}"
        s += "-dpast" if self.dev_past else ""
        s += f"-div{self.tab_div}" if self.tab_div > 1 else ""
        s += "" if self.off_is_past else "-scratch"
        s += "-qs" if self.prescale else ""
        return s + ("-null" if self.null else "")


ROPE_L = (1, 31, 32, 63, 64, 65, 130)                # 32: the switch to the one-launch V transpose; 63 / 64 / 65: its 64-token tile
ROPE_PAST = (0, 8, 13)
ROPE_HD = (96, 64, 32)
ROPE_HEADS = ((4, 4), (8, 2), (3, 1))


def _rope_cases():
    cases = []
    for i, L in enumerate(ROPE_L):
        for j, past in enumerate(ROPE_PAST):
            n = 3 * i + j
            nh, nkv = ROPE_HEADS[(2 * i + j) % 3]
            cases.append(RopeCase(L, past, ROPE_HD[(i + j) % 3], nh, nkv, B=(1, 3)[n % 2], prescale=(n // 2) % 2 == 1,
                                  base=(0, 4090, 100000)[n % 3]))
    for L, past, kw in ((1, 13, {}), (32, 8, {"hd": 64}), (65, 13, {"nh": 8, "nkv": 2, "prescale": True}), (130, 13, {"B": 3, "hd": 32})):
        cases.append(RopeCase(L, past, dev_past=True, base=4090, **kw))
    for L, past, kw in ((1, 13, {}), (31, 0, {"hd": 32, "prescale": True}), (64, 8, {"nh": 3, "nkv": 1}), (32, 13, {"hd": 64, "nh": 8, "nkv": 2})):
        cases.append(RopeCase(L, past, B=6, tab_div=3, base=4000, **kw))
    for L, past, kw in ((1, 13, {}), (31, 8, {"hd": 64, "B": 3}), (63, 13, {"nh": 8, "nkv": 2, "prescale": True}), (130, 0, {"hd": 32}),
                        (64, 13, {"dev_past": True, "nh": 3, "nkv": 1, "B": 3})):
        cases.append(RopeCase(L, past, off_is_past=False, base=100000, **kw))
    for L, past, kw in ((1, 13, {}), (32, 8, {"hd": 64, "nh": 8, "nkv": 2, "B": 3}), (65, 13, {"hd": 32, "nh": 3, "nkv": 1})):
        cases.append(RopeCase(L, past, null=True, **kw))
    return tuple(cases)


ROPE_CASES = _rope_cases()
assert len({c.id for c in ROPE_CASES}) == len(ROPE_CASES)


def sentinel(n):
    """bf16 of (index % 251) + 300: no two neighbours alike, nothing a kernel would write."""
    return to_bf16((torch.arange(n) % 251 + 300).float())


class RopeProbe:
    """qkv Gaussian bf16; rotation tables fp64 cos / sin (plain RoPE, base 10000) rounded to fp32, so nothing here depends on
    p3v_rope_table; one spare table row behind the window (for the position + 1 defect)."""

    def __init__(self, case):
        self.case = c = case
        gen = _gen("rope", c.id)
        self.heads = c.nh + 2 * c.nkv
        self.qkv = to_bf16(torch.randn((c.B * c.L, self.heads * c.hd), generator=gen))
        self.cos = self.sin = None
        if not c.null:
            G = c.B // c.tab_div
            pos = (c.base + 1000 * torch.arange(G, dtype=F64))[:, None] + torch.arange(c.tab_t, dtype=F64)[None]
            ang = pos[..., None] * (10000.0 ** (-torch.arange(0, c.hd, 2, dtype=F64) / c.hd))
            self.cos, self.sin = torch.cos(ang).to(F32), torch.sin(ang).to(F32)       # [G, tab_t, hd / 2]
        self.shapes = {"q": (c.B, c.nh, c.L, c.hd), "k": (c.B, c.nkv, c.dst_t, c.hd), "v": (c.B, c.nkv, c.hd, c.dst_t)}
        self.ref, self.E = self.rotate(F64)
        (self.q_lo, self.q_hi), (self.k_lo, self.k_hi) = self.brackets_at(1.0)
        self.v = self.qkv.view(c.B, c.L, self.heads, c.hd)[:, :, c.nh + c.nkv:].permute(0, 2, 3, 1)      # [B, nkv, hd, L]

    def rotate(self, dtype, sin_sign=1, partner_next=False, pos_shift=0, row_b=False, scale_after=False, scale_keys=False):
        """Rotated q and k heads [B, nh + nkv, L, hd] in `dtype`, and the bound E (fp64 only).  In fp32 every product, the sum and
        the scale round separately, as p3v_rope_pair pins them; the result is rounded to bf16.  Defects: see
        tests/test_glue_probe_cpu.py."""
        c, half = self.case, self.case.hd // 2
        x = self.qkv.view(c.B, c.L, self.heads, c.hd)[:, :, :c.nh + c.nkv].transpose(1, 2).to(dtype)      # [B, heads, L, hd]
        qs = torch.ones(c.nh + c.nkv, dtype=dtype)
        qs[:c.nh if not scale_keys else None] = c.q_scale
        qs = qs[None, :, None, None]
        if c.null:
            return (x, torch.zeros_like(x)) if dtype == F64 else x.to(BF16)
        rows = torch.arange(c.B).clamp_max(self.cos.shape[0] - 1) if row_b else torch.arange(c.B) // c.tab_div
        t = c.past + torch.arange(c.L) + pos_shift
        cs = self.cos[rows][:, t].to(dtype)[:, None]                                  # [B, 1, L, half]
        sn = sin_sign * self.sin[rows][:, t].to(dtype)[:, None]
        a, b = x[..., :half], x[..., half:]
        b1, a2 = (x[..., 1:half + 1], torch.roll(x, -1, -1)[..., half:]) if partner_next else (b, a)
        out = torch.cat([a * cs - b1 * sn, b * cs + a2 * sn], dim=-1)
        if dtype == F64:
            E = 2.0 ** -21 * torch.cat([(a * cs).abs() + (b * sn).abs(), (b * cs).abs() + (a * sn).abs()], dim=-1) * qs
            return out * qs, E
        if scale_after:
            return (out.to(BF16).float() * qs).to(BF16)
        return (out * qs).to(BF16)

    def brackets_at(self, s):
        nh = self.case.nh
        return bracket(self.ref[:, :nh], self.E[:, :nh] * s), bracket(self.ref[:, nh:], self.E[:, nh:] * s)

    def buffers(self):
        """Sentinel-filled flat buffers with guard bands: name -> (flat bf16 buffer, the destination's view into it)."""
        res = {}
        for name, shape in self.shapes.items():
            n = math.prod(shape)
            flat = sentinel(n + 2 * GUARD)
            res[name] = (flat, flat[GUARD:GUARD + n].view(shape))
        return res

    def emulate(self, **defect):
        """The buffers as a kernel with the restated arithmetic (and `defect`) leaves them."""
        c, bufs = self.case, self.buffers()
        o = self.rotate(F32, **defect)
        w = slice(c.dpos0, c.dpos0 + c.L)
        bufs["q"][1].copy_(o[:, :c.nh])
        bufs["k"][1][:, :, w] = o[:, c.nh:]
        bufs["v"][1][:, :, :, w] = self.v
        return {k: f for k, (f, _) in bufs.items()}

    def verify(self, flat, s=1.0):
        """flat: name -> the flat buffer after the call.  -> '' or what is wrong (s: the brackets under s x E)."""
        c, msgs = self.case, []
        q_br, k_br = self.brackets_at(s)
        w = slice(c.dpos0, c.dpos0 + c.L)
        for name, shape in self.shapes.items():
            n = math.prod(shape)
            got = flat[name][GUARD:GUARD + n].view(shape)
            clean = sentinel(n + 2 * GUARD)
            mask = torch.ones(n + 2 * GUARD, dtype=torch.bool)
            body = mask[GUARD:GUARD + n].view(shape)
            if name == "q":
                body[:] = False
                m = worst(got, *q_br)
            elif name == "k":
                body[:, :, w] = False
                m = worst(got[:, :, w], *k_br)
            else:
                body[:, :, :, w] = False
                m = "" if torch.equal(got[:, :, :, w].view(torch.int16), self.v.contiguous().view(torch.int16)) else "V is not a bit-exact copy"
            if m:
                msgs.append(f"{name}: {m}")
            bad = mask & (flat[name].view(torch.int16) != clean.view(torch.int16))
            if bool(bad.any()):
                msgs.append(f"{name}: {int(bad.sum())} elements outside the window changed, first at flat index {int(bad.nonzero()[0]) - GUARD}")
        return "; ".join(msgs)


# ---------------------------------------------------------------- vocabulary tail: arg-max, top-k, log-softmax
VOCAB_N = (1, 7, 8, 9, 1023, 1024, 1025, 8200, 32064)
VOCAB_ROWS = 9                       # n = 1025: rows 0 and 8 are 16-byte aligned, the others are not
PEAK = 20.0
# the planted rows of the three 9-row matrices of every n (a kind that does not fit n falls back to "mid": the maximum at n // 2)
VOCAB_VARIANTS = {
    "a": ("max0", "maxlast", "maxvec", "maxtail", "tie_vec_tail", "tie1024", "neginf", "equal", "posinf"),
    "b": ("eight_head", "tie1024", "posinf", "maxtail", "neginf", "eight_tail", "maxlast", "tie_vec_tail", "maxvec"),
    "nan": ("nan_tail", "mid", "eight_spread", "nan_mid", "maxlast", "tie_vec_tail", "nan_tail", "eight_tail", "max0"),
}


@dataclass(frozen=True)
class VocabCase:
    n: int
    variant: str

    @property
    def id(self):
        return f"vocab-n{self.n}-{self.variant}"


VOCAB_CASES = tuple(VocabCase(n, v) for n in VOCAB_N for v in VOCAB_VARIANTS)


def topk_ks(n):
    return sorted({k for k in (1, 3, 8) if k <= n} | ({n} if n <= 8 else set()))


class VocabProbe:
    """Rows of bf16 logits (background N(0, 2)) with the maximum PEAK planted where the vector body, the scalar tail and the
    unaligned path of row_argmax_partial meet: index 0, n - 1, 8 (n // 8) - 1 (last vector element), 8 (n // 8) (first tail
    element), a tie across that boundary, a tie 1024 apart (the same thread's next element in the scalar path), all -inf, all
    equal, one +inf, eight equal maxima, and a NaN (arg-max -1; top-k is not asserted on those rows)."""

    def __init__(self, case):
        self.case = case
        n, v8 = case.n, 8 * (case.n // 8)
        gen = _gen("vocab", n, case.variant)
        x = to_bf16(torch.randn((VOCAB_ROWS, n), generator=gen) * 2.0)
        self.kinds = []
        for r, kind in enumerate(VOCAB_VARIANTS[case.variant]):
            at = {"max0": [0], "maxlast": [n - 1], "maxvec": [v8 - 1], "maxtail": [v8], "tie_vec_tail": [v8 - 1, v8],
                  "tie1024": [min(5, n - 1025), min(5, n - 1025) + 1024], "eight_head": list(range(8)),
                  "eight_tail": list(range(n - 8, n)), "eight_spread": [(i * (n - 1)) // 7 for i in range(8)]}.get(kind)
            if at is not None and (min(at) < 0 or max(at) >= n or len(set(at)) != len(at)):
                kind, at = "mid", None
            if kind == "mid":
                at = [n // 2]
            if at is not None:
                x[r, at] = PEAK
            elif kind == "neginf":
                x[r] = -math.inf
            elif kind == "equal":
                x[r] = 1.5
            elif kind == "posinf":
                x[r, (2 * n) // 3] = math.inf
            elif kind == "nan_tail":
                x[r, n - 1] = math.nan
            elif kind == "nan_mid":
                x[r, n // 2] = math.nan
            self.kinds.append(kind)
        self.x = x
        self.has_nan = torch.isnan(x.float()).any(-1)
        self.order = np.argsort(-x.to(F64).numpy(), axis=-1, kind="stable")          # by (-value, index); -0 == +0
        self.argmax = torch.where(self.has_nan, torch.tensor(-1), torch.from_numpy(self.order[:, 0].copy())).to(torch.int32)

    def topk(self, k):
        return torch.from_numpy(self.order[:, :k].copy()).to(torch.int32)

    def restate_argmax(self, last_wins=False, no_tail=False):
        x = self.x.float().numpy()
        x = x[:, :8 * (self.case.n // 8)] if no_tail else x
        if x.shape[1] == 0:
            return torch.zeros(VOCAB_ROWS, dtype=torch.int32)
        i = x.shape[1] - 1 - np.argmax(x[:, ::-1], axis=-1) if last_wins else np.argmax(x, axis=-1)
        return torch.where(self.has_nan, torch.tensor(-1), torch.from_numpy(i)).to(torch.int32)

    def restate_topk(self, k, last_wins=False, no_tail=False):
        """k rounds of arg-max over what is not picked yet, as k_topk runs them."""
        x = self.x.to(F64).numpy().copy()
        x = x[:, :8 * (self.case.n // 8)] if no_tail else x
        out = np.zeros((VOCAB_ROWS, k), dtype=np.int32)
        if x.shape[1] < k:
            return torch.from_numpy(out)
        live = np.ones(x.shape, dtype=bool)
        for j in range(k):
            v = np.where(live, x, -np.inf)
            cand = live & (v == v.max(-1, keepdims=True))    # an all -inf remainder: every index not picked yet
            i = x.shape[1] - 1 - np.argmax(cand[:, ::-1], axis=-1) if last_wins else np.argmax(cand, axis=-1)
            out[:, j] = i
            live[np.arange(VOCAB_ROWS), i] = False
        return torch.from_numpy(out)

    def verify_argmax(self, got):
        bad = (got.cpu().to(torch.int32) != self.argmax).nonzero().flatten().tolist()
        return "" if not bad else "; ".join(f"row {r} ({self.kinds[r]}): got {int(got[r])}, want {int(self.argmax[r])}" for r in bad)

    def verify_topk(self, got, k):
        want, rows = self.topk(k), (~self.has_nan).nonzero().flatten().tolist()
        bad = [r for r in rows if not torch.equal(got[r].cpu().to(torch.int32), want[r])]
        return "" if not bad else "; ".join(f"row {r} ({self.kinds[r]}), k {k}: got {got[r].tolist()}, want {want[r].tolist()}" for r in bad)


@dataclass(frozen=True)
class LsmCase:
    n: int

    @property
    def id(self):
        return f"lsm-n{self.n}"


LSM_CASES = tuple(LsmCase(n) for n in VOCAB_N)
LSM_KINDS = ("gauss", "gauss", "dominant0", "equal", "neginf", "gauss", "dominant_last", "neginf", "gauss")


class LsmProbe:
    """Rows: Gaussian (std 2), one dominant logit (25 against -30), all equal, Gaussian with -inf entries (whose outputs are -inf)."""

    def __init__(self, case):
        self.case = case
        n = case.n
        x = to_bf16(torch.randn((VOCAB_ROWS, n), generator=_gen("lsm", n)) * 2.0)
        for r, kind in enumerate(LSM_KINDS):
            if kind.startswith("dominant"):
                x[r] = -30.0
                x[r, 0 if kind == "dominant0" else n - 1] = 25.0
            elif kind == "equal":
                x[r] = 1.5
            elif kind == "neginf":
                x[r, 1::3] = -math.inf
        self.x = x
        self.lse = torch.logsumexp(x.to(F64), dim=-1, keepdim=True)
        self.lo, self.hi = self.bracket_at(1.0)

    def bracket_at(self, s):
        x64 = self.x.to(F64)
        l_lo, l_hi = bracket(self.lse, s * (2.0 ** -16 + 2.0 ** -22 * self.lse.abs()))
        return f32_down(x64 - l_hi.to(F64)).to(BF16), f32_up(x64 - l_lo.to(F64)).to(BF16)

    def restate(self, keep_f32=False, no_tail=False):
        """fp32 max, sum of exp, log; the normaliser rounded to bf16, then the subtraction.  Defects: the normaliser kept in fp32,
        the tail n % 1024 left out of the sum."""
        x = self.x.float()
        m = x.amax(-1, keepdim=True)
        e = torch.exp(x - m)
        if no_tail:
            e = e[:, :1024 * (self.case.n // 1024)]
        lse = m + torch.log(e.sum(-1, keepdim=True))
        return (x - (lse if keep_f32 else lse.to(BF16).float())).to(BF16)

    def verify(self, got, s=1.0):
        return worst(got, *self.bracket_at(s))


# ---------------------------------------------------------------- CLS rows
@dataclass(frozen=True)
class ClsCase:
    n_img: int
    dim: int
    tokens: int = 7

    @property
    def id(self):
        return f"cls-n{self.n_img}-d{self.dim}"


CLS_CASES = tuple(ClsCase(n, d) for n in (1, 5) for d in (8, 1024, 1030))


class ClsProbe:
    def __init__(self, case):
        self.case = c = case
        gen = _gen("cls", c.n_img, c.dim)
        self.cls = to_bf16(torch.randn((c.dim,), generator=gen))
        self.pos = to_bf16(torch.randn((c.tokens, c.dim), generator=gen))
        n = c.n_img * c.tokens * c.dim
        self.x = ((torch.arange(n) % 251) + 300).float().view(c.n_img, c.tokens, c.dim)
        self.want = self.x.clone()
        self.want[:, 0] = self.cls.float() + self.pos[0].float()

    def verify(self, got):
        bad = (got.view(torch.int32) != self.want.view(torch.int32)).nonzero()
        return "" if not len(bad) else f"{len(bad)} elements differ, first at {tuple(bad[0].tolist())}"


_PROBES = {RmsCase: RmsProbe, TableCase: TableProbe, RopeCase: RopeProbe, VocabCase: VocabProbe, LsmCase: LsmProbe, ClsCase: ClsProbe}


@lru_cache(maxsize=4)
def probe(case):
    """The inputs and reference of a case (the two LayerNorm output types share theirs)."""
    return ln_probe(case.hidden) if isinstance(case, LnCase) else _PROBES[type(case)](case)
