"""Probing inputs, fp64 references and acceptance rules for the QUANTISERS: the int8 KV cache -- p3v_kv_quantize (k_kv_quantize_v and the
scalar k_kv_quantize), p3v_kv_dequantize and the append paths of the three p3v_attention_decode_q8 kernels (csrc/p3v_attention.hip) -- and
the e4m3 activation quantiser p3v_quant_fp8_rows (k_quant_fp8_rows, csrc/p3v_gemm_fp8.hip).  Vocabulary of tests/glue_probe.py, whose
bracket / inside / worst / needed_scale are used as they are.  Everything here is torch on the CPU: tests/test_quant_probe_cpu.py shows on
the references alone that the inputs expose each defect, tests/test_quant_kernels_gpu.py runs the kernels.  Nothing here ever looks at
what a kernel produced.

INT8 KV CACHE.  A token (one K row, one V^T column of one batch row and kv head) is stored as a scale s and offset-binary codes.
  * SCALE RULE: s == fl32(amax / 127) bit for bit, ONE IEEE division of the token's largest magnitude (a bf16 value, exact in fp32); 1 for
    an all-zero token.
  * CODE RULE, AN INTEGER ROUNDING BRACKET: v = x / s in fp64 with s the expected fp32 scale; code - 128 must lie in
    [rint(v - E), rint(v + E)] (rint: to nearest, ties to even) for EVERY element, no shares.  E = 2^-22 |v|: the kernels compute
    x * fl(1 / s) for K and for every appended row and x / s for V in the two prefill quantisers -- the reciprocal rounds by relative 2^-24
    and the product by another 2^-24 (the division by 2^-24 alone); the sum 2^-23 is taken twice as large.  Both forms are accepted.
    Where s is a power of two every operation is exact and E = 0 (the GRID family).  On >= 98 % of the elements of every case the bracket
    is one value (asserted on the CPU): the rule reads "the correctly rounded code, except where x / s sits within 2^-22 of a tie".
  * INPUTS, per token.  GRID (exact ties): one element is +-127 2^e, the others (k / 2) 2^e with |k| <= 253, e per token in [-6, 6]: exact
    bf16 values, s = 2^e, about half of the elements exact .5 ties; the expected code is round-half-to-even, bit for bit.  SPREAD: 8-bit
    mantissas at exponents e - 3 .. e, one element (the maximum) m 2^(e + 1), e per token in [-6, 6] -- a neighbour token's scale is wrong
    by a power of two or by its mantissa.  In both families the maximum's position walks over hot_dims(hd): dim 0, dim hd - 1, the other
    half of their 2-element pairs, both sides of every 8-dim chunk edge (K and V start 13 positions apart; every batch row 5 further), and
    its sign alternates from token to token.  One token of K and one of V (in different rows) is all zero.
  * MEMORY.  Source positions outside [t0, t0 + n_tok) hold 1e4, so a leaked token takes the scale.  Destinations (codes and scales) hold
    position-dependent sentinels and sit between GUARD sentinel elements; everything outside the written window must come back
    bit-identical, and the sources untouched.
  * p3v_kv_dequantize: codes uniform over 0 .. 255 with 0, 128 and 255 in every token, scales with all 24 mantissa bits drawn, per token in
    [2^-10, 2^3).  Reference fp64 (code - 128) scale under bracket(v, 2^-24 |v|): the fp32 product rounds once (an 8-bit integer times 24
    bits), then the one rounding to bf16.  Tokens >= n_tok of the destination and the guards stay bit-identical.
  * Append (p3v_attention_decode_q8): rotation tables cos = 1, sin = 0, so a new key is its bf16 input exactly; the K and V parts of qkv
    are GRID and SPREAD tokens (alternating over batch row, head and new token; one V token all zero); the cache below `past` holds code
    128 with scale 1.  Scale and code rule on the appended K rows and V^T columns, bit-identity of everything else.  The attention output
    is tests/attn_probe.py's business and is not judged.

E4M3 ACTIVATION QUANTISER.  Inputs: the rows and weights of glue_probe's RMS_CASES (Gaussian rows and HOT-CHUNK rows at hidden 8, 520, 3064,
3072, 3080, 8192 -- a partly filled pass, both sides of the full 6-chunk layout, the first size on the 16-chunk layout and the full one --
and 1 / 6 / 33 rows: partly filled workgroups of four rows).
  * Without a norm weight (row 0 zeroed where there is more than one row): s == fl32(amax / 448) (1 for the zero row) and
    codes == e4m3_rne(fl32(x fl32(1 / s))), bit for bit.
  * With a norm weight: glue_probe's bracket [lo, hi] of the RMSNorm row h is the row the kernel quantises.  A row is KEPT when the two
    ends have the same largest magnitude and one element holds it at both ends (the maximum is one value); in kept rows
    s == fl32(amax / 448) bit for bit and every code lies between e4m3(fl32(lo inv)) and e4m3(fl32(hi inv)), inv = fl32(1 / s), the ends
    ordered as floats: one IEEE multiply and one correctly rounded conversion are monotonic and add no E of their own.  At least 3 of 4
    rows of a case are kept and the code bracket is one value on >= 98 % of the elements of kept rows (asserted on the CPU; a case that
    falls short takes the first seed at which the reference alone meets both, F8Probe / f8_probe()).
  * q and scale sit between GUARD sentinels, x is left alone, and quant(x, w) == quant(rmsnorm(x, w), None) bit for bit (GPU test).
"""
import math
from dataclasses import dataclass
from functools import lru_cache

import torch

import glue_probe as gp
from glue_probe import BF16, F32, F64, GUARD, _gen, bracket, inside, needed_scale, sentinel, to_bf16, unique_share, worst, worst_abs  # noqa: F401
from proj_probe import MIN_KEPT, MIN_UNIQUE
from qproj_probe import F8, U8, _full_f32

I32, I64 = torch.int32, torch.int64
BH = 3                                   # batch rows x kv heads of every p3v_kv_quantize / p3v_kv_dequantize case
OUTSIDE = 1.0e4                          # what the source holds outside [t0, t0 + n_tok)
FAMILIES = ("grid", "spread")


# ---------------------------------------------------------------- tokens
def hot_dims(hd):
    """Where the maximum of a token is put, in order of priority: dim 0, dim hd - 1, the other halves of their pairs, both sides of every
    8-dim chunk edge."""
    pos = [0, hd - 1, 1, hd - 2]
    for e in range(8, hd, 8):
        pos += [e - 1, e]
    seen = []
    for p in pos:
        if 0 <= p < hd and p not in seen:
            seen.append(p)
    return seen


def make_tokens(gen, n, hd, family, rot):
    """[n, hd] bf16 tokens of `family` (module docstring); token j has its maximum at hot_dims(hd)[(rot + j) % len]."""
    hot = hot_dims(hd)
    j = torch.arange(n)
    at = torch.tensor(hot)[(rot + j) % len(hot)]
    sign = (1 - 2 * ((rot + j) % 2)).to(F64)
    e = torch.randint(-6, 7, (n, 1), generator=gen).to(F64)
    if family == "grid":
        x = torch.randint(-253, 254, (n, hd), generator=gen).to(F64) / 2
        x[j, at] = 127.0 * sign
        x = x * 2.0 ** e
    else:
        mant = (128 + torch.randint(0, 128, (n, hd), generator=gen)).to(F64) / 128
        sg = torch.randint(0, 2, (n, hd), generator=gen).to(F64) * 2 - 1
        x = sg * mant * 2.0 ** (e - torch.randint(0, 4, (n, hd), generator=gen).to(F64))
        x[j, at] = sign * mant[j, at] * 2.0 ** (e[:, 0] + 1)
    assert torch.equal(to_bf16(x).to(F64), x), "a token element that bf16 does not hold"
    return to_bf16(x), at


def token_scale(x):
    """The expected fp32 scale of tokens [..., hd]: fl32(amax / 127), 1 for an all-zero token."""
    amax = x.to(F32).abs().amax(-1)
    return torch.where(amax > 0, amax / 127.0, torch.ones_like(amax))


def code_bracket(x, s, scale=1.0):
    """(lo, hi) of code - 128 for tokens x [..., hd] under their expected scales s [...], int64; E = scale x 2^-22 |v|, 0 where s is a
    power of two."""
    v = x.to(F64) / s.to(F64)[..., None]
    pow2 = ((s.contiguous().view(I32) & 0x7FFFFF) == 0)[..., None]
    E = torch.where(pow2, torch.zeros_like(v), v.abs() * (2.0 ** -22 * scale))
    return torch.round(v - E).to(I64), torch.round(v + E).to(I64)


def quantise(x, form="mul", rnd="even", s=None):
    """The kernels' documented arithmetic in torch fp32: (scale, codes uint8) of tokens x [..., hd].  form: "mul" x fl(1 / s) | "div" x / s;
    rnd: "even" (rintf) | "trunc" | "away" (half away from zero); s: the scales to use instead of the tokens' own."""
    s = token_scale(x) if s is None else s
    xf = x.to(F32)
    q = xf * (1.0 / s)[..., None] if form == "mul" else xf / s[..., None]
    q = torch.round(q) if rnd == "even" else torch.trunc(q) if rnd == "trunc" else torch.sign(q) * torch.floor(q.abs() + 0.5)
    return s, (q.to(I64) + 128).clamp(0, 255).to(U8)


def _code_msg(name, got_u8, lo, hi):
    g = got_u8.to(I64) - 128
    bad = (g < lo) | (g > hi)
    if not bool(bad.any()):
        return ""
    i = tuple(bad.nonzero()[0].tolist())
    return f"{name}: {int(bad.sum())} of {bad.numel()} codes outside; first at {i}: got {int(g[i])}, lo {int(lo[i])}, hi {int(hi[i])}"


def _scale_msg(name, got, want):
    bad = got.contiguous().view(I32) != want.contiguous().view(I32)
    if not bool(bad.any()):
        return ""
    i = tuple(bad.nonzero()[0].tolist())
    return f"{name}: {int(bad.sum())} of {bad.numel()} scales differ; first at {i}: got {float(got[i])!r}, want {float(want[i])!r}"


def u8_sentinel(n):
    """index % 251 as bytes: position-dependent, and no run of it is what a quantiser writes."""
    return (torch.arange(n) % 251).to(U8)


def f32_sentinel(n):
    return (torch.arange(n) % 251 + 300).to(F32)


def _outside_msg(name, flat, clean, mask):
    it = {1: U8, 2: torch.int16, 4: I32}[flat.element_size()]
    bad = mask & (flat.view(it) != clean.view(it))
    if not bool(bad.any()):
        return ""
    return f"{name}: {int(bad.sum())} elements outside the window changed, first at flat index {int(bad.nonzero()[0]) - GUARD}"


# ---------------------------------------------------------------- p3v_kv_quantize
@dataclass(frozen=True)
class KvCase:
    kernel: str                  # the kernel p3v_kv_quantize must take (asserted by arithmetic below)
    hd: int
    src_t: int
    dst_t: int
    t0: int
    n_tok: int
    knobs: tuple = ()

    @property
    def id(self):
        return f"kvq-{self.kernel}-hd{self.hd}-src{self.src_t}-dst{self.dst_t}-t0_{self.t0}-n{self.n_tok}" + ("-kvq_old" if self.knobs else "")

    @property
    def vector_ok(self):
        """The dispatch conditions of p3v_kv_quantize for k_kv_quantize_v (the buffers of these tests are 16-byte aligned)."""
        whole_tiles = -(-self.n_tok // 64) * 64 + self.t0 <= self.src_t
        return self.hd == 96 and self.t0 % 8 == 0 and self.src_t % 8 == 0 and self.dst_t % 8 == 0 and whole_tiles


KV_CASES = (
    KvCase("k_kv_quantize_v", 96, 256, 320, 0, 197),     # three whole tiles and a ragged one (5 tokens): the byte-wise tail of V^T
    KvCase("k_kv_quantize_v", 96, 128, 128, 64, 64),     # the tile ends at src_t
    KvCase("k_kv_quantize_v", 96, 256, 256, 8, 1),
    KvCase("k_kv_quantize", 96, 80, 96, 3, 70),          # unaligned t0, no whole tiles
    KvCase("k_kv_quantize", 64, 72, 72, 0, 65),
    KvCase("k_kv_quantize", 32, 64, 64, 5, 7),
    KvCase("k_kv_quantize", 96, 256, 320, 0, 197, knobs=(("kvq_old", 1),)),
)
for _c in KV_CASES:
    assert (_c.kernel == "k_kv_quantize_v") == (_c.vector_ok and not _c.knobs), _c.id
    assert _c.t0 + _c.n_tok <= min(_c.src_t, _c.dst_t) and _c.n_tok <= 320 and _c.hd % 2 == 0 and _c.hd <= 96
assert KV_CASES[0].n_tok % 8 != 0 and KV_CASES[0].n_tok % 64 != 0
assert len({c.id for c in KV_CASES}) == len(KV_CASES)


class KvProbe:
    """Sources K [BH, src_t, hd] and V [BH, src_t, hd] (token-major here; the kernel takes V^T), expected scales and code brackets of the
    window, sentinel-filled destinations, an emulation of the kernel with defects, and the acceptance rule."""

    def __init__(self, case, family):
        self.case, self.family, c = case, family, case
        assert family in FAMILIES
        gen = _gen("kvq", c.hd, c.src_t, c.dst_t, c.t0, c.n_tok, family)
        w = slice(c.t0, c.t0 + c.n_tok)
        self.k = to_bf16(torch.full((BH, c.src_t, c.hd), OUTSIDE))
        self.v = self.k.clone()
        self.at = {"k": [], "v": []}
        for bh in range(BH):
            for name, buf, rot in (("k", self.k, 5 * bh), ("v", self.v, 5 * bh + 13)):
                buf[bh, w], at = make_tokens(gen, c.n_tok, c.hd, family, rot)
                self.at[name] += at.tolist()
        self.zero = {"k": (1, c.n_tok // 2), "v": (2, c.n_tok // 2)}                     # (row, token of the window) that is all zero
        self.k[1, c.t0 + c.n_tok // 2] = 0
        self.v[2, c.t0 + c.n_tok // 2] = 0
        self.shapes = {"k8": (BH, c.dst_t, c.hd), "v8": (BH, c.hd, c.dst_t), "ksc": (BH, c.dst_t), "vsc": (BH, c.dst_t)}
        self.s = {"k": token_scale(self.k[:, w]), "v": token_scale(self.v[:, w])}       # [BH, n_tok]
        self.br = self.brackets_at(1.0)

    @property
    def vt(self):
        return self.v.transpose(1, 2).contiguous()                                      # [BH, hd, src_t]

    def brackets_at(self, scale):
        w = slice(self.case.t0, self.case.t0 + self.case.n_tok)
        return {"k": code_bracket(self.k[:, w], self.s["k"], scale), "v": code_bracket(self.v[:, w], self.s["v"], scale)}

    def unique(self):
        return min(float((lo == hi).double().mean()) for lo, hi in self.br.values())

    def tie_share(self):
        """Share of the window's elements whose x / s is an exact .5 tie (GRID: about half)."""
        w = slice(self.case.t0, self.case.t0 + self.case.n_tok)
        v = torch.cat([(t[:, w].to(F64) / self.s[n].to(F64)[..., None]).flatten() for n, t in (("k", self.k), ("v", self.v))])
        return float(((v * 2) % 2 == 1).double().mean())

    def buffers(self):
        """name -> the flat destination before the call: sentinel everywhere, GUARD elements in front and behind."""
        return {n: (u8_sentinel if n in ("k8", "v8") else f32_sentinel)(math.prod(sh) + 2 * GUARD) for n, sh in self.shapes.items()}

    def view(self, flat, name):
        return flat[GUARD:flat.numel() - GUARD].view(self.shapes[name])

    def emulate(self, form_k="mul", form_v="div", rnd="even", miss=None, neighbour=False, wrong_axis=False, leak=False, one_past=False):
        """The destinations as a kernel with the documented arithmetic leaves them.  Defects: `rnd`; miss = a dim left out of the maximum;
        the neighbour token's scale; V^T read as if it were token-major; the token behind the window leaking into the last scale; a write
        one token past the window."""
        c, flat = self.case, self.buffers()
        n = c.n_tok + (1 if one_past else 0)
        w = slice(c.t0, c.t0 + n)
        if n > c.n_tok and c.t0 + n > min(c.src_t, c.dst_t):
            return None                                                                  # (no room behind the window in this case)
        v_src = self.vt.reshape(BH, c.src_t, c.hd) if wrong_axis else self.v
        for name, src, form in (("k", self.k, form_k), ("v", v_src, form_v)):
            x = src[:, w]
            seen = x.clone()
            if miss is not None:
                seen[..., miss] = 0
            s = token_scale(seen)
            if leak and c.t0 + n < c.src_t:
                s[:, -1] = token_scale(torch.cat([seen[:, -1], src[:, c.t0 + n]], -1))
            if neighbour:
                s = s.roll(1, 1)
            s, q = quantise(x, form, rnd, s)
            self.view(flat[name + "sc"], name + "sc")[:, w] = s
            if name == "k":
                self.view(flat["k8"], "k8")[:, w] = q
            else:
                self.view(flat["v8"], "v8")[:, :, w] = q.transpose(1, 2)
        return flat

    def verify(self, flat, scale=1.0):
        """flat: name -> the flat destination after the call.  -> '' or what is wrong (scale: the code brackets under scale x E)."""
        c, msgs = self.case, []
        w = slice(c.t0, c.t0 + c.n_tok)
        br = self.brackets_at(scale)
        got = {n: self.view(flat[n], n) for n in self.shapes}
        msgs.append(_scale_msg("k_scale", got["ksc"][:, w], self.s["k"]))
        msgs.append(_scale_msg("v_scale", got["vsc"][:, w], self.s["v"]))
        msgs.append(_code_msg("k8", got["k8"][:, w], *br["k"]))
        msgs.append(_code_msg("v8t", got["v8"][:, :, w].transpose(1, 2), *br["v"]))
        clean = self.buffers()
        for n in self.shapes:
            mask = torch.ones(clean[n].numel(), dtype=torch.bool)
            body = self.view(mask, n)
            if n == "v8":
                body[:, :, w] = False
            else:
                body[:, w] = False
            msgs.append(_outside_msg(n, flat[n], clean[n], mask))
        return "; ".join(m for m in msgs if m)


# ---------------------------------------------------------------- p3v_kv_dequantize
@dataclass(frozen=True)
class DqCase:
    hd: int
    n_tok: int
    src_t: int = 320
    dst_t: int = 256

    @property
    def id(self):
        return f"kvdq-hd{self.hd}-n{self.n_tok}-src{self.src_t}-dst{self.dst_t}"


DQ_CASES = tuple(DqCase(hd, n) for hd in (96, 64) for n in (1, 70, 256))
assert any(c.n_tok * c.hd > 64 * 256 for c in DQ_CASES)                                  # the grid-stride loop of k_kv_dequantize wraps


class DqProbe:
    def __init__(self, case):
        self.case = c = case
        gen = _gen("kvdq", c.hd, c.n_tok)
        hot = hot_dims(c.hd)
        self.codes, self.scales = {}, {}
        for i, name in enumerate(("k", "v")):
            q = torch.randint(0, 256, (BH, c.src_t, c.hd), generator=gen)
            t = torch.arange(c.src_t)
            for j, val in enumerate((0, 128, 255)):                                     # in every token, at walking dims
                q[:, t, torch.tensor(hot)[(t + 7 * i + 3 * j) % len(hot)]] = val
            self.codes[name] = q.to(U8)                                                  # token-major [BH, src_t, hd]
            self.scales[name] = _full_f32(gen, (BH, c.src_t), -10, 2)
        self.shapes = {"k": (BH, c.dst_t, c.hd), "v": (BH, c.hd, c.dst_t)}
        self.ref = {n: (self.codes[n][:, :c.n_tok].to(F64) - 128) * self.scales[n][:, :c.n_tok].to(F64)[..., None] for n in ("k", "v")}

    @property
    def v8t(self):
        return self.codes["v"].transpose(1, 2).contiguous()

    def brackets_at(self, scale):
        return {n: bracket(r, r.abs() * (2.0 ** -24 * scale)) for n, r in self.ref.items()}

    def unique(self):
        return min(unique_share(lo, hi) for lo, hi in self.brackets_at(1.0).values())

    def buffers(self):
        return {n: sentinel(math.prod(sh) + 2 * GUARD) for n, sh in self.shapes.items()}

    def view(self, flat, name):
        return flat[GUARD:flat.numel() - GUARD].view(self.shapes[name])

    def emulate(self, offset=128.0, neighbour=False):
        """(code - 128) * scale in fp32, rounded once.  Defects: an offset of 127, the neighbour token's scale."""
        c, flat = self.case, self.buffers()
        for n in ("k", "v"):
            s = self.scales[n].roll(1, 1) if neighbour else self.scales[n]
            y = ((self.codes[n][:, :c.n_tok].to(F32) - offset) * s[:, :c.n_tok, None]).to(BF16)
            if n == "k":
                self.view(flat["k"], "k")[:, :c.n_tok] = y
            else:
                self.view(flat["v"], "v")[:, :, :c.n_tok] = y.transpose(1, 2)
        return flat

    def verify(self, flat, scale=1.0):
        c, msgs = self.case, []
        br, clean = self.brackets_at(scale), self.buffers()
        for n in ("k", "v"):
            got = self.view(flat[n], n)
            got = got[:, :c.n_tok] if n == "k" else got[:, :, :c.n_tok].transpose(1, 2)
            m = worst(got, *br[n])
            msgs.append(m and f"{n}: {m}")
            mask = torch.ones(clean[n].numel(), dtype=torch.bool)
            body = self.view(mask, n)
            if n == "k":
                body[:, :c.n_tok] = False
            else:
                body[:, :, :c.n_tok] = False
            msgs.append(_outside_msg(n, flat[n], clean[n], mask))
        return "; ".join(m for m in msgs if m)


# ---------------------------------------------------------------- append paths of p3v_attention_decode_q8
AP_B, AP_NH, AP_HD, AP_T = 2, 2, 96, 256                 # the geometry of test_kv_quantize_and_q8_decode


@dataclass(frozen=True)
class ApCase:
    n_split: int
    past: int
    L: int
    fused: bool = False
    knobs: tuple = ()

    @property
    def kernel(self):
        """p3v_attention_decode_q8's dispatch at cache_t = 256 (q8_old = 1 switches the two newer kernels off)."""
        T, S, new = AP_T, self.n_split, not self.knobs
        if new and T % 128 == 0 and S * 128 >= T and S * 64 < T:
            return "k_attn_decode128_q8"
        return "k_attn_decode_q8s" if new and S * 64 >= T and S <= 16 else "k_attn_decode_q8"

    @property
    def id(self):
        return f"append-{self.kernel}-split{self.n_split}-past{self.past}-L{self.L}" + ("-merge_in_launch" if self.fused else "")


# (62, 5) / (126, 5) cross a 64-key / a 128-key tile edge.  At 256 keys n_split = 3 is a 128-key plan too (3 x 128 >= 256 > 3 x 64, the third
# split empty): the multi-tile single-wave kernel takes it only with the launcher's A/B knob q8_old, two 64-key tiles a split.
AP_PAST_L = ((200, 1), (62, 5), (126, 5))
AP_CASES = (tuple(ApCase(3, p, L, knobs=(("q8_old", 1),)) for p, L in AP_PAST_L) + (ApCase(3, 200, 1),)
            + tuple(ApCase(S, p, L, f) for S in (4, 2) for p, L in AP_PAST_L for f in (False, True)))
assert [ApCase(s, 200, 1).kernel for s in (3, 4, 2)] == ["k_attn_decode128_q8", "k_attn_decode_q8s", "k_attn_decode128_q8"]
assert {c.kernel for c in AP_CASES if c.n_split == 3 and c.knobs} == {"k_attn_decode_q8"} and not any(c.knobs for c in AP_CASES if c.n_split != 3)
for _k in ("k_attn_decode_q8", "k_attn_decode_q8s", "k_attn_decode128_q8"):
    assert {(c.past, c.L) for c in AP_CASES if c.kernel == _k} == set(AP_PAST_L)
assert len({c.id for c in AP_CASES}) == len(AP_CASES)


class ApProbe:
    """qkv [B L, 3 nh hd] whose K and V heads are GRID / SPREAD tokens, caches that hold (128, scale 1) below `past` and sentinels from
    there on, the expected scales and code brackets of the appended tokens."""

    def __init__(self, case):
        self.case = c = case
        B, nh, hd, T, L = AP_B, AP_NH, AP_HD, AP_T, c.L
        gen = _gen("append", c.past, c.L)                                                # (shared by the kernels: the same rows everywhere)
        qkv = to_bf16(torch.randn((B, L, 3 * nh, hd), generator=gen))
        self.fam = {}
        for b in range(B):
            for h in range(nh):
                for r in range(L):
                    i = (b * nh + h) * L + r
                    for name, head, fam in (("k", nh + h, FAMILIES[i % 2]), ("v", 2 * nh + h, FAMILIES[(i + 1) % 2])):
                        qkv[b, r, head] = make_tokens(gen, 1, hd, fam, 3 * i + (13 if name == "v" else 0))[0][0]
                        self.fam[name, b, h, r] = fam
        qkv[1, 0, 2 * nh + 1] = 0                                                        # one all-zero V token
        self.qkv = qkv.view(B * L, 3 * nh * hd)
        self.cos, self.sin = torch.ones((B, L, hd // 2), dtype=F32), torch.zeros((B, L, hd // 2), dtype=F32)
        self.new = {"k": qkv[:, :, nh:2 * nh].transpose(1, 2).contiguous(), "v": qkv[:, :, 2 * nh:].transpose(1, 2).contiguous()}      # [B, nh, L, hd]
        self.s = {n: token_scale(x) for n, x in self.new.items()}
        self.shapes = {"k8": (B, nh, T, hd), "v8": (B, nh, hd, T), "ksc": (B, nh, T), "vsc": (B, nh, T)}
        self.br = self.brackets_at(1.0)

    def brackets_at(self, scale):
        return {n: code_bracket(self.new[n], self.s[n], scale) for n in ("k", "v")}

    def unique(self):
        return min(float((lo == hi).double().mean()) for lo, hi in self.br.values())

    def view(self, flat, name):
        return flat[GUARD:flat.numel() - GUARD].view(self.shapes[name])

    def buffers(self):
        c, flat = self.case, {}
        for n, sh in self.shapes.items():
            codes = n in ("k8", "v8")
            flat[n] = (u8_sentinel if codes else f32_sentinel)(math.prod(sh) + 2 * GUARD)
            body = self.view(flat[n], n)
            if n == "v8":
                body[..., :c.past] = 128
            elif n == "k8":
                body[:, :, :c.past] = 128
            else:
                body[..., :c.past] = 1.0
        return flat

    def emulate(self, form="mul", rnd="even", miss=None, neighbour=False):
        c, flat = self.case, self.buffers()
        w = slice(c.past, c.past + c.L)
        for n in ("k", "v"):
            seen = self.new[n].clone()
            if miss is not None:
                seen[..., miss] = 0
            s = token_scale(seen)
            s, q = quantise(self.new[n], form, rnd, s.roll(1, 0) if neighbour else s)
            self.view(flat[n + "sc"], n + "sc")[:, :, w] = s
            if n == "k":
                self.view(flat["k8"], "k8")[:, :, w] = q
            else:
                self.view(flat["v8"], "v8")[:, :, :, w] = q.transpose(2, 3)
        return flat

    def verify(self, flat, scale=1.0):
        c, msgs = self.case, []
        w = slice(c.past, c.past + c.L)
        br = self.brackets_at(scale)
        got = {n: self.view(flat[n], n) for n in self.shapes}
        msgs.append(_scale_msg("k_scale", got["ksc"][:, :, w], self.s["k"]))
        msgs.append(_scale_msg("v_scale", got["vsc"][:, :, w], self.s["v"]))
        msgs.append(_code_msg("k8", got["k8"][:, :, w], *br["k"]))
        msgs.append(_code_msg("v8t", got["v8"][:, :, :, w].transpose(2, 3), *br["v"]))
        clean = self.buffers()
        for n in self.shapes:
            mask = torch.ones(clean[n].numel(), dtype=torch.bool)
            body = self.view(mask, n)
            if n == "v8":
                body[..., w] = False
            elif n == "k8":
                body[:, :, w] = False
            else:
                body[..., w] = False
            msgs.append(_outside_msg(n, flat[n], clean[n], mask))
        return "; ".join(m for m in msgs if m)


# ---------------------------------------------------------------- p3v_quant_fp8_rows
@dataclass(frozen=True)
class F8Case:
    hidden: int
    rows: int
    norm: bool

    @property
    def rms(self):
        return gp.RmsCase(self.hidden, self.rows)

    @property
    def kernel(self):
        return f"k_quant_fp8_rows<{'true' if self.norm else 'false'}, {6 if -(-(self.hidden // 8) // 64) <= 6 else 16}>"

    @property
    def id(self):
        return f"qf8-h{self.hidden}-r{self.rows}" + ("-norm" if self.norm else "")


F8_CASES = tuple(F8Case(c.hidden, c.rows, norm) for c in gp.RMS_CASES for norm in (False, True))
assert {c.hidden for c in F8_CASES} == {8, 520, 3064, 3072, 3080, 8192} and {c.rows for c in F8_CASES} == {1, 6, 33}


def e4m3(x):
    """fp32 -> e4m3 bytes, round to nearest even (saturating at 448 as the hardware conversion does; nothing here exceeds 448 (1 + 2^-22))."""
    return x.to(F32).clamp(-448.0, 448.0).to(F8).view(U8)


def f8_value(b):
    return b.contiguous().view(F8).to(F64)


def f8_quantise(h, per_element_inv=False):
    """The kernel's documented arithmetic on rows h (bf16): s = amax / 448 (1 for a zero row), codes = e4m3(h * (1 / s)).  Defect: the
    factor computed as 448 / amax."""
    hf = h.to(F32)
    amax = hf.abs().amax(-1)
    s = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    inv = torch.where(amax > 0, 448.0 / amax, torch.ones_like(amax)) if per_element_inv else 1.0 / s
    return s, e4m3(hf * inv[:, None])


class F8Probe:
    """The rows of glue_probe's RmsProbe (seed > 0: the same construction on another stream of the generator), the expected scale and the
    codes (no norm) or code brackets (norm), and the kept rows."""

    def __init__(self, case, seed=0):
        self.case = case
        rms = gp.probe(case.rms) if seed == 0 else gp.RmsProbe(case.rms, seed)
        self.rms, self.w = rms, rms.w
        self.x = rms.x.clone()
        if not case.norm and case.rows > 1:
            self.x[0] = 0
        if not case.norm:
            self.s, self.codes = f8_quantise(self.x)
            self.kept = torch.ones(case.rows, dtype=torch.bool)
            return
        lo, hi = rms.lo.to(F32), rms.hi.to(F32)
        a_lo, a_hi = lo.abs().amax(-1), hi.abs().amax(-1)
        one = ((lo.abs() == a_lo[:, None]) & (hi.abs() == a_lo[:, None])).any(-1)
        self.kept = (a_lo == a_hi) & one
        amax = torch.where(self.kept, a_lo, torch.ones_like(a_lo))
        self.s = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
        inv = 1.0 / self.s
        c1, c2 = f8_value(e4m3(lo * inv[:, None])), f8_value(e4m3(hi * inv[:, None]))
        self.c_lo, self.c_hi = torch.minimum(c1, c2), torch.maximum(c1, c2)

    def shares(self):
        """(share of rows kept, share of the elements of kept rows whose code bracket is one value)."""
        if not self.case.norm:
            return 1.0, 1.0
        k = self.kept
        return float(k.double().mean()), (float((self.c_lo[k] == self.c_hi[k]).double().mean()) if bool(k.any()) else 0.0)

    def buffers(self):
        c = self.case
        return {"q": u8_sentinel(c.rows * c.hidden + 2 * GUARD), "scale": f32_sentinel(c.rows + 2 * GUARD)}

    def emulate(self, drop=None, skip_round=False, amax_before_w=False, per_element_inv=False):
        """The buffers as a kernel with the documented arithmetic leaves them.  Defects (norm): chunk `drop` left out of the sum of squares,
        the first rounding of the norm skipped, amax taken before the norm weight; (both) the factor computed as 448 / amax."""
        c, flat = self.case, self.buffers()
        h = self.rms.restate(drop=drop, skip_round=skip_round) if c.norm else self.x
        s, q = f8_quantise(h, per_element_inv)
        if amax_before_w:
            x = self.x.float()
            n = (x * torch.rsqrt((x * x).sum(-1, keepdim=True) * (1.0 / c.hidden) + gp.EPS)).to(BF16)
            amax = n.float().abs().amax(-1)
            s = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
            q = e4m3(h.float() * (1.0 / s)[:, None])
        flat["q"][GUARD:-GUARD] = q.flatten()
        flat["scale"][GUARD:-GUARD] = s
        return flat

    def verify(self, flat):
        c, msgs = self.case, []
        q = flat["q"][GUARD:-GUARD].view(c.rows, c.hidden)
        s = flat["scale"][GUARD:-GUARD]
        k = self.kept
        msgs.append(_scale_msg("scale", s[k], self.s[k]))
        if not c.norm:
            bad = q != self.codes
            if bool(bad.any()):
                i = tuple(bad.nonzero()[0].tolist())
                msgs.append(f"{int(bad.sum())} of {bad.numel()} codes differ, first at {i}: got {int(q[i]):#04x}, want {int(self.codes[i]):#04x}")
        else:
            m = worst(f8_value(q)[k], self.c_lo[k], self.c_hi[k])
            msgs.append(m and f"codes: {m}")
        clean = self.buffers()
        for n in ("q", "scale"):
            mask = torch.ones(clean[n].numel(), dtype=torch.bool)
            mask[GUARD:-GUARD] = False
            msgs.append(_outside_msg(n, flat[n], clean[n], mask))
        return "; ".join(m for m in msgs if m)


@lru_cache(maxsize=None)
def f8_probe(case):
    """The probe of a case: the first seed (0: glue_probe's own rows) at which the REFERENCE keeps >= 3 of 4 rows and has a one-valued code
    bracket on >= 98 % of the elements of kept rows.  Nothing here looks at a kernel's output."""
    for seed in range(64):
        pr = F8Probe(case, seed)
        kept, uniq = pr.shares()
        if kept >= MIN_KEPT and uniq >= MIN_UNIQUE:
            pr.seed = seed
            return pr
    raise AssertionError(f"{case.id}: no seed below 64 meets the caps")


@lru_cache(maxsize=4)
def probe(case, family=None):
    if isinstance(case, KvCase):
        return KvProbe(case, family)
    return {DqCase: DqProbe, ApCase: ApProbe, F8Case: f8_probe}[type(case)](case)
