"""Probing inputs, fp64 references and acceptance rules for p3v_gemm_qkv: the qkv projection with the head split, the rotation and
the KV append in its epilogue (csrc/p3v_gemm_qkv.h), as k_gemm_skinny<QKV>, k_gemm<QKV> and k_gemm256<QKV> run it.  Layout and
vocabulary of tests/glue_probe.py and tests/proj_probe.py, whose parts are used as they are: the projection's inputs, exact sums and
accumulator bound are proj_probe's (GRID and SPIKES), the rotation reference and its bound glue_probe.RopeProbe's, the rounding bracket,
`worst`, `needed_scale`, the sentinel and GUARD glue_probe's.  Everything here is torch on the CPU: tests/test_qkv_probe_cpu.py shows on
the references alone that the inputs expose each defect, tests/test_qkv_kernels_gpu.py runs the kernels.

WHAT A CASE IS.  A [B L, K] and W [(nh + 2 nkv) hd, K] (and a bias) from proj_probe.Probe under both families; rotation tables as
RopeProbe builds them (fp64 cos / sin rounded to fp32, table g = batch row / tab_div starts at position base + 1000 g, one spare row
behind the window); destinations q [B, nh, L, hd], k [B, nkv, dst_t, hd], v [B, nkv, hd, dst_t] with dst_t = roundup(dpos0 + L, 8) + 8
(no multiple of 64 unless by accident), each inside a sentinel buffer with GUARD elements on both sides.

ACCEPTANCE: EVERY ELEMENT, NO SHARES, NO ATOL.
  * y, the Linear's bf16 output.  GRID: the exact sum (+ bias) rounded once -- one known tensor, E = 0.  SPIKES: the bracket [y_lo, y_hi]
    of proj_probe's accumulator rule.
  * V^T.  GRID: bit-equal to y's V columns, transposed.  SPIKES: inside [y_lo, y_hi].
  * Q / K with tables: RopeProbe's bracket, E = 2^-21 (|a cos| + |b sin|) q_scale, around the fp64 rotation of y.  On SPIKES a member of
    a pair may have two candidate values; a cos - b sin and b cos + a sin are monotonic in each member, so the smallest low end and the
    largest high end over the four corner combinations bound what a kernel may store.
  * Q / K with null tables.  q_scale = 1: y itself (GRID: bit-equal).  Otherwise bf16(float(y) q_scale) restated in torch fp32: ONE IEEE
    multiply, monotonic in y, so the two ends of y's bracket give the two ends here (GRID: bit-equal).
  * Memory.  Everything outside the windows -- guard bands, cache rows outside [dpos0, dpos0 + L), V^T columns outside it -- comes back
    bit-identical.  (That A, W with their 2^15 padding and the tables are left alone is asserted by the GPU test on its own copies.)
On >= 98 % of the judged elements of every case the bracket is one value (asserted on the CPU); a case of fewer than 4096 projection
outputs takes the first seed at which that and proj_probe's own conditions hold.  Nothing here ever looks at what a kernel produced.

THE CASES come from gemm_route() (csrc/p3v_gemm.hip) and DESIGN.md section 3.2: M < 1024 rows without a bias run on k_gemm_skinny<QKV>
(9 .. gemm_skinny_max_m rows, Q region % 64, K / V regions % 128); M >= 1024 on k_gemm256<QKV> for the first gemm_big_rows() rows where
the Q and K / V regions are multiples of 256, the rest on k_gemm<QKV>, which gets m_base = the rows in front of it.  Every case pins the
knobs and states the launches the route must answer (`QkvCase.launches`; check_route asserts them through ops.gemm_route)."""
import math
from dataclasses import dataclass
from functools import lru_cache

import numpy as np
import torch

import glue_probe as gp
import proj_probe as pp
from glue_probe import BF16, F32, F64, GUARD, bracket, needed_scale, sentinel, unique_share, worst  # noqa: F401 (needed_scale: for the tests)

FAMILIES = pp.FAMILIES
SKINNY, K128, K256 = "k_gemm_skinny", "k_gemm", "k_gemm256"
MIN_UNIQUE = 0.98
AUTO = -1                                 # gemm_big_rows = -1: the launcher's own cost model


@dataclass(frozen=True)
class QkvCase:
    kernel: str                  # SKINNY | K128 | K256 | K256 + "+" + K128
    B: int
    L: int
    hd: int
    nh: int
    nkv: int
    K: int
    past: int = 0
    off_is_past: bool = True     # False: the append goes to offset 0, the rotation still uses position past + l
    tab_div: int = 1
    prescale: bool = False       # q_scale = hd^-0.5 log2 e
    null: bool = False           # null tables: a plain head split
    bias: bool = False
    ld: bool = False             # lda = K + 8, ldw = K + 24, the padding holds 2^15
    big_rows: int = 512          # the gemm_big_rows knob
    rows_big: int = 0            # rows the route must put on k_gemm256<QKV>
    base: int = 0                # position of table row 0

    @property
    def M(self):
        return self.B * self.L

    @property
    def N(self):
        return (self.nh + 2 * self.nkv) * self.hd

    @property
    def q_scale(self):
        return float(np.float32(self.hd ** -0.5 * gp.Q_PRESCALE)) if self.prescale else 1.0

    @property
    def dpos0(self):
        return self.past if self.off_is_past else 0

    @property
    def dst_t(self):
        return 8 * -(-(self.dpos0 + self.L) // 8) + 8

    @property
    def tab_t(self):
        return self.past + self.L + 1

    @property
    def knobs(self):
        return (("gemm_big_rows", self.big_rows), ("gemm_skinny_max_m", 256), ("gemm_128", 0), ("gemm_no_skinny", 0), ("gemm_no_qkv_fuse", 0))

    @property
    def launches(self):
        """((kernel, row0, rows), ...): what the route must answer."""
        if self.kernel == SKINNY:
            return ((SKINNY, 0, self.M),)
        big = ((K256, 0, self.rows_big),) if self.rows_big else ()
        return big + (((K128, self.rows_big, self.M - self.rows_big),) if self.rows_big < self.M else ())

    @property
    def id(self):
        s = f"{self.kernel}-B{self.B}-L{self.L}-hd{self.hd}-h{self.nh}x{self.nkv}-K{self.K}-past{self.past}"
        s += "" if self.off_is_past else "-scratch"
        s += f"-div{self.tab_div}" if self.tab_div > 1 else ""
        s += "-qs" if self.prescale else ""
        s += "-null" if self.null else ""
        s += "-bias" if self.bias else ""
        s += "-ld" if self.ld else ""
        return s + ("" if self.kernel == SKINNY else "-auto" if self.big_rows == AUTO else f"-big{self.big_rows}")


# ---------------------------------------------------------------- the table
def _cases():
    c = []
    # k_gemm_skinny<QKV>: 9 <= M <= 256, no bias.  (B, L): one tile less than full / one row past a 128-row tile / two rows / odd L (V runs at
    # odd offsets and across row ends) / rows shorter than a V run of 8 tokens: (16, 1), (3, 3), (5, 5) -- a run spans three and more rows --
    # and (6, 7).  K = 64 is one K-tile.
    sk = lambda B, L, heads, K, **kw: QkvCase(SKINNY, B, L, *heads, K, **kw)
    H96, H64, H32, H128 = (96, 2, 4), (64, 2, 2), (32, 4, 4), (128, 1, 1)
    c += [sk(1, 9, H96, 64), sk(1, 9, H128, 192, past=8, prescale=True, ld=True),
          sk(1, 129, H64, 192, past=8, prescale=True), sk(1, 129, H32, 64, past=200, base=4090),
          sk(2, 64, H32, 64, past=64, ld=True), sk(2, 64, H96, 192, null=True),
          sk(3, 85, H128, 192, ld=True, base=100000), sk(3, 85, H96, 3072, past=8, prescale=True), sk(3, 85, H64, 64, null=True, prescale=True),
          sk(4, 61, H96, 192, past=200, prescale=True), sk(4, 61, H64, 64, past=13, off_is_past=False, base=4090),
          sk(16, 1, H64, 64, past=8), sk(16, 1, H96, 192, past=64, prescale=True, ld=True),
          sk(3, 3, H32, 192, null=True, prescale=True), sk(3, 3, H96, 64, past=200),
          sk(5, 5, H96, 64, past=13, off_is_past=False), sk(5, 5, H128, 192, past=8, ld=True),
          sk(6, 7, H128, 3072, past=64, tab_div=3, base=4000), sk(6, 7, H32, 64, tab_div=3, prescale=True)]
    # k_gemm<QKV> alone: M >= 1024 with gemm_big_rows = 0, or a region that is no multiple of 256 (96 x 4 = 384)
    c += [QkvCase(K128, 1, 1024, 96, 4, 4, 64, big_rows=0),
          QkvCase(K128, 1, 1025, 96, 4, 4, 128, past=8, prescale=True, ld=True),
          QkvCase(K128, 3, 343, 96, 8, 4, 64, past=64, base=100000),                                   # GQA: regions of 768 and 384 columns
          QkvCase(K128, 3, 343, 96, 4, 4, 64, past=13, off_is_past=False, bias=True, prescale=True, big_rows=0),   # rotation AND bias
          QkvCase(K128, 2, 577, 64, 2, 2, 1024, null=True, bias=True, off_is_past=False),              # the CLIP call
          QkvCase(K128, 6, 171, 64, 2, 2, 64, past=200, tab_div=3, big_rows=0, base=4000),
          # gemm_big_rows = -1: at 1100 x 2304 x 3072 nine tiles of rows x 18 small column tiles are one partial round (0.42) against >= 1 for
          # any split with a big tile (gemm_big_rows(), p3v_gemm.hip): all rows on k_gemm -- its K = 3072 case, the largest reference
          QkvCase(K128, 1, 1100, 96, 8, 8, 3072, past=8, bias=True, prescale=True, big_rows=AUTO)]
    # k_gemm256<QKV>: regions % 256.  All rows big (a ragged last tile of 6 / 76 rows), or 512 big rows and the rest on k_gemm<QKV> with
    # m_base = 512 inside batch row 0 (2 x 550) and inside batch row 1 (3 x 343)
    c += [QkvCase(K256, 1, 1030, 64, 4, 4, 64, big_rows=1000000, rows_big=1030),
          QkvCase(K256, 2, 550, 64, 4, 4, 3072, past=200, ld=True, big_rows=1000000, rows_big=1100),
          QkvCase(K256, 3, 343, 96, 8, 8, 64, past=64, bias=True, prescale=True, big_rows=1000000, rows_big=1029),
          QkvCase(K256 + "+" + K128, 2, 550, 96, 8, 8, 64, past=8, rows_big=512),
          QkvCase(K256 + "+" + K128, 3, 343, 64, 4, 4, 128, bias=True, prescale=True, rows_big=512, base=4090),
          QkvCase(K256 + "+" + K128, 3, 343, 96, 8, 8, 64, past=13, off_is_past=False, ld=True, rows_big=512),
          QkvCase(K256 + "+" + K128, 2, 550, 64, 4, 4, 64, null=True, bias=True, rows_big=512)]
    return tuple(c)


CASES = _cases()
assert len({c.id for c in CASES}) == len(CASES)


def check_route(ops, case, cu_count=0):
    """Asserts through ops.gemm_route, under the knobs as they are now, that the call of `case` runs the launches the case states."""
    L = ops.L
    kinds = {SKINNY: L.GEMM_K_SKINNY_QKV, K128: L.GEMM_K_128_QKV, K256: L.GEMM_K_256_QKV}
    r = ops.gemm_route(case.M, case.N, case.K, epilogue=pp.BIAS if case.bias else pp.NONE, entry=L.GEMM_ENTRY_QKV,
                       lda=case.K + (8 if case.ld else 0), ldw=case.K + (24 if case.ld else 0), has_bias=case.bias, n_heads=case.nh,
                       n_kv=case.nkv, hd=case.hd, dst_off=case.dpos0, dst_t=case.dst_t, cu_count=cu_count)
    got = tuple((r.launch[i].kernel, r.launch[i].name.decode().split("<")[0], r.launch[i].row0, r.launch[i].rows) for i in range(r.n_launches))
    want = tuple((kinds[k], k, row0, rows) for k, row0, rows in case.launches)
    assert r.status == 0 and r.S == 1 and got == want, f"{case.id}: route status {r.status}, launches {got}, the case is built for {want}"
    return r


# ---------------------------------------------------------------- which token goes where
def token_maps(case, defect=None):
    """Where the epilogues store token m: (b, l, stored) for the Q / K rows and for the V^T columns, each over the M tokens.  V^T is
    stored in runs of 8 tokens that start at multiples of 8: a run inside one batch row and inside M goes out as one store (three at
    an odd offset), every other run token by token.  `defect`: see tests/test_qkv_probe_cpu.py."""
    M, L = case.M, case.L
    m = torch.arange(M)
    b, l = m // L, m % L
    qk = [b.clone(), l.clone(), torch.ones(M, dtype=torch.bool)]
    v = [b.clone(), l.clone(), torch.ones(M, dtype=torch.bool)]
    m0 = m // 8 * 8
    b0, l0 = m0 // L, m0 % L
    fast = (m0 + 8 <= M) & (l0 + 8 <= L)
    if defect == "m_base_dropped":                               # the second launch takes its own row 0 for token 0
        late = m >= case.rows_big
        for mp in (qk, v):
            mp[0] = torch.where(late, (m - case.rows_big) // L, mp[0])
            mp[1] = torch.where(late, (m - case.rows_big) % L, mp[1])
    elif defect == "v_odd_shift":
        v[1] = torch.where(fast & (l0 % 2 == 1), l + 1, l)
    elif defect == "v_wrap_once":                                # le = l0 + e; if (le >= L) { le -= L; ++be; }
        le = l0 + (m - m0)
        over = le >= L
        v[0], v[1] = torch.where(fast, b, b0 + over.long()), torch.where(fast, l, le - L * over.long())
    elif defect == "v_tail_dropped":
        v[2] = m < M // 8 * 8
    return qk, v


def odd_runs(case):
    """Number of whole V^T runs that start at an odd offset of a batch row."""
    m0 = torch.arange(0, case.M, 8)
    return int(((m0 + 8 <= case.M) & (m0 % case.L + 8 <= case.L) & (m0 % case.L % 2 == 1)).sum())


def _scatter(flat, idx, val):
    ok = (idx >= 0) & (idx < flat.numel())                       # (what would leave the allocation is dropped, guard bands are inside)
    flat[idx[ok]] = val[ok]


class QkvProbe:
    """Inputs, fp64 reference, brackets, buffers and a torch restatement (with defects) of one case under one family."""

    def __init__(self, case, family, seed=0):
        self.case, self.family, c = case, family, case
        self.grid = family == "grid"
        self.heads = c.nh + 2 * c.nkv
        self.lin = pp.Probe(pp.Case(c.kernel, c.M, c.N, c.K, pp.BIAS if c.bias else pp.NONE, ld=c.ld, tag=c.id), family, seed)
        self.rope = self.cos = self.sin = None
        if not c.null:
            self.rope = gp.RopeProbe(gp.RopeCase(c.L, c.past, c.hd, c.nh, c.nkv, B=c.B, tab_div=c.tab_div, off_is_past=c.off_is_past,
                                                 prescale=c.prescale, base=c.base))
            assert self.rope.case.q_scale == c.q_scale and self.rope.case.tab_t == c.tab_t
            self.cos, self.sin = self.rope.cos, self.rope.sin    # [B / tab_div, tab_t, hd / 2] fp32
        self.shapes = {"q": (c.B, c.nh, c.L, c.hd), "k": (c.B, c.nkv, c.dst_t, c.hd), "v": (c.B, c.nkv, c.hd, c.dst_t)}
        self._br1 = self._y = None

    # ---- the reference
    def _heads(self, y):
        c = self.case
        return y.view(c.B, c.L, self.heads, c.hd)

    def _rotate(self, y, dtype, **defect):
        """RopeProbe's rotation of the Linear output y [M, N] bf16."""
        self.rope.qkv = y.contiguous()
        return self.rope.rotate(dtype, **defect)

    def _plain(self, y, scale_keys=False):
        """Null tables: the head split [B, nh + nkv, L, hd], the queries times q_scale in one fp32 multiply."""
        c = self.case
        x = self._heads(y)[:, :, :c.nh + c.nkv].transpose(1, 2)
        if c.q_scale == 1.0:
            return x.contiguous()
        qs = torch.ones(c.nh + c.nkv, dtype=F32)
        qs[:c.nh if not scale_keys else None] = c.q_scale
        return (x.float() * qs[None, :, None, None]).to(BF16)

    def brackets(self, s=1.0):
        """name -> (lo, hi) over the windows, under s x E: q [B, nh, L, hd], k [B, nkv, L, hd], v [B, nkv, hd, L]."""
        if s == 1.0 and self._br1 is not None:
            return self._br1
        c, half = self.case, self.case.hd // 2
        _, y_lo, y_hi, _ = self.lin.reference(s)
        one = bool(torch.equal(y_lo.view(torch.int16), y_hi.view(torch.int16)))
        assert one or not self.grid
        vt = lambda y: self._heads(y)[:, :, c.nh + c.nkv:].permute(0, 2, 3, 1)
        res = {"v": (vt(y_lo), vt(y_hi))}
        if c.null:
            lo, hi = self._plain(y_lo), self._plain(y_hi)
        else:
            lo = hi = None
            for ya, yb in (((y_lo, y_lo),) if one else ((y_lo, y_lo), (y_lo, y_hi), (y_hi, y_lo), (y_hi, y_hi))):
                y = self._heads(ya).clone()
                y[..., half:] = self._heads(yb)[..., half:]
                ref, E = self._rotate(y.view(c.M, c.N), F64)
                b_lo, b_hi = bracket(ref, E * s)
                lo = b_lo.float() if lo is None else torch.minimum(lo, b_lo.float())
                hi = b_hi.float() if hi is None else torch.maximum(hi, b_hi.float())
            lo, hi = lo.to(BF16), hi.to(BF16)
        res["q"], res["k"] = (lo[:, :c.nh], hi[:, :c.nh]), (lo[:, c.nh:], hi[:, c.nh:])
        if s == 1.0:
            self._br1 = res
        return res

    def unique_shares(self):
        """name -> share of the judged elements whose bracket is one value."""
        return {n: unique_share(lo, hi) for n, (lo, hi) in self.brackets().items()}

    # ---- buffers
    def buffers(self):
        """name -> the flat sentinel buffer of a destination, GUARD elements in front of and behind it."""
        return {n: sentinel(math.prod(sh) + 2 * GUARD) for n, sh in self.shapes.items()}

    def operand_buffers(self):
        """A and W inside their [rows, ld] buffers (the padding holds 2^15)."""
        return self.lin.operand_buffers()

    def window(self, name, flat):
        """The elements of a flat destination buffer that the call writes, in the bracket's shape."""
        c = self.case
        body = flat[GUARD:GUARD + math.prod(self.shapes[name])].view(self.shapes[name])
        w = slice(c.dpos0, c.dpos0 + c.L)
        return body if name == "q" else body[:, :, w] if name == "k" else body[:, :, :, w]

    # ---- acceptance
    def verify(self, flat, s=1.0):
        """flat: name -> the flat buffer after the call.  -> '' or what is wrong (s: the brackets under s x E)."""
        c, msgs = self.case, []
        br = self.brackets(s)
        for name in ("q", "k", "v"):
            got, (lo, hi) = self.window(name, flat[name]), br[name]
            m = worst(got, lo, hi)
            if not m and self.grid and (name == "v" or c.null) and not torch.equal(got.contiguous().view(torch.int16), lo.contiguous().view(torch.int16)):
                m = "not bit-equal to the exact value"
            if m:
                msgs.append(f"{name}: {m}")
            clean = sentinel(flat[name].numel())
            mask = torch.ones(clean.numel(), dtype=torch.bool)
            self.window(name, mask)[:] = False
            bad = mask & (flat[name].view(torch.int16) != clean.view(torch.int16))
            if bool(bad.any()):
                msgs.append(f"{name}: {int(bad.sum())} elements outside the window changed, first at flat index {int(bad.nonzero()[0]) - GUARD} "
                            f"of {tuple(self.shapes[name])}")
        return "; ".join(msgs)

    # ---- the documented arithmetic in torch fp32, with defects
    def linear(self, defect=None):
        """The Linear's bf16 output [M, N]: fp32 sums (GRID: exact in any order), the bias added, one rounding."""
        c, lin = self.case, self.lin
        plain = defect not in ("drop_last_ktile", "lda_as_k", "bias_half", "v_bias_by_token")
        if plain and self._y is not None:
            return self._y
        A, W = lin.A.float(), lin.W.float()
        if defect == "lda_as_k":                                 # (the padded buffer read with the wrong stride)
            A = lin.operand_buffers()[0].flatten()[:c.M * c.K].view(c.M, c.K).float()
        if defect == "drop_last_ktile":
            A[:, c.K - 64:] = 0
        acc = A @ W.T
        if c.bias:
            bias, nqk = lin.bias.float().clone(), (c.nh + c.nkv) * c.hd
            if defect == "bias_half":                            # the second halves of the pairs get the first halves' bias
                bh = bias[:nqk].view(-1, c.hd)
                bh[:, c.hd // 2:] = bh[:, :c.hd // 2]
            if defect == "v_bias_by_token":                      # the swapped tile's lanes hold tokens where the others hold columns
                acc[:, nqk:] += bias[nqk + torch.arange(c.M) % (c.nkv * c.hd)][:, None]
                bias[nqk:] = 0
            acc = acc + bias
        y = acc.to(BF16)
        if plain:
            self._y = y
        return y

    def emulate(self, defect=None):
        """The buffers as a kernel with the restated arithmetic (and `defect`) leaves them."""
        c, half = self.case, self.case.hd // 2
        y = self.linear(defect)
        if c.null:
            o = self._plain(y, scale_keys=defect == "scale_keys")
        elif defect == "pair_half32":                            # the partner taken 32 columns away instead of hd / 2
            y1, y2 = self._heads(y).clone(), self._heads(y).clone()
            y1[..., half:] = self._heads(torch.roll(y, -32, 1))[..., :half]
            y2[..., :half] = self._heads(torch.roll(y, 32, 1))[..., half:]
            o = torch.cat([self._rotate(y1.view(c.M, c.N), F32)[..., :half], self._rotate(y2.view(c.M, c.N), F32)[..., half:]], dim=-1)
        else:
            kw = {"pos_dpos0": {"pos_shift": c.dpos0 - c.past}, "tab_div_ignored": {"row_b": True}, "scale_keys": {"scale_keys": True},
                  "scale_after": {"scale_after": True}}.get(defect, {})
            o = self._rotate(y, F32, **kw)
        rows = o.transpose(1, 2).reshape(c.M, c.nh + c.nkv, c.hd)                # per token
        vrows = self._heads(y)[:, :, c.nh + c.nkv:].reshape(c.M, c.nkv, c.hd)
        (bq, lq, sq), (bv, lv, sv) = token_maps(c, defect)
        if defect == "clamped_row_stored":                       # row M, filled with row M - 1's operands, goes out too
            rows = torch.cat([rows, rows[-1:]])
            bq, lq, sq = (torch.cat([t, torch.tensor([v], dtype=t.dtype)]) for t, v in ((bq, c.M // c.L), (lq, c.M % c.L), (sq, True)))
        flat = self.buffers()
        d = torch.arange(c.hd)[None, None, :]
        hq, hk = torch.arange(c.nh)[None, :, None], torch.arange(c.nkv)[None, :, None]
        bq, lq, bv, lv = (t[:, None, None] for t in (bq, lq, bv, lv))
        k_heads = c.nh if defect == "k_head_stride_nh" else c.nkv
        _scatter(flat["q"], (GUARD + ((bq * c.nh + hq) * c.L + lq) * c.hd + d)[sq], rows[:, :c.nh][sq])
        _scatter(flat["k"], (GUARD + ((bq * k_heads + hk) * c.dst_t + c.dpos0 + lq) * c.hd + d)[sq], rows[:, c.nh:][sq])
        _scatter(flat["v"], (GUARD + ((bv * c.nkv + hk) * c.hd + d) * c.dst_t + c.dpos0 + lv)[sv], vrows[sv])
        return flat


# defect -> the cases it exists on (tests/test_qkv_probe_cpu.py has what each one is)
DEFECTS = {
    "pair_half32": lambda c: not c.null and c.hd != 64,
    "pos_dpos0": lambda c: not c.null and c.dpos0 != c.past,
    "tab_div_ignored": lambda c: not c.null and c.tab_div > 1,
    "scale_keys": lambda c: c.prescale,
    "scale_after": lambda c: c.prescale and not c.null,
    "bias_half": lambda c: c.bias,
    "v_bias_by_token": lambda c: c.bias,
    "m_base_dropped": lambda c: 0 < c.rows_big < c.M,
    "k_head_stride_nh": lambda c: c.nh != c.nkv and c.B > 1,
    "v_odd_shift": lambda c: odd_runs(c) > 0,
    "v_wrap_once": lambda c: any(not torch.equal(a, b) for a, b in zip(token_maps(c)[1], token_maps(c, "v_wrap_once")[1])),
    "v_tail_dropped": lambda c: c.M % 8 != 0,
    "clamped_row_stored": lambda c: True,
    "drop_last_ktile": lambda c: True,
    "lda_as_k": lambda c: c.ld,
}


@lru_cache(maxsize=2)
def probe(case, family):
    """The probe of a case.  The conditions on the reference -- proj_probe's builder assertions, one value on >= 98 % of the judged
    elements -- hold at seed 0 for every case of a few thousand outputs; a smaller one takes the first seed at which they do, as
    proj_probe.probe() does.  Nothing here looks at a kernel's output."""
    small = case.M * case.N < 4096
    for seed in range(64 if small else 1):
        try:
            pr = QkvProbe(case, family, seed)
        except AssertionError:
            if not small or seed == 63:
                raise
            continue
        if not small or min(pr.unique_shares().values()) >= MIN_UNIQUE:
            break
    return pr
