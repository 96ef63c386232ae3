"""Probing inputs and an fp64 reference for the split-KV decode attention (p3v_attention_decode / p3v_attention_decode_q8).

Gaussian q / K / V cannot fail at long contexts: over n Gaussian keys the softmax is nearly flat, the output shrinks like
n^-1/2 and a kernel that loses a quarter of its keys stays inside `rtol 2^-6, atol 2e-2`.  The inputs built here keep the
output O(1) at any length and move it by many tolerances when one specific key is lost, leaks through a mask or is merged
with the wrong weight:

  * PLANTED KEYS.  A planted key of a kv head is zero except for the constant KEY_C on its own block of `w` dims (exact
    in bf16, and the row maximum of the int8 quantiser).  A rotated query is the constant `a` on the union of the blocks of
    the keys it attends to, so it scores `scale * w * KEY_C * a` on each of them and ~0 on every other planted key.  `a` is
    set so that one planted key weighs about e times the whole Gaussian background (K std 0.5, V std 1).  The kernel
    rotates q itself: `qkv` holds the inverse rotation of the wanted query (fp64, rounded to bf16).
  * POSITIONS.  Per batch row: the first and the last live key of every split that holds live keys, a key on each side of
    a 64-key tile edge inside a split, the first visible key (pad_len[b]), the last cached key (past - 1) and every new row.
    Cached positions alternate between the two kv heads; when one batch row cannot hold them all (more blocks than head
    dims: 128 splits) the batch rows in which a split is live share it between them (split s goes to the (s mod n)-th of its n rows).
  * CLASSES.  The queries (row r, head g of the kv group) of a kv head fall into `nq` classes, class (4 r + g) % nq, and a
    planted key belongs to one class.  With two or more live splits no key of split s is given to class s % nq: those
    queries see nothing but background there, their partial maximum m_s is far below the row maximum, and a merge that
    forgets the weight exp(m_s - m) is visible.
  * NEW ROWS.  Every new row's key has a block of its own.  Every query row looks for the key of the LAST new row; only the
    last row may see it, so a causal leak among the new rows shows in rows 0 .. L-2.  Row r also looks for the new rows
    r' <= r with r' = r mod 3.
  * DEAD REGION.  K rows and V^T columns at positions >= past (the kernel must overwrite [past, past + L) itself) and at
    positions < pad_len[b] hold POISON (1e4, the sign of the planted blocks; finite, as include/p3v.h requires): a leaked
    key takes the whole row instead of hiding in noise.  The int8 cache carries code 255 with scale POISON / 127.

The reference is plain fp64: rotate-half of the bf16 q / new K under the fp32 tables, rounded to bf16 as the cache stores
them; visibility pad_len[b] <= t <= past + i; softmax; P.V.  For the int8 cache it runs over the dequantised stored values,
the new rows quantise-dequantised.  Everything here is torch on the CPU.
"""
import math
from dataclasses import dataclass
from functools import lru_cache

import torch

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NH, NKV, HD = 8, 2, 96
GRP = NH // NKV
SCALE = HD ** -0.5
KEY_C = 16.0
POISON = 1.0e4
RTOL, ATOL = 2 ** -6, 2e-2
FULL_NH = 32                     # the heads of the full model, for model._split_plan


@dataclass(frozen=True)
class Case:
    kind: str                    # "bf16" | "q8"
    cap: int
    n_split: int
    past: int
    L: int
    B: int = 1
    pads: tuple = None
    dev_past: int = None         # None: host `past` alone; k: d_past on the device with the lower bound max(0, past - k) (0: bound 0)
    fused: bool = False          # merge_in_launch
    plan_B: int = 1              # batch at which model._split_plan yields n_split for this capacity
    plan_fused: bool = False     # ... and the merge form it picks

    @property
    def chunk(self):             # the launcher's rule: keys per split, a multiple of 64
        return (-(-self.cap // self.n_split) + 63) // 64 * 64

    @property
    def pad(self):
        return list(self.pads) if self.pads else [0] * self.B

    @property
    def lower_bound(self):
        return self.past if self.dev_past is None else (max(0, self.past - self.dev_past) if self.dev_past else 0)

    @property
    def kernel(self):
        """The kernel p3v_attention_decode(_q8) launches for (cap, n_split) (csrc/p3v_attention.hip), and the merge."""
        one64, one128 = self.n_split * 64 >= self.cap, self.cap % 128 == 0 and self.n_split * 128 >= self.cap
        if self.kind == "bf16":
            k = "k_attn_decode" if one64 else "k_attn_decode128" if one128 else "k_attn_decode_stream"
            return k + (" (merge in launch)" if self.fused else " + k_attn_combine2")
        if one128 and not one64:
            return "k_attn_decode128_q8" + (" (merge in launch)" if self.fused else " + k_attn_combine2")
        if one64 and self.n_split <= 16:
            return "k_attn_decode_q8s" + (" (merge in launch)" if self.fused else " + k_attn_combine2")
        return "k_attn_decode_q8 + k_attn_combine2"

    @property
    def id(self):
        s = f"{self.kind}-cap{self.cap}-s{self.n_split}-past{self.past}-L{self.L}-B{self.B}"
        s += "-pads" if self.pads else ""
        s += "-host" if self.dev_past is None else f"-dpast{self.dev_past}"
        return s + ("-inlaunch" if self.fused else "-mergelaunch")


def _rows(kind, cap, n_split, variants, **kw):
    return [Case(kind, cap, n_split, *v[:2], **{**kw, **(v[2] if len(v) > 2 else {})}) for v in variants]


RAG16 = (0, 3, 150, 290, 17, 64, 63, 65, 128, 127, 1, 200, 129, 250, 0, 301)        # ragged pad_len of the batched plan
_DP40, _DP0, _IN, _OUT = {"dev_past": 40}, {"dev_past": 0}, {"fused": True}, {"fused": False}

CASES = (
    # ---- bf16 cache.  33280 / 24: chunk 1408 = 22 tiles, split 23 holds 896 keys (config 3)
    _rows("bf16", 33280, 24, [(33270, 1), (33255, 16, _DP40), (300, 1, _DP0), (300, 5), (12 * 1408 - 2, 5, _DP0), (12 * 1408, 1),
                              (12 * 1408 - 1, 1, _DP40), (33000, 5, {"B": 3, "pads": (0, 150, 1500), **_DP40}),
                              (33270, 5, _IN)])
    # 8256 / 24: chunk 384 = 6 tiles, splits 22 and 23 start beyond the capacity
    + _rows("bf16", 8256, 24, [(8250, 1), (8235, 16, _DP40), (300, 1, _DP0), (10 * 384 - 2, 5), (10 * 384, 1, _DP0), (10 * 384 - 1, 1),
                               (8200, 5, {"B": 3, "pads": (0, 150, 500), **_DP40}), (8250, 5, {**_IN, **_DP40})])
    # 640 / 2 at B = 16: the batched plan, stream kernel with the in-launch merge
    + _rows("bf16", 640, 2, [(630, 1, _IN), (620, 5, {**_IN, **_DP40}), (318, 5, {**_IN, **_DP0}), (320, 1), (319, 16, _DP40)],
            B=16, pads=RAG16, plan_B=16, plan_fused=True)
    # 6144 / 48: one 128-key tile per split, the largest in-launch merge
    + _rows("bf16", 6144, 48, [(6138, 1, _IN), (6120, 16, {**_IN, **_DP40}), (300, 5, {**_IN, **_DP0}), (24 * 128 - 2, 5), (24 * 128, 1, {**_IN, **_DP0}),
                               (24 * 128 - 1, 1, _DP40), (6100, 5, {"B": 3, "pads": (0, 150, 300), **_IN, **_DP40})], plan_fused=True)
    # 8192 / 128: one 64-key tile per split, 128 partials through the merge launch (three batch rows share the 256 split edges)
    + _rows("bf16", 8192, 128, [(8186, 1), (8170, 16, _DP40), (300, 5, _DP0), (64 * 64 - 2, 5), (64 * 64, 1, _DP0), (64 * 64 - 1, 1),
                                (8100, 5, {"pads": (0, 150, 300), **_DP40})], B=3)
    # ---- int8 cache.  33280 / 40: chunk 832 = 13 tiles (config 5 at 32k)
    + _rows("q8", 33280, 40, [(33270, 1), (33250, 16, _DP40), (300, 1, _DP0), (20 * 832 - 2, 5), (20 * 832, 1, _DP0), (20 * 832 - 1, 1),
                              (33000, 5, {"B": 3, "pads": (0, 150, 900), **_DP40})])
    # 8256 / 40: chunk 256, splits 33 .. 39 hold no keys
    + _rows("q8", 8256, 40, [(8250, 1), (8230, 16, _DP40), (300, 5, _DP0), (16 * 256 - 2, 5), (16 * 256, 1, _DP0), (16 * 256 - 1, 1),
                             (8200, 5, {"B": 3, "pads": (0, 150, 300), **_DP40})])
    # 2688 / 21: one 128-key tile per split at config 5's own length, both merge forms
    + _rows("q8", 2688, 21, [(2680, 1, _IN), (2665, 16, _DP40), (300, 5, {**_IN, **_DP0}), (10 * 128 - 2, 5, _IN), (10 * 128, 1, _DP0),
                             (10 * 128 - 1, 1, _IN), (2600, 5, {"B": 3, "pads": (0, 150, 300), **_IN, **_DP40}),
                             (2600, 5, {"B": 3, "pads": (0, 150, 300), **_DP40})], plan_fused=True)
    # 1024 / 16: the single-tile four-wave kernel at its limit, both merge forms
    + _rows("q8", 1024, 16, [(1018, 1, _IN), (1000, 16, _DP40), (300, 5, {**_IN, **_DP0}), (8 * 64 - 2, 5), (8 * 64, 1, {**_IN, **_DP0}),
                             (8 * 64 - 1, 1), (1000, 5, {"B": 3, "pads": (0, 150, 300), **_IN, **_DP40})], plan_fused=True)
    # 1088 / 17: one tile per split, but 17 of them: the single-wave kernel
    + _rows("q8", 1088, 17, [(1080, 1), (1060, 16, _DP40), (300, 5, _DP0), (8 * 64 - 2, 5), (8 * 64, 1), (1050, 5, {"B": 3, "pads": (0, 150, 300), **_DP40})],
            plan_fused=True)
    # 640 / 2 at B = 16 (the model's plan from B = 20 on), and 640 / 3: its plan at B = 16 (chunk 256, the last split half full)
    + _rows("q8", 640, 2, [(630, 1), (318, 5, _DP0), (320, 16, _DP40)], B=16, pads=RAG16, plan_B=20, plan_fused=True)
    + _rows("q8", 640, 3, [(630, 5, _DP40)], B=16, pads=RAG16, plan_B=16, plan_fused=True)
)
assert len({c.id for c in CASES}) == len(CASES)


def bf16_round(x):
    return x.to(F32).to(BF16)


def rope_tables(past, L):
    """cos / sin [L, HD / 2] fp32 of positions past .. past + L - 1 (plain RoPE, base 10000)."""
    inv = 10000.0 ** (-torch.arange(0, HD, 2, dtype=F64) / HD)
    ang = (past + torch.arange(L, dtype=F64))[:, None] * inv[None, :]
    return torch.cos(ang).to(F32), torch.sin(ang).to(F32)


def rotate(x, cos, sin):
    """rotate-half in fp64: x [..., L, HD] (any dtype), cos / sin [L, HD / 2] fp32."""
    x, c, s = x.to(F64), cos.to(F64), sin.to(F64)
    x1, x2 = x[..., :HD // 2], x[..., HD // 2:]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)


def unrotate(y, cos, sin):
    """The inverse of `rotate` (the tables are a pure rotation), fp64."""
    y, c, s = y.to(F64), cos.to(F64), sin.to(F64)
    y1, y2 = y[..., :HD // 2], y[..., HD // 2:]
    return torch.cat([y1 * c + y2 * s, y2 * c - y1 * s], dim=-1)


def quantize_rows(x):
    """The int8 cache's quantiser on rows [..., hd]: u = round(x / s) + 128, s = amax / 127 (fp32). -> codes (uint8), scales."""
    x = x.to(F32)
    sc = x.abs().amax(-1) / 127
    q = torch.round(x / sc[..., None]).clamp(-127, 127) + 128
    return q.to(torch.uint8), sc


def dequant(codes, sc):
    return (codes.to(F64) - 128.0) * sc.to(F64)[..., None]


def live_range(case, b, s):
    """Live keys of split s in batch row b: [lo, hi) (empty when lo >= hi)."""
    return max(s * case.chunk, case.pad[b]), min((s + 1) * case.chunk, case.past + case.L, case.cap)


def required_positions(case, b, every_split=False):
    """The positions the planted keys of a case must cover in batch row b (module docstring); every_split: without the
    sharing of the splits between the batch rows."""
    past, L, chunk, lo = case.past, case.L, case.chunk, case.pad[b]
    live = [s for s in range(case.n_split) if live_range(case, b, s)[0] < live_range(case, b, s)[1]]
    share = not every_split and case.B > 1 and 2 * len(live) > 88
    req = set()
    for s in live:
        rows = [r for r in range(case.B) if live_range(case, r, s)[0] < live_range(case, r, s)[1]]
        if not share or rows[s % len(rows)] == b:
            a, z = live_range(case, b, s)
            req |= {a, z - 1}
    edges = [t for t in range(64, past, 64) if t % chunk and t - 1 >= lo]            # a tile edge inside a split, both sides cached
    if edges:
        req |= {edges[0] - 1, edges[0]}
    req |= {lo, past - 1} | set(range(past, past + L))
    return sorted(req), live


@dataclass
class Planted:
    b: int
    kvh: int
    t: int
    cls: int          # -1: a new row (looked for by rows, not by a class)
    blk: int


class Probe:
    """The inputs of one case and their fp64 reference (module docstring)."""

    def __init__(self, case, seed=0):
        self.case = c = case
        B, L, past, cap = c.B, c.L, c.past, c.cap
        assert all(0 <= p < past for p in c.pad) and past + L <= cap and cap % 64 == 0
        gen = torch.Generator().manual_seed(1234 + seed)
        self.cos, self.sin = rope_tables(past, L)
        k = bf16_round(torch.randn((B, NKV, cap, HD), generator=gen) * 0.5)
        v = bf16_round(torch.randn((B, NKV, cap, HD), generator=gen))
        x = bf16_round(torch.randn((B, L, NH + 2 * NKV, HD), generator=gen))       # the V part stays Gaussian
        self.planted, self.live = [], []
        s_t = math.log(past + L) + 1.0                                               # a planted key ~ e x the whole background
        q_want = torch.zeros((B, NH, L, HD), dtype=F64)
        k_want = torch.zeros((B, NKV, L, HD), dtype=F64)
        for b in range(B):
            req, live = required_positions(c, b)
            self.live.append(live)
            cached = [t for t in req if t < past]
            blind = len(live) >= 2
            for kvh in range(NKV):
                mine = cached[kvh::2]
                nq = min(4 * L, max(3, -(-len(mine) // 8)))
                is_blind = lambda cls, t: blind and (t // c.chunk) % nq == cls
                keys, cnt, n = [], [0] * nq, 0
                for t in mine:                                                       # no key of split s for class s % nq
                    n += is_blind(n % nq, t)
                    keys.append((t, n % nq))
                    cnt[n % nq] += 1
                    n += 1
                used = set(cached)
                for cls in range(nq):                                                # two cached keys per class, where it may have any
                    for s in live:
                        a, z = live_range(c, b, s)
                        if cnt[cls] >= 2:
                            break
                        if is_blind(cls, a):
                            continue
                        for t in range(a + (min(z, past) - a) // 2, min(z, past)):
                            if t not in used:
                                used.add(t), keys.append((t, cls))
                                cnt[cls] += 1
                                break
                nb = len(keys) + L                                                   # one block per planted key, new rows included
                assert nb <= HD, f"{c.id}: {nb} planted keys on one kv head"
                w = min(12, HD // nb)
                a_q = s_t / (SCALE * w * KEY_C)
                blk_of = lambda i: slice(i * w, (i + 1) * w)
                for i, (t, cls) in enumerate(keys):
                    k[b, kvh, t] = 0
                    k[b, kvh, t, blk_of(i)] = KEY_C
                    self.planted.append(Planted(b, kvh, t, cls, i))
                for r in range(L):
                    k_want[b, kvh, r, blk_of(len(keys) + r)] = KEY_C
                    self.planted.append(Planted(b, kvh, past + r, -1, len(keys) + r))
                wanted = set()
                for r in range(L):
                    # row r looks for the cached keys of its class, the new rows r' <= r of its residue mod 3 and the LAST new
                    # row (which only the last row may see) -- but for nothing in a split its class is blind to.  A query that
                    # would then see no planted key at all (its row lies in the only split it could look at) takes the next class
                    for g in range(GRP):
                        for cls in [(4 * r + g + d) % nq for d in range(nq)]:
                            blocks = [j for j, (t, kc) in enumerate(keys) if kc == cls]
                            blocks += [len(keys) + r2 for r2 in range(r + 1) if r2 % 3 == r % 3 and not is_blind(cls, past + r2)]
                            if blocks:
                                break
                        assert blocks, (c.id, b, kvh, r, g)
                        if not is_blind(cls, past + L - 1):
                            blocks.append(len(keys) + L - 1)
                        wanted |= {j for j in blocks if j < len(keys) + r + 1}
                        for j in blocks:
                            q_want[b, kvh * GRP + g, r, blk_of(j)] = a_q
                assert len(wanted) == nb, (c.id, b, kvh, sorted(set(range(nb)) - wanted))      # every planted key has a query that sees it
            k[b, :, :c.pad[b]] = POISON
            v[b, :, :c.pad[b]] = POISON
        k[:, :, past:] = POISON
        v[:, :, past:] = POISON
        x[:, :, :NH] = bf16_round(unrotate(q_want, self.cos, self.sin)).transpose(1, 2)
        x[:, :, NH:NH + NKV] = bf16_round(unrotate(k_want, self.cos, self.sin)).transpose(1, 2)
        self.qkv = x.reshape(B * L, (NH + 2 * NKV) * HD).contiguous()
        self.k, self.vt = k, v.transpose(2, 3).contiguous()                          # bf16 K [B, nkv, cap, hd], V^T [B, nkv, hd, cap]
        # what the step stores and attends on
        self.q_rot = bf16_round(rotate(x[:, :, :NH].transpose(1, 2), self.cos, self.sin))         # [B, nh, L, hd]
        self.k_new = bf16_round(rotate(x[:, :, NH:NH + NKV].transpose(1, 2), self.cos, self.sin))  # [B, nkv, L, hd]
        self.v_new = x[:, :, NH + NKV:].transpose(1, 2).contiguous()
        if c.kind == "q8":
            self.k8, self.ks = quantize_rows(k)
            v8, self.vs = quantize_rows(v)
            for codes, sc in ((self.k8, self.ks), (v8, self.vs)):                    # poison the codes and scales to the same effect
                for b in range(B):
                    codes[b, :, :c.pad[b]], sc[b, :, :c.pad[b]] = 255, POISON / 127
                codes[:, :, past:], sc[:, :, past:] = 255, POISON / 127
            self.v8t = v8.transpose(2, 3).contiguous()
            self.k8_new, self.ks_new = quantize_rows(self.k_new)
            self.v8_new, self.vs_new = quantize_rows(self.v_new)
            kd, vd = dequant(self.k8, self.ks), dequant(v8, self.vs)
            kd[:, :, past:past + L], vd[:, :, past:past + L] = dequant(self.k8_new, self.ks_new), dequant(self.v8_new, self.vs_new)
            vs_all = self.vs.clone()
            vs_all[:, :, past:past + L] = self.vs_new
            self.vs_all = vs_all[:, :, :min(cap, past + L + 1)].to(F64)
        else:
            kd, vd = k.to(F64), v.to(F64)
            kd[:, :, past:past + L], vd[:, :, past:past + L] = self.k_new.to(F64), self.v_new.to(F64)
        T = min(cap, past + L + 1)                                                    # one dead key for the mutants
        self.kd, self.vd = kd[:, :, :T], vd[:, :, :T]
        self.scores = SCALE * torch.einsum("bkgld,bktd->bkglt", self.q_rot.to(F64).view(B, NKV, GRP, L, HD), self.kd).reshape(B, NH, L, T)
        self.ref = self.attend(self.visible())

    # ---- the reference and its mutants
    def visible(self):
        """[B, L, T] bool: pad_len[b] <= t <= past + i."""
        c, T = self.case, self.kd.shape[2]
        t = torch.arange(T)[None, None, :]
        return (t >= torch.tensor(c.pad)[:, None, None]) & (t <= (c.past + torch.arange(c.L))[None, :, None])

    def attend(self, vis):
        """softmax over the visible keys, then P.V -> [B, L, nh * hd] fp64."""
        c = self.case
        s = self.scores.masked_fill(~vis[:, None], -math.inf)
        p = torch.softmax(s, dim=-1)
        out = torch.einsum("bkglt,bktd->bkgld", p.view(c.B, NKV, GRP, c.L, -1), self.vd).reshape(c.B, NH, c.L, HD)
        return out.transpose(1, 2).reshape(c.B, c.L, NH * HD)

    def weights(self):
        return torch.softmax(self.scores.masked_fill(~self.visible()[:, None], -math.inf), dim=-1)      # [B, nh, L, T]

    def without_key(self, p):
        """The reference with planted key `p` removed from its kv head: rows of the heads of that group, [GRP, L, hd]."""
        c = self.case
        h = slice(p.kvh * GRP, (p.kvh + 1) * GRP)
        if not hasattr(self, "_w"):
            self._w = self.weights()
        w = self._w[p.b, h, :, p.t][..., None]                                        # [GRP, L, 1]
        o = self.ref[p.b].view(c.L, NH, HD).transpose(0, 1)[h]
        return (o - w * self.vd[p.b, p.kvh, p.t]) / (1 - w), o

    def split_partials(self, scores=None, p_f16=False):
        """fp64 partials (m, l, O) of every split under the launcher's chunk rule: m [B, nh, L, S], l likewise, O [.., S, hd].
        p_f16 (int8 cache): P times the key's V scale is rounded to fp16 before it meets the V codes, as the int8 kernels do."""
        c, T = self.case, self.kd.shape[2]
        s = (self.scores if scores is None else scores).masked_fill(~self.visible()[:, None], -math.inf)
        ms, ls, os_ = [], [], []
        for i in range(c.n_split):
            lo, hi = min(i * c.chunk, T), min((i + 1) * c.chunk, T)
            if lo >= hi or bool((s[..., lo:hi] == -math.inf).all()):
                ms.append(torch.full(s.shape[:3], -math.inf, dtype=F64))
                ls.append(torch.zeros(s.shape[:3], dtype=F64))
                os_.append(torch.zeros(s.shape[:3] + (HD,), dtype=F64))
                continue
            m = s[..., lo:hi].amax(-1)
            e = torch.exp(s[..., lo:hi] - torch.where(m == -math.inf, torch.zeros_like(m), m)[..., None])
            e = torch.where(s[..., lo:hi] == -math.inf, torch.zeros_like(e), e)
            ms.append(m), ls.append(e.sum(-1))
            if p_f16:
                vs = self.vs_all[:, :, None, None, lo:hi]
                pv = (e.view(c.B, NKV, GRP, c.L, -1) * vs).to(F32).to(torch.float16).to(F64)
                os_.append(torch.einsum("bkglt,bktd->bkgld", pv, self.vd[:, :, lo:hi] / self.vs_all[:, :, lo:hi, None]).reshape(c.B, NH, c.L, HD))
                continue
            os_.append(torch.einsum("bkglt,bktd->bkgld", e.view(c.B, NKV, GRP, c.L, -1), self.vd[:, :, lo:hi]).reshape(c.B, NH, c.L, HD))
        return torch.stack(ms, -1), torch.stack(ls, -1), torch.stack(os_, -2)

    def merge(self, m, l, O, unit=None):
        """Merge of the split partials; unit = s: split s merged with weight 1 instead of exp(m_s - m) (wherever it holds keys)."""
        c = self.case
        w = torch.exp(m - m.amax(-1, keepdim=True))
        if unit is not None:
            w[..., unit] = torch.where(l[..., unit] > 0, torch.ones_like(w[..., unit]), w[..., unit])
        out = (w[..., None] * O).sum(-2) / (w * l).sum(-1)[..., None]
        return out.transpose(1, 2).reshape(c.B, c.L, NH * HD)


def restated(pr):
    """The int8 kernels' documented roundings restated in fp64 (csrc/p3v_attention.hip, "Q and P are rounded to fp16"): the rotated
    query is rounded to fp16 -- 11 significant bits, from the exact rotation, where the plain reference rounds it to bf16 -- and
    P times the V scale is rounded to fp16 per split; partials and merge stay fp64 (the kernel's are fp32, its exp2 runs on
    scale * log2 e: both ~1e-6 relative, not restated).  -> [B, L, nh * hd] fp64, to be compared with pr.ref."""
    c = pr.case
    x = pr.qkv.view(c.B, c.L, NH + 2 * NKV, HD)
    q16 = rotate(x[:, :, :NH].transpose(1, 2), pr.cos, pr.sin).to(F32).to(torch.float16).to(F64)
    scores = SCALE * torch.einsum("bkgld,bktd->bkglt", q16.view(c.B, NKV, GRP, c.L, HD), pr.kd).reshape(c.B, NH, c.L, -1)
    return pr.merge(*pr.split_partials(scores, p_f16=True))


def worst_ratio(got, ref, rtol=RTOL, atol=ATOL):
    """max |got - ref| / (atol + rtol |ref|): > 1 is what close(..., rtol, atol) rejects."""
    got, ref = got.to(F64), ref.to(F64)
    return float(((got - ref).abs() / (atol + rtol * ref.abs())).max())


@lru_cache(maxsize=2)
def probe(case):
    return Probe(case)


def launch(ops, pr, device="cuda"):
    """Run the case of `pr` through ops.attention_decode / ops.attention_decode_q8 (twice on the same workspace for the
    in-launch merge) -> dict of CPU tensors: out (and out2), the caches after the launch, the workspace words."""
    c = pr.case
    B, L = c.B, c.L
    dev = lambda t: t.to(device)
    cos, sin = (dev(t[None].expand(B, L, HD // 2).contiguous()) for t in (pr.cos, pr.sin))
    pad = dev(torch.tensor(c.pad, dtype=torch.int32)) if c.pads else None
    d_past = dev(torch.tensor([c.past], dtype=torch.int32)) if c.dev_past is not None else None
    ws = ops.attention_ws(B, L, NH, HD, c.n_split, device)
    qkv, res = dev(pr.qkv), {}
    caches = [dev(t) for t in ((pr.k8, pr.v8t, pr.ks, pr.vs) if c.kind == "q8" else (pr.k, pr.vt))]
    for name in ("out", "out2") if c.fused else ("out",):
        out = torch.full((B, L, NH * HD), float("nan"), dtype=BF16, device=device)
        if c.kind == "q8":
            ops.attention_decode_q8(qkv, cos, sin, L, *caches, out, B, L, NH, NKV, HD, SCALE, c.lower_bound, c.cap, ws, c.n_split,
                                    pad_len=pad, d_past=d_past, merge_in_launch=c.fused)
        else:
            ops.attention_decode(qkv, cos, sin, L, *caches, out, B, L, NH, NKV, HD, SCALE, c.lower_bound, c.cap, ws, c.n_split,
                                 pad_len=pad, d_past=d_past, merge_in_launch=c.fused)
        res[name] = out.cpu()
    res["ws"] = ws.view(torch.int32).cpu()
    res["caches"] = [t.cpu() for t in caches]
    return res
