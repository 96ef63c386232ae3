"""Probing inputs and an fp64 reference for the shared-prefix decode attention (p3v_attention_decode_family).

The scheme is tests/attn_probe.py's (planted keys of constant KEY_C on a block of head dims, queries that are a constant on the
blocks they look for, POISON in every dead position), laid out for FAMILIES: groups of batch rows whose caches are identical in
[pad, share_end) and differ from share_end on.

  * PREFIX KEYS, common to a group, on both kv heads, one block each: the first visible key, both sides of every split edge at or
    below share_end, both sides of the first 64-key tile edge inside a split, and share_end - 1.
  * PRIVATE KEYS of member j (its j-th row): share_end, past - 1 and both sides of the first tile edge and of the first split edge
    inside (share_end, past), where the suffix holds them, and the new key at `past`.  They carry the blocks j and (j + 1) % n.
  * QUERIES.  Head g of member j looks for block j -- its own private keys, and NOT its neighbour's: those carry j + 1 and j + 2 --
    and for the prefix keys i with (i + rho_j + g) % 3 != 0, rho_j = j % 3 (1 for the last member where that would repeat member
    0's): every prefix key is common to two thirds of the queries, of two consecutive prefix keys (the two ends of a split) a
    query sees at least one, and no two neighbours look for the same keys of a split.  The private keys of member j - 1 carry
    block j too: leaked into member j's row they weigh as much as its own.
  * One planted key weighs about e times the whole Gaussian background (K std 0.5, V std 1), as in attn_probe.
  * DEAD POSITIONS, below a row's pad and at or beyond `past` (the kernel writes `past` itself), hold POISON in K and V^T.

The reference is plain fp64, per row over that row's own copy, with visibility pad <= t <= past.  Everything here is torch on the
CPU; `launch` runs a case through ops.attention_decode_family.
"""
import math
from dataclasses import dataclass
from functools import lru_cache

import torch

from attn_probe import ATOL, HD, KEY_C, NH, NKV, POISON, RTOL, SCALE, bf16_round, rope_tables, rotate, unrotate, worst_ratio  # noqa: F401

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
GRP = NH // NKV
FAMILY_MAX, FAMILY_INTS = 16, 18


@dataclass(frozen=True)
class FamCase:
    cap: int
    n_split: int
    share_end: int
    past: int
    groups: tuple                # tuple of row tuples, the leader first; a group of one row is a single row
    pads: tuple = None           # per row
    dev_past: int = None         # None: host `past`; 0: d_past on the device with the bound 0; k: with the bound past - k
    twice: bool = False          # two consecutive launches on one workspace

    @property
    def B(self):
        return sum(len(g) for g in self.groups)

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
    def dead_end(self):          # a follower's columns [0, dead_end) are not read
        return self.share_end // self.chunk * self.chunk

    @property
    def id(self):
        s = f"cap{self.cap}-s{self.n_split}-se{self.share_end}-past{self.past}-" + "+".join(str(len(g)) for g in self.groups)
        s += f"-pad{max(self.pads)}" if self.pads else ""
        s += "-host" if self.dev_past is None else f"-dpast{self.dev_past}"
        return s + ("-twice" if self.twice else "")


def table(case, shared=True):
    """The family table [B, 18] int32 of a case: {lead, share_end, member[16]} per row; shared=False: every row a single row."""
    t = torch.full((case.B, FAMILY_INTS), -1, dtype=torch.int32)
    for g in case.groups:
        for r in g:
            if shared and len(g) > 1:
                t[r, 0], t[r, 1] = g[0], case.share_end
            else:
                t[r, 0], t[r, 1], t[r, 2] = r, 0, r
        if shared and len(g) > 1:
            t[g[0], 2:2 + len(g)] = torch.tensor(g, dtype=torch.int32)
    return t


def shared_splits(case, g):
    """The splits the kernel shares for group g."""
    return [s for s in range(case.n_split) if len(g) > 1 and (s + 1) * case.chunk <= case.share_end]


def prefix_positions(case, g):
    c, se = case.chunk, case.share_end
    lo = max(case.pad[r] for r in g)
    req = {lo, se - 1}
    for e in range(c, se + 1, c):
        req |= {e - 1, e}
    edges = [t for t in range(64, se, 64) if t % c and t - 1 >= lo]
    if edges:
        req |= {edges[0] - 1, edges[0]}
    return sorted(t for t in req if lo <= t < se)


def private_positions(case):
    c, se, past = case.chunk, case.share_end, case.past
    req = {se, past - 1}
    for step in (64, c):
        edges = [t for t in range(se // step * step + step, past, step) if t - 1 >= se]
        if edges:
            req |= {edges[0] - 1, edges[0]}
    return sorted(t for t in req if se <= t < past)


class FamProbe:
    def __init__(self, case, seed=0):
        self.case = c = case
        B, cap, past, se = c.B, c.cap, c.past, c.share_end
        assert sorted(r for g in c.groups for r in g) == list(range(B)) and all(len(g) <= FAMILY_MAX for g in c.groups)
        assert all(0 <= p < se for p in c.pad) and se <= past < cap and cap % 64 == 0
        gen = torch.Generator().manual_seed(4321 + seed)
        self.cos, self.sin = rope_tables(past, 1)
        k = torch.empty((B, NKV, cap, HD), dtype=BF16)
        v = torch.empty((B, NKV, cap, HD), dtype=BF16)
        x = bf16_round(torch.randn((B, 1, NH + 2 * NKV, HD), generator=gen))         # the V part stays Gaussian
        s_t = math.log(past + 1) + 1.0
        q_want = torch.zeros((B, NH, 1, HD), dtype=F64)
        k_want = torch.zeros((B, NKV, 1, HD), dtype=F64)
        self.prefix, self.private = {}, {}
        for g in c.groups:
            n = len(g)
            base_k = bf16_round(torch.randn((NKV, cap, HD), generator=gen) * 0.5)
            base_v = bf16_round(torch.randn((NKV, cap, HD), generator=gen))
            pre, prv = prefix_positions(c, g), private_positions(c)
            nb = n + len(pre)                                                        # blocks 0 .. n - 1: the members'; then the prefix keys'
            assert nb <= HD // 2, (c.id, nb)
            w = min(12, HD // nb)
            a_q = s_t / (SCALE * w * KEY_C)
            blk = lambda i: slice(i * w, (i + 1) * w)
            for i, t in enumerate(pre):
                base_k[:, t] = 0
                base_k[:, t, blk(n + i)] = KEY_C
            for j, r in enumerate(g):
                k[r], v[r] = base_k, base_v
                k[r, :, se:] = bf16_round(torch.randn((NKV, cap - se, HD), generator=gen) * 0.5)
                v[r, :, se:] = bf16_round(torch.randn((NKV, cap - se, HD), generator=gen))
                for t in prv:
                    k[r, :, t] = 0
                    k[r, :, t, blk(j)] = KEY_C
                    k[r, :, t, blk((j + 1) % n)] = KEY_C
                k_want[r, :, 0, blk(j)] = KEY_C
                k_want[r, :, 0, blk((j + 1) % n)] = KEY_C
                rho = 1 if (j == n - 1 and n % 3 == 1 and n > 1) else j % 3              # never the residue of a neighbour, the wrap included
                for h in range(NH):
                    q_want[r, h, 0, blk(j)] = a_q
                    for i in range(len(pre)):
                        if (i + rho + h % GRP) % 3:
                            q_want[r, h, 0, blk(n + i)] = a_q
                self.prefix[r], self.private[r] = pre, prv + [past]
        self.k_clean, self.v_clean = k.clone(), v.clone()
        for b in range(B):
            k[b, :, :c.pad[b]] = POISON
            v[b, :, :c.pad[b]] = POISON
        k[:, :, past:] = POISON
        v[:, :, past:] = POISON
        x[:, :, :NH] = bf16_round(unrotate(q_want, self.cos, self.sin)).transpose(1, 2)
        x[:, :, NH:NH + NKV] = bf16_round(unrotate(k_want, self.cos, self.sin)).transpose(1, 2)
        self.qkv = x.reshape(B, (NH + 2 * NKV) * HD).contiguous()
        self.k, self.vt = k, v.transpose(2, 3).contiguous()                          # bf16 K [B, nkv, cap, hd], V^T [B, nkv, hd, cap]
        self.q_rot = bf16_round(rotate(x[:, :, :NH].transpose(1, 2), self.cos, self.sin))[:, :, 0]          # [B, nh, hd]
        self.k_new = bf16_round(rotate(x[:, :, NH:NH + NKV].transpose(1, 2), self.cos, self.sin))[:, :, 0]  # [B, nkv, hd]
        self.v_new = x[:, 0, NH + NKV:].contiguous()                                                         # [B, nkv, hd]
        T = past + 1
        self.kd, self.vd = self.k_clean[:, :, :T].to(F64), self.v_clean[:, :, :T].to(F64)
        self.kd[:, :, past], self.vd[:, :, past] = self.k_new.to(F64), self.v_new.to(F64)
        self.ref = self.attend()

    # ---- the reference and its mutants
    def scores(self, q_of=None, k_of=None):
        """[B, nh, T] fp64: row b's scores with the query of row q_of[b] over the keys of row k_of[b]."""
        B = self.case.B
        q = self.q_rot.to(F64)[list(q_of) if q_of is not None else slice(None)]
        kd = self.kd[list(k_of) if k_of is not None else slice(None)]
        return SCALE * torch.einsum("bkgd,bktd->bkgt", q.view(B, NKV, GRP, HD), kd).reshape(B, NH, -1)

    def visible(self):
        t = torch.arange(self.case.past + 1)[None, :]
        return t >= torch.tensor(self.case.pad)[:, None]                             # [B, T]; t <= past by construction

    def attend(self, vis=None, s=None, extra=None):
        """softmax over the visible keys, then P.V -> [B, nh * hd] fp64.  extra: (scores [B, nh, E], values [B, nkv, E, hd]) of
        further keys every row sees."""
        c = self.case
        vis = self.visible() if vis is None else vis
        s = (self.scores() if s is None else s).masked_fill(~vis[:, None], -math.inf)
        vd = self.vd
        if extra is not None:
            s, vd = torch.cat([s, extra[0]], -1), torch.cat([vd, extra[1]], 2)
        p = torch.softmax(s, dim=-1)
        return torch.einsum("bkgt,bktd->bkgd", p.view(c.B, NKV, GRP, -1), vd).reshape(c.B, NH * HD)

    def partials(self):
        """fp64 partials of every split under the launcher's chunk rule: m, l [B, nh, S], O [B, nh, S, hd]."""
        c, T = self.case, self.case.past + 1
        s = self.scores().masked_fill(~self.visible()[:, None], -math.inf)
        ms, ls, os_ = [], [], []
        for i in range(c.n_split):
            lo, hi = min(i * c.chunk, T), min((i + 1) * c.chunk, T)
            if lo >= hi or bool((s[..., lo:hi] == -math.inf).all()):
                ms.append(torch.full(s.shape[:2], -math.inf, dtype=F64))
                ls.append(torch.zeros(s.shape[:2], dtype=F64))
                os_.append(torch.zeros(s.shape[:2] + (HD,), dtype=F64))
                continue
            m = s[..., lo:hi].amax(-1)
            e = torch.exp(s[..., lo:hi] - torch.where(m == -math.inf, torch.zeros_like(m), m)[..., None])
            e = torch.where(s[..., lo:hi] == -math.inf, torch.zeros_like(e), e)
            ms.append(m), ls.append(e.sum(-1))
            os_.append(torch.einsum("bkgt,bktd->bkgd", e.view(c.B, NKV, GRP, -1), self.vd[:, :, lo:hi]).reshape(c.B, NH, HD))
        return torch.stack(ms, -1), torch.stack(ls, -1), torch.stack(os_, -2)

    def merge(self, m, l, O):
        mx = m.amax(-1, keepdim=True)
        w = torch.exp(m - torch.where(mx == -math.inf, torch.zeros_like(mx), mx))
        w = torch.where(m == -math.inf, torch.zeros_like(w), w)
        return ((w[..., None] * O).sum(-2) / (w * l).sum(-1)[..., None]).reshape(self.case.B, NH * HD)

    def live_shared(self, g):
        """The shared splits of group g in which every member sees a key."""
        return [s for s in shared_splits(self.case, g) if (s + 1) * self.case.chunk > max(self.case.pad[r] for r in g)]


@lru_cache(maxsize=4)
def probe(case):
    return FamProbe(case)


def launch(ops, pr, shared=True, poison_followers=False, device="cuda"):
    """Run the case of `pr` through ops.attention_decode_family (twice on one workspace for case.twice) -> dict of CPU tensors:
    out (and out2), the caches before and after.  poison_followers: columns [0, dead_end) of every follower's K and V^T hold
    POISON."""
    c = pr.case
    B = c.B
    dev = lambda t: t.to(device)
    cos, sin = (dev(t[None].expand(B, 1, HD // 2).contiguous()) for t in (pr.cos, pr.sin))
    pad = dev(torch.tensor(c.pad, dtype=torch.int32)) if c.pads else None
    d_past = dev(torch.tensor([c.past], dtype=torch.int32)) if c.dev_past is not None else None
    ws = ops.attention_ws(B, 1, NH, HD, c.n_split, device)
    k, vt = pr.k.clone(), pr.vt.clone()
    if poison_followers:
        for g in c.groups:
            for r in g[1:]:
                k[r, :, :c.dead_end] = POISON
                vt[r, :, :, :c.dead_end] = POISON
    tab = table(c, shared)
    res = {"k_in": k, "vt_in": vt}
    qkv, kd, vd, tab_d = dev(pr.qkv), dev(k), dev(vt), dev(tab)
    for name in ("out", "out2") if c.twice else ("out",):
        out = torch.full((B, 1, NH * HD), float("nan"), dtype=BF16, device=device)
        ops.attention_decode_family(qkv, cos, sin, 1, kd, vd, out, B, NH, NKV, HD, SCALE, c.lower_bound, c.cap, ws, c.n_split, tab_d,
                                    family_host=tab, pad_len=pad, d_past=d_past)
        res[name] = out.cpu().view(B, NH * HD)
    res["ws"] = ws.view(torch.int32).cpu()
    res["k"], res["vt"] = kd.cpu(), vd.cpu()
    return res


def _c(cap, n_split, se, past, groups, **kw):
    return FamCase(cap, n_split, se, past, groups, **kw)


_PAIR, _F16 = ((0, 1),), (tuple(range(16)),)
_MIX8 = ((5, 2, 7), (3, 0, 6), (1,), (4,))          # two families of non-adjacent rows led by rows 5 and 3, two single rows
CASES = (
    # capacity 640 / 10 splits: chunk 64, one tile per split
    _c(640, 10, 63, 63, _PAIR),                                   # nothing shared; the first step after the fork
    _c(640, 10, 64, 64, _PAIR, dev_past=0),
    _c(640, 10, 129, 129, _PAIR, pads=(17, 17)),
    _c(640, 10, 129, 199, _PAIR, pads=(17, 40)),                  # unequal pads: each member's own value counts
    _c(640, 10, 191, 261, _PAIR, dev_past=40),                    # the suffix crosses a tile edge that is a split edge
    _c(640, 10, 191, 261, _F16, pads=(17,) * 16, twice=True),
    _c(640, 10, 191, 191, _F16, pads=(150,) * 16, dev_past=0),    # whole shared splits below the padding
    _c(640, 10, 129, 199, _MIX8, pads=(0, 17, 3, 0, 40, 3, 0, 3), dev_past=40),
    # capacity 640 / 3 splits: chunk 256, four tiles per split, the last split half full
    _c(640, 3, 255, 325, _PAIR),                                  # nothing shared
    _c(640, 3, 256, 256, _PAIR, pads=(17, 17), dev_past=0),
    _c(640, 3, 513, 583, _F16, dev_past=40),
    _c(640, 3, 513, 513, _MIX8, pads=(0, 150, 17, 0, 40, 17, 0, 17), twice=True),
    # capacity 1280 / 5 splits: chunk 256
    _c(1280, 5, 767, 837, _PAIR, pads=(150, 150), dev_past=40),
    _c(1280, 5, 767, 767, _MIX8, dev_past=0),
)
assert len({c.id for c in CASES}) == len(CASES)
