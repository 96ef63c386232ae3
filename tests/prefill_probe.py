"""Probing inputs and an fp64 reference for the prompt-sized attention kernels behind p3v_attention (k_attn_prefill_dma, k_attn_prefill_il,
k_attn_prefill_pp; csrc/p3v_attn_prompt.hip), in the instantiations the model launches: pre-scaled Q, every key read from the cache (new_is_cache).

Gaussian q / K / V cannot fail here for the reason tests/attn_probe.py gives: over n keys the softmax is nearly flat, and a causal or
pad boundary off by one, a ring slot reused a tile too early or a neighbour's kv head moves an output by ~1/n.  The inputs built here keep
the output O(1) and put most of a query's weight on a few keys whose identity shows in the output:

  * K (the same construction for every batch row and kv head).  k_t[0] = t // 64 and k_t[1] = t % 64, exact in bf16; 4.0 on the dim
    2 + (t // 64 + 5 kvh + 3 b) mod (hd - 2), which names the 64-key tile -- and, through the shift, the kv head and the batch row; bounded
    noise (uniform, +-1/32) on the dims from 2 on.
  * V.  10.0 on the dims d and d + 21 (mod hd), d = (t mod 64 + 7 (t // 64) + 5 kvh + 3 b) mod hd: they name the key inside its tile, the
    tile (7 being odd) and, through the shift, the kv head and the batch row (two dims, so that no key's only dim is one where the output is
    large for another reason); 4.0 on dim (13 (t // 64) + 5) mod hd, so that an output carries every tile's share of the weight on a dim of
    its own; noise uniform +-1/4.
  * Q.  Query i of head h belongs to family (h + i) mod 3 -- the families ride on the rows of every head, so that every kv head is
    probed by all three and neighbouring rows of an MFMA tile never agree; `tile_only` cases use TILE on every row:
      UP    q[0] = 64, q[1] = 1, noise +-1/8 elsewhere: the score rises by 1 (log2) per key, the LAST visible key holds ~half the
            weight, the one before a quarter ...: every query's own causal boundary is probed, the exponent reference moves in every tile.
      DOWN  q[0] = -64, q[1] = -1: the FIRST visible key (pad_len[b], or 0) holds ~half the weight: the left boundary of every row.
            (With one head per kv head the last two rows of a causal case take UP instead: nobody else sees their keys.  The cases
            with pads run two heads per kv head, six heads in all: every row then has a DOWN head and every kv head one that is not.)
      TILE  4.0 on the dim of a primary tile and 3.0 on the dim of a secondary one, zero elsewhere: the visible keys of the primary
            tile share ~16/17 of the weight evenly (within 2^+-1/4: the noise bound), the secondary tile 1/17.  Losing one key of the primary
            tile moves its two dims by ~10/64 x 0.8; counting the primary tile twice halves the secondary's share, on a dim where the output is
            small.  Primaries are dealt from the last row down so that every visible tile -- the first and the diagonal one included -- is
            some row's primary on every head (on the spot rows where only those are compared); the rest is pseudo-random.
  * DEAD REGION.  K rows and V^T columns at t < pad_len[b] and at past + L <= t < past_t hold POISON (1e4; finite, as include/p3v.h
    requires): a leaked key takes the whole row.  The capacity is past_t = roundup(past + L, 64) + 128: the row stride is not the tile count.

The reference is plain fp64 on the bf16 tensors the kernel is given: s = q_in . k (q_in carries scale * log2 e already); query i of
row b sees t iff t >= pad_len[b] and (not causal or t <= past + i); p = 2^(s - max); o = p . v / sum p; rows with past + i < pad_len[b]
are exactly 0.  Nothing in it is rounded.  Everything here is torch / numpy on the CPU; which kernel a call takes and its head_group are
asked of the library's route (ops.attention_route: host-only, no GPU).
"""
import math
from contextlib import contextmanager
from dataclasses import dataclass
from functools import lru_cache

import numpy as np
import torch

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
POISON = 1.0e4
RTOL, ATOL = 2 ** -6, 2e-2
K_SPIKE, Q_MAIN, Q_SIDE = 4.0, 4.0, 3.0
V_KEY, V_TILE = 10.0, 4.0
UP, DOWN, TILE = 0, 1, 2

# path -> (attn_pp, attn_il, attn_il_waves) for ops.set_tuning, and the kernel the library then takes for a call whose keys all lie in
# a cache of whole tiles (pre: Q pre-scaled or plain; il takes pre-scaled Q only)
KNOBS = ("attn_pp", "attn_il", "attn_il_waves")
PATHS = {"dma": (0, 0, 0), "il4": (1, 1, 4), "il8": (1, 1, 8), "pp": (1, 0, 0)}
KERNELS = {"dma": "k_attn_prefill_dma<{hd}, {pre}>", "il4": "k_attn_prefill_il<{hd}, 4>", "il8": "k_attn_prefill_il<{hd}, 8>",
           "pp": "k_attn_prefill_pp<{hd}, {pre}>"}


def kernel_of(path, hd, q_prescaled=True):
    return KERNELS[path].format(hd=hd, pre="true" if q_prescaled else "false")


def takes(ops, path, **call):
    """Does the library, with the knobs of `path`, run the kernel of `path` for this call (the arguments of ops.attention_route)?"""
    r = ops.attention_route(**call, **dict(zip(KNOBS, PATHS[path])))
    return r.status == 0 and r.kernel_name.decode() == kernel_of(path, call["hd"], call.get("q_prescaled", False))


@contextmanager
def pinned(ops, path, **call):
    """Pin the kernel of `path` for the ops.attention call about to be made: sets the three knobs, asserts from the library's route
    (ops.attention_route(**call), the library's own settings) that this call takes that kernel, and restores the knobs."""
    old = [ops.set_tuning(name, val) for name, val in zip(KNOBS, PATHS[path])]
    try:
        r = ops.attention_route(**call)
        want = kernel_of(path, call["hd"], call.get("q_prescaled", False))
        assert r.status == 0 and r.kernel_name.decode() == want, f"pinned {path}: the call runs {r.kernel_name.decode()!r}, not {want}"
        yield r
    finally:
        for name, val in zip(KNOBS, old):
            ops.set_tuning(name, val)


@dataclass(frozen=True)
class Case:
    name: str
    B: int
    L: int
    past: int = 0
    hd: int = 96
    nh: int = 3
    nkv: int = 3
    causal: bool = True
    pads: tuple = None
    tile_only: bool = False      # TILE on every row
    spot: bool = False           # compare (and build the reference) on spot rows only

    @property
    def T(self):
        return self.past + self.L

    @property
    def past_t(self):
        return (self.T + 63) // 64 * 64 + 128

    @property
    def n_tiles(self):
        return (self.T + 63) // 64

    @property
    def pad(self):
        return list(self.pads) if self.pads else [0] * self.B

    @property
    def head_group(self):
        """The heads whose query blocks the launch interleaves: the route's answer (csrc/p3v_attn_prompt.hip: prompt_route)."""
        from phi_3_vision_mlx_amd import ops
        return ops.attention_route(**self.call).head_group

    @property
    def call(self):
        """The arguments of ops.attention_route for the call `launch` makes."""
        return dict(B=self.B, Lq=self.L, nh=self.nh, nkv=self.nkv, hd=self.hd, past=self.past, past_t=self.past_t, new_is_cache=True,
                    q_prescaled=True)

    @property
    def id(self):
        return self.name


CASES = (
    Case("B1-L700-hd96", 1, 700),                                             # 11 tiles, the last 256-row block ragged
    Case("B2-L300-pads0,77", 2, 300, nh=6, pads=(0, 77)),                            # pad boundary inside the second tile, padded query rows
    Case("B1-L257", 1, 257, nh=6),                                                   # a block that holds one query
    Case("B1-L200-past448-pad5", 1, 200, nh=6, past=448, pads=(5,)),                 # the prefix-cache shape
    Case("B1-L40-past200", 1, 40, nh=6, past=200),
    Case("B2-L33-past100-pads3,100", 2, 33, nh=6, past=100, pads=(3, 100)),          # row 1: its whole past is padding
    Case("B3-L577-hd64-noncausal", 3, 577, hd=64, causal=False),               # the CLIP crop shape
    Case("B1-L330-gqa6,2", 1, 330, nh=6, nkv=2),
    Case("B1-L64", 1, 64, nh=6),                                                     # one tile
    Case("B1-L17", 1, 17, nh=6),                                                     # fewer queries than a wave
    Case("B1-L5632-nh32-headgroup8", 1, 5632, nh=32, nkv=32, tile_only=True, spot=True),
)
assert len({c.id for c in CASES}) == len(CASES)
assert CASES[-1].head_group == 8 and all(c.head_group == c.nh for c in CASES[:-1])


def bf16_round(x):
    return x.to(F32).to(BF16)


def spot_rows(L):
    """The first and last row of every 256-row block and 64 rows spread between them: the last rows of the 64 highest 64-key tiles that do
    not end a block.  (Rows that end a tile see the whole of it: with them every tile can be some spot row's primary with all of its keys
    visible; the lowest tiles left over go to the rows that start a block.)"""
    rows = {r for b0 in range(0, L, 256) for r in (b0, min(b0 + 255, L - 1))}
    ends = [r for r in range(63, L, 64) if r not in rows]
    return sorted(rows | set(ends[-64:]))


def tile_dim(j, b, kvh, hd):
    return 2 + (j + 5 * kvh + 3 * b) % (hd - 2)


def key_dims(t, b, kvh, hd):
    d = (t % 64 + 7 * (t // 64) + 5 * kvh + 3 * b) % hd
    return d, (d + 21) % hd


def share_dim(j, hd):
    return (13 * j + 5) % hd


class Probe:
    """The inputs of one case and their fp64 reference (module docstring)."""

    def __init__(self, case, seed=0):
        self.case = c = case
        B, L, past, hd, nh, nkv, T, Tp = c.B, c.L, c.past, c.hd, c.nh, c.nkv, c.T, c.past_t
        grp = nh // nkv
        assert nh % nkv == 0 and c.n_tiles <= hd - 2 and all(0 <= p <= T for p in c.pad)
        gen = torch.Generator().manual_seed(4321 + seed)
        rng = np.random.default_rng(99 + seed)
        uni = lambda shape, a: (torch.rand(shape, generator=gen, dtype=F32) * 2 - 1) * a
        t = torch.arange(Tp)
        tile = t // 64
        # ---- K [B, nkv, past_t, hd], V [B, nkv, past_t, hd] (handed over transposed)
        k = uni((B, nkv, Tp, hd), 1 / 32)
        k[..., 0], k[..., 1] = tile.float(), (t % 64).float()
        v = uni((B, nkv, Tp, hd), 0.25)
        for b in range(B):
            for kvh in range(nkv):
                k[b, kvh, t, 2 + (tile + 5 * kvh + 3 * b) % (hd - 2)] += K_SPIKE
                for d in key_dims(t, b, kvh, hd):
                    v[b, kvh, t, d] += V_KEY
                v[b, kvh, t, share_dim(tile, hd)] += V_TILE
            k[b, :, :c.pad[b]] = POISON
            v[b, :, :c.pad[b]] = POISON
        k[:, :, T:] = POISON
        v[:, :, T:] = POISON
        k, v = bf16_round(k), bf16_round(v)
        # ---- Q [B, nh, L, hd]
        self.rows = spot_rows(L) if c.spot else list(range(L))
        self.family = np.zeros((B, nh, L), dtype=np.int64)
        self.primary = np.full((B, nh, L), -1, dtype=np.int64)
        q = uni((B, nh, L, hd), 1 / 8)
        i = np.arange(L)
        for b in range(B):
            lo = c.pad[b] // 64
            hi = np.minimum((past + i) // 64, c.n_tiles - 1) if c.causal else np.full(L, c.n_tiles - 1)
            live = past + i >= c.pad[b]
            for h in range(nh):
                fam = np.full(L, TILE) if c.tile_only else (h + i) % 3
                if c.causal and not c.tile_only and grp == 1:
                    fam[-2:] = np.where(fam[-2:] == DOWN, UP, fam[-2:])
                self.family[b, h] = fam
                sign = torch.from_numpy(np.where(fam == DOWN, -1.0, 1.0)).float()
                q[b, h, :, 0], q[b, h, :, 1] = 64.0 * sign, sign
                mine = [r for r in self.rows[::-1] if fam[r] == TILE and live[r]]
                seen = set(mine)
                mine += [r for r in range(L - 1, -1, -1) if fam[r] == TILE and live[r] and r not in seen]
                if not mine:
                    continue
                mine, kvh = np.array(mine), h // grp
                n_vis = hi[mine] - lo + 1
                j1 = lo + rng.integers(0, 1 << 30, len(mine)) % n_vis
                nxt = c.n_tiles - 1                                                   # the highest tile that is nobody's primary yet
                for n, r in enumerate(mine):
                    if nxt < lo:
                        break
                    j1[n] = min(nxt, hi[r])
                    nxt = j1[n] - 1
                # a secondary tile, pseudo-random (none where the primary is the only visible tile)
                j2, start = np.full(len(mine), -1), rng.integers(0, 1 << 30, len(mine))
                for s in range(2):
                    j = lo + (start + s) % n_vis
                    ok = (j2 < 0) & (j != j1)
                    j2 = np.where(ok, j, j2)
                qt = torch.zeros((len(mine), hd))
                has2 = j2 >= 0
                qt[np.flatnonzero(has2), tile_dim(j2[has2], b, kvh, hd)] = Q_SIDE
                qt[np.arange(len(mine)), tile_dim(j1, b, kvh, hd)] = Q_MAIN
                q[b, h, mine] = qt
                self.primary[b, h, mine] = j1
        self.q, self.k, self.vt = bf16_round(q), k, v.transpose(2, 3).contiguous()
        # ---- fp64: raw scores over whole tiles [B, nh, R, Tc], the visibility [B, R, Tc], the reference
        self.Tc = Tc = c.n_tiles * 64
        self.kd, self.vd = k[:, :, :Tc].to(F64), v[:, :, :Tc].to(F64)
        self.qd = self.q[:, :, self.rows].to(F64)
        self.s = self.scores(self.kd)
        self.vis = self.visible()
        self.o, self.m, self.den = self.attend(self.s, self.vis, self.vd)
        self.ref = self.flat(self.o)
        self.live = torch.tensor([[past + r >= c.pad[b] for r in self.rows] for b in range(B)])            # [B, R]

    # ---- the reference and its mutants
    def scores(self, kd):
        c = self.case
        R = len(self.rows)
        return torch.einsum("bkgrd,bktd->bkgrt", self.qd.view(c.B, c.nkv, c.nh // c.nkv, R, c.hd), kd).reshape(c.B, c.nh, R, -1)

    def visible(self, causal_shift=0, pad_shift=0, past=None):
        """[B, R, Tc] bool: pad_len[b] + pad_shift <= t < past + L, and t <= past + i + causal_shift under the causal mask; rows that
        are themselves padding (past + i < pad_len[b]) see nothing."""
        c = self.case
        past = c.past if past is None else past
        t = torch.arange(self.Tc)[None, None, :]
        i = torch.tensor(self.rows)[None, :, None]
        pad = torch.tensor(c.pad)[:, None, None]
        vis = (t >= pad + pad_shift) & (t < c.T) & (c.past + i >= pad)
        return vis & (t <= past + i + causal_shift) if c.causal else vis.expand(c.B, len(self.rows), self.Tc)

    def attend(self, s, vis, vd):
        """p = 2^(s - max) over the visible keys; o = p . v / sum p -> o [B, nh, R, hd], max [B, nh, R], sum p [B, nh, R] (fp64)."""
        c = self.case
        s = s.masked_fill(~vis[:, None], -math.inf)
        m = s.amax(-1)
        m = torch.where(m == -math.inf, torch.zeros_like(m), m)
        e = torch.exp2(s - m[..., None])
        den = e.sum(-1)
        o = torch.einsum("bkgrt,bktd->bkgrd", e.view(c.B, c.nkv, c.nh // c.nkv, len(self.rows), -1), vd).reshape(c.B, c.nh, len(self.rows), c.hd)
        return o / den.clamp_min(1e-300)[..., None], m, den

    def flat(self, o):
        """[B, nh, R, hd] -> [B, R, nh * hd], the layout of `out`."""
        return o.transpose(1, 2).reshape(self.case.B, len(self.rows), -1)

    def weights(self):
        e = torch.exp2(self.s.masked_fill(~self.vis[:, None], -math.inf) - self.m[..., None])
        return e / self.den.clamp_min(1e-300)[..., None]

    def tol(self, o=None):
        return ATOL + RTOL * (self.o if o is None else o).abs()

    def lost_key_moves(self):
        """[B, nkv, Tc]: for every key, the largest move / tolerance over the queries and elements of its kv head when that key alone is
        lost (o' = (o - w v) / (1 - w); a query that saw nothing else: o' = 0).  Dead keys: 0."""
        c = self.case
        grp = c.nh // c.nkv
        w = self.weights()
        b, h, r, t = (w > 1e-4).nonzero(as_tuple=True)                              # below that a key cannot move anything by a tolerance
        wv, o = w[b, h, r, t][:, None], self.o[b, h, r]
        alone = wv > 1 - 1e-9
        gone = torch.where(alone, torch.zeros_like(o), (o - wv * self.vd[b, h // grp, t]) / torch.where(alone, torch.ones_like(wv), 1 - wv))
        ratio = ((gone - o).abs() / self.tol(o)).amax(-1)
        out = torch.zeros(c.B * c.nkv * self.Tc, dtype=F64)
        out.scatter_reduce_(0, (b * c.nkv + h // grp) * self.Tc + t, ratio, "amax")
        return out.view(c.B, c.nkv, self.Tc)

    def with_key(self, t_of_row, add):
        """The reference with key t_of_row[b, r] (-1: none) made visible (add) or hidden (not add) for row r -> [B, nh, R, hd].
        Exact: w = 1 / (1 + sum p . 2^(max - s_t)) is the weight the key takes or has."""
        c = self.case
        t = t_of_row.clamp_min(0)[:, None, :, None].expand(c.B, c.nh, len(self.rows), 1)
        s_t = self.s.gather(-1, t).squeeze(-1)
        grp = c.nh // c.nkv
        v_t = torch.stack([self.vd[b, torch.arange(c.nh) // grp][:, t_of_row[b].clamp_min(0)] for b in range(c.B)])       # [B, nh, R, hd]
        rel = torch.exp2((self.m - s_t).clamp(-1000, 1000))                                 # 2^(max - s_t)
        if add:
            w = torch.where(self.den > 0, 1 / (1 + self.den * rel), torch.ones_like(rel))[..., None]
            new = (1 - w) * self.o + w * v_t
        else:
            w = (1 / (self.den * rel).clamp_min(1e-300)).clamp_max(1.0)[..., None]
            alone = w > 1 - 1e-9
            new = torch.where(alone, torch.zeros_like(self.o), (self.o - w * v_t) / torch.where(alone, torch.ones_like(w), 1 - w))
        return torch.where((t_of_row >= 0)[:, None, :, None], new, self.o)

    def tile_mutants(self, b, h):
        """Row b, head h: every whole-tile defect of the walk over the key tiles, evaluated from per-tile partial sums.  -> dict name ->
        [n_tiles] worst move / tolerance over the rows and elements (0 where the defect does not exist: no tile d before it)."""
        c = self.case
        nt, R, hd = c.n_tiles, len(self.rows), c.hd
        kvh = h // (c.nh // c.nkv)
        vis = self.vis[b].view(R, nt, 64).transpose(0, 1)                                   # [nt, R, 64]
        s = self.s[b, h].view(R, nt, 64).transpose(0, 1)
        m = self.m[b, h][None, :, None]
        e = torch.where(vis, torch.exp2((s - m).clamp_max(900)), torch.zeros_like(s))
        vt = self.vd[b, kvh].view(nt, 64, hd)
        N, D = torch.bmm(e, vt), e.sum(-1)                                                  # [nt, R, hd], [nt, R]
        Ntot, Dtot = N.sum(0), D.sum(0)
        o, tol = self.o[b, h], self.tol(self.o[b, h])
        seen = vis.any(-1)                                                                  # [nt, R]: the row walks this tile

        def worst(N2, D2, d=0):
            """The partial (N, D)[j] of tile j replaced by (N2, D2)[j - d], one j >= d at a time -> [nt]."""
            den = (Dtot[None] - D[d:] + D2)[..., None]
            new = torch.where(den > 0, (Ntot[None] - N[d:] + N2) / den.clamp_min(1e-300), torch.zeros_like(N2))
            return torch.cat([torch.zeros(d, dtype=F64), (((new - o[None]).abs() / tol[None]).amax(-1) * seen[d:]).amax(-1)])

        res = {"skipped": worst(torch.zeros_like(N), torch.zeros_like(D)), "counted twice": worst(2 * N, 2 * D)}
        for d in (3, 4, 5):
            if nt <= d:
                continue
            res[f"V^T tile from {d} before"] = worst(torch.bmm(e[d:], vt[:-d]), D[d:], d)
            e2 = torch.where(vis[d:], torch.exp2((s[:-d] - m).clamp_max(900)), torch.zeros_like(s[d:]))
            res[f"K tile from {d} before"] = worst(torch.bmm(e2, vt[d:]), e2.sum(-1), d)
        return res


def worst_ratio(got, ref, rtol=RTOL, atol=ATOL):
    """max |got - ref| / (atol + rtol |ref|): > 1 is what close(..., rtol, atol) rejects."""
    got, ref = got.to(F64), ref.to(F64)
    return float(((got - ref).abs() / (atol + rtol * ref.abs())).max()) if got.numel() else 0.0


@lru_cache(maxsize=2)
def probe(case):
    return Probe(case)


GUARD = 4096                     # bf16 words on either side of `out`


def launch(ops, pr, path, device="cuda"):
    """Run the case of `pr` through ops.attention with the kernel of `path` pinned, twice on the same inputs -> dict of CPU tensors:
    out, out2 [B, L, nh * hd], the whole guarded buffer `buf` and its initial image `buf0`, the K / V^T buffers after the launches."""
    c = pr.case
    n = c.B * c.L * c.nh * c.hd
    q, k, vt = pr.q.to(device), pr.k.to(device), pr.vt.to(device)
    pad = torch.tensor(c.pad, dtype=torch.int32, device=device) if c.pads else None
    buf0 = torch.full((2 * GUARD + n,), -77.0, dtype=BF16)
    buf0[GUARD:GUARD + n] = float("nan")
    res = {"buf0": buf0}
    with pinned(ops, path, **c.call):
        for name in ("out", "out2"):
            buf = buf0.to(device)
            out = buf[GUARD:GUARD + n].view(c.B, c.L, c.nh * c.hd)
            ops.attention(q, out, c.B, c.L, c.nh, c.nkv, c.hd, 1.0, c.causal, past=c.past, k_past=k, v_past=vt, past_t=c.past_t,
                          pad_len=pad, new_is_cache=True, q_prescaled=True)
            torch.cuda.synchronize()
            res[name] = out.cpu()
            res["buf"] = buf.cpu()
    res["k"], res["vt"] = k.cpu(), vt.cpu()
    return res
