"""The two beam-search kernels against the rule as beam.py states it (include/p3v.h, "beam search"), bits compared: p3v_beam_end
on hand-made and random rows -- the next beams, the record, the counters, the ticket, guard bands around every output --
and p3v_kv_permute against torch.index_select on caches with a pattern of its own in every element."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
I32, F32, BF16 = torch.int32, torch.float32, torch.bfloat16
CANARY, FCANARY, GUARD = -77, -1234.5, 16
NINF = float("-inf")


def to_bits(x):
    return torch.as_tensor(np.asarray(x, dtype=np.float32)).to(BF16).view(torch.int16).numpy().view(np.uint16).copy()


def _guarded(n, dtype, fill, pinned=False):
    """n words between two guard bands -> (whole buffer, the view in the middle)"""
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype)
    buf = buf.pin_memory() if pinned else buf.to(DEV)
    return buf, buf[GUARD:GUARD + n]


def _guards_ok(buf, n, fill):
    b = buf.cpu()
    return bool((b[:GUARD] == fill).all()) and bool((b[GUARD + n:] == fill).all())


class Loop:
    """The loop state of p3v_beam_end, every output between guard bands."""

    def __init__(self, W, cum_in, rec_cap=4, step=0, past=40):
        from phi_3_vision_mlx_amd import _lib, ops
        self.W, self.rec_cap, self.step, self.past = W, rec_cap, step, past
        self.cum_in = np.asarray(cum_in, dtype=np.float32)
        self.bufs = {}
        g = {}
        for k, n, dt, fill in (("tok", W, I32, CANARY), ("parent", W, I32, CANARY), ("cum", W, F32, FCANARY), ("cand_id", 128, I32, CANARY),
                               ("cand_score", 128, F32, FCANARY), ("ticket", 1, I32, CANARY), ("d_step", 1, I32, CANARY),
                               ("d_past", 1, I32, CANARY)):
            self.bufs[k], g[k] = _guarded(n, dt, fill)
        self.bufs["rec"], rec = _guarded(rec_cap * _lib.BEAM_REC_INTS, I32, CANARY, pinned=True)
        g["rec"] = rec.view(rec_cap, _lib.BEAM_REC_INTS)
        self.g = g
        self.reset()
        self.state = ops.beam_state(g)

    def reset(self):
        g = self.g
        g["cum"].fill_(FCANARY)
        g["cum"][:len(self.cum_in)] = torch.from_numpy(self.cum_in)
        g["tok"].fill_(CANARY), g["parent"].fill_(CANARY), g["ticket"].zero_(), g["rec"].fill_(CANARY)
        g["d_step"].fill_(self.step), g["d_past"].fill_(self.past)
        torch.cuda.synchronize()

    def snapshot(self):
        torch.cuda.synchronize()
        return {k: self.bufs[k].cpu().clone() for k in ("tok", "parent", "cum", "ticket", "d_step", "d_past", "rec")}

    def check(self, ref, what):
        """`ref`: the record of beam.reference_step for the step just launched."""
        from phi_3_vision_mlx_amd import _lib
        torch.cuda.synchronize()
        g, W = self.g, self.W
        for k, n, fill in (("tok", W, CANARY), ("parent", W, CANARY), ("cum", W, FCANARY), ("cand_id", 128, CANARY),
                           ("cand_score", 128, FCANARY), ("ticket", 1, CANARY), ("d_step", 1, CANARY), ("d_past", 1, CANARY),
                           ("rec", self.rec_cap * _lib.BEAM_REC_INTS, CANARY)):
            assert _guards_ok(self.bufs[k], n, fill), f"{what}: a store next to {k}"
        assert int(g["ticket"][0]) == 0, f"{what}: arrival counter left at {int(g['ticket'][0])}"
        assert int(g["d_step"][0]) == self.step + 1 and int(g["d_past"][0]) == self.past + 1, what
        rec = g["rec"].numpy()
        for t in range(self.rec_cap):
            want = ref if t == self.step else np.full(_lib.BEAM_REC_INTS, CANARY, dtype=np.int32)
            assert np.array_equal(rec[t], want), f"{what}: record {t}\n{rec[t]}\n{want}"
        tok, parent = g["tok"].cpu().numpy(), g["parent"].cpu().numpy()
        cum = g["cum"].cpu().numpy().view(np.int32)
        if ref[0] == 0:
            assert np.array_equal(tok, ref[2:2 + W]) and np.array_equal(parent, ref[10:10 + W]), f"{what}: {tok} {parent}\n{ref}"
            assert np.array_equal(cum, ref[18:18 + W]), f"{what}: cum {cum} != {ref[18:18 + W]}"
        else:                                                              # a failed step: tok -1, the rows and their sums stay
            assert (tok == -1).all() and np.array_equal(parent, np.arange(W)), what
            want = np.full(W, FCANARY, dtype=np.float32)
            want[:len(self.cum_in)] = self.cum_in
            assert np.array_equal(cum, want.view(np.int32)), what


def _launch(bits, loop, eos):
    from phi_3_vision_mlx_amd import ops
    logits = torch.from_numpy(bits.view(np.int16)).to(DEV).view(BF16)
    ops.beam_end(logits, loop.state, loop.W, eos)
    return logits


def _one(bits, cum_in, W, eos, what, **kw):
    from phi_3_vision_mlx_amd import beam
    ref = beam.reference_step(bits, cum_in, W, eos)
    loop = Loop(W, cum_in, **kw)
    _launch(bits, loop, eos)
    loop.check(ref, what)
    return ref


def _cases(W, R, n, rng):
    """(name, bits [R, n], cum_in [R], eos) -- the hand-made rows of the issue at this shape"""
    C = 2 * W
    cum = (-rng.random(R) * 3).astype(np.float32) if R > 1 else np.zeros(1, np.float32)
    x = rng.standard_normal((R, n)).astype(np.float32) * 2
    out = [("random", to_bits(x), cum, int(rng.integers(0, n))),
           ("all equal", to_bits(np.ones((R, n))), np.full(R, cum[0], np.float32), 1)]
    y = x.copy()
    y[:, n - 1] = 30.0
    out.append(("eos first in every row", to_bits(y), cum, n - 1))
    # distinct descending values in row 0, the other rows far below: order index j is row 0's place j
    for place in (W - 1, W):
        y = np.full((R, n), -40.0, np.float32)
        ids = rng.permutation(n)[:C]
        y[0, ids] = 8.0 - 0.25 * np.arange(C)
        c = np.full(R, -30.0, np.float32)
        c[0] = 0
        out.append((f"eos at order index {place}", to_bits(y), c, int(ids[place])))
    if R > 1:
        y = x.copy()
        y[1] = y[0]
        c = cum.copy()
        c[1] = c[0] = 0
        out.append(("two equal rows", to_bits(y), c, int(rng.integers(0, n))))
        c = np.full(R, -60.0, np.float32)
        c[R - 1] = 0
        out.append(("one parent takes all", to_bits(x), c, n))             # (eos = n: no token is the EOS)
    y = np.full((R, n), NINF, np.float32)
    for r in range(R):
        y[r, rng.permutation(n)[:3]] = rng.standard_normal(3)
    out.append(("three finite logits per row", to_bits(y), cum, int(np.flatnonzero(np.isfinite(y[0]))[0])))
    for bad in (float("nan"), float("inf")):
        y = x.copy()
        y[R - 1, int(rng.integers(0, n))] = bad
        out.append((f"a {bad} row", to_bits(y), cum, 0))
    return out


@pytest.mark.parametrize("W", [2, 3, 4, 8])
def test_beam_end_matches_the_rule_bit_for_bit(W):
    rng = np.random.default_rng(W)
    seen = set()
    for R in (1, W):
        for n in (2 * W, 2 * W + 1, 1031, 32064):
            for name, bits, cum, eos in _cases(W, R, n, rng):
                ref = _one(bits, cum, W, eos, f"W={W} R={R} n={n} {name}", step=int(rng.integers(0, 4)))
                seen.add((name, int(ref[0]), int(ref[1])))
    # the hand-made rows mean what their names say
    assert (f"eos at order index {W - 1}", 0, 1) in seen and (f"eos at order index {W}", 0, 0) in seen
    assert {name for name, s, _ in seen if s == 1} == {"a nan row", "a inf row"}
    assert not {name for name, s, _ in seen if s == 0} & {"a nan row", "a inf row"}


def test_beam_end_large_row_takes_the_wide_kernel():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((4, 65536)).astype(np.float32) * 3
    _one(to_bits(x), [-1.0, -0.5, -2.0, -0.25], 4, 7, "n=65536")
    _one(to_bits(x[:, :40001]), [-1.0, -0.5, -2.0, -0.25], 4, 7, "n=40001")


def test_beam_end_record_capacity_second_launch_and_graph_replay():
    from phi_3_vision_mlx_amd import beam, ops
    rng = np.random.default_rng(11)
    W, n = 4, 1031
    bits, cum = to_bits(rng.standard_normal((W, n)) * 2), (-rng.random(W)).astype(np.float32)
    ref = beam.reference_step(bits, cum, W, 3)
    # rec_cap reached: the step runs, nothing is recorded
    loop = Loop(W, cum, rec_cap=2, step=2)
    _launch(bits, loop, 3)
    torch.cuda.synchronize()
    assert (loop.bufs["rec"] == CANARY).all() and loop.g["tok"].tolist() == ref[2:2 + W].tolist()
    assert int(loop.g["d_step"][0]) == 3 and int(loop.g["ticket"][0]) == 0
    # a second launch from the same state, then a graph replay: every output word the same
    loop = Loop(W, cum, step=1)
    logits = _launch(bits, loop, 3)
    loop.check(ref, "first")
    first = loop.snapshot()
    loop.reset()
    ops.beam_end(logits, loop.state, W, 3)
    second = loop.snapshot()
    loop.reset()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        g = ops.Graph()
        g.begin()
        ops.beam_end(logits, loop.state, W, 3)
        g.end()
        g.launch()
        side.synchronize()
    replay = loop.snapshot()
    for k, v in first.items():
        assert torch.equal(v.view(I32), second[k].view(I32)) and torch.equal(v.view(I32), replay[k].view(I32)), k
    # two steps in a row on the device's own state: cum feeds the next step
    loop.reset()
    ops.beam_end(logits, loop.state, W, 3)
    ops.beam_end(logits, loop.state, W, 3)
    torch.cuda.synchronize()
    ref2 = beam.reference_step(bits, ref[18:18 + W].view(np.float32), W, 3)
    assert np.array_equal(loop.g["rec"].numpy()[2], ref2) and np.array_equal(loop.g["rec"].numpy()[1], ref)


def test_beam_end_refusals_write_nothing():
    from phi_3_vision_mlx_amd import _lib
    import ctypes as C
    lib = _lib.lib()
    W = 4
    loop = Loop(W, np.zeros(W, np.float32))
    before = loop.snapshot()
    big = torch.zeros(W, 65537, dtype=BF16, device=DEV)
    p = big.data_ptr()

    def call(st=loop.state, logits=p, R=W, W_=W, n=64):
        return lib.p3v_beam_end(logits, C.byref(st) if st is not None else None, R, W_, n, 0, None)
    assert call(logits=None) == -22 and call(st=None) == -22
    for f, _ in _lib.BeamState._fields_[:9]:
        st = _lib.BeamState.from_buffer_copy(loop.state)
        setattr(st, f, None)
        assert call(st=st) == -22, f
    assert call(W_=1, R=1) == -22 and call(W_=9, R=9) == -22 and call(R=2) == -22 and call(R=0) == -22
    assert call(n=2 * W - 1) == -22 and call(R=1, n=2 * W - 1) == -22
    assert call(n=65537) == -95
    after = loop.snapshot()
    for k, v in before.items():
        assert torch.equal(v.view(I32), after[k].view(I32)), k


# ------------------------------------------------------------------------------------------------ the reorder
def _pattern(n, salt):
    i = torch.arange(n, dtype=torch.int64, device=DEV)
    return ((i * 40503 + (i >> 16) * 977 + salt) & 0x7FFF).to(torch.int16)      # a pattern of its own per element; never a NaN


class Caches:
    def __init__(self, nl, B, nkv, T, hd, W, stage_cols):
        pad = 64                                                          # elements: the views stay 16-byte aligned
        self.shape, self.W, self.pad = (nl, B, nkv, T, hd), W, pad
        nkv_el, st_el = nl * B * nkv * T * hd, nl * W * nkv * stage_cols * hd
        self.flat = [(_pattern(nkv_el + 2 * pad, 1)), _pattern(nkv_el + 2 * pad, 2),
                     torch.full((st_el + 2 * pad,), 0x1111, dtype=torch.int16, device=DEV),
                     torch.full((st_el + 2 * pad,), 0x2222, dtype=torch.int16, device=DEV)]
        mid = [f[pad:-pad].view(BF16) for f in self.flat]
        self.k, self.vt = mid[0].view(nl, B, nkv, T, hd), mid[1].view(nl, B, nkv, hd, T)
        self.stage = (mid[2].view(nl, W, nkv, stage_cols, hd), mid[3].view(nl, W, nkv, hd, stage_cols))
        self.parent = torch.zeros(W, dtype=I32, device=DEV)
        self.d_past = torch.zeros(1, dtype=I32, device=DEV)

    def move(self, parent, c0a, past):
        from phi_3_vision_mlx_amd import ops
        self.parent.copy_(torch.tensor(parent, dtype=I32))
        self.d_past.fill_(past)
        for phase in (0, 1):
            ops.kv_permute((self.k, self.vt), self.parent, self.W, c0a, self.d_past, self.stage, phase)


def _expected(c, parent, c0a, past, cols=None):
    """torch.index_select of the window; rows >= W, rows that stay and everything outside the window as before"""
    nl, B, nkv, T, hd = c.shape
    W = c.W
    end = min((min(max(past, 0), T) + 7) // 8 * 8, T, c0a + (cols if cols is not None else T))
    k, vt = c.k.clone(), c.vt.clone()
    if end > c0a:
        ok = [j for j in range(W) if 0 <= parent[j] < W and parent[j] != j]
        if ok:
            src = torch.tensor([parent[j] for j in ok], device=DEV)
            dst = torch.tensor(ok, device=DEV)
            k[:, dst, :, c0a:end] = c.k.index_select(1, src)[:, :, :, c0a:end]
            vt[:, dst, :, :, c0a:end] = c.vt.index_select(1, src)[..., c0a:end]
    return k, vt


@pytest.mark.parametrize("hd", [32, 96, 128])
def test_kv_permute_against_index_select(hd):
    nl, nkv = 2, 2
    for W, B in ((4, 4), (3, 5)):
        patterns = [list(range(W)), [1, 0] + list(range(2, W)), [1, 2, 0] + list(range(3, W)), [W - 1] * W,
                    ([2, 2, 0, 1] if W == 4 else [2, 1, 1])]
        for T in (64, 72):
            for c0a in (0, 8, 16):
                c = Caches(nl, B, nkv, T, hd, W, T - c0a)
                for past in sorted({c0a + 1, c0a + 8, c0a + 9, T - 9, T - 1, T}):
                    for parent in patterns:
                        flat0 = [f.clone() for f in c.flat]
                        want_k, want_vt = _expected(c, parent, c0a, past)
                        c.move(parent, c0a, past)
                        what = f"hd={hd} W={W} B={B} T={T} c0a={c0a} past={past} parent={parent}"
                        assert torch.equal(c.k.view(torch.int16), want_k.view(torch.int16)), what
                        assert torch.equal(c.vt.view(torch.int16), want_vt.view(torch.int16)), what
                        for f, f0 in zip(c.flat, flat0):                 # guard bands of the caches and of the staging buffers
                            assert torch.equal(f[:c.pad], f0[:c.pad]) and torch.equal(f[-c.pad:], f0[-c.pad:]), what
                        if parent == list(range(W)):                     # identity: caches AND stage bit-identical
                            assert all(torch.equal(f, f0) for f, f0 in zip(c.flat, flat0)), what


def test_kv_permute_defensive_words_and_short_stage():
    """A parent of -1 / W leaves its row alone, a *d_past of T + 100 (or below zero) is clamped to the row, and a staging
    buffer shorter than the window cuts the window: nothing outside the buffers is touched."""
    nl, nkv, hd, W, B, T = 2, 2, 96, 4, 6, 72
    for cols, c0a, past, parent in ((T, 0, T + 100, [1, -1, W, 0]), (T - 8, 8, T + 100, [3, 0, 1, 2]), (16, 16, 60, [1, 0, 3, 2]),
                                    (8, 8, 2 ** 31 - 1, [W, W, -1, -5]), (T, 0, -3, [1, 0, 3, 2]), (T, 64, 3, [1, 0, 3, 2])):
        c = Caches(nl, B, nkv, T, hd, W, cols)
        flat0 = [f.clone() for f in c.flat]
        want_k, want_vt = _expected(c, parent, c0a, past, cols)
        c.move(parent, c0a, past)
        what = f"cols={cols} c0a={c0a} past={past} parent={parent}"
        assert torch.equal(c.k.view(torch.int16), want_k.view(torch.int16)), what
        assert torch.equal(c.vt.view(torch.int16), want_vt.view(torch.int16)), what
        for f, f0 in zip(c.flat, flat0):
            assert torch.equal(f[:c.pad], f0[:c.pad]) and torch.equal(f[-c.pad:], f0[-c.pad:]), what


def test_kv_permute_refusals_launch_nothing():
    from phi_3_vision_mlx_amd import _lib, ops
    lib = _lib.lib()
    nl, nkv, hd, W, B, T = 2, 2, 32, 4, 4, 64
    c = Caches(nl, B, nkv, T, hd, W, T)
    flat0 = [f.clone() for f in c.flat]
    c.parent.copy_(torch.tensor([1, 0, 3, 2], dtype=I32))
    c.d_past.fill_(T)
    k, v, sk, sv, par, dp = (t.data_ptr() for t in (c.k, c.vt, c.stage[0], c.stage[1], c.parent, c.d_past))

    def call(k=k, v=v, B=B, T=T, par=par, W=W, c0a=0, dp=dp, sk=sk, sv=sv, cols=T, phase=0, hd=hd, es=2):
        return lib.p3v_kv_permute(k, v, B, T, par, W, c0a, dp, sk, sv, cols, phase, nl, nkv, hd, es, None)
    assert call(es=1) == -95 and call(hd=12) == -95 and call(T=60) == -95          # the int8 cache, hd * 2 % 16, T % 8
    for name in ("k", "v", "par", "dp", "sk", "sv"):
        assert call(**{name: None}) == -22, name
    assert call(W=1) == -22 and call(W=9) == -22 and call(B=3) == -22 and call(phase=2) == -22
    assert call(c0a=4) == -22 and call(c0a=T + 8) == -22 and call(c0a=-8) == -22 and call(cols=0) == -22 and call(cols=12) == -22
    assert call(k=k + 2) == -22 and call(sv=sv + 8) == -22
    k8 = torch.zeros(nl, B, nkv, T, hd, dtype=torch.uint8, device=DEV)
    v8 = torch.zeros(nl, B, nkv, hd, T, dtype=torch.uint8, device=DEV)
    sc = torch.zeros(nl, B, nkv, T, dtype=F32, device=DEV)
    with pytest.raises((RuntimeError, TypeError, ValueError)):                     # the int8 cache through the operator layer
        ops.kv_permute((k8, v8, sc, sc.clone()), c.parent, W, 0, c.d_past, (k8[:, :W], v8[:, :W]), 0)
    torch.cuda.synchronize()
    assert all(torch.equal(f, f0) for f, f0 in zip(c.flat, flat0))
