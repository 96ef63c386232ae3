"""p3v_attention_decode_family on the probing inputs of tests/attn_family_probe.py (whose power tests/test_attn_family_cpu.py
shows on the reference alone).  Every case asserts:
  (a) `out` within `RTOL 2^-6, ATOL 2e-2` of the fp64 reference of each row over its own copy;
  (b) `out` and both caches bit-identical between the populated table and the table of single rows: sharing changes no bit;
  (c) the same bits again with POISON in every follower's columns [0, floor(share_end / chunk) * chunk), which the launch leaves
      as they were: the followers' prefix is not read;
and that no cache byte outside column `past` changes, that `past` holds the rotated key / the value of the row, and that the
workspace is left all-ones (a second launch on it gives the same bits)."""
import ctypes as C

import pytest
import torch

import attn_family_probe as fp
from attn_family_probe import BF16, CASES, HD, NH, NKV, POISON, SCALE, launch, probe, table, worst_ratio

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from phi_3_vision_mlx_amd import ops
    return ops


def _bits(t):
    return t.contiguous().view(torch.int16)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_family_launch(ops, case):
    pr = probe(case)
    shared, single, poisoned = launch(ops, pr), launch(ops, pr, shared=False), launch(ops, pr, poison_followers=True)
    ratio = worst_ratio(shared["out"], pr.ref)
    print(f"{case.id}: worst ratio {ratio:.3f}")
    assert ratio <= 1.0                                                              # (a)
    assert worst_ratio(single["out"], pr.ref) <= 1.0
    for name in ("out", "k", "vt") + (("out2",) if case.twice else ()):              # (b), (c)
        assert _same(shared[name], single[name]), f"{name}: the populated table and the table of single rows differ"
        if name in ("out", "out2"):
            assert _same(poisoned[name], shared[name]), f"{name} depends on a follower's shared columns"
    if case.twice:
        assert _same(shared["out2"], shared["out"])
    for res in (shared, single, poisoned):
        k_exp, vt_exp = res["k_in"].clone(), res["vt_in"].clone()                    # nothing but column `past` is written
        err = (res["k"][:, :, case.past].float() - pr.k_new.float()).abs()           # the appended K row: test_attn_probe_gpu's bound
        assert bool((err <= 1e-2 + 2 ** -7 * pr.k_new.float().abs()).all())
        k_exp[:, :, case.past], vt_exp[:, :, :, case.past] = res["k"][:, :, case.past], pr.v_new      # the appended V: bit exact
        assert _same(res["k"], k_exp) and _same(res["vt"], vt_exp)
        assert bool((res["ws"] == -1).all())                                         # every launch leaves `ws` as the next one needs it
    for g in case.groups:                                                            # (c): POISON still in place
        for r in g[1:]:
            assert bool((poisoned["k"][r, :, :case.dead_end] == POISON).all())
            assert bool((poisoned["vt"][r, :, :, :case.dead_end] == POISON).all())


def _refusal_setup(ops, B=3, cap=640, n_split=10, past=200):
    g = torch.Generator().manual_seed(7)
    dev = "cuda"
    t = {
        "qkv": torch.randn((B, (NH + 2 * NKV) * HD), generator=g).to(BF16).to(dev),
        "cos": torch.ones((B, 1, HD // 2), device=dev), "sin": torch.zeros((B, 1, HD // 2), device=dev),
        "k": torch.randn((B, NKV, cap, HD), generator=g).to(BF16).to(dev),
        "vt": torch.randn((B, NKV, HD, cap), generator=g).to(BF16).to(dev),
        "out": torch.full((B, 1, NH * HD), 3.0, dtype=BF16, device=dev),
        "ws": ops.attention_ws(B, 16, NH, HD, n_split, dev),
    }
    tab = torch.full((B, 18), -1, dtype=torch.int32)
    tab[:, 0], tab[:, 1] = 0, 100
    tab[0, 2:5] = torch.tensor([0, 1, 2], dtype=torch.int32)
    return t, tab, dict(B=B, cap=cap, n_split=n_split, past=past)


def _call(ops, t, tab, kw, tab_dev=None, **over):
    a = dict(Lq=1, hd=HD, merge_in_launch=False, o_proj_w=None, past=kw["past"], family_host=tab)
    a.update(over)
    tab_d = (tab if tab_dev is None else tab_dev).to("cuda")
    before = {n: x.clone() for n, x in t.items()}
    with pytest.raises(RuntimeError, match=r"-95"):                                  # P3V_ERR_UNSUPPORTED
        ops.attention_decode_family(t["qkv"], t["cos"], t["sin"], 1, t["k"], t["vt"], t["out"], kw["B"], NH, NKV, a["hd"], SCALE,
                                    a["past"], kw["cap"], t["ws"], kw["n_split"], tab_d, family_host=a["family_host"], Lq=a["Lq"],
                                    merge_in_launch=a["merge_in_launch"], o_proj_w=a["o_proj_w"])
    torch.cuda.synchronize()
    for n, x in t.items():                                                           # nothing written, nothing launched
        assert torch.equal(x.view(torch.uint8), before[n].view(torch.uint8)), f"{n} changed by a refused call"


def test_refusals_write_nothing(ops):
    t, tab, kw = _refusal_setup(ops)
    _call(ops, t, tab, kw, Lq=2)
    _call(ops, t, tab, kw, hd=64)
    _call(ops, t, tab, kw, o_proj_w=torch.zeros((8, NH * HD), dtype=BF16, device="cuda"))
    _call(ops, t, tab, kw, merge_in_launch=True)
    for row, col, val in ((1, 0, 3), (1, 0, -1), (0, 3, 3), (0, 4, -2)):             # lead / member outside [0, B)
        bad = tab.clone()
        bad[row, col] = val
        _call(ops, t, bad, kw)
    _call(ops, t, tab, kw, past=99)                                                  # share_end beyond the host's `past`


def test_a_family_of_17_is_refused(ops):
    t, tab, kw = _refusal_setup(ops, B=17)
    tab[:, 0] = 0
    tab[0, 2:18] = torch.arange(16, dtype=torch.int32)
    _call(ops, t, tab, kw)


def test_the_refused_tables_are_taken_when_mended(ops):
    """The set-up of the refusal tests is a valid call: what refuses above is the one thing each test breaks."""
    t, tab, kw = _refusal_setup(ops)
    ops.attention_decode_family(t["qkv"], t["cos"], t["sin"], 1, t["k"], t["vt"], t["out"], kw["B"], NH, NKV, HD, SCALE, kw["past"],
                                kw["cap"], t["ws"], kw["n_split"], tab.cuda(), family_host=tab)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(t["out"].float()).all()) and not bool((t["out"] == 3.0).all())


@pytest.mark.parametrize("case", [c for c in CASES if c.id in ("cap640-s10-se191-past261-16-pad17-host-twice", "cap1280-s5-se767-past837-2-pad150-dpast40")],
                         ids=lambda c: c.id)
def test_the_appended_row_is_the_one_p3v_attention_decode_appends(ops, case):
    """Both launchers rotate the new key with the one rope_chunk of csrc/p3v_attn_shared.h: the caches after the family launch
    and after p3v_attention_decode on the same inputs are equal bit for bit (and the outputs agree within the tolerance: the
    split kernels differ)."""
    pr = probe(case)
    fam = launch(ops, pr)
    B, dev = case.B, "cuda"
    cos, sin = (t[None].expand(B, 1, HD // 2).contiguous().to(dev) for t in (pr.cos, pr.sin))
    pad = torch.tensor(case.pad, dtype=torch.int32, device=dev) if case.pads else None
    d_past = torch.tensor([case.past], dtype=torch.int32, device=dev) if case.dev_past is not None else None
    k, vt = pr.k.to(dev), pr.vt.to(dev)
    out = torch.full((B, 1, NH * HD), float("nan"), dtype=BF16, device=dev)
    ops.attention_decode(pr.qkv.to(dev), cos, sin, 1, k, vt, out, B, 1, NH, NKV, HD, SCALE, case.lower_bound, case.cap,
                         ops.attention_ws(B, 1, NH, HD, case.n_split, dev), case.n_split, pad_len=pad, d_past=d_past)
    assert _same(k.cpu(), fam["k"]) and _same(vt.cpu(), fam["vt"])
    assert worst_ratio(out.cpu().view(B, -1), pr.ref) <= 1.0
