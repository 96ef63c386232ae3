"""The probes of tests/glue_probe.py, checked on the references alone (no GPU).  For every kernel family three things:
  * on >= 98 % of the elements of every bf16 case the rounding bracket is ONE value (the rule is "bit-exact but for ties");
  * a straightforward torch-fp32 restatement of the documented arithmetic stays inside every bracket and bound, so the bounds are
    not so tight that a correct kernel fails them;
  * every planted defect, applied to that restatement, leaves the bracket or bound in some element of some case.
A kernel with such a defect therefore cannot pass tests/test_glue_kernels_gpu.py."""
import pytest
import torch

import glue_probe as gp

ids = lambda c: c.id


# ---------------------------------------------------------------- the bracket itself
def test_bracket_and_inside():
    v = torch.tensor([1.0, -1.0, 0.0, 1.00390625, 3.0e-5], dtype=gp.F64)       # 1.00390625 = 1 + 2^-8: a bf16 rounding tie
    lo, hi = gp.bracket(v, torch.tensor([1e-6, 1e-6, 0.0, 1e-6, 1e-6], dtype=gp.F64))
    assert lo.dtype == hi.dtype == gp.BF16
    assert lo.tolist() == [1.0, -1.0, 0.0, 1.0, lo[4].item()] and hi.tolist() == [1.0, -1.0, 0.0, 1.0078125, hi[4].item()]
    assert gp.inside(torch.tensor([-0.0]).to(gp.BF16), lo[2:3], hi[2:3]).all()                   # -0 == +0
    assert not gp.inside(torch.tensor([float("nan")]), lo[:1], hi[:1]).any()
    assert not gp.inside(torch.tensor([1.0078125]).to(gp.BF16), lo[:1], hi[:1]).any()
    # the fp64 -> fp32 step rounds outwards: an end just inside a tie is not pulled onto it
    x = torch.tensor([1.00390625 + 2.0 ** -40], dtype=gp.F64)
    assert x.to(gp.F32).to(gp.BF16).item() == 1.0                                                # plain double rounding: the wrong side
    assert gp.bracket(x, 0.0)[1].item() == 1.0078125 and gp.bracket(-x, 0.0)[0].item() == -1.0078125
    assert gp.worst(torch.tensor([1.0, 2.0]), torch.tensor([1.0, 1.0]), torch.tensor([1.0, 1.5])).startswith("1 of 2 outside; worst at (1,)")


# ---------------------------------------------------------------- RMSNorm
@pytest.mark.parametrize("case", gp.RMS_CASES, ids=ids)
def test_rmsnorm_probe(case):
    pr = gp.probe(case)
    share = gp.unique_share(pr.lo, pr.hi)
    print(f"{case.id}: bracket is one value on {100 * share:.2f} %")
    assert share >= 0.98
    assert pr.verify(pr.restate()) == "", pr.verify(pr.restate())
    chunks = case.hidden // 8
    if case.rows == 33:                                                    # every probed position has its row
        assert [p for _, p in pr.hot] == gp.hot_positions(chunks)
        need = {0, 63, 64, chunks - 1, chunks - 2} | {p for q in range(0, chunks, 64) for p in (q, min(q + 63, chunks - 1))}
        assert {p for p in need if 0 <= p < chunks} == set(gp.hot_positions(chunks))
    for row, p in pr.hot:                                                  # (1) any single chunk dropped from the sum of squares
        assert pr.verify(pr.restate(drop=p)), f"chunk {p} dropped goes unseen"
        assert not bool(gp.inside(pr.restate(drop=p)[row], pr.lo[row], pr.hi[row]).all()), f"chunk {p}: its own row does not see it"
        assert bool((pr.x[row, 8 * p:8 * p + 8].float() == torch.tensor([8.0] * 4 + [16.0] * 4)).all())
    if chunks > 1:
        assert pr.verify(pr.restate(shift_w=True))                         # (2) weights shifted by one chunk
    if case.hidden > 8 and case.rows > 1:
        assert pr.verify(pr.restate(skip_round=True))                      # (3) the first rounding skipped


def test_rmsnorm_every_defect_fails():
    """Per defect, over the cases: a dropped chunk at every probed position of every hidden size, the shifted weights, the skipped
    first rounding (which moves ~10 % of the elements of a Gaussian row by one bf16 ulp)."""
    for case in gp.RMS_CASES:
        pr = gp.probe(case)
        if case.rows == 33:
            assert len(pr.hot) == len(gp.hot_positions(case.hidden // 8)) and all(pr.verify(pr.restate(drop=p)) for _, p in pr.hot)
        if case.hidden > 8:
            assert pr.verify(pr.restate(shift_w=True)), case.id
        if case.rows > 1 and case.hidden > 8:
            assert pr.verify(pr.restate(skip_round=True)), case.id
    assert {c.hidden for c in gp.RMS_CASES} == {8, 520, 3064, 3072, 3080, 8192} and {c.rows for c in gp.RMS_CASES} == {1, 6, 33}


# ---------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("hidden", gp.LN_HIDDEN)
def test_layernorm_probe(hidden):
    pr = gp.ln_probe(hidden)
    share = gp.unique_share(pr.lo, pr.hi)
    y = pr.restate()
    msg, ratio = pr.verify(y, True)
    print(f"ln-h{hidden}: bracket is one value on {100 * share:.2f} %; fp32 restatement at {ratio:.3f} of E")
    assert share >= 0.98
    assert msg == "" and pr.verify(y.to(gp.BF16), False)[0] == ""
    assert [p for _, p in pr.hot] == gp.hot_positions(hidden // 4)
    for row, p in pr.hot:
        for defect in ({"drop_mean": p}, {"drop_var": p}):                 # (1), (2) a chunk dropped from the mean / the variance
            bad = pr.restate(**defect)
            assert pr.verify(bad, True)[0] and pr.verify(bad.to(gp.BF16), False)[0], (defect, "goes unseen")
    bad = pr.restate(one_pass=True)                                        # (3) one-pass fp32 variance: the LARGE-MEAN row
    msg, ratio = pr.verify(bad, True)
    print(f"ln-h{hidden}: one-pass variance at {ratio:.0f} x E")
    assert msg and pr.verify(bad.to(gp.BF16), False)[0]
    assert ratio >= 4 and float(((bad[0] - pr.ref[0]).abs() / pr.E[0]).max()) == ratio         # far outside, and on row 0


# ---------------------------------------------------------------- RoPE table
@pytest.mark.parametrize("case", gp.TABLE_CASES, ids=ids)
def test_rope_table_probe(case):
    pr = gp.probe(case)
    msg, ratio = pr.verify(*pr.restate())
    assert msg == "", msg
    assert pr.verify(*pr.restate(pos_shift=1))[0]                          # (2) position + 1
    if case.group in ("edges", "seeded"):
        assert pr.pos.min() >= 4095 and pr.pos.max() <= 131071
        assert pr.verify(*pr.restate(wrong_factors=True))[0]               # (1) the other factor set
        msg, r = pr.verify(*pr.restate(reduce_f32=True))                   # (3) fp32 range reduction before the cosine
        print(f"{case.id}: restatement at {ratio:.3f} of the bound, fp32 range reduction at {r:.0f} x")
        assert msg and r >= 100


def test_rope_table_cases_cover_the_issue():
    assert {(c.half, c.factors) for c in gp.TABLE_CASES} == {(h, f) for h in (16, 32, 48) for f in ("short", "long")}
    edges = gp.table_positions("edges")
    assert edges.max() == 131071 and {4095.0, 4097.0, 8191.0, 8193.0} <= set(edges.tolist())
    lp = gp.table_positions("leftpad")
    assert (lp[:201] == 0).all() and lp[201] == 1 and lp[-1] == 319
    ext = gp.table_positions("extended")
    assert ext[:4].tolist() == [1, 1, 1, 0] and ext[11:14].tolist() == [8, 9, 10]
    for half in gp.ROPE_HALF:                                              # full blocks of 256 threads, and a partly filled last one
        sizes = {gp.table_positions(g).numel() * half % 256 == 0 for g in gp.ROPE_GROUPS}
        assert sizes == {True, False}


# ---------------------------------------------------------------- split + rotation + append
ROPE_DEFECTS = ({"sin_sign": -1}, {"partner_next": True}, {"pos_shift": 1}, {"row_b": True}, {"scale_after": True}, {"scale_keys": True})


@pytest.mark.parametrize("case", gp.ROPE_CASES, ids=ids)
def test_rope_append_probe(case):
    pr = gp.probe(case)
    shares = [gp.unique_share(pr.q_lo, pr.q_hi), gp.unique_share(pr.k_lo, pr.k_hi)]
    print(f"{case.id}: bracket is one value on {100 * min(shares):.2f} %")
    assert min(shares) >= 0.98
    assert pr.verify(pr.emulate()) == "", pr.verify(pr.emulate())
    assert case.dst_t % 8 == 0 and case.dpos0 + case.L <= case.dst_t and case.past + case.L < case.tab_t
    # the sentinel sees a stray write: one element behind the window, one in each guard band
    flat = pr.emulate()
    if case.dpos0 + case.L < case.dst_t:
        flat["k"][gp.GUARD:].view(-1)[(case.dpos0 + case.L) * case.hd] = 0
        assert "outside the window" in pr.verify(flat)
    for name in ("q", "k", "v"):
        for at in (gp.GUARD - 1, -gp.GUARD):
            flat = pr.emulate()
            flat[name][at] = 0
            assert f"{name}: 1 elements outside the window" in pr.verify(flat)
    flat = pr.emulate()
    flat["v"][gp.GUARD + case.dpos0] = 7.0                                  # V: bit-exact
    assert "V is not a bit-exact copy" in pr.verify(flat)
    if case.null:
        assert torch.equal(pr.q_lo.view(torch.int16), pr.q_hi.view(torch.int16))                # a copy: the bracket is the value
        return
    turns = case.base + case.past + case.L > 1                             # position 0 alone: sin = 0, nothing to flip or to pair
    applies = {"sin_sign": turns, "partner_next": turns, "row_b": case.tab_div > 1, "scale_after": case.prescale, "scale_keys": case.prescale}
    for defect in ROPE_DEFECTS:
        if applies.get(next(iter(defect)), True):
            assert pr.verify(pr.emulate(**defect)), (defect, "goes unseen")


def test_rope_append_cases_cover_the_issue():
    cs = gp.ROPE_CASES
    assert 35 <= len(cs) <= 45
    assert {c.L for c in cs} == {1, 31, 32, 63, 64, 65, 130} and {c.hd for c in cs} == {32, 64, 96}
    assert {(c.nh, c.nkv) for c in cs} == {(4, 4), (8, 2), (3, 1)} and {c.B for c in cs} == {1, 3, 6}
    assert {c.past for c in cs} == {0, 8, 13}
    assert {(c.L, c.past) for c in cs if c.past % 8 and c.off_is_past and not c.dev_past} >= {(L, 13) for L in gp.ROPE_L}
    for flag in ("dev_past", "prescale", "null"):
        assert {getattr(c, flag) for c in cs} == {False, True}
    assert {c.off_is_past for c in cs} == {False, True} and all(c.dst_t == 8 * -(-c.L // 8) for c in cs if not c.off_is_past)
    assert {(c.tab_div, c.B) for c in cs if c.tab_div > 1} == {(3, 6)} and all(gp.probe(c).cos.shape[0] == 2 for c in cs if c.tab_div > 1)
    assert all(c.q_scale == 1.0 for c in cs if c.null)
    assert any(c.base + c.past >= 4096 for c in cs) and any(c.base < 4096 <= c.base + c.past + c.L for c in cs)
    for case in cs:                                                        # L on each side of the switch, with and without a V tile tail
        assert {c.L >= 32 for c in cs if c.hd == case.hd} == {False, True}
    from phi_3_vision_mlx_amd import ops
    assert ops.Q_PRESCALE == gp.Q_PRESCALE


# ---------------------------------------------------------------- vocabulary tail
@pytest.mark.parametrize("case", gp.VOCAB_CASES, ids=ids)
def test_vocab_probe(case):
    pr = gp.probe(case)
    n = case.n
    assert pr.verify_argmax(pr.restate_argmax()) == "", pr.verify_argmax(pr.restate_argmax())
    for k in gp.topk_ks(n):
        assert pr.verify_topk(pr.restate_topk(k), k) == "", pr.verify_topk(pr.restate_topk(k), k)
    for r, kind in enumerate(pr.kinds):
        if kind == "neginf":
            assert pr.argmax[r] == 0
        if kind.startswith("nan"):
            assert pr.argmax[r] == -1
        if kind.startswith("eight") and not pr.has_nan[r]:
            assert (pr.x[r].float() == gp.PEAK).sum() == 8 and (pr.x[r].float()[pr.topk(8)[r].long()] == gp.PEAK).all()
    ties = [r for r, kind in enumerate(pr.kinds) if kind in ("tie_vec_tail", "tie1024", "equal", "neginf") or kind.startswith("eight")]
    tail = [r for r, kind in enumerate(pr.kinds) if kind in ("maxlast", "maxtail")] if n % 8 and n > 1 else []
    if ties and n > 1:                                                     # (1) the last maximum wins instead of the first
        assert pr.verify_argmax(pr.restate_argmax(last_wins=True)) and pr.verify_topk(pr.restate_topk(1, last_wins=True), 1)
    if tail:                                                               # (2) the tail n % 8 ignored
        assert pr.verify_argmax(pr.restate_argmax(no_tail=True)) and pr.verify_topk(pr.restate_topk(1, no_tail=True), 1)


def test_vocab_cases_cover_the_issue():
    assert gp.VOCAB_N == (1, 7, 8, 9, 1023, 1024, 1025, 8200, 32064) and gp.VOCAB_ROWS == 9
    assert [gp.topk_ks(n) for n in (1, 7, 8, 9)] == [[1], [1, 3, 7], [1, 3, 8], [1, 3, 8]]
    want = {"max0", "maxlast", "maxvec", "maxtail", "tie_vec_tail", "tie1024", "neginf", "equal", "posinf", "nan_tail", "nan_mid"}
    for n in (1025, 8200):                                                 # everything fits there; 1025: the unaligned rows
        kinds = {k for v in gp.VOCAB_VARIANTS for k in gp.probe(gp.VocabCase(n, v)).kinds}
        assert want - ({"maxtail", "tie_vec_tail"} if n % 8 == 0 else set()) <= kinds and {"eight_head", "eight_tail", "eight_spread"} <= kinds
    pr = gp.probe(gp.VocabCase(1025, "nan"))
    assert pr.kinds[0] == "nan_tail" and pr.kinds[3] == "nan_mid" and (3 * 1025 * 2) % 16 != 0     # aligned row: tail; row 3: unaligned
    pr = gp.probe(gp.VocabCase(1025, "a"))
    assert pr.x[4, 1023] == gp.PEAK and pr.x[4, 1024] == gp.PEAK and pr.argmax[4] == 1023
    assert pr.x[5, 0] == gp.PEAK and pr.x[5, 1024] == gp.PEAK and pr.argmax[5] == 0


@pytest.mark.parametrize("case", gp.LSM_CASES, ids=ids)
def test_log_softmax_probe(case):
    pr = gp.probe(case)
    share = gp.unique_share(pr.lo, pr.hi)
    print(f"{case.id}: bracket is one value on {100 * share:.2f} %")
    assert share >= 0.98
    assert pr.verify(pr.restate()) == "", pr.verify(pr.restate())
    neg = pr.x.float() == -float("inf")
    assert (pr.lo.float()[neg] == -float("inf")).all() and (pr.hi.float()[neg] == -float("inf")).all()
    assert torch.isfinite(pr.lse).all()
    if case.n > 1:
        assert pr.verify(pr.restate(keep_f32=True))                        # (1) lse not rounded to bf16
    if case.n % 1024:
        assert pr.verify(pr.restate(no_tail=True))                         # (2) the tail n % 1024 left out of the sum


def test_cls_probe():
    for case in gp.CLS_CASES:
        pr = gp.probe(case)
        assert pr.verify(pr.want) == "" and pr.verify(pr.x) != ""
        assert torch.equal(pr.want[:, 1:], pr.x[:, 1:]) and pr.want.shape == (case.n_img, 7, case.dim)
