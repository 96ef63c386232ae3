"""The probes of tests/quant_probe.py, checked on the references alone (no GPU).  For the int8 KV cache and the e4m3 activation quantiser
three things:
  * every cap holds on the references: the code brackets are one value on >= 98 % of the elements, GRID tokens are half exact ties, the
    maxima hit every hot dim, >= 3 of 4 norm rows are kept;
  * a straightforward torch-fp32 restatement of each kernel's documented arithmetic passes every rule -- for the int8 codes both the
    multiply form x fl(1 / s) and the divide form x / s;
  * every planted defect, applied to that restatement, fails some element of some case.
A kernel with such a defect therefore cannot pass tests/test_quant_kernels_gpu.py."""
import pytest
import torch

import glue_probe as gp
import quant_probe as qp

ids = lambda c: c.id


# ---------------------------------------------------------------- int8 KV: p3v_kv_quantize
@pytest.mark.parametrize("family", qp.FAMILIES)
@pytest.mark.parametrize("case", qp.KV_CASES, ids=ids)
def test_kv_quantize_probe(case, family):
    pr = qp.probe(case, family)
    c = case
    uniq, ties = pr.unique(), pr.tie_share()
    mul, div = pr.emulate("mul", "mul"), pr.emulate("div", "div")
    differ = float((mul["k8"] != div["k8"]).double().mean())
    print(f"{c.id} [{family}]: code bracket is one value on {100 * uniq:.2f} %, exact ties {100 * ties:.1f} %, multiply and divide form differ on {100 * differ:.3f} %")
    assert uniq >= 0.98
    hot = qp.hot_dims(c.hd)
    for name in ("k", "v"):                                                # the maxima walk the hot dims: all of them where the case has the tokens
        assert set(pr.at[name]) == set(hot) if qp.BH * c.n_tok >= 3 * len(hot) else set(pr.at[name]) <= set(hot)
        bh, j = pr.zero[name]
        assert bool((getattr(pr, name)[bh, c.t0 + j] == 0).all()) and float(pr.s[name][bh, j]) == 1.0
    src = torch.cat([pr.k, pr.v])
    outside = torch.ones(c.src_t, dtype=torch.bool)
    outside[c.t0:c.t0 + c.n_tok] = False
    assert bool((src[:, outside].float() == float(gp.to_bf16(torch.tensor(qp.OUTSIDE)))).all())
    if family == "grid":                                                   # s = 2^e: E = 0, the bracket is the round-half-to-even code
        assert uniq == 1.0 and (0.4 if c.n_tok > 1 else 0.25) <= ties <= 0.6 and differ == 0.0     # (n_tok = 1: two of the six tokens are the zero ones)
        assert bool((((pr.s["k"].view(torch.int32) & 0x7FFFFF) == 0)).all())
    for form_k, form_v in (("mul", "div"), ("mul", "mul"), ("div", "div"), ("div", "mul")):       # (2) both forms pass
        assert pr.verify(pr.emulate(form_k, form_v)) == "", (form_k, form_v, pr.verify(pr.emulate(form_k, form_v)))
    assert pr.verify(pr.emulate(), 0.0) == "" or family != "grid"


def _kv_fails(defect, families=qp.FAMILIES, cases=qp.KV_CASES):
    """The (case, family) pairs on which the defect is seen."""
    seen = []
    for case in cases:
        for family in families:
            pr = qp.probe(case, family)
            flat = pr.emulate(**defect)
            if flat is not None and pr.verify(flat):
                seen.append((case.id, family))
    return seen


def test_kv_quantize_every_defect_fails():
    n = len(qp.KV_CASES)
    trunc = _kv_fails({"rnd": "trunc"})
    assert len(trunc) == 2 * n, trunc                                      # truncation: every case, either family
    away = _kv_fails({"rnd": "away"}, families=("grid",))
    assert len(away) == n, away                                            # round-half-away: every GRID case
    pr = qp.probe(qp.KV_CASES[0], "grid")
    moved = float((pr.emulate(rnd="away")["k8"] != pr.emulate()["k8"]).double().mean()) * 320 / 197
    print(f"round-half-away moves {100 * moved:.1f} % of the GRID codes of the window")
    assert 0.2 <= moved <= 0.3
    for case in qp.KV_CASES:                                               # a maximum that misses one lane / chunk / pair half: every hot dim
        for family in qp.FAMILIES:
            pr = qp.probe(case, family)
            w = slice(case.t0, case.t0 + case.n_tok)
            live = torch.cat([pr.k[:, w], pr.v[:, w]]).reshape(-1, case.hd).float().abs()
            for d in sorted(set(live[live.amax(-1) > 0].argmax(-1).tolist())):       # (where the maxima of the non-zero tokens are)
                assert pr.verify(pr.emulate(miss=d)), (case.id, family, f"dim {d} missed goes unseen")
    multi = tuple(c for c in qp.KV_CASES if c.n_tok > 1)
    assert len(_kv_fails({"neighbour": True}, cases=multi)) == 2 * len(multi)              # the neighbour token's scale
    assert len(_kv_fails({"wrong_axis": True})) == 2 * n                   # V read along the wrong axis
    room = tuple(c for c in qp.KV_CASES if c.t0 + c.n_tok < min(c.src_t, c.dst_t))
    assert len(room) >= 5
    assert len(_kv_fails({"leak": True}, cases=room)) == 2 * len(room)     # a token beyond n_tok leaking into a scale
    assert len(_kv_fails({"one_past": True}, cases=room)) == 2 * len(room)  # a write one token past the window


# ---------------------------------------------------------------- int8 KV: p3v_kv_dequantize
@pytest.mark.parametrize("case", qp.DQ_CASES, ids=ids)
def test_kv_dequantize_probe(case):
    pr = qp.probe(case)
    uniq = pr.unique()
    print(f"{case.id}: bracket is one value on {100 * uniq:.3f} %")
    assert uniq >= 0.98
    for name in ("k", "v"):
        q = pr.codes[name][:, :max(case.n_tok, 1)]
        assert all(bool((q == v).any(-1).all()) for v in (0, 128, 255))
        s = pr.scales[name]
        assert float(s.min()) >= 2.0 ** -10 and float(s.max()) < 2.0 ** 3 and float((s.view(torch.int32) & 0xFF != 0).double().mean()) > 0.9
    assert pr.verify(pr.emulate()) == "", pr.verify(pr.emulate())
    assert pr.verify(pr.emulate(offset=127.0))                             # an offset of 127
    assert pr.verify(pr.emulate(neighbour=True))                           # the neighbour token's scale


# ---------------------------------------------------------------- int8 KV: the append paths
@pytest.mark.parametrize("case", qp.AP_CASES, ids=ids)
def test_append_probe(case):
    pr = qp.probe(case)
    uniq = pr.unique()
    print(f"{case.id}: code bracket is one value on {100 * uniq:.2f} %")
    assert uniq >= 0.98
    assert set(pr.fam.values()) == set(qp.FAMILIES)
    assert float(pr.s["v"][1, 1, 0]) == 1.0
    for form in ("mul", "div"):
        assert pr.verify(pr.emulate(form)) == "", pr.verify(pr.emulate(form))
    assert pr.verify(pr.emulate(rnd="trunc")) and pr.verify(pr.emulate(rnd="away")) and pr.verify(pr.emulate(neighbour=True))
    for d in (0, 1, 94, 95):                                               # lanes 0 and 47 of the key, lanes 0 / 63 / 31 of the value reads
        hit = any(int(x.float().abs().argmax()) == d for x in list(pr.new["k"].reshape(-1, 96)) + list(pr.new["v"].reshape(-1, 96)))
        assert not hit or pr.verify(pr.emulate(miss=d))


# ---------------------------------------------------------------- e4m3 activation quantiser
@pytest.mark.parametrize("case", qp.F8_CASES, ids=ids)
def test_quant_fp8_rows_probe(case):
    pr = qp.probe(case)
    kept, uniq = pr.shares()
    print(f"{case.id}: seed {pr.seed}, rows kept {100 * kept:.0f} %, code bracket one value on {100 * uniq:.2f} % of kept rows")
    assert kept >= qp.MIN_KEPT and uniq >= qp.MIN_UNIQUE
    assert pr.verify(pr.emulate()) == "", pr.verify(pr.emulate())
    if not case.norm:
        assert case.rows == 1 or (float(pr.s[0]) == 1.0 and bool((pr.codes[0] == 0).all()))
        return
    for row, p in pr.rms.hot:                                              # a dropped chunk at each hot position
        assert pr.verify(pr.emulate(drop=p)), f"chunk {p} dropped goes unseen"


def test_quant_fp8_rows_every_defect_fails():
    seen = {"skip_round": 0, "amax_before_w": 0, "per_element_inv": 0}
    for case in qp.F8_CASES:
        pr = qp.probe(case)
        for d in seen:
            if d != "per_element_inv" and not case.norm:
                continue
            seen[d] += bool(pr.verify(pr.emulate(**{d: True})))
    print(seen)
    norm_big = sum(1 for c in qp.F8_CASES if c.norm and c.hidden > 8)
    assert seen["skip_round"] >= norm_big - 6 and seen["amax_before_w"] >= norm_big - 6       # (one-row cases may miss by chance)
    assert seen["per_element_inv"] >= len(qp.F8_CASES) // 4                                     # (0.03 % of the codes of a row: a matter of rows)
    for hidden in (520, 3064, 3072, 3080, 8192):                           # and the 33-row case of every size sees each of them
        for norm in (False, True):
            pr = qp.probe(qp.F8Case(hidden, 33, norm))
            assert pr.verify(pr.emulate(per_element_inv=True))
            if norm:
                assert pr.verify(pr.emulate(skip_round=True)) and pr.verify(pr.emulate(amax_before_w=True))
                assert [p for _, p in pr.rms.hot] == gp.hot_positions(hidden // 8)
