"""Split-KV decode attention against plain fp64 at the shapes the model runs (8k - 32k keys, 24 / 40 / 48 / 128 splits, splits
without keys, a short live length inside a large capacity, B = 16 ragged), on the probing inputs of tests/attn_probe.py:
the output is O(1) and moves by at least 4x the tolerance when a single planted key is lost, a dead key leaks or a split is
merged with the wrong weight (tests/test_attn_probe_cpu.py asserts that on the reference alone).

Tolerance: the project's `rtol 2^-6, atol 2e-2`.  The bf16 kernels sit at 0.07 - 0.18 of it.  The int8 kernels round the rotated
query to fp16 (from the exact rotation) where the plain reference rounds it to bf16: on these inputs a planted key scores ~11 and
half a bf16 ulp of q moves its weight by up to 2 %, so the int8 cases sit at 0.1 - 1.14 of the tolerance -- and within 0.03 of it of
where the fp64 restatement of the kernels' documented roundings (attn_probe.restated: fp16 q, fp16 P x V scale) sits on the CPU, case
by case.  Two cases, both with 16 new rows on one-dim blocks, miss the plain tolerance for that reason (measured 1.081 and 1.140; the
restatement alone 1.083 and 1.137, no kernel involved) and are widened to twice the restatement's worst error, WIDENED below;
tests/test_attn_probe_cpu.py holds those factors to the restatement."""
import pytest
import torch

import attn_probe as ap

pytestmark = pytest.mark.gpu


# case id -> factor on (rtol, atol): 2 x the worst error / tolerance of attn_probe.restated() against the plain reference (CPU)
WIDENED = {"q8-cap8256-s40-past8230-L16-B1-dpast40-mergelaunch": 2 * 1.083,
           "q8-cap640-s2-past320-L16-B16-pads-dpast40-mergelaunch": 2 * 1.137}


@pytest.fixture(scope="module")
def ops():
    from phi_3_vision_mlx_amd import ops as o
    o.L.lib()
    return o


def _eq_outside(after, before, lo, hi, dim):
    """Every element outside [lo, hi) along `dim` is bit-identical."""
    n = before.shape[dim]
    return all(torch.equal(after.narrow(dim, a, z - a), before.narrow(dim, a, z - a)) for a, z in ((0, lo), (hi, n)) if z > a)


@pytest.mark.parametrize("case", ap.CASES, ids=lambda c: c.id)
def test_decode_attention_matches_fp64_on_probing_inputs(ops, case):
    pr = ap.probe(case)
    c, past, L = case, case.past, case.L
    res = ap.launch(ops, pr)
    out = res["out"]
    ratio = ap.worst_ratio(out, pr.ref) if torch.isfinite(out.float()).all() else float("inf")
    bound = WIDENED.get(c.id, 1.0)
    print(f"{c.id}: {c.kernel}: worst error / tolerance {ratio:.3f} (bound {bound:.3f})")
    assert ratio <= bound, f"{c.kernel}: worst error is {ratio:.2f}x the tolerance (rtol 2^-6, atol 2e-2) against fp64"
    assert (res["ws"] == -1).all()                                            # the workspace is left all-ones
    if c.fused:                                                               # a second launch on the same workspace: the same bits
        assert torch.equal(res["out2"].view(torch.int16), out.view(torch.int16))
    new = slice(past, past + L)
    if c.kind == "bf16":
        k, vt = res["caches"]
        err = (k[:, :, new].float() - pr.k_new.float()).abs()
        assert (err <= 1e-2 + 2 ** -7 * pr.k_new.float().abs()).all()         # appended K rows (close(..., atol=1e-2))
        assert torch.equal(vt[:, :, :, new], pr.v_new.transpose(2, 3))        # appended V: bit exact
        assert _eq_outside(k, pr.k, past, past + L, 2) and _eq_outside(vt, pr.vt, past, past + L, 3)
    else:
        k8, v8t, ks, vs = res["caches"]
        assert torch.allclose(ks[:, :, new], pr.ks_new, rtol=1e-6) and torch.allclose(vs[:, :, new], pr.vs_new, rtol=1e-6)
        assert (k8[:, :, new].int() - pr.k8_new.int()).abs().max() <= 1       # ties may round either way
        assert (v8t[:, :, :, new].int() - pr.v8_new.transpose(2, 3).int()).abs().max() <= 1
        assert _eq_outside(k8, pr.k8, past, past + L, 2) and _eq_outside(v8t, pr.v8t, past, past + L, 3)
        assert _eq_outside(ks, pr.ks, past, past + L, 2) and _eq_outside(vs, pr.vs, past, past + L, 2)
