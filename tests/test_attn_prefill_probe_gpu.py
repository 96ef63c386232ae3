"""The prompt-sized attention kernels behind p3v_attention against plain fp64, in the instantiations the model launches (pre-scaled Q,
keys from the cache), on the probing inputs of tests/prefill_probe.py: the output is O(1) and moves by at least 4x the tolerance when a
single key is lost, a causal or pad boundary is off by one, a K or V^T tile is stale by a ring depth, skipped or counted twice, or a kv
head, batch row or query row is read from the neighbour (tests/test_prefill_probe_cpu.py asserts that on the reference alone).

Every case runs on the four pinned paths: k_attn_prefill_dma, k_attn_prefill_il with 4 and with 8 waves, k_attn_prefill_pp.
Tolerance: the project's `rtol 2^-6, atol 2e-2`, on every case; what the kernels round (P to bf16 before P x V, the output once,
include/p3v.h) stays far inside it: measured 0.19 - 0.27 of the tolerance over the 44 (case, path) pairs
(profiles/prefill_probe_parity.txt), so no case carries a restated rounding or a widened bound."""
import pytest
import torch

import prefill_probe as pp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from phi_3_vision_mlx_amd import ops as o
    o.L.lib()
    return o


@pytest.mark.parametrize("path", list(pp.PATHS))
@pytest.mark.parametrize("case", pp.CASES, ids=lambda c: c.id)
def test_prefill_attention_matches_fp64_on_probing_inputs(ops, case, path):
    pr = pp.probe(case)
    c, n = case, case.B * case.L * case.nh * case.hd
    res = pp.launch(ops, pr, path)
    out = res["out"]
    kernel = pp.kernel_of(path, c.hd)
    # ---- accuracy over the live rows (the spot rows where the reference is built for those alone)
    got = out[:, pr.rows].double()
    finite = bool(torch.isfinite(out.float()).all())
    ratio = pp.worst_ratio(got[pr.live], pr.ref[pr.live]) if finite else float("inf")
    print(f"{c.id}: {kernel}: {c.n_tiles} tiles: worst error / tolerance {ratio:.3f}")
    assert finite, f"{kernel}: the output holds a NaN or an infinity"
    assert ratio <= 1.0, f"{kernel}: worst error is {ratio:.2f}x the tolerance (rtol 2^-6, atol 2e-2) against fp64"
    # ---- nothing else touched
    pad_rows = torch.tensor([[c.past + i < c.pad[b] for i in range(c.L)] for b in range(c.B)])
    assert (out[pad_rows].view(torch.int16) == 0).all()                       # padded query rows: exactly 0
    buf, buf0 = res["buf"].view(torch.int16), res["buf0"].view(torch.int16)
    assert torch.equal(buf[:pp.GUARD], buf0[:pp.GUARD]) and torch.equal(buf[pp.GUARD + n:], buf0[pp.GUARD + n:])
    assert torch.equal(res["k"].view(torch.int16), pr.k.view(torch.int16))    # K and V^T as they were, poison included
    assert torch.equal(res["vt"].view(torch.int16), pr.vt.view(torch.int16))
    # ---- a second launch on the same inputs: the same bits
    assert torch.equal(res["out2"].view(torch.int16), out.view(torch.int16))
