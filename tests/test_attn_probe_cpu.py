"""The probing inputs of tests/attn_probe.py, checked on the fp64 reference alone (no GPU): for every case of the decode
attention parity table a reference that is wrong in one specific way -- a planted key lost, a key leaking through the padding,
the live length or the causal mask, a split merged with the wrong weight -- misses `rtol 2^-6, atol 2e-2` by 4x at least
in some element, and every query's output is O(1).  A kernel with such a defect therefore cannot pass test_attn_probe_gpu.py."""
import math

import pytest
import torch

import attn_probe as ap

MARGIN = 4.0


@pytest.mark.parametrize("case", ap.CASES, ids=lambda c: c.id)
def test_probe_inputs_catch_every_mutant(case):
    pr = ap.probe(case)
    c, ref = case, pr.ref
    B, L, past = c.B, c.L, c.past
    assert torch.isfinite(ref).all()
    # ---- the planted positions cover what the issue lists
    at = [{p.t for p in pr.planted if p.b == b} for b in range(B)]
    for b in range(B):
        need = {c.pad[b], past - 1} | set(range(past, past + L))
        edges = [t for t in range(64, past, 64) if t % c.chunk and t - 1 >= c.pad[b]]
        if edges:
            need |= {edges[0] - 1, edges[0]}
        assert need <= at[b], (b, sorted(need - at[b]))
    n_live = 0
    for s in range(c.n_split):
        rows = [b for b in range(B) if ap.live_range(c, b, s)[0] < ap.live_range(c, b, s)[1]]
        n_live += bool(rows)
        assert not rows or any({ap.live_range(c, b, s)[0], ap.live_range(c, b, s)[1] - 1} <= at[b] for b in rows), f"split {s}"
    # ---- every query's output is O(1)
    per_query = ref.view(B, L, ap.NH, ap.HD).abs().amax(-1)
    assert 0.25 <= float(per_query.min()) and float(per_query.max()) <= 4.0, (float(per_query.min()), float(per_query.max()))
    worst = {}

    def mutant(name, wrong, true=ref):
        r = ap.worst_ratio(wrong, true)
        worst[name] = min(worst.get(name, math.inf), r)
        assert r >= MARGIN, f"mutant {name}: misses the tolerance by {r:.2f}x only"

    # (a) any single planted key removed
    for p in pr.planted:
        wrong, true = pr.without_key(p)
        mutant(f"(a) key {p.t} of kv head {p.kvh}, row {p.b}, removed", wrong, true)
    vis = pr.visible()
    # (b) key pad_len[b] - 1 visible
    for b in range(B):
        if c.pad[b]:
            v = vis.clone()
            v[b, :, c.pad[b] - 1] = True
            mutant(f"(b) row {b}", pr.attend(v))
    # (c) key past + L visible (the first dead one), where the capacity has one
    if past + L < c.cap:
        v = vis.clone()
        v[:, :, past + L] = True
        mutant("(c)", pr.attend(v))
    # (d) the last new key visible to row i < L - 1
    for i in range(L - 1):
        v = vis.clone()
        v[:, i, past + L - 1] = True
        mutant(f"(d) row {i}", pr.attend(v))
    # (e) one split's partial merged with weight 1 (two live splits at least: with one there is nothing to weigh)
    m, l, O = pr.split_partials()
    assert ap.worst_ratio(pr.merge(m, l, O), ref) < 1e-6               # the split form is the same function
    if n_live >= 2:
        for s in range(c.n_split):
            if bool((l[..., s] > 0).any()):
                mutant(f"(e) split {s}", pr.merge(m, l, O, unit=s))
    print(f"{c.id}: max|ref| per query {float(per_query.min()):.3f} .. {float(per_query.max()):.3f}; weakest mutant "
          f"{min(worst.values()):.1f}x the tolerance ({min(worst, key=worst.get)})")


# (kind, capacity, n_split) -> (batch of the plan, in-launch merge in the plan, kernel): the table of the GPU parity cases.
# (int8, 640 keys: the model's plan has 2 splits from B = 20 on and 3 at B = 16; the cases run both at B = 16.)
PLANS = {("bf16", 33280, 24): (1, False, "k_attn_decode_stream"), ("bf16", 8256, 24): (1, False, "k_attn_decode_stream"),
         ("bf16", 640, 2): (16, True, "k_attn_decode_stream"), ("bf16", 6144, 48): (1, True, "k_attn_decode128"),
         ("bf16", 8192, 128): (1, False, "k_attn_decode"),
         ("q8", 33280, 40): (1, False, "k_attn_decode_q8"), ("q8", 8256, 40): (1, False, "k_attn_decode_q8"),
         ("q8", 2688, 21): (1, True, "k_attn_decode128_q8"), ("q8", 1024, 16): (1, True, "k_attn_decode_q8s"),
         ("q8", 1088, 17): (1, True, "k_attn_decode_q8"), ("q8", 640, 2): (20, True, "k_attn_decode_q8"),
         ("q8", 640, 3): (16, True, "k_attn_decode_q8")}


def test_case_table_is_the_models_split_plan(monkeypatch):
    """Every (capacity, n_split) of the case table is what the split plan of model._plan yields for the full 32-head model at that capacity
    and batch, with the merge form named in the table, and reaches the kernel named there (the launcher's rule on (cap, n_split))."""
    from types import SimpleNamespace

    from phi_3_vision_mlx_amd.model import AttnPlan, Phi3VModel
    for name in ("P3V_ATTN_TILE128", "P3V_ATTN_NSPLIT", "P3V_ATTN_FUSED_MERGE", "P3V_PROFILING"):
        monkeypatch.delenv(name, raising=False)
    model = SimpleNamespace(cfg=SimpleNamespace(num_attention_heads=ap.FULL_NH), hd=ap.HD, device="cpu", serving=False, _alloc_bufs=lambda B, L: {"plan": AttnPlan()})
    assert {(c.kind, c.cap, c.n_split) for c in ap.CASES} == set(PLANS)
    for c in ap.CASES:
        plan_B, plan_fused, kernel = PLANS[c.kind, c.cap, c.n_split]
        assert (c.plan_B, c.plan_fused) == (plan_B, plan_fused) and c.kernel.split()[0] == kernel, c.id
    for (kind, cap, n_split), (plan_B, plan_fused, _) in PLANS.items():
        st = SimpleNamespace(Tp=cap, quantized=kind == "q8", serving=False, family=None)
        plan = Phi3VModel._plan(model, st, plan_B, 1, fuse_o=False)["plan"]
        assert (plan.n_split, plan.attn_merge) == (n_split, plan_fused), (kind, cap, plan.n_split, plan.attn_merge)
    # both merge forms wherever the launcher has both
    for key in (("bf16", 33280), ("bf16", 8256), ("bf16", 640), ("bf16", 6144), ("q8", 2688), ("q8", 1024)):
        assert {c.fused for c in ap.CASES if (c.kind, c.cap) == key} == {False, True}, key


def test_widened_cases_are_twice_the_restatement_at_most():
    """The two int8 cases whose tolerance is widened (tests/test_attn_probe_gpu.py): the factor is at most twice the worst error of
    the fp64 restatement of the kernels' documented roundings against the plain reference -- and the restatement itself misses the plain
    tolerance there, which is why they are widened at all."""
    import test_attn_probe_gpu as gpu
    by_id = {c.id: c for c in ap.CASES}
    assert set(gpu.WIDENED) <= set(by_id) and all(by_id[i].kind == "q8" for i in gpu.WIDENED)
    for cid, factor in gpu.WIDENED.items():
        pr = ap.probe(by_id[cid])
        r = ap.worst_ratio(ap.restated(pr), pr.ref)
        print(f"{cid}: restatement at {r:.3f} of the tolerance, widened to {factor:.3f}")
        assert 1.0 < r and factor <= 2 * r + 1e-3
