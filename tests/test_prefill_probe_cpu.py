"""The probing inputs of tests/prefill_probe.py, checked on the fp64 reference alone (no GPU): for every case of the prompt attention
parity table a reference that is wrong in one specific way -- a key lost, the causal or the pad boundary off by one, `past` ignored, a
64-key tile of K or of V^T stale by a ring depth, skipped or counted twice, a kv head, batch row or query row read from the neighbour --
misses `rtol 2^-6, atol 2e-2` by 4x at least in some live element.  A kernel with such a defect cannot pass
test_attn_prefill_probe_gpu.py.

What "every" means below, and what arithmetic rules out:
  * lost key: every visible key of every (batch row, kv head) -- each kv head is probed by all three query families.
  * causal boundary: every live row -- but in the one TILE-only case (head_group < nh, spot rows), where a query whose primary tile lies
    wholly below its own position does not look at its boundary: there, the rows whose primary tile is their diagonal tile.  The mask code is
    the same for every head_group; the ten other cases probe it on every row.
  * `past` off by one is the causal boundary off by one (the kernels use `past` for nothing else); both directions are tried there.
  * a tile counted twice cannot show where it is the only tile a row of the batch sees (the output is a ratio): asserted for every tile
    of every batch row that sees two tiles or more."""
import pytest
import torch

import prefill_probe as pp

MARGIN = 4.0


def _row_moves(pr, wrong):
    """[B, R]: worst move / tolerance of each query row over its heads and elements."""
    return ((wrong - pr.o).abs() / pr.tol()).amax(-1).amax(1)


@pytest.mark.parametrize("case", pp.CASES, ids=lambda c: c.id)
def test_probe_inputs_catch_every_mutant(case):
    pr = pp.probe(case)
    c, B, L, past, T, Tc = case, case.B, case.L, case.past, case.T, pr.Tc
    grp, R = c.nh // c.nkv, len(pr.rows)
    rows = torch.tensor(pr.rows)
    pad = torch.tensor(c.pad)
    live = pr.live
    n_vis = pr.vis.sum(-1)                                                     # [B, R]
    worst = {}

    def need(name, ratios, where=None):
        """Every entry of `ratios` (where `where`) is MARGIN at least."""
        sel = ratios if where is None else ratios[where]
        if sel.numel():
            worst[name] = float(sel.min())
            assert worst[name] >= MARGIN, f"{name}: moves the output by {worst[name]:.2f}x the tolerance only"

    # ---- the reference itself
    assert torch.isfinite(pr.ref).all() and float(pr.ref.abs().max()) <= 16.0
    assert (pr.ref[~live] == 0).all() and bool((n_vis[live] > 0).all()) and bool((n_vis[~live] == 0).all())
    assert (pr.k[:, :, T:] == pp.POISON).all() and (pr.vt[:, :, :, T:] == pp.POISON).all() and c.past_t == (T + 63) // 64 * 64 + 128
    for b in range(B):
        assert (pr.k[b, :, :c.pad[b]] == pp.POISON).all() and (pr.vt[b, :, :, :c.pad[b]] == pp.POISON).all()
    if c.spot:
        assert R == 2 * ((L + 255) // 256) + 64 and c.head_group < c.nh

    # ---- a single key lost: every visible key of every (row, kv head)
    lost = pr.lost_key_moves()
    for b in range(B):
        need(f"key lost (row {b})", lost[b, :, c.pad[b]:T])

    # ---- the causal boundary (equally: `past`) off by one, either way: every live row, with two visible keys where one gets hidden
    if c.causal:
        own = (past + rows)[None].expand(B, R)
        nxt = torch.where(own + 1 < Tc, own + 1, torch.full_like(own, -1))     # (the key after the last tile is never walked)
        short, far = live & (n_vis >= 2), live & (nxt >= 0)
        if c.tile_only:                                                        # no UP rows: the rows whose primary tile is their diagonal tile
            diag = torch.from_numpy(pr.primary)[:, :, rows].eq(own[:, None] // 64).any(1)
            short, far = short & diag, far & diag & (nxt // 64 == own // 64)
            assert int(short.sum()) >= 16 and int(far.sum()) >= 4
        need("causal boundary one short", _row_moves(pr, pr.with_key(own, add=False)), short)
        need("causal boundary one far", _row_moves(pr, pr.with_key(nxt, add=True)), far)
    # ---- the pad boundary off by one, either way (seeing pad - 1 is seeing poison): every live row
    for b in range(B):
        if c.pad[b]:
            only_b = torch.arange(B)[:, None] == b
            first = torch.where(only_b, pad[:, None].expand(B, R), torch.full((B, R), -1))
            need(f"pad boundary one far (row {b})", _row_moves(pr, pr.with_key(first, add=False))[b], (live & (n_vis >= 2))[b])
            need(f"pad boundary one short (row {b})", _row_moves(pr, pr.with_key(first - 1, add=True))[b], live[b])
    # ---- `past` ignored
    if past:
        wrong = pr.attend(pr.s, pr.visible(past=0), pr.vd)[0]
        need("past ignored", _row_moves(pr, wrong), live)

    # ---- a whole tile stale by a ring depth (K alone, V^T alone), skipped, counted twice: every tile index of every batch row
    for b in range(B):
        per = {}
        for h in range(c.nh):
            for name, r in pr.tile_mutants(b, h).items():
                per[name] = torch.maximum(per.get(name, torch.zeros_like(r)), r)
        lo_t, hi_t = c.pad[b] // 64, (T - 1) // 64
        if c.pad[b] >= T:
            continue
        for name, r in per.items():
            d = int(name.split()[-2]) if name.endswith("before") else 0
            if name == "counted twice" and bool((pr.vis[b].view(R, -1, 64).any(-1).sum(-1) <= 1).all()):
                continue
            need(f"tile {name} (row {b})", r[max(lo_t, d):hi_t + 1])

    # ---- a wrong operand
    if c.nkv > 1:                                                              # the next kv head: its K alone, its V^T alone
        by_kvh = lambda o: (((o - pr.o).abs() / pr.tol()).amax(-1) * live[:, None]).view(B, c.nkv, grp, R).amax(-1).amax(-1)
        need("K of the next kv head", by_kvh(pr.attend(pr.scores(pr.kd.roll(-1, 1)), pr.vis, pr.vd)[0]))
        need("V^T of the next kv head", by_kvh(pr.attend(pr.s, pr.vis, pr.vd.roll(-1, 1))[0]))
    if B > 1:                                                                  # batch row b reads K and V^T of row b + 1 / b - 1
        for sh in (1, -1):
            wrong = pr.attend(pr.scores(pr.kd.roll(sh, 0)), pr.vis, pr.vd.roll(sh, 0))[0]
            need(f"batch row {'b - 1' if sh > 0 else 'b + 1'}", _row_moves(pr, wrong).amax(-1))
    if not c.spot:                                                             # query rows r and r + 16 of a block swapped
        r = torch.arange(L - 16)
        r = r[(r // 128 == (r + 16) // 128) & (r % 32 < 16)]
        if r.numel():
            diff = ((pr.o[:, :, r] - pr.o[:, :, r + 16]).abs() / torch.minimum(pr.tol()[:, :, r], pr.tol()[:, :, r + 16])).amax(-1).amax(1)
            need("query rows r and r + 16 swapped", diff, (live[:, r] | live[:, r + 16]))
    print(f"{c.id}: max |ref| {float(pr.ref.abs().max()):.2f}; weakest mutant {min(worst.values()):.1f}x the tolerance "
          f"({min(worst, key=worst.get)}); weakest lost key {min(v for k, v in worst.items() if k.startswith('key lost')):.1f}x")


def test_case_table_reaches_every_mechanism():
    """The shapes of the table are the ones the mechanisms need: a ragged last 256-row block, a block of one query, pads inside a tile and
    over a whole past, cached calls, head dim 64 without a mask, GQA, one tile, fewer queries than a wave, and head_group < nh under the
    library's own rule (csrc/p3v_attn_prompt.hip, prompt_route: kv_bytes * nh > 64 MiB; Case.head_group asks the route)."""
    by = {c.id: c for c in pp.CASES}
    assert by["B1-L700-hd96"].n_tiles == 11 and 700 % 256 not in (0, 1)
    assert by["B1-L257"].L % 256 == 1
    assert 64 < by["B2-L300-pads0,77"].pads[1] < 128
    assert by["B2-L33-past100-pads3,100"].pads[1] == by["B2-L33-past100-pads3,100"].past
    c = by["B3-L577-hd64-noncausal"]
    assert (c.B, c.L, c.hd, c.nh, c.causal) == (3, 577, 64, 3, False)
    c = by["B1-L5632-nh32-headgroup8"]
    assert c.T * c.hd * 4 * c.nh > 64 << 20 and c.head_group == 8
    assert all(c.L > 16 for c in pp.CASES)                                     # above P3V_DECODE_MAX_L: the prompt path
    assert set(pp.PATHS) == set(pp.KERNELS) == {"dma", "il4", "il8", "pp"}
