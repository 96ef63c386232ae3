"""What guided decoding costs on the full-size synthetic model (2531-token context by default), at B = 1 / 8 / 16, in ONE call: the
penalised step with every row inactive (the step a guided state would otherwise take), the guided step with every guide row
inactive, with a 3-state guide on every row, with a 255-state guide on every row, and with two WIDE guides on every row (a compiled
JSON schema of several hundred states and a hand-built guide exactly at the entry bound, S = 1023 and C = 63) -- all graph replays on ONE state (the
captures share the greedy capture's loop-state buffers), walked in turn, every region rewound to the SAME cache length and every
guide record back at its start state, medians of the repeated regions -- and the p3v_guide_mask launch alone (eager, on the
step's own adjusted-logits buffer: inactive rows, DONE rows, the 3-state and the 255-state guide at their start states).

--parent DIR: a built checkout of the PARENT commit.  Its package is loaded beside this one (own library, own model with the same
seed) and its penalised step with the same rows inactive is measured in the same run, alternated with the others: the yardstick
the guided steps are held against.  Its own 3-state and 255-state guided steps are measured in the same alternation, and its
p3v_guide_mask launch alone between two rounds of this tree's, so the narrow guides of the two trees stand side by side.  Without it the tree's own penalised step -- code this feature does not touch -- is the only
yardstick.

The 3-state guide is `([a-y]*z[a-z])*` and the 255-state one `[a-z]{254}`: neither lets a row finish inside a region other than by
a rare EOS in the first one's accepting state; a finished row costs less (a DONE row stages no table), so the rows DONE at the end
of the last region are reported with the times.

    python tools/guide_step_time.py [--batches 1,8,16] [--ctx 2531] [--steps 40] [--reps 5] [--parent DIR]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from phi_3_vision_mlx_amd import guide, ops, penalties, sampling  # noqa: E402
from phi_3_vision_mlx_amd.api import ID_EOS, load_synthetic  # noqa: E402

SMALL, LARGE = "([a-y]*z[a-z])*", "[a-z]{254}"
# a nested object plus an array of up to four 3-field objects: several hundred states, a wide guide
SCHEMA = {"type": "object", "properties": {
    "owner": {"type": "object", "properties": {"name": {"type": "string", "maxLength": 26}, "id": {"type": "integer"}}, "required": ["name", "id"]},
    "entries": {"type": "array", "maxItems": 4, "items": {"type": "object", "properties": {
        "label": {"type": "string"}, "count": {"type": "integer"}, "kept": {"type": "boolean"}}, "required": ["label", "count", "kept"]}}},
    "required": ["owner", "entries"]}


def bound_guide():
    """A hand-built guide exactly at the wide entry bound: 1023 states, 63 byte classes (62 letters and digits, each with a column
    of its own, and the dead column); every letter or digit steps on, so no row finishes inside a region."""
    import numpy as np
    S = 1023
    d = np.zeros((S + 1, 256), dtype=np.uint16)
    for k, b in enumerate(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789"):
        d[1:S, b] = np.arange(2, S + 1)
        d[k + 1, b] = min(k + 3, S)                                 # (one entry apart: the column is no other byte's)
    acc = np.zeros(S + 1, dtype=np.uint8)
    acc[S] = 1
    dfa = guide.Dfa(d, acc, "hand-built: 1023 states, 63 classes")
    assert dfa.n_classes == 63 and (S + 1) * 64 == guide.WIDE_MAX_ENTRIES
    return dfa


def load_parent(path):
    """The package of another checkout under a name of its own (its relative imports and its libp3v.so stay its own)."""
    import types
    pkg = os.path.join(path, "phi-3-vision-mlx_amd")
    if not os.path.exists(os.path.join(pkg, "libp3v.so")):
        raise SystemExit(f"--parent: {pkg} holds no libp3v.so (build that checkout first)")
    mod = types.ModuleType("p3v_parent")
    mod.__path__ = [pkg]                             # (the package directory has no __init__: a bare package, as the import shim makes)
    sys.modules["p3v_parent"] = mod
    mod.api = importlib.import_module("p3v_parent.api")
    mod.sampling = importlib.import_module("p3v_parent.sampling")
    mod.penalties = importlib.import_module("p3v_parent.penalties")
    mod.guide = importlib.import_module("p3v_parent.guide")
    mod.ops = importlib.import_module("p3v_parent.ops")
    return mod


def timed(fn, tok, cache, n, model, start):
    cache[0].state.offset = start                    # every region starts at the same cache length and at step 0
    model.restart_history(cache[0].state)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        _, tok = fn(tok, cache)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n, tok


def launches_us(fn, n=100, warm=5):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(warm):
        fn()
    ev0.record()
    for _ in range(n):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) * 1e3 / n


def prepare(model, samp, pen, ids, budget):
    """prefill, T-only sampling records, a penalty state whose rows are all inactive"""
    logits, cache = model(input_ids=ids, max_tokens=budget)
    st = cache[0].state
    B = ids.shape[0]
    model.set_sampling(st, samp.pack(samp.rows(B, 1.0, 0, 1.0, 1234), 1))
    model.set_penalties(st, pen.pack(pen.rows(B)), ids.numpy(), 0)
    return cache, st, logits


def steps(model, processor, parent, a):
    V = model.cfg.vocab_size
    table = guide.vocab_for(processor.tokenizer, V)
    model.set_guide_vocab(table, ID_EOS)
    small, large = guide.checked(guide.compile_regex(SMALL), table, ID_EOS), guide.checked(guide.compile_regex(LARGE), table, ID_EOS)
    assert (small.n_states, large.n_states) == (3, 255)
    wide_json, wide_bound = guide.checked(guide.compile_json(SCHEMA), table, ID_EOS), guide.checked(bound_guide(), table, ID_EOS)
    assert wide_json.n_states > 255
    if parent is not None:
        p_guide = parent[3]
        p_table = p_guide.vocab_for(processor.tokenizer, V)
        parent[0].set_guide_vocab(p_table, ID_EOS)
        p_small, p_large = p_guide.compile_regex(SMALL), p_guide.compile_regex(LARGE)
        p_ops = parent[4]
    for B in [int(x) for x in a.batches.split(",")]:
        ids = torch.randint(3, 32000, (B, a.ctx), dtype=torch.int64, generator=torch.Generator().manual_seed(B))
        budget = a.steps + 8
        cache, st, logits = prepare(model, sampling, penalties, ids, budget)
        tok = ops.argmax(logits[:, -1].contiguous())[:, None]
        variants = [("penalised_inactive", model, model.penal_step, cache, False), ("guided_inactive", model, model.guide_step, cache, None),
                    ("guided_3_states", model, model.guide_step, cache, small), ("guided_255_states", model, model.guide_step, cache, large),
                    (f"guided_wide_json_{wide_json.n_states}_states", model, model.guide_step, cache, wide_json),
                    ("guided_wide_bound_1023_states", model, model.guide_step, cache, wide_bound)]
        toks = {"own": tok}
        if parent is not None:
            p_model, p_samp, p_pen = parent[:3]
            p_cache, p_st, p_logits = prepare(p_model, p_samp, p_pen, ids, budget)
            toks["parent"] = p_logits[:, -1].argmax(-1).to(torch.int32)[:, None]
            variants.insert(0, ("parent_penalised_inactive", p_model, p_model.penal_step, p_cache, False))
            variants.insert(4, ("parent_guided_3_states", p_model, p_model.guide_step, p_cache, p_small))
            variants.insert(6, ("parent_guided_255_states", p_model, p_model.guide_step, p_cache, p_large))
        done = {}

        def run(name, m, fn, c, dfa):
            key = "parent" if m is not model else "own"
            # every region is first fed a token without bytes (the tokenizer's prefix id): the last region's newest token -- an EOS,
            # a byte the next guide bans -- must not finish a row before its region starts
            toks[key] = torch.full_like(toks[key], 29871)
            if dfa is not False:
                m.set_guides(c[0].state, [dfa] * B)                                   # region and record, back at the start state
            t, toks[key] = timed(fn, toks[key], c, a.steps, m, a.ctx)
            if dfa:
                done[name] = int((c[0].state.guide["rows"][:, 2] < 1).sum())
            return t
        for v in variants:                                                              # capture + warm every graph
            run(*v)
        times = {v[0]: [] for v in variants}
        for _ in range(a.reps):
            for v in variants:
                times[v[0]].append(run(*v))
        # the kernel alone (eager launches on the step's own adjusted-logits buffer, nothing fed: the states stay)
        g, gd, adj, vt = st.graphs["greedy"], st.guide, st.penalty["adj"], model._guide_vocab
        alone = {}
        for name, dfa, state in (("inactive", None, 1), ("done", small, guide.DONE), ("3_states", small, 1), ("255_states", large, 1),
                                 ("wide_json", wide_json, 1), ("wide_bound", wide_bound, 1), ("wide_done", wide_bound, guide.DONE)):
            model.set_guides(st, [dfa] * B, states=[state] * B)
            alone[name] = launches_us(lambda: ops.guide_mask(adj, gd["rows"], gd["delta"], gd["accept"], vt["tok_off"], vt["tok_bytes"],
                                                             vt["eos"], fed=None, n_bytes=vt["n_bytes"]))
        if parent is not None:                                                         # the parent's launch alone, in the same run
            p_gd, p_adj, p_vt = p_st.guide, p_st.penalty["adj"], p_model._guide_vocab
            for name, dfa, state in (("inactive", None, 1), ("done", p_small, p_guide.DONE), ("3_states", p_small, 1), ("255_states", p_large, 1)):
                p_model.set_guides(p_st, [dfa] * B, states=[state] * B)
                alone["parent_" + name] = launches_us(lambda: p_ops.guide_mask(p_adj, p_gd["rows"], p_gd["delta"], p_gd["accept"], p_vt["tok_off"],
                                                                               p_vt["tok_bytes"], p_vt["eos"], fed=None, n_bytes=p_vt["n_bytes"]))
            for name, dfa, state in (("inactive", None, 1), ("done", small, guide.DONE), ("3_states", small, 1), ("255_states", large, 1)):
                model.set_guides(st, [dfa] * B, states=[state] * B)                     # ... and this tree's once more behind it
                alone[name + "_again"] = launches_us(lambda: ops.guide_mask(adj, gd["rows"], gd["delta"], gd["accept"], vt["tok_off"],
                                                                            vt["tok_bytes"], vt["eos"], fed=None, n_bytes=vt["n_bytes"]))
        model.set_guides(st, [large] * B, states=[100] * B)                            # mid-pattern, fed a letter each launch: the
        fed = torch.full((B,), 3 + ord("a"), dtype=torch.int32, device="cuda")         # state store included (it advances to 255 and stops)
        alone["255_states_fed"] = launches_us(lambda: ops.guide_mask(adj, gd["rows"], gd["delta"], gd["accept"], vt["tok_off"],
                                                                     vt["tok_bytes"], vt["eos"], fed=fed, n_bytes=vt["n_bytes"]), n=100)
        med = {k: statistics.median(v) for k, v in times.items()}
        base = med.get("parent_penalised_inactive", med["penalised_inactive"])
        print(json.dumps(dict(
            B=B, ctx=a.ctx, steps_per_region=a.steps, reps=a.reps,
            yardstick="parent_penalised_inactive" if parent is not None else "penalised_inactive",
            **{f"{k}_step_us": round(v, 1) for k, v in med.items()},
            **{f"{k}_over_own_penalised_us": round(med[k] - med["penalised_inactive"], 1) for k in med if k.startswith("guided")},
            **{f"{k}_over_parent_penalised_us": round(med[k] - base, 1) for k in med if k.startswith("parent_guided")},
            **{f"{k}_over_yardstick_us": round(med[k] - base, 1) for k in med if k.startswith("guided")},
            own_penalised_vs_yardstick_pct=round(100.0 * (med["penalised_inactive"] / base - 1.0), 3),
            guide_mask_kernel_us={k: round(v, 2) for k, v in alone.items()},
            table_bytes_staged={"3_states": B * 3 * 512, "255_states": B * 255 * 512,
                                "wide_json": B * (guide.region_rows(wide_json) * 512 + 256), "wide_bound": B * (256 * 512 + 256)},
            rows_done_at_end=done,
            reps_us={k: [round(x, 1) for x in v] for k, v in times.items()})), flush=True)
        del logits, cache, st, g, gd, adj, variants
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,16")
    ap.add_argument("--ctx", type=int, default=2531)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("guide_step_time.py measures on the GPU: none found")
    model, processor = load_synthetic(device="cuda:0")
    parent = None
    if a.parent:
        mod = load_parent(os.path.abspath(a.parent))
        parent = (mod.api.load_synthetic(device="cuda:0")[0], mod.sampling, mod.penalties, mod.guide, mod.ops)
    steps(model, processor, parent, a)


if __name__ == "__main__":
    main()
