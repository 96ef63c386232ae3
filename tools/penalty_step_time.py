"""What the penalties cost on the full-size synthetic model (2531-token context by default), at B = 1 / 8 / 16, in ONE call: the
plain sampled step (T only), the penalised step (repetition + frequency + presence on every row) and the penalised step with a
bias table -- all graph replays on ONE state (the captures share the greedy capture's loop-state buffers), walked in turn, every
region rewound to the SAME cache length (a step's time grows with its context), medians of the repeated regions -- and the
p3v_penalize launch alone (eager, on the step's own logits buffer; with and without bias, and with every row inactive).

--parent DIR: a built checkout of the PARENT commit.  Its package is loaded beside this one (own library, own model with the same
seed) and its T-only sampled step is measured in the same run, alternated with the others: the yardstick the new steps are held
against.  Without it the tree's own sampled step -- code this feature does not touch -- is the only yardstick.

    python tools/penalty_step_time.py [--batches 1,8,16] [--ctx 2531] [--steps 40] [--reps 5] [--parent DIR]
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from phi_3_vision_mlx_amd import ops, penalties, sampling  # noqa: E402
from phi_3_vision_mlx_amd.api import load_synthetic  # noqa: E402


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


def prepare(model, samp, ids, budget):
    logits, cache = model(input_ids=ids, max_tokens=budget)
    st = cache[0].state
    B = ids.shape[0]
    model.set_sampling(st, samp.pack(samp.rows(B, 1.0, 0, 1.0, 1234), 1))              # T only
    return cache, st, logits


def steps(model, parent, a):
    V = model.cfg.vocab_size
    for B in [int(x) for x in a.batches.split(",")]:
        ids = torch.randint(3, 32000, (B, a.ctx), dtype=torch.int64, generator=torch.Generator().manual_seed(B))
        budget = a.steps + 8
        cache, st, logits = prepare(model, sampling, ids, budget)
        tok = ops.argmax(logits[:, -1].contiguous())[:, None]
        rows = penalties.rows(B, 1.3, 0.5, 0.5)
        rows_bias = penalties.rows(B, 1.3, 0.5, 0.5, {7: -float("inf"), 11: 2.0})
        model.set_penalties(st, penalties.pack(rows_bias), ids.numpy(), 0, bias=penalties.bias_table(rows_bias, V))
        variants = [("sampled_T", model, model.sample_step, cache, None), ("penalised", model, model.penal_step, cache, rows),
                    ("penalised_bias", model, model.penal_step, cache, rows_bias)]
        toks = {"own": tok}
        if parent is not None:
            p_model, p_samp = parent
            p_cache, _, p_logits = prepare(p_model, p_samp, ids, budget)
            toks["parent"] = p_logits[:, -1].argmax(-1).to(torch.int32)[:, None]
            variants.insert(0, ("parent_sampled_T", p_model, p_model.sample_step, p_cache, None))

        def run(name, m, fn, c, prow):
            key = "parent" if m is not model else "own"
            if prow is not None:
                st.penalty["rows"].copy_(penalties.pack(prow))                         # (the table and the bias stay: same bytes moved)
            t, toks[key] = timed(fn, toks[key], c, a.steps, m, a.ctx)
            return t
        for v in variants:                                                              # capture + warm every graph
            run(*v)
        times = {v[0]: [] for v in variants}
        for _ in range(a.reps):
            for v in variants:
                times[v[0]].append(run(*v))
        # the kernel alone (eager launches on the step's own logits buffer)
        g = st.graphs["greedy"]
        pen, lg = st.penalty, g["logits"]
        alone = {}
        for name, prow, bias in (("penalised", rows, None), ("penalised_bias", rows_bias, pen["bias"]),
                                 ("all_rows_inactive", penalties.rows(B), None)):
            rec = penalties.pack(prow).cuda()
            alone[name] = launches_us(lambda: ops.penalize(lg, rec, pen["seen"], bias, g["tok"], out=pen["adj"]))
        srec = sampling.pack(sampling.rows(B, 1.0, 0, 1.0, 1234), 0).cuda()
        alone["sample_T"] = launches_us(lambda: ops.sample(lg, srec))
        med = {k: statistics.median(v) for k, v in times.items()}
        base = med.get("parent_sampled_T", med["sampled_T"])
        moved = {"penalised": B * V * (2 + 4 + 2), "penalised_bias": B * V * (2 + 4 + 4 + 2)}
        print(json.dumps(dict(
            B=B, ctx=a.ctx, steps_per_region=a.steps, reps=a.reps, yardstick="parent_sampled_T" if parent is not None else "sampled_T",
            **{f"{k}_step_us": round(v, 1) for k, v in med.items()},
            penalised_adds_us=round(med["penalised"] - base, 1), penalised_bias_adds_us=round(med["penalised_bias"] - base, 1),
            own_sampled_T_vs_yardstick_pct=round(100.0 * (med["sampled_T"] / base - 1.0), 3),
            penalize_kernel_us={k: round(v, 2) for k, v in alone.items() if k != "sample_T"},
            penalize_kernel_GB_per_s={k: round(moved[k] / alone[k] / 1e3, 1) for k in moved},
            bytes_moved=moved, sample_kernel_T_us=round(alone["sample_T"], 2),
            reps_us={k: [round(x, 1) for x in v] for k, v in times.items()})), flush=True)
        del logits, cache, st, g, lg, pen, variants
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
        raise SystemExit("penalty_step_time.py measures on the GPU: none found")
    model, _ = load_synthetic(device="cuda:0")
    parent = None
    if a.parent:
        mod = load_parent(os.path.abspath(a.parent))
        parent = (mod.api.load_synthetic(device="cuda:0")[0], mod.sampling)
    steps(model, parent, a)


if __name__ == "__main__":
    main()
