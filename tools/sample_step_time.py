"""Greedy versus sampled graph-replayed decode step on the full-size synthetic model (2531-token context by default), plus the
eager p3v_sample launch alone, at B = 1 / 8 / 16.  Replays of the two variants alternate on ONE state (the sampled capture
shares the greedy capture's loop-state buffers), so both see the same cache lengths.  One JSON line per batch size.

    python tools/sample_step_time.py [--batches 1,8,16] [--ctx 2531] [--steps 40] [--reps 4] [--top-k 50] [--top-p 0.9]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from phi_3_vision_mlx_amd import ops, sampling  # noqa: E402
from phi_3_vision_mlx_amd.api import load_synthetic  # noqa: E402


def timed(fn, tok, cache, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        _, tok = fn(tok, cache)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n, tok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,16")
    ap.add_argument("--ctx", type=int, default=2531)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--top-k", type=int, default=50)
    ap.add_argument("--top-p", type=float, default=0.9)
    a = ap.parse_args()
    model, _ = load_synthetic(device="cuda:0")
    for B in [int(x) for x in a.batches.split(",")]:
        ids = torch.randint(3, 32000, (B, a.ctx), dtype=torch.int64, generator=torch.Generator().manual_seed(B))
        budget = 2 * (a.reps + 1) * a.steps + 8
        logits, cache = model(input_ids=ids, max_tokens=budget)
        tok = ops.argmax(logits[:, -1].contiguous())[:, None]
        rows = sampling.rows(B, 1.0, a.top_k, a.top_p, 1234)
        model.set_sampling(cache[0].state, sampling.pack(rows, 1))
        _, tok = timed(model.greedy_step, tok, cache, a.steps)         # capture + warm both variants
        _, tok = timed(model.sample_step, tok, cache, a.steps)
        g, s = [], []
        for _ in range(a.reps):
            t, tok = timed(model.greedy_step, tok, cache, a.steps)
            g.append(t)
            t, tok = timed(model.sample_step, tok, cache, a.steps)
            s.append(t)
        # the sampling kernel alone (eager launches on the step's own logits buffer)
        lg = cache[0].state.graphs["greedy"]["logits"]
        rec = sampling.pack(rows, 0).cuda()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(5):
            ops.sample(lg, rec)
        ev0.record()
        for _ in range(100):
            ops.sample(lg, rec)
        ev1.record()
        torch.cuda.synchronize()
        gm, sm = statistics.median(g), statistics.median(s)
        print(json.dumps(dict(B=B, ctx=a.ctx, temperature=1.0, top_k=a.top_k, top_p=a.top_p, greedy_step_us=round(gm, 1), sampled_step_us=round(sm, 1), ratio=round(sm / gm, 4),
                              sample_kernel_us=round(ev0.elapsed_time(ev1) * 10, 2), greedy_reps=[round(x, 1) for x in g],
                              sampled_reps=[round(x, 1) for x in s])), flush=True)
        del logits, cache
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
