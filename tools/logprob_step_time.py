"""What token log-probabilities cost on the full-size synthetic model (2531-token context by default), at B = 1 / 8 / 16, in ONE
call: the plain greedy step, the T-only sampled step, greedy + logprobs at N = 0 and N = 8, sampled + logprobs at N = 8 -- all
graph replays on ONE state (the captures share the greedy capture's loop-state buffers), walked in turn, every region rewound to
the SAME cache length (a step's time grows with its context: at B = 16 by ~0.6 us per token, which would otherwise be charged
to whichever variant runs later), medians of the repeated regions -- and the eager p3v_logprobs launch alone.  Then score() of the
config-2 request (2531 rows): the p3v_logprobs launch alone as rows/s and GB/s of logits read, and the whole call against the
same request's plain prefill.  One JSON line per batch size, one for score().

    python tools/logprob_step_time.py [--batches 1,8,16] [--ctx 2531] [--steps 40] [--reps 5] [--no-score]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from phi_3_vision_mlx_amd import api, ops, sampling  # noqa: E402
from phi_3_vision_mlx_amd.api import load_synthetic  # noqa: E402


def timed(fn, tok, cache, n, model=None, start=None):
    if start is not None:                            # every region starts at the same cache length and at step 0 (record slots)
        cache[0].state.offset = start
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


def steps(model, a):
    for B in [int(x) for x in a.batches.split(",")]:
        ids = torch.randint(3, 32000, (B, a.ctx), dtype=torch.int64, generator=torch.Generator().manual_seed(B))
        variants = [("greedy", model.greedy_step, None), ("sampled_T", model.sample_step, None),
                    ("greedy_lp0", model.logprob_step, 0), ("greedy_lp8", model.logprob_step, 8),
                    ("sampled_lp8", model.sample_logprob_step, 8)]
        budget = a.steps + 8
        logits, cache = model(input_ids=ids, max_tokens=budget)
        st = cache[0].state
        tok = ops.argmax(logits[:, -1].contiguous())[:, None]
        model.set_sampling(st, sampling.pack(sampling.rows(B, 1.0, 0, 1.0, 1234), 1))       # T only: the yardstick of the issue
        model.set_logprobs(st, [0] * B)
        for _, fn, _ in variants[:3] + variants[4:]:                                           # capture + warm every graph
            _, tok = timed(fn, tok, cache, a.steps, model, a.ctx)
        times = {name: [] for name, _, _ in variants}
        for _ in range(a.reps):
            for name, fn, want in variants:
                if want is not None:
                    model.set_logprobs(st, [want] * B)
                t, tok = timed(fn, tok, cache, a.steps, model, a.ctx)
                times[name].append(t)
        # the kernel alone (eager launches on the step's own logits buffer)
        g = st.graphs["greedy"]
        lg, nt = g["logits"], g["next_tok"]
        out = torch.zeros((B, ops.L.LOGPROB_WORDS), dtype=torch.int32, device=lg.device)
        alone = {}
        for want in (0, 8):
            w = torch.full((B,), want, dtype=torch.int32, device=lg.device)
            alone[want] = launches_us(lambda: ops.logprobs(lg, nt, w, out=out))
        off = torch.full((B,), -1, dtype=torch.int32, device=lg.device)
        alone["off"] = launches_us(lambda: ops.logprobs(lg, nt, off, out=out))
        rec = sampling.pack(sampling.rows(B, 1.0, 0, 1.0, 1234), 0).cuda()
        alone["sample_T"] = launches_us(lambda: ops.sample(lg, rec))
        med = {k: statistics.median(v) for k, v in times.items()}
        print(json.dumps(dict(
            B=B, ctx=a.ctx, steps_per_region=a.steps, reps=a.reps,
            **{f"{k}_step_us": round(v, 1) for k, v in med.items()},
            sampled_T_adds_us=round(med["sampled_T"] - med["greedy"], 1),
            greedy_lp0_adds_us=round(med["greedy_lp0"] - med["greedy"], 1),
            greedy_lp8_adds_us=round(med["greedy_lp8"] - med["greedy"], 1),
            sampled_lp8_adds_us=round(med["sampled_lp8"] - med["sampled_T"], 1),
            logprobs_kernel_us={"N0": round(alone[0], 2), "N8": round(alone[8], 2), "all_rows_off": round(alone["off"], 2)},
            sample_kernel_T_us=round(alone["sample_T"], 2),
            reps_us={k: [round(x, 1) for x in v] for k, v in times.items()})), flush=True)
        del logits, cache, st, g, lg, nt
        torch.cuda.empty_cache()


def score(model, processor, a):
    from phi_3_vision_mlx_amd.workloads import vqa_request
    inputs = vqa_request(processor.img_processor, 0, device="cuda:0")
    rows, V = inputs["input_ids"].shape[1], model.cfg.vocab_size

    def wall(fn, n):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(n):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts), ts

    plain, plain_all = wall(lambda: model(**inputs), a.reps)
    full, full_all = wall(lambda: model(**inputs, full_logits=True), a.reps)
    whole, whole_all = wall(lambda: api._score_inputs(model, inputs, 0), a.reps)
    logits, _ = model(**inputs, full_logits=True)
    lg = logits.view(rows, V)
    tok = torch.randint(0, V, (rows,), dtype=torch.int32, device=lg.device)
    out = torch.zeros((rows, ops.L.LOGPROB_WORDS), dtype=torch.int32, device=lg.device)
    res = {}
    for want in (0, 8):
        w = torch.full((rows,), want, dtype=torch.int32, device=lg.device)
        us = launches_us(lambda: ops.logprobs(lg, tok, w, out=out), n=20, warm=3)
        res[f"N{want}"] = dict(launch_us=round(us, 1), rows_per_s=round(rows / us * 1e6), logits_GB_per_s=round(rows * V * 2 / us / 1e3, 1))
    print(json.dumps(dict(score_request="config 2", rows=rows, vocab=V, logprobs_launch=res,
                          plain_prefill_ms=round(plain, 2), full_logits_prefill_ms=round(full, 2), score_call_ms=round(whole, 2),
                          score_over_plain=round(whole / plain, 4),
                          reps_ms=dict(plain=[round(x, 2) for x in plain_all], full_logits=[round(x, 2) for x in full_all],
                                       score=[round(x, 2) for x in whole_all]))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,16")
    ap.add_argument("--ctx", type=int, default=2531)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-score", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("logprob_step_time.py measures on the GPU: none found")
    model, processor = load_synthetic(device="cuda:0")
    steps(model, a)
    if not a.no_score:
        score(model, processor, a)


if __name__ == "__main__":
    main()
