"""What embeddings and retrieval cost on the full-size synthetic model, with device events, every shape warmed first, the two sides
of each comparison ALTERNATED 8 times in one call, medians and the spread (min .. max) printed.  One JSON line per measurement.

  * model.embed (pooling last / mean, normalised) against the plain prefill `model(**inputs)` of the SAME inputs in the same
    process: the 128-token text prompt, the one-image request (2,531 tokens), a 32k-token prompt.  The `last` embed skips lm_head
    and runs the final layer's tail on one row, as the prefill does: it should not cost more.
  * p3v_sim_topk at D = 3072, N = 131,072 (805 MB: beyond the Infinity Cache) and 1,048,576, Q in {1, 16}, k in {1, 10, 32}:
    time, N * D * 2 bytes over time, the project's launch model 2.4 us + bytes / 7.2 TB/s, and what a user would otherwise write,
    torch.topk(torch.mm(index, q.T).float(), k, dim=0).

    python tools/embed_time.py [--out profiles/embed_time.txt] [--only embed|sim] [--reps 8] [--no-32k]
    python tools/embed_time.py --trace N,Q,k        (that one shape, 20 launches, nothing else: the run to put under a profiler)
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from phi_3_vision_mlx_amd import api, ops  # noqa: E402
from phi_3_vision_mlx_amd.api import load_synthetic  # noqa: E402

D = 3072
LAUNCH_US, HBM_TBPS = 2.4, 7.2                     # README.md, the projections' row


def device_ms(fn, inner=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def alternate(sides, reps, inner=1):
    """sides: {name: fn}.  Every side warmed twice, then `reps` rounds of one timed region per side, in turn."""
    for fn in sides.values():
        fn()
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in sides}
    for _ in range(reps):
        for name, fn in sides.items():
            times[name].append(device_ms(fn, inner))
    return times


def stats(ts, digits=3):
    return dict(median=round(statistics.median(ts), digits), min=round(min(ts), digits), max=round(max(ts), digits))


def embed_side(model, processor, emit, reps, with_32k):
    from phi_3_vision_mlx_amd.workloads import vqa_request
    gen = torch.Generator().manual_seed(0)
    shapes = [("text 128 tokens", dict(input_ids=torch.randint(3, 32000, (1, 128), dtype=torch.int64, generator=gen))),
              ("one image, 2531 tokens", vqa_request(processor.img_processor, 0, device="cuda:0"))]
    if with_32k:
        shapes.append(("text 32768 tokens", dict(input_ids=torch.randint(3, 32000, (1, 32768), dtype=torch.int64, generator=gen))))
    for name, inputs in shapes:
        sides = {"prefill": lambda: model(**inputs),
                 "embed_last": lambda: api._embed_inputs(model, inputs, "last", True),
                 "embed_mean": lambda: api._embed_inputs(model, inputs, "mean", True)}
        t = alternate(sides, reps)
        med = {k: statistics.median(v) for k, v in t.items()}
        emit(dict(measure="embed vs plain prefill", request=name, tokens=int(inputs["input_ids"].shape[1]), reps=reps,
                  **{f"{k}_ms": stats(v) for k, v in t.items()},
                  embed_last_over_prefill=round(med["embed_last"] / med["prefill"], 4),
                  embed_mean_over_prefill=round(med["embed_mean"] / med["prefill"], 4)))
        torch.cuda.empty_cache()


def make_index(n):
    index = torch.empty((n, D), dtype=torch.bfloat16, device="cuda:0")
    for i in range(0, n, 65536):                     # in pieces: no fp32 copy of the whole index
        index[i:i + 65536].normal_(0.0, D ** -0.5)
    return index


def sim_side(emit, reps, sizes=(131072, 1 << 20)):
    index = make_index(max(sizes))
    gen = torch.Generator(device="cuda:0").manual_seed(1)
    for n in sizes:
        for Q in (1, 16):
            q = (torch.randn((Q, D), device="cuda:0", generator=gen) * D ** -0.5).to(torch.bfloat16)
            for k in (1, 10, 32):
                live = index[:n]
                out = (torch.empty((Q, k), dtype=torch.int32, device="cuda:0"), torch.empty((Q, k), dtype=torch.float32, device="cuda:0"))
                sides = {"sim_topk": lambda: ops.sim_topk(index, q, k, n=n, out=out),
                         "torch": lambda: torch.topk(torch.mm(live, q.T).float(), k, dim=0)}
                t = alternate(sides, reps, inner=4)
                nbytes = n * D * 2
                model_us = LAUNCH_US + nbytes / (HBM_TBPS * 1e6)
                med = {s: statistics.median(v) * 1e3 for s, v in t.items()}
                emit(dict(measure="sim_topk", N=n, Q=Q, k=k, D=D, index_bytes=nbytes, plan=ops.sim_topk_plan(n, Q, k, D), reps=reps,
                          sim_topk_us=stats([x * 1e3 for x in t["sim_topk"]], 1), torch_us=stats([x * 1e3 for x in t["torch"]], 1),
                          sim_topk_TB_per_s=round(nbytes / med["sim_topk"] / 1e6, 3), launch_model_us=round(model_us, 1),
                          sim_topk_over_model=round(med["sim_topk"] / model_us, 3), sim_topk_over_torch=round(med["sim_topk"] / med["torch"], 3)))
    del index
    torch.cuda.empty_cache()


def trace(shape):
    n, Q, k = (int(x) for x in shape.split(","))
    index = make_index(n)
    q = (torch.randn((Q, D), device="cuda:0") * D ** -0.5).to(torch.bfloat16)
    for _ in range(20):
        ops.sim_topk(index, q, k)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "embed_time.txt"))
    ap.add_argument("--only", choices=["embed", "sim"])
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--no-32k", action="store_true")
    ap.add_argument("--trace")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("embed_time.py measures on the GPU: none found")
    if a.trace:
        return trace(a.trace)
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
        with open(a.out, "w") as f:                  # rewritten after every record: a cut-off run keeps what it measured
            f.write("\n".join(lines) + "\n")

    emit(dict(tool="tools/embed_time.py", device=torch.cuda.get_device_name(0), timing="device events; every shape warmed twice; sides "
              f"alternated {a.reps} times; median (min .. max)"))
    if a.only != "embed":
        sim_side(emit, a.reps)
    if a.only != "sim":
        model, processor = load_synthetic(device="cuda:0")
        embed_side(model, processor, emit, a.reps, not a.no_32k)


if __name__ == "__main__":
    main()
