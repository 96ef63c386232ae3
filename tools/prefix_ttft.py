"""Time to first token with and without the prompt prefix cache, full-size synthetic model.

The cold request is BASELINE config 2 (workloads.vqa_request: a 336 x 336 picture, 2,531 tokens); the warm request asks a new
question of `--question` tokens (<= 32) about the SAME picture after the first request's prefix (through the last image slot)
was captured.  Both are timed in one process, alternating, as min and median of `--runs` runs after `--warmup`: device events
around processor + prefill + first-token arg-max, plus one host wall-clock figure for the whole request (digest and store lookup
included).  Then the restore launch alone (p3v_kv_copy, entry -> a slot-state row at an odd column and at column 0) beside
torch's strided `copy_` of the same two slices: microseconds, bytes moved (read + written) and the rate as a fraction of the
6.29 TB/s a float4 copy reaches on this part.

    python tools/prefix_ttft.py [--runs 10] [--warmup 2] [--question 24]
    python tools/prefix_ttft.py --warm-only N          # N warm requests and nothing else timed: for a kernel trace
    python tools/prefix_ttft.py --split A.csv NA B.csv NB   # per-kernel split of ONE warm request from two kernel-stats files
                                                             # (runs with NA and NB warm requests: everything else cancels)
"""
import argparse
import csv
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_PEAK = 6.29e12            # measured float4 copy rate of the MI355X, bytes / s (read + written)


def split(a_csv, n_a, b_csv, n_b):
    def load(f):
        with open(f, newline="") as fh:
            return {r["Name"]: (int(r["Calls"]), int(r["TotalDurationNs"])) for r in csv.DictReader(fh)}
    a, b, d = load(a_csv), load(b_csv), n_b - n_a
    rows = []
    for name in set(a) | set(b):
        ca, ta = a.get(name, (0, 0))
        cb, tb = b.get(name, (0, 0))
        if cb != ca:
            rows.append(((tb - ta) / d / 1e3, (cb - ca) / d, name))
    total = sum(r[0] for r in rows)
    print(f"per-kernel split of one warm request (difference of runs with {n_a} and {n_b} warm requests): {total:.0f} us of kernels, "
          f"{sum(r[1] for r in rows):.0f} launches")
    for us, calls, name in sorted(rows, reverse=True)[:24]:
        print(f"  {us:9.1f} us  {100 * us / total:5.1f} %  {calls:7.1f} launches  {name[:110]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--question", type=int, default=24)
    ap.add_argument("--warm-only", type=int, default=0)
    ap.add_argument("--split", nargs=4, metavar=("A", "NA", "B", "NB"))
    a = ap.parse_args()
    if a.split:
        return split(a.split[0], int(a.split[1]), a.split[2], int(a.split[3]))
    import numpy as np
    import torch
    from PIL import Image
    from phi_3_vision_mlx_amd import ops
    from phi_3_vision_mlx_amd.api import load_synthetic
    from phi_3_vision_mlx_amd.prefix import PrefixCache, capture_len, image_digests
    assert 1 <= a.question <= 32
    dev = "cuda:0"
    model, proc = load_synthetic(device=dev)
    cfg = model.cfg
    rng = np.random.default_rng(0)
    img = Image.fromarray(rng.integers(0, 256, (336, 336, 3), dtype=np.uint8))
    text = rng.integers(3, 32000, 20 + 64 * 32).astype(np.int64)
    max_tokens = 100

    def request(question):
        """processor part of a request: HD preprocessing on the device + the ids as `_merge` lays them out (workloads.vqa_request)."""
        im = proc.img_processor.device_call([img], dev)
        n_img = im["num_img_tokens"][0]
        ids = np.concatenate([[1], text[:8], -np.ones(n_img, dtype=np.int64), [1], question])[None].astype(np.int64)
        return {"input_ids": ids, "pixel_values": im["pixel_values"], "image_sizes": np.asarray(im["image_sizes"], dtype=np.int64),
                "positions": np.argwhere(ids < 0)}

    store = PrefixCache(8 << 30)
    key = store.key(model.epoch, None, False, "bf16")

    def cold():
        inp = request(text[8:20])
        tok, cache = model.greedy_prefill(max_tokens, **inp)
        return inp, tok, cache

    def warm(i):
        q = text[20 + 32 * i:20 + 32 * i + a.question]
        dg = image_digests([img])
        inp = request(q)
        hit = store.lookup(inp["input_ids"].reshape(-1), dg, key)
        logits, cache = model(**inp, max_tokens=max_tokens, prefix=hit)
        return ops.argmax(logits[:, -1, :].contiguous()), hit[1], inp["input_ids"].shape[1]

    def timed(fn, *args):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        out = fn(*args)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3, out

    inp, _, cache = cold()
    ids = inp["input_ids"].reshape(-1)
    P = capture_len(ids)
    entry = store.insert(ids[:P], image_digests([img]), key, model.capture_prefix(cache[0].state, 0, 0, P))
    del cache
    if a.warm_only:
        for i in range(a.warm_only):
            warm(i % 60)
        torch.cuda.synchronize()
        return
    rec = {"cold": [], "warm": []}
    for i in range(a.warmup + a.runs):
        c = timed(cold)
        w = timed(warm, i)
        if i >= a.warmup:
            rec["cold"].append(c[:2]), rec["warm"].append(w[:2])
        S_w, P_w = w[2][2], w[2][1]
    print(f"prefix cache, time to first token: full-size synthetic model, cold S = {ids.size}, warm S = {S_w} with P = {P_w} tokens restored "
          f"(entry {entry.nbytes / 1e6:.0f} MB), {a.runs} runs after {a.warmup} warm-ups, cold and warm alternating")
    stat = {}
    for k in ("cold", "warm"):
        ev, wall = [r[0] for r in rec[k]], [r[1] for r in rec[k]]
        stat[k] = statistics.median(ev)
        print(f"  {k}: device events min {min(ev):7.3f} ms  median {statistics.median(ev):7.3f} ms | host wall clock min {min(wall):7.3f} ms  "
              f"median {statistics.median(wall):7.3f} ms")
    ratio = stat["warm"] / stat["cold"]
    print(f"  warm / cold (medians, device events): {ratio:.3f}  -> gate warm < 0.5 x cold: {'MET' if ratio < 0.5 else 'NOT MET'}")

    # ---- the restore launch alone, beside torch's strided copy_ of the same slices
    st = model.new_slot_state(2, 4096)
    nl, nkv, hd = cfg.num_hidden_layers, cfg.num_key_value_heads, model.hd
    moved = 2 * 2 * nl * nkv * P * hd * 2
    k_e, v_e = entry.kv

    def many(fn, n):
        out = []
        for i in range(a.warmup + n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                out.append(e0.elapsed_time(e1) * 1e3)
        return out
    ok = True
    for col in (19, 0):
        def kv_copy():
            model._restore_prefix(st, 1, col, entry, P)

        def torch_copy():
            st.k[:, 1, :, col:col + P].copy_(k_e[:, :, :P])
            st.v[:, 1, :, :, col:col + P].copy_(v_e[:, :, :, :P])
        tk, tt = many(kv_copy, a.runs), many(torch_copy, a.runs)
        mk, mt = statistics.median(tk), statistics.median(tt)
        ok = ok and mk <= mt
        print(f"  restore of {P} tokens to column {col:2d}: p3v_kv_copy min {min(tk):7.1f} us  median {mk:7.1f} us  = {moved / mk / 1e6:5.2f} TB/s "
              f"({100 * moved / (mk * 1e-6) / COPY_PEAK:4.1f} % of the 6.29 TB/s float4 copy) | torch copy_ x 2 min {min(tt):7.1f} us  median {mt:7.1f} us "
              f"= {moved / mt / 1e6:5.2f} TB/s | {moved / 1e6:.0f} MB read + written")
    print(f"  -> gate restore not slower than torch's copy_ (median against median): {'MET' if ok else 'NOT MET'}")


if __name__ == "__main__":
    main()
