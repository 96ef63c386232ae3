"""n completions per prompt: what the KV fork costs and what it saves (profiles/kv_fork.txt is a run of this file).

(a) the fork kernel against the copy the prefix cache had, on raw tensors of the full model's geometry (32 layers, 32 kv
    heads, hd 96; bf16 and int8 + scales) for the one-image request's 2,531 tokens: ONE p3v_kv_fork launch to m = 1, 3, 7, 15
    rows against ceil(m / 4) p3v_kv_copy launches of up to 4 jobs, alternating `--runs` times each in one process.  Bytes moved
    (read + written) from the shapes: (1 + m) units for the fork, 2 m for the copies; rate = bytes / median time.
(b) time to the n first tokens, full-size synthetic model, n = 4 and 8: one prefill + model.fork_state + n draws from the one
    logits row, against n warm prefix-cache requests (image request: what the parent can do for a picture) and against the
    batched prefill of the prompt repeated n times (1,024-token text prompt: the prefill generate([p] * n) runs, on THIS tree's
    model -- the same kernels as the parent commit's, standing in for that call on a parent checkout).  All arms are model-level
    calls: processor (text) and streamer are left out on both sides.
(c) the B = n sampled decode step on forked rows at 2,531 keys against the same step on a state that a batched prefill built.

Times are device events around work that ends in a synchronise; every shape is warmed up first.

    python tools/fork_time.py [--runs 8] [--warmup 2] [--only a|b|c]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NL, NKV, HD, N_TOK = 32, 32, 96, 2531                      # the full model's cache geometry; the one-image request's tokens
COPY_PEAK = 6.29e12                                        # measured float4 copy rate of the MI355X, bytes / s (read + written)


def odd_tiles(t):
    tp = (t + 127) // 128 * 128
    return tp + 128 if (tp // 128) % 2 == 0 else tp


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3, out


def alternate(fns, runs, warmup):
    """{name: [ms]}: the functions in turn, `runs` timed rounds after `warmup` untimed ones."""
    rec = {k: [] for k in fns}
    for i in range(warmup + runs):
        for k, fn in fns.items():
            ms = timed(fn)[0]
            if i >= warmup:
                rec[k].append(ms)
    return rec


def line(name, ms, nbytes=None):
    med = statistics.median(ms)
    s = f"    {name:34s} min {min(ms):8.3f}  median {med:8.3f}  max {max(ms):8.3f} ms"
    if nbytes is not None:
        s += f" | {nbytes / 1e9:6.2f} GB read + written = {nbytes / med / 1e9:5.2f} TB/s ({100 * nbytes / (med * 1e-3) / COPY_PEAK:4.1f} % of the float4 copy)"
    return s


def part_a(a):
    import torch
    from phi_3_vision_mlx_amd import ops
    dev = "cuda:0"
    T = odd_tiles(N_TOK + 100)
    print(f"(a) p3v_kv_fork against p3v_kv_copy: {NL} layers x {NKV} kv heads x hd {HD}, {N_TOK} tokens from column 0, rows of {T} columns, "
          f"B = 1 -> B = 16; {a.runs} alternations after {a.warmup} warm-ups")
    for kind, es in (("bf16", 2), ("int8", 1)):
        def cache(B):
            if es == 2:
                return (torch.zeros((NL, B, NKV, T, HD), dtype=torch.bfloat16, device=dev), torch.zeros((NL, B, NKV, HD, T), dtype=torch.bfloat16, device=dev))
            return (torch.zeros((NL, B, NKV, T, HD), dtype=torch.uint8, device=dev), torch.zeros((NL, B, NKV, HD, T), dtype=torch.uint8, device=dev),
                    torch.ones((NL, B, NKV, T), dtype=torch.float32, device=dev), torch.ones((NL, B, NKV, T), dtype=torch.float32, device=dev))
        src, dst = cache(1), cache(16)
        for t in src:
            t.copy_(torch.randint(1, 100, t.shape, device=dev).to(t.dtype))
        unit = 2 * NL * NKV * N_TOK * HD * es + (2 * NL * NKV * N_TOK * 4 if es == 1 else 0)
        print(f"  {kind}: one row's run = {unit / 1e6:.0f} MB")
        for m in (1, 3, 7, 15):
            rows = list(range(1, m + 1))

            def fork():
                ops.kv_fork(src, 0, 0, dst, rows, 0, N_TOK)

            def copies():
                for i in range(0, m, 4):
                    ops.kv_copy([(src, 0, 0, dst, r, 0, N_TOK) for r in rows[i:i + 4]])
            rec = alternate({"fork": fork, "copy": copies}, a.runs, a.warmup)
            ok = all(bool((t[:, r] == t[:, 1]).all()) for t in dst for r in rows[1:]) and bool((dst[0][:, 1, :, :N_TOK] == src[0][:, 0, :, :N_TOK]).all())
            print(f"   m = {m:2d} rows ({'rows equal the source' if ok else 'ROWS DIFFER'})")
            print(line(f"p3v_kv_fork, 1 launch", rec["fork"], (1 + m) * unit))
            print(line(f"p3v_kv_copy, {-(-m // 4)} launch(es)", rec["copy"], 2 * m * unit))
            mf, mc = statistics.median(rec["fork"]), statistics.median(rec["copy"])
            spread = max(max(rec["fork"]) - min(rec["fork"]), max(rec["copy"]) - min(rec["copy"]))
            print(f"    copy - fork (medians) = {mc - mf:+8.3f} ms, the alternation's spread (max - min) = {spread:.3f} ms; byte model "
                  f"{(1 + m)} : {2 * m} units -> fork / copy = {(1 + m) / (2 * m):.2f}, measured {mf / mc:.2f}"
                  + ("" if m < 3 else f" -> gate fork faster by more than the spread: {'MET' if mc - mf > spread else 'NOT MET'}"))
        del src, dst
        torch.cuda.empty_cache()


def part_bc(a):
    import numpy as np
    import torch
    from PIL import Image
    from phi_3_vision_mlx_amd import ops, sampling
    from phi_3_vision_mlx_amd.api import load_synthetic
    from phi_3_vision_mlx_amd.prefix import PrefixCache, capture_len, image_digests
    dev = "cuda:0"
    model, proc = load_synthetic(device=dev)
    rng = np.random.default_rng(0)
    img = Image.fromarray(rng.integers(0, 256, (336, 336, 3), dtype=np.uint8))
    text = rng.integers(3, 32000, 2048).astype(np.int64)
    max_tokens = 100

    def image_request():
        im = proc.img_processor.device_call([img], dev)
        ids = np.concatenate([[1], text[:8], -np.ones(im["num_img_tokens"][0], dtype=np.int64), [1], text[8:20]])[None].astype(np.int64)
        return {"input_ids": ids, "pixel_values": im["pixel_values"], "image_sizes": np.asarray(im["image_sizes"], dtype=np.int64),
                "positions": np.argwhere(ids < 0)}

    def draws(logits, n):
        recs = sampling.pack(sampling.rows(n, 0.8, 0, 0.95, 1), 0).to(dev)
        return ops.sample(logits[:, -1].expand(n, -1).contiguous(), recs)

    store = PrefixCache(8 << 30)
    key = store.key(model.epoch, None, False, "bf16")
    inp = image_request()
    ids = inp["input_ids"].reshape(-1)
    P = capture_len(ids)
    _, cache = model.greedy_prefill(max_tokens, **inp)
    store.insert(ids[:P], image_digests([img]), key, model.capture_prefix(cache[0].state, 0, 0, P))
    del cache
    if a.only in (None, "b"):
        print(f"(b) time to the n first tokens, full-size synthetic model, max_tokens {max_tokens}; {a.runs} alternations after {a.warmup} warm-ups")
        for n in (4, 8):
            def family_image():
                r = image_request()
                logits, c = model(**r, max_tokens=max_tokens)
                c = model.fork_state(c[0].state, n)
                return draws(logits, n), c

            def warm_requests():
                out = []
                for j in range(n):
                    r = image_request()
                    hit = store.lookup(r["input_ids"].reshape(-1), image_digests([img]), key)
                    logits, c = model(**r, max_tokens=max_tokens, prefix=hit)
                    out.append((draws(logits, 1), c))
                return out
            def family_warm():                                       # the family through the store: ONE warm prefill, then the fork
                r = image_request()
                hit = store.lookup(r["input_ids"].reshape(-1), image_digests([img]), key)
                logits, c = model(**r, max_tokens=max_tokens, prefix=hit)
                c = model.fork_state(c[0].state, n)
                return draws(logits, n), c
            rec = alternate({"family": family_image, "warm": warm_requests, "family_warm": family_warm}, a.runs, a.warmup)
            print(f"  image request ({ids.size} tokens, prefix entry of {P}), n = {n}")
            print(line("one prefill + fork_state + n draws", rec["family"]))
            print(line("n warm prefix-cache requests", rec["warm"]))
            print(line("one WARM prefill + fork_state + n", rec["family_warm"]))
            tids = text[:1024][None]

            def family_text():
                logits, c = model(input_ids=tids, max_tokens=max_tokens)
                c = model.fork_state(c[0].state, n)
                return draws(logits, n), c

            def batched_text():
                logits, c = model(input_ids=np.repeat(tids, n, axis=0), max_tokens=max_tokens)
                recs = sampling.pack(sampling.rows(n, 0.8, 0, 0.95, 1), 0).to(dev)
                return ops.sample(logits[:, -1].contiguous(), recs), c
            rec = alternate({"family": family_text, "batched": batched_text}, a.runs, a.warmup)
            print(f"  text prompt (1024 tokens), n = {n}")
            print(line("one prefill + fork_state + n draws", rec["family"]))
            print(line("prefill of the prompt repeated n times", rec["batched"]))
    if a.only in (None, "c"):
        steps = 32
        print(f"(c) B = n sampled decode step at {N_TOK} keys, mean of {steps} graph replays per sample; {a.runs} alternations after {a.warmup} warm-ups")
        tids = text[:N_TOK][None]
        for n in (4, 8):
            recs = sampling.rows(n, 0.8, 0, 0.95, 1)
            logits, c1 = model(input_ids=tids, max_tokens=(a.runs + a.warmup + 1) * steps + 8)
            forked = model.fork_state(c1[0].state, n)
            del c1
            lb, batched = model(input_ids=np.repeat(tids, n, axis=0), max_tokens=(a.runs + a.warmup + 1) * steps + 8)
            state = {}
            for name, c, lg in (("forked", forked, logits[:, -1].expand(n, -1).contiguous()), ("batched", batched, lb[:, -1].contiguous())):
                model.set_sampling(c[0].state, sampling.pack(recs, 0))
                state[name] = [model.sample_logits(c[0].state, lg), c]
                state[name][0] = model.sample_step(state[name][0], c)[1]          # (builds the sampled capture)

            def run(name):
                def go():
                    tok, c = state[name]
                    for _ in range(steps):
                        _, tok = model.sample_step(tok, c)
                    state[name][0] = tok
                return go
            rec = alternate({"forked": run("forked"), "batched": run("batched")}, a.runs, a.warmup)
            print(f"  n = {n}")
            print(line("step on forked rows", [x / steps for x in rec["forked"]]))
            print(line("step on a batched prefill's rows", [x / steps for x in rec["batched"]]))
            del forked, batched, state
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=["a", "b", "c"], default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("fork_time.py measures on the GPU: none found")
    if a.only in (None, "a"):
        part_a(a)
    if a.only in (None, "b", "c"):
        part_bc(a)


if __name__ == "__main__":
    main()
