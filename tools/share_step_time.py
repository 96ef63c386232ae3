"""share_prefix: what reading a family's prompt K/V once saves per decode step (profiles/share_prefix_step_time.txt is a run of
this file).

Full-size synthetic model, bf16 weights and cache.  For each prompt length (512, 2,531 and 32,768 keys) one text prompt is prefilled
once and its B = 1 state forked (model.fork_state) into B = n states, n = 2, 4, 8, 16 where memory allows (the cleared arm is left out where a third state does not fit):
    unshared  fork_state(n)              the B = n sampled step as without the feature: p3v_attention_decode under the split plan of model._plan
    cleared   fork_state(n, share=True), then set_families(st, []): the family launch under the family plan of model._plan with a table of
              single rows -- every row reads its own copy: what the PLAN costs or gains without any sharing
    shared    fork_state(n, share=True)  the same launch, the family registered: whole splits below share_end read once
The three captured sampled steps (temperature 0.8, seeds s + j) are replayed in turn, `--replays` replays per timing between two
device events with a synchronise, `--runs` alternations after `--warmup` untimed ones, in one process.  Reported per arm: the
median and max - min.  The caches grow by the same number of tokens in every arm.

Byte model: K + V^T of one token, all 32 layers = 2 * 32 * 32 * 96 * 2 B = 393 KB.  With chunk the family plan's keys per split,
the shared step reads (n - 1) * floor(share_end / chunk) * chunk * 393 KB less than the cleared one, and has one merge launch per
layer wherever the unshared plan merged in the attention launch.

    python tools/share_step_time.py [--keys 512,2531,32768] [--n 2,4,8,16] [--runs 8] [--warmup 2] [--replays 20] [--chunks 128,256] [--register-all]
--chunks: also time the shared arm under other chunk targets of the family plan (model.FAMILY_CHUNK) at 2,531 keys.
--register-all: switch the break-even rule (parallel.family_pays) off, so that small families are registered too: how the
losing shapes were found.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TOKEN_BYTES = 2 * 32 * 32 * 96 * 2
HBM = 7.2e12                                               # bytes / s the decode step's streams reach (profiles/pack13_step_ab.txt)
MAX_TOKENS = 704                                           # cache columns behind the prompt: every arm's replays fit


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", default="512,2531,32768")
    ap.add_argument("--n", default="2,4,8,16")
    ap.add_argument("--runs", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--chunks", default="")
    ap.add_argument("--register-all", action="store_true", help="register every family, also below the break-even of parallel.family_pays")
    a = ap.parse_args()
    import numpy as np
    import torch
    from phi_3_vision_mlx_amd import ops, sampling
    from phi_3_vision_mlx_amd.api import load_synthetic
    assert torch.cuda.is_available(), "a timing needs the GPU"
    if a.register_all:
        from phi_3_vision_mlx_amd import parallel
        parallel.FAMILY_BREAK_EVEN = 0
        print("--register-all: every family is registered (the break-even rule is off)")
    assert (a.warmup + a.runs) * a.replays + 8 <= MAX_TOKENS
    dev = "cuda:0"
    model, _ = load_synthetic(device=dev)
    rng = np.random.default_rng(0)

    def arm(st1, logits, n, kind, chunk=None):
        """-> (replay function, state, plan description) of one arm; None when the state does not fit."""
        default = type(model).FAMILY_CHUNK
        if chunk is not None:
            model.FAMILY_CHUNK = int(chunk)
        try:
            cache = model.fork_state(st1, n, **({} if kind == "unshared" else {"share": True}))
            st = cache[0].state
            if kind == "cleared":
                model.set_families(st, [])
            model.set_sampling(st, sampling.pack(sampling.rows(n, 0.8, 0, 1.0, 7), 0))
            tok = [model.sample_logits(st, logits[:, -1].expand(n, -1).contiguous())]
            _, tok[0] = model.sample_step(tok[0], cache)      # builds both captures
            torch.cuda.synchronize()
        except torch.cuda.OutOfMemoryError:
            cache = st = None
            torch.cuda.empty_cache()
            return None
        finally:
            model.FAMILY_CHUNK = default
        p = st.graphs["greedy"]["bufs"]["plan"]
        plan = f"{p.n_split} splits of {ops.attention_family_chunk(st.Tp, p.n_split)} keys, " + \
               ("family launch + merge launch" if p.family else "merge in launch" if p.attn_merge else "merge launch")

        def replay():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.replays):
                _, tok[0] = model.sample_step(tok[0], cache)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / a.replays
        return replay, st, plan

    def report(keys, n, arms):
        rec = {k: [] for k in arms}
        for i in range(a.warmup + a.runs):
            for k, (fn, _, _) in arms.items():
                ms = fn()
                if i >= a.warmup:
                    rec[k].append(ms)
        for k, ms in rec.items():
            print(f"    {k:22s} median {statistics.median(ms):8.4f} ms/step  max - min {max(ms) - min(ms):7.4f}  ({arms[k][2]})")
        return {k: (statistics.median(ms), max(ms) - min(ms)) for k, ms in rec.items()}

    for keys in [int(k) for k in a.keys.split(",")]:
        ids = rng.integers(3, 32000, (1, keys)).astype(np.int64)
        logits, cache1 = model(input_ids=ids, max_tokens=MAX_TOKENS)
        st1 = cache1[0].state
        torch.cuda.synchronize()
        print(f"{keys} prompt keys (cache of {st1.Tp} columns), {a.replays} replays per timing, {a.runs} alternations after {a.warmup} warm-ups")
        for n in [int(x) for x in a.n.split(",")]:
            arms = {k: arm(st1, logits, n, k) for k in ("unshared", "shared")}
            if any(v is None for v in arms.values()):
                print(f"  n = {n:2d}: the two states do not fit in memory together -- not measured")
                del arms
                torch.cuda.empty_cache()
                continue
            third = arm(st1, logits, n, "cleared")               # (the third state may not fit: the comparison that counts is above)
            if third is not None:
                arms["cleared"] = third
            del third
            st = arms["shared"][1]
            chunk = ops.attention_family_chunk(st.Tp, st.graphs["greedy"]["bufs"]["plan"].n_split)
            saved = (n - 1) * (keys // chunk) * chunk * TOKEN_BYTES
            print(f"  n = {n:2d}: byte model: shared reads {saved / 1e9:6.2f} GB less than cleared = {saved / HBM * 1e3:7.4f} ms at 7.2 TB/s")
            r = report(keys, n, arms)
            gain, spread = r["unshared"][0] - r["shared"][0], max(r["unshared"][1], r["shared"][1])
            print(f"    unshared - shared = {gain * 1e3:+9.1f} us per step ({100 * gain / r['unshared'][0]:+5.1f} %), larger spread {spread * 1e3:6.1f} us -> "
                  f"{'shared WINS by more than the spread' if gain > spread else 'shared LOSES by more than the spread' if -gain > spread else 'inside the spread'};"
                  + (f" cleared - shared = {(r['cleared'][0] - r['shared'][0]) * 1e3:+9.1f} us = {100 * (r['cleared'][0] - r['shared'][0]) / (saved / HBM * 1e3 + 1e-12):4.0f} % of the byte model"
                     if "cleared" in r else " cleared: not measured (memory)"))
            del arms, st
            torch.cuda.empty_cache()
            if a.chunks and keys == 2531 and n in (4, 8):
                alt = {f"shared, chunk {c}": arm(st1, logits, n, "shared", chunk=int(c)) for c in a.chunks.split(",")}
                if all(v is not None for v in alt.values()):
                    print(f"  n = {n:2d}: the family plan's chunk target")
                    report(keys, n, alt)
                del alt
                torch.cuda.empty_cache()
        del st1, cache1, logits
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
