"""What a beam step costs on the full-size synthetic bf16 model (2531-key prompt by default), at W = 2 / 4 / 8 beams and a suffix
of 16 / 128 / 512 columns, in ONE call: the captured beam step (graph replays on the B = W state model.beam_start makes, re-armed to
the same cache length before every region) against the plain greedy B = W step at the same cache length, alternated, medians of
the repeated regions; then the three new launches alone, eagerly -- p3v_beam_end on the step's own logits, the reorder's gather
and scatter with every row moved -- and the reorder's rate against its byte model (2 launches x moved rows x window x bytes per
column, read + written).

--parent DIR: a built checkout of the PARENT commit.  Its package is loaded beside this one (own library, own model with the same
seed) and ITS plain greedy B = W step is the yardstick, measured in the same alternation.  Without it the tree's own plain step --
code this feature does not touch -- is the yardstick.

The suffix columns of the timed states are copies of prompt columns (a search that long would have written them; a timing run has
not), so every step sees finite keys and the rows really move: the mean number of moved rows per step is reported.

    python tools/beam_step_time.py [--beams 2,4,8] [--suffix 16,128,512] [--ctx 2531] [--steps 30] [--reps 5] [--parent DIR]
                                   [--out profiles/beam_step_time.txt]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from phi_3_vision_mlx_amd import beam, ops  # noqa: E402
from phi_3_vision_mlx_amd.api import ID_EOS, load_synthetic  # noqa: E402


def load_parent(path):
    """The package of another checkout under a name of its own (its relative imports and its libp3v.so stay its own)."""
    import types
    pkg = os.path.join(path, "phi-3-vision-mlx_amd")
    if not os.path.exists(os.path.join(pkg, "libp3v.so")):
        raise SystemExit(f"--parent: {pkg} holds no libp3v.so (build that checkout first)")
    mod = types.ModuleType("p3v_parent")
    mod.__path__ = [pkg]
    sys.modules["p3v_parent"] = mod
    mod.api = importlib.import_module("p3v_parent.api")
    return mod


def region_us(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def fill_suffix(st, S0, n):
    """columns [S0, S0 + n) of every row <- prompt columns (finite keys for a timing run)"""
    n = min(n, st.Tp - S0)
    for lo in range(0, n, S0):
        m = min(S0, n - lo)
        st.k[:, :, :, S0 + lo:S0 + lo + m] = st.k[:, :, :, :m]
        st.v[..., S0 + lo:S0 + lo + m] = st.v[..., :m]


def plain_state(model, W, ids, budget, S0):
    logits, cache = model(input_ids=ids.expand(W, -1).contiguous(), max_tokens=budget)
    fill_suffix(cache[0].state, S0, budget)
    return cache, logits[:, -1].float().argmax(-1).to(torch.int32)[:, None]


def measure(model, parent_model, a, out):
    suffixes = [int(x) for x in a.suffix.split(",")]
    budget = max(suffixes) + a.steps + 16
    ids = torch.randint(3, 32000, (1, a.ctx), dtype=torch.int64, generator=torch.Generator().manual_seed(7))
    cfg = model.cfg
    col_bytes = cfg.num_hidden_layers * cfg.num_key_value_heads * model.hd * 2 * 2      # K + V^T of one column of one row
    for W in [int(x) for x in a.beams.split(",")]:
        logits, cache1 = model(input_ids=ids, max_tokens=budget)
        g = model.beam_start(cache1, logits[:, -1, :], W, ID_EOS)
        bcache, st = g["cache"], g["cache"][0].state
        S0 = g["S0"]
        fill_suffix(st, S0, budget)
        del cache1
        pcache, ptok = plain_state(model, W, ids, budget, S0)
        yard = [("own_plain", model, pcache, ptok)]
        if parent_model is not None:
            qcache, qtok = plain_state(parent_model, W, ids, budget, S0)
            yard.insert(0, ("parent_plain", parent_model, qcache, qtok))
        tok0 = torch.randint(3, 32000, (W,), dtype=torch.int32, generator=torch.Generator().manual_seed(W)).to(g["tok"].device)

        def beam_region(s):
            g["tok"].copy_(tok0), g["cum"].zero_(), g["d_step"].zero_(), g["d_past"].fill_(S0 + s)
            g["n_replays"] = 1
            t = region_us(lambda: model.beam_step(bcache), a.steps)
            recs = g["rec"][:a.steps].numpy()
            moved = float(np.mean([(r[10:10 + W] != np.arange(W)).sum() for r in recs]))
            failed = int((recs[:, 0] != 0).sum())
            return t, moved, failed

        def plain_region(m, cache, tok, s):
            cache[0].state.offset = S0 + s
            m.restart_history(cache[0].state)
            box = [tok]

            def step():
                box[0] = m.greedy_step(box[0], cache)[1]
            return region_us(step, a.steps)
        for s in suffixes:
            beam_region(s)                                               # warm
            for name, m, c, t in yard:
                plain_region(m, c, t, s)
            times, moved, failed = {"beam": []}, [], 0
            for _ in range(a.reps):
                for name, m, c, t in yard:
                    times.setdefault(name, []).append(plain_region(m, c, t, s))
                t_b, mv, fl = beam_region(s)
                times["beam"].append(t_b), moved.append(mv)
                failed += fl
            med = {k: statistics.median(v) for k, v in times.items()}
            base = med[yard[0][0]]
            window = min((S0 + s + a.steps // 2 + 7) // 8 * 8, st.Tp) - g["c0a"]
            model_us = 2 * statistics.mean(moved) * window * col_bytes * 2 / 5e12 * 1e6
            # the three launches alone, eager; the reorder with every row moved (a rotation)
            g["d_past"].fill_(S0 + s)
            g["d_step"].zero_()
            sel = region_us(lambda: (g["d_step"].zero_(), ops.beam_end(g["logits"], g["state"], W, ID_EOS)), 50)
            zero = region_us(lambda: g["d_step"].zero_(), 50)
            g["parent"].copy_(torch.tensor([(k + 1) % W for k in range(W)], dtype=torch.int32))
            g["d_past"].fill_(S0 + s)
            kv = (st.k, st.v)
            w_cols = min((S0 + s + 7) // 8 * 8, st.Tp) - g["c0a"]
            ph = [region_us(lambda p=p: ops.kv_permute(kv, g["parent"], W, g["c0a"], g["d_past"], g["stage"], p), 50) for p in (0, 1)]
            moved_bytes = W * w_cols * col_bytes * 2                     # one launch: read + written
            line = dict(W=W, ctx=a.ctx, suffix=s, steps_per_region=a.steps, reps=a.reps, yardstick=yard[0][0],
                        **{f"{k}_step_us": round(v, 1) for k, v in med.items()},
                        beam_over_yardstick_us=round(med["beam"] - base, 1), beam_vs_yardstick=round(med["beam"] / base, 4),
                        mean_rows_moved_per_step=round(statistics.mean(moved), 2), failed_steps=failed,
                        permute_byte_model_us_at_5TBps=round(model_us, 1),
                        bound_1p5x_us=round(1.5 * (base + model_us), 1), within_bound=bool(med["beam"] <= 1.5 * (base + model_us)),
                        beam_end_alone_us=round(sel - zero, 2), gather_alone_us=round(ph[0], 2), scatter_alone_us=round(ph[1], 2),
                        permute_window_cols=w_cols, permute_all_rows_TBps=[round(moved_bytes / (t * 1e-6) / 1e12, 3) for t in ph],
                        reps_us={k: [round(x, 1) for x in v] for k, v in times.items()})
            print(json.dumps(line), flush=True)
            out.write(json.dumps(line) + "\n")
            out.flush()
        del g, bcache, st, pcache, yard, logits
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--beams", default="2,4,8")
    ap.add_argument("--suffix", default="16,128,512")
    ap.add_argument("--ctx", type=int, default=2531)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beam_step_time.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("beam_step_time.py measures on the GPU: none found")
    assert beam.MAX >= max(int(x) for x in a.beams.split(","))
    model, _ = load_synthetic(device="cuda:0")
    parent_model = load_parent(os.path.abspath(a.parent)).api.load_synthetic(device="cuda:0")[0] if a.parent else None
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as out:
        out.write(f"# tools/beam_step_time.py --beams {a.beams} --suffix {a.suffix} --ctx {a.ctx} --steps {a.steps} --reps {a.reps}"
                  f"{' --parent <parent checkout>' if a.parent else ''}\n# one JSON line per (W, suffix); times in microseconds\n")
        measure(model, parent_model, a, out)


if __name__ == "__main__":
    main()
