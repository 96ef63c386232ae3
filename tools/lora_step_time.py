"""Graph-replayed decode step with LoRA adapters on the full-size synthetic model (512 keys by default) at B = 1 / 8 / 16:
  none          no adapter
  one_qkv       model.set_adapters: ONE rank-8 adapter on qkv_proj of all layers (every row gets it)
  one_all       model.set_adapters: one rank-8 adapter on all four projection types of all layers
  bank_*_one    model.set_adapter_bank: FOUR such adapters resident, every row on the first
  bank_*_spread the same bank, rows spread over the four adapters
  bank_*_off    the same bank, every row at -1 (no adapter)
Attaching an adapter or a bank drops the captured step, so variants cannot alternate on one state: every repetition walks ALL
variants in turn (attach, prefill, capture, warm up, time), which spreads drift over them alike; medians and every repetition
are reported.  One JSON line per batch size.

    python tools/lora_step_time.py [--batches 1,8,16] [--ctx 512] [--steps 40] [--reps 3] [--rank 8]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from phi_3_vision_mlx_amd import ops  # noqa: E402
from phi_3_vision_mlx_amd.api import load_synthetic  # noqa: E402

ALL = ["self_attn.qkv_proj", "self_attn.o_proj", "mlp.gate_up_proj", "mlp.down_proj"]


def adapter(cfg, targets, rank, seed):
    """{weight key: (lora_a, lora_b, scale)} on every layer, as weights.resolve_adapter returns it."""
    gen = torch.Generator().manual_seed(seed)
    H, I = cfg.hidden_size, cfg.intermediate_size
    qkv = (cfg.num_attention_heads + 2 * cfg.num_key_value_heads) * (H // cfg.num_attention_heads)
    dims = {"self_attn.qkv_proj": (H, qkv), "self_attn.o_proj": (H, H), "mlp.gate_up_proj": (H, 2 * I), "mlp.down_proj": (I, H)}
    out = {}
    for i in range(cfg.num_hidden_layers):
        for t in targets:
            k_in, k_out = dims[t]
            out[f"model.layers.{i}.{t}.weight"] = ((torch.rand((k_in, rank), generator=gen) * 2 - 1) * k_in ** -0.5,
                                                   torch.randn((rank, k_out), generator=gen) * 0.01, 2.0)
    return out


def timed(model, tok, cache, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        _, tok = model.greedy_step(tok, cache)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n, tok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,16")
    ap.add_argument("--ctx", type=int, default=512)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rank", type=int, default=8)
    ap.add_argument("--tiny", action="store_true", help="the 2-layer test model (rehearsal of the script, not a measurement)")
    a = ap.parse_args()
    model, _ = load_synthetic(device="cuda:0", blind_model=True, tiny=a.tiny)
    cfg = model.cfg
    qkv4 = {f"ad{i}": adapter(cfg, ALL[:1], a.rank, 10 + i) for i in range(4)}
    all4 = {f"ad{i}": adapter(cfg, ALL, a.rank, 20 + i) for i in range(4)}

    def attach(kind):
        """-> the row table to write after the prefill (None: leave it alone)."""
        model.set_adapter_bank({})
        model.set_adapters({})
        if kind == "none":
            return None
        if kind.startswith("one_"):
            model.set_adapters((qkv4 if kind == "one_qkv" else all4)["ad0"])
            return None
        _, targets, rows = kind.split("_")
        model.set_adapter_bank(qkv4 if targets == "qkv" else all4)
        return {"one": lambda B: [0] * B, "spread": lambda B: [i % 4 for i in range(B)], "off": lambda B: [-1] * B}[rows]

    kinds = ["none", "one_qkv", "one_all", "bank_qkv_one", "bank_qkv_spread", "bank_qkv_off", "bank_all_one", "bank_all_spread", "bank_all_off"]
    for B in [int(x) for x in a.batches.split(",")]:
        ids = torch.randint(3, 32000, (B, a.ctx), dtype=torch.int64, generator=torch.Generator().manual_seed(B))
        times = {k: [] for k in kinds}
        for _ in range(a.reps):
            for kind in kinds:
                rows = attach(kind)
                logits, cache = model(input_ids=ids, max_tokens=2 * a.steps + 8, **({} if rows is None else {"row_adapters": rows(B)}))
                tok = ops.argmax(logits[:, -1].contiguous())[:, None]
                _, tok = timed(model, tok, cache, a.steps)              # capture + warm up
                t, tok = timed(model, tok, cache, a.steps)
                times[kind].append(t)
                del logits, cache
        med = {k: statistics.median(v) for k, v in times.items()}
        print(json.dumps(dict(B=B, ctx=a.ctx, rank=a.rank, steps=a.steps,
                              step_us={k: round(v, 1) for k, v in med.items()},
                              vs_none={k: round(v / med["none"], 4) for k, v in med.items()},
                              reps={k: [round(x, 1) for x in v] for k, v in times.items()})), flush=True)
        torch.cuda.empty_cache()
    attach("none")


if __name__ == "__main__":
    main()
