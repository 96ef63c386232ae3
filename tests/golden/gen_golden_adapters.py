"""Generator of tests/golden/tiny_adapters_oracle.npz: per-request LoRA adapters on the blind tiny model, from the CPU oracle.

Two synthetic adapters (made as tests/test_model_gpu.py's `_synth_adapter` makes its own) beside the base model:
  A  rank 8 on all four projection types of both layers, generator seed 5, config scale 3.0
  B  rank 1 on self_attn.qkv_proj of the last layer (train_lora's default shape), seed 6, scale 10.0
(with the scale 1.5 of `_synth_adapter` B moves no greedy token of these requests; with 3.0 / 10.0 the prefill logits of any two of
{none, A, B} fail the model tests' logit tolerance against each other on 76 - 94 % of the entries).

Requests: the six text prompts golden_inputs.SERVE_TEXTS[1:], request i ASSIGNED the variant ASSIGN[i], every run at B = 1.
The generator walks lm_head seeds upwards and keeps the first one under which
  * every assigned run is clear on its first step and shows at least two distinct tokens (search_head), and
  * for each of the six ordered pairs (assigned variant -> other variant) some request WITNESSES it: the other variant's run
    (also stored) picks a different token at a step up to which both runs are clear -- so a test that compares a request's
    tokens with its assigned run cannot pass with another variant, or none, applied to that row.
Stored: head seed, spread, rel_tol, adapter seeds / scales, ASSIGN, tokens and margins [6, 3, SERVE_STEPS] (variant order
VARIANTS), the witness list [(request, assigned, other, step)].  Regenerating reproduces the file byte for byte:

    python tests/golden/gen_golden_adapters.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "oracle"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

VARIANTS = ["none", "A", "B"]
ASSIGN = ["A", "none", "B", "B", "none", "A"]
ALL_TARGETS = ["self_attn.qkv_proj", "self_attn.o_proj", "mlp.gate_up_proj", "mlp.down_proj"]
ADAPTER_SPECS = {"A": dict(targets=ALL_TARGETS, layers=[0, 1], rank=8, seed=5, scale=3.0),
                 "B": dict(targets=["self_attn.qkv_proj"], layers=1, rank=1, seed=6, scale=10.0)}
FIXTURE = os.path.join(HERE, "tiny_adapters_oracle.npz")
MAX_SEEDS = 20000


def synth_adapter(cfg, targets, layers, rank, seed, scale):
    """A 'trained' adapter in the reference's file format (adapter_config.json dict, adapters.safetensors dict): lora_a ~
    U(-1/sqrt(in), 1/sqrt(in)) as LoRALinear.__init__ (phi.py:121-126), lora_b non-zero."""
    gen = torch.Generator().manual_seed(seed)
    H, I = cfg.hidden_size, cfg.intermediate_size
    qkv = (cfg.num_attention_heads + 2 * cfg.num_key_value_heads) * (H // cfg.num_attention_heads)
    dims = {"self_attn.qkv_proj": (H, qkv), "self_attn.o_proj": (H, H), "mlp.gate_up_proj": (H, 2 * I), "mlp.down_proj": (I, H)}
    idx = list(range(cfg.num_hidden_layers))[-layers:] if isinstance(layers, int) else layers
    tensors = {}
    for i in idx:
        for t in targets:
            k_in, k_out = dims[t]
            tensors[f"model.layers.{i}.{t}.lora_a"] = (torch.rand((k_in, rank), generator=gen) * 2 - 1) * k_in ** -0.5
            tensors[f"model.layers.{i}.{t}.lora_b"] = torch.randn((rank, k_out), generator=gen) * 0.04
    lora_cfg = {"model_path": "models/x", "adapter_path": "adapters/x", "lora_layers": layers, "lora_targets": targets,
                "lora_parameters": {"rank": rank, "alpha": 2 * rank, "dropout": 0.0, "scale": scale}}
    return lora_cfg, tensors


def fixture_adapter(cfg, name):
    """(adapter_config dict, tensors dict) of fixture adapter "A" or "B" for a model of configuration `cfg`."""
    return synth_adapter(cfg, **ADAPTER_SPECS[name])


def find_witnesses(tokens, margins):
    """[(request, assigned variant index, other variant index, step)]: the first step at which the other variant's run differs
    from the assigned one while both runs are clear up to and including it.  tokens / margins: [6, 3, steps]."""
    wit = []
    for i, name in enumerate(ASSIGN):
        a = VARIANTS.index(name)
        for b in range(len(VARIANTS)):
            if b == a:
                continue
            for s in range(tokens.shape[2]):
                if margins[i, a, s] <= 1.0 or margins[i, b, s] <= 1.0:
                    break
                if tokens[i, a, s] != tokens[i, b, s]:
                    wit.append((i, a, b, s))
                    break
    return wit


def witnesses_cover(wit):
    """Every ordered pair assigned -> other over the three variants has a witness."""
    have = {(a, b) for _, a, b, _ in wit}
    return all((a, b) in have for a in range(3) for b in range(3) if a != b)


def main():
    import phi3v_oracle as orc
    from gen_golden_oracle import COMMON, SPREAD, Prefilled, row_norms, search_head
    from golden_inputs import SERVE_STEPS, SERVE_TEXTS
    from phi_3_vision_mlx_amd.config import make_config, tiny_config_dict
    from phi_3_vision_mlx_amd.processor import Phi3VProcessor
    from phi_3_vision_mlx_amd.weights import peaked_lm_head, resolve_adapter, synth_weights
    cfg = make_config(tiny_config_dict(vision=False))
    w = synth_weights(cfg, seed=0, std_scale=4.0)
    proc = Phi3VProcessor(None)
    runs = {}                                                   # (request, variant) -> Prefilled
    for v, name in enumerate(VARIANTS):
        ad = None if name == "none" else resolve_adapter(cfg, *fixture_adapter(cfg, name))
        o = orc.OraclePhi3V(cfg, w, cache_fp32=True, adapters=ad)
        for i, text in enumerate(SERVE_TEXTS[1:]):
            runs[i, v] = Prefilled(o, proc(text), SERVE_STEPS)
    assigned = [runs[i, VARIANTS.index(name)] for i, name in enumerate(ASSIGN)]
    first = 0
    while True:
        hs, res = search_head(assigned, w["lm_head.weight"], SERVE_STEPS, max_seeds=MAX_SEEDS - first, first_seed=first, need=1,
                              min_distinct=2)
        head = peaked_lm_head(w["lm_head.weight"].to(torch.float32), SPREAD, hs)
        norms = row_norms(head)
        tokens = np.zeros((len(ASSIGN), len(VARIANTS), SERVE_STEPS), dtype=np.int32)
        margins = np.zeros(tokens.shape, dtype=np.float32)
        for i, name in enumerate(ASSIGN):
            for v in range(len(VARIANTS)):                      # (i) the other two variants under the same head, as they come
                r = res[i] if v == VARIANTS.index(name) else runs[i, v].greedy(head, SERVE_STEPS, need_clear_steps=0, norms=norms)
                tokens[i, v], margins[i, v] = r[0].reshape(-1).numpy(), r[2].reshape(-1).numpy()
        wit = find_witnesses(tokens, margins)
        print(f"  head seed {hs}: {len(wit)} witnesses {wit}", flush=True)
        if witnesses_cover(wit):                                # (ii)
            break
        first = hs + 1
    assert all(margins[i, VARIANTS.index(n), 0] > 1.0 for i, n in enumerate(ASSIGN))
    assert witnesses_cover(wit) and tokens.shape == (6, 3, SERVE_STEPS)
    out = dict(COMMON, head_seed=np.asarray([hs], dtype=np.int32),
               adapter_seeds=np.asarray([ADAPTER_SPECS[n]["seed"] for n in ("A", "B")], dtype=np.int32),
               adapter_scales=np.asarray([ADAPTER_SPECS[n]["scale"] for n in ("A", "B")], dtype=np.float32),
               assign=np.asarray([VARIANTS.index(n) for n in ASSIGN], dtype=np.int32),
               tokens=tokens, margins=margins, witnesses=np.asarray(wit, dtype=np.int32).reshape(-1, 4))
    np.savez_compressed(FIXTURE, **out)
    print(f"wrote {os.path.basename(FIXTURE)}: head seed {hs}, {len(wit)} witnesses, tokens of the assigned runs "
          f"{[tokens[i, VARIANTS.index(n)].tolist() for i, n in enumerate(ASSIGN)]}")


if __name__ == "__main__":
    main()
