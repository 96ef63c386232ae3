"""Generator of tests/golden/tiny_embed_oracle.npz: the embedding fixture on the tiny synthetic VISION checkpoint, from the CPU oracle.

`OraclePhi3V.backbone` already returns the final-normed hidden state api.embed pools, so the fixture is that state's last row and
its mean over the live rows (fp64 sum of the bf16 rows, stored fp32), UN-normalised, for
  * "text":  one chat-templated text prompt,
  * "batch": three prompts of different lengths as ONE left-padded batch (the processor's mask / position ids),
  * "image": one prompt with the 336 x 336 seed-0 picture of the smoke test.
The model is `synth_weights(tiny vision config, seed=0, std_scale=4.0)`, as `api.load_synthetic(tiny=True, seed=0, std_scale=4.0)`
builds it.  Stored per request: input ids, live-token counts, `last` and `mean` [B, H].  Regenerating reproduces the arrays:

    python tests/golden/gen_golden_embed.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "oracle"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

FIXTURE = os.path.join(HERE, "tiny_embed_oracle.npz")
TEXT = "Which shelf holds the maps?"
BATCH = ["Maps.", "Which shelf holds the maps of the northern coast?", "Name a colour of the sky."]
IMAGE_PROMPT = "<|image_1|>\nWhat is shown?"


def image():
    from PIL import Image
    return Image.fromarray(np.random.default_rng(0).integers(0, 256, (336, 336, 3), dtype=np.uint8))


def requests():
    """name -> (prompt or list of prompts, images) as api.embed takes them (chat template applied there)."""
    return {"text": (TEXT, None), "batch": (BATCH, None), "image": (IMAGE_PROMPT, [image()])}


def main():
    import torch
    import phi3v_oracle as orc
    from phi_3_vision_mlx_amd.api import _apply_chat_template, _make_processor
    from phi_3_vision_mlx_amd.config import make_config, tiny_config_dict
    from phi_3_vision_mlx_amd.weights import synth_weights
    cfg = make_config(tiny_config_dict(vision=True))
    o = orc.OraclePhi3V(cfg, synth_weights(cfg, seed=0, std_scale=4.0))
    processor = _make_processor(cfg, None)
    out = {}
    for name, (prompt, images) in requests().items():
        text, imgs = _apply_chat_template(prompt, images, False)
        inp = processor(text, imgs)
        ids = np.asarray(inp["input_ids"])
        ids = ids[None] if ids.ndim == 1 else ids
        h, _ = o.backbone(inp["input_ids"], inp.get("pixel_values"), inp.get("image_sizes"), inp.get("positions"), None, inp.get("pids"),
                          inp.get("mask"), 0, None, 1)
        h = h.to(torch.float64).reshape(ids.shape[0], ids.shape[1], -1)
        live = torch.as_tensor(np.asarray(inp["mask"]).reshape(ids.shape) != 0) if inp.get("mask") is not None else torch.ones(ids.shape, dtype=torch.bool)
        n = live.sum(1, keepdim=True).to(torch.float64)
        out[name + "_ids"] = ids.astype(np.int32)
        out[name + "_live"] = n.reshape(-1).numpy().astype(np.int32)
        out[name + "_last"] = h[:, -1].numpy().astype(np.float32)
        out[name + "_mean"] = ((h * live[:, :, None]).sum(1) / n).numpy().astype(np.float32)
        print(f"  {name}: ids {ids.shape}, live {out[name + '_live'].tolist()}, |last|max {np.abs(out[name + '_last']).max():.3f}, "
              f"|mean|max {np.abs(out[name + '_mean']).max():.3f}", flush=True)
    np.savez_compressed(FIXTURE, **out)
    print(f"wrote {os.path.basename(FIXTURE)}: {os.path.getsize(FIXTURE)} bytes")


if __name__ == "__main__":
    main()
