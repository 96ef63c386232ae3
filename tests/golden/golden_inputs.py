"""Seeded inputs shared by the golden-vector generator (which feeds them to the
reference) and the tests (which feed them to the build)."""
import contextlib
import re

import numpy as np

# name -> (width, height, kind, seed)
IMAGE_CASES = {
    "sq336": (336, 336, "noise", 0),        # BASELINE config 2: 1344x1344 HD, 17 crops, 2509 tokens
    "land640x480": (640, 480, "smooth", 1),  # 1008x1344 HD, 13 live crops
    "port500x1000": (500, 1000, "noise", 2),  # portrait -> transposed path
    "wide900x300": (900, 300, "smooth", 3),  # height needs white padding
}

TOKENIZE_TEXTS = ["ab", "abcde", "xyz"]
MERGE_PROMPT = "<|user|>\n<|image_1|>\nhi<|end|>\n<|assistant|>\n"


def make_image(w, h, kind, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    if kind == "noise":
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    else:
        yy, xx = np.mgrid[0:h, 0:w]
        ph = rng.uniform(0, 6.28, 3)
        a = np.stack([127.5 + 127.5 * np.sin(xx / (17.0 + 5 * c) + yy / (29.0 - 3 * c) + ph[c]) for c in range(3)], -1)
        a = a.clip(0, 255).astype(np.uint8)
    return Image.fromarray(a, "RGB")


# A mixed request set for the tiny vision model (serving / sharding tests): user prompts (request 0 carries an image) and
# the same prompts as the chat template renders them (phi_3_vision_mlx.py:346-351).  tests/golden/tiny_serve_oracle.npz
# holds the per-request B = 1 oracle tokens.
SERVE_PROMPTS = ["What is shown?", "hi", ("a longer question " * 6).strip(), "mid size prompt here", "x",
                 ("tell me more about it " * 3).strip(), "last one"]
SERVE_TEXTS = [f"<|user|>\n{'<|image_1|>' + chr(10) if i == 0 else ''}{p}<|end|>\n<|assistant|>\n" for i, p in enumerate(SERVE_PROMPTS)]
SERVE_STEPS = 6


def serve_requests(proc):
    """B = 1 model inputs of SERVE_TEXTS (request 0 carries the seeded 336x336 noise image)."""
    return [proc(t, [make_image(336, 336, "noise", 0)]) if "<|image_1|>" in t else proc(t) for t in SERVE_TEXTS]


class _Enc:
    def __init__(self, input_ids):
        self.input_ids = input_ids


class FakeTokenizer:
    """BOS(1)-prepending character tokenizer with single ids for chat markers."""
    SPECIAL = {"<|user|>": 32010, "<|end|>": 32007, "<|assistant|>": 32001}

    def _one(self, t):
        ids = [1]
        for part in re.split("(" + "|".join(re.escape(k) for k in self.SPECIAL) + ")", t):
            if part in self.SPECIAL:
                ids.append(self.SPECIAL[part])
            else:
                ids.extend(100 + ord(ch) for ch in part)
        return ids

    def __call__(self, texts):
        if isinstance(texts, str):
            return _Enc(self._one(texts))
        return _Enc([self._one(t) for t in texts])


# synthetic requests of the BASELINE configs live in the package (bench.py uses them too)
import os as _os
import sys as _sys
_sys.path.insert(0, _os.path.dirname(_os.path.dirname(_os.path.dirname(_os.path.abspath(__file__)))))
from phi_3_vision_mlx_amd.workloads import c4_share, text_request, vqa_request  # noqa: E402,F401


# ref_live_blind.json (gen_golden_refmodel.py live): the reference's model-level contract and `_generate` on a blind tiny checkpoint
LIVE_PROMPTS = ["<|user|>\nabc<|end|>\n<|assistant|>\n", "<|user|>\na much longer second prompt<|end|>\n<|assistant|>\n"]
LIVE_GEN_PROMPTS = ["<|user|>\nPick A or B.<|end|>\n<|assistant|>\n", "<|user|>\nhello<|end|>\n<|assistant|>\n"]
LIVE_STEP = [[5, 9, 11], [7, 8, 12]]
LIVE_BEAM = [[3, 4]] * 6


def live_blind_weights():
    """-> (config dict, weights) of the blind tiny checkpoint of ref_live_blind.json (seed 3, peaked head)."""
    from phi_3_vision_mlx_amd.config import make_config, tiny_config_dict
    from phi_3_vision_mlx_amd.weights import synth_weights
    d = tiny_config_dict(vision=False)
    return d, synth_weights(make_config(d), seed=3, std_scale=4.0, lm_head_spread=4.0, lm_head_seed=1)


@contextlib.contextmanager
def one_thread():
    """torch-CPU on one thread: how a multi-threaded fp32 GEMM splits its work follows the thread count, so bits recorded on one
    machine hold on another only at a fixed count (ref_live_blind.json is recorded and checked at one)."""
    import torch
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def tensor_digest(t):
    """dtype, shape and sha256 of a tensor's bytes: equal digests <=> bit-identical tensors."""
    import hashlib
    import torch
    t = t.detach().contiguous()
    return {"dtype": str(t.dtype), "shape": list(t.shape),
            "sha256": hashlib.sha256(t.reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()}
