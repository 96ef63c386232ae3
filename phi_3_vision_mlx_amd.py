"""Import shim: makes the hyphenated package directory ``phi-3-vision-mlx_amd/``
importable as ``phi_3_vision_mlx_amd`` and re-exports the reference's public
API (`load/generate/choose/constrain/benchmark`, reference
phi_3_vision_mlx.py:1178-1487) so that
``from phi_3_vision_mlx_amd import generate`` is the drop-in for
``from phi_3_vision_mlx import generate``.
"""
import os as _os

_PKG_DIR = _os.path.join(_os.path.dirname(_os.path.abspath(__file__)), "phi-3-vision-mlx_amd")
__path__ = [_PKG_DIR]
__package__ = __name__
if __spec__ is not None:
    __spec__.submodule_search_locations = __path__

from phi_3_vision_mlx_amd import api as _api  # noqa: E402
from phi_3_vision_mlx_amd.api import (  # noqa: E402,F401
    ID_ASS, ID_EOS, VDB, LogitStopper, Streamer, TokenStopper, benchmark, choose,
    constrain, embed, load,
)


def generate(prompt, images=None, preload=None, blind_model=False, quantize_model=False, quantize_cache=False,
             use_adapter=False, max_tokens=512, verbose=True, return_tps=False, early_stop=False, stream=True,
             apply_chat_template=True, enable_api=False):
    """The reference's `generate`, with its exact signature (greedy).  Seeded sampling is
    `phi_3_vision_mlx_amd.api.generate(..., temperature=, top_k=, top_p=, seed=)`."""
    return _api.generate(prompt, images, preload, blind_model, quantize_model, quantize_cache, use_adapter, max_tokens,
                         verbose, return_tps, early_stop, stream, apply_chat_template, enable_api)
