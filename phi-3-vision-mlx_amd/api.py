"""Public inference API -- the drop-in boundary.

Same names, signatures, defaults, return types and error behaviour as the
reference's `load / generate / choose / constrain / benchmark`
(reference phi_3_vision_mlx.py:1178-1487) and the decoding loops underneath
(`_generate :376-409`, `_choose_from :466-487`, `_constrain :500-619`,
`Streamer / LogitStopper / TokenStopper :45-117`, `_apply_chat_template :341-357`).
Host code stays Python; everything that touches the device goes through
`model(...)` (model.py) and `model_ops` (ops.py), i.e. hand-written HIP kernels.

`quantize_cache=True` selects the int8 KV cache and `quantize_model=True` fp8 (e4m3) decoder weights (or the reference's
own 4-bit group-64 format: an MLX `*_Q` checkpoint directory if present, or `quantize_format="int4"`) -- the build's
analogues of the reference's 4-bit prompt cache / int4 weights (BASELINE config 5).
`use_adapter=True` attaches the LoRA adapter of `adapters/<model dir name>` (or `adapter_path=...`) at inference
(reference phi_3_vision_mlx.py:266-271); training adapters is not part of this build.
Not carried over (out of scope): the `<|api_input|>` tool hook,
HF-hub download (`_setup`): a model directory must exist locally, or pass
`synthetic=...` to `load()` for seeded random weights of the real architecture.
"""
import json
import math
import os
import sys
import time
from io import BytesIO
from pathlib import Path

import numpy as np
import torch

from . import ops as model_ops
from . import sampling as sampling_mod
from . import logprobs as logprobs_mod
from . import penalties as penalties_mod
from . import guide as guide_mod
from . import parallel as parallel_mod
from . import row_options
from .steps import kind_for
from .config import is_vision, load_config, make_config, phi3v_config_dict, tiny_config_dict
from .processor import Phi3FProcessor, Phi3VProcessor
from .weights import load_adapter, load_safetensors_dir, resolve_adapter, synth_weights
from .retrieval import VDB  # noqa: F401

PATH_ADAPTERS = "adapters"
PATH_ORIGINAL_PHI3_VISION = "models/phi3_v"
PATH_QUANTIZED_PHI3_VISION = "models/phi3_v_Q"
PATH_ORIGINAL_PHI3_BLIND = "models/phi3_mini_128k"
PATH_QUANTIZED_PHI3_BLIND = "models/phi3_mini_128k_Q"
ID_EOS = 32007
ID_ASS = 32001


class Tic:
    """reference phi.py:16-24."""

    def __init__(self):
        self.last_time = time.perf_counter()

    def __call__(self):
        now = time.perf_counter()
        dt, self.last_time = now - self.last_time, now
        return dt


def _rows(token):
    """token: int tensor [B,1] / [B] or nested list -> list[int] per row (one D2H copy).  A negative id is the device's
    report of a failed step (NaN logits, see p3v_argmax / p3v_step_end): raise instead of decoding garbage."""
    rows = token.reshape(-1).tolist() if torch.is_tensor(token) else np.asarray(token).reshape(-1).tolist()
    if rows and min(rows) < 0:
        raise RuntimeError(f"device step failed: NaN logits (token ids {rows})")
    return rows


class _StepFailed(RuntimeError):
    """a decode step delivered a negative token id (NaN logits, or a poisoned row)"""


class Streamer:
    """reference phi_3_vision_mlx.py:45-77."""

    def __init__(self, processor, stream, mute):
        self.tokenizer = processor.tokenizer
        self.mute = mute
        self.stream = stream and (not mute)
        self.list_tokens = []
        self.idx_sofar = 0

    def __call__(self, token):
        rows = _rows(token)
        if not self.stream:
            self.list_tokens.append(rows)
            return None
        if len(rows) > 1:
            self.list_tokens.append(rows)
            self.stream = False
            return None
        self.list_tokens.append(rows[0])
        txt = self.tokenizer.decode(self.list_tokens)
        idx_split = txt.rfind(" ", self.idx_sofar)
        if idx_split > 0:
            print(txt[self.idx_sofar:idx_split], end="", flush=True)
            self.idx_sofar = idx_split

    def end(self):
        if self.stream:
            txt = self.tokenizer.decode(self.list_tokens)
            print(txt[self.idx_sofar:], "\n", flush=True)
            return txt, len(self.list_tokens)
        steps = [s if isinstance(s, list) else [s] for s in self.list_tokens]
        per_row = [list(r) for r in zip(*steps)]                  # [B][n_steps]
        list_txt = self.tokenizer.batch_decode([(r[:r.index(ID_EOS) + 1] if ID_EOS in r else r) for r in per_row])
        if not self.mute:
            for i, gen in enumerate(list_txt):
                print(f"\n< Generated text for prompt #{i} >\n{gen}")
        return list_txt, sum(len(r) for r in per_row)


class LogitStopper:
    """Early-stop heuristic, B=1 only (reference phi_3_vision_mlx.py:79-104)."""

    def __init__(self, max_tokens, early_stop):
        self.step = 0
        # isinstance(True, int) holds in Python: the reference takes early_stop=True as the integer 1 (:82) -- kept
        self.early_stop = early_stop if isinstance(early_stop, int) and (early_stop < max_tokens) else False
        self.log_prob_sum = 0.0
        self.best_eos_sofar = -math.inf
        self.log_prob_sum_at_best_eos = 0.0

    def __call__(self, logits):
        if not self.early_stop:
            return False
        if logits.shape[0] > 1:
            self.early_stop = False
            return False
        log_prob = model_ops.log_softmax(logits[:, -1, :].contiguous())
        log_prob_best = log_prob.float().max().item()
        log_prob_eos = log_prob[0, ID_EOS].float().item()
        if log_prob_eos > self.best_eos_sofar:
            self.log_prob_sum_since_last_best_eos = self.log_prob_sum - self.log_prob_sum_at_best_eos
            if (self.log_prob_sum_since_last_best_eos < self.best_eos_sofar) and (self.step > self.early_stop):
                return True
            self.best_eos_sofar = log_prob_eos
            self.log_prob_sum_at_best_eos = self.log_prob_sum
        self.log_prob_sum += log_prob_best
        self.step += 1
        return False


class TokenStopper:
    """Stop when every row has emitted EOS (reference phi_3_vision_mlx.py:105-117)."""

    def __init__(self, processor, batch_size):
        self.tokenizer = processor.tokenizer
        self.eos_id = ID_EOS
        self.batch_size = batch_size
        self.eos_rows = [1] * batch_size

    def __call__(self, token):
        rows = _rows(token)
        if self.eos_id in rows:
            self.eos_rows = [a * int(t != self.eos_id) for a, t in zip(self.eos_rows, rows)]
            if sum(self.eos_rows) < 1:
                return True
        return False


# ----------------------------------------------------------------------------- loading
def _load_image(image_source):
    """reference phi_3_vision_mlx.py:307-326 (PIL images are passed through)."""
    from PIL import Image
    if isinstance(image_source, Image.Image):
        return image_source
    if isinstance(image_source, BytesIO):
        try:
            return Image.open(image_source)
        except IOError as e:
            raise ValueError(f"Failed to load image from BytesIO with error: {e}")
    elif image_source.startswith(("http://", "https://")):
        try:
            import requests
            response = requests.get(image_source, stream=True)
            response.raise_for_status()
            return Image.open(response.raw)
        except Exception as e:
            raise ValueError(f"Failed to load image from URL: {image_source} with error {e}")
    elif Path(image_source).is_file():
        try:
            return Image.open(image_source)
        except IOError as e:
            raise ValueError(f"Failed to load image {image_source} with error: {e}")
    else:
        raise ValueError(f"The image {image_source} must be a valid URL or existing file.")


def _apply_chat_template(prompt, images, verbose, apply_chat_template=True):
    """reference phi_3_vision_mlx.py:341-357."""
    if apply_chat_template is False:
        print(f"*** Prompt ***\n{prompt}\n*** Images ***\n{images}\n*** Output ***") if verbose else None
        return prompt, images
    if images is not None:
        images = [_load_image(i) for i in images] if isinstance(images, list) else [_load_image(images)]
        img_prompt = "\n".join([f"<|image_{i+1}|>" for i in range(len(images))]) + "\n"
    else:
        img_prompt = ""
    prompt = [prompt] if isinstance(prompt, str) else prompt
    prompt = [f"<|user|>\n{img_prompt}{i.strip()}<|end|>\n<|assistant|>\n" for i in prompt]
    if verbose:
        prompt_str = "\n".join(map(str.strip, prompt)).strip()
        images_str = "\n".join(map(str, images)) if images else "None"
        print(f"*** Prompt ***\n{prompt_str}\n*** Images ***\n{images_str}\n*** Output ***")
    prompt = prompt[0] if len(prompt) == 1 else prompt
    return prompt, images


def _get_cfg(json_path, **kwargs):
    return load_config(json_path, **kwargs)


def _make_processor(cfg, model_path, return_mx=True):
    cls = Phi3VProcessor if is_vision(cfg) else Phi3FProcessor
    return cls(model_path, return_mx=return_mx)


def _load(model_path=PATH_ORIGINAL_PHI3_VISION, adapter_path=None, return_mx=True, device=None, **kwargs):
    """reference phi_3_vision_mlx.py:257-274: config -> model class by `architectures[0]`,
    HF safetensors -> device weights."""
    from .model import Phi3VModel
    cfg = _get_cfg(f"{model_path}/config.json", **kwargs)
    processor = _make_processor(cfg, model_path, return_mx)
    device = device or f"cuda:{torch.cuda.current_device()}"
    model = Phi3VModel(cfg, load_safetensors_dir(model_path, cfg, device="cpu"), device=device)
    if adapter_path:
        _attach_adapter(model, adapter_path, model_path)
    return model, processor


def _get_adapter_path(model_path):
    """reference phi_3_vision_mlx.py:462-464."""
    print(f"{PATH_ADAPTERS}/{Path(model_path).name}")
    return f"{PATH_ADAPTERS}/{Path(model_path).name}"


def _attach_adapter(model, adapter_path, model_path=None):
    """reference phi_3_vision_mlx.py:266-271: adapter_config.json -> LoRA layers, adapters.safetensors -> their weights."""
    lora_cfg, tensors = load_adapter(adapter_path)
    if model_path is not None and lora_cfg.get("model_path") != model_path:
        print(f"WARNING: LoRA trained for {lora_cfg.get('model_path')} is being used with {model_path}")
    model.set_adapters(resolve_adapter(model.cfg, lora_cfg, tensors))


def load_adapters(preload, adapters, model_path=None):
    """Attach an adapter BANK to a loaded model: {name: adapter directory} in the reference's format (adapter_config.json +
    adapters.safetensors, what `train_lora` writes).  All of them stay resident beside the one set of frozen weights;
    `generate(..., adapter=name)`, `engine.submit(..., adapter=name)` and the server's "adapter" field pick one per request, rows
    with different adapters (or none) share one captured decode step (model.set_adapter_bank).  `model_path`: warn, as `load`
    does for its one adapter, when an adapter was trained for another checkpoint.  Returns the names."""
    model = preload[0]
    bank = {}
    for name, path in dict(adapters).items():
        lora_cfg, tensors = load_adapter(path)
        if model_path is not None and lora_cfg.get("model_path") != model_path:
            print(f"WARNING: LoRA trained for {lora_cfg.get('model_path')} is being used with {model_path}")
        bank[name] = resolve_adapter(model.cfg, lora_cfg, tensors)
    model.set_adapter_bank(bank)
    return list(model.adapter_names)


def load_synthetic(blind_model=False, tiny=False, seed=0, device=None, std_scale=1.0, adapter_path=None, lm_head_spread=0.0,
                   lm_head_seed=0, outliers=None, residual_scale=None, **kwargs):
    """Seeded random weights of the real (or tiny) architecture -- no checkpoint needed.
    lm_head_spread / lm_head_seed: decisive-argmax head of the parity fixtures (weights.peaked_lm_head);
    outliers: heavy-tailed activations (weights.add_outliers); residual_scale: the well-conditioned checkpoint (weights.synth_weights)."""
    from .model import Phi3VModel
    d = tiny_config_dict(vision=not blind_model) if tiny else phi3v_config_dict(vision=not blind_model)
    cfg = make_config(d, **kwargs)
    device = device or f"cuda:{torch.cuda.current_device()}"
    model = Phi3VModel(cfg, synth_weights(cfg, seed=seed, device=device, std_scale=std_scale, lm_head_spread=lm_head_spread,
                                          lm_head_seed=lm_head_seed, outliers=outliers, residual_scale=residual_scale), device=device)
    if adapter_path:
        _attach_adapter(model, adapter_path)
    return model, _make_processor(cfg, None)


def load(blind_model=False, quantize_model=False, quantize_cache=False, use_adapter=False, **kwargs):
    """reference phi_3_vision_mlx.py:1279-1322.  Extra: `synthetic=True|'tiny'` builds seeded
    random weights instead of reading `models/...` (there is no hub access here)."""
    synthetic = kwargs.pop("synthetic", None)
    adapter_path = kwargs.pop("adapter_path", None)
    fmt = kwargs.pop("quantize_format", "fp8")               # on-the-fly weight format of quantize_model=True: "fp8" | "int4"
    if fmt not in ("fp8", "int4"):
        raise ValueError(f"quantize_format must be 'fp8' or 'int4', got {fmt!r}")
    model_path = kwargs.pop("model_path", None)
    if model_path is None:
        model_path = PATH_ORIGINAL_PHI3_BLIND if blind_model else PATH_ORIGINAL_PHI3_VISION
        q_path = PATH_QUANTIZED_PHI3_BLIND if blind_model else PATH_QUANTIZED_PHI3_VISION
        if quantize_model and not synthetic and os.path.exists(q_path):
            model_path, quantize_model = q_path, False          # reference :1305-1311: an MLX 4-bit checkpoint, loaded as is
    if use_adapter and adapter_path is None:
        adapter_path = _get_adapter_path(model_path)                                   # reference :1316-1317
    if synthetic:
        return load_synthetic(blind_model=blind_model, tiny=(synthetic == "tiny"), use_quantized_cache=quantize_cache,
                              quantized_fp8=quantize_model and fmt == "fp8", quantized_int4=quantize_model and fmt == "int4",
                              adapter_path=adapter_path if use_adapter else None, **kwargs)
    if not os.path.exists(model_path):
        raise FileNotFoundError(
            f"model directory {model_path!r} not found and this build cannot download checkpoints; "
            "place HF-layout safetensors + config.json there, or use load(synthetic=True)")
    return _load(model_path=model_path, use_quantized_cache=quantize_cache, quantized_fp8=quantize_model and fmt == "fp8",
                 quantized_int4=quantize_model and fmt == "int4",
                 adapter_path=adapter_path if use_adapter else None, **kwargs)


# ----------------------------------------------------------------------------- generate
def _last_logits(logits):
    return logits[:, -1, :].contiguous()


def greedy_loop(model, token, cache, n_steps, streamer, token_stopper, logit_stopper=None, mask=None, pids=None, sampling=None,
                logprobs=None, penalties=None, guides=None):
    """The decode loop of `_generate` (reference phi_3_vision_mlx.py:390-398): `n_steps` greedy steps after the prefill token,
    every token handed to the streamer and the stoppers in order, stops as the reference stops.

    With the graph-replayed step and no logit stopper the loop is ONE STEP AHEAD of the host: step i + 1 is enqueued (its input
    token never leaves the device) before the host reads token i, so the per-token work the reference does after `mx.eval` --
    D2H copy, Streamer, TokenStopper -- runs while the GPU computes the next step.  Tokens, texts and stop step are identical;
    when a stop fires one speculative step has been enqueued: it is dropped -- the cache offset is rewound past it and the
    STOP step's token is returned, so cache and return value are what the one-sync-per-token loop leaves.  With a logit stopper (it reads step i's logits
    on the host before deciding) or an eager model the loop is the reference's, one sync per token.

    sampling: per-row (temperature, top_k, top_p, seed) tuples (sampling.rows) -- the loop then drives the SAMPLED replay
    (model.sample_step) on records whose draw index starts at 1 (the prefill token was draw 0); None: the greedy replay.

    logprobs: a logprobs.Collector -- the loop then drives the replay that ends in the log-probability launch
    (model.logprob_step / sample_logprob_step: the same step plus one launch) and hands the collector every step's records
    right after the streamer got its tokens.  The one-step-ahead loop reads them from the capture's pinned `records` buffer
    behind the event that guards `history`: no sync and no copy of their own.  None: the replays and launches of today.

    penalties: {"prompt_ids", "pad"} of a state whose rows carry penalty records (model.set_penalties, done by the caller with
    the prefill token drawn from the adjusted prefill logits) -- the loop then drives the PENALISED replay for every step
    (model.penal_step / penal_logprob_step: each step counts the token it is fed), greedy rows under greedy sampling records.
    If the loop re-plans after a failed step, the rows' tables are rebuilt from the prompt and the tokens fed so far rather than
    trusted.  None: the replays and launches of today.

    guides: {"dfas", "table", "eos"} of a state whose rows carry guide records (model.set_guides, done by the caller with the
    prefill token drawn from the masked prefill logits) -- the loop then drives the GUIDED replay for every step
    (model.guide_step / guide_logprob_step: the penalised step plus p3v_guide_mask, which walks the token it is fed).  After a
    re-plan the rows' states are rebuilt by walking the tokens fed so far.  None: the replays and launches of today."""
    # the ONE kind of step the arguments ask for (steps.py); an eager model class has none of its methods: the reference's loop
    kind = kind_for(sampling is not None, penalties is not None, guides is not None, logprobs is not None)
    graph_step, records, want_dev = row_options.begin_loop(model, getattr(cache[0], "state", None), kind, token, sampling,
                                                           logprobs and logprobs.wants, penalties is not None, guides is not None)

    def slot(g_):
        """the pinned records of the replay just enqueued ([B, 20], valid once the step has run)"""
        k_ = g_["n_replays"] - 1
        if k_ >= g_["records"].shape[1]:
            raise RuntimeError(f"logprobs: step {k_} lies beyond the {g_['records'].shape[1]} record slots of this cache (max_tokens)")
        return g_["records"][:, k_]
    ahead = graph_step is not None and (logit_stopper is None or not logit_stopper.early_stop) and torch.is_tensor(token) and token.is_cuda
    if not ahead:
        for _ in range(n_steps):
            if graph_step is not None:
                logits, token = graph_step(token, cache)
            else:
                logits, cache = model(input_ids=token, cache=cache, mask=mask, pids=pids)
                token = (model_ops.argmax(_last_logits(logits)) if records is None else
                         model_ops.sample(_last_logits(logits), records))[:, None]
            rows = _rows(token)                                     # ONE D2H copy per step, shared by the streamer and the stopper
            streamer(rows)
            if logprobs is not None:                                # (the copy above waited for the step, its last launch included)
                logprobs.add(slot(cache[0].state.graphs["greedy"]) if want_dev is None else
                             model_ops.logprobs(_last_logits(logits), token.reshape(-1).to(torch.int32).contiguous(), want_dev))
            if logit_stopper is not None and logit_stopper(logits):
                break
            if token_stopper(rows):
                break
        return token
    B = token.shape[0]
    host = []                                                       # pinned staging buffers of the copy fallback (rarely needed)
    pending = None                                                  # (event, pinned buffer) of the step the host has not read yet

    debug = os.environ.get("P3V_DEBUG_STEP") == "1"
    fail_at = int(os.environ.get("P3V_DEBUG_FAIL_STEP", "-1"))      # tests: report this step's tokens as failed, once
    taken = []
    n_done = 0                                                      # steps of this call whose tokens reached the streamer

    def take(p):
        nonlocal n_done, fail_at
        p[0].synchronize()
        if debug and p[2] is not None:                              # the pinned-history read trusts n_replays == the device's step
            g_, k_ = p[2]                                           # counter; a direct graph.launch() or a d_step reset breaks that
            assert int(g_["d_step"].item()) >= k_ + 1, f"history column {k_} read, device step counter {int(g_['d_step'].item())}"
        rows = p[1].tolist()
        if n_done == fail_at:                                       # (tests) what a poisoned step leaves: a negative token, NaN cache rows
            rows, fail_at = [-1] * len(rows), -1
            torch.cuda.synchronize()
            if not st.quantized:
                st.v[..., st.offset - (i - n_done):st.offset] = float("nan")
                st.k[:, :, :, st.offset - (i - n_done):st.offset] = float("nan")
        if min(rows) < 0:
            raise _StepFailed(f"device step failed: NaN logits (token ids {rows})")
        taken[:] = rows
        n_done += 1
        if penalties is not None or guides is not None:
            delivered.append(list(rows))
        streamer(rows)
        if p[3] is not None:
            logprobs.add(p[3])
        return token_stopper(rows)
    st = cache[0].state
    token0 = token.clone()                                          # (the caller's tensor may be the step's own output buffer)
    delivered = []                                                  # (penalties) every step's tokens, for a rebuild of the tables
    degraded = False
    i = 0
    while True:
        try:
            while i < n_steps:
                _, token = graph_step(token, cache)                 # enqueue step i
                i += 1
                g = st.graphs["greedy"]
                k, hist = g["n_replays"] - 1, g["history"]
                ev = torch.cuda.Event()
                if k < hist.shape[1] and not hist.is_cuda:
                    # the step wrote its tokens into pinned host memory itself (history[:, k], model._build_decode_graph): nothing to
                    # copy, the replays run back to back (an in-line D2H copy node costs the step ~18 us of idle GPU: 550 -> 556 tok/s)
                    ev.record()
                    src, chk = hist[:, k], (g, k)
                else:                                               # (history full, or kept on the device by another model class)
                    if not host:
                        host = [torch.empty((B,), dtype=torch.int32).pin_memory() for _ in range(2)]
                    host[i & 1].copy_(token.reshape(-1), non_blocking=True)   # stream-ordered copy, before the next replay overwrites it
                    ev.record()
                    src, chk = host[i & 1], None
                prev, pending = pending, (ev, src, chk, slot(g) if logprobs is not None else None)
                if prev is not None and take(prev):                 # host work of step i - 2 under the GPU's step i - 1
                    st.offset -= 1                                  # drop the speculative step: its K/V row lies beyond the offset
                    return torch.tensor(taken, dtype=torch.int32, device=token.device).view(-1, 1)
            if pending is not None:
                last, pending = pending, None
                take(last)
            return token
        except _StepFailed:
            # A step delivered no token.  The one launch of the step that depends on the rest of the GPU is the fused attention +
            # o_proj (every workgroup resident at once: another process on the same GPU can starve it until its bound runs out and
            # the row is poisoned).  Once per call: plan without it (as a server-owned model does), rewind to the last good token,
            # go on.  Anything else -- or a second failure -- is raised.
            g = st.graphs.get("greedy")
            if degraded or g is None or not g["bufs"]["plan"].fuse_o:
                st.mark_dirty() if hasattr(st, "mark_dirty") else None    # (a captured-prefill entry on these buffers is dropped)
                raise
            degraded = True
            torch.cuda.synchronize()
            model.serving = True
            st.graphs.clear()
            st.offset -= i - n_done                                 # the failed step and the speculative one behind it
            st.scrub(st.offset, st.offset + i - n_done)             # (their cache rows hold NaN: 0 x NaN would poison every later step)
            i, pending = n_done, None
            token = torch.tensor(taken, dtype=torch.int32, device=token0.device).view(-1, 1) if n_done else token0
            fed = ([_rows(token0)] + delivered)[:n_done] if penalties is not None or guides is not None else None
            row_options.rebuild(model, st, n_done, fed, sampling, penalties, guides)
            print("[phi3v] a decode step timed out in the fused attention + o_proj launch (is another process using this GPU?): "
                  "continuing with separate launches", file=sys.stderr)


def speculative_loop(model, ids, token, cache, n_steps, K, streamer, token_stopper, info=None):
    """`greedy_loop` with speculative verify steps (B = 1, greedy; include/p3v.h "speculative greedy decoding"): up to `n_steps`
    tokens after the prefill token `token`, every one handed to the streamer and the token stopper in order.  `ids`: the ids
    the cache holds (the prompt).  Each replay of model.spec_step emits accepted + 1 tokens; replays are enqueued ahead of the
    host (a step needs no host input), tokens and per-step records are read from pinned memory behind an event.  A stop token
    inside an accepted run, or the n_steps budget, cuts the output there; the cache offset is then what the plain loop leaves:
    prompt + delivered tokens - 1 (rows of dropped tokens lie beyond it).  A negative token raises, as in greedy_loop.
    info (a dict) receives steps / drafted / accepted / emitted.  Returns the last delivered token as an int32 [1, 1] tensor."""
    st = cache[0].state
    S0 = st.offset
    stats = dict(steps=0, drafted=0, accepted=0, emitted=0)
    last = token
    if n_steps > 0:
        g = model.spec_start(cache, ids, token, K, n_limit=S0 + 1 + n_steps)
        hist, rec = g["history"], g["rec"]
        pending, pos, r, delivered, done = [], 0, 0, 0, False
        while not done:
            # every step emits at least one token until the budget is reached: never more replays in flight than tokens missing
            while len(pending) < 2 and len(pending) < n_steps - pos:
                model.spec_step(cache, K)
                ev = torch.cuda.Event()
                ev.record()
                pending.append(ev)
            if not pending:
                break
            pending.pop(0).synchronize()
            c, kd = int(rec[r, 0]), int(rec[r, 1])
            r += 1
            toks = hist[pos:pos + c].tolist()
            pos += c
            if c == 0:
                break
            if min(toks) < 0:
                torch.cuda.current_stream().synchronize()
                st.offset = S0 + delivered
                st.mark_dirty() if hasattr(st, "mark_dirty") else None
                raise RuntimeError(f"device step failed: NaN logits (token ids {toks})")
            stats["steps"] += 1
            stats["drafted"] += kd
            stats["accepted"] += c - 1
            stats["emitted"] += c
            for t in toks:
                streamer([t])
                delivered += 1
                last = t
                if token_stopper([t]):
                    done = True
                    break
            if pos >= n_steps:
                done = True
        if pending:
            torch.cuda.current_stream().synchronize()              # replays enqueued ahead: their rows lie beyond the offset
        st.offset = S0 + delivered
        if not torch.is_tensor(last):
            last = torch.tensor([[last]], dtype=torch.int32, device=token.device)
    if info is not None:
        info.update(stats)
    return last


def beam_loop(model, logits_row, cache, W, max_tokens, length_penalty=1.0, share=False):
    """Beam search of width W behind one prompt's prefill (include/p3v.h "beam search"; the host's part is beam.Search):
    model.beam_start forks the B = 1 state into W rows and launches step 0, every further step is one replay of the captured
    beam step with no host input, so the device runs up to two replays ahead; records are read from pinned memory behind an
    event.  When the search is done the overrun records are dropped and the offset rewound past them (model.beam_sync).  A
    failed step raises, as a negative token does in greedy_loop.  Returns (the beam.Search, the B = W cache)."""
    from . import beam as beam_mod
    search = beam_mod.Search(W, max_tokens, ID_EOS, length_penalty)
    g = model.beam_start(cache, logits_row, W, ID_EOS, share=share)
    bcache, rec, pending, enq, t = g["cache"], g["rec"], [], 1, 0
    ev = torch.cuda.Event()
    ev.record()
    pending.append(ev)
    try:
        while True:
            while len(pending) < 3 and enq < max_tokens:
                model.beam_step(bcache)
                ev = torch.cuda.Event()
                ev.record()
                pending.append(ev)
                enq += 1
            pending.pop(0).synchronize()
            t += 1
            if search.add(rec[t - 1].numpy().copy()):
                break
    finally:
        model.beam_sync(bcache, t)
    return search, bcache


def _generate_beam(model, processor, prompt, images, max_tokens, verbose, return_tps, mute, prefix_cache, share_prefix, W,
                   length_penalty, beam_info):
    """`_generate` with num_beams = W >= 2: one prefill, `beam_loop`, the best pooled hypothesis' text."""
    why = model.beam_refusal(None, W) if hasattr(model, "beam_refusal") else "beam search needs the device model's captured step (this model class has none)"
    if why:
        raise ValueError(why)
    if not isinstance(max_tokens, int) or max_tokens < 1:
        raise ValueError(f"num_beams={W}: max_tokens must be a positive integer, got {max_tokens!r}")
    digests = None
    if prefix_cache is not None and images is not None:
        from .prefix import image_digests
        digests = image_digests(images)
    dict_input = processor(prompt, images)
    tic = Tic()
    if prefix_cache is not None:
        logits, cache = _prefill_with_store(model, prefix_cache, dict_input, digests, max_tokens, {}, False)
    else:
        logits, cache = model(**dict_input, max_tokens=max_tokens)
    prompt_time = tic()
    search, _ = beam_loop(model, logits[:, -1, :], cache, W, max_tokens, length_penalty, share=bool(share_prefix))
    hyps = search.result()
    result = processor.tokenizer.decode(hyps[0]["token_ids"])
    gen_time, steps = tic(), len(search.steps)
    if beam_info is not None:
        beam_info.update(hypotheses=[dict(h) for h in hyps], steps=steps)
    if not mute:
        print(result, "\n", flush=True)
    prompt_len = dict_input["input_ids"].size
    prompt_tps, gen_tps = prompt_len / prompt_time, max(steps - 1, 0) / gen_time
    if verbose:
        print(f"\nPrompt: {prompt_tps:.2f} tokens-per-sec ({prompt_len} tokens / {prompt_time:.1f} sec)")
        print(f"Generate: {gen_tps:.2f} beam steps-per-sec ({steps} steps of {W} beams / {gen_time:.1f} sec)")
    return (prompt_tps, gen_tps) if return_tps else result


def _check_beam(num_beams, length_penalty, prompt, temperature, top_k, top_p, seed, speculate, n, best_of, logprobs, repetition_penalty,
                presence_penalty, frequency_penalty, logit_bias, guided_regex, guided_choice, guided_json, early_stop, adapter):
    """(W, length_penalty) of a call, W = 1: the plain path.  Every refusal of beam search that needs no model, as a ValueError."""
    from . import beam as beam_mod
    W, lp = beam_mod.check_request(num_beams, length_penalty)
    if W == 1:
        return W, lp
    batched = isinstance(prompt, list)
    beam_mod.check_request(W, lp, batched=batched)
    sampled = not sampling_mod.greedy(sampling_mod.rows(1, temperature, top_k, top_p, seed))
    pen = penalties_mod.rows(1, repetition_penalty, presence_penalty, frequency_penalty, logit_bias)
    return beam_mod.check_request(W, lp, batched, sampled, bool(speculate), (n, best_of) not in ((1, None), (1, 1)), logprobs is not None,
                                  not penalties_mod.off(pen), not (guided_regex is None and guided_choice is None and guided_json is None),
                                  bool(early_stop), adapter is not None)


def _check_speculate(model, speculate, batched, sampled, early_stop):
    """The refusals of speculative decoding: a ValueError that names the limit, never a silent fallback."""
    K = int(speculate)
    if K < 0:
        raise ValueError(f"speculate must be >= 0, got {speculate}")
    if batched:
        raise ValueError("speculate: one prompt at a time (B = 1); a list of prompts is not supported")
    if sampled:
        raise ValueError("speculate: greedy decoding only (temperature must be 0)")
    if early_stop:
        raise ValueError("speculate: early_stop is not supported (the logit stopper reads one row per step)")
    why = model.spec_refusal(None, K)
    if why:
        raise ValueError(why)
    return K


def _prefill_with_store(model, store, dict_input, digests, max_tokens, kw_adapter, batched, cache_prompt=True, prefix_len=None):
    """The prefill of `_generate` through a prefix store: look up, restore + compute the rest (or the cold call), capture."""
    from . import prefix as prefix_mod
    ids = np.asarray(dict_input["input_ids"])
    cfg = model.cfg
    kind = "int8" if getattr(cfg, "use_quantized_cache", False) else "bf16"
    if batched or ids.shape[0] != 1 or "mask" in dict_input or max_tokens < 1 or \
            (kind == "int8" and getattr(cfg, "cache_format", "int8") == "mlx4"):
        store.bypass()
        return model(**dict_input, max_tokens=max_tokens, **kw_adapter)
    ids = ids.reshape(-1)
    adapter = (kw_adapter.get("row_adapters") or [None])[0]
    key = store.key(model.epoch, adapter, ids.size + max_tokens > cfg.original_max_position_embeddings, kind)
    hit = store.lookup(ids, digests, key)
    logits, cache = model(**dict_input, max_tokens=max_tokens, **kw_adapter, **({} if hit is None else {"prefix": hit}))
    P = prefix_mod.capture_len(ids, prefix_len)
    nbytes = prefix_mod.kv_bytes(P, cfg.num_hidden_layers, cfg.num_key_value_heads, model.hd, kind)
    if cache_prompt and store.wants(ids, digests, key, P, nbytes):
        store.insert(ids[:P], digests, key, model.capture_prefix(cache[0].state, 0, 0, P))
    return logits, cache


def _generate(model, processor, prompt, images=None, max_tokens=512, verbose=True, return_tps=False, early_stop=False,
              stream=True, mute=False, temperature=0.0, top_k=0, top_p=1.0, seed=None, adapter=None, prefix_cache=None,
              speculate=0, spec_info=None, logprobs=None, logprob_info=None, repetition_penalty=1.0, presence_penalty=0.0,
              frequency_penalty=0.0, logit_bias=None, n=1, best_of=None, family_info=None, share_prefix=False,
              guided_regex=None, guided_choice=None, guided_json=None, num_beams=1, length_penalty=1.0, beam_info=None):
    """Greedy decoding loop (reference phi_3_vision_mlx.py:376-409).  speculate=K > 0 (one prompt, greedy): prompt-lookup
    drafts verified K at a time (`speculative_loop`) -- the same tokens, fewer passes over the weights; spec_info (a dict)
    receives steps / drafted / accepted / emitted.  speculate=0 -- the default -- is the plain path, launch for launch.  adapter: the name of one adapter of the model's bank
    (`load_adapters`) for every row, or one name / None per prompt of a batched call; None -- the default -- is the base model.  temperature > 0 samples instead (include/p3v.h:
    p3v_sample_row_t; each of temperature / top_k / top_p / seed a scalar or a per-row list, see sampling.rows); temperature 0
    -- the default -- is today's greedy path, launch for launch.  prefix_cache: a prefix.PrefixCache -- a single prompt (string)
    reuses the K/V of the longest stored prefix with the same tokens and pictures and leaves its own prefix in the store; a list
    of prompts ignores it (counted as a bypass).  logprobs: None (off: today's path, launch for launch), an int N in 0..8, or one
    such value per prompt -- every generated token's log-probability under the RAW logits, its rank and the N most likely
    tokens (include/p3v.h: p3v_logprob_t); logprob_info (a dict) receives token_ids / token_logprobs / ranks / top_logprobs,
    each a list per prompt (None for a prompt that did not ask) with one entry per token handed to the streamer.
    repetition_penalty (> 0; 1 = off; over prompt and output, the HF / vLLM convention), presence_penalty and frequency_penalty
    (0 = off; over the output), each a scalar or a per-prompt list, and logit_bias ({token id: bias} for every prompt, or one
    mapping / None per prompt; -inf bans a token): the rule of include/p3v.h above p3v_penalty_row_t, applied to every step's
    logits BEFORE temperature, top-k and top-p (a greedy row takes the arg-max of the adjusted row); log-probabilities stay
    those of the raw logits.  The defaults are today's path, launch for launch; under speculate they raise.
    n (1..16; ONE prompt, with or without images) completions of the prompt, returned as a list of n strings: the prompt is
    prefilled ONCE, its B = 1 state forked into a B = m state (model.fork_state: one p3v_kv_fork launch), the m first tokens
    drawn from the one prefill logits row, and the batched loop runs on the m rows (include/p3v.h above p3v_kv_fork_t).
    seed=s gives completion j the seed (s + j) mod 2^64; every per-row argument (temperature, top_k, top_p, seed, logprobs, the
    penalties, logit_bias) is a scalar or one value per GENERATED completion.  At temperature 0 the n completions are equal.
    best_of=m (n <= m <= 16): m completions are generated and the n with the largest cumulative raw-logit log-probability
    through the first EOS are returned, best first, ties to the lower index (logprobs.rank_best_of); logprob_info then
    describes the n returned ones, and family_info (a dict) receives "chosen" (their indices among the m) and "seeds".
    n == 1 without best_of (or best_of 1) is today's path, launch for launch.
    share_prefix=True (bf16 KV cache): the m rows of the family are registered as one (model.fork_state(share=True)) and every
    decode step reads the prompt's K/V once for all of them (include/p3v.h: p3v_attention_decode_family) instead of m times;
    the copies are made all the same.  On a bf16 cache without a family (n == 1, no best_of) it is accepted and does nothing; on a model whose
    cache is int8 or mlx4 it raises whatever n is (the option cannot be honoured there, and says so before anything runs).  False -- the default -- allocates, launches and captures nothing that was not there before.
    guided_regex (a pattern of guide.py's subset) or guided_choice (a non-empty list of strings): the output's UTF-8 bytes up
    to EOS must full-match it -- one value for every prompt, or a list of one value / None per prompt (a per-prompt list of
    choices is a list of lists); both for one prompt raise.  The guide is compiled to a byte-level DFA on the host and walked on
    the device (include/p3v.h: p3v_guide_mask): every step bans, in the penalised logits, the tokens whose bytes the row's
    state does not allow, and allows EOS exactly in accepting states; the sampler then draws as usual and `logprobs` stay those
    of the raw logits.  With n / best_of every completion walks its own state.  max_tokens can still cut the output before
    the pattern completes.  None -- the default -- launches, allocates and captures nothing that was not there before; under
    speculate a guide raises.
    guided_json (a JSON schema: a dict or its JSON text, one for every prompt, or a list of one schema / None per prompt): the
    output is the JSON text of an instance of the schema, in declared key order with at most one space after ':' and ','
    (guide.json_regex lists the keywords it translates and the ones it refuses by name).  It is a third kind of guide and
    excludes the other two for the same prompt; a schema may need more than 255 states and then travels in the wide,
    class-compressed form of the same record and kernel (include/p3v.h: P3V_GUIDE_WIDE), bounded by 65,536 table entries.
    num_beams=W (2..8; ONE prompt, greedy, bf16 KV cache): beam search under the rule of include/p3v.h ("beam search") -- one
    prefill forked into W rows, one replay of the captured beam step per token (`beam_loop`), the text of the best pooled
    hypothesis returned; a hypothesis of l tokens scores sum_logprob / l ** length_penalty (length_penalty >= 0, default 1.0).
    beam_info (a dict) receives "hypotheses" (the pool, best first: token_ids, score, sum_logprob, finished) and "steps".
    Everything beam search does not run beside raises a ValueError that names it.  num_beams=1 -- the default -- is the plain
    path, launch for launch."""
    if images is not None and isinstance(prompt, list):
        raise ValueError("Images cannot be provided when prompt is a list")
    num_beams, length_penalty = _check_beam(num_beams, length_penalty, prompt, temperature, top_k, top_p, seed, speculate, n, best_of,
                                            logprobs, repetition_penalty, presence_penalty, frequency_penalty, logit_bias, guided_regex,
                                            guided_choice, guided_json, early_stop, adapter)
    n, fam = parallel_mod.check(n, best_of)                     # (beam search: _check_beam has left n = 1 alone)
    if share_prefix:
        why = model.family_refusal() if hasattr(model, "family_refusal") else "share_prefix needs the device model (this model class has no family table)"
        if why:
            raise ValueError(why)
    if num_beams > 1:
        return _generate_beam(model, processor, prompt, images, max_tokens, verbose, return_tps, mute, prefix_cache, share_prefix,
                              num_beams, length_penalty, beam_info)
    if fam > 1:                                                 # (n == 1: the model is not asked anything here)
        cfg_ = getattr(model, "cfg", None)
        why = parallel_mod.refusal(fam, isinstance(prompt, list), speculate,
                                   getattr(cfg_, "use_quantized_cache", False) and getattr(cfg_, "cache_format", "int8") == "mlx4",
                                   hasattr(model, "fork_state") and hasattr(model, "sample_step"))
        if why:
            raise ValueError(why)
    fam = fam if fam > 1 else 0                                 # rows of the family; 0: the plain path
    B = fam or (len(prompt) if isinstance(prompt, list) else 1)
    lp_wants = logprobs_mod.wants(logprobs, B)                  # (checked before anything runs)
    logprobs_mod.refuse_speculation(lp_wants, speculate)
    lp_asked = lp_wants
    if fam > n:                                                 # best_of ranks on every row's records: N = 0 where nobody asked
        lp_wants = [0 if w == logprobs_mod.OFF else w for w in (lp_wants or [logprobs_mod.OFF] * fam)]
    pen = penalties_mod.rows(B, repetition_penalty, presence_penalty, frequency_penalty, logit_bias,
                             getattr(getattr(model, "cfg", None), "vocab_size", None))
    pen = None if penalties_mod.off(pen) else pen
    penalties_mod.refuse_speculation(pen, speculate)
    guides = guide_mod.per_prompt(len(prompt) if isinstance(prompt, list) else 1, guided_regex, guided_choice, guided_json)
    guide_mod.refuse_speculation(guides, speculate)
    guide_state = None
    row_options.on_device(model, None, pen is not None, guides is not None)   # (refused before anything runs)
    if guides is not None:                                      # compiled and checked against the vocabulary before anything runs
        table = guide_mod.vocab_for(processor.tokenizer, model.cfg.vocab_size)
        for d in guides:
            if d is not None:
                guide_mod.checked(d, table, ID_EOS)
        guide_state = dict(dfas=guides * fam if fam else guides, table=table, eos=ID_EOS)
    kw_adapter = {}
    if adapter is not None:
        from .engine import _check_adapter, adapter_list
        if fam and not isinstance(adapter, str):
            raise ValueError("n > 1: one adapter name for the family (the prompt is prefilled once, under one adapter)")
        names = adapter_list(adapter, 1 if fam else B)
        for a in names:
            _check_adapter(a, list(getattr(model, "adapter_names", None) or []))
        kw_adapter = {"row_adapters": names}
    rows = sampling_mod.rows(B, temperature, top_k, top_p, seed)
    sampled = None if sampling_mod.greedy(rows) else rows
    if speculate:
        speculate = _check_speculate(model, speculate, isinstance(prompt, list), sampled is not None, early_stop)
        kw_adapter = dict(kw_adapter, extra_tokens=speculate)   # (rides with the prefill call: cache columns for the draft rows)
    logit_stopper = LogitStopper(max_tokens, early_stop)
    streamer = Streamer(processor, stream, mute)
    digests = None
    if prefix_cache is not None and not isinstance(prompt, list) and images is not None:   # (a family is ONE prompt too: B = fam there)
        from .prefix import image_digests                       # of the source images, next to the processor call
        digests = image_digests(images)
    dict_input = processor(prompt, images)
    mask, pids = dict_input.get("mask", None), dict_input.get("pids", None)
    token_stopper = TokenStopper(processor, fam or dict_input["input_ids"].shape[0])
    tic = Tic()
    if prefix_cache is not None:
        logits, cache = _prefill_with_store(model, prefix_cache, dict_input, digests, max_tokens, kw_adapter, isinstance(prompt, list))
    else:
        logits, cache = model(**dict_input, max_tokens=max_tokens, **kw_adapter)
    if fam:
        # ONE prefill behind us: its state forked into `fam` rows (another allocation; the B = 1 state is dropped here), its
        # one logits row repeated -- every row's draw 0 reads it under the row's own record
        cache = model.fork_state(cache[0].state, fam, **({"share": True} if share_prefix else {}))
        if adapter is not None:
            model.set_row_adapters(cache[0].state, [adapter] * fam)
        logits = logits[:, -1:, :].expand(fam, -1, -1).contiguous()
    # the rows' tables, then the first token and its record from the prefill logits (row_options: the engine's order of calls);
    # the one D2H copy of the token = the per-token sync the reference has (mx.eval)
    st, spans = getattr(cache[0], "state", None), [(0, logits.shape[0])]
    asked = row_options.Asked(sampled, pen, guide_state and guide_state["dfas"], lp_wants, alone=True)
    if row_options.on_device(model):
        row_options.install(model, st, spans, asked, dict_input, processor)
    token, first, words = row_options.first_tokens(model, st, spans, asked, logits)
    pen_state = None if pen is None else dict(zip(("prompt_ids", "pad"), row_options.prompt_bits(dict_input, fam)))
    streamer(first)
    collector = None
    if lp_wants is not None:
        collector = logprobs_mod.Collector(lp_wants)
        collector.add(words)
    prompt_time = tic()
    if speculate:
        stats = {}
        speculative_loop(model, dict_input["input_ids"], token, cache, max_tokens - 1, speculate, streamer, token_stopper, stats)
        if spec_info is not None:
            spec_info.update(stats)
    else:
        greedy_loop(model, token, cache, max_tokens - 1, streamer, token_stopper, logit_stopper, mask, pids, sampling=sampled,
                    logprobs=collector, penalties=pen_state, guides=guide_state)
    result, gen_len = streamer.end()
    chosen = list(range(fam or B))
    if fam > n:                                                 # best_of: the n best of the m rows, by their own records
        chosen = logprobs_mod.rank_best_of([[r["token"] for r in rs] for rs in collector.rows],
                                           [[r["logprob"] for r in rs] for rs in collector.rows], n, ID_EOS)
        result = [result[j] for j in chosen]
    if family_info is not None:
        family_info.update(chosen=chosen, seeds=[rows[j][3] for j in chosen])
    if collector is not None and logprob_info is not None and lp_asked is not None:
        logprob_info.update(logprobs_mod.result([collector.rows[j] if lp_asked[j] != logprobs_mod.OFF else None for j in chosen]))
    gen_time = tic()
    prompt_len = dict_input["input_ids"].size
    prompt_tps = prompt_len / prompt_time
    gen_tps = (gen_len - 1) / gen_time
    if verbose:
        print(f"\nPrompt: {prompt_tps:.2f} tokens-per-sec ({prompt_len} tokens / {prompt_time:.1f} sec)")
        print(f"Generate: {gen_tps:.2f} tokens-per-sec ({gen_len} tokens / {gen_time:.1f} sec)")
        if speculate:
            print(f"Speculation: {stats['steps']} verify steps, {stats['accepted']} of {stats['drafted']} drafts accepted, "
                  f"{stats['emitted']} tokens emitted")
    if return_tps:
        return prompt_tps, gen_tps
    return result


def generate(prompt, images=None, preload=None, blind_model=False, quantize_model=False, quantize_cache=False,
             use_adapter=False, max_tokens=512, verbose=True, return_tps=False, early_stop=False, stream=True,
             apply_chat_template=True, enable_api=False, temperature=0.0, top_k=0, top_p=1.0, seed=None, adapter=None,
             prefix_cache=None, speculate=0, spec_info=None, logprobs=None, logprob_info=None, repetition_penalty=1.0,
             presence_penalty=0.0, frequency_penalty=0.0, logit_bias=None, n=1, best_of=None, family_info=None,
             share_prefix=False, guided_regex=None, guided_choice=None, guided_json=None, num_beams=1, length_penalty=1.0,
             beam_info=None):
    """reference phi_3_vision_mlx.py:1324-1374, plus beam search (`num_beams=W`, `length_penalty`, `beam_info`, see `_generate`), plus n completions of one prompt from ONE prefill (`n`, `best_of`: a list of n
    strings, see `_generate`), plus speculative greedy decoding (`speculate=K`, see `_generate`), seeded sampling (`_generate`; temperature 0 = greedy, the default) and
    per-request LoRA adapters (`adapter`: a name of the bank `load_adapters` attached, or one name / None per prompt) and the
    prompt prefix cache (`prefix_cache`: a prefix.PrefixCache the caller keeps between calls; single prompts only) and token
    log-probabilities (`logprobs=N`, `logprob_info`, see `_generate`) and the penalties on tokens already seen
    (`repetition_penalty`, `presence_penalty`, `frequency_penalty`) and per-token biases (`logit_bias`), see `_generate`, and
    `share_prefix` (the n rows of a family read their prompt's K/V once per decode step, see `_generate`), and guided decoding
    (`guided_regex`, `guided_choice`, `guided_json`: the output full-matches a regular expression, is one of a list, or is the
    JSON text of an instance of a JSON schema, see `_generate`)."""
    if "<|api_input|>" in prompt and enable_api:
        raise NotImplementedError("the <|api_input|> tool hook is outside the inference hot path of this build")
    num_beams, length_penalty = _check_beam(num_beams, length_penalty, prompt, temperature, top_k, top_p, seed, speculate, n, best_of,
                                            logprobs, repetition_penalty, presence_penalty, frequency_penalty, logit_bias, guided_regex,
                                            guided_choice, guided_json, early_stop, adapter)   # before a model is loaded or run
    n, fam = parallel_mod.check(n, best_of)
    why = parallel_mod.refusal(fam, isinstance(prompt, list), speculate)
    if why:
        raise ValueError(why)
    B = fam if fam > 1 else len(prompt) if isinstance(prompt, list) else 1
    lp_wants = logprobs_mod.wants(logprobs, B)
    logprobs_mod.refuse_speculation(lp_wants, speculate)
    penalties_mod.refuse_speculation(penalties_mod.rows(B, repetition_penalty,
                                                        presence_penalty, frequency_penalty, logit_bias), speculate)
    guide_mod.refuse_speculation(guide_mod.per_prompt(len(prompt) if isinstance(prompt, list) else 1, guided_regex, guided_choice,
                                                      guided_json), speculate)   # (a bad pattern raises here, before a model is loaded)
    if preload is None:
        preload = load(blind_model=blind_model, quantize_model=quantize_model, quantize_cache=quantize_cache, use_adapter=use_adapter)
    return _generate(*preload, *_apply_chat_template(prompt, images, verbose, apply_chat_template), max_tokens=max_tokens,
                     verbose=verbose, return_tps=return_tps, early_stop=early_stop, stream=stream, temperature=temperature,
                     top_k=top_k, top_p=top_p, seed=seed, adapter=adapter, prefix_cache=prefix_cache, speculate=speculate,
                     spec_info=spec_info, logprobs=logprobs, logprob_info=logprob_info, repetition_penalty=repetition_penalty,
                     presence_penalty=presence_penalty, frequency_penalty=frequency_penalty, logit_bias=logit_bias,
                     **({} if (n, best_of, family_info) == (1, None, None) else dict(n=n, best_of=best_of, family_info=family_info)),
                     **({"share_prefix": True} if share_prefix else {}),
                     **({} if guided_regex is None and guided_choice is None else
                        dict(guided_regex=guided_regex, guided_choice=guided_choice)),
                     **({} if guided_json is None else dict(guided_json=guided_json)),
                     **({} if num_beams == 1 else dict(num_beams=num_beams, length_penalty=length_penalty, beam_info=beam_info)))


# ----------------------------------------------------------------------------- score
def _score(model, processor, prompt, images, top):
    return _score_inputs(model, processor(prompt, images), top)


def _score_inputs(model, dict_input, top):
    """One prefill with every position's logits and ONE p3v_logprobs launch over its rows: row i - 1 scores token i."""
    ids = np.asarray(dict_input["input_ids"]).astype(np.int64)
    ids = ids[None] if ids.ndim == 1 else ids
    B, S = ids.shape
    logits, _ = model(**dict_input, full_logits=True)
    V = logits.shape[-1]
    pad = (np.asarray(dict_input["mask"]).reshape(B, S) == 0).sum(1) if "mask" in dict_input else np.zeros(B, dtype=np.int64)
    # row (b, i) scores the token after it; the last row of a prompt has none, rows inside the left padding are skipped
    tok = np.full((B, S), -1, dtype=np.int32)
    tok[:, :-1] = ids[:, 1:]
    want = np.full((B, S), top, dtype=np.int32)
    want[:, -1] = logprobs_mod.OFF
    for b in range(B):
        want[b, :pad[b]] = logprobs_mod.OFF
    dev = logits.device
    words = model_ops.logprobs(logits.view(B * S, V), torch.as_tensor(tok.reshape(-1)).to(dev), torch.as_tensor(want.reshape(-1)).to(dev))
    recs = logprobs_mod.unpack(words)
    out = []
    for b in range(B):
        p = int(pad[b])
        row = [None] * (p + 1) + [recs[b * S + i - 1] if 0 <= ids[b, i] < V else None for i in range(p + 1, S)]
        out.append(dict(token_ids=[int(t) for t in ids[b]], token_logprobs=[None if r is None else r["logprob"] for r in row],
                        ranks=[None if r is None else r["rank"] for r in row],
                        top_logprobs=[None if r is None else list(r["top"]) for r in row]))
    return out


def score(prompt, images=None, preload=None, top=0, apply_chat_template=True):
    """The log-probability of GIVEN text under the model (evaluation, perplexity, reranking): per prompt a dict of token_ids,
    token_logprobs, ranks and top_logprobs (`top` = 0..8 most likely tokens per position), aligned with the prompt's row of
    input ids.  The first token has nothing in front of it: its entries are None, as are those of a batched call's left
    padding and of ids outside the vocabulary (image slots).  The rule is p3v_logprob_t's (include/p3v.h): raw logits, fp64
    log-sum-exp over integer weights.  Returns one dict for a single prompt, a list of them for a list of prompts."""
    top = logprobs_mod.check(top, "top")
    if top == logprobs_mod.OFF:
        raise ValueError(f"top must be an integer in 0..{logprobs_mod.MAX}, got None")
    if images is not None and isinstance(prompt, list):
        raise ValueError("Images cannot be provided when prompt is a list")
    if preload is None:
        preload = load()
    model, processor = preload
    prompt, images = _apply_chat_template(prompt, images, False, apply_chat_template)
    out = _score(model, processor, prompt, images, top)
    return out if isinstance(prompt, list) else out[0]


# ----------------------------------------------------------------------------- embed
POOLINGS = ("last", "mean")


def check_pooling(pooling):
    if pooling not in POOLINGS:
        raise ValueError(f"pooling must be 'last' or 'mean', got {pooling!r}")
    return pooling


def _embed_inputs(model, dict_input, pooling, normalize, kw_adapter=None):
    kw = {k: v for k, v in dict_input.items() if k in ("input_ids", "pixel_values", "image_sizes", "positions", "pids", "mask")}
    return model.embed(**kw, pooling=pooling, normalize=normalize, **(kw_adapter or {}))


def prompt_token_counts(dict_input):
    """Live tokens of every row of a processor result (the left padding of a batch does not count)."""
    ids = np.asarray(dict_input["input_ids"])
    ids = ids[None] if ids.ndim == 1 else ids
    if dict_input.get("mask") is None:
        return [int(ids.shape[1])] * ids.shape[0]
    return [int(n) for n in (np.asarray(dict_input["mask"]).reshape(ids.shape) != 0).sum(1)]


def embed(prompt, images=None, preload=None, pooling="last", normalize=True, adapter=None, apply_chat_template=True, info=None):
    """The prompt as a vector (retrieval, reranking, deduplication, classification heads): the final-normed hidden state of the
    last token (pooling="last", what embedding fine-tunes of this architecture pool) or its mean over the prompt's tokens
    ("mean"), L2-normalised unless normalize=False (include/p3v.h: p3v_embed_pool).  One prefill without lm_head; a list of prompts
    runs as one left-padded batch.  adapter: as in generate.  info (a dict) receives "prompt_tokens", one count per prompt.
    Returns np.float32 [H] for one prompt, [n, H] for a list."""
    check_pooling(pooling)
    if images is not None and isinstance(prompt, list):
        raise ValueError("Images cannot be provided when prompt is a list")
    if preload is None:
        preload = load()
    model, processor = preload
    kw_adapter = {}
    if adapter is not None:
        from .engine import _check_adapter, adapter_list
        names = adapter_list(adapter, len(prompt) if isinstance(prompt, list) else 1)
        for a in names:
            _check_adapter(a, list(getattr(model, "adapter_names", None) or []))
        kw_adapter = {"row_adapters": names}
    prompt, images = _apply_chat_template(prompt, images, False, apply_chat_template)
    dict_input = processor(prompt, images)
    if info is not None:
        info["prompt_tokens"] = prompt_token_counts(dict_input)
    out = _embed_inputs(model, dict_input, pooling, bool(normalize), kw_adapter).cpu().numpy()
    return out if isinstance(prompt, list) else out[0]


# ----------------------------------------------------------------------------- choose
def _choose_from(model, processor, prompt, choices="ABCDE", mute=False):
    """Option scoring with one prefill (reference phi_3_vision_mlx.py:466-487)."""
    def _ord(s):
        return processor([f" {i}" for i in s])["input_ids"][:, -1]
    _was_prompt_str = isinstance(prompt, str)
    options = torch.as_tensor(np.asarray(_ord(choices)), dtype=torch.long)
    dict_input = processor(prompt)
    logits, _ = model(**dict_input, max_tokens=0)
    logp = model_ops.log_softmax(_last_logits(logits))
    picked = logp[:, options.to(logp.device)].float().cpu()
    indices = torch.argmax(picked, dim=-1).tolist()              # first maximum, 5-wide host argmax
    output = [choices[i] for i in indices]
    if not mute:
        if _was_prompt_str:
            print(output[0])
        else:
            for i, o in enumerate(output):
                print(f"\n< Chosen option for prompt #{i} >\n{o}")
    if _was_prompt_str:
        output = output[0]
    return output


def choose(prompt, choices="ABCDE", images=None, preload=None, blind_model=False, quantize_model=False,
           quantize_cache=False, use_adapter=False, verbose=True, apply_chat_template=True):
    """reference phi_3_vision_mlx.py:1376-1423."""
    if preload is None:
        preload = load(blind_model=blind_model, quantize_model=quantize_model, quantize_cache=quantize_cache, use_adapter=use_adapter)
    if apply_chat_template:
        prompt, _ = _apply_chat_template(prompt, images, verbose)
    return _choose_from(*preload, prompt=prompt, choices=choices)


# ----------------------------------------------------------------------------- constrain
def _preprocess(s):
    """reference phi_3_vision_mlx.py:489-493."""
    for i in ["<|system|>", "<|user|>", "<|end|>"]:
        s = s.replace(f"{i} ", f"{i}\n").replace(f"{i}\n\n", f"{i}\n")
    s = s.replace("<|end|><|assistant|>", "<|end|>\n<|assistant|>")
    return s


BF16 = torch.bfloat16


def _sum_last(x):
    return x.float().sum(-1).to(x.dtype)


def _div(x, n):
    return (x.float() / n).to(x.dtype)


def _mean_last(x):
    """`x.mean(axis=-1)` as MLX composes it: sum (rounded to x.dtype) times 1/n (rounded to x.dtype), rounded once more
    (reference phi_3_vision_mlx.py:513 on bf16 scores; tests/golden/mlx_shim.py `mean`)."""
    return _sum_last(x) * torch.tensor(1.0 / x.shape[-1], dtype=x.dtype)


def _already(a2, a1):
    """reference phi_3_vision_mlx.py:495-498: 1 where the row does NOT yet end with a1."""
    if a2.shape[1] < a1.shape[0]:
        return torch.ones(a2.shape[0])
    return (~torch.all(a2[:, -len(a1):] == a1, dim=1)).float()


def constrain_tokens(model, dict_input, constraint, id_constraint, use_beam=False, log_norm=False, trace=None):
    """One (max_new, text) constraint of the reference's `_constrain`
    (phi_3_vision_mlx.py:537-601).  Vocabulary-wide work (log-softmax, argmax,
    top-3) runs in HIP kernels; the [B, C]-sized score bookkeeping is host-side
    on CPU tensors in the logits dtype, like the reference keeps it in bf16.
    Returns (synth_sofar [B, *] int64 padded with ID_EOS, score_sofar [B]).
    trace: optional list receiving (kind, outcome ids / booleans) per data-dependent decision (parity tests walk it
    against the oracle's trace)."""
    dev = model.device
    ar = torch.arange

    def _note(kind, outcome):
        if trace is not None:
            trace.append((kind, torch.as_tensor(outcome).reshape(-1).tolist()))

    def _log_mean(x):
        return _div(_sum_last(x), math.log(x.shape[-1]) if log_norm else x.shape[-1])

    def lsm(logits):                                          # [B, L, V] -> log-probs, same shape (device)
        return model_ops.log_softmax(logits.contiguous())

    def pick(lp, pos_idx, tok):                               # lp[b, pos_idx[j], tok[b, j]] -> host [B, J]
        tok = torch.as_tensor(tok).to(dev).long()
        return lp[ar(lp.shape[0], device=dev)[:, None], torch.as_tensor(pos_idx).to(dev)[None, :], tok].cpu()

    def amax(lp, pos):                                        # host int64 [B]
        return model_ops.argmax(lp[:, pos, :].contiguous()).long().cpu()

    idc = torch.as_tensor(np.asarray(id_constraint)).long()
    C_ = idc.shape[0]
    Bn = np.asarray(dict_input["input_ids"]).shape[0]
    synth_pad = torch.full((Bn, 1), ID_EOS, dtype=torch.long)
    tiled = idc[None].expand(Bn, -1)

    def _get_beam(lp, cache, beam_idx=0, n_beam=3):
        token = amax(lp, beam_idx)
        arg_beam = model_ops.topk(lp[:, beam_idx, :].contiguous(), n_beam).long().cpu()      # (-value, index) order, Q9
        _note("argmax", token), _note("top3_set", arg_beam.sort(dim=-1).values)
        beam = torch.cat([arg_beam.reshape(-1)[:, None], idc[None].expand(Bn * n_beam, -1)], dim=-1)
        bl, _ = model(input_ids=beam, cache=cache, n_beam=n_beam, advance_offset=0)
        bl = lsm(bl)
        s0 = lp[ar(Bn, device=dev)[:, None], beam_idx, arg_beam.to(dev)].cpu().reshape(-1)[:, None]
        s1 = pick(bl, ar(C_), beam[:, 1:])
        score_all = torch.cat([s0, s1], dim=1)
        mean = _mean_last(score_all)
        am = torch.argmax(mean.reshape(-1, n_beam).float(), dim=-1)
        _note("beam_pick", arg_beam[ar(Bn), am])
        return token, arg_beam[ar(Bn), am], score_all.reshape(Bn, n_beam, -1)[ar(Bn), am]

    logits, cache = model(**dict_input, max_tokens=constraint[0] + C_ + 10)
    lp = lsm(logits)                                          # [B, 1, V] (last prompt position)
    score_0 = pick(lp, torch.tensor([lp.shape[1] - 1]), idc[0].expand(Bn)[:, None])[:, 0]
    lr, _ = model(input_ids=tiled, cache=cache, advance_offset=0)
    lr = lsm(lr)
    score_1 = pick(lr, ar(C_ - 1), tiled[:, 1:])
    running_score = lp[:, -1, :].float().max(dim=-1).values.to(lp.dtype).cpu()[:, None]
    pre_score = _log_mean(torch.cat([score_0[:, None], score_1], dim=1))
    pre_synth = torch.cat([tiled, synth_pad], dim=1)
    if use_beam and constraint[0] > 0:
        token, beam_token, beam_score = _get_beam(lp, cache, -1)
        post_score = _log_mean(beam_score)
        post_synth = torch.cat([beam_token[:, None], tiled], dim=1)
        win = pre_score > post_score
        _note("pre_vs_post", win)
        score_sofar = torch.where(win, pre_score, post_score)
        synth_sofar = torch.where(win[:, None], pre_synth, post_synth)
    else:
        token = amax(lp, -1)
        _note("argmax", token)
        score_sofar, synth_sofar = pre_score, pre_synth
    token = token[:, None]
    tokens = []
    finished = torch.ones(Bn)
    for _ in range(constraint[0]):
        tokens.append(token)
        token_plus = torch.cat([token, tiled], dim=1)
        logits, cache = model(input_ids=token_plus, cache=cache, advance_offset=1)
        lp = lsm(logits)
        g = pick(lp, ar(C_), token_plus[:, 1:])
        pre_score = _log_mean(torch.cat([running_score, g], dim=1))
        pre_synth = torch.cat(tokens + [tiled, synth_pad], dim=1)
        if use_beam:
            token, beam_token, beam_score = _get_beam(lp, cache)
            post_score = _log_mean(torch.cat([running_score, beam_score], dim=1))
            post_synth = torch.cat(tokens + [beam_token[:, None], tiled], dim=1)
            win = pre_score > post_score
            _note("pre_vs_post", win)
            score = torch.where(win, pre_score, post_score)
            synth = torch.where(win[:, None], pre_synth, post_synth)
        else:
            token = amax(lp, 0)
            _note("argmax", token)
            score, synth = pre_score, pre_synth
        synth_sofar = torch.cat([synth_sofar, synth_pad], dim=1)
        finished = finished * _already(torch.cat(tokens, dim=1), idc)
        upd = (score > score_sofar).float() * finished
        _note("update", upd)
        synth_sofar = torch.where(upd[:, None] > 0, synth, synth_sofar)
        score_sofar = torch.where(upd > 0, score, score_sofar)
        running_score = torch.cat([running_score, pick(lp, torch.tensor([0]), token[:, None])], dim=1)
        finished = finished * (token != ID_EOS).float()
        if finished.sum() < 1:
            break
        token = token[:, None]
    return synth_sofar, score_sofar


def _constrain(model, processor, prompt, constraints, return_full_text=False, mute=False, use_beam=False, verbose=True,
               log_norm=False):
    """reference phi_3_vision_mlx.py:500-619."""
    _was_prompt_str = isinstance(prompt, str)
    if _was_prompt_str:
        prompt = [prompt]
    tic = Tic()
    constrain_time = 0
    prompt = [_preprocess(s) for s in prompt]
    len_ps = [len(p) for p in prompt]
    output = prompt
    for constraint in constraints:
        if isinstance(constraint, str):
            _output = _choose_from(model, processor, prompt, constraint, True)
            output = [" ".join([p, o]) for p, o in zip(prompt, _output)]
            prompt = output
            continue
        id_constraint = processor.tokenizer.encode(constraint[1], add_special_tokens=False)[1:]
        dict_input = processor(prompt)
        synth_sofar, _ = constrain_tokens(model, dict_input, constraint, id_constraint, use_beam, log_norm)
        constrain_time += tic()
        ids = np.asarray(dict_input["input_ids"])
        output = np.concatenate([ids, synth_sofar.numpy()], axis=1).tolist()
        S = ids.shape[1]
        output = [(i[:i.index(ID_EOS, S)] if ID_EOS in i[S:] else i) for i in output]
        output = [[num for num in sublist if num not in (0, 1)] for sublist in output]
        output = processor.tokenizer.batch_decode(output)
        output = [_preprocess(s) for s in output]
        prompt = output
    if not return_full_text:
        output = [o[l:] for o, l in zip(output, len_ps)]
    if not mute:
        if _was_prompt_str:
            print(output[0])
        else:
            for i, o in enumerate(output):
                print(f"\n< Constrained text for prompt #{i} >\n{o}")
    if verbose:
        print(f"Constrain: {constrain_time:.2f} sec")
    if _was_prompt_str:
        output = output[0]
    return output


def constrain(prompt, constraints=[(0, "\nThe"), (100, " The correct answer is"), "ABCDE"], images=None, preload=None,
              blind_model=False, quantize_model=False, quantize_cache=False, use_adapter=False, verbose=True,
              apply_chat_template=True, use_beam=False):
    """reference phi_3_vision_mlx.py:1425-1487."""
    if preload is None:
        preload = load(blind_model=blind_model, quantize_model=quantize_model, quantize_cache=quantize_cache, use_adapter=use_adapter)
    if apply_chat_template:
        prompt = _apply_chat_template(prompt, None, verbose)[0]
    return _constrain(*preload, prompt=prompt, constraints=constraints, use_beam=use_beam, verbose=verbose)


# ----------------------------------------------------------------------------- benchmark
BENCHMARK_IMAGE_URL = "https://collectionapi.metmuseum.org/api/collection/v1/iiif/344291/725918/main-image"
BENCHMARK_BATCH = [                                            # the reference's list (:1226-1243): 16 literals, 15 prompts --
    "Write an executive summary for a communications business plan",     # a missing comma fuses two of them (kept: same workload)
    "Explain quantum computing.",
    "Write a poem about the first snowfall of the year.",
    "Write a Python function to implement a neural network from scratch, with detailed comments.",
    "Write a resume.",
    "Explain the key concepts of quantum computing and provide a Rust code example demonstrating quantum superposition.",
    "Explain the concept of dark matter and its significance in the universe.",
    "Summarize the major events of the French Revolution.",
    "Describe the water cycle.",
    "Write a Neurology ICU Admission Note.",
    "Describe a bustling alien marketplace on a distant planet with unique goods and creatures."
    "Imagine you have a magic potion that grants one wish. What would you wish for and how would it change your life?",
    "Compose a limerick about a clumsy robot.",
    "Write a JavaScript function to sort an array of objects by a specific property.",
    "Design a database schema for a social media platform, considering user profiles, posts, and interactions.",
    "Implement a basic encryption algorithm in Python.",
]


def _format_benchmark(json_path="benchmark.json"):
    """reference phi_3_vision_mlx.py:427-443: the README's table (decode tokens-per-second per task and variant)."""
    with open(json_path, "r") as f:
        data = json.load(f)
    names = ["Text Generation", "Image Captioning", "Batched Generation"]
    table = """
    | Task                  | Vanilla Model | Quantized Model | Quantized Cache | LoRA Adapter |
    |-----------------------|---------------|-----------------|-----------------|--------------|"""
    for i, name in enumerate(names):
        if i >= len(data["vanilla"]):
            break
        v, qm, qc, lo = (data[k][i][2] for k in ("vanilla", "q_model", "q_cache", "lora"))
        table += f"\n    | {name}{' ' * (22 - len(name))}|  {v:.2f} tps     |  {qm:.2f} tps      |  {qc:.2f} tps       |  {lo:.2f} tps    |"
    print(table)
    return table


def _benchmark_adapter(model, path):
    """The LoRA column needs an adapter; the reference trains one first (`train_lora(take=1)`, :1246-1252 -- training is
    outside this build).  When `path` holds none, write a seeded synthetic one of the shape `train_lora` produces by
    default (last layer, qkv_proj, rank 1, alpha = rank, scale 1; :898, :1011): the kernels do the same work per token."""
    from .weights import ADAPTER_CONFIG, save_adapter
    if os.path.exists(os.path.join(path, ADAPTER_CONFIG)):
        return path
    cfg = model.cfg
    H, hd = cfg.hidden_size, cfg.hidden_size // cfg.num_attention_heads
    n_qkv = (cfg.num_attention_heads + 2 * cfg.num_key_value_heads) * hd
    gen = torch.Generator().manual_seed(0)
    i = cfg.num_hidden_layers - 1
    tensors = {f"model.layers.{i}.self_attn.qkv_proj.lora_a": (torch.rand((H, 1), generator=gen) * 2 - 1) * H ** -0.5,
               f"model.layers.{i}.self_attn.qkv_proj.lora_b": torch.randn((1, n_qkv), generator=gen) * 0.01}
    save_adapter(path, {"model_path": "synthetic", "adapter_path": path, "lora_layers": 1, "lora_targets": ["self_attn.qkv_proj"],
                        "lora_parameters": {"rank": 1, "alpha": 1, "dropout": 0.0, "scale": 1.0}}, tensors)
    return path


def benchmark(blind_model=False, json_path="benchmark.json", *, synthetic=None, image=None, max_tokens=100, adapter_path=None):
    """reference phi_3_vision_mlx.py:1178-1277, like for like: the same three tasks (text generation, image captioning,
    the 15-prompt batch), the same four variants (`vanilla`, `q_model` = quantize_model, `q_cache` = quantize_cache,
    `lora` = use_adapter), 100 new tokens, results[variant] = [[task, prompt_tps, gen_tps], ...] written to `json_path`
    and printed as the README's table (README.md:274-280 holds the reference's Apple M1 Max numbers).
    Keyword-only extras (no network / no checkpoints here): `synthetic=True` uses seeded random weights, `image` replaces
    the museum URL (a seeded 336x336 noise image when the URL cannot be fetched), `adapter_path` names an existing adapter.
    The image task is skipped for `blind_model=True` exactly as the reference's processor would warn and ignore it."""
    if image is None:
        try:
            image = _load_image(BENCHMARK_IMAGE_URL)
        except Exception:
            from PIL import Image
            image = Image.fromarray(np.random.default_rng(0).integers(0, 256, (336, 336, 3), dtype=np.uint8))
    prompts = [("Write a mystery horror.",), ("What is shown in this image?", image), (list(BENCHMARK_BATCH), None)]
    results = {"vanilla": [], "q_model": [], "q_cache": [], "lora": []}
    for method in results:
        kwargs = {"blind_model": blind_model}
        if synthetic:
            kwargs["synthetic"] = synthetic
        if method == "q_model":
            kwargs["quantize_model"] = True
        elif method == "q_cache":
            kwargs["quantize_cache"] = True
        preload = load(**kwargs)
        if method == "lora":
            ap = adapter_path or _benchmark_adapter(preload[0], os.path.join(PATH_ADAPTERS, "benchmark_synthetic" + ("_blind" if blind_model else "")))
            _attach_adapter(preload[0], ap)
        for i, prompt in enumerate(prompts):
            if blind_model and i == 1:
                prompt = prompt[:1]                                # text-only model: the image is ignored (phi.py:247-249)
            prompt_tps, gen_tps = generate(*prompt, preload=preload, max_tokens=max_tokens, return_tps=True, verbose=False)
            results[method].append([i, prompt_tps, gen_tps])
        del preload
        torch.cuda.empty_cache()
    with open(json_path, "w") as f:
        json.dump(results, f, indent=4)
    _format_benchmark(json_path)
    return results
