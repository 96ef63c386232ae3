"""Phi-3-Vision / Phi-3-mini-128K on MI355X: the model object behind
`generate()/choose()/constrain()`.

Drop-in for the reference's `Phi3VForCausalLM` / `Phi3ForCausalLM`
(reference phi.py:565-617): same call signature and return contract

    model(input_ids, pixel_values=None, image_sizes=None, positions=None, cache=None,
          pids=None, mask=None, max_tokens=0, advance_offset=None, n_beam=1) -> (logits, cache)

but every tensor op is a hand-written gfx950 kernel from ``csrc/`` (see ops.py).
This module only owns device buffers and sequences launches.

HBM layout
  weights      bf16 [out, in] row-major (HF layout, K contiguous = MFMA fragment order)
  KV cache     per layer K bf16 [B, n_kv, Tp, hd] and V TRANSPOSED bf16 [B, n_kv, hd, Tp]
               (Tp = prompt + max_tokens rounded up to 64, allocated once): both are then
               k-contiguous MFMA operands for QK^T and PV with plain 16-byte loads
  RoPE tables  fp32 cos/sin [B, T, hd/2] built once per prompt (one short/long choice, Q2)
  residual     decoder: bf16 [B*L, H]; ViT: fp32 [crops, 577, 1024]
Dtype flow differs from the reference only where stated in DESIGN.md
(bf16 K cache / bf16 MFMA operands instead of fp32 attention), within the
tolerance the parity tests state.
"""
import math
import copy
import dataclasses
import os

import numpy as np
import torch

from . import ops, steps
from .parallel import families_without, family_pays, family_table
from .config import head_dim, is_vision, rope_scaling_factor
from .weights import Q4Weight, mlx_quantize, q4_repack
from .ops import (BF16, EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_QGELU, EPI_BIAS_RESID_F32, EPI_NONE, EPI_PATCH,
                  EPI_RESID_BF16, EPI_SILU_MUL, F32, I32)

import functools
import weakref


def _on_device(fn):
    """Run a model entry point with the model's GPU as the current device: ops.py launches on
    `torch.cuda.current_stream()` of the CURRENT device, and a thread other than the one that loaded the model (the
    server's engine thread) starts on device 0."""
    @functools.wraps(fn)
    def wrapped(self, *a, **kw):
        with torch.cuda.device(self.device):
            return fn(self, *a, **kw)
    return wrapped


_ATTR = {flag: attr for flag, attr, _ in steps.NEEDS}      # an option's flag -> the CacheState attribute of its table
_OFF = {"logprobs": -1}         # the word that makes a row of an option's table inactive, by flag (steps.FLAGS); the others: 0


def _shared_table(name, doc):
    return property(lambda self: self.shared.get(name), doc=doc)


def _records(table):
    """The per-row records of an option's table (CacheState): the table itself, or the `rows` of a penalty or guide state."""
    return table["rows"] if isinstance(table, dict) else table


def _last_rows(logits, row0):
    """(the last position's rows of prefill logits [n, L, V] or [n, V], the slice of state rows row0 .. row0+n-1 they belong to)"""
    last = logits[:, -1, :] if logits.dim() == 3 else logits
    return last, slice(row0, row0 + last.shape[0])


V_PREFIX = "model.vision_embed_tokens.img_processor.vision_model."
E_PREFIX = "model.vision_embed_tokens."


@dataclasses.dataclass(slots=True)
class AttnPlan:
    """The decode attention's plan of one pass over a state (Phi3VModel._plan makes it; nothing writes it afterwards): `bufs["plan"]` of
    an eager pass, `g["bufs"]["plan"]` of a capture."""
    n_split: int = 0            # key splits per (row, head); 0: a prompt-sized pass (no split plan, no workspace)
    ws: object = None           # the split partials' workspace, all-ones between launches (ops.attention_ws)
    attn_merge: bool = False    # the partials are merged inside the attention launch (`merge_in_launch`), not by a launch of their own
    fuse_o: bool = False        # the layer's o_proj + residual ride in the attention launch, or in the merge launch without attn_merge
    family: bool = False        # ops.attention_decode_family: the state's families read their prompt K/V once
    past_lb: int = -1           # captured step: the host's lower bound of the device-side cache length (-1: none)
    rope_cos: object = None     # captured step: the step's staged rotation rows [B, L, hd / 2]
    rope_sin: object = None
    o_f: object = None          # fuse_o: the attention output's two buffers, used by alternate layers, all-ones = "not written yet"
    o_f2: object = None


def _attn_knobs():
    """The environment's say in a plan, read once per plan (at plan time: tests set them per test) -> (128-key tiles allowed, forced
    n_split or None, P3V_ATTN_FUSED_MERGE's mode: "0" never / "1" by rule / "2" wherever the kernels can, fused o_proj allowed,
    profiling).  P3V_PROFILING=1: no launch of the step may wait for another workgroup of its own grid (whole-graph rocprofv3 --pmc
    passes serialise / mask what they profile) -- separate merge launch, separate o_proj launch."""
    env = os.environ.get
    forced = env("P3V_ATTN_NSPLIT")
    return (env("P3V_ATTN_TILE128", "1") != "0", int(forced) if forced else None, env("P3V_ATTN_FUSED_MERGE", "1"),
            env("P3V_ATTN_FUSE_OPROJ", "1") != "0", env("P3V_PROFILING") == "1")


class CacheState:
    """All layers' KV cache + per-prompt RoPE tables / pad lengths.

    Mirrors reference KVCache (phi.py:509-548) semantics: `offset` auto-advances
    by L, can be rewound (`advance_offset`), `max_tokens < 1` disables caching,
    `n_beam > 1` reads the cache without writing it."""

    def __init__(self, cfg, B, S, max_tokens, device):
        self.B, self.S, self.max_tokens = B, S, max_tokens
        self.T = S + max(max_tokens, 0)
        self.quantized = bool(getattr(cfg, "use_quantized_cache", False))
        # cache_format="mlx4" (opt-in): the reference's OWN quantised cache -- MLX 4-bit group-32 codes of the PROMPT's K / V, later
        # tokens unquantised (phi.py:528-540).  The codes are kept in the reference's format (k4 / v4 + scale | bias), and the
        # bf16 cache rows hold their dequantised values, which is what every later call of the reference attends on: the decode
        # path is then the plain bf16 one.  (Default for quantize_cache=True: int8 for all tokens, BASELINE config 5.)
        self.mlx4 = self.quantized and getattr(cfg, "cache_format", "int8") == "mlx4"
        if self.quantized and getattr(cfg, "cache_format", "int8") not in ("int8", "mlx4"):
            raise ValueError(f"cache_format must be 'int8' or 'mlx4', got {cfg.cache_format!r}")
        if self.mlx4:
            self.quantized = False
        # row/column stride of the caches: whole 128-key tiles (the decode attention takes one 128-key tile per workgroup
        # when the capacity allows it)
        gran = 128
        self.Tp = (self.T + gran - 1) // gran * gran
        if (self.Tp // gran) % 2 == 0:
            # V^T rows are Tp * 2 bytes apart: at multiples of 512 B the 96 rows of a tile crowd the same memory channels
            # (measured decode step at B = 1: +3.5 % at Tp = 2560, +2 % at 3584, +1.4 % at 4096, +5.7 % at 33024 = 258 tiles
            # against the neighbouring lengths) -- an ODD number of 128-key tiles keeps the stride off that grid
            self.Tp += gran
        nl, nkv, hd = cfg.num_hidden_layers, cfg.num_key_value_heads, head_dim(cfg)
        if self.quantized:
            # int8 KV (quantize_cache=True): offset-binary bytes + one fp32 scale per (layer, row, head, token);
            # one bf16 K / V^T scratch layer holds the exact prompt keys while a layer's prefill attends (phi.py:531-533)
            self.k8 = torch.full((nl, B, nkv, self.Tp, hd), 128, dtype=torch.uint8, device=device)
            self.v8 = torch.full((nl, B, nkv, hd, self.Tp), 128, dtype=torch.uint8, device=device)
            self.ks = torch.ones((nl, B, nkv, self.Tp), dtype=F32, device=device)
            self.vs = torch.ones((nl, B, nkv, self.Tp), dtype=F32, device=device)
            self.k_tmp = torch.empty((B, nkv, self.Tp, hd), dtype=BF16, device=device)
            self.v_tmp = torch.zeros((B, nkv, hd, self.Tp), dtype=BF16, device=device)
        else:
            self.k = torch.empty((nl, B, nkv, self.Tp, hd), dtype=BF16, device=device)    # K   [.., t, hd]
            self.v = torch.zeros((nl, B, nkv, hd, self.Tp), dtype=BF16, device=device)    # V^T [.., hd, t] (zero: tail keys stay finite)
        if self.mlx4:
            g = hd // 32
            self.k4 = torch.zeros((nl, B, nkv, max(S, 1), g, 4), dtype=I32, device=device)
            self.v4 = torch.zeros_like(self.k4)
            self.k_sb = torch.zeros((nl, B, nkv, max(S, 1), g, 2), dtype=F32, device=device)
            self.v_sb = torch.zeros_like(self.k_sb)
            self.mlx4_tokens = 0                                # prompt tokens held as codes (set by the first call)
        self.offset = 0
        self.cos = self.sin = self.pad_len = None
        self.graphs = {}
        self.epoch = None                                       # model.epoch the graphs were captured under
        self.shared = {"dirty": False}                          # shared by the per-request views of a captured-prefill entry (copy.copy)
        self.slots = False                                      # a slot state of the continuous-batching engine (model.new_slot_state)
        self.serving = False                                    # owned by a long-lived server (engine.py): see _plan
        self.fresh_rows = False                                 # a rows_view whose columns left of its offset hold nothing its rows may see
        self.row_adapter = None                                 # adapter bank: int32 [B] slot per row, made on first use (model._state_rows)
        # shared-prefix decode (model.set_families): the device table int32 [B, 18] of ops.attention_decode_family, made on first
        # use -- from then on the state's L = 1 steps take that launch, whatever the table holds --, the host's copy of it and the
        # families it was built from [(rows, share_end)]
        self.family = self.family_host = None
        self.families = []

    # The tables of the per-row options (steps.NEEDS names them, model._option_table makes them), each None until made.  They live
    # with `shared`: the leases of a captured-prefill entry share their captures, which bake the tables' addresses in -- a later
    # lease must write the SAME tensors, not some of its own.
    sample_rows = _shared_table("sample_rows", """The sampling records, int32 [B, 6] on the device, or None before
        `model.set_sampling` made them.""")
    logprob_want = _shared_table("logprob_want", """The log-probability want-table, int32 [B] on the device (-1 = off), or None
        before `model.set_logprobs` made it.""")
    penalty = _shared_table("penalty", """The penalty state (model.set_penalties): a dict of the rows' records (int32 [B, 4]),
        their `seen` table (int32 [B, n]: the uint32 words of the rule), the adjusted-logits buffer (bf16 [B, n]) and, once a
        request brought one, the bias table (fp32 [B, n]) -- or None before the first penalised request.""")
    guide = _shared_table("guide", """The guide state (model.set_guides): a dict of the rows' records (int32 [B, 4]) and their
        table regions (`delta` int16 [B, 256, 256]: the uint16 entries; `accept` uint8 [B, 256]) -- or None before the first
        guided request.""")

    def rows_view(self, rows, offset, S):
        """Batch rows `rows` (a slice) as a cache of their own at `offset`, for a prompt of S tokens (model.prefill_slot): the same
        buffers sliced, no captured graphs, none of the slot state's roles (slots, serving; the caller names the rows' adapters;
        the option tables are the whole state's, and nothing reads them on a view).  fresh_rows: columns left of `offset` hold
        nothing these rows may see (pad_len >= offset)."""
        view = copy.copy(self)
        view.B = rows.stop - rows.start
        view.S = S
        view.offset = offset
        view.graphs = {}
        view.fresh_rows = True
        view.slots = False
        view.serving = False
        view.row_adapter = None
        view.family = view.family_host = None                   # (the table is the whole state's: a view's rows are single rows)
        view.families = []
        view.mlx4 = False                                       # (the view carries k / v alone, never the 4-bit prompt codes)
        view.cos = self.cos[rows]
        view.sin = self.sin[rows]
        view.pad_len = self.pad_len[rows]
        if self.quantized:
            view.k8 = self.k8[:, rows]
            view.v8 = self.v8[:, rows]
            view.ks = self.ks[:, rows]
            view.vs = self.vs[:, rows]
            view.k_tmp = self.k_tmp[rows]
            view.v_tmp = self.v_tmp[rows]
        else:
            view.k = self.k[:, rows]
            view.v = self.v[:, rows]
        return view

    def mark_dirty(self):
        """An unrecovered failed step may have left NaN rows beyond the offset and half-armed buffers in the decode graph: a
        captured-prefill entry built on these buffers must not be reused (model._prefill_captured drops it)."""
        self.shared["dirty"] = True

    def scrub(self, lo, hi):
        """Forget cache positions [lo, hi) that a FAILED step wrote (api.greedy_loop's recovery): a poisoned step leaves NaN there,
        and the decode attention multiplies every V^T column of a tile -- live or not -- by its (zero) probability."""
        hi = min(hi, self.Tp)
        if hi <= lo:
            return
        if self.quantized:
            self.v8[..., lo:hi] = 128
            self.k8[:, :, :, lo:hi] = 128
            self.vs[..., lo:hi] = 1.0
            self.ks[..., lo:hi] = 1.0
        else:
            self.v[..., lo:hi] = 0
            self.k[:, :, :, lo:hi] = 0


class LayerCache:
    """`cache[i]` view with the reference's `.offset` attribute."""

    def __init__(self, state, i):
        self.state, self.i = state, i

    @property
    def offset(self):
        return self.state.offset

    @offset.setter
    def offset(self, v):
        self.state.offset = int(v)


@steps.methods(_on_device)                                      # the eight public step methods: steps.py's table
class Phi3VModel:
    def __init__(self, cfg, weights, device="cuda:0"):
        if not torch.cuda.is_available():
            raise RuntimeError("Phi3VModel needs a GPU: the hot path is HIP-only (no CPU fallback)")
        ops.L.lib()                                  # fail loudly if libp3v.so is missing
        self.cfg, self.device = cfg, torch.device(device)
        self.vision = is_vision(cfg)
        self.w = {k: v.to(self.device, BF16).contiguous() for k, v in weights.items() if not isinstance(v, Q4Weight)}
        # 4-bit group-64 projections (MLX nn.quantize checkpoints / quantized_int4): device layout of p3v_gemv_q4
        self.w4 = {k: tuple(t.to(self.device) for t in q4_repack(*v)) for k, v in weights.items() if isinstance(v, Q4Weight)}
        self.hd = head_dim(cfg)
        if self.hd != 96:
            raise ValueError(f"decoder head_dim must be 96 (got {self.hd})")
        self.hidden_hook = None                      # fn(layer, x [B*L, H], B, L) after every decoder layer (diagnostics)
        self.w8 = {}
        self._rope_tables = {}                                   # (B, T, factors, ..) -> (cos, sin): shared read-only (see _new_state)
        self._vit_graphs, self._vit_seen = {}, {}                # captured vision tower per crop count (clip_forward)
        self.adapters = {}                           # weight key -> (lora_a, lora_b, scale), see set_adapters
        self._lora_tmp = {}                          # decode-sized (M <= 16) adapter scratch: captured graphs point at it
        self._lora_flat = None                       # ONE grow-only scratch for prefill-sized calls (not graph-captured)
        self.adapter_names = []                      # bank slot -> name (set_adapter_bank); a row names its slot in st.row_adapter
        self._bank = {}                              # weight key -> (bank table int64 [n_slots, 3], r_max), union of the adapters' targets
        self._bank_keep = []                         # the uploaded lora_a / lora_b tensors the tables point at
        self._rows_cur = None                        # row table of the _layers call in flight (int32 [M] on the device)
        # A long-lived owner that may share the GPU with other streams / processes (server.py) sets this: the decode step then
        # uses no launch that needs all of its workgroups resident at once (the fused attention + o_proj launch, the in-launch
        # split-KV merge on grids larger than the machine) -- ADVICE r04.  One-shot generate() on an exclusive GPU keeps them.
        self.serving = os.environ.get("P3V_SHARED_GPU", "0") == "1"
        self.epoch = 0                               # bumped whenever captured decode graphs become stale
        self._prefill_graphs = {}                    # (S, max_tokens) -> captured short-prompt prefill (see _prefill_captured)
        self._prefill_seen = {}
        self._states = weakref.WeakSet()             # every live CacheState (their graphs bake pointers into this model)
        # quantize_model=True (fp8): prompt-sized projections run W8A8 on the fp8 MFMA unless fp8_activations=False
        # (then: dequantise to a bf16 scratch + bf16 MFMA, weight-only accuracy at bf16 prefill speed)
        self.fp8_act = bool(getattr(cfg, "fp8_activations", True)) and os.environ.get("P3V_FP8_PREFILL", "mfma") != "dequant"
        if getattr(cfg, "quantized_fp8", False):     # e4m3 bytes + per-row scale: 7.4 GB -> 3.7 GB streamed per token
            self._quantize_decoder(self.w8, ops.quantize_fp8_rows)
        if getattr(cfg, "quantized_int4", False):    # 4-bit group-64 (the reference's nn.quantize(model, 64, 4)) by the MLX algorithm, on the device: -> 2.1 GB
            self._quantize_decoder(self.w4, lambda v: tuple(t.to(self.device) for t in q4_repack(*mlx_quantize(v))))
        if self.w8 or self.w4:                       # one dequantised matrix (prefill GEMM scratch): the largest there is
            n_max = max(math.prod(ops.weight_shape(v)) for v in (*self.w8.values(), *self.w4.values()))
            self._deq = torch.empty(n_max, dtype=BF16, device=self.device)
        self.w13 = {}                                # weight key -> ops.PackedB13: what the one-row decode projections stream
        if os.environ.get("P3V_PACK13", "1") != "0":
            self._pack_decoder_b13()
        if self.vision:
            self._prep_vision()

    # ------------------------------------------------------------------ fp8 / 4-bit weights (quantize_model=True, quantized_int4)
    def _quantize_decoder(self, dst, quantise):
        """Decoder projections + lm_head leave `w` for `dst` (w8 or w4) as `quantise` makes them; the rest stays bf16 (prefill-only / tiny).
        A key lives in exactly ONE of w, w8 and w4: `_handle` and the fused o_proj's format rule (`_fused_oproj_kw`) rely on it."""
        for k in [k for k in self.w if k == "lm_head.weight" or (k.startswith("model.layers.") and k.endswith("_proj.weight"))]:
            dst[k] = quantise(self.w.pop(k))

    # ------------------------------------------------------------------ 13-bit packed bf16 weights (B = 1 decode)
    @_on_device
    def _pack_decoder_b13(self):
        """A second, exact copy of every bf16 qkv / gate_up / down projection and of lm_head as 13-bit codes:
        the one-row decode projections stream it instead -- 13/16 of the bytes, the same bits out.  `self.w` keeps the bf16 matrices
        (prefill, batched decode, adapters and the fused attention + o_proj launch read them).  A matrix that does not fit the format
        (ops.pack_b13 answers None) or whose K is not 3072 / 8192 is simply not in the dict and stays on bf16."""
        for k, v in self.w.items():
            if k != "lm_head.weight" and not (k.startswith("model.layers.") and k.endswith(("qkv_proj.weight", "gate_up_proj.weight", "down_proj.weight"))):
                continue
            if v.dim() != 2 or v.shape[1] not in (3072, 8192) or v.shape[0] % 2:
                continue
            pk = ops.pack_b13(v, silu_pairs=k.endswith("gate_up_proj.weight"))
            if pk is not None:
                self.w13[k] = pk

    def _packed(self, key):
        """The packed copy of self.w[key], or None: there is none, or the bf16 matrix was replaced or written to since it was made
        (the copy is then dropped: that matrix runs on bf16 from here on).  This is looked at where a launch is ISSUED -- eager calls and
        graph captures; a step that is already captured keeps replaying the copy it was captured with, so whoever changes decoder
        weights of a live model calls `repack_b13`."""
        pk = self.w13.get(key)
        if pk is not None and not pk.current(self.w.get(key)):
            del self.w13[key]
            self.epoch += 1
            return None
        return pk

    def repack_b13(self):
        """After decoder weights were replaced or written to: drop every packed copy and every captured step that may stream one, and
        pack again from `self.w` as it stands (nothing if P3V_PACK13=0)."""
        self.w13.clear()
        self.epoch += 1
        for st in list(self._states):
            st.graphs.clear()
        if os.environ.get("P3V_PACK13", "1") != "0":
            self._pack_decoder_b13()

    # ------------------------------------------------------------------ LoRA adapters (use_adapter=True)
    def set_adapters(self, adapters):
        """Attach LoRA adapters: {"model.layers.<i>.<target>.weight": (lora_a [in,r] f32, lora_b [r,out] f32, scale)}
        (weights.resolve_adapter).  An adapted projection runs unfused: materialised RMSNorm -> frozen projection with a
        plain epilogue -> p3v_lora_down / p3v_lora_up, which carries the residual / SiLU*up epilogue (phi.py:129-133)."""
        if adapters and self._bank:
            raise ValueError("this model carries an adapter bank (set_adapter_bank): detach it before set_adapters -- one or the other")
        self._set_adapters(adapters)

    @_on_device
    def _set_adapters(self, adapters):
        for k, (a, b, _) in adapters.items():
            shape = ops.weight_shape(self._weight(k))
            if tuple(a.shape[:1]) != (shape[1],) or tuple(b.shape[1:]) != (shape[0],):
                raise ValueError(f"LoRA shapes {tuple(a.shape)} x {tuple(b.shape)} do not fit {k} {tuple(shape)}")
        self.adapters = {k: (a.to(self.device, F32).contiguous(), b.to(self.device, F32).contiguous(), float(s))
                         for k, (a, b, s) in adapters.items()}
        self.epoch += 1                              # captured decode graphs bake the kernel sequence and the scratch
        for st in list(self._states):                # pointers in: drop them on EVERY live cache before the scratch goes
            st.graphs.clear()
        self._lora_tmp, self._lora_flat = {}, None
        self._prefill_graphs.clear()

    def _handle(self, key, rows=0):
        """(weight handle, its format as ops.py names it) a launch of `rows` rows streams for `key`, or (None, None): for one row the packed
        copy while `_packed` still returns it, else the entry of `w`, `w8` or `w4` (the dict names the format).  Every eager projection pays for this call."""
        if rows == 1 and (pk := self.w13.get(key)) is not None and (pk.current(self.w.get(key)) or self._packed(key)):
            return pk, "b13"                         # (a stale copy: `_packed` drops it, bumps `epoch` and answers None)
        if self.w8 and (w := self.w8.get(key)) is not None:      # (a quantised model holds every decoder matrix in w8 or w4,
            return w, "fp8"                                       #  a bf16 model leaves both empty: one lookup either way)
        if self.w4 and (w := self.w4.get(key)) is not None:
            return w, "q4"
        return (w, "bf16") if (w := self.w.get(key)) is not None else (None, None)

    def _weight(self, key, rows=0):
        return self._handle(key, rows)[0]            # the handle alone

    def _fold_weight(self, key, B):
        """The handle a decode step of B rows streams where `key`'s projection carries the step's head or tail (ops.gemv_step_begin /
        gemv_step_end), or None where it runs through `_proj`: an adapter or the bank on it, or P3V_STEP_FOLD=0.  (The bank never holds
        lm_head -- set_adapter_bank refuses it -- so one test serves both ends; `_proj_frozen` then drops a stale packed copy, same step.)"""
        if key in self.adapters or key in self._bank or os.environ.get("P3V_STEP_FOLD", "1") == "0":
            return None
        return self._weight(key, B)

    def _fused_oproj_kw(self, o_key, x, rearm):
        """The o_proj keywords of a fused attention + o_proj launch.  The weight format names the launch: bf16 and 4-bit weights go
        with the bf16 cache (ops.attention_decode), e4m3 weights with the int8 cache (ops.attention_decode_q8; `_plan`)."""
        w, fmt = self._handle(o_key)
        kw = dict(o_proj_x=x, o_rearm=rearm)
        if fmt == "fp8":
            return dict(kw, o_proj_w8=w[0], o_proj_scale=w[1])
        return dict(kw, o_proj_w=w[0], o_proj_sb=w[1]) if fmt == "q4" else dict(kw, o_proj_w=w)

    # ------------------------------------------------------------------ adapter bank: N resident adapters, one per row
    def set_adapter_bank(self, bank):
        """Attach N LoRA adapters beside the one set of frozen weights: {name: weights.resolve_adapter(...) result}.  Bank slot i is
        the i-th name (`adapter_names`); every batch row names its slot in the state's row table (`set_row_adapters`, -1 = the base
        model), which the kernels read from device memory: rows with different adapters -- or none -- share one captured decode
        step, and a row changes adapter without a recapture.  Every projection in the UNION of the adapters' targets runs
        frozen projection (own fused norm, plain epilogue) -> p3v_lora_down_rows -> p3v_lora_up_rows (include/p3v.h); the others
        run untouched.  A/B are uploaded once, `epoch` is bumped once.  An empty dict removes the bank.  A bank and a
        `set_adapters` adapter on one model is a ValueError."""
        bank = dict(bank or {})
        if not bank and not self._bank:
            return                                   # nothing attached, nothing to remove: the captured steps stay valid
        if bank and self.adapters:
            raise ValueError("this model carries a set_adapters adapter: detach it (set_adapters({})) before set_adapter_bank -- one or the other")
        for name, ad in bank.items():
            if not isinstance(name, str) or not name:
                raise ValueError(f"adapter names are non-empty strings, got {name!r}")
            for k, (a, b, _) in ad.items():
                if not (k.startswith("model.layers.") and k.endswith("_proj.weight")) or self._weight(k) is None:
                    raise ValueError(f"adapter {name!r}: {k} is not a decoder projection of this model")
                shape = ops.weight_shape(self._weight(k))
                if a.dim() != 2 or b.dim() != 2 or a.shape[0] != shape[1] or b.shape[1] != shape[0] or a.shape[1] != b.shape[0]:
                    raise ValueError(f"adapter {name!r}: LoRA shapes {tuple(a.shape)} x {tuple(b.shape)} do not fit {k} {tuple(shape)}")
                if not 1 <= a.shape[1] <= ops.L.LORA_MAX_RANK:
                    raise ValueError(f"adapter {name!r}: rank {a.shape[1]} of {k} is outside 1..{ops.L.LORA_MAX_RANK}")
        self._attach_bank(bank)

    @_on_device
    def _attach_bank(self, bank):
        names = list(bank)
        dev = {n: {k: (a.to(self.device, F32).contiguous(), b.to(self.device, F32).contiguous(), float(s)) for k, (a, b, s) in ad.items()}
               for n, ad in bank.items()}
        union = sorted({k for ad in dev.values() for k in ad})
        self._bank = {k: (ops.lora_table([dev[n].get(k) for n in names], self.device), max(dev[n][k][0].shape[1] for n in names if k in dev[n]))
                      for k in union}
        self._bank_keep, self.adapter_names = dev, names
        self.epoch += 1                              # as set_adapters: the captured steps bake the kernel sequence and the scratch
        for st in list(self._states):
            st.graphs.clear()
        self._lora_tmp, self._lora_flat = {}, None
        self._prefill_graphs.clear()

    def _bank_has(self, suffix):
        return any(k.endswith(suffix) for k in self._bank)

    def _state_rows(self, st):
        """The state's row table (int32 [B] on the device, -1 = no adapter), made on first use."""
        if st.row_adapter is None:
            st.row_adapter = torch.full((st.B,), -1, dtype=I32, device=self.device)
        return st.row_adapter

    @_on_device
    def set_row_adapters(self, st, adapters, row0=0):
        """Name the adapter of rows row0 .. row0+n-1 of a state: bank slots, adapter names, or None / -1 for the base model.  One small
        H2D copy outside any graph, like `set_sampling`: the captured steps read the table, so the next replay serves the new
        assignment.  Rows never written are -1."""
        if isinstance(adapters, (str, int)) or adapters is None:
            adapters = [adapters]
        slots = []
        for a in adapters:
            if a is None:
                slots.append(-1)
            elif isinstance(a, str):
                if a not in self.adapter_names:
                    raise ValueError(f"unknown adapter {a!r}; known: {self.adapter_names}")
                slots.append(self.adapter_names.index(a))
            else:
                a = int(a)
                if not -1 <= a < len(self.adapter_names):
                    raise ValueError(f"adapter slot {a} is outside -1..{len(self.adapter_names) - 1}")
                slots.append(a)
        if row0 < 0 or row0 + len(slots) > st.B:
            raise ValueError(f"rows {row0}..{row0 + len(slots) - 1} are outside the state's {st.B} rows")
        self._state_rows(st)[row0:row0 + len(slots)].copy_(torch.tensor(slots, dtype=I32))
        return st

    def _lora_scratch(self, M, specs):
        """The adapter scratch tensors of one projection call on M rows, one per (tag, shape, dtype) of `specs`."""
        if M <= ops.GEMV_MAX_M:                                 # decode-sized: persistent buffers (graph replays read them)
            for tag, shape, dtype in specs:
                if (tag,) + shape not in self._lora_tmp:
                    self._lora_tmp[(tag,) + shape] = torch.empty(shape, dtype=dtype, device=self.device)
            return [self._lora_tmp[(tag,) + shape] for tag, shape, _ in specs]
        # prefill-sized: carved out of one grow-only allocation at 256-byte offsets, not one set per prompt length (a server
        # would leak VRAM)
        sizes = [math.prod(shape) * dtype.itemsize for _, shape, dtype in specs]
        offs = [0]
        for nb in sizes:
            offs.append((offs[-1] + nb + 255) // 256 * 256)
        if self._lora_flat is None or self._lora_flat.numel() < offs[-1]:
            self._lora_flat = torch.empty(offs[-1], dtype=torch.uint8, device=self.device)
        return [self._lora_flat[o:o + nb].view(dtype).view(shape) for o, nb, (_, shape, dtype) in zip(offs, sizes, specs)]

    def _proj_bank(self, x, key, table, r_max, epilogue, resid, norm_w, out, h):
        M, K = x.shape
        N, S = ops.weight_shape(self._weight(key))[0], ops.lora_slices(K)
        y, t = self._lora_scratch(M, [("y", (M, N), BF16), ("t", (M, S, r_max), F32)])
        rows = self._rows_cur
        if rows is None or rows.numel() != M:
            raise RuntimeError(f"{key}: no row table for {M} rows (an adapter bank serves the decoder stack only)")
        # the frozen projection keeps its own fused norm; the down kernel norms the rows it streams itself (bit-identical)
        self._proj_frozen(x, key, EPI_NONE, None, norm_w, y, h)
        ops.lora_down_rows(x, table, rows, r_max, norm_w=norm_w, norm_eps=self.cfg.rms_norm_eps, out=t)
        return ops.lora_up_rows(y, t, table, rows, K, r_max, epilogue, resid=resid, out=out)

    def _proj(self, x, key, epilogue=EPI_NONE, resid=None, norm_w=None, out=None, h=None):
        """One projection of the decoder (+ its LoRA adapter, if one is attached)."""
        ad = self.adapters.get(key)
        if ad is None:
            bk = self._bank.get(key) if self._bank else None
            if bk is not None:
                return self._proj_bank(x, key, bk[0], bk[1], epilogue, resid, norm_w, out, h)
            return self._proj_frozen(x, key, epilogue, resid, norm_w, out, h)
        a, b, scale = ad
        M, K, N, r = x.shape[0], x.shape[1], b.shape[1], a.shape[1]
        hbuf, y, t = self._lora_scratch(M, [("h", (M, K), BF16), ("y", (M, N), BF16), ("t", (M, r), F32)])
        if norm_w is not None:                                  # the adapter needs the normalised input itself
            x = ops.rmsnorm(x, norm_w, self.cfg.rms_norm_eps, out=hbuf)
        self._proj_frozen(x, key, EPI_NONE, None, None, y, None)
        ops.lora_down(x, a, out=t)
        return ops.lora_up(y, t, b, scale, epilogue, resid=resid, out=out)

    def _proj_frozen(self, x, key, epilogue=EPI_NONE, resid=None, norm_w=None, out=None, h=None):
        """Weight-streaming kernel for skinny x, MFMA GEMM otherwise; bf16 or fp8 weights."""
        eps = self.cfg.rms_norm_eps
        M, K = x.shape
        w, fmt = self._handle(key, M)
        if fmt == "b13":
            if w.silu_pairs == (epilogue == EPI_SILU_MUL):
                return ops.gemv_b13(x, w, epilogue, resid=resid, norm_w=norm_w, norm_eps=eps, out=out)
            w, fmt = self.w[key], "bf16"                          # (an adapted gate_up runs with a plain epilogue: bf16)
        skinny = M <= 8 or (M <= ops.GEMV_MAX_M and K % 512 == 0)
        if fmt == "q4":
            if M == 1 and K in (3072, 8192):
                return ops.gemv_q4(x, w[0], w[1], epilogue, resid=resid, norm_w=norm_w, norm_eps=eps, out=out)
            if (2 <= M <= 16 and K in (3072, 8192) and os.environ.get("P3V_Q4_ROWS", "1") != "0"
                    and (w[0].shape[0] // (2 if epilogue == EPI_SILU_MUL else 1)) % 16 == 0):
                # 2 .. 16 rows straight on the 4-bit weights (round 6: k_gemv8_q4 / k_gemm_rows_q4; the reference runs QuantizedLinear at
                # every batch size, phi_3_vision_mlx.py:296) instead of dequantising the whole matrix into the bf16 scratch per call
                if norm_w is not None and (M > 8 or os.environ.get("P3V_Q4_ROWS8_NORM", "1") == "0"):
                    x, norm_w = ops.rmsnorm(x, norm_w, eps, out=h), None       # 9 .. 16 rows: one p3v_rmsnorm launch in front
                return ops.gemv_q4(x, w[0], w[1], epilogue, resid=resid, norm_w=norm_w, norm_eps=eps, out=out)
            w = ops.dequant_q4(w[0], w[1], out=self._deq[:w[0].numel() * 8].view(w[0].shape[0], w[0].shape[1] * 8))
        elif fmt == "fp8":
            if skinny and K in (3072, 8192):
                return ops.gemv_fp8(x, w[0], w[1], epilogue, resid=resid, norm_w=norm_w, norm_eps=eps, out=out)
            if not skinny and self.fp8_act and ops.gemm_fp8_ok(M, w[0].shape[0], K, epilogue):
                # prompt-sized input: W8A8 on the fp8 matrix cores, activations quantised per token row (fused with the norm)
                a8, sa = ops.quant_fp8_rows(x, norm_w, eps)
                return ops.gemm_fp8(a8, sa, w[0], w[1], epilogue, resid=resid, out=out)
            w = ops.dequant_fp8(w[0], w[1], out=self._deq[:w[0].numel()].view(w[0].shape))
        elif skinny and M > 8 and K % 64 == 0 and w.shape[0] % 64 == 0:
            # 9 .. 16 rows on bf16 weights: the 64-row tiles of the weight-streaming GEMM (p3v_gemm_skinny.hip) beat the 16-row MFMA
            # GEMV by a quarter of the step (B = 16 at 512 keys: 3.9 -> 3.1 ms); up to 8 rows k_gemv_mfma8 stays ahead
            skinny = False
        if skinny:
            return ops.gemv(x, w, epilogue, resid=resid, norm_w=norm_w, norm_eps=eps, out=out)
        if norm_w is not None:
            x = ops.rmsnorm(x, norm_w, eps, out=h)
        return ops.gemm(x, w, epilogue, resid=resid, out=out)

    def _proj_resid_norm(self, o, key, x, norm_w, h):
        """x += bf16(o @ W^T) and h = RMSNorm(x) * norm_w from the projection's own launches (ops.gemm_resid_norm); False -- nothing
        done -- where that does not apply (adapters, quantised weights, shapes the library does not run as K slices)."""
        M = o.shape[0]
        if (key in self.adapters or key in self._bank or key not in self.w or M <= 8 or h.shape[0] < M
                or os.environ.get("P3V_RESID_NORM_FUSE", "1") == "0"):
            return False
        return ops.gemm_resid_norm(o, self.w[key], x, norm_w, self.cfg.rms_norm_eps, h[:M], out=x)

    # ------------------------------------------------------------------ vision tower
    def _prep_vision(self):
        c = self.cfg.clip
        D, P = c["hidden_size"], c["patch_size"]
        if D // c["num_attention_heads"] != 64:
            raise ValueError("CLIP head_dim must be 64")
        kk = 3 * P * P
        self.kpad = (kk + 63) // 64 * 64
        wp = torch.zeros((D, self.kpad), dtype=BF16, device=self.device)
        wp[:, :kk] = self.w[V_PREFIX + "embeddings.patch_embedding.weight"].reshape(D, kk)
        self.w_patch = wp
        self.clip_qkv = []
        for j in range(c["num_hidden_layers"] - 1):          # the last layer never runs (phi.py:219)
            q = V_PREFIX + f"encoder.layers.{j}.self_attn."
            wq = torch.cat([self.w[q + f"{n}_proj.weight"] for n in "qkv"], dim=0).contiguous()
            bq = torch.cat([self.w[q + f"{n}_proj.bias"] for n in "qkv"], dim=0).contiguous()
            self.clip_qkv.append((wq, bq))

    VIT_GRAPH_ENTRIES = 2

    def _clip_bufs(self, n):
        """Every intermediate of the tower for n crops (one allocation set per call on the eager path; owned by the graph entry otherwise)."""
        c, dev = self.cfg.clip, self.device
        D, P, I_ = c["hidden_size"], c["patch_size"], c["intermediate_size"]
        G = c["image_size"] // P
        T, nh = G * G + 1, c["num_attention_heads"]
        Tp = (T + 63) // 64 * 64
        return dict(
            patches=torch.empty((n * G * G, self.kpad), dtype=BF16, device=dev), x=torch.empty((n, T, D), dtype=F32, device=dev),
            q=torch.empty((n, nh, T, 64), dtype=BF16, device=dev), k=torch.empty((n, nh, Tp, 64), dtype=BF16, device=dev),
            v=torch.zeros((n, nh, 64, Tp), dtype=BF16, device=dev),              # V^T, zero tail
            o=torch.empty((n * T, D), dtype=BF16, device=dev), h=torch.empty((n * T, D), dtype=BF16, device=dev),
            qkv=torch.empty((n * T, 3 * D), dtype=BF16, device=dev), f=torch.empty((n * T, I_), dtype=BF16, device=dev))

    @_on_device
    def clip_forward(self, pix):
        """ClipModel.__call__ (phi.py:216-221) on live crops; pix f32 [n,3,336,336] -> f32 [n,577,D]
        (row 0 = CLS, which the caller skips).
        Round 6: the tower's ~280 launches cost the host as long to enqueue (25 - 30 us each in Python + ctypes) as the GPU to run, so a
        crop count seen for the SECOND time is captured as one hipGraph over buffers the entry owns (as the short-prompt prefill,
        _prefill_captured) and later images of that geometry cost one copy + one graph launch; the returned features are the
        entry's buffer -- the caller consumes them on the same stream before the next image can overwrite them.  Same kernels in
        the same order: bit-identical.  P3V_VIT_GRAPH=0 keeps eager launches."""
        n = pix.shape[0]
        w = self.w
        key = (n, w[V_PREFIX + "embeddings.position_embedding.weight"].data_ptr(), w[V_PREFIX + "encoder.layers.0.mlp.fc1.weight"].data_ptr())
        if os.environ.get("P3V_VIT_GRAPH", "1") == "0" or self.hidden_hook is not None:
            return self._clip_body(pix, self._clip_bufs(n))
        e = self._vit_graphs.get(key)
        if e is None:
            if self._vit_seen.get(key, 0) < 1:                    # first sight of this crop count: eager, remember it
                if len(self._vit_seen) > 64:
                    self._vit_seen.clear()
                self._vit_seen[key] = 1
                return self._clip_body(pix, self._clip_bufs(n))
            e = self._build_vit_graph(pix)
            if len(self._vit_graphs) >= self.VIT_GRAPH_ENTRIES:
                self._vit_graphs.pop(next(iter(self._vit_graphs)))
            self._vit_graphs[key] = e
        e["pix"].copy_(pix, non_blocking=True)
        e["graph"].launch()
        return e["bufs"]["x"]

    def _capture(self, run, ws):
        """`run()` -- a launch sequence over buffers its caller owns -- as one ops.Graph: the capture protocol of every captured
        path of the model (vision tower, short-prompt prefill, greedy / sampled / verify decode step).  A warm-up run first (sets
        func attributes, pages code in, sizes the split-K GEMM workspace in `ws`, a dict the caller keeps alive as long as the
        graph), then the capture on a side stream with that workspace frozen: nothing may be allocated under capture, and the
        pointer is baked into the graph (ops.owned_gemm_workspace).  `run` executes twice: loop state the warm-up must not
        advance is the builder's to reset or restore."""
        with ops.owned_gemm_workspace(ws, frozen=False):
            run()
        torch.cuda.synchronize()
        graph = ops.Graph()
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), ops.owned_gemm_workspace(ws, frozen=True):
            graph.begin()
            run()
            graph.end()
        torch.cuda.current_stream().wait_stream(side)
        return graph

    def _build_vit_graph(self, pix):
        e = dict(pix=torch.empty_like(pix), bufs=self._clip_bufs(pix.shape[0]), ws={})
        e["pix"].copy_(pix)
        e["graph"] = self._capture(lambda: self._clip_body(e["pix"], e["bufs"]), e["ws"])
        return e

    def _clip_body(self, pix, B_):
        c, w = self.cfg.clip, self.w
        n, D, P = pix.shape[0], c["hidden_size"], c["patch_size"]
        G = c["image_size"] // P
        T, nh, eps = G * G + 1, c["num_attention_heads"], c["layer_norm_eps"]
        e = V_PREFIX + "embeddings."
        patches = ops.im2col_patches(pix, P, self.kpad, out=B_["patches"])
        x = B_["x"]
        pos = w[e + "position_embedding.weight"]
        ops.gemm(patches, self.w_patch, EPI_PATCH, out=x, n_out=D, pos=pos, patches_per_img=G * G, ldo=D)
        ops.clip_cls_rows(x, w[e + "class_embedding"], pos)
        x2 = x.view(n * T, D)
        ops.layernorm(x2, w[V_PREFIX + "pre_layrnorm.weight"], w[V_PREFIX + "pre_layrnorm.bias"], 1e-5, out_f32=True, out=x2)
        Tp = (T + 63) // 64 * 64
        q, k, v, o, h, qkv, f = (B_[t] for t in ("q", "k", "v", "o", "h", "qkv", "f"))
        for j in range(c["num_hidden_layers"] - 1):
            lp = V_PREFIX + f"encoder.layers.{j}."
            ops.layernorm(x2, w[lp + "layer_norm1.weight"], w[lp + "layer_norm1.bias"], eps, out=h)
            wq, bq = self.clip_qkv[j]
            # head split; the queries leave it multiplied by scale * log2(e) like the decoder's (the attention's softmax is then the
            # bare exp2: k_attn_prefill_dma<64, PRE> 59 -> 49 us per layer at 17 crops, tools/clip_attn_probe.py).  Round 6: the split
            # rides in the projection's epilogue here too (ops.gemm_qkv: Q, K rows and V^T columns straight from the accumulators) --
            # a crop is 577 tokens, so the 8-token V^T runs start one token later in every crop; the epilogue now stores them at
            # whatever offset they fall on (one dwordx4 at even offsets, three stores at odd ones, element-wise across a crop end).
            pre = os.environ.get("P3V_VIT_PLAIN_Q") != "1"
            qs = 64 ** -0.5 * ops.Q_PRESCALE if pre else 1.0
            if not (os.environ.get("P3V_QKV_FUSE", "1") != "0"
                    and ops.gemm_qkv(h, wq, None, None, q, k, v, n, T, nh, nh, 64, 0, Tp, False, q_scale=qs, bias=bq)):
                ops.gemm(h, wq, EPI_BIAS, bias=bq, out=qkv)
                ops.rope_kv_append(qkv, None, None, q, k, v, n, T, nh, nh, 64, 0, Tp, False, q_scale=qs)
            ops.attention(q, o, n, T, nh, nh, 64, 64 ** -0.5, False, k_past=k, v_past=v, past_t=Tp, new_is_cache=True, q_prescaled=pre)
            ops.gemm(o, w[lp + "self_attn.out_proj.weight"], EPI_BIAS_RESID_F32, bias=w[lp + "self_attn.out_proj.bias"],
                     resid=x2, out=x2)
            ops.layernorm(x2, w[lp + "layer_norm2.weight"], w[lp + "layer_norm2.bias"], eps, out=h)
            ops.gemm(h, w[lp + "mlp.fc1.weight"], EPI_BIAS_QGELU, bias=w[lp + "mlp.fc1.bias"], out=f)
            ops.gemm(f, w[lp + "mlp.fc2.weight"], EPI_BIAS_RESID_F32, bias=w[lp + "mlp.fc2.bias"], resid=x2, out=x2)
        return x

    def vision_embed(self, x, pixel_values, image_sizes, positions, L):
        """Phi3ImageEmbedding.__call__ (phi.py:393-416): ViT on the live crops
        (dead zero-padded crop slots are skipped, Q5), HD merge, projector, and
        the projector's second GEMM writes straight into the text embeddings."""
        w = self.w
        if torch.is_tensor(pixel_values):                                  # processor(return_mx=True): already f32 on the GPU
            pv = pixel_values.to(F32)
        else:
            pv = torch.as_tensor(np.asarray(pixel_values), dtype=F32)      # f64 -> f32 as mx.array does
        sizes = (np.asarray(image_sizes) // 336).tolist()
        positions = np.asarray(positions).tolist()
        live = [h * ww + 1 for h, ww in sizes]
        if len(live) == 1 and pv.is_contiguous():                          # one image: its live crops are a view, nothing to gather
            pix = pv[0, :live[0]].to(self.device)
        else:
            pix = torch.cat([pv[i, :n] for i, n in enumerate(live)], dim=0).contiguous().to(self.device)
        feats = self.clip_forward(pix)
        C_ = self.cfg.img_processor["image_dim_out"]
        G = self.cfg.clip["image_size"] // self.cfg.clip["patch_size"]
        H = self.cfg.hidden_size
        idx, crop0 = 0, 0
        for i, (h, ww) in enumerate(sizes):
            merged = ops.hd_merge(feats[crop0:crop0 + live[i]], w[E_PREFIX + "sub_GN"], w[E_PREFIX + "glb_GN"], h, ww, G, C_)
            t = ops.gemm(merged, w[E_PREFIX + "img_projection.0.weight"], EPI_BIAS_GELU, bias=w[E_PREFIX + "img_projection.0.bias"])
            r, c0 = positions[idx]
            cnt = merged.shape[0]
            dst = x[r * L + c0: r * L + c0 + cnt]
            ops.gemm(t, w[E_PREFIX + "img_projection.2.weight"], EPI_BIAS, bias=w[E_PREFIX + "img_projection.2.bias"], out=dst)
            idx += cnt
            crop0 += live[i]
        return x

    # ------------------------------------------------------------------ per-prompt state
    ROPE_TABLE_ENTRIES = 8

    def _rope_factors(self, n_tokens):
        """The su-scaled RoPE factors for a context of n_tokens: ONE short / long choice per prompt (phi.py:492), long beyond the
        original context length."""
        cfg = self.cfg
        return cfg.rope_scaling["long_factor" if n_tokens > cfg.original_max_position_embeddings else "short_factor"]

    def _inv_freq(self, n_tokens):
        """Inverse frequencies (f32 [hd / 2] on the host) of the su-scaled RoPE for a context of n_tokens."""
        return 1.0 / (torch.tensor(self._rope_factors(n_tokens), dtype=F32)
                      * (torch.tensor(float(self.cfg.rope_theta), dtype=F32) ** (torch.arange(0, self.hd, 2, dtype=F32) / self.hd)))

    def _new_state(self, B, S, max_tokens, pids, mask, shared_tables=True, extra_tokens=0):
        cfg = self.cfg
        # extra_tokens: columns beyond prompt + max_tokens (a speculative verify step writes K/V rows up to offset + K); the
        # short / long RoPE-factor choice below stays on prompt + max_tokens, as the plain path takes it
        st = CacheState(cfg, B, S, max_tokens + int(extra_tokens) if max_tokens > 0 else max_tokens, self.device)
        self._states.add(st)
        half = self.hd // 2
        L_all = S + max_tokens                                  # reference sizes tables with max_tokens as given
        su = self._rope_factors(L_all)
        if mask is not None:
            st.pad_len = torch.as_tensor((np.asarray(mask) == 0).sum(axis=1).astype(np.int32)).to(self.device)
        # Prompts without explicit position ids (every unpadded request) of one geometry rotate by the same table: it is built once
        # and shared read-only between their states (a server's requests repeat a few geometries; building it costs three small host ->
        # device copies and a launch in front of every prefill).  Slot states write per-row tables: they get their own.
        tkey = (B, st.T, tuple(float(v) for v in su), float(cfg.rope_theta), rope_scaling_factor(cfg), self.hd) if pids is None and shared_tables else None
        if tkey is not None and tkey in self._rope_tables:
            st.cos, st.sin = self._rope_tables[tkey]
            return st
        inv_freq = self._inv_freq(L_all)
        T = st.T
        if pids is None:
            pos = torch.arange(T, dtype=F32)[None].expand(B, T)
        else:
            p = torch.as_tensor(np.asarray(pids)).to(F32)
            ext = p[:, -1:] + 1 + torch.arange(T - p.shape[1], dtype=F32)[None]
            pos = torch.cat([p, ext], dim=1)
        pos = pos.contiguous().to(self.device)
        cos, sin = ops.rope_table(pos.view(-1), inv_freq.to(self.device), rope_scaling_factor(cfg))
        st.cos, st.sin = cos.view(B, T, half), sin.view(B, T, half)
        if tkey is not None:
            if len(self._rope_tables) >= self.ROPE_TABLE_ENTRIES:
                self._rope_tables.pop(next(iter(self._rope_tables)))
            self._rope_tables[tkey] = (st.cos, st.sin)
        return st

    # ------------------------------------------------------------------ slot state of the continuous-batching engine
    @_on_device
    def new_slot_state(self, slots, window):
        """A cache of `slots` batch rows and `window` columns that is not tied to one prompt batch (engine.py): every row
        has its OWN left padding and position table, so a request can be prefilled into a free row while the other rows
        are mid-generation.  All rows start empty (pad_len = window: every key masked).  The window fixes the RoPE regime
        of every row (phi.py:492: one choice per call from prompt + max_tokens): window <= 4096 -> short factors, beyond
        -> long factors; the engine admits only requests that would pick the same factors alone.  With
        `quantize_cache=True` the rows keep the int8 KV cache (BASELINE config 5)."""
        st = self._new_state(slots, 0, window, None, None, shared_tables=False)
        st.pad_len = torch.full((slots,), window, dtype=I32, device=self.device)
        st.slots = True
        return st

    @_on_device
    def prefill_slot(self, st, row, inputs, return_logits=False, prefix=None):
        """Prefill one request (a B = 1 `processor(...)` result) -- or n requests as one batch (`collate_requests` of them:
        equal lengths, or shorter rows left-padded inside the group) -- into the batch rows row .. row+n-1 of a slot state so
        that every row's LAST prompt token sits in column st.offset - 1: row i gets left padding pad_i = st.offset - S_i and
        position ids 0..S_i-1 from column pad_i on.  Keys left of pad_i (stale rows of an earlier occupant, the group's own
        padding) are masked by pad_len.  Returns the first greedy tokens (int32 [n, 1] on the device; with return_logits also
        the last-position logits).  Each row computes what a B = 1 run of its request computes (pad invariance).
        prefix=(entry, P) (prefix.PrefixCache.lookup; one request only): the row keeps the same geometry, the entry's first P
        tokens are copied to columns [pad, pad + P) (ops.kv_copy) and the model runs on the LAST S - P ids alone, as a cached call
        at offset pad + P.  Images whose slots the prefix covers are not computed: no vision tower when it covers them all."""
        cfg = self.cfg
        ids = np.asarray(inputs["input_ids"])
        ids = ids[None] if ids.ndim == 1 else ids
        n, S = ids.shape
        if prefix is not None and (n != 1 or "mask" in inputs):
            raise ValueError("prefill_slot: a prefix is restored for ONE unpadded request")
        lens = np.full(n, S, dtype=np.int64)
        if "mask" in inputs:
            m = np.asarray(inputs["mask"]).reshape(n, S)
            lens = m.sum(1).astype(np.int64)
            if not all(int(m[i, S - lens[i]:].sum()) == lens[i] for i in range(n)) or lens.min() < 1:
                raise ValueError("prefill_slot takes LEFT-padded rows")
        win = st.offset - S                                      # first column the group's batch writes
        if win < 0:
            raise ValueError(f"prompt of {S} tokens does not fit left of column {st.offset}")
        pads = torch.as_tensor(st.offset - lens, dtype=torch.int32)
        half = self.hd // 2
        inv_freq = self._inv_freq(st.T)                          # (a slot state's T is its window: new_slot_state)
        rows = slice(row, row + n)
        uniq = np.unique(lens)
        for L_ in uniq:                                          # one table per distinct length
            pos = (torch.arange(st.T, dtype=F32) - float(st.offset - L_)).clamp_min(0).to(self.device)
            cos, sin = ops.rope_table(pos, inv_freq.to(self.device), rope_scaling_factor(cfg))
            for i in np.nonzero(lens == L_)[0]:
                st.cos[row + i].copy_(cos.view(st.T, half)), st.sin[row + i].copy_(sin.view(st.T, half))
        st.pad_len[rows].copy_(pads.to(self.device))
        view = st.rows_view(rows, win, S)                        # these rows as an n-row cache at offset `win`
        view.epoch = self.epoch
        if self._bank:
            view.row_adapter = self._state_rows(st)[rows]        # (the rows' adapters: set_row_adapters BEFORE this prefill)
        kw = {k: v for k, v in inputs.items() if k in ("pixel_values", "image_sizes", "positions")}
        if prefix is not None:
            P, kw = self._prefix_split(ids, prefix, kw)
            self._restore_prefix(st, row, win, prefix[0], P)
            view.fresh_rows = False                              # columns [win, win + P) hold keys these rows DO see
            view.offset, ids = win + P, ids[:, P:]
        logits, _ = self(input_ids=ids, cache=[LayerCache(view, i) for i in range(cfg.num_hidden_layers)], full_logits=False, **kw)
        assert view.offset == st.offset
        tok = ops.argmax(logits[:, -1, :].contiguous())[:, None]
        return (tok, logits) if return_logits else tok

    # ------------------------------------------------------------------ prompt prefix cache (prefix.py)
    def _state_kv(self, st):
        if st.mlx4:
            raise ValueError('cache_format="mlx4" states are never captured or restored')
        return (st.k8, st.v8, st.ks, st.vs) if st.quantized else (st.k, st.v)

    def _prefix_split(self, ids, prefix, kw):
        """(P, vision inputs of the suffix) for a prompt `ids` [1, S] whose first P tokens come from `prefix` = (entry, P): only
        the images whose slots lie in the suffix are kept, their slot positions re-based by -P."""
        from .prefix import slot_runs
        entry, P = prefix
        P, S = int(P), ids.shape[1]
        runs = slot_runs(ids[0])
        if not 1 <= P <= min(S - 1, entry.P) or any(a < P < b for a, b, _ in runs):
            raise ValueError(f"prefix of {P} tokens does not fit a prompt of {S} (entry: {entry.P}; never inside an image's slots)")
        if not np.array_equal(ids[0, :P], entry.ids[:P]):
            raise ValueError("prefix entry does not hold these token ids")
        covered = [i for a, b, i in runs if b <= P]
        if covered != list(range(len(covered))) or [i for _, _, i in runs] != list(range(len(runs))):
            raise ValueError("prefix reuse needs the images in tag order")
        if kw.get("pixel_values") is None or not runs:
            return P, kw
        k = len(covered)
        if k == len(runs):
            return P, {}                                         # every image is cached: no vision tower at all
        pos = np.asarray(kw["positions"])
        pos = pos[pos[:, 1] >= P].copy()
        pos[:, 1] -= P
        return P, {"pixel_values": kw["pixel_values"][k:], "image_sizes": np.asarray(kw["image_sizes"])[k:], "positions": pos}

    def _restore_prefix(self, st, row, col, entry, P):
        kind = "int8" if st.quantized else "bf16"
        if entry.key[3] != kind or len(entry.kv) != (4 if st.quantized else 2):
            raise ValueError(f"prefix entry holds a {entry.key[3]} cache, the state a {kind} one")
        ops.kv_copy([(tuple(t.unsqueeze(1) for t in entry.kv), 0, 0, self._state_kv(st), row, col, P)])

    @_on_device
    def capture_prefix(self, st, row, pad, P):
        """K/V of tokens [0, P) of the request in batch row `row` (its first token in column `pad`) as compact tensors for the
        prefix store: (k [nl, nkv, P8, hd], vt [nl, nkv, hd, P8]) bf16, or int8 codes + two fp32 scale rows.  One launch."""
        from .prefix import alloc_kv
        cfg = self.cfg
        src = self._state_kv(st)
        if P < 1 or pad < 0 or pad + P > st.Tp:
            raise ValueError(f"capture_prefix: columns [{pad}, {pad + P}) are outside the state")
        kv = alloc_kv(P, cfg.num_hidden_layers, cfg.num_key_value_heads, self.hd, "int8" if st.quantized else "bf16", self.device)
        ops.kv_copy([(src, row, pad, tuple(t.unsqueeze(1) for t in kv), 0, 0, P)])
        return kv

    # ------------------------------------------------------------------ n completions per prompt (include/p3v.h: p3v_kv_fork_t)
    @_on_device
    def fork_rows(self, st, src_row, dst_rows, pad=None, share=False):
        """Make rows `dst_rows` of a slot state exact continuations of row `src_row` at st.offset: its K/V columns
        [pad, st.offset) (ops.kv_fork: one launch, every piece of the source read once), its cos / sin table rows and its
        pad_len (`pad`: the source row's pad_len where the caller knows it on the host; None reads it back).  K is stored rotated by logical position, so the columns are valid in any row.  NOT copied -- their setters
        take a row range and the caller sets them: sampling records, the penalty record / `seen` row / bias, the
        log-probability want-table entry, the row's adapter.  A state with guides: the destination rows get the source row's
        guide region and its record at the START state (an inactive source row makes inactive copies).
        share: also register the source and destination rows as a family that shares columns [pad, st.offset)
        (`set_families`; the rows leave whatever family they were in).  The copies are made all the same."""
        if st.mlx4:
            raise ValueError('cache_format="mlx4" states are never forked: n > 1 completions need the bf16 or the int8 cache')
        dst_rows = [int(r) for r in dst_rows]
        src_row = int(src_row)
        if not dst_rows:
            return
        if not 0 <= src_row < st.B or any(not 0 <= r < st.B for r in dst_rows) or src_row in dst_rows or len(set(dst_rows)) != len(dst_rows):
            raise ValueError(f"fork_rows: {dst_rows} must be distinct rows of the state's {st.B}, none of them the source row {src_row}")
        if st.pad_len is None:
            raise ValueError("fork_rows: a slot state (per-row pad_len and position tables)")
        kv = self._state_kv(st)
        pad = int(st.pad_len[src_row].item()) if pad is None else int(pad)
        if not 0 <= pad <= st.Tp:
            raise ValueError(f"fork_rows: pad {pad} is outside the state's {st.Tp} columns")
        idx = torch.tensor(dst_rows, dtype=torch.int64, device=self.device)
        for i in range(0, len(dst_rows), ops.L.KV_FORK_MAX_DST):
            ops.kv_fork(kv, src_row, pad, kv, dst_rows[i:i + ops.L.KV_FORK_MAX_DST], pad, max(st.offset - pad, 0))
        st.cos.index_copy_(0, idx, st.cos[src_row:src_row + 1].expand(len(dst_rows), -1, -1))
        st.sin.index_copy_(0, idx, st.sin[src_row:src_row + 1].expand(len(dst_rows), -1, -1))
        st.pad_len.index_fill_(0, idx, pad)
        gd = st.guide
        if gd is not None:                                      # the leader's guide region, at its start state
            k = len(dst_rows)
            gd["delta"].index_copy_(0, idx, gd["delta"][src_row:src_row + 1].expand(k, -1, -1))
            gd["accept"].index_copy_(0, idx, gd["accept"][src_row:src_row + 1].expand(k, -1))
            rec = gd["rows"][src_row:src_row + 1].clone()
            rec[:, 2] = 1
            gd["rows"].index_copy_(0, idx, rec.expand(k, -1))
        if share:
            rows = (src_row, *dst_rows)
            self.set_families(st, families_without(st.families, rows) + [(rows, st.offset)])

    @_on_device
    def fork_state(self, st1, n, share=False):
        """The B = 1 state of a finished prefill as a NEW B = n state of the same geometry whose n rows all continue that
        prompt (api._generate(n=...)): another allocation, K/V columns [0, offset) through ONE ops.kv_fork launch with n
        destination rows, position tables and pad_len replicated, offset and epoch carried over, captures not.  Returns the
        new state's cache list; the B = 1 state is left as it was (the caller drops it: n + 1 copies of the prompt are held
        only between this call's two ends).  share: the n rows are registered as one family sharing columns [0, offset)
        (`set_families`): decode steps of the new state read the prompt's K/V once -- where that pays (parallel.family_pays);
        a smaller family gets the plain state."""
        n = int(n)
        if st1.B != 1 or not 1 <= n <= ops.L.KV_FORK_MAX_DST + 1:
            raise ValueError(f"fork_state: a B = 1 state into 1..{ops.L.KV_FORK_MAX_DST + 1} rows, got B = {st1.B}, n = {n}")
        if st1.mlx4:
            raise ValueError('cache_format="mlx4" states are never forked: n > 1 completions need the bf16 or the int8 cache')
        st = CacheState(self.cfg, n, st1.S, st1.T - st1.S, self.device)
        assert (st.T, st.Tp) == (st1.T, st1.Tp)
        self._states.add(st)
        src, dst = self._state_kv(st1), self._state_kv(st)
        rows = list(range(n))
        ops.kv_fork(src, 0, 0, dst, rows[:ops.L.KV_FORK_MAX_DST], 0, st1.offset)
        if n > ops.L.KV_FORK_MAX_DST:                            # the 16th row: a second launch
            ops.kv_fork(src, 0, 0, dst, rows[ops.L.KV_FORK_MAX_DST:], 0, st1.offset)
        st.cos, st.sin = st1.cos.expand(n, -1, -1).contiguous(), st1.sin.expand(n, -1, -1).contiguous()
        st.pad_len = None if st1.pad_len is None else st1.pad_len.expand(n).contiguous()
        st.offset, st.epoch, st.serving = st1.offset, st1.epoch, st1.serving
        if share and family_pays(n, st.offset):                 # (below the break-even the state has no table: the plain plan)
            self.set_families(st, [(tuple(rows), st.offset)])
        return [LayerCache(st, i) for i in range(self.cfg.num_hidden_layers)]

    # ------------------------------------------------------------------ shared-prefix decode (include/p3v.h: p3v_attention_decode_family)
    def family_refusal(self, st=None):
        """Why this model / state cannot share a prefix between rows, or None: the family launch reads the bf16 cache."""
        quantized = bool(getattr(self.cfg, "use_quantized_cache", False)) if st is None else (st.quantized or st.mlx4)
        if quantized:
            fmt = getattr(self.cfg, "cache_format", "int8") if st is None else ("mlx4" if st.mlx4 else "int8")
            return f"share_prefix needs the bf16 KV cache: the shared-prefix attention has no {fmt} form (quantize_cache=True)"
        return None

    @_on_device
    def set_families(self, st, families, create=False):
        """Name the rows of `st` whose caches are identical up to a column: families = [(rows, share_end), ...], the leader -- the
        row whose copy is read -- first; [] clears the table.  Decode steps (L = 1, no beams) of a state that has a table go
        through ops.attention_decode_family, which reads columns [0, floor(share_end / chunk) * chunk) of a family once, from its
        leader; those columns of the other members are then dead positions (finite, otherwise ignored).  The table is made on
        first use and lives on the device: this call is one host-to-device copy, and a step captured AFTER the table was made
        follows it without a new capture.  A state that already holds a captured step and no table is refused (ValueError: its
        capture would keep the plain launch beside eager steps on the family launch); a long-lived state makes the table first,
        with create=True and no families.  Nothing here drops a capture.
        Families below the measured break-even (parallel.family_pays: few rows x few shared keys) stay single rows, and make no
        table where there is none; `st.families` lists the registered ones.  The caller keeps the contract: no row is rewritten
        below share_end while it is in a family."""
        families = [(tuple(int(r) for r in rows), int(se)) for rows, se in families]
        if st.family is None and not families and not create:
            return
        why = self.family_refusal(st)
        if why:
            raise ValueError(why)
        family_table(st.B, families)                            # (every family is checked, also those left out below)
        if any(se > st.offset for rows, se in families if len(rows) > 1):
            raise ValueError(f"set_families: share_end beyond the cache length {st.offset}")
        families = [f for f in families if len(f[0]) > 1 and family_pays(len(f[0]), f[1])]   # below the break-even: single rows
        if st.family is None and not families and not create:
            return
        tab = torch.from_numpy(family_table(st.B, families))
        if st.family is None:
            if st.graphs:                                       # a step captured without a table keeps the plain launch: two plans on one state
                raise ValueError("set_families: the state already holds a captured step; make the table before the first capture "
                                 "(set_families(st, [], create=True))")
            st.family = torch.empty((st.B, ops.L.FAMILY_INTS), dtype=I32, device=self.device)
        st.family.copy_(tab)
        st.family_host = tab
        st.families = families

    @_on_device
    def decode_graph(self, st):
        """The captured greedy step of a state (built on first use): its `tok` / `next_tok` / `d_past` device buffers."""
        return self._greedy_capture(st)

    def _sync_epoch(self, st):
        """Drop the state's captures if the adapters changed since they were made: they bake stale pointers in."""
        if st.epoch != self.epoch:
            st.graphs.clear()
            st.epoch = self.epoch

    def _greedy_capture(self, st):
        """The state's greedy capture (`st.graphs["greedy"]`, see _build_decode_graph) of the current epoch: built on first use,
        and rebuilt if the cache was rewound below the lower bound it was captured with."""
        self._sync_epoch(st)
        g = st.graphs.get("greedy")
        if g is None or st.offset < g["bufs"]["plan"].past_lb:
            g = st.graphs["greedy"] = self._build_decode_graph(st)
            g["host_tok"] = None
        return g

    # ------------------------------------------------------------------ decoder stack
    FAMILY_CHUNK = 256          # keys per split of the family plan (tools/share_step_time.py sets it on its model to time the alternatives)

    def _plan(self, st, B, L, fuse_o, captured=False, family=True):
        """The buffers of a pass over B x L rows of a state and, as `bufs["plan"]`, its attention plan (AttnPlan), chosen top to
        bottom: family or split plan, n_split, workspace, merge form, o_proj form.  fuse_o: the caller can take the layer's o_proj +
        residual inside the attention's launches.  captured: the plan is for a captured step, which reads the cache length from the
        device -- it carries the step's staging rows for the rotation tables and `past_lb`, the host's lower bound of that length: the
        cache only grows under a captured step (the capture is rebuilt if it is ever found below the bound); a slot state's column
        moves both ways (engine.py), so it gets none.
        The split plan comes from the cache CAPACITY, eager or captured: same kernel, same split boundaries -> eager and replayed
        steps agree bit for bit.  Which kernel the library runs for (n_split, capacity), and which o_proj form it takes, is its
        route's to say (ops.attention_decode_route; tests/test_attn_probe_cpu.py ties the two)."""
        cfg, T = self.cfg, st.Tp
        nh, hd = cfg.num_attention_heads, self.hd
        bufs = self._alloc_bufs(B, L)
        plan = bufs["plan"]
        if family and L == 1 and st.family is not None and B == st.B and not st.quantized and not st.mlx4:
            # A state with a family table (ops.attention_decode_family, no fused o_proj).  A family's whole splits below share_end are
            # read once, by its leader, and the up-to-one-chunk remainder by every member, so the chunk is small and fixed: 256 keys
            # (four tiles of the one-wave kernel per split), as many splits as the workspace and the merge launch take (128; longer
            # caches get longer chunks: 320 keys at 32k).  Always the separate merge launch.  Timed at 2,531 keys, shared step,
            # n = 4 / n = 8 (profiles/share_prefix_step_time.txt): 64 keys 2.4306 / 2.8538 ms, 128 keys 2.2363 / 2.4925 ms, 256 keys
            # 2.1288 / 2.4102 ms -- fewer, longer single-wave workgroups and half the partials to merge outweigh the longer remainder.
            plan.family, fuse_o = True, False
            plan.n_split = max(1, min(128, -(-T // int(self.FAMILY_CHUNK))))
            plan.ws = ops.attention_ws(B, 1, nh, hd, plan.n_split, self.device)
        elif L <= ops.L.DECODE_MAX_L:
            # Split-KV plan of the decode-shaped attention: enough blocks to fill 256 CUs.  64-key tiles; up to ~4096 workgroups ONE
            # tile per 4-wave workgroup (the kernel then lasts a single tile's dependency chain); beyond that ~768 single-wave
            # workgroups (one resident round, each with its next 24 KB tile in flight) walking several tiles
            tile128_ok, forced_split, merge_mode, fuse_o_ok, profiling = _attn_knobs()   # (the family plan has none)
            tiles = -(-T // 64)
            tiles128 = T // 128 if T % 128 == 0 else 0
            if tiles128 and tiles > 16 and tiles128 <= 48 and B * nh * tiles128 <= 2048 and tile128_ok:
                # one 128-key tile per workgroup: every workgroup of the launch resident at once (3 per CU), half the
                # partials to merge (k_attn_decode128).  Short caches keep 64-key tiles (more workgroups than CUs matters more)
                n_split = tiles128
            elif tiles <= 128 and B * nh * tiles <= 4096:
                n_split = tiles
            else:
                # (int8 KV: a tile is half the bytes and the single-wave kernel's 27.5 KB of LDS lets 5 workgroups share a CU,
                #  so ~1280 workgroups keep as many bytes in flight: 3.68 -> 3.40 ms/step at 32k)
                n_split = max(1, min(128, tiles, -(-(1280 if st.quantized else 768) // max(1, B * nh))))
            plan.n_split = n_split = n_split if forced_split is None else forced_split
            plan.ws = ops.attention_ws(B, L, nh, hd, n_split, self.device)
            # in-launch split-KV merge (`merge_in_launch`): with the one-tile-per-workgroup plans, and with the
            # multi-tile streaming kernel when a head has at most 4 splits (B = 8: 3 splits -- the merge launch costs 4.9 us a
            # layer, the in-launch merge 0.5; with 24 splits at B = 1 / 32k the one merging workgroup per head is the slower
            # way: +1.6 % per step, +4.5 % at 8k)
            merge = (n_split in (tiles, tiles128) or n_split <= 4 or merge_mode == "2") and n_split <= 48 and merge_mode != "0"
            # The merging workgroup of a (row, head) waits -- bounded, NaN-poisoned on expiry -- for partials of workgroups that
            # the hardware dispatches before it (linear order; observed, not documented).  When the whole grid is resident at once
            # (128-key tiles: 3 workgroups per CU, 64-key: 5) nothing depends on that order.  A plan for a long-lived server (a slot
            # state of the continuous-batching engine, a server-owned model) takes the separate merge launch wherever the grid is
            # larger (B = 8: +4.9 us per layer); one-shot generate() keeps the faster in-launch form, whose failure mode is loud
            # (api._rows raises).  P3V_ATTN_FUSED_MERGE=2 forces it everywhere.
            if (st.serving or self.serving) and merge and merge_mode != "2":
                per_cu = 3 if n_split == tiles128 else 5
                merge = B * nh * n_split <= per_cu * ops.device_props(torch.device(self.device).index or 0)["cu_count"]
            plan.attn_merge = bool(merge and not profiling)
        if captured:
            plan.past_lb = -1 if st.slots else int(st.offset)
            plan.rope_cos = torch.empty((B, L, hd // 2), dtype=F32, device=self.device)
            plan.rope_sin = torch.empty_like(plan.rope_cos)
        # B = L = 1: attention + o_proj + residual as ONE launch per layer where the library takes the shape -- on bf16 or MLX 4-bit
        # weights and a bf16 cache (k_attn_decode128_o / _o4), or on e4m3 weights and the int8 cache (config 5:
        # k_attn_decode128_q8<true>); without the in-launch merge (long contexts, round 6) the MERGE launch carries the o_proj
        # (k_attn_combine_o).  The launch of layer i re-arms the OTHER output buffer, so the two alternate cleanly only over an EVEN
        # number of layers (an odd stack would hand layer 0 of the next step the buffer the last layer just filled: stale words read
        # as "written").  It also needs the GPU to itself (every workgroup resident at once): not for a server-owned model.
        o_key = "model.layers.0.self_attn.o_proj.weight"
        if (fuse_o and B == 1 and L == 1 and fuse_o_ok and not profiling and cfg.num_hidden_layers % 2 == 0 and not self.serving   # (L = 1: the knobs were read)
                and not self.adapters and not self._bank_has("self_attn.o_proj.weight") and (self._handle(o_key)[1] == "fp8") == bool(st.quantized)):
            can = ops.attention_decode_q8_can_fuse_oproj if st.quantized else ops.attention_decode_can_fuse_oproj
            # The merge forms to offer the library, the plan's own first.  Short contexts on the bf16 cache (64-key one-tile plans: the
            # in-launch o_proj is for 128-key tiles): attention that only writes its partials + the merge launch carrying the o_proj
            # beats attention with the in-launch merge + an o_proj launch (1.587 -> 1.570 ms per step at 128 keys, 1.662 -> 1.652 at
            # 1000; with the int8 cache it loses: 1.165 -> 1.179 at 128 keys, so not there)
            for merge in (plan.attn_merge, False) if plan.attn_merge and not st.quantized else (plan.attn_merge,):
                if can(B, L, nh, hd, plan.n_split, T, cfg.hidden_size, merge):
                    plan.attn_merge, plan.fuse_o = merge, True
                    plan.o_f, plan.o_f2 = (torch.full((1, nh * hd), -1, dtype=torch.int16, device=self.device).view(BF16) for _ in range(2))
                    break
        return bufs

    def _alloc_bufs(self, B, L):
        cfg = self.cfg
        nh, nkv, hd, H, I = cfg.num_attention_heads, cfg.num_key_value_heads, self.hd, cfg.hidden_size, cfg.intermediate_size
        M, dev = B * L, self.device
        return dict(
            q=torch.empty((B, nh, L, hd), dtype=BF16, device=dev), o=torch.empty((M, nh * hd), dtype=BF16, device=dev),
            qkv=torch.empty((M, (nh + 2 * nkv) * hd), dtype=BF16, device=dev), a=torch.empty((M, I), dtype=BF16, device=dev),
            h=torch.empty((M, H), dtype=BF16, device=dev), plan=AttnPlan())

    def _layers(self, x, st, B, L, past, n_beam, bufs=None, d_past=None, last_only=False, step_begin=None):
        """Phi3DecoderLayer stack (phi.py:473-485).  `d_past` (device int32) makes every
        position-dependent kernel read the cache length from HBM -> graph-replayable.
        last_only: the caller reads the LAST position only (prefill of generate / choose, Q8): the final layer still builds
        K / V for every position, but its o_proj and MLP run on the B last rows alone (0.4 ms of a 30 ms prefill);
        returns [B, H] then."""
        cfg, w = self.cfg, self.w
        nh, nkv, hd, eps = cfg.num_attention_heads, cfg.num_key_value_heads, self.hd, cfg.rms_norm_eps
        M = B * L
        skinny = M <= 8 or (M <= ops.GEMV_MAX_M and cfg.hidden_size % 512 == 0)   # weight-streaming projections
        scale = hd ** -0.5
        decode = L <= ops.L.DECODE_MAX_L                        # decode-shaped rows: one fused attention launch (+ merge) per layer
        if bufs is None:
            bufs = self._plan(st, B, L, fuse_o=decode and n_beam == 1, family=n_beam == 1)
        q, o, qkv, a, h, plan = (bufs[k] for k in ("q", "o", "qkv", "a", "h", "plan"))
        n_split, ws, fuse_o, attn_merge = plan.n_split, plan.ws, plan.fuse_o, plan.attn_merge
        if decode and d_past is not None:                       # graph replay: rotation rows staged once per step by the caller
            rc, rs, rb = plan.rope_cos, plan.rope_sin, L
        elif decode:                                            # eager: views into the prompt tables at `past`
            rc, rs, rb = st.cos[:, past:], st.sin[:, past:], st.T
        if self._bank:                                          # adapter bank: one table entry per row of x (token rows share their request's)
            ra = self._state_rows(st)                           # (a captured step reads the state's own table: L = 1, no copy)
            self._rows_cur = ra if M == st.B else ra.repeat_interleave(M // st.B)
        mlx4 = st.mlx4
        if (st.quantized or mlx4) and n_beam > 1:
            raise NotImplementedError("Beam Search is not yet compatible with Quantized Cache")       # as phi.py:525
        mlx4_first = mlx4 and past == 0 and st.mlx4_tokens == 0 and L <= st.k4.shape[3]             # the call that fills the cache (phi.py:531-533)
        if n_beam > 1:                                          # beams: K/V of this call go to a scratch, cache is read-only
            Lp = (L + 7) // 8 * 8
            k_new = torch.empty((B, nkv, Lp, hd), dtype=BF16, device=self.device)
            v_new = torch.zeros((B, nkv, hd, Lp), dtype=BF16, device=self.device)
        normed_in = False                                       # `h` already holds the layer's normalised input
        for i in range(cfg.num_hidden_layers):
            p = f"model.layers.{i}."
            # Prompt-sized calls on bf16 weights: the qkv projection writes rotated Q, the K cache rows and the V^T cache columns from
            # its own epilogue (ops.gemm_qkv: bit-identical to the projection + rope_kv_append, one launch sequence instead of two).
            fused_qkv = False
            k_w = p + "self_attn.qkv_proj.weight"
            if (not decode and n_beam == 1 and k_w in w and k_w not in self.adapters and k_w not in self._bank and not mlx4_first
                    and (M >= 1024 or M <= 256) and os.environ.get("P3V_QKV_FUSE", "1") != "0"):
                kd, vd = (st.k_tmp, st.v_tmp) if st.quantized else (st.k[i], st.v[i])
                if not (st.quantized and past > 0 and not st.fresh_rows):
                    hn = h if normed_in else ops.rmsnorm(x, w[p + "input_layernorm.weight"], eps, out=h)
                    normed_in = True                            # (`h` holds the normalised input now, whatever the fused call answers)
                    fused_qkv = ops.gemm_qkv(hn, w[k_w], st.cos, st.sin, q, kd, vd, B, L, nh, nkv, hd, past, st.Tp, True, st.T, 1,
                                             q_scale=scale * ops.Q_PRESCALE)
            if i == 0 and step_begin is not None:               # replayed greedy step: the embedding gather + rotation-row staging
                sb = step_begin                                 # ride in this projection's prologue when the library takes the shape
                w_fold = self._fold_weight(k_w, B)
                if not (w_fold is not None and ops.gemv_step_begin(sb["tok"], sb["table"], x, st.cos, st.sin, d_past, sb["cos_o"],
                                                                   sb["sin_o"], w_fold, w[p + "input_layernorm.weight"], eps, qkv)):
                    ops.step_begin(sb["tok"], sb["table"], x, st.cos, st.sin, d_past, sb["cos_o"], sb["sin_o"])
                    self._proj(x, k_w, norm_w=w[p + "input_layernorm.weight"], out=qkv, h=h)
            elif not fused_qkv:
                if normed_in:                                   # `h` holds RMSNorm(x) already (the previous down_proj's reduction launch)
                    self._proj(h, p + "self_attn.qkv_proj.weight", out=qkv)
                else:
                    self._proj(x, p + "self_attn.qkv_proj.weight", norm_w=w[p + "input_layernorm.weight"], out=qkv, h=h)
            o_i, kw_o = o, {}
            if fuse_o:                                          # (B = L = 1 plans only) + o_proj + residual in the attention's launch,
                o_i, o_other = (plan.o_f, plan.o_f2) if i % 2 == 0 else (plan.o_f2, plan.o_f)   # x += bf16(W_o . o)
                kw_o = self._fused_oproj_kw(p + "self_attn.o_proj.weight", x, o_other)
            if st.quantized:
                if decode:
                    ops.attention_decode_q8(qkv, rc, rs, rb, st.k8[i], st.v8[i], st.ks[i], st.vs[i], o_i, B, L, nh, nkv,
                                            hd, scale, past, st.Tp, ws, n_split, pad_len=st.pad_len, d_past=d_past,
                                            merge_in_launch=attn_merge, **kw_o)
                else:                                           # prefill: exact attention, quantised copy stored
                    if past > 0 and not st.fresh_rows:          # long cached call (constrain with > 16 tokens): attend on a
                        ops.kv_dequantize(st.k8[i], st.v8[i], st.ks[i], st.vs[i], st.k_tmp, st.v_tmp, past)   # dequantised copy
                    if not fused_qkv:
                        ops.rope_kv_append(qkv, st.cos, st.sin, q, st.k_tmp, st.v_tmp, B, L, nh, nkv, hd, past, st.Tp, True, st.T, 1,
                                           q_scale=scale * ops.Q_PRESCALE)
                    ops.attention(q, o, B, L, nh, nkv, hd, scale, True, past=past, k_past=st.k_tmp, v_past=st.v_tmp,
                                  past_t=st.Tp, pad_len=st.pad_len, new_is_cache=True, q_prescaled=True)
                    ops.kv_quantize(st.k_tmp, st.v_tmp, st.k8[i], st.v8[i], st.ks[i], st.vs[i], past, L)
            elif n_beam > 1:
                ops.rope_kv_append(qkv, st.cos, st.sin, q, k_new, v_new, B, L, nh, nkv, hd, past, Lp, False, st.T, n_beam)
                ops.attention(q, o, B, L, nh, nkv, hd, scale, True, k_new=k_new, v_new=v_new, new_t=Lp, past=past,
                              k_past=st.k[i], v_past=st.v[i], past_t=st.Tp, past_div=n_beam, pad_len=st.pad_len,
                              pad_div=n_beam, ws=ws, n_split=n_split)
            elif decode and plan.family:                        # a state with a family table: its prompts' K/V read once per family
                ops.attention_decode_family(qkv, rc, rs, rb, st.k[i], st.v[i], o_i, B, nh, nkv, hd, scale,
                                            past if d_past is None else plan.past_lb, st.Tp, ws, n_split, st.family,
                                            family_host=st.family_host, pad_len=st.pad_len, d_past=d_past)
            elif decode:
                # (captured step: `past` is read from d_past; the host value passed along is a LOWER BOUND of it -- the kernel fetches
                #  tiles below it at once and lets the others wait for the length, so tiles beyond the live keys cost nothing)
                ops.attention_decode(qkv, rc, rs, rb, st.k[i], st.v[i], o_i, B, L, nh, nkv, hd, scale,
                                     past if d_past is None else plan.past_lb, st.Tp, ws, n_split,
                                     pad_len=st.pad_len, d_past=d_past, merge_in_launch=attn_merge, **kw_o)
            else:
                # queries leave the RoPE kernel multiplied by scale * log2(e) (before their one rounding to bf16, as
                # phi.py:454 scales q before the product): the prefill attention's softmax is then the exponential alone
                if not fused_qkv:
                    ops.rope_kv_append(qkv, st.cos, st.sin, q, st.k[i], st.v[i], B, L, nh, nkv, hd, past, st.Tp, True, st.T, 1,
                                       q_scale=scale * ops.Q_PRESCALE)
                ops.attention(q, o, B, L, nh, nkv, hd, scale, True, past=past, k_past=st.k[i], v_past=st.v[i],
                              past_t=st.Tp, pad_len=st.pad_len, new_is_cache=True, q_prescaled=True)
            if mlx4_first:                                      # this layer attended on the exact keys (phi.py:533); from now on: the codes
                self._mlx4_quantize(st, i, L, qkv, nh)          # (keys from their exact fp32 values: recomputed from `qkv`)
            if last_only and i == cfg.num_hidden_layers - 1 and L > 1:
                o = o.view(B, L, -1)[:, -1].contiguous()
                x = x.view(B, L, -1)[:, -1].contiguous()
                a, h = a[:B], h[:B]
                if self._bank:
                    self._rows_cur = self._state_rows(st) if B == st.B else self._state_rows(st).repeat_interleave(B // st.B)
            # Short prompts and decode batches (9 .. 256 rows): o_proj and down_proj run as K slices, and the launch that adds the slices also writes the
            # RMSNorm of the new residual stream into `h` -- the next projection's input (ops.gemm_resid_norm; bit-identical to the
            # two launches it replaces).
            normed = False
            if not (fuse_o and decode and n_beam == 1):
                normed = self._proj_resid_norm(o, p + "self_attn.o_proj.weight", x, w[p + "post_attention_layernorm.weight"], h)
                if not normed:
                    self._proj(o, p + "self_attn.o_proj.weight", EPI_RESID_BF16, resid=x, out=x)
            if normed:
                self._proj(h, p + "mlp.gate_up_proj.weight", EPI_SILU_MUL, out=a)
            else:
                self._proj(x, p + "mlp.gate_up_proj.weight", EPI_SILU_MUL, norm_w=w[p + "post_attention_layernorm.weight"], out=a, h=h)
            normed_in = False
            if i + 1 < cfg.num_hidden_layers:
                normed_in = self._proj_resid_norm(a, p + "mlp.down_proj.weight", x, w[f"model.layers.{i + 1}.input_layernorm.weight"], h)
            if not normed_in:
                self._proj(a, p + "mlp.down_proj.weight", EPI_RESID_BF16, resid=x, out=x)
            if self.hidden_hook is not None:                     # diagnostics only (tools/precision_decomp.py); never set
                self.hidden_hook(i, x, B, x.shape[0] // B)       # while a decode graph is captured
        if mlx4_first:
            st.mlx4_tokens = L
        return x

    def _mlx4_quantize(self, st, i, L, qkv, nh):
        if st.k4.shape[3] != L:                                 # (first call shorter than the state was sized for)
            nl, B, nkv, _, g, _ = st.k4.shape
            st.k4 = torch.zeros((nl, B, nkv, L, g, 4), dtype=I32, device=self.device)
            st.v4 = torch.zeros_like(st.k4)
            st.k_sb = torch.zeros((nl, B, nkv, L, g, 2), dtype=F32, device=self.device)
            st.v_sb = torch.zeros_like(st.k_sb)
        ops.kv_quantize_mlx4(st.k[i], st.v[i], st.k4[i], st.v4[i], st.k_sb[i], st.v_sb[i], L, qkv=qkv, cos_t=st.cos, sin_t=st.sin, nh=nh,
                             past=0, tab_t=st.T, tab_div=1)

    # ------------------------------------------------------------------ graph-replayed greedy decode step
    def _build_decode_graph(self, st):
        """Capture ONE greedy decode step (embed -> 32 layers -> norm+lm_head -> argmax ->
        bookkeeping) as a hipGraph.  All loop state lives in HBM: `tok` (next input ids),
        `d_past` (cache length), `d_step`, `history` -- so replays need no host input and
        a token costs one graph launch instead of ~170 kernel launches."""
        cfg, B, dev = self.cfg, st.B, self.device
        g = dict(tok=torch.zeros((B,), dtype=I32, device=dev), d_past=torch.zeros((1,), dtype=I32, device=dev),
                 d_step=torch.zeros((1,), dtype=I32, device=dev),
                 # the step's tokens land in PINNED HOST memory straight from `k_step_end` (one 4-byte store per row and step):
                 # the host loop reads them after the step's event, no D2H copy node sits between two replays (api.greedy_loop)
                 history=torch.zeros((B, max(1, st.max_tokens) + 1), dtype=I32).pin_memory(),
                 x=torch.empty((B, cfg.hidden_size), dtype=BF16, device=dev),
                 logits=torch.empty((B, cfg.vocab_size), dtype=BF16, device=dev),
                 next_tok=torch.zeros((B,), dtype=I32, device=dev), ticket=torch.zeros((1,), dtype=I32, device=dev))
        g["bufs"] = self._plan(st, B, 1, fuse_o=not st.slots, captured=True)
        g["amax_ws"] = torch.zeros((ops.L.GEMV_STEP_WS_BYTES // 4,), dtype=F32, device=dev)   # (its arrival counters start at zero)
        g["d_past"].fill_(st.offset)
        g["gemm_ws"] = {}                                        # B > 16 rows: the projections are split-K GEMMs; their workspace
        g["graph"] = self._capture(lambda: self._decode_step(st, g), g["gemm_ws"])   # belongs to the graph
        g["d_step"].zero_()                                      # the warm-up run counted as a step
        return g

    def _decode_step(self, st, g, kind=steps.GREEDY):
        """The launches of one decode step of a kind (steps.StepKind) over the loop state `g` of a greedy capture: the layers,
        then the step's tail -- final norm + lm_head + arg-max + bookkeeping, or with kind.sampled each row's token drawn under
        its record (`set_sampling`) where the greedy step has its arg-max.
        (round 6) the step's two ends have no launch of their own where the library folds them into the first / last projection
        (B = 1 on bf16, e4m3 or 4-bit weights: ops.gemv_step_begin / gemv_step_end; 129 launches per step instead of 131); the
        sampled tail always goes through `_proj` (every weight format, adapters honoured).
        kind.logprobs: ONE more launch behind that tail, whichever it is -- the record of each row's emitted token
        (p3v_logprobs_step) into the pinned `records` buffer; it reads the logits and the loop state and changes neither.
        kind.penalized (a sampled tail): ONE more launch between lm_head and the tail -- p3v_penalize counts the token this step
        was fed into the rows' `seen` table and writes the adjusted rows to the penalty state's second buffer, which the tail
        draws from (a T = 0 row: its arg-max); `logits` stays raw, for the caller and for the log-probability launch.
        kind.guided (a penalised step): ONE more launch between p3v_penalize and the tail -- p3v_guide_mask walks the token this
        step was fed through each guided row's DFA and bans, in the adjusted rows, what the new state does not allow."""
        cfg, w, bufs, head = self.cfg, self.w, g["bufs"], "lm_head.weight"
        self._layers(g["x"], st, st.B, 1, 0, 1, bufs=bufs, d_past=g["d_past"],
                     step_begin=dict(tok=g["tok"], table=w["model.embed_tokens.weight"], cos_o=bufs["plan"].rope_cos, sin_o=bufs["plan"].rope_sin))
        end = (g["next_tok"], g["tok"], g["history"], g["d_step"], g["d_past"], g["ticket"])
        if not kind.sampled:
            w_fold = self._fold_weight(head, st.B)
            if w_fold is not None and ops.gemv_step_end(g["x"], w_fold, w["model.norm.weight"], cfg.rms_norm_eps, g["logits"], *end, g["amax_ws"]):
                return self._logprobs_tail(st, g) if kind.logprobs else None
        self._proj(g["x"], head, norm_w=w["model.norm.weight"], out=g["logits"], h=bufs["h"])   # (h: the norm's output)
        if kind.penalized:
            pen = st.penalty
            ops.penalize(g["logits"], pen["rows"], pen["seen"], pen["bias"], g["tok"], out=pen["adj"])
            if kind.guided:
                self._guide_mask(pen["adj"], st.guide, slice(0, st.B), g["tok"])
            ops.sample_step_end(pen["adj"], st.sample_rows, *end)
        elif kind.sampled:
            ops.sample_step_end(g["logits"], st.sample_rows, *end)
        else:
            ops.step_end(g["logits"], *end)
        if kind.logprobs:
            self._logprobs_tail(st, g)

    def _logprobs_tail(self, st, g):
        ops.logprobs_step(g["logits"], g["next_tok"], st.logprob_want, g["d_step"], g["records"])

    def _replay(self, token, cache, kind):
        """One decode step of a kind (steps.StepKind) through its captured graph.  The greedy kind's graph is the greedy capture's
        own; every other kind is a further capture over the same loop state, built on first use (`_build_capture`) -- after the
        token and the cache length are in place, which its warm-up run reads.  Returns (logits [B,1,V], next_token [B,1]), views
        of persistent buffers."""
        st = cache[0].state
        if st.offset + 1 > st.T:
            raise ValueError(f"KV cache overflow: {st.offset}+1 > {st.T} (prompt + max_tokens)")
        g = self._greedy_capture(st)
        if g["host_tok"] is None or token is not g["host_tok"]:
            g["tok"].copy_(token.reshape(-1).to(self.device, I32))   # first step / caller-chosen token
        if g.get("synced_offset") != st.offset:
            g["d_past"].fill_(st.offset)
        if kind.capture not in g:
            g[kind.capture] = self._build_capture(st, g, kind)
        g[kind.capture].launch()
        g["n_replays"] = g.get("n_replays", 0) + 1              # replay r, greedy or sampled, wrote its token to history[:, r - 1] (while it fits)
        st.offset += 1
        g["synced_offset"] = st.offset
        g["host_tok"] = g["next_tok"].view(-1, 1)
        return g["logits"].view(st.B, 1, -1), g["host_tok"]

    @staticmethod
    def _reset_replays(g):
        """A greedy capture starts a new run on the same buffers (a reused captured-prefill entry): forget the last run's replays."""
        g["n_replays"], g["host_tok"], g["synced_offset"] = 0, None, None
        g["d_step"].zero_()

    @_on_device
    def restart_history(self, st):
        """A long-lived state (the engine's slot state) has used up the `history` / `records` slots of its greedy capture: count
        its steps from 0 again.  Tokens, logits and the cache are untouched; the next replay writes slot 0."""
        g = st.graphs.get("greedy")
        if g is not None:
            self._reset_replays(g)

    @_on_device
    def greedy_prefill(self, max_tokens, **inputs):
        """Prefill + first greedy token: `logits, cache = model(**inputs, max_tokens); argmax(logits[:, -1])`
        (reference phi_3_vision_mlx.py:385-386).  Returns (token [B,1] int32 on the device, cache)."""
        logits, cache = self(**inputs, max_tokens=max_tokens)
        return ops.argmax(logits[:, -1, :].contiguous())[:, None], cache

    # ------------------------------------------------------------------ speculative greedy decoding (include/p3v.h, speculate.py)
    def spec_refusal(self, st=None, K=None):
        """Why this model (and state) cannot run verify steps -- a sentence that names the limit -- or None."""
        from . import speculate
        cfg = self.cfg
        if K is not None and not 1 <= int(K) <= ops.L.DECODE_MAX_L - 1:
            return f"speculate must be 1 .. {ops.L.DECODE_MAX_L - 1} (P3V_DECODE_MAX_L - 1 draft rows), got {K}"
        if getattr(cfg, "use_quantized_cache", False):
            fmt = getattr(cfg, "cache_format", "int8")
            return f"speculative decoding needs the bf16 KV cache (cache_format={fmt!r} is not supported)"
        if self.w8 or self.w4:
            return "speculative decoding needs bf16 weights (fp8 / 4-bit weights are not supported)"
        if self.adapters or self._bank:
            return "speculative decoding does not support LoRA adapters or an adapter bank"
        if st is not None and st.B != 1:
            return f"speculative decoding is B = 1 only (got a batch of {st.B})"
        if st is not None and st.slots:
            return "speculative decoding does not run on a slot state of the continuous engine"
        return None

    def _build_spec_graph(self, st, K, n_max, n_min):
        """Capture ONE verify step (B = 1, L = K + 1 rows: p3v_spec_begin -> the layers at L rows -> final norm + lm_head on L rows
        -> p3v_spec_end) beside the greedy capture, over loop-state buffers of its own.  Same conventions: split plan from the cache
        CAPACITY, the graph owns its GEMM workspace, a warm-up run before the capture, nothing allocated under it."""
        cfg, w, dev, Lq = self.cfg, self.w, self.device, K + 1
        n_tok = max(1, st.max_tokens)
        g = dict(K=K, tok=torch.zeros((Lq,), dtype=I32, device=dev), ctx=torch.zeros((st.T + Lq,), dtype=I32, device=dev),
                 ctl=torch.zeros((ops.L.SPEC_CTL_INTS,), dtype=I32, device=dev), amax=torch.zeros((Lq,), dtype=I32, device=dev),
                 ticket=torch.zeros((1,), dtype=I32, device=dev), d_past=torch.zeros((1,), dtype=I32, device=dev),
                 d_step=torch.zeros((1,), dtype=I32, device=dev),
                 # pinned host memory, written by p3v_spec_end itself: the run's tokens and one record per replay
                 history=torch.zeros((n_tok + K + 1,), dtype=I32).pin_memory(),
                 rec=torch.zeros((n_tok + 2, ops.L.SPEC_REC_INTS), dtype=I32).pin_memory(),
                 x=torch.empty((Lq, cfg.hidden_size), dtype=BF16, device=dev),
                 logits=torch.empty((Lq, cfg.vocab_size), dtype=BF16, device=dev), n_replays=0)
        g["state"] = ops.spec_state(g, n_max, n_min)
        bufs = g["bufs"] = self._plan(st, 1, Lq, fuse_o=False, captured=True)

        def step():
            ops.spec_begin(g["tok"], w["model.embed_tokens.weight"], g["x"], st.cos, st.sin, g["d_past"], bufs["plan"].rope_cos, bufs["plan"].rope_sin)
            self._layers(g["x"], st, 1, Lq, 0, 1, bufs=bufs, d_past=g["d_past"])
            self._proj(g["x"], "lm_head.weight", norm_w=w["model.norm.weight"], out=g["logits"], h=bufs["h"])
            ops.spec_end(g["logits"], g["state"])
        g["step"] = step
        # the warm-up run is a step at the budget (n = n_limit = 0): it emits nothing and moves no counter but `replay`
        g["d_past"].fill_(st.offset)
        g["gemm_ws"] = {}
        g["graph"] = self._capture(step, g["gemm_ws"])
        return g

    @_on_device
    def spec_start(self, cache, ids, token, K, n_limit=None, forced=False, n_max=None, n_min=None):
        """Arm the verify-step capture of a state for a run: `ids` (the ids in the cache, prompt first: st.offset of them) and
        `token` (the newest token, not yet in the cache) become ctx with ONE host -> device copy, the first draft is proposed by
        p3v_ngram_propose.  n_limit: ctx never grows beyond it (default: the state's prompt + max_tokens budget).  forced: the tail
        proposes nothing; the caller writes the drafts before every step (`spec_force`).  Returns the capture's buffers."""
        from . import speculate
        st = cache[0].state
        why = self.spec_refusal(st, K)
        if why:
            raise ValueError(why)
        n_max, n_min = speculate.N_MAX if n_max is None else n_max, speculate.N_MIN if n_min is None else n_min
        ids = np.asarray(ids.cpu() if torch.is_tensor(ids) else ids).reshape(-1).astype(np.int32)
        if ids.size != st.offset:
            raise ValueError(f"spec_start: {ids.size} ids for a cache that holds {st.offset}")
        budget = st.T - K                                         # a step at n writes cache rows n - 1 .. n - 1 + K
        n_limit = budget if n_limit is None else int(n_limit)
        if n_limit > budget or ids.size + 1 > budget:
            raise ValueError(f"KV cache too small for verify steps up to {n_limit} tokens: capacity {st.T}, K = {K} "
                             "(prefill with extra_tokens=K)")
        self._sync_epoch(st)
        key = ("spec", K, n_max, n_min)
        g = st.graphs.get(key)
        if g is not None and st.offset < g["bufs"]["plan"].past_lb:  # rewound below the captured lower bound (as _greedy_capture)
            g = None
        if g is None:
            g = st.graphs[key] = self._build_spec_graph(st, K, n_max, n_min)
        n = ids.size + 1
        tok0 = int(np.asarray(token.cpu() if torch.is_tensor(token) else token).reshape(-1)[0])
        host = torch.empty((n + ops.L.SPEC_CTL_INTS,), dtype=I32).pin_memory() if g.get("host_ctx") is None or g["host_ctx"].numel() < n + ops.L.SPEC_CTL_INTS else g["host_ctx"]
        g["host_ctx"] = host
        host[:ids.size] = torch.from_numpy(ids)
        host[ids.size] = tok0
        g["ctx"][:n].copy_(host[:n], non_blocking=True)          # the one H2D copy of the run
        ctl = [n, 0, int(bool(forced)), 0, n_limit, 0, 0, 0]
        g["ctl"].copy_(torch.tensor(ctl, dtype=I32))
        g["tok"].fill_(tok0)
        g["d_past"].fill_(st.offset)
        g["d_step"].zero_()
        g["n_replays"], g["forced"], g["n0"] = 0, bool(forced), n
        if not forced:
            ops.ngram_propose(g["ctx"], n, K, n_max, n_min, self.cfg.vocab_size, g["tok"][1:], g["ctl"][ops.L.SPEC_CTL_NDRAFT:ops.L.SPEC_CTL_NDRAFT + 1])
        st.graphs["spec"] = g                                    # the armed capture
        return g

    @_on_device
    def spec_force(self, cache, drafts):
        """Forced-draft hook (tests): the next verify step checks `drafts` (at most K ids) instead of a proposal."""
        g = cache[0].state.graphs["spec"]
        d = [int(t) for t in drafts][:g["K"]]
        if d:
            g["tok"][1:1 + len(d)].copy_(torch.tensor(d, dtype=I32))
        g["ctl"][ops.L.SPEC_CTL_NDRAFT:ops.L.SPEC_CTL_NDRAFT + 1].fill_(len(d))

    @_on_device
    def spec_step(self, cache, K, eager=False):
        """One verify step through its captured graph (after `spec_start`): feeds the last token + up to K drafts, accepts the
        longest run the arg-maxes confirm, emits accepted + 1 tokens into the capture's pinned `history`, records
        {emitted, drafted, drafts} in `rec[replay]`, advances the device's cache length and proposes the next drafts -- no host
        input, so steps replay back to back.  The host's `st.offset` is NOT advanced here: the caller adds what `rec` reports
        (`spec_sync`).  eager=True runs the same launches outside the graph.  Returns the capture's buffers."""
        st = cache[0].state
        g = st.graphs.get("spec")
        if g is None or g["K"] != K or st.epoch != self.epoch:
            raise RuntimeError("spec_step: no armed capture for this K on this state (model.spec_start)")
        if g["n_replays"] >= g["rec"].shape[0]:
            raise ValueError(f"spec_step: more than {g['rec'].shape[0]} steps on a run of {st.max_tokens} tokens")
        if eager:
            with ops.owned_gemm_workspace(g["gemm_ws"], frozen=True):
                g["step"]()
        else:
            g["graph"].launch()
        g["n_replays"] += 1
        return g

    @_on_device
    def spec_sync(self, cache):
        """Wait for the steps enqueued so far and bring the host's offset up to the device's: returns the run's tokens so far
        (a list, from the pinned history)."""
        st = cache[0].state
        g = st.graphs["spec"]
        torch.cuda.current_stream().synchronize()
        n_emit = int(g["rec"][:g["n_replays"], 0].sum())
        st.offset = g["n0"] - 1 + (n_emit if not (n_emit and g["history"][n_emit - 1] < 0) else 0)
        return g["history"][:n_emit].tolist()

    # ------------------------------------------------------------------ beam search (include/p3v.h "beam search", beam.py)
    def beam_refusal(self, st=None, W=None):
        """Why this model (and the B = 1 state of a finished prefill) cannot run beam steps -- a sentence that names the limit --
        or None."""
        cfg = self.cfg
        if W is not None and (isinstance(W, bool) or not isinstance(W, int) or not 2 <= W <= ops.L.BEAM_MAX):
            return f"num_beams must be 1 (off) or an integer in 2..{ops.L.BEAM_MAX} (P3V_BEAM_MAX), got {W!r}"
        if getattr(cfg, "use_quantized_cache", False):
            fmt = getattr(cfg, "cache_format", "int8")
            return f"beam search needs the bf16 KV cache: the reorder has no {fmt} form (cache_format={fmt!r} is not supported)"
        if self._bank:
            return "beam search does not run on an adapter bank (rows of one request would need one table entry each)"
        if st is not None and (st.B != 1 or st.slots):
            return "beam search starts from the B = 1 state of one prompt's prefill (not a batch, not a slot state of the continuous engine)"
        if W is not None and cfg.vocab_size < 2 * W:
            return f"beam search needs a vocabulary of at least 2 * num_beams = {2 * W} tokens"
        return None

    def _build_beam_graph(self, st, W, eos):
        """Capture ONE beam step of a B = W state beside whatever else it holds, over loop-state buffers of its own: the step head
        on tok[W] -> the layers at B = W (the path n completions take; the family launch where the state has a table) -> final
        norm + lm_head on W rows -> p3v_beam_end -> the reorder's gather and scatter.  The window of the reorder starts at the
        prompt's end rounded down to 8 columns, a launch constant: the state is one request's.  The capture's warm-up run is a
        step like any other (it writes the not-yet-live column st.offset and moves bytes only among equal prompt columns and that
        column); `beam_start` arms the loop state afterwards."""
        cfg, w, dev = self.cfg, self.w, self.device
        n_tok = max(1, st.max_tokens)
        g = dict(W=W, eos=int(eos), tok=torch.zeros((W,), dtype=I32, device=dev), parent=torch.zeros((W,), dtype=I32, device=dev),
                 cum=torch.zeros((W,), dtype=F32, device=dev),
                 cand_id=torch.zeros((2 * ops.L.BEAM_MAX * ops.L.BEAM_MAX,), dtype=I32, device=dev),
                 cand_score=torch.zeros((2 * ops.L.BEAM_MAX * ops.L.BEAM_MAX,), dtype=F32, device=dev),
                 ticket=torch.zeros((1,), dtype=I32, device=dev), d_past=torch.zeros((1,), dtype=I32, device=dev),
                 d_step=torch.zeros((1,), dtype=I32, device=dev),
                 # pinned host memory, written by p3v_beam_end itself: one record per step
                 rec=torch.full((n_tok + 2, ops.L.BEAM_REC_INTS), -1, dtype=I32).pin_memory(),
                 x=torch.empty((W, cfg.hidden_size), dtype=BF16, device=dev),
                 logits=torch.empty((W, cfg.vocab_size), dtype=BF16, device=dev), n_replays=0)
        g["state"] = ops.beam_state(g)
        bufs = g["bufs"] = self._plan(st, W, 1, fuse_o=False, captured=True)
        kv = self._state_kv(st)
        c0a = g["c0a"] = st.offset // 8 * 8
        g["stage"] = ops.kv_permute_stage(kv, W, max(8, (st.T - c0a + 7) // 8 * 8))

        def forward():
            self._layers(g["x"], st, W, 1, 0, 1, bufs=bufs, d_past=g["d_past"],
                         step_begin=dict(tok=g["tok"], table=w["model.embed_tokens.weight"], cos_o=bufs["plan"].rope_cos, sin_o=bufs["plan"].rope_sin))
            self._proj(g["x"], "lm_head.weight", norm_w=w["model.norm.weight"], out=g["logits"], h=bufs["h"])

        def select():
            ops.beam_end(g["logits"], g["state"], W, eos)

        def reorder():
            for phase in (0, 1):
                ops.kv_permute(kv, g["parent"], W, c0a, g["d_past"], g["stage"], phase)

        def step():
            forward(), select(), reorder()
        g["parts"], g["step"] = (forward, select, reorder), step
        g["d_past"].fill_(st.offset)
        g["gemm_ws"] = {}
        g["graph"] = self._capture(step, g["gemm_ws"])
        return g

    @_on_device
    def beam_start(self, cache, logits_row, W, eos, share=False):
        """Start a beam search of width W behind ONE prompt's prefill: `cache` is its B = 1 cache, `logits_row` its last logits
        row.  The state is forked into W rows (`fork_state`; share: registered as a family where parallel.family_pays says so --
        the shared columns are never permuted, so the table stays valid), the step is captured on the new state
        (`st.graphs[("beam", W)]`), the loop state armed, and step 0 -- the selection from the one prefill row, R = 1 -- launched.
        Returns the capture's buffers; `g["cache"]` is the B = W cache the steps run on."""
        st1 = cache[0].state
        W = int(W) if isinstance(W, (int, np.integer)) and not isinstance(W, bool) else W
        why = self.beam_refusal(st1, W)
        if why:
            raise ValueError(why)
        row = logits_row.reshape(1, -1).to(self.device, BF16).contiguous()
        if row.shape[1] != self.cfg.vocab_size:
            raise ValueError(f"beam_start: one row of {self.cfg.vocab_size} logits, got {tuple(logits_row.shape)}")
        bcache = self.fork_state(st1, W, share=share)
        st = bcache[0].state
        self._sync_epoch(st)
        if st.family is None:                                    # every beam state takes the family launch, shared prefix or not: ONE
            self.set_families(st, [], create=True)               # split plan, so a search's records do not depend on `share`
        g = st.graphs[("beam", W)] = self._build_beam_graph(st, W, eos)
        g["cache"], g["S0"] = bcache, st.offset
        g["cum"].zero_(), g["d_step"].zero_(), g["ticket"].zero_(), g["rec"].fill_(-1)
        g["d_past"].fill_(st.offset - 1)                         # step 0 appends no column: its count of one brings the length to st.offset
        ops.beam_end(row, g["state"], W, eos)
        g["n_replays"] = 1
        st.graphs["beam"] = g                                    # the armed capture
        return g

    @_on_device
    def beam_step(self, cache, eager=False):
        """One beam step through its captured graph (after `beam_start`, on `g["cache"]`): feeds the W beams' tokens, selects the
        next W from their 2W best continuations each, writes record `n_replays` to the capture's pinned `rec`, advances the
        device's counters and reorders the cache rows -- no host input, so steps replay back to back.  The host's `st.offset` is
        NOT advanced here (`beam_sync`).  eager=True runs the same launches outside the graph.  Returns the capture's buffers."""
        st = cache[0].state
        g = st.graphs.get("beam")
        if g is None or st.epoch != self.epoch:
            raise RuntimeError("beam_step: no armed capture on this state (model.beam_start)")
        if g["n_replays"] >= max(1, st.max_tokens) or g["S0"] + g["n_replays"] > st.T:
            raise ValueError(f"KV cache overflow: beam step {g['n_replays']} of a run of {st.max_tokens} tokens (prompt + max_tokens = {st.T})")
        if eager:
            with ops.owned_gemm_workspace(g["gemm_ws"], frozen=True):
                g["step"]()
        else:
            g["graph"].launch()
        g["n_replays"] += 1
        return g

    @_on_device
    def beam_sync(self, cache, n_records=None):
        """Wait for the steps enqueued so far and set the host's offset behind record `n_records - 1` (default: every record so
        far; fewer: the overrun steps are dropped, their columns lie beyond the offset).  Returns the records, int32 [n, 42]."""
        st = cache[0].state
        g = st.graphs["beam"]
        torch.cuda.current_stream().synchronize()
        n = g["n_replays"] if n_records is None else max(1, min(int(n_records), g["n_replays"]))
        st.offset = g["S0"] + n - 1
        return g["rec"][:n].numpy().copy()

    # ------------------------------------------------------------------ seeded sampling (include/p3v.h: p3v_sample_row_t)
    @_on_device
    def set_sampling(self, st, records, row0=0):
        """Write the per-row sampling records (sampling.pack: int32 [n, 6] on the host) of rows row0 .. row0+n-1 of a state (one
        H2D copy, outside any graph).  Rows never written are greedy (temperature 0).  The records live with the state's decode
        graphs and are read -- and their counters advanced -- by `sample_logits` and every replay of `sample_step`."""
        self._option_table(st, "sampled")[row0:row0 + records.shape[0]].copy_(records)

    @_on_device
    def sample_logits(self, st, logits, row0=0):
        """The first token of rows row0 .. row0+n-1 from their prefill logits ([n, L, V] or [n, V]) under their records (the
        draw index is the record's counter, 0 after `set_sampling(..., counter=0)`).  int32 [n, 1] on the device."""
        last, rows = _last_rows(logits, row0)
        return ops.sample(last, st.sample_rows[rows])[:, None]

    # ------------------------------------------------------------------ captures of the step kinds (steps.py has the table)
    # what a warm-up run of a kind moves beside the loop state, by flag: it is saved before the capture and put back after it
    _WARMUP_MOVES = (("sampled", lambda st: st.sample_rows),        # the records' draw counters
                     ("penalized", lambda st: st.penalty["seen"]),  # the count of the fed token
                     ("guided", lambda st: st.guide["rows"]))       # the walk of the fed token

    def _build_capture(self, st, g, kind):
        """Capture the step of a kind over the loop state of the greedy capture `g` (`_decode_step` has the launches).  The warm-up
        run leaves every piece of state it moves -- tokens, counters, history, and by the kind's flags the `_WARMUP_MOVES` -- as
        it found it.  The records of the log-probability kinds land in a pinned buffer beside `history`, made with the first of
        them (row b's record of replay r: `records[b, r - 1]`).  Each capture owns its GEMM workspaces."""
        torch.cuda.synchronize()
        if kind.logprobs and "records" not in g:
            g["records"] = torch.zeros((st.B, g["history"].shape[1], ops.L.LOGPROB_WORDS), dtype=I32).pin_memory()
        moved = [g[k] for k in ("tok", "next_tok", "d_step", "d_past", "history")]
        moved += [of(st) for flag, of in self._WARMUP_MOVES if getattr(kind, flag)]
        saved = [t.clone() for t in moved]
        ws = g["gemm_ws_" + kind.capture] = {}
        graph = self._capture(lambda: self._decode_step(st, g, kind), ws)
        for t, v in zip(moved, saved):
            t.copy_(v)
        torch.cuda.synchronize()
        return graph

    @staticmethod
    def _drop_captures(st, flag):
        """Forget the state's captures of every kind with a flag set: they baked in a pointer that is being replaced."""
        g = st.graphs.get("greedy")
        if g is not None:
            for kind in steps.with_flag(flag):
                g.pop(kind.capture, None)

    # ------------------------------------------------------------------ the option tables of a state (steps.NEEDS; CacheState)
    def _option_table(self, st, flag, bias=False):
        """The state's table of the option with that flag, made on first use at the shapes ops.L names, every row inactive (greedy
        sampling records, penalty and guide records their kernels copy through, wants of -1).  bias: the penalty state's [B,
        vocab] bias table too.  What is made replaces a pointer -- or a null -- the captures with that flag baked in: dropped."""
        attr, zeros = _ATTR[flag], functools.partial(torch.zeros, dtype=I32, device=self.device)
        B, V, L = st.B, self.cfg.vocab_size, ops.L
        t = st.shared.get(attr)
        if t is None or _records(t).shape[0] != B:
            t = st.shared[attr] = {
                "sampled": lambda: zeros((B, L.C.sizeof(L.SampleRow) // 4)),
                "penalized": lambda: dict(rows=zeros((B, L.PENALTY_WORDS)), seen=zeros((B, V)),
                                          adj=torch.empty((B, V), dtype=BF16, device=self.device), bias=None),
                "guided": lambda: dict(rows=zeros((B, L.GUIDE_WORDS)), delta=zeros((B, 256, 256), dtype=torch.int16),
                                       accept=zeros((B, 256), dtype=torch.uint8)),
                "logprobs": lambda: zeros((B,)).fill_(_OFF["logprobs"])}[flag]()
            self._drop_captures(st, flag)
        if bias and t["bias"] is None:
            t["bias"] = zeros((B, V), dtype=F32)
            self._drop_captures(st, flag)
        return t

    def _clear(self, st, flag, row0=0, n=None):
        """Rows row0 .. row0+n-1 (default: to the end) become inactive for an option, where the state has its table."""
        t = st.shared.get(_ATTR[flag])
        if t is not None:
            _records(t)[row0:None if n is None else row0 + n].fill_(_OFF.get(flag, 0))

    # ------------------------------------------------------------------ penalties and logit_bias (include/p3v.h: p3v_penalty_row_t)
    @_on_device
    def set_penalties(self, st, records, prompt_ids, row0=0, bias=None, pad=None):
        """Give rows row0 .. row0+n-1 of a state their penalty records (penalties.pack: int32 [n, 4] on the host) and start their
        `seen` rows from their prompts: prompt_ids (int [n, S] on the host; pad: per-row count of left-padding ids to skip, None =
        0) are noted with p3v_penalty_note(clear=1, as_prompt=1) -- ids outside the vocabulary (image slots) are skipped.
        bias: fp32 [n, vocab] on the host (penalties.bias_table) or None.  The first call makes the state's `seen` table and the
        adjusted-logits buffer ([B, vocab] each) and greedy sampling records where the state has none (the penalised step's tail
        is the sampled one); the first call WITH a bias makes the [B, vocab] bias table -- captures made before it baked a null
        pointer in and are dropped.  One H2D copy per operand and one scatter, outside any graph."""
        n = records.shape[0]
        pen = self._option_table(st, "penalized", bias=bias is not None)
        self._option_table(st, "sampled")
        if bias is not None:
            pen["bias"][row0:row0 + n].copy_(torch.as_tensor(np.ascontiguousarray(bias, dtype=np.float32)).view(n, self.cfg.vocab_size))
        pen["rows"][row0:row0 + n].copy_(records)
        self.rebuild_penalties(st, prompt_ids, None, row0, pad)

    @_on_device
    def rebuild_penalties(self, st, prompt_ids, emitted, row0=0, pad=None):
        """Rebuild the `seen` rows row0 .. row0+n-1 from scratch -- wherever a step may be repeated or a state re-planned, instead
        of replaying increments: the prompts with clear=1, as_prompt=1, then `emitted` (int [n, m] on the host, or None: the
        tokens the rows have been FED so far, i.e. everything they emitted but the newest) with as_prompt=0."""
        pen, dev = st.penalty, self.device
        ids = np.asarray(prompt_ids)
        ids = (ids[None] if ids.ndim == 1 else ids).astype(np.int32)
        n, S = ids.shape
        first = np.zeros(n, dtype=np.int32) if pad is None else np.asarray(pad, dtype=np.int32).reshape(n)
        seen = pen["seen"][row0:row0 + n]
        ops.penalty_note(seen, torch.from_numpy(np.ascontiguousarray(ids)).to(dev), torch.from_numpy(first).to(dev),
                         torch.from_numpy((S - first).astype(np.int32)).to(dev), as_prompt=True, clear=True)
        if emitted is not None:
            em = np.asarray(emitted).astype(np.int32).reshape(n, -1)
            if em.shape[1]:
                ops.penalty_note(seen, torch.from_numpy(np.ascontiguousarray(em)).to(dev), torch.zeros((n,), dtype=I32, device=dev),
                                 torch.full((n,), em.shape[1], dtype=I32, device=dev), as_prompt=False)

    @_on_device
    def clear_penalties(self, st, row0=0, n=None):
        """Rows row0 .. row0+n-1 (default: to the end) become inactive: the penalised step copies their logits through."""
        self._clear(st, "penalized", row0, n)

    @_on_device
    def penalized_logits(self, st, logits, row0=0):
        """The adjusted rows of rows row0 .. row0+n-1's logits ([n, L, V] or [n, V]: the last position) under their records --
        the eager form, for the token drawn from the PREFILL logits: nothing is fed, nothing is counted.  bf16 [n, V], a new
        tensor; `logits` is not written."""
        pen = st.penalty
        if pen is None:
            raise RuntimeError("penalized_logits: no penalty state on this state (model.set_penalties)")
        last, rows = _last_rows(logits, row0)
        return ops.penalize(last, pen["rows"][rows], pen["seen"][rows], None if pen["bias"] is None else pen["bias"][rows])

    # ------------------------------------------------------------------ guided decoding (include/p3v.h: p3v_guide_row_t, guide.py)
    @_on_device
    def set_guide_vocab(self, table, eos):
        """The vocabulary table of guided decoding (guide.token_bytes: one per processor) as device tensors, made once, and the
        EOS id the mask is launched with.  A different table replaces the old one; captures that baked the old pointers in are
        dropped with their states' guide state."""
        cur = getattr(self, "_guide_vocab", None)
        if cur is not None and cur["table"] is table and cur["eos"] == int(eos):
            return
        if table.n < self.cfg.vocab_size:
            raise ValueError(f"set_guide_vocab: the table covers {table.n} ids, the model's vocabulary holds {self.cfg.vocab_size}")
        if cur is not None:
            for st in list(self._states):
                if st.guide is not None:
                    self._drop_captures(st, "guided")
        dev = self.device
        self._guide_vocab = dict(table=table, eos=int(eos), n_bytes=table.n_bytes,
                                 tok_off=torch.from_numpy(table.tok_off.view(np.int32).copy()).to(dev),
                                 tok_bytes=torch.from_numpy(table.tok_bytes.copy()).to(dev))

    def _guide_mask(self, rows2d, gd, rows, fed):
        v = self._guide_vocab
        return ops.guide_mask(rows2d, gd["rows"][rows], gd["delta"][rows], gd["accept"][rows], v["tok_off"], v["tok_bytes"], v["eos"],
                              fed=fed, n_bytes=v["n_bytes"])

    @_on_device
    def set_guides(self, st, guides, row0=0, states=None):
        """Give rows row0 .. row0+n-1 of a state their guides (guide.Dfa, or None for a row without one): each row's table
        region (at most 128 KB) and its record, at the start state -- or at states[i] (rebuilding a row after a re-plan).  The
        first call makes the state's guide state (records [B, 4], delta [B, 256, 256], accept [B, 256]) and, where the state has
        none, the penalty state and greedy sampling records, as `set_penalties` does: the guided step is the penalised one with
        one more launch.  One H2D copy per operand, outside any graph.  Needs `set_guide_vocab`."""
        from . import guide as guide_mod
        if getattr(self, "_guide_vocab", None) is None:
            raise RuntimeError("set_guides: no vocabulary table on this model (model.set_guide_vocab)")
        n = len(guides)
        if row0 < 0 or row0 + n > st.B:
            raise ValueError(f"set_guides: rows {row0} .. {row0 + n - 1} are outside the state's {st.B}")
        gd = [self._option_table(st, flag) for flag in ("guided", "penalized", "sampled")][0]
        recs = []
        for i, dfa in enumerate(guides):
            recs.append(guide_mod.record(dfa, 1 if states is None else states[i]))
            if dfa is None:
                continue
            delta, accept = guide_mod.region(dfa)               # (narrow up to 255 states, wide above: include/p3v.h)
            filled = guide_mod.region_rows(dfa)                 # (only the part of the 128 KB the guide fills is copied)
            gd["delta"][row0 + i, :filled].copy_(torch.from_numpy(delta[:filled].view(np.int16)))
            gd["accept"][row0 + i].copy_(torch.from_numpy(accept))
        if n:
            gd["rows"][row0:row0 + n].copy_(torch.tensor(recs, dtype=I32))

    @_on_device
    def clear_guides(self, st, row0=0, n=None):
        """Rows row0 .. row0+n-1 (default: to the end) become inactive: the guided step does not touch them."""
        self._clear(st, "guided", row0, n)

    @_on_device
    def guided_logits(self, st, logits, row0=0):
        """The masked rows of rows row0 .. row0+n-1 -- the eager form, for the token drawn from the PREFILL logits ([n, L, V] or
        [n, V]: the last position; after `penalized_logits` where the rows are penalised): nothing is fed, no state moves.
        bf16 [n, V], a new tensor; `logits` is not written."""
        gd = st.guide
        if gd is None:
            raise RuntimeError("guided_logits: no guide state on this state (model.set_guides)")
        last, rows = _last_rows(logits, row0)
        return self._guide_mask(last.clone(), gd, rows, None)

    # ------------------------------------------------------------------ token log-probabilities (include/p3v.h: p3v_logprob_t)
    @_on_device
    def set_logprobs(self, st, wants, row0=0):
        """Write the want-table entries of rows row0 .. row0+n-1 of a state: the N (0 .. 8) of a row whose tokens are to be
        scored, -1 for a row nobody asks about (every row, before the first call).  Like `set_sampling`, one H2D copy outside
        any graph: the captured log-probability launch reads the table."""
        wants = torch.as_tensor(list(wants), dtype=I32)
        if wants.numel() and (int(wants.min()) < -1 or int(wants.max()) > ops.L.LOGPROBS_MAX):
            raise ValueError(f"set_logprobs: entries are -1 (off) or 0..{ops.L.LOGPROBS_MAX}")
        self._option_table(st, "logprobs")[row0:row0 + wants.numel()].copy_(wants)

    @_on_device
    def logprobs_of(self, st, logits, tokens, row0=0):
        """The records of `tokens` (int32 [n] or [n, 1] on the device) on rows row0 .. row0+n-1's logits ([n, L, V] or [n, V]:
        the last position) under their want-table entries -- the eager call for a request's FIRST token, from its prefill
        logits.  int32 [n, 20] on the device (logprobs.unpack); rows at -1 are left zero."""
        if st.logprob_want is None:
            raise RuntimeError("logprobs_of: no want-table on this state (model.set_logprobs)")
        last, rows = _last_rows(logits, row0)
        return ops.logprobs(last, tokens.reshape(-1).to(I32).contiguous(), st.logprob_want[rows])

    @_on_device
    def __call__(self, input_ids, pixel_values=None, image_sizes=None, positions=None, cache=None, pids=None, mask=None,
                 max_tokens=0, advance_offset=None, n_beam=1, full_logits=None, row_adapters=None, prefix=None, extra_tokens=0):
        """Phi3ForCausalLM.__call__ (phi.py:606-608) + Phi3F.__call__ (phi.py:576-592).
        `extra_tokens` (prefill calls): cache columns beyond prompt + max_tokens, for speculative verify steps (`spec_step`).
        `row_adapters` (adapter bank only): one bank slot / name / None per batch row, written to the state's row table first
        (a prefill call's new state starts with every row at -1; later calls keep what `set_row_adapters` wrote).
        `prefix` = (entry, P) of a prefix.PrefixCache (B = 1 prefill calls only): the new state's columns [0, P) are restored from
        the entry and the call computes the last S - P ids at offset P; the captured short-prompt prefill is bypassed.

        Returns (logits bf16 [B, L', V], cache).  On a prefill call (cache is None)
        only the last position is projected through lm_head (L' = 1) unless
        `full_logits=True`: every caller in the reference reads `logits[:, -1]`
        of a prefill only; cached calls return all L rows."""
        cfg, w = self.cfg, self.w
        if torch.is_tensor(input_ids):
            ids = input_ids.to(self.device, I32)
        else:
            ids = torch.as_tensor(np.asarray(input_ids).astype(np.int32)).to(self.device)
        if ids.dim() == 1:
            ids = ids[None]
        ids = ids.contiguous()
        B, L = ids.shape
        H = cfg.hidden_size
        prefill = cache is None
        if prefix is not None:
            if not prefill or B != 1 or pids is not None or mask is not None or n_beam != 1:
                raise ValueError("prefix: B = 1 prefill calls without padding only")
            ids_h = np.asarray(input_ids.cpu() if torch.is_tensor(input_ids) else input_ids).reshape(1, -1)
            P, kw = self._prefix_split(ids_h, prefix, dict(pixel_values=pixel_values, image_sizes=image_sizes, positions=positions))
            pixel_values, image_sizes, positions = kw.get("pixel_values"), kw.get("image_sizes"), kw.get("positions")
            st = self._new_state(1, L, max_tokens, None, None, extra_tokens=extra_tokens)
            cache = [LayerCache(st, i) for i in range(cfg.num_hidden_layers)]
            self._restore_prefix(st, 0, 0, prefix[0], P)
            st.offset, ids, L = P, ids[:, P:].contiguous(), L - P
        elif prefill and pixel_values is None and B == 1 and pids is None and mask is None and n_beam == 1 and not full_logits \
                and advance_offset is None and not extra_tokens:
            got = self._prefill_captured(ids, L, max_tokens)
            if got is not None:
                return got
        if prefill and prefix is None:
            # (before the vision tower is enqueued: the host is launch-bound through the ViT's ~280 launches, so whatever it does between
            #  the tower and the decoder -- cache allocation, its zero fill, the rotation tables -- would show as idle GPU time there)
            st = self._new_state(B, L, max_tokens, pids, mask, extra_tokens=extra_tokens)
            cache = [LayerCache(st, i) for i in range(cfg.num_hidden_layers)]
        else:
            st = cache[0].state
        if row_adapters is not None:
            self.set_row_adapters(st, row_adapters)
        x = ops.embed_gather(ids.view(-1), w["model.embed_tokens.weight"])
        if pixel_values is not None and self.vision:
            self.vision_embed(x, pixel_values, image_sizes, positions, L)
        past = st.offset
        if n_beam == 1 and past + L > st.T:
            raise ValueError(f"KV cache overflow: {past}+{L} > {st.T} (prompt + max_tokens)")
        if full_logits is None:
            full_logits = not prefill
        x = self._layers(x, st, B, L, past, n_beam, last_only=not full_logits)
        if n_beam == 1:
            st.offset = past + L                                 # KVCache.__call__ auto-advance (phi.py:544-547)
        if advance_offset is not None:
            st.offset = past + advance_offset                    # phi.py:589-591
        if not full_logits and x.shape[0] != B:
            x = x.view(B, L, H)[:, -1, :].contiguous()
        logits = self._proj(x, "lm_head.weight", norm_w=w["model.norm.weight"])
        return logits.view(B, -1, cfg.vocab_size), cache

    @_on_device
    def embed(self, input_ids, pixel_values=None, image_sizes=None, positions=None, pids=None, mask=None, pooling="last",
              normalize=True, row_adapters=None):
        """The prompt as a vector: a prefill that ends in p3v_embed_pool (include/p3v.h) instead of lm_head -> fp32 [B, H] on the
        device.  pooling="last": the final-normed hidden state of the last position (the final layer builds one row per prompt,
        as generate's prefill does); "mean": its mean over the live positions, the left-pad counts taken from `mask`.
        normalize: divided by its L2 norm.  The KV state is the call's own (max_tokens = 0) and is dropped on return; the captured
        short-prompt prefill is bypassed, as full_logits bypasses it.  `row_adapters` as in __call__."""
        cfg, w = self.cfg, self.w
        if pooling not in ops.POOLING:
            raise ValueError(f"pooling must be 'last' or 'mean', got {pooling!r}")
        if torch.is_tensor(input_ids):
            ids = input_ids.to(self.device, I32)
        else:
            ids = torch.as_tensor(np.asarray(input_ids).astype(np.int32)).to(self.device)
        if ids.dim() == 1:
            ids = ids[None]
        ids = ids.contiguous()
        B, L = ids.shape
        st = self._new_state(B, L, 0, pids, mask)
        if row_adapters is not None:
            self.set_row_adapters(st, row_adapters)
        x = ops.embed_gather(ids.view(-1), w["model.embed_tokens.weight"])
        if pixel_values is not None and self.vision:
            self.vision_embed(x, pixel_values, image_sizes, positions, L)
        last = pooling == "last"
        x = self._layers(x, st, B, L, 0, 1, last_only=last)
        start = None
        if not last and mask is not None:
            pad = (np.asarray(mask.cpu() if torch.is_tensor(mask) else mask).reshape(B, L) == 0).sum(1)
            start = torch.as_tensor(pad.astype(np.int32)).to(self.device)
        return ops.embed_pool(x.view(B, -1, cfg.hidden_size), w["model.norm.weight"], cfg.rms_norm_eps, start, pooling, normalize)

    # ------------------------------------------------------------------ captured prefill of short text prompts
    PREFILL_GRAPH_MAX_S = 512
    PREFILL_GRAPH_ENTRIES = 4
    PREFILL_GRAPH_MAX_CACHE_BYTES = 2 << 30                       # an entry pins its (S + max_tokens) KV cache: 393 KB per token at full size

    def _prefill_captured(self, ids, S, max_tokens):
        """Short text prompts (B = 1, 17 .. 512 tokens) are launch-bound: ~390 launches of a few microseconds each, every one paid
        for in Python + ctypes time (BASELINE config 1: 4.5 ms of wall time for 3.6 ms of kernels).  A (length, max_tokens) pair seen
        for the SECOND time is captured as ONE hipGraph over buffers the entry owns -- ids, activations, rotation tables, the KV
        cache itself -- and later prompts of that geometry cost one 0.5 KB copy + one graph launch.  The entry's cache is LEASED to
        the caller: every call gets its own CacheState object (a shallow copy of the entry's: same tensors, same decode graphs, its
        own offset) and the lease IS that object -- while it is alive, through the returned cache list or through a kept
        `cache[i].state`, a new prompt of the same geometry takes the eager path, so a caller that keeps two caches gets two caches
        (the reference's contract).  An entry whose caller died in an unrecovered failed step is dropped (`CacheState.mark_dirty`),
        and entries whose cache would exceed PREFILL_GRAPH_MAX_CACHE_BYTES are not made.  Bit-identical to the eager path (same
        kernels, same order).  P3V_PREFILL_GRAPH=0 switches it off.  Returns None when not applicable."""
        cfg = self.cfg
        if (os.environ.get("P3V_PREFILL_GRAPH", "1") == "0" or S <= ops.L.DECODE_MAX_L or S > self.PREFILL_GRAPH_MAX_S or max_tokens < 1
                or getattr(cfg, "use_quantized_cache", False) or self.adapters or self._bank or self.hidden_hook is not None or self.w8):
            return None                                           # (4-bit weights are captured too, round 6: their prefill is the bf16 one + a
                                                                  #  dequantise launch per projection into the model's own scratch)
        if 4 * cfg.num_hidden_layers * cfg.num_key_value_heads * self.hd * (S + max_tokens + 256) > self.PREFILL_GRAPH_MAX_CACHE_BYTES:
            return None
        # the graph bakes in the rotation tables and the weight pointers: both are part of the key (tests mutate `cfg` and swap weight
        # tensors on a live model; in-place weight updates are seen by the graph as they are by every launch)
        nl = cfg.num_hidden_layers - 1
        def wptr(k):
            w, fmt = self._handle(k)
            return (w if fmt == "bf16" else w[0]).data_ptr()
        key = (S, max_tokens, rope_scaling_factor(cfg), float(cfg.rope_theta), cfg.original_max_position_embeddings,
               self.w["model.embed_tokens.weight"].data_ptr(), wptr("lm_head.weight"),
               wptr("model.layers.0.self_attn.qkv_proj.weight"), wptr(f"model.layers.{nl}.mlp.down_proj.weight"))
        e = self._prefill_graphs.get(key)
        if e is None:
            if self._prefill_seen.get(key, 0) < 1:                # first sighting: eager (one-off lengths never pay for a capture)
                if len(self._prefill_seen) > 64:
                    self._prefill_seen.clear()
                self._prefill_seen[key] = 1
                return None
            if len(self._prefill_graphs) >= self.PREFILL_GRAPH_ENTRIES:
                self._prefill_graphs.pop(next(iter(self._prefill_graphs)))
            e = self._prefill_graphs[key] = self._build_prefill_graph(S, max_tokens)
        if e["lease"] is not None and e["lease"]() is not None:    # the previous caller still holds this entry's cache
            return None
        if e["st"].shared["dirty"]:                               # its last caller died in a failed step: NaN rows, half-armed buffers
            del self._prefill_graphs[key]
            self._prefill_seen[key] = 1                           # (the next prompt of this geometry captures afresh)
            return None
        st = copy.copy(e["st"])                                   # this call's state: the entry's tensors and graphs, its own offset
        self._states.add(st)
        e["ids"].copy_(ids.view(-1), non_blocking=True)
        st.offset = 0
        g = st.graphs.get("greedy")
        if g is not None:                                         # the decode graph of this cache geometry stays valid: same buffers
            self._reset_replays(g)
        e["graph"].launch()
        st.offset = S
        e["lease"] = weakref.ref(st)
        return e["logits"].clone().view(1, 1, cfg.vocab_size), [LayerCache(st, i) for i in range(cfg.num_hidden_layers)]

    def _build_prefill_graph(self, S, max_tokens):
        cfg, w, dev = self.cfg, self.w, self.device
        st = self._new_state(1, S, max_tokens, None, None)
        e = dict(st=st, lease=None, ids=torch.zeros((S,), dtype=I32, device=dev), x=torch.empty((S, cfg.hidden_size), dtype=BF16, device=dev),
                 logits=torch.empty((1, cfg.vocab_size), dtype=BF16, device=dev), bufs=self._alloc_bufs(1, S), ws={})

        def run():
            st.offset = 0
            ops.embed_gather(e["ids"], w["model.embed_tokens.weight"], out=e["x"])
            xl = self._layers(e["x"], st, 1, S, 0, 1, bufs=e["bufs"], last_only=True)
            self._proj(xl.view(1, -1), "lm_head.weight", norm_w=w["model.norm.weight"], out=e["logits"])
        e["graph"] = self._capture(run, e["ws"])
        return e

    @property
    def layers(self):
        return range(self.cfg.num_hidden_layers)
