"""Operator layer: torch tensors in, HIP kernels (via the C ABI) underneath.

torch is used for device memory and the current stream only; every function
here launches a hand-written gfx950 kernel from ``csrc/`` and nothing else.
Each op names the MLX call site of the reference it replaces.
"""
import collections
import contextlib
import ctypes as C
import weakref

import numpy as np
import torch

from . import _lib as L
from ._lib import (EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_QGELU, EPI_BIAS_RESID_F32, EPI_F32, EPI_NONE,  # noqa: F401
                   EPI_PATCH, EPI_RESID_BF16, EPI_SILU_MUL)

BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return 0 if t is None else t.data_ptr()


def _chk(t, dtype, name):
    if not t.is_cuda:
        raise RuntimeError(f"{name}: expected a device tensor (the hot path has no CPU fallback)")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous tensor")
    return t


def embed_gather(ids, table, out=None):
    """nn.Embedding (phi.py:577); ids int32 [n], table bf16 [V,H] -> bf16 [n,H]."""
    _chk(ids, I32, "ids"), _chk(table, BF16, "table")
    n, (V, H) = ids.numel(), table.shape
    out = torch.empty((n, H), dtype=BF16, device=table.device) if out is None else out
    L.check(L.lib().p3v_embed_gather(_p(ids), _p(table), _p(out), n, H, V, _stream()), "embed_gather")
    return out


def rmsnorm(x, w, eps, out=None):
    """nn.RMSNorm (phi.py:478-479,571)."""
    _chk(x, BF16, "x"), _chk(w, BF16, "w")
    rows, H = x.numel() // x.shape[-1], x.shape[-1]
    out = torch.empty_like(x) if out is None else out
    L.check(L.lib().p3v_rmsnorm(_p(x), _p(w), _p(out), rows, H, float(eps), _stream()), "rmsnorm")
    return out


def layernorm(x, w, b, eps, out_f32=False, out=None):
    """nn.LayerNorm (phi.py:165,167,212): fp32 rows -> bf16 (or fp32, may be in place)."""
    _chk(x, F32, "x"), _chk(w, BF16, "w"), _chk(b, BF16, "b")
    rows, H = x.numel() // x.shape[-1], x.shape[-1]
    if out is None:
        out = torch.empty(x.shape, dtype=F32 if out_f32 else BF16, device=x.device)
    L.check(L.lib().p3v_layernorm(_p(x), _p(w), _p(b), _p(out), int(out_f32), rows, H, float(eps), _stream()), "layernorm")
    return out


def set_tuning(name, value):
    """Pin a launch-policy knob of the library (include/p3v.h: p3v_set_tuning); returns the previous value."""
    old = C.c_int(0)
    L.check(L.lib().p3v_get_tuning(name.encode(), C.byref(old)), f"get_tuning({name})")
    L.check(L.lib().p3v_set_tuning(name.encode(), int(value)), f"set_tuning({name})")
    return old.value


_gemm_ws = {}     # (device index, stream handle) -> grow-only byte buffer for p3v_gemm's split-K partials


_ws_owner = None     # (holder dict, frozen?) while a hipGraph is being built: the GRAPH owns its split-K workspace


@contextlib.contextmanager
def owned_gemm_workspace(holder, frozen):
    """Route every split-K workspace request inside the block to `holder["buf"]` (a dict the caller keeps alive as long as the
    graph).  frozen=False (the warm-up run): the buffer is allocated / grown as needed.  frozen=True (the capture): no allocation
    may happen under hipStreamBeginCapture, and the pointer is baked into the graph -- a request the warm-up did not size
    raises instead.  (the per-(device, stream) buffer below was first allocated on the capture's side stream,
    i.e. under capture, and a later regrow would have freed what the graph still writes to.)"""
    global _ws_owner
    prev, _ws_owner = _ws_owner, (holder, frozen)
    try:
        yield holder
    finally:
        _ws_owner = prev


def _gemm_workspace(device, nbytes):
    """The library never allocates (include/p3v.h): the caller owns the split-K workspace.  One grow-only torch buffer per
    (device, stream): it is live only between the two launches of one p3v_gemm call, so launches on one stream share it."""
    if _ws_owner is not None:
        holder, frozen = _ws_owner
        buf = holder.get("buf")
        if buf is None or buf.numel() < nbytes:
            if frozen:
                raise RuntimeError(f"split-K workspace of {nbytes} bytes requested under graph capture (warm-up sized "
                                   f"{0 if buf is None else buf.numel()})")
            buf = holder["buf"] = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        return buf
    key = (device.index, _stream())
    buf = _gemm_ws.get(key)
    if buf is None or buf.numel() < nbytes:
        # the old buffer may still be read by launches already queued on this stream: torch's caching allocator keeps
        # freed blocks stream-ordered, so dropping the reference is safe
        buf = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _gemm_ws[key] = buf
    return buf


def gemm(a, w, epilogue=EPI_NONE, bias=None, resid=None, out=None, n_out=None, pos=None, patches_per_img=0, ldo=None):
    """nn.Linear / patch conv: out[M,N] = a[M,K] @ w[N,K]^T (+ epilogue), bf16 MFMA."""
    _chk(a, BF16, "a"), _chk(w, BF16, "w")
    M, K = a.shape
    N = n_out if n_out is not None else (w.shape[0] // 2 if epilogue == EPI_SILU_MUL else w.shape[0])
    if w.shape[1] != K:
        raise ValueError(f"gemm: K mismatch {a.shape} x {w.shape}")
    f32_out = epilogue in (EPI_BIAS_RESID_F32, EPI_PATCH, EPI_F32)
    if out is None:
        out = torch.empty((M, N), dtype=F32 if f32_out else BF16, device=a.device)
    ws_bytes = L.lib().p3v_gemm_ws_bytes(M, N, K, epilogue)
    ws = _gemm_workspace(a.device, ws_bytes) if ws_bytes else None
    args = L.GemmArgs(_p(a), _p(w), _p(out), _p(bias), _p(resid), _p(pos), M, N, K, a.stride(0), w.stride(0),
                      ldo if ldo is not None else N, epilogue, patches_per_img, _p(ws), ws.numel() if ws is not None else 0)
    L.check(L.lib().p3v_gemm(C.byref(args), _stream()), "gemm")
    return out


def gemm_route(M, N, K, epilogue=EPI_NONE, entry=L.GEMM_ENTRY_GEMM, lda=None, ldw=None, has_bias=False, ws_bytes=0, n_heads=0, n_kv=0,
               hd=0, dst_off=0, dst_t=0, cu_count=0):
    """What `gemm` (entry: `gemm_resid_norm`, `gemm_qkv`) launches for this call -> L.GemmRoute: status, the launches in order (kernel,
    name, grid, block, rows), the K slices and the workspace they need (include/p3v.h: p3v_gemm_route).  The gemm_* knobs are the
    library's settings; with `cu_count` given no device is asked."""
    q = L.GemmRouteQuery(entry, M, N, K, K if lda is None else lda, K if ldw is None else ldw, epilogue, int(bool(has_bias)), ws_bytes,
                         n_heads, n_kv, hd, dst_off, dst_t, cu_count)
    r = L.GemmRoute()
    L.check(L.lib().p3v_gemm_route(C.byref(q), C.byref(r)), "gemm_route")
    return r


def gemm_resid_norm(a, w, resid, norm_w, eps, normed, out=None):
    """out = resid + bf16(a @ w^T) and normed = RMSNorm(out) * norm_w from the projection's own launch sequence (the K-slice GEMM +
    ONE reduction launch that also normalises).  Returns False, nothing launched, where the library does not split the shape
    (P3V_ERR_UNSUPPORTED): the caller runs gemm(..., EPI_RESID_BF16) and rmsnorm."""
    _chk(a, BF16, "a"), _chk(w, BF16, "w"), _chk(resid, BF16, "resid"), _chk(norm_w, BF16, "norm_w"), _chk(normed, BF16, "normed")
    M, K = a.shape
    N = w.shape[0]
    if w.shape[1] != K or resid.shape != (M, N) or normed.shape != (M, N) or norm_w.numel() != N:
        raise ValueError(f"gemm_resid_norm: shapes {a.shape} x {w.shape}, resid {resid.shape}, normed {normed.shape}")
    if out is None:
        out = torch.empty((M, N), dtype=BF16, device=a.device)
    ws_bytes = L.lib().p3v_gemm_ws_bytes(M, N, K, EPI_RESID_BF16)
    if not ws_bytes:
        return False
    ws = _gemm_workspace(a.device, ws_bytes)
    args = L.GemmArgs(_p(a), _p(w), _p(out), None, _p(resid), None, M, N, K, a.stride(0), w.stride(0), out.stride(0), EPI_RESID_BF16, 0,
                      _p(ws), ws.numel())
    rc = L.lib().p3v_gemm_resid_norm(C.byref(args), _p(norm_w), float(eps), _p(normed), _stream())
    if rc == L.ERR_UNSUPPORTED:
        return False
    L.check(rc, "gemm_resid_norm")
    return True


GEMV_MAX_M = 16


class PackedB13:
    """A bf16 matrix [rows, K] as exact 13-bit codes (include/p3v.h: p3v_pack_b13): `data` u8 [rows, K * 13 / 8] in the container layout
    of the streaming GEMV, `base` the matrix's exponent base, `silu_pairs` the row pairing it was packed for (gate / up rows of
    EPI_SILU_MUL, or neighbouring rows for every other epilogue); `src` / `version` a weak reference to the tensor it was made from and
    that tensor's in-place modification count then (`current` says whether the copy still stands for a given tensor)."""
    __slots__ = ("data", "base", "rows", "K", "silu_pairs", "src", "version")

    def __init__(self, data, base, rows, K, silu_pairs, src=None):
        self.data, self.base, self.rows, self.K, self.silu_pairs = data, int(base), int(rows), int(K), bool(silu_pairs)
        self.src, self.version = (weakref.ref(src) if src is not None else None), (src._version if src is not None else 0)

    def current(self, w):
        return w is not None and self.src is not None and w is self.src() and w._version == self.version


# One record per weight format, for the GEMV wrappers: `shape` handle -> (rows, K); `tensors` handle -> what the struct points at, in
# field order; `checks` (index into tensors, _chk name, dtype) for a handle nobody has looked at yet; `struct` the argument struct;
# `entry` the plain symbol (entry + "_step" carries a decode step's head or tail); `tail` handle -> the fields behind `epilogue`.
_WeightFormat = collections.namedtuple("_WeightFormat", "name shape tensors checks struct entry tail", defaults=(lambda w: (),))
_BF16 = _WeightFormat("bf16", lambda w: tuple(w.shape), lambda w: (w,), ((0, "w", BF16),), L.GemvArgs, "p3v_gemv")
_FP8 = _WeightFormat("fp8", lambda w: tuple(w[0].shape), lambda w: w, ((0, "w8", torch.uint8), (1, "w_scale", F32)), L.GemvF8Args, "p3v_gemv_fp8")
# (a pair is 4-bit BECAUSE its first tensor is int32: `_weight_format` has read that dtype, gemv_q4 checks it under its own name)
_Q4 = _WeightFormat("q4", lambda w: (w[0].shape[0], w[0].shape[1] * 8), lambda w: w, ((1, "sb", I32),), L.GemvQ4Args, "p3v_gemv_q4")
_B13 = _WeightFormat("b13", lambda w: (w.rows, w.K), lambda w: (w.data,), (), L.GemvB13Args, "p3v_gemv_b13",
                     lambda w: (w.base, int(w.silu_pairs)))


def _weight_format(w):
    """The format of a weight HANDLE: the one value that stands for a decoder matrix wherever one is streamed -- what
    `gemv_step_begin` / `gemv_step_end` take as `w`, what Phi3VModel's `w` / `w8` / `w4` / `w13` dicts hold and its `_weight` returns:
        bf16 tensor [N, K]                                          "bf16"   gemv      p3v_gemv[_step]
        (u8 e4m3 [N, K], f32 row scales [N])                        "fp8"    gemv_fp8  p3v_gemv_fp8[_step]
        (i32 nibbles [N, K / 8], i32 scale | bias words [N, K / 64])  "q4"     gemv_q4   p3v_gemv_q4[_step]
        PackedB13 (exact 13-bit codes of a bf16 matrix)             "b13"    gemv_b13  p3v_gemv_b13[_step]
    This is the only place that tells the formats apart by what a value looks like: `weight_shape` and `_gemv_launch` work
    from its record (Phi3VModel knows the name from the dict it keeps the handle in: `_handle`)."""
    t = type(w)
    if t is tuple:
        return _Q4 if w[0].dtype is I32 else _FP8
    return _B13 if t is PackedB13 else _BF16


def weight_shape(w):
    """(rows, K) of a weight handle (`_weight_format`): the matrix it stands for, whatever its storage (4-bit: K = 8 x columns)."""
    return _weight_format(w).shape(w)


def _gemv_launch(what, f, w, x, M, epilogue, resid, norm_w, norm_eps, out, step=None):
    """The one GEMV launch: handle `w` of format `f`, `x` [M, K] (None: the step's prologue gathers it), optional fused RMSNorm /
    epilogue, and with `step` (a GemvStep) the entry that carries the decode step's head or tail.  Allocates `out` for a plain
    call that gave none.  Returns (the library's code, out)."""
    rows, K = f.shape(w)
    tensors = f.tensors(w)
    for i, name, dtype in f.checks:
        _chk(tensors[i], dtype, name)
    if x is not None:
        if f is _B13 and x.shape[1] != K:
            raise ValueError(f"{what}: x has {x.shape[1]} columns, the packed matrix {K}")
        K = x.shape[1]
    N = rows // 2 if epilogue == EPI_SILU_MUL else rows
    if out is None and step is None:
        out = torch.empty((M, N), dtype=F32 if epilogue == EPI_F32 else BF16, device=x.device)
    args = f.struct(_p(x), *map(_p, tensors), _p(out), _p(resid), _p(norm_w), float(norm_eps), M, N, K, epilogue, *f.tail(w))
    if step is None:
        return getattr(L.lib(), f.entry)(C.byref(args), _stream()), out
    return getattr(L.lib(), f.entry + "_step")(C.byref(args), C.byref(step), _stream()), out


def gemv(x, w, epilogue=EPI_NONE, resid=None, norm_w=None, norm_eps=0.0, out=None):
    """Skinny nn.Linear for decode (M<=16) with optional fused RMSNorm / epilogue."""
    _chk(x, BF16, "x")
    rc, out = _gemv_launch("gemv", _BF16, w, x, x.shape[0], epilogue, resid, norm_w, norm_eps, out)
    L.check(rc, "gemv")
    return out


def gemv_route(M, N, K, epilogue=EPI_NONE, fmt="bf16", step=L.GEMV_STEP_NONE, has_norm=False, has_resid=True, exp_base=0, cu_count=0):
    """What `gemv` / `gemv_fp8` / `gemv_q4` / `gemv_b13` (fmt: a `_weight_format` name) or, with `step`, `gemv_step_begin` /
    `gemv_step_end` launch for this call -> L.GemvRoute: status, kernel and its instantiation, name, grid, block, LDS, the streaming
    plan (include/p3v.h: p3v_gemv_route).  The gemv* knobs are the library's settings; with `cu_count` given no device is asked."""
    q = L.GemvRouteQuery(("bf16", "fp8", "q4", "b13").index(fmt), step, M, N, K, epilogue, int(bool(has_norm)), int(bool(has_resid)),
                         exp_base, cu_count)
    r = L.GemvRoute()
    L.check(L.lib().p3v_gemv_route(C.byref(q), C.byref(r)), "gemv_route")
    return r


def resample_u8(src, out_len, axis, coeffs, bounds):
    """One pass of Pillow's 8-bit bilinear resample (phi.py:301) along `axis` (0 = rows, 1 = columns) of a uint8 image
    [H, W, C]; coeffs [out_len, ksize] int32, bounds [out_len, 2] int32 (processor.pil_bilinear_coeffs)."""
    _chk(src, torch.uint8, "src"), _chk(coeffs, I32, "coeffs"), _chk(bounds, I32, "bounds")
    H, W, Cn = src.shape
    if axis == 1:
        out = torch.empty((H, out_len, Cn), dtype=torch.uint8, device=src.device)
        outer, in_len, inner = H, W, Cn
    else:
        out = torch.empty((out_len, W, Cn), dtype=torch.uint8, device=src.device)
        outer, in_len, inner = 1, H, W * Cn
    L.check(L.lib().p3v_resample_u8(_p(src), _p(out), outer, in_len, out_len, inner, _p(coeffs), _p(bounds), coeffs.shape[1],
                                    _stream()), "resample_u8")
    return out


def hd_preprocess(resized, top, hp, portrait, lut, hw, hi, ww, wi, out):
    """Padded / transposed-back / normalised HD image -> crop slots + global view of `out` [n_slots, 3, 336, 336] f32."""
    _chk(resized, torch.uint8, "resized"), _chk(lut, torch.float64, "lut"), _chk(out, F32, "out")
    L.check(L.lib().p3v_hd_preprocess(_p(resized), resized.shape[0], resized.shape[1], int(top), int(hp), int(bool(portrait)), _p(lut),
                                      _p(hw), _p(hi), _p(ww), _p(wi), _p(out), out.shape[0], _stream()), "hd_preprocess")
    return out


def lora_down(x, lora_a, out=None):
    """t = x @ lora_a  (first half of LoRALinear.__call__, phi.py:131): x [M,K] bf16, lora_a [K,r] f32 -> [M,r] f32."""
    _chk(x, BF16, "x"), _chk(lora_a, F32, "lora_a")
    M, K = x.shape
    r = lora_a.shape[1]
    if out is None:
        out = torch.empty((M, r), dtype=F32, device=x.device)
    L.check(L.lib().p3v_lora_down(_p(x), _p(lora_a), _p(out), M, K, r, _stream()), "lora_down")
    return out


def lora_up(y, t, lora_b, scale, epilogue=EPI_NONE, resid=None, out=None):
    """out = epilogue((y + scale * (t @ lora_b)).astype(bf16))  (phi.py:131-133): y [M,N] bf16 (frozen projection),
    t [M,r] f32, lora_b [r,N] f32.  epilogue: EPI_NONE / EPI_RESID_BF16 / EPI_SILU_MUL (out [M, N/2])."""
    _chk(y, BF16, "y"), _chk(t, F32, "t"), _chk(lora_b, F32, "lora_b")
    M, N = y.shape
    r = lora_b.shape[0]
    if out is None:
        out = torch.empty((M, N // 2 if epilogue == EPI_SILU_MUL else N), dtype=BF16, device=y.device)
    L.check(L.lib().p3v_lora_up(_p(y), _p(t), _p(lora_b), float(scale), epilogue, _p(resid), _p(out), M, N, r, _stream()), "lora_up")
    return out


def lora_slices(K):
    """K slices of the gathered LoRA kernels (P3V_LORA_SLICE_K elements each): t of lora_down_rows is [M, lora_slices(K), r_max]."""
    return -(-int(K) // L.LORA_SLICE_K)


def lora_table(entries, device):
    """Bank table of one projection (p3v_lora_entry_t per bank slot) as an int64 [n_slots, 3] device tensor.  `entries`: per
    slot None (this adapter leaves the projection alone) or (lora_a [K, r] f32, lora_b [r, N] f32, scale), tensors on `device`
    and kept alive by the caller (the table holds their addresses)."""
    rows = []
    for e in entries:
        if e is None:
            rows.append([0, 0, 0])
            continue
        a, b, scale = e
        _chk(a, F32, "lora_a"), _chk(b, F32, "lora_b")
        r = a.shape[1]
        if not (1 <= r <= L.LORA_MAX_RANK) or b.shape[0] != r:
            raise ValueError(f"LoRA rank must be 1..{L.LORA_MAX_RANK} and agree between lora_a and lora_b, got {tuple(a.shape)} x {tuple(b.shape)}")
        word = int(np.array([r], dtype=np.int32).view(np.uint32)[0]) | (int(np.array([scale], dtype=np.float32).view(np.uint32)[0]) << 32)
        rows.append([a.data_ptr(), b.data_ptr(), word if word < (1 << 63) else word - (1 << 64)])
    return torch.tensor(rows, dtype=torch.int64).reshape(-1, 3).to(device)


def lora_down_rows(x, table, row_adapter, r_max, norm_w=None, norm_eps=0.0, out=None):
    """Per-row adapters, first half (include/p3v.h, adapter bank): t[m, s, :rank] = h[m, slice s] @ lora_a[slot(m)] with h = x or,
    with norm_w, RMSNorm(x) * norm_w computed in the launch.  x [M,K] bf16, table from `lora_table`, row_adapter int32 [M]
    (-1 = none) -> t [M, lora_slices(K), r_max] f32 (rows without an adapter are left untouched)."""
    _chk(x, BF16, "x"), _chk(table, torch.int64, "table"), _chk(row_adapter, I32, "row_adapter")
    M, K = x.shape
    if row_adapter.numel() < M:
        raise ValueError(f"row_adapter has {row_adapter.numel()} entries for {M} rows")
    if norm_w is not None:
        _chk(norm_w, BF16, "norm_w")
    if out is None:
        out = torch.empty((M, lora_slices(K), r_max), dtype=F32, device=x.device)
    elif out.numel() < M * lora_slices(K) * r_max:
        raise ValueError("lora_down_rows: `out` is too small")
    L.check(L.lib().p3v_lora_down_rows(_p(x), _p(norm_w), float(norm_eps), _p(table), _p(row_adapter), _p(out), M, K, int(r_max),
                                       table.shape[0], _stream()), "lora_down_rows")
    return out


def lora_up_rows(y, t, table, row_adapter, K, r_max, epilogue=EPI_NONE, resid=None, out=None):
    """Per-row adapters, second half: out = epilogue(bf16(y + scale * (sum_s t[m, s] @ lora_b[slot(m)]))); a row without an
    adapter gets epilogue(y).  y [M,N] bf16 (frozen projection, plain epilogue), t from `lora_down_rows` on the same K / r_max."""
    _chk(y, BF16, "y"), _chk(t, F32, "t"), _chk(table, torch.int64, "table"), _chk(row_adapter, I32, "row_adapter")
    M, N = y.shape
    if row_adapter.numel() < M or t.numel() < M * lora_slices(K) * r_max:
        raise ValueError("lora_up_rows: row_adapter / t too small for y")
    if epilogue == EPI_RESID_BF16:
        _chk(resid, BF16, "resid")
    if out is None:
        out = torch.empty((M, N // 2 if epilogue == EPI_SILU_MUL else N), dtype=BF16, device=y.device)
    L.check(L.lib().p3v_lora_up_rows(_p(y), _p(t), _p(table), _p(row_adapter), epilogue, _p(resid), _p(out), M, N, int(K),
                                     int(r_max), table.shape[0], _stream()), "lora_up_rows")
    return out


def gemv_q4(x, w4, sb, epilogue=EPI_NONE, resid=None, norm_w=None, norm_eps=0.0, out=None):
    """`gemv` on 4-bit group-64 weights (device layout of weights.q4_repack): x [M,K] bf16, w4 [N,K/8] i32, sb [N,K/64] i32.
    M = 1: the streaming GEMV (fused RMSNorm allowed); 2 <= M <= 8: k_gemv8_q4 (fused RMSNorm allowed); 9 <= M <= 16: k_gemm_rows_q4
    (no fused norm)."""
    _chk(x, BF16, "x"), _chk(w4, I32, "w4")
    rc, out = _gemv_launch("gemv_q4", _Q4, (w4, sb), x, x.shape[0], epilogue, resid, norm_w, norm_eps, out)
    L.check(rc, "gemv_q4")
    return out


def dequant_q4(w4, sb, out=None):
    """4-bit group-64 weights -> bf16 [N, K] (scale * q + bias, rounded once)."""
    _chk(w4, I32, "w4"), _chk(sb, I32, "sb")
    N, K = w4.shape[0], w4.shape[1] * 8
    if out is None:
        out = torch.empty((N, K), dtype=BF16, device=w4.device)
    L.check(L.lib().p3v_dequant_q4(_p(w4), _p(sb), _p(out), N, K, _stream()), "dequant_q4")
    return out


def quantize_fp8_rows(w):
    """bf16 [N,K] -> (u8 e4m3fn bit patterns [N,K], fp32 scale [N]); w ~ fp8 * scale.  Load-time weight prep."""
    wf = w.float()
    scale = (wf.abs().amax(dim=1) / 448.0).clamp_min(1e-12)
    w8 = (wf / scale[:, None]).to(torch.float8_e4m3fn).view(torch.uint8).contiguous()
    return w8, scale.contiguous()


def gemv_fp8(x, w8, w_scale, epilogue=EPI_NONE, resid=None, norm_w=None, norm_eps=0.0, out=None):
    """`gemv` on fp8 weights (half the streamed bytes)."""
    _chk(x, BF16, "x")
    rc, out = _gemv_launch("gemv_fp8", _FP8, (w8, w_scale), x, x.shape[0], epilogue, resid, norm_w, norm_eps, out)
    L.check(rc, "gemv_fp8")
    return out


def pack_b13(w, silu_pairs=False):
    """bf16 [rows, K] -> PackedB13, or None when the matrix does not fit the format (a value more than 30 binades below its largest,
    a denormal, Inf or NaN): the caller then keeps the bf16 matrix.  Load-time weight prep: reads the verdict back (one sync)."""
    _chk(w, BF16, "w")
    rows, K = w.shape
    if K not in (3072, 8192) or rows % 2:
        return None
    data = torch.empty((rows, K * 13 // 8), dtype=torch.uint8, device=w.device)
    info = torch.empty(4, dtype=I32, device=w.device)
    L.check(L.lib().p3v_pack_b13(_p(w), rows, K, int(bool(silu_pairs)), _p(data), _p(info), _stream()), "pack_b13")
    status, base = info.tolist()[:2]
    return None if status else PackedB13(data, base, rows, K, silu_pairs, src=w)


def unpack_b13(pk, out=None):
    """PackedB13 -> the bf16 matrix, bit for bit."""
    out = torch.empty((pk.rows, pk.K), dtype=BF16, device=pk.data.device) if out is None else out
    L.check(L.lib().p3v_unpack_b13(_p(pk.data), pk.rows, pk.K, int(pk.silu_pairs), pk.base, _p(out), _stream()), "unpack_b13")
    return out


def gemv_b13(x, pk, epilogue=EPI_NONE, resid=None, norm_w=None, norm_eps=0.0, out=None):
    """`gemv` on 13-bit packed bf16 weights: one row of x, 13/16 of the streamed bytes, the same bits out."""
    _chk(x, BF16, "x")
    rc, out = _gemv_launch("gemv_b13", _B13, pk, x, x.shape[0], epilogue, resid, norm_w, norm_eps, out)
    L.check(rc, "gemv_b13")
    return out


def gemv_b13_plan(N, K, epilogue, n_cu):
    """(row pairs per wave, waves that take rows, row-streaming waves per workgroup, workgroups) of a `gemv_b13` launch at the current
    knobs.  Host arithmetic only (include/p3v.h: p3v_gemv_b13_plan)."""
    out = (C.c_int32 * 4)()
    L.check(L.lib().p3v_gemv_b13_plan(int(N), int(K), int(epilogue), int(n_cu), out), "gemv_b13_plan")
    return tuple(out)


def dequant_fp8(w8, w_scale, out=None):
    """fp8 rows -> bf16 (scratch for the prefill GEMM)."""
    N, K = w8.shape
    out = torch.empty((N, K), dtype=BF16, device=w8.device) if out is None else out
    L.check(L.lib().p3v_dequant_fp8(_p(w8), _p(w_scale), _p(out), N, K, _stream()), "dequant_fp8")
    return out


def quant_fp8_rows(x, norm_w=None, norm_eps=0.0, out=None, scale=None):
    """bf16 rows -> (e4m3 bytes [M, K], fp32 scale [M]), one scale per row = max|h| / 448; with `norm_w` h is the
    RMSNorm of x (the fused activation quantiser of the W8A8 prefill projections)."""
    _chk(x, BF16, "x")
    M, K = x.shape
    out = torch.empty((M, K), dtype=torch.uint8, device=x.device) if out is None else out
    scale = torch.empty((M,), dtype=F32, device=x.device) if scale is None else scale
    L.check(L.lib().p3v_quant_fp8_rows(_p(x), _p(norm_w), float(norm_eps), _p(out), _p(scale), M, K, _stream()), "quant_fp8_rows")
    return out, scale


def gemm_fp8(a8, a_scale, w8, w_scale, epilogue=EPI_NONE, resid=None, out=None):
    """W8A8 nn.Linear on the fp8 matrix cores: out[M,N] = epilogue(a_scale[m] w_scale[n] sum_k a8[m,k] w8[n,k]), bf16 out."""
    _chk(a8, torch.uint8, "a8"), _chk(w8, torch.uint8, "w8"), _chk(a_scale, F32, "a_scale"), _chk(w_scale, F32, "w_scale")
    M, K = a8.shape
    N = w8.shape[0] // 2 if epilogue == EPI_SILU_MUL else w8.shape[0]
    if w8.shape[1] != K:
        raise ValueError(f"gemm_fp8: K mismatch {a8.shape} x {w8.shape}")
    out = torch.empty((M, N), dtype=BF16, device=a8.device) if out is None else out
    args = L.GemmF8Args(_p(a8), _p(a_scale), _p(w8), _p(w_scale), _p(out), _p(resid), M, N, K, a8.stride(0), w8.stride(0), N, epilogue)
    L.check(L.lib().p3v_gemm_fp8(C.byref(args), _stream()), "gemm_fp8")
    return out


def gemm_fp8_ok(M, N_rows, K, epilogue):
    """Shapes p3v_gemm_fp8 takes (N_rows = rows of the weight matrix)."""
    n = N_rows // 2 if epilogue == EPI_SILU_MUL else N_rows
    return K % 128 == 0 and n % (128 if epilogue == EPI_SILU_MUL else 256) == 0 and epilogue in (EPI_NONE, EPI_RESID_BF16, EPI_SILU_MUL)


def linear(x, w, epilogue=EPI_NONE, resid=None, out=None):
    """Dispatch a projection to the weight-streaming GEMV (M<=8) or the MFMA GEMM."""
    if x.shape[0] <= GEMV_MAX_M and x.shape[1] % 512 == 0 or x.shape[0] <= 8 and epilogue in (EPI_NONE, EPI_RESID_BF16, EPI_SILU_MUL, EPI_F32):
        return gemv(x, w, epilogue, resid=resid, out=out)
    return gemm(x, w, epilogue, resid=resid, out=out)


def rope_table(pos, inv_freq, scale):
    """SuRoPE tables (phi.py:494-504): pos [n] f32, inv_freq [half] f32 -> cos, sin [n, half] f32."""
    _chk(pos, F32, "pos"), _chk(inv_freq, F32, "inv_freq")
    n, half = pos.numel(), inv_freq.numel()
    cos = torch.empty((n, half), dtype=F32, device=pos.device)
    sin = torch.empty_like(cos)
    L.check(L.lib().p3v_rope_table(_p(pos), _p(inv_freq), float(scale), _p(cos), _p(sin), n, half, _stream()), "rope_table")
    return cos, sin


def rope_kv_append(qkv, cos_t, sin_t, q_out, k_dst, v_dst, B, Lq, nh, nkv, hd, past, dst_t, dst_off_is_past, tab_t=0,
                   tab_div=1, d_past=None, q_scale=1.0):
    """split + _rotate_half + KVCache append (phi.py:443-452, 542-548).  q_scale: rotated queries are multiplied by it
    before their rounding to bf16 (`attention(..., q_prescaled=True)` then skips the per-score multiply)."""
    L.check(L.lib().p3v_rope_kv_append(_p(qkv), _p(cos_t), _p(sin_t), _p(q_out), _p(k_dst), _p(v_dst), B, Lq, nh, nkv, hd,
                                       int(past), _p(d_past), dst_t, int(dst_off_is_past), tab_t, tab_div, float(q_scale),
                                       _stream()),
            "rope_kv_append")


def gemm_qkv(a, w, cos_t, sin_t, q_out, k_dst, v_dst, B, Lq, nh, nkv, hd, past, dst_t, dst_off_is_past, tab_t=0, tab_div=1,
             q_scale=1.0, bias=None):
    """qkv projection + head split + _rotate_half + KVCache append in the GEMM's own launches (include/p3v.h: p3v_gemm_qkv) ==
    gemm(a, w[, bias]) followed by rope_kv_append(...), bit for bit.  Returns False -- nothing launched -- when the library does not
    take the shape (short prompts, unaligned append offsets, ...): the caller then runs the two calls."""
    _chk(a, BF16, "a"), _chk(w, BF16, "w")
    M, K = a.shape
    g = L.GemmArgs(_p(a), _p(w), 0, _p(bias), 0, 0, M, w.shape[0], K, a.stride(0), w.stride(0), w.shape[0],
                   EPI_BIAS if bias is not None else EPI_NONE, 0, 0, 0)
    sp = L.QkvSplit(_p(cos_t), _p(sin_t), _p(q_out), _p(k_dst), _p(v_dst), B, Lq, nh, nkv, hd, int(past), dst_t, int(dst_off_is_past),
                    tab_t, tab_div, float(q_scale))
    rc = L.lib().p3v_gemm_qkv(C.byref(g), C.byref(sp), _stream())
    if rc == L.ERR_UNSUPPORTED:
        return False
    L.check(rc, "gemm_qkv")
    return True


Q_PRESCALE = 1.4426950408889634          # log2(e): q_scale = Q_PRESCALE * softmax scale for q_prescaled attention


def attention(q, out, B, Lq, nh, nkv, hd, scale, causal, k_new=None, v_new=None, new_t=0, past=0, k_past=None, v_past=None,
              past_t=0, past_div=1, pad_len=None, pad_div=1, d_past=None, ws=None, n_split=0, new_is_cache=False,
              q_prescaled=False):
    """softmax((q*scale) k^T + mask) v (phi.py:454-457 / phi.py:148), mask never materialised.
    K tensors are [B, nkv, t, hd]; V tensors are TRANSPOSED [B, nkv, hd, t] (t = past_t / new_t).
    q_prescaled: q already carries scale * log2(e) (rope_kv_append's q_scale = Q_PRESCALE * scale)."""
    args = L.AttnArgs(_p(q), _p(k_past), _p(v_past), _p(k_new), _p(v_new), _p(out), _p(pad_len), _p(d_past), _p(ws),
                      B, Lq, nh, nkv, hd, int(past), past_t, past_div, new_t, pad_div, int(causal), float(scale), n_split, int(new_is_cache),
                      int(bool(q_prescaled)))
    L.check(L.lib().p3v_attention(C.byref(args), _stream()), "attention")
    return out


def attention_route(B, Lq, nh, nkv, hd, past=0, past_t=0, n_split=0, new_is_cache=False, q_prescaled=False, has_ws=False, attn_old=-1,
                    attn_no_dma=-1, attn_pp=-1, attn_il=-1, attn_il_waves=-1, combine_g=-1):
    """What `attention` launches for this call -> L.AttnPromptRoute: status, kernel and its name, grid, block, dynamic LDS, head_group and
    the merge launch (include/p3v.h: p3v_attention_route).  A negative knob is the library's setting; no device is asked."""
    q = L.AttnPromptQuery(B, Lq, nh, nkv, hd, int(past), past_t, n_split, int(bool(new_is_cache)), int(bool(q_prescaled)), int(bool(has_ws)),
                          attn_old, attn_no_dma, attn_pp, attn_il, attn_il_waves, combine_g)
    r = L.AttnPromptRoute()
    L.check(L.lib().p3v_attention_route(C.byref(q), C.byref(r)), "attention_route")
    return r


def attention_decode_can_fuse_oproj(B, Lq, nh, hd, n_split, cache_t, o_n, merge_in_launch):
    """Does the fused attention + o_proj + residual launch take this shape on this device (include/p3v.h)?"""
    return bool(L.lib().p3v_attention_decode_can_fuse_oproj(B, Lq, nh, hd, n_split, cache_t, o_n, int(bool(merge_in_launch))))


def attention_decode_q8_can_fuse_oproj(B, Lq, nh, hd, n_split, cache_t, o_n, merge_in_launch):
    """Does the fused int8-KV attention + fp8 o_proj + residual launch take this shape on this device (include/p3v.h)?"""
    return bool(L.lib().p3v_attention_decode_q8_can_fuse_oproj(B, Lq, nh, hd, n_split, cache_t, o_n, int(bool(merge_in_launch))))


def attention_decode_route(kv_int8, B, Lq, nh, hd, n_split, cache_t, merge_in_launch, o_proj=L.ATTN_O_NONE, o_n=0, q8_old=-1,
                           attn_fo_map=-1, attn_fo_map_q8=-1, capacity=-1, cu_count=-1):
    """What `attention_decode` (kv_int8: `attention_decode_q8`) launches for this call -> L.AttnRoute: kernel, grid, block, merge form,
    fused-o_proj form (the can_fuse answer) and status (include/p3v.h: p3v_attention_decode_route).  A negative knob is the library's
    setting; with `capacity` and `cu_count` given no device is asked."""
    q = L.AttnRouteQuery(int(bool(kv_int8)), B, Lq, nh, hd, n_split, cache_t, int(bool(merge_in_launch)), o_proj, o_n, q8_old, attn_fo_map,
                         attn_fo_map_q8, capacity, cu_count)
    r = L.AttnRoute()
    L.check(L.lib().p3v_attention_decode_route(C.byref(q), C.byref(r)), "attention_decode_route")
    return r


def attention_decode(qkv, cos_new, sin_new, rope_bstride, k_cache, v_cache, out, B, Lq, nh, nkv, hd, scale, past, cache_t, ws,
                     n_split, pad_len=None, d_past=None, merge_in_launch=False, o_proj_w=None, o_proj_x=None, o_rearm=None,
                     o_proj_sb=None):
    """Fused decode-step attention: head split + RoPE + KV append + split-KV attention + merge.
    cos_new/sin_new: rows of the new positions, row (b, r) at b*rope_bstride + r.
    merge_in_launch: the split partials are merged inside the attention launch (ws: see `attention_ws`).
    o_proj_w / o_proj_x / o_rearm: also the layer's o_proj + residual, x += bf16(W_o . out), in the same launch (`out` must be
    all 0xFF on entry; `o_rearm`, the other layer parity's output buffer, is set to 0xFF): see p3v_attn_decode_args_t.
    o_proj_sb: o_proj_w is then the 4-bit group-64 W4 [o_n, K / 8] (int32) of `gemv_q4` and o_proj_sb its scale | bias words."""
    if o_proj_w is not None:
        if o_proj_sb is not None:
            _chk(o_proj_w, I32, "o_proj_w"), _chk(o_proj_sb, I32, "o_proj_sb")
            if tuple(o_proj_w.shape) != (o_proj_sb.shape[0], nh * hd // 8) or o_proj_sb.shape[1] != nh * hd // 64:
                raise ValueError("fused o_proj (4-bit): o_proj_w is [o_n, K / 8], o_proj_sb [o_n, K / 64]")
        else:
            _chk(o_proj_w, BF16, "o_proj_w")
            if o_proj_w.dim() != 2 or o_proj_w.shape[1] != nh * hd:      # (the kernel reads o_n rows of n_heads * hd bf16)
                raise ValueError(f"fused o_proj: o_proj_w must be [o_n, {nh * hd}], got {tuple(o_proj_w.shape)}")
        _chk(o_proj_x, BF16, "o_proj_x"), _chk(o_rearm, BF16, "o_rearm")
        if out.numel() < nh * hd or o_rearm.numel() < nh * hd:
            raise ValueError("fused o_proj: out and o_rearm are [n_heads * hd] rows")
        if o_proj_x.numel() < o_proj_w.shape[0]:                         # x[0 : o_n] is updated in place
            raise ValueError(f"fused o_proj: o_proj_x holds {o_proj_x.numel()} values, the projection writes {o_proj_w.shape[0]}")
    args = L.AttnDecArgs(_p(qkv), _p(cos_new), _p(sin_new), _p(k_cache), _p(v_cache), _p(out), _p(pad_len), _p(d_past), _p(ws),
                         B, Lq, nh, nkv, hd, int(past), cache_t, rope_bstride, n_split, float(scale), int(bool(merge_in_launch)),
                         _p(o_proj_w), _p(o_proj_x), _p(o_rearm), 0 if o_proj_w is None else o_proj_w.shape[0], _p(o_proj_sb))
    L.check(L.lib().p3v_attention_decode(C.byref(args), _stream()), "attention_decode")
    return out


def attention_family_chunk(cache_t, n_split):
    """Keys per split of the decode attention launchers: the unit in which `attention_decode_family` shares a prefix."""
    return (-(-cache_t // n_split) + 63) & ~63


def attention_decode_family(qkv, cos_new, sin_new, rope_bstride, k_cache, v_cache, out, B, nh, nkv, hd, scale, past, cache_t, ws,
                            n_split, family, family_host=None, pad_len=None, d_past=None, Lq=1, merge_in_launch=False, o_proj_w=None):
    """`attention_decode` for one new token per row, reading the prompt keys of every family of `family` once (include/p3v.h:
    p3v_attention_decode_family).  family: int32 [B, 18] on the device, {lead, share_end, member[16]} per row; family_host: the
    same table on the host (a CPU int32 tensor) for the library to check before it launches, or None.  Lq, merge_in_launch and
    o_proj_w exist to be refused: the library takes Lq == 1, the separate merge launch and no fused o_proj."""
    _chk(family, I32, "family")
    if tuple(family.shape) != (B, L.FAMILY_INTS):
        raise ValueError(f"family table must be [{B}, {L.FAMILY_INTS}], got {tuple(family.shape)}")
    host = None
    if family_host is not None:
        if family_host.is_cuda or family_host.dtype != torch.int32 or not family_host.is_contiguous() or \
                tuple(family_host.shape) != (B, L.FAMILY_INTS):
            raise ValueError(f"family_host must be a contiguous CPU int32 [{B}, {L.FAMILY_INTS}] tensor")
        host = family_host.data_ptr()
    args = L.AttnDecArgs(_p(qkv), _p(cos_new), _p(sin_new), _p(k_cache), _p(v_cache), _p(out), _p(pad_len), _p(d_past), _p(ws),
                         B, Lq, nh, nkv, hd, int(past), cache_t, rope_bstride, n_split, float(scale), int(bool(merge_in_launch)),
                         _p(o_proj_w), None, None, 0, None)
    L.check(L.lib().p3v_attention_decode_family(C.byref(args), _p(family), host, _stream()), "attention_decode_family")
    return out


def kv_quantize(k, vt, k8, v8t, k_scale, v_scale, t0, n_tok):
    """bf16 K [B,nkv,Ts,hd] / V^T [B,nkv,hd,Ts] rows [t0,t0+n) -> offset-binary u8 caches + per-token scales."""
    B, nkv, src_t, hd = k.shape
    L.check(L.lib().p3v_kv_quantize(_p(k), _p(vt), _p(k8), _p(v8t), _p(k_scale), _p(v_scale), B * nkv, hd, src_t,
                                    k8.shape[2], int(t0), int(n_tok), _stream()), "kv_quantize")


def kv_quantize_mlx4(k, vt, k4, v4, k_sb, v_sb, n_tok, qkv=None, cos_t=None, sin_t=None, nh=0, past=0, tab_t=0, tab_div=1):
    """The reference's own prompt-cache format (phi.py:528-540: mx.quantize, group 32, 4 bits): tokens [0, n_tok) of bf16
    K [B,nkv,T,hd] / V^T [B,nkv,hd,T] -> codes [B,nkv,n_tok,hd/32,4] int32 + (scale, bias) [B,nkv,n_tok,hd/32,2] fp32, and the
    cache rows rewritten with the dequantised values.  qkv (+ cos_t / sin_t, nh): quantise the keys from their exact fp32 values,
    recomputed from the projection output (the reference's keys are fp32), instead of the bf16 cache rows."""
    _chk(k, BF16, "k"), _chk(vt, BF16, "vt"), _chk(k4, I32, "k4"), _chk(v4, I32, "v4"), _chk(k_sb, F32, "k_sb"), _chk(v_sb, F32, "v_sb")
    B, nkv, T, hd = k.shape
    if tuple(vt.shape) != (B, nkv, hd, T) or tuple(k4.shape) != (B, nkv, n_tok, hd // 32, 4) or tuple(k_sb.shape) != (B, nkv, n_tok, hd // 32, 2) \
            or k4.shape != v4.shape or k_sb.shape != v_sb.shape:
        raise ValueError("kv_quantize_mlx4: shapes")
    if qkv is not None:
        _chk(qkv, BF16, "qkv"), _chk(cos_t, F32, "cos_t"), _chk(sin_t, F32, "sin_t")
        if tuple(qkv.shape) != (B * n_tok, (nh + 2 * nkv) * hd):
            raise ValueError("kv_quantize_mlx4: qkv must be the projection output of exactly the n_tok tokens being quantised")
    L.check(L.lib().p3v_kv_quantize_mlx4(_p(k), _p(vt), _p(k4), _p(v4), _p(k_sb), _p(v_sb), B * nkv, hd, T, int(n_tok), _p(qkv), _p(cos_t),
                                         _p(sin_t), nh, nkv, int(past), tab_t, tab_div, _stream()), "kv_quantize_mlx4")


def kv_dequantize(k8, v8t, k_scale, v_scale, k, vt, n_tok):
    """offset-binary u8 caches -> bf16 K [B,nkv,Td,hd] / V^T [B,nkv,hd,Td], tokens [0, n_tok)."""
    B, nkv, src_t, hd = k8.shape
    L.check(L.lib().p3v_kv_dequantize(_p(k8), _p(v8t), _p(k_scale), _p(v_scale), _p(k), _p(vt), B * nkv, hd, src_t, k.shape[2],
                                      int(n_tok), _stream()), "kv_dequantize")


def kv_copy(jobs):
    """Prompt prefix cache (p3v_kv_copy): every job moves tokens [t0_src, +n) of batch row b_src of a source cache to tokens
    [t0_dst, +n) of row b_dst of a destination cache, all layers and heads, up to KV_COPY_MAX_JOBS jobs per launch.
    A job is (src, b_src, t0_src, dst, b_dst, t0_dst, n_tok); src / dst are (k, vt) of a bf16 cache -- K [nl,B,nkv,T,hd],
    V^T [nl,B,nkv,hd,T] -- or (k8, v8t, k_scale, v_scale) of an int8 cache (uint8 codes + fp32 [nl,B,nkv,T]).  The two
    sides may differ in B and T only.  Nothing outside the destination runs is written."""
    jobs = list(jobs)
    if not 1 <= len(jobs) <= L.KV_COPY_MAX_JOBS:
        raise ValueError(f"kv_copy: 1..{L.KV_COPY_MAX_JOBS} jobs per launch, got {len(jobs)}")
    recs = (L.KvCopyJob * len(jobs))()
    geom = None
    for rec, (src, b_src, t0_src, dst, b_dst, t0_dst, n_tok) in zip(recs, jobs):
        if len(src) != len(dst) or len(src) not in (2, 4):
            raise ValueError("kv_copy: a cache is (k, vt) or (k8, v8t, k_scale, v_scale), the same kind on both sides")
        dt = src[0].dtype
        if dt not in (BF16, torch.uint8) or (dt == BF16) != (len(src) == 2):
            raise TypeError(f"kv_copy: bf16 (k, vt) or uint8 codes with scales, got {dt} with {len(src)} tensors")
        for side in (src, dst):
            _chk(side[0], dt, "k"), _chk(side[1], dt, "vt")
            nl, B, nkv, T, hd = side[0].shape
            if tuple(side[1].shape) != (nl, B, nkv, hd, T):
                raise ValueError("kv_copy: V^T must be [nl, B, nkv, hd, T] of its K [nl, B, nkv, T, hd]")
            for sc in side[2:]:
                _chk(sc, F32, "scale")
                if tuple(sc.shape) != (nl, B, nkv, T):
                    raise ValueError("kv_copy: scale rows must be [nl, B, nkv, T]")
            g = (nl, nkv, hd, dt)
            if geom is None:
                geom = g
            elif g != geom:
                raise ValueError("kv_copy: every cache of a launch has the same layers, heads, head size and element type")
        rec.k_src, rec.v_src, rec.k_dst, rec.v_dst = _p(src[0]), _p(src[1]), _p(dst[0]), _p(dst[1])
        if len(src) == 4:
            rec.ks_src, rec.vs_src, rec.ks_dst, rec.vs_dst = _p(src[2]), _p(src[3]), _p(dst[2]), _p(dst[3])
        rec.B_src, rec.b_src, rec.T_src, rec.t0_src = src[0].shape[1], int(b_src), src[0].shape[3], int(t0_src)
        rec.B_dst, rec.b_dst, rec.T_dst, rec.t0_dst = dst[0].shape[1], int(b_dst), dst[0].shape[3], int(t0_dst)
        rec.n_tok = int(n_tok)
    nl, nkv, hd, dt = geom
    L.check(L.lib().p3v_kv_copy(recs, len(jobs), nl, nkv, hd, 2 if dt == BF16 else 1, _stream()), "kv_copy")


def _kv_side(side, what):
    """(nl, B, nkv, T, hd, dtype) of one side of a KV move: (k, vt) bf16 or (k8, v8t, k_scale, v_scale)."""
    if len(side) not in (2, 4):
        raise ValueError(f"{what}: a cache is (k, vt) or (k8, v8t, k_scale, v_scale)")
    dt = side[0].dtype
    if dt not in (BF16, torch.uint8) or (dt == BF16) != (len(side) == 2):
        raise TypeError(f"{what}: bf16 (k, vt) or uint8 codes with scales, got {dt} with {len(side)} tensors")
    _chk(side[0], dt, "k"), _chk(side[1], dt, "vt")
    nl, B, nkv, T, hd = side[0].shape
    if tuple(side[1].shape) != (nl, B, nkv, hd, T):
        raise ValueError(f"{what}: V^T must be [nl, B, nkv, hd, T] of its K [nl, B, nkv, T, hd]")
    for sc in side[2:]:
        _chk(sc, F32, "scale")
        if tuple(sc.shape) != (nl, B, nkv, T):
            raise ValueError(f"{what}: scale rows must be [nl, B, nkv, T]")
    return nl, B, nkv, T, hd, dt


def kv_fork(src, b_src, t0_src, dst, b_dst, t0_dst, n_tok):
    """n completions of one prompt (p3v_kv_fork): tokens [t0_src, +n_tok) of batch row b_src of `src` go to tokens
    [t0_dst, +n_tok) of EVERY row in `b_dst` (1..KV_FORK_MAX_DST distinct rows) of `dst`, all layers and heads in one launch;
    each piece of the source is read once.  src / dst as in `kv_copy`; `dst` may be `src` itself (rows of one state, none
    of them b_src).  Equal 16-byte phase of the two runs only: anything else raises (kv_copy takes any phase pair)."""
    b_dst = [int(b) for b in b_dst]
    if not 1 <= len(b_dst) <= L.KV_FORK_MAX_DST:
        raise ValueError(f"kv_fork: 1..{L.KV_FORK_MAX_DST} destination rows per launch, got {len(b_dst)}")
    if len(src) != len(dst):
        raise ValueError("kv_fork: the same kind of cache on both sides")
    nl, B_s, nkv, T_s, hd, dt = _kv_side(src, "kv_fork")
    g = _kv_side(dst, "kv_fork")
    if (g[0], g[2], g[4], g[5]) != (nl, nkv, hd, dt):
        raise ValueError("kv_fork: both caches have the same layers, heads, head size and element type")
    rec = L.KvFork()
    rec.k_src, rec.v_src, rec.k_dst, rec.v_dst = _p(src[0]), _p(src[1]), _p(dst[0]), _p(dst[1])
    if len(src) == 4:
        rec.ks_src, rec.vs_src, rec.ks_dst, rec.vs_dst = _p(src[2]), _p(src[3]), _p(dst[2]), _p(dst[3])
    rec.B_src, rec.b_src, rec.T_src, rec.t0_src = B_s, int(b_src), T_s, int(t0_src)
    rec.B_dst, rec.T_dst, rec.t0_dst, rec.n_tok, rec.n_dst = g[1], g[3], int(t0_dst), int(n_tok), len(b_dst)
    for i, b in enumerate(b_dst):
        rec.b_dst[i] = b
    L.check(L.lib().p3v_kv_fork(rec, nl, nkv, hd, 2 if dt == BF16 else 1, _stream()), "kv_fork")


def attention_decode_q8(qkv, cos_new, sin_new, rope_bstride, k8, v8t, k_scale, v_scale, out, B, Lq, nh, nkv, hd, scale, past,
                        cache_t, ws, n_split, pad_len=None, d_past=None, merge_in_launch=False, o_proj_w8=None, o_proj_scale=None,
                        o_proj_x=None, o_rearm=None):
    """`attention_decode` on the int8 KV cache (merge_in_launch: as there).  o_proj_w8 / o_proj_scale / o_proj_x / o_rearm: also
    the layer's o_proj on e4m3 weights + residual in the same launch (as attention_decode's o_proj_*; see p3v.h)."""
    if o_proj_w8 is not None:
        _chk(o_proj_w8, torch.uint8, "o_proj_w8"), _chk(o_proj_scale, F32, "o_proj_scale"), _chk(o_proj_x, BF16, "o_proj_x"), _chk(o_rearm, BF16, "o_rearm")
        if tuple(o_proj_w8.shape) != (o_proj_scale.numel(), nh * hd) or out.numel() < nh * hd or o_rearm.numel() < nh * hd:
            raise ValueError("fused o_proj (fp8): o_proj_w8 is [o_n, n_heads * hd] with o_n row scales; out and o_rearm are rows")
        if o_proj_x.numel() < o_proj_w8.shape[0]:
            raise ValueError(f"fused o_proj (fp8): o_proj_x holds {o_proj_x.numel()} values, the projection writes {o_proj_w8.shape[0]}")
    args = L.AttnDecQ8Args(_p(qkv), _p(cos_new), _p(sin_new), _p(k8), _p(v8t), _p(k_scale), _p(v_scale), _p(out), _p(pad_len),
                           _p(d_past), _p(ws), B, Lq, nh, nkv, hd, int(past), cache_t, rope_bstride, n_split, float(scale), int(bool(merge_in_launch)),
                           _p(o_proj_w8), _p(o_proj_scale), _p(o_proj_x), _p(o_rearm), 0 if o_proj_w8 is None else o_proj_w8.shape[0])
    L.check(L.lib().p3v_attention_decode_q8(C.byref(args), _stream()), "attention_decode_q8")
    return out


def stage_rope(cos_t, sin_t, cos_out, sin_out, B, Lq, tab_t, past=0, d_past=None):
    """Copy the cos/sin rows of positions [past, past+L) into compact [B, L, half] buffers (graph-replayed decode)."""
    L.check(L.lib().p3v_stage_rope(_p(cos_t), _p(sin_t), int(past), _p(d_past), _p(cos_out), _p(sin_out), B, Lq, tab_t,
                                   cos_t.shape[-1], _stream()), "stage_rope")


def attention_ws_bytes(B, Lq, nh, hd, n_split):
    return int(L.lib().p3v_attention_ws_bytes(B, Lq, nh, hd, n_split))


def attention_ws(B, Lq, nh, hd, n_split, device):
    """The split-partial workspace in the state every decode-attention launch expects and leaves it in: all bytes 0xFF
    (the 'not written yet' sentinel of the in-launch merge, include/p3v.h)."""
    return torch.full((attention_ws_bytes(B, Lq, nh, hd, n_split) // 4,), -1, dtype=torch.int32, device=device).view(F32)


def im2col_patches(pix, patch, kpad, out=None):
    _chk(pix, F32, "pix")
    n, _, S, _ = pix.shape
    if out is None:
        out = torch.empty((n * (S // patch) ** 2, kpad), dtype=BF16, device=pix.device)
    L.check(L.lib().p3v_im2col_patches(_p(pix), _p(out), n, S, patch, kpad, _stream()), "im2col")
    return out


def clip_cls_rows(x, cls, pos):
    n, T, D = x.shape
    L.check(L.lib().p3v_clip_cls_rows(_p(x), _p(cls), _p(pos), n, T, D, _stream()), "clip_cls_rows")


def hd_merge(feats, sub_gn, glb_gn, h, w, grid, C_):
    """Phi3ImageEmbedding reshape/concat (phi.py:403-407) as one gather."""
    _chk(feats, F32, "feats")
    g2 = grid // 2
    n_out = h * g2 * (w * g2 + 1) + 1 + g2 * (g2 + 1)
    out = torch.empty((n_out, 4 * C_), dtype=BF16, device=feats.device)
    L.check(L.lib().p3v_hd_merge(_p(feats), _p(sub_gn), _p(glb_gn), _p(out), h, w, grid, C_, _stream()), "hd_merge")
    return out


def argmax(logits2d, out=None):
    """mx.argmax(logits[:, -1, :]) (phi_3_vision_mlx.py:386): bf16 rows, first max wins."""
    _chk(logits2d, BF16, "logits")
    rows, n = logits2d.shape
    out = torch.empty((rows,), dtype=I32, device=logits2d.device) if out is None else out
    L.check(L.lib().p3v_argmax(_p(logits2d), _p(out), rows, n, n, _stream()), "argmax")
    return out


def log_softmax(x):
    """nn.log_softmax over the last axis: x - bf16(logsumexp(x)), rounded to bf16 (the reference's composite)."""
    _chk(x, BF16, "x")
    n = x.shape[-1]
    y = torch.empty_like(x)
    L.check(L.lib().p3v_log_softmax(_p(x), _p(y), x.numel() // n, n, _stream()), "log_softmax")
    return y


def topk(x2d, k):
    """k largest per row ordered by (-value, index); replaces mx.argpartition (Q9)."""
    _chk(x2d, BF16, "x")
    rows, n = x2d.shape
    out = torch.empty((rows, k), dtype=I32, device=x2d.device)
    L.check(L.lib().p3v_topk(_p(x2d), _p(out), rows, n, k, n, _stream()), "topk")
    return out


POOLING = {"last": L.POOL_LAST, "mean": L.POOL_MEAN}


def embed_pool(x, w, eps, start=None, pooling="last", normalize=True, out=None):
    """Final RMSNorm + pooling + L2 normalisation (include/p3v.h: p3v_embed_pool): x bf16 [B, L, H] before model.norm, w bf16 [H],
    start int32 [B] left-pad counts (None: no padding) -> fp32 [B, H].  "last" reads row L - 1 only."""
    if pooling not in POOLING:
        raise ValueError(f"pooling must be 'last' or 'mean', got {pooling!r}")
    _chk(x, BF16, "x"), _chk(w, BF16, "w")
    if x.dim() != 3 or w.shape != (x.shape[-1],):
        raise ValueError(f"embed_pool: x must be [B, L, H] and w [H], got {tuple(x.shape)} and {tuple(w.shape)}")
    B, Lq, H = x.shape
    if start is None:
        start = torch.zeros((B,), dtype=I32, device=x.device)
    _chk(start, I32, "start")
    if start.shape != (B,):
        raise ValueError(f"embed_pool: start must be [{B}], got {tuple(start.shape)}")
    out = torch.empty((B, H), dtype=F32, device=x.device) if out is None else _chk(out, F32, "out")
    if out.shape != (B, H):
        raise ValueError(f"embed_pool: out must be [{B}, {H}], got {tuple(out.shape)}")
    mode = POOLING[pooling]
    nbytes = L.lib().p3v_embed_pool_ws_bytes(B, Lq, H, mode)
    ws = torch.empty((max(nbytes, 4) // 4,), dtype=F32, device=x.device)
    L.check(L.lib().p3v_embed_pool(_p(x), _p(w), _p(start), _p(out), B, Lq, H, float(eps), mode, int(bool(normalize)), _p(ws),
                                   nbytes, _stream()), "embed_pool")
    return out


def sim_topk_plan(N, Q, k, D):
    """(rows per workgroup, workgroups, rows of one wave's pass) of a `sim_topk` launch.  Host arithmetic only."""
    a, b, c = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    L.check(L.lib().p3v_sim_topk_plan(int(N), int(Q), int(k), int(D), C.byref(a), C.byref(b), C.byref(c)), "sim_topk_plan")
    return a.value, b.value, c.value


def sim_topk(index, queries, k, n=None, out=None):
    """The k best rows of index[:n] (bf16 [>= n, D]) for each of <= 16 bf16 queries [Q, D], by (-score, row): (idx int32 [Q, k],
    score fp32 [Q, k]); fp32 scores, the score matrix never written (include/p3v.h: p3v_sim_topk).  out: an (idx, score) pair."""
    _chk(index, BF16, "index"), _chk(queries, BF16, "queries")
    if index.dim() != 2 or queries.dim() != 2 or index.shape[1] != queries.shape[1]:
        raise ValueError(f"sim_topk: index [N, D] and queries [Q, D], got {tuple(index.shape)} and {tuple(queries.shape)}")
    N = index.shape[0] if n is None else int(n)
    Q, D = queries.shape
    if not 0 <= N <= index.shape[0]:
        raise ValueError(f"sim_topk: n = {N} outside the index's {index.shape[0]} rows")
    if not 1 <= k <= L.SIM_TOPK_MAX:
        raise ValueError(f"sim_topk: k = {k} outside 1..{L.SIM_TOPK_MAX} (P3V_SIM_TOPK_MAX)")
    if not 1 <= Q <= L.SIM_TOPK_MAX_Q:
        raise ValueError(f"sim_topk: {Q} queries, one launch takes 1..{L.SIM_TOPK_MAX_Q}")
    idx, score = out if out is not None else (torch.empty((Q, k), dtype=I32, device=queries.device),
                                              torch.empty((Q, k), dtype=F32, device=queries.device))
    _chk(idx, I32, "idx"), _chk(score, F32, "score")
    if idx.shape != (Q, k) or score.shape != (Q, k):
        raise ValueError(f"sim_topk: idx and score must be [{Q}, {k}]")
    nbytes = L.lib().p3v_sim_topk_ws_bytes(N, Q, k, D)
    ws = torch.empty((max(nbytes, 8) // 8,), dtype=torch.int64, device=queries.device)
    L.check(L.lib().p3v_sim_topk(_p(index), _p(queries), _p(idx), _p(score), N, Q, k, D, _p(ws), nbytes, _stream()), "sim_topk")
    return idx, score


def gemv_step_begin(tok, table, x_out, cos_t, sin_t, d_past, cos_out, sin_out, w, norm_w, norm_eps, out):
    """The step's FIRST projection with `step_begin` in its prologue (include/p3v.h: p3v_gemv_step): out = W . RMSNorm(table[tok]),
    x_out = table[tok], rotation rows of *d_past staged.  False (nothing launched) where the library keeps the separate launch."""
    _chk(table, BF16, "table"), _chk(x_out, BF16, "x_out"), _chk(tok, I32, "tok")
    B, tab_t, half = tok.numel(), cos_t.shape[-2], cos_t.shape[-1]
    st = L.GemvStep(_p(tok), _p(table), table.shape[0], _p(x_out), _p(cos_t), _p(sin_t), _p(cos_out), _p(sin_out), tab_t, half,
                    None, None, None, None, None, None, 0, _p(d_past))
    f = _weight_format(w)
    if f is _B13 and (table.shape[1] != w.K or x_out.shape[-1] != w.K):
        raise ValueError(f"gemv_step_begin: table / x_out rows of {table.shape[1]} / {x_out.shape[-1]} columns, the packed matrix {w.K}")
    rc, _ = _gemv_launch("gemv_step_begin", f, w, None, B, EPI_NONE, None, norm_w, norm_eps, out, step=st)
    if rc == L.ERR_UNSUPPORTED:
        return False
    L.check(rc, "gemv_step(begin)")
    return True


def gemv_step_end(x, w, norm_w, norm_eps, out, next_tok, tok, history, d_step, d_past, ticket, amax_ws):
    """The step's LAST projection (final norm + lm_head) with `step_end` in its epilogue: logits -> out, their arg-max -> next_tok /
    tok / history[:, *d_step], counters bumped -- by the last workgroup to finish.  False where the library keeps the separate launch."""
    _chk(x, BF16, "x"), _chk(out, BF16, "out")
    if amax_ws.numel() * amax_ws.element_size() < L.GEMV_STEP_WS_BYTES:
        raise ValueError("gemv_step_end: amax_ws smaller than P3V_GEMV_STEP_WS_BYTES")
    st = L.GemvStep(None, None, 0, None, None, None, None, None, 0, 0,
                    _p(next_tok), _p(tok), _p(history), _p(d_step), _p(ticket), _p(amax_ws), history.shape[1], _p(d_past))
    rc, _ = _gemv_launch("gemv_step_end", _weight_format(w), w, x, x.shape[0], EPI_NONE, None, norm_w, norm_eps, out, step=st)
    if rc == L.ERR_UNSUPPORTED:
        return False
    L.check(rc, "gemv_step(end)")
    return True


def add_i32(x, delta):
    L.check(L.lib().p3v_add_i32(_p(x), x.numel(), int(delta), _stream()), "add_i32")


def step_begin(tok, table, x_out, cos_t, sin_t, d_past, cos_out, sin_out, zero_buf=None):
    """Head of a replayed greedy step: embedding rows of `tok` + rotation rows of position *d_past (one launch);
    `zero_buf` (int32) is cleared as well (the in-launch producer flags of the step's fused launches)."""
    B, tab_t, half = tok.numel(), cos_t.shape[-2], cos_t.shape[-1]
    L.check(L.lib().p3v_step_begin(_p(tok), _p(table), _p(x_out), _p(cos_t), _p(sin_t), _p(d_past), _p(cos_out), _p(sin_out),
                                   B, table.shape[1], table.shape[0], tab_t, half, _p(zero_buf),
                                   0 if zero_buf is None else zero_buf.numel(), _stream()), "step_begin")


def step_end(logits, next_tok, tok, history, d_step, d_past, ticket):
    """Tail of a replayed greedy step: argmax + history/tok bookkeeping + counters (one launch)."""
    B, n = logits.shape[0], logits.shape[-1]
    L.check(L.lib().p3v_step_end(_p(logits), _p(next_tok), _p(tok), _p(history), _p(d_step), _p(d_past), _p(ticket), B, n,
                                 history.shape[1], _stream()), "step_end")


def _chk_rows(rows_params, B):
    _chk(rows_params, I32, "rows_params")
    if rows_params.shape != (B, 6):                             # p3v_sample_row_t: 24 bytes per row
        raise ValueError(f"rows_params: expected int32 [{B}, 6] records, got {tuple(rows_params.shape)}")


def sample(logits2d, rows_params, out=None):
    """Seeded sampling (include/p3v.h: p3v_sample): one token per bf16 row under that row's record (temperature, top_k, top_p,
    seed, counter); every record's counter advances by one.  Rows may be strided (logits[:, -1, :])."""
    if not logits2d.is_cuda:
        raise RuntimeError("logits: expected a device tensor (the hot path has no CPU fallback)")
    if logits2d.dtype != BF16 or logits2d.dim() != 2 or logits2d.stride(1) != 1:
        raise ValueError("logits: expected bf16 [rows, n] with unit stride along n")
    rows, n = logits2d.shape
    _chk_rows(rows_params, rows)
    out = torch.empty((rows,), dtype=I32, device=logits2d.device) if out is None else out
    L.check(L.lib().p3v_sample(_p(logits2d), logits2d.stride(0), _p(rows_params), _p(out), rows, n, _stream()), "sample")
    return out


def sample_step_end(logits, rows_params, next_tok, tok, history, d_step, d_past, ticket):
    """Tail of a replayed SAMPLED step: `step_end` with the token drawn under each row's record (one launch)."""
    B, n = logits.shape[0], logits.shape[-1]
    _chk_rows(rows_params, B)
    L.check(L.lib().p3v_sample_step_end(_p(logits), _p(rows_params), _p(next_tok), _p(tok), _p(history), _p(d_step), _p(d_past),
                                        _p(ticket), B, n, history.shape[1], _stream()), "sample_step_end")


def _chk_want(want, rows):
    _chk(want, I32, "want")
    if want.shape != (rows,):
        raise ValueError(f"want: expected int32 [{rows}], got {tuple(want.shape)}")


def logprobs(logits2d, token, want, out=None):
    """Token log-probabilities (include/p3v.h: p3v_logprobs): the record of token[r] on bf16 row r with N = want[r] top entries;
    rows with want[r] < 0 are skipped and their `out` rows left alone.  Rows may be strided (logits[:, -1, :]).  Returns the
    records as int32 [rows, 20] on the device (logprobs.unpack reads them)."""
    if not logits2d.is_cuda:
        raise RuntimeError("logits: expected a device tensor (the hot path has no CPU fallback)")
    if logits2d.dtype != BF16 or logits2d.dim() != 2 or logits2d.stride(1) != 1:
        raise ValueError("logits: expected bf16 [rows, n] with unit stride along n")
    rows, n = logits2d.shape
    _chk(token, I32, "token"), _chk_want(want, rows)
    if token.shape != (rows,):
        raise ValueError(f"token: expected int32 [{rows}], got {tuple(token.shape)}")
    if out is None:
        out = torch.zeros((rows, L.LOGPROB_WORDS), dtype=I32, device=logits2d.device)
    elif out.dtype != I32 or out.shape != (rows, L.LOGPROB_WORDS) or not out.is_contiguous():
        raise ValueError(f"out: expected contiguous int32 [{rows}, {L.LOGPROB_WORDS}] records")
    stride = logits2d.stride(0) if rows > 1 else n              # (a one-row tensor's row stride is arbitrary, 0 included: never used)
    L.check(L.lib().p3v_logprobs(_p(logits2d), stride, _p(token), _p(want), _p(out), rows, n, _stream()), "logprobs")
    return out


def logprobs_step(logits, next_tok, want, d_step, records):
    """The launch after a replayed step's tail: row b's record of the token the step emitted -> records[b, *d_step - 1]
    (int32 [B, max_steps, 20], pinned host or device memory) for rows with want[b] >= 0."""
    _chk(logits, BF16, "logits"), _chk(next_tok, I32, "next_tok"), _chk(d_step, I32, "d_step")
    B, n = logits.shape[0], logits.shape[-1]
    _chk_want(want, B)
    if (records.dtype != I32 or records.dim() != 3 or records.shape[0] != B or records.shape[2] != L.LOGPROB_WORDS
            or not records.is_contiguous() or not (records.is_pinned() or records.is_cuda)):
        raise ValueError(f"records: expected contiguous int32 [{B}, max_steps, {L.LOGPROB_WORDS}] in pinned host (or device) memory")
    L.check(L.lib().p3v_logprobs_step(_p(logits), _p(next_tok), _p(want), _p(d_step), _p(records), B, n, records.shape[1],
                                      _stream()), "logprobs_step")


def _rows2d(t, dtype, name, rows=None, n=None):
    """A [rows, n] device view with unit stride along n (rows may be strided) -> its row stride in elements."""
    if not t.is_cuda:
        raise RuntimeError(f"{name}: expected a device tensor (the hot path has no CPU fallback)")
    if t.dtype != dtype or t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f"{name}: expected {dtype} [rows, n] with unit stride along n")
    if (rows is not None and t.shape[0] != rows) or (n is not None and t.shape[1] != n):
        raise ValueError(f"{name}: expected [{rows}, {n}], got {tuple(t.shape)}")
    return t.stride(0) if t.shape[0] > 1 else max(t.shape[1], t.stride(0))   # (a one-row tensor's row stride is arbitrary: never used)


def _chk_i32_vec(t, rows, name):
    _chk(t, I32, name)
    if t.shape != (rows,):
        raise ValueError(f"{name}: expected int32 [{rows}], got {tuple(t.shape)}")


def penalty_note(seen, ids, first, count, as_prompt, clear=False):
    """Build the penalty table from token ids (include/p3v.h: p3v_penalty_note): seen int32 [rows, n] (the uint32 words of the
    rule), ids int32 [rows, m]; row r notes ids[r, first[r] : first[r] + count[r]] -- bit 31 with as_prompt, one count each
    otherwise; ids outside [0, n) are skipped.  clear: the rows are zeroed first.  One scatter launch (two with clear)."""
    rows, n = seen.shape
    s_stride = _rows2d(seen, I32, "seen")
    i_stride = _rows2d(ids, I32, "ids", rows)
    _chk_i32_vec(first, rows, "first"), _chk_i32_vec(count, rows, "count")
    L.check(L.lib().p3v_penalty_note(_p(seen), s_stride, _p(ids), i_stride, _p(first), _p(count), rows, n, int(bool(as_prompt)),
                                     int(bool(clear)), _stream()), "penalty_note")


def penalize(logits2d, rows_params, seen, bias=None, fed=None, out=None):
    """The penalty rule (include/p3v.h: p3v_penalize) on bf16 rows: out[r] = the adjusted row r under record r (int32 [rows, 4],
    penalties.pack), its seen table row (int32 [rows, n]) and, with `bias` (fp32 [rows, n]), its bias row.  fed (int32 [rows]):
    the token each row was fed this step, counted into `seen` before the row is adjusted.  The logits are not written; returns
    `out` (bf16 [rows, n], made when None).  Every operand may have strided rows."""
    rows, n = logits2d.shape
    l_stride = _rows2d(logits2d, BF16, "logits")
    s_stride = _rows2d(seen, I32, "seen", rows, n)
    b_stride = 0 if bias is None else _rows2d(bias, F32, "bias", rows, n)
    _chk(rows_params, I32, "rows_params")
    if rows_params.shape != (rows, L.PENALTY_WORDS):
        raise ValueError(f"rows_params: expected int32 [{rows}, {L.PENALTY_WORDS}] records (penalties.pack), got {tuple(rows_params.shape)}")
    if fed is not None:
        _chk_i32_vec(fed, rows, "fed")
    if out is None:
        out = torch.empty((rows, n), dtype=BF16, device=logits2d.device)
    o_stride = _rows2d(out, BF16, "out", rows, n)
    L.check(L.lib().p3v_penalize(_p(logits2d), l_stride, _p(rows_params), _p(seen), s_stride, _p(bias), b_stride, _p(fed), _p(out),
                                 o_stride, rows, n, _stream()), "penalize")
    return out


def guide_mask(logits2d, rows_state, delta, accept, tok_off, tok_bytes, eos, fed=None, n_bytes=None):
    """The guide rule (include/p3v.h: p3v_guide_mask) IN PLACE on bf16 rows [rows, n] (rows may be strided): row r under its
    record rows_state[r] (int32 [rows, 4]) and its table region delta[r] (int16 [rows, 256, 256]: the uint16 entries) / accept[r]
    (uint8 [rows, 256]); tok_off int32 [>= n + 1] (the uint32 offsets) and tok_bytes uint8: the vocabulary table; fed (int32
    [rows]): the token each row was fed this step, walked before the row is masked.  One launch; returns `logits2d`."""
    rows, n = logits2d.shape
    l_stride = _rows2d(logits2d, BF16, "logits")
    _chk(rows_state, I32, "rows_state"), _chk(delta, torch.int16, "delta"), _chk(accept, torch.uint8, "accept")
    _chk(tok_off, I32, "tok_off"), _chk(tok_bytes, torch.uint8, "tok_bytes")
    if rows_state.shape != (rows, L.GUIDE_WORDS) or delta.shape != (rows, 256, 256) or accept.shape != (rows, 256):
        raise ValueError(f"guide_mask: expected records [{rows}, {L.GUIDE_WORDS}], delta [{rows}, 256, 256] and accept [{rows}, 256], "
                         f"got {tuple(rows_state.shape)}, {tuple(delta.shape)}, {tuple(accept.shape)}")
    if tok_off.dim() != 1 or tok_off.numel() < n + 1 or tok_bytes.dim() != 1 or tok_bytes.numel() < 1:
        raise ValueError(f"guide_mask: the vocabulary table covers {tok_off.numel() - 1} ids, the rows hold {n}")
    n_bytes = tok_bytes.numel() if n_bytes is None else int(n_bytes)
    if not 0 <= n_bytes <= tok_bytes.numel():
        raise ValueError(f"guide_mask: n_bytes {n_bytes} lies outside tok_bytes ({tok_bytes.numel()} bytes)")
    if fed is not None:
        _chk_i32_vec(fed, rows, "fed")
    L.check(L.lib().p3v_guide_mask(_p(logits2d), l_stride, _p(rows_state), _p(delta), _p(accept), _p(tok_off), _p(tok_bytes),
                                   n_bytes, _p(fed), int(eos), rows, n, _stream()), "guide_mask")
    return logits2d


def spec_state(g, n_max, n_min):
    """p3v_spec_state_t over the loop-state buffers of a speculative capture (model._build_spec_graph)."""
    _chk(g["tok"], I32, "tok"), _chk(g["ctx"], I32, "ctx"), _chk(g["ctl"], I32, "ctl"), _chk(g["amax"], I32, "amax")
    if g["ctl"].numel() < L.SPEC_CTL_INTS or g["amax"].numel() < g["tok"].numel():
        raise ValueError("spec_state: ctl / amax too small")
    for k in ("history", "rec"):
        if g[k].dtype != I32 or not g[k].is_contiguous() or not (g[k].is_pinned() or g[k].is_cuda):
            raise ValueError(f"spec_state: {k} must be contiguous int32 in pinned host (or device) memory")
    if g["rec"].shape[-1] != L.SPEC_REC_INTS:
        raise ValueError("spec_state: rec rows hold P3V_SPEC_REC_INTS words")
    return L.SpecState(_p(g["tok"]), _p(g["ctx"]), _p(g["ctl"]), _p(g["amax"]), _p(g["ticket"]), _p(g["history"]), _p(g["rec"]),
                       _p(g["d_step"]), _p(g["d_past"]), g["ctx"].numel(), g["history"].numel(), g["rec"].shape[0], int(n_max), int(n_min))


def spec_begin(tok, table, x_out, cos_t, sin_t, d_past, cos_out, sin_out):
    """Head of a verify step (B = 1): embedding rows of tok[0..L) + rotation rows of positions *d_past + j, one launch."""
    _chk(tok, I32, "tok"), _chk(table, BF16, "table"), _chk(x_out, BF16, "x_out")
    Lq, tab_t, half = tok.numel(), cos_t.shape[-2], cos_t.shape[-1]
    if x_out.shape != (Lq, table.shape[1]) or cos_out.numel() != Lq * half or sin_out.numel() != Lq * half or cos_t.shape[0] != 1:
        raise ValueError("spec_begin: x_out [L, H], cos_out / sin_out [1, L, half], one table row")
    L.check(L.lib().p3v_spec_begin(_p(tok), _p(table), _p(x_out), _p(cos_t), _p(sin_t), _p(d_past), _p(cos_out), _p(sin_out),
                                   Lq, table.shape[1], table.shape[0], tab_t, half, _stream()), "spec_begin")


def spec_end(logits, state):
    """Tail of a verify step: arg-max of the L rows, acceptance, history / record stores, counters, the next proposal."""
    _chk(logits, BF16, "logits")
    Lq, n = logits.shape
    L.check(L.lib().p3v_spec_end(_p(logits), C.byref(state), Lq, n, _stream()), "spec_end")


def ngram_propose(ctx, n, K, n_max, n_min, vocab, draft, n_draft):
    """Prompt-lookup proposal alone: ctx[0..n) -> draft[0 .. n_draft[0]) (speculate.propose on the device)."""
    _chk(ctx, I32, "ctx"), _chk(draft, I32, "draft"), _chk(n_draft, I32, "n_draft")
    if n > ctx.numel() or draft.numel() < K or n_draft.numel() < 1:
        raise ValueError("ngram_propose: n beyond ctx, or draft / n_draft too small")
    L.check(L.lib().p3v_ngram_propose(_p(ctx), int(n), int(K), int(n_max), int(n_min), int(vocab), _p(draft), _p(n_draft), _stream()),
            "ngram_propose")


def beam_state(g):
    """p3v_beam_state_t over the loop-state buffers of a beam capture (model._build_beam_graph): tok / parent [W] int32, cum [W]
    fp32, cand_id int32 / cand_score fp32 [BEAM_MAX * 2 * BEAM_MAX], ticket, d_step, d_past [1] int32 on the device; rec
    [rec_cap, BEAM_REC_INTS] int32 in pinned host (or device) memory."""
    for k in ("tok", "parent", "cand_id", "ticket", "d_step", "d_past"):
        _chk(g[k], I32, k)
    _chk(g["cum"], F32, "cum"), _chk(g["cand_score"], F32, "cand_score")
    W = g["tok"].numel()
    if g["parent"].numel() != W or g["cum"].numel() != W or min(g["cand_id"].numel(), g["cand_score"].numel()) < 2 * L.BEAM_MAX * L.BEAM_MAX:
        raise ValueError("beam_state: tok / parent / cum hold W words, cand_id / cand_score 128")
    rec = g["rec"]
    if rec.dtype != I32 or not rec.is_contiguous() or not (rec.is_pinned() or rec.is_cuda) or rec.dim() != 2 or rec.shape[1] != L.BEAM_REC_INTS:
        raise ValueError("beam_state: rec must be contiguous int32 [rec_cap, P3V_BEAM_REC_INTS] in pinned host (or device) memory")
    return L.BeamState(_p(g["tok"]), _p(g["parent"]), _p(g["cum"]), _p(g["cand_id"]), _p(g["cand_score"]), _p(g["ticket"]), _p(rec),
                       _p(g["d_step"]), _p(g["d_past"]), rec.shape[0])


def beam_end(logits, state, W, eos):
    """Tail of a beam step (p3v_beam_end): logits [R, n] bf16, R = 1 (the prefill row) or W -> the next beams, the record, the
    counters.  Raises for what the library refuses."""
    _chk(logits, BF16, "logits")
    R, n = logits.shape
    L.check(L.lib().p3v_beam_end(_p(logits), C.byref(state), R, int(W), n, int(eos), _stream()), "beam_end")


def kv_permute_stage(cache, W, stage_cols):
    """Staging buffers of `kv_permute` for a bf16 cache (k, vt): [nl, W, nkv, stage_cols, hd] and [nl, W, nkv, hd, stage_cols]."""
    nl, _, nkv, _, hd, dt = _kv_side(cache, "kv_permute")
    return (torch.empty(nl, W, nkv, stage_cols, hd, dtype=dt, device=cache[0].device),
            torch.empty(nl, W, nkv, hd, stage_cols, dtype=dt, device=cache[0].device))


def kv_permute(cache, parent, W, c0a, d_past, stage, phase):
    """One launch of the beam reorder (p3v_kv_permute): phase 0 gathers the window [c0a, ceil8(*d_past)) of row parent[k] into
    stage[k], phase 1 scatters stage[k] into row k, for every k < W with parent[k] != k.  bf16 caches only: the int8 cache
    raises (P3V_ERR_UNSUPPORTED), as everything else the library refuses."""
    nl, B, nkv, T, hd, dt = _kv_side(cache, "kv_permute")
    _chk(parent, I32, "parent"), _chk(d_past, I32, "d_past")
    if parent.numel() < W or d_past.numel() < 1:
        raise ValueError("kv_permute: parent holds W words, d_past one")
    sk, sv = stage
    _chk(sk, dt, "stage_k"), _chk(sv, dt, "stage_v")
    if sk.dim() != 5 or tuple(sk.shape) != (nl, W, nkv, sk.shape[3], hd) or tuple(sv.shape) != (nl, W, nkv, hd, sk.shape[3]):
        raise ValueError("kv_permute: stage must be [nl, W, nkv, cols, hd] and [nl, W, nkv, hd, cols]")
    L.check(L.lib().p3v_kv_permute(_p(cache[0]), _p(cache[1]), B, T, _p(parent), int(W), int(c0a), _p(d_past), _p(sk), _p(sv),
                                   sk.shape[3], int(phase), nl, nkv, hd, 2 if dt == BF16 else 1, _stream()), "kv_permute")


def store_token(tok, history, d_step, tok_next=None):
    B, max_steps = history.shape
    L.check(L.lib().p3v_store_token(_p(tok), _p(history), _p(d_step), _p(tok_next), B, max_steps, _stream()), "store_token")


class Graph:
    """hipGraph capture/replay of a launch sequence on the current stream."""

    def __init__(self):
        self.exec = C.c_void_p()

    def begin(self):
        L.check(L.lib().p3v_graph_begin(_stream()), "graph_begin")

    def end(self):
        L.check(L.lib().p3v_graph_end(_stream(), C.byref(self.exec)), "graph_end")

    def launch(self):
        L.check(L.lib().p3v_graph_launch(self.exec, _stream()), "graph_launch")

    def __del__(self):
        try:
            if self.exec:
                L.lib().p3v_graph_destroy(self.exec)
        except Exception:
            pass


class Event:
    def __init__(self):
        self.h = C.c_void_p()
        L.check(L.lib().p3v_event_create(C.byref(self.h)), "event_create")

    def record(self):
        L.check(L.lib().p3v_event_record(self.h, _stream()), "event_record")

    def elapsed_ms(self, stop):
        ms = C.c_float()
        L.check(L.lib().p3v_event_elapsed_ms(self.h, stop.h, C.byref(ms)), "event_elapsed")
        return ms.value

    def __del__(self):
        try:
            L.lib().p3v_event_destroy(self.h)
        except Exception:
            pass


def device_props(device=0):
    p = L.Props()
    L.check(L.lib().p3v_device_props(device, C.byref(p)), "device_props")
    return {f: (getattr(p, f).decode() if f == "arch" else getattr(p, f)) for f, _ in L.Props._fields_}
