"""Host side of seeded sampling: argument checking and the per-row records of p3v_sample / p3v_sample_step_end.

The rule itself (temperature, top-k, top-p, Philox draw) is written out in include/p3v.h above `p3v_sample_row_t`; the device
kernels in csrc/p3v_sample.hip implement it.  Here the public arguments -- each a scalar or a per-row list -- become one
(temperature, top_k, top_p, seed) tuple per row:

  * a per-row seed list is used as given; a scalar seed s gives row b the seed s + b (mod 2^64); None draws 64 bits from
    os.urandom for each call (then row b gets that value + b);
  * temperature 0 is greedy: such a row takes the arg-max exactly as p3v_argmax does.
"""
import math
import numbers
import os

import numpy as np
import torch

from . import _lib as L

SEED_MOD = 1 << 64
RECORD_WORDS = 6                      # sizeof(p3v_sample_row_t) / 4
GREEDY = (0.0, 0, 1.0, 0)             # the (temperature, top_k, top_p, seed) of a row that takes the arg-max


def _per_row(name, v, B):
    if isinstance(v, (list, tuple, np.ndarray)):
        v = list(v)
        if len(v) != B:
            raise ValueError(f"{name}: {len(v)} values for {B} rows")
        return v
    return [v] * B


def _number(name, v):
    if isinstance(v, bool) or not isinstance(v, numbers.Real):
        raise ValueError(f"{name} must be a number, got {type(v).__name__}")
    return float(v)


def _integer(name, v):
    if isinstance(v, bool) or not isinstance(v, numbers.Integral):
        raise ValueError(f"{name} must be an integer, got {type(v).__name__}")
    return int(v)


def rows(B, temperature=0.0, top_k=0, top_p=1.0, seed=None):
    """-> [(temperature, top_k, top_p, seed)] * B, checked; ValueError on a bad value or a per-row list of the wrong length."""
    ts = [_number("temperature", t) for t in _per_row("temperature", temperature, B)]
    ks = [_integer("top_k", k) for k in _per_row("top_k", top_k, B)]
    ps = [_number("top_p", p) for p in _per_row("top_p", top_p, B)]
    for t in ts:
        if not math.isfinite(t) or t < 0:
            raise ValueError(f"temperature must be finite and >= 0, got {t}")
    for k in ks:
        if k < 0:
            raise ValueError(f"top_k must be >= 0, got {k}")
    for p in ps:
        if not (0.0 < p <= 1.0):
            raise ValueError(f"top_p must lie in (0, 1], got {p}")
    if isinstance(seed, (list, tuple, np.ndarray)):
        seeds = [_integer("seed", s) for s in _per_row("seed", seed, B)]
    else:
        s = int.from_bytes(os.urandom(8), "little") if seed is None else _integer("seed", seed)
        if not 0 <= s < SEED_MOD:
            raise ValueError(f"seed must lie in [0, 2^64), got {s}")
        seeds = [(s + b) % SEED_MOD for b in range(B)]
    for s in seeds:
        if not 0 <= s < SEED_MOD:
            raise ValueError(f"seed must lie in [0, 2^64), got {s}")
    return list(zip(ts, ks, ps, seeds))


def greedy(rows_):
    """True when every row takes the arg-max (temperature 0): the caller keeps the greedy path."""
    return all(r[0] == 0.0 for r in rows_)


def pack(rows_, counter=0):
    """Host int32 tensor [B, 6] in the p3v_sample_row_t layout (counter: the draw index c of every row's next token)."""
    arr = (L.SampleRow * len(rows_))()
    for i, (t, k, p, s) in enumerate(rows_):
        arr[i] = L.SampleRow(t, k, p, s & 0xFFFFFFFF, s >> 32, int(counter))
    return torch.frombuffer(bytearray(arr), dtype=torch.int32).view(len(rows_), RECORD_WORDS).clone()


def unpack(records):
    """int32 [B, 6] (host or device) -> [{"temperature", "top_k", "top_p", "seed", "counter"}] (tests, observability)."""
    raw = records.detach().to("cpu").contiguous().numpy().tobytes()
    arr = (L.SampleRow * (len(raw) // C_SIZE)).from_buffer_copy(raw)
    return [dict(temperature=r.temperature, top_k=r.top_k, top_p=r.top_p, seed=r.seed_lo | (r.seed_hi << 32), counter=r.counter)
            for r in arr]


C_SIZE = RECORD_WORDS * 4
