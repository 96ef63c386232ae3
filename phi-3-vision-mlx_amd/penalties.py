"""Host side of the repetition / presence / frequency penalties and logit_bias: argument checking, the per-row records of
p3v_penalize, and a plain NumPy restatement of the rule.

The rule itself is written out in include/p3v.h above `p3v_penalty_row_t`; the device kernels in csrc/p3v_penalty.hip implement
it.  Here the public arguments -- each penalty a scalar or a per-row list, `logit_bias` one {token id: bias} mapping for every
row or a per-row list of mappings / None -- become one (repetition, frequency, presence, bias) tuple per row:

  * repetition_penalty 1, presence_penalty 0, frequency_penalty 0 and no logit_bias leave a row INACTIVE: its logits pass
    through bit for bit, and a call whose rows are all inactive keeps today's path (`off`);
  * a logit_bias key is an int, or the decimal string JSON sends; a value of -inf bans the token.

Every step of the rule is one correctly rounded fp32 operation, so `reference_adjust` -- NumPy in float32 -- gives the bits the
kernel gives (NaNs compare as "is NaN").
"""
import math
import numbers

import numpy as np
import torch

from . import _lib as L
from .sampling import _number, _per_row

RECORD_WORDS = L.PENALTY_WORDS        # sizeof(p3v_penalty_row_t) / 4
C_SIZE = RECORD_WORDS * 4
ACTIVE, BIAS = L.PENALTY_ACTIVE, L.PENALTY_BIAS
PROMPT_BIT = 0x80000000               # seen: the token occurs in the prompt
COUNT_MASK = 0x7FFFFFFF               # seen: how often the row has emitted the token
INACTIVE = (1.0, 0.0, 0.0, None)      # (repetition, frequency, presence, bias)


def _bias_key(k, vocab):
    if isinstance(k, bool) or not isinstance(k, (numbers.Integral, str)):
        raise ValueError(f"logit_bias keys must be token ids (an int, or a decimal string), got {k!r}")
    if isinstance(k, str):
        if not (k.isascii() and k.isdigit()):
            raise ValueError(f"logit_bias keys must be token ids (an int, or a decimal string), got {k!r}")
    k = int(k)
    if k < 0 or (vocab is not None and k >= vocab):
        raise ValueError(f"logit_bias key {k} lies outside the vocabulary [0, {vocab if vocab is not None else 'n'})")
    return k


def _bias(d, vocab):
    """One row's logit_bias -> {int id: float} or None (absent or empty)."""
    if d is None:
        return None
    if not isinstance(d, dict):
        raise ValueError(f"logit_bias must be a mapping of token id to bias, got {type(d).__name__}")
    out = {}
    for k, v in d.items():
        k = _bias_key(k, vocab)
        v = _number(f"logit_bias[{k}]", v)
        if math.isnan(v) or v == math.inf:
            raise ValueError(f"logit_bias[{k}] must be a finite number or -inf, got {v}")
        out[k] = v
    return out or None


def rows(B, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, logit_bias=None, vocab=None):
    """-> [(repetition, frequency, presence, bias)] * B, checked (bias: {id: float} or None); ValueError on a bad value or a
    per-row list of the wrong length.  vocab: the vocabulary size the logit_bias keys must lie below (None: only >= 0)."""
    rps = [_number("repetition_penalty", v) for v in _per_row("repetition_penalty", repetition_penalty, B)]
    pps = [_number("presence_penalty", v) for v in _per_row("presence_penalty", presence_penalty, B)]
    fps = [_number("frequency_penalty", v) for v in _per_row("frequency_penalty", frequency_penalty, B)]
    for v in rps:
        if not math.isfinite(v) or v <= 0:
            raise ValueError(f"repetition_penalty must be finite and > 0, got {v}")
    for name, vs in (("presence_penalty", pps), ("frequency_penalty", fps)):
        for v in vs:
            if not math.isfinite(v):
                raise ValueError(f"{name} must be finite, got {v}")
    if isinstance(logit_bias, (list, tuple)):
        if len(logit_bias) != B:
            raise ValueError(f"logit_bias: {len(logit_bias)} values for {B} rows")
        biases = [_bias(d, vocab) for d in logit_bias]
    else:
        biases = [_bias(logit_bias, vocab)] * B
    return list(zip(rps, fps, pps, biases))


def active(row):
    """Does this row's record change its logits?"""
    rp, fp, pp, bias = row
    return rp != 1.0 or fp != 0.0 or pp != 0.0 or bias is not None


def off(rows_):
    """True when no row is penalised or biased: the caller keeps today's path, launch for launch."""
    return all(not active(r) for r in rows_)


def flags(row):
    return (ACTIVE if active(row) else 0) | (BIAS if row[3] is not None else 0)


def pack(rows_):
    """Host int32 tensor [B, 4] in the p3v_penalty_row_t layout."""
    arr = (L.PenaltyRow * len(rows_))()
    for i, r in enumerate(rows_):
        arr[i] = L.PenaltyRow(r[0], r[1], r[2], flags(r))
    return torch.frombuffer(bytearray(arr), dtype=torch.int32).view(len(rows_), RECORD_WORDS).clone()


def unpack(records):
    """int32 [B, 4] (host or device) -> [{"repetition", "frequency", "presence", "flags"}] (tests, observability)."""
    raw = records.detach().to("cpu").contiguous().numpy().tobytes()
    arr = (L.PenaltyRow * (len(raw) // C_SIZE)).from_buffer_copy(raw)
    return [dict(repetition=r.repetition, frequency=r.frequency, presence=r.presence, flags=r.flags) for r in arr]


def bias_table(rows_, vocab):
    """The rows' biases as fp32 [B, vocab] (zero where a row names nothing), or None when no row has a bias."""
    if all(r[3] is None for r in rows_):
        return None
    t = np.zeros((len(rows_), vocab), dtype=np.float32)
    for b, r in enumerate(rows_):
        for k, v in (r[3] or {}).items():
            t[b, k] = v
    return t


def seen_table(prompt_ids, emitted, vocab):
    """The table p3v_penalty_note builds, on the host: uint32 [vocab] from one row's prompt ids and emitted ids (ids outside
    [0, vocab) are skipped)."""
    seen = np.zeros((vocab,), dtype=np.uint32)
    p = np.asarray(prompt_ids, dtype=np.int64).reshape(-1)
    p = p[(p >= 0) & (p < vocab)]
    seen[p] |= np.uint32(PROMPT_BIT)
    e = np.asarray(emitted, dtype=np.int64).reshape(-1)
    e = e[(e >= 0) & (e < vocab)]
    np.add.at(seen, e, np.uint32(1))
    return seen


def bf16_bits_to_f32(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def f32_to_bf16_bits(a):
    """Round to nearest even; a NaN becomes a quiet NaN."""
    u = np.asarray(a, dtype=np.float32).view(np.uint32)
    rounded = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    return np.where(nan, ((u >> np.uint32(16)) | np.uint32(0x40)).astype(np.uint16), rounded)


def reference_adjust(logits_bf16, record, seen, bias=None):
    """The rule of include/p3v.h on ONE row, in NumPy float32.  logits_bf16: uint16 [n] (the bf16 bits); record: (repetition,
    frequency, presence, flags) or an `unpack` dict; seen: uint32 [n]; bias: fp32 [n] or None.  Returns the adjusted row's
    bf16 bits, uint16 [n]."""
    if isinstance(record, dict):
        record = (record["repetition"], record["frequency"], record["presence"], record["flags"])
    rp, fp, pp = (np.float32(v) for v in record[:3])
    flg = int(record[3])
    bits = np.asarray(logits_bf16, dtype=np.uint16)
    if not flg & ACTIVE:
        return bits.copy()                                                      # 0.
    seen = np.asarray(seen, dtype=np.uint32)
    with np.errstate(all="ignore"):
        a = bf16_bits_to_f32(bits)                                              # 1.
        c = seen & np.uint32(COUNT_MASK)
        s = seen != 0
        if rp != np.float32(1.0):                                               # 2.
            a = np.where(s, np.where(a > 0, a / rp, a * rp), a).astype(np.float32)
        f = (fp * c.astype(np.float32)).astype(np.float32)                      # 3. (rounded on its own)
        a = (a - f).astype(np.float32)
        a = np.where(c > 0, (a - pp).astype(np.float32), a)                     # 4.
        if flg & BIAS and bias is not None:                                     # 5.
            a = (a + np.asarray(bias, dtype=np.float32)).astype(np.float32)
    return f32_to_bf16_bits(a)                                                  # 6.


def refuse_speculation(rows_, speculate):
    if rows_ is not None and speculate and not off(rows_):
        raise ValueError("speculate: penalties and logit_bias are not supported (a verify step scores several tokens per replay "
                         "against one table; speculate must be 0)")


# ---- a request's penalties as one JSON-able dict (engine.penalty_args, the fleet, the server)
FIELDS = ("repetition_penalty", "presence_penalty", "frequency_penalty", "logit_bias")


def request_row(d, vocab=None):
    """One request's {"repetition_penalty", "presence_penalty", "frequency_penalty", "logit_bias"} (missing keys: the defaults)
    -> its checked row tuple, or None when it asks for nothing."""
    if d is None:
        return None
    if not isinstance(d, dict):
        raise ValueError(f"penalties must be a mapping, got {type(d).__name__}")
    unknown = set(d) - set(FIELDS)
    if unknown:
        raise ValueError(f"unknown penalty fields: {sorted(unknown)}")
    d = {k: v for k, v in d.items() if v is not None}           # (a JSON null: the default)
    for k in FIELDS[:3]:
        if isinstance(d.get(k, 0.0), (list, tuple, np.ndarray)):
            raise ValueError(f"{k} must be a number, got {type(d[k]).__name__}")
    if isinstance(d.get("logit_bias"), (list, tuple)):
        raise ValueError("logit_bias must be a mapping of token id to bias, got a list")
    row = rows(1, d.get("repetition_penalty", 1.0), d.get("presence_penalty", 0.0), d.get("frequency_penalty", 0.0),
               d.get("logit_bias"), vocab)[0]
    return row if active(row) else None
