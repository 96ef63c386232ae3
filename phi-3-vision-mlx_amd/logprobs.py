"""Host side of token log-probabilities: argument checking and the records of p3v_logprobs / p3v_logprobs_step.

The rule itself (integer-weight log-sum-exp, rank, top-N) is written out in include/p3v.h above `p3v_logprob_t`; the device
kernel in csrc/p3v_logprobs.hip implements it.  Here the public `logprobs` argument -- None (off), an int 0 .. 8, or one such
value per prompt -- becomes the per-row want-table (int32, -1 = off), and the 80-byte records become plain Python values.
"""
import math
import numbers

import numpy as np

from . import _lib as L

MAX = L.LOGPROBS_MAX
RECORD_WORDS = L.LOGPROB_WORDS        # sizeof(p3v_logprob_t) / 4
OFF = -1                              # a want-table row nobody asked about
KEYS = ("token_ids", "token_logprobs", "ranks", "top_logprobs")


def check(v, name="logprobs"):
    """One request's `logprobs` value -> its want-table entry: None -> OFF, an int 0 .. 8 -> itself.  ValueError (naming the
    range) for a bool, a float, a string, a negative value or a value above 8."""
    if v is None:
        return OFF
    if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not 0 <= int(v) <= MAX:
        raise ValueError(f"{name} must be None or an integer in 0..{MAX}, got {v!r}")
    return int(v)


def wants(v, B, name="logprobs"):
    """The public argument of a call over B prompts -> [want] * B, or None when no row asks (the caller keeps today's path)."""
    if isinstance(v, (list, tuple, np.ndarray)):
        v = list(v)
        if len(v) != B:
            raise ValueError(f"{name}: {len(v)} values for {B} rows")
        out = [check(x, name) for x in v]
    else:
        out = [check(v, name)] * B
    return None if all(w == OFF for w in out) else out


def refuse_speculation(wants_, speculate):
    if wants_ is not None and speculate:
        raise ValueError("speculate: logprobs are not supported (a verify step emits several tokens per replay; speculate must be 0)")


def unpack(words):
    """int32 [..., 20] records (NumPy array or tensor, host or device) -> a flat list of dicts: token, logprob, rank, and
    top = [(id, logprob)] * n_top."""
    if hasattr(words, "detach"):
        words = words.detach().to("cpu").contiguous().numpy()
    raw = np.ascontiguousarray(words, dtype=np.int32).reshape(-1, RECORD_WORDS)
    ids, lps = raw[:, 4:4 + MAX], raw[:, 4 + MAX:].view(np.float32)
    head_lp = raw[:, 1].view(np.float32)
    return [dict(token=int(r[0]), logprob=float(head_lp[i]), rank=int(r[2]),
                 top=[(int(ids[i, j]), float(lps[i, j])) for j in range(min(max(int(r[3]), 0), MAX))]) for i, r in enumerate(raw)]   # (a skipped row: whatever the buffer held)


class Collector:
    """Per-row lists of one call's records, in the order the loop hands tokens to its streamer."""

    def __init__(self, wants_):
        self.wants = list(wants_)
        self.rows = [[] for _ in self.wants]

    def add(self, words):
        """One step: int32 [B, 20]; rows whose want is OFF are not read."""
        recs = unpack(words)
        for b, w in enumerate(self.wants):
            if w != OFF:
                self.rows[b].append(recs[b])

    def result(self):
        """{"token_ids": [per prompt], "token_logprobs": .., "ranks": .., "top_logprobs": ..}; None for a prompt that did not ask."""
        return result([rs if w != OFF else None for rs, w in zip(self.rows, self.wants)])


def entry(recs):
    """One prompt's records -> its four aligned lists."""
    return dict(token_ids=[r["token"] for r in recs], token_logprobs=[r["logprob"] for r in recs],
                ranks=[r["rank"] for r in recs], top_logprobs=[list(r["top"]) for r in recs])


def result(per_prompt):
    out = {k: [] for k in KEYS}
    for recs in per_prompt:
        e = None if recs is None else entry(recs)
        for k in KEYS:
            out[k].append(None if e is None else e[k])
    return out


def cumulative(token_ids, token_logprobs, eos_id):
    """One completion's best_of score: the sum of its tokens' RAW-logit log-probabilities through the first `eos_id`
    (included); what follows an EOS is not text and does not count.  None (a completion without records), an empty list,
    a NaN or a -inf entry: -inf."""
    if token_ids is None or token_logprobs is None or len(token_ids) == 0:
        return -math.inf
    ids = list(token_ids)
    stop = ids.index(eos_id) + 1 if eos_id is not None and eos_id in ids else len(ids)
    lps = list(token_logprobs)[:stop]
    if len(lps) < stop or any(x is None or math.isnan(x) for x in lps):
        return -math.inf
    return float(math.fsum(lps))


def rank_best_of(token_ids, token_logprobs, n, eos_id=None):
    """best_of: the indices of the n completions with the largest `cumulative` score, best first; ties go to the lower
    index (a stable sort on the negated score).  token_ids / token_logprobs: one list (or None) per generated completion."""
    scores = [cumulative(i, l, eos_id) for i, l in zip(token_ids, token_logprobs)]
    if not 1 <= n <= len(scores):
        raise ValueError(f"best_of: {n} completions out of {len(scores)}")
    return sorted(range(len(scores)), key=lambda j: -scores[j])[:n]


def finite_or_none(x):
    """JSON has no NaN / Infinity: non-finite values travel as null."""
    return float(x) if x is not None and math.isfinite(x) else None
