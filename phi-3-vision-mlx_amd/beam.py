"""Beam search: the rule of include/p3v.h ("beam search") restated in NumPy and plain Python, and the host side of the loop.

`reference_step` is the selection of one step -- what p3v_beam_end computes, bit for bit (the reorder behind it is a row
gather: torch.index_select on the window states it); `Search` is the host: it reads one record per step, keeps the pool
of finished hypotheses, decides when the search is done and rebuilds the token lists; `check_request` holds the
request-level refusals.  Nothing here imports the HIP library.
"""
import math
import numbers

import numpy as np

MAX = 8                               # P3V_BEAM_MAX
REC_INTS = 2 + 5 * MAX                # P3V_BEAM_REC_INTS
_TOK, _PARENT, _CUM, _FIN_PARENT, _FIN_SCORE = (2 + i * MAX for i in range(5))


def check_width(W, name="num_beams"):
    if isinstance(W, bool) or not isinstance(W, numbers.Integral) or not 2 <= int(W) <= MAX:
        raise ValueError(f"{name} must be 1 (off) or an integer in 2..{MAX}, got {W!r}")
    return int(W)


def check_length_penalty(v, name="length_penalty"):
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v) or v < 0:
        raise ValueError(f"{name} must be a finite number >= 0, got {v!r}")
    return float(v)


def check_request(num_beams, length_penalty=1.0, batched=False, sampled=False, speculate=False, family=False, logprobs=False,
                  penalties=False, guides=False, early_stop=False, adapter=False):
    """The request-level refusals of beam search, before any model call: (W, length_penalty) for W beams, (1, length_penalty)
    for the plain path; a ValueError that names the limit for everything beam search does not run beside."""
    lp = check_length_penalty(length_penalty)
    if not isinstance(num_beams, bool) and isinstance(num_beams, numbers.Integral) and int(num_beams) == 1:
        return 1, lp
    W = check_width(num_beams)
    for on, why in ((batched, "one prompt at a time; a list of prompts is not supported"),
                    (sampled, "deterministic search only (temperature must be 0 and no sampling record set)"),
                    (speculate, "speculate must be 0 (a verify step feeds one sequence)"),
                    (family, "n / best_of are not supported (the beams are the request's rows; the pool is returned through beam_info)"),
                    (logprobs, "logprobs are not supported (beam_info carries every hypothesis' sum_logprob)"),
                    (penalties, "penalties and logit_bias are not supported (the beams are scored on the raw logits)"),
                    (guides, "guided decoding is not supported (guided_regex / guided_choice / guided_json must be None)"),
                    (early_stop, "early_stop is not supported (the search has its own exact end test)"),
                    (adapter, "a per-request adapter is not supported (the B = num_beams step has no row table of its own)")):
        if on:
            raise ValueError(f"num_beams={W}: {why}")
    return W, lp


def bf16_values(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def row_logprobs(bits):
    """Steps 1 - 6 of the logprobs rule for one row of bf16 bit patterns: the fp32 log-probability of every token, or None
    for an UNDEFINED row (a NaN, a +inf, no finite logit)."""
    x = bf16_values(bits)
    if np.isnan(x).any() or np.isposinf(x).any() or not np.isfinite(x).any():
        return None
    m = np.float32(x.max())
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        w = np.floor(np.exp(x.astype(np.float64) - np.float64(m)) * 4294967296.0)      # a -inf logit: 0
        W = int(w.astype(np.uint64).sum())                                                # an exact integer
        lse = np.float64(m) + np.log(np.float64(W)) - 32.0 * 0.6931471805599453094
        return (x.astype(np.float64) - lse).astype(np.float32)


def empty_record():
    return np.full(REC_INTS, -1, dtype=np.int32)


def reference_step(bits, cum_in, W, eos):
    """One selection: bits uint16 [R, n] (bf16 bit patterns), cum_in fp32 [R] -> the record, int32 [REC_INTS]
    {status, n_fin, tok[8], parent[8], cum bits[8], fin_parent[8], fin_score bits[8]}, unused entries -1."""
    bits = np.asarray(bits, dtype=np.uint16)
    cum_in = np.asarray(cum_in, dtype=np.float32)
    R, n = bits.shape
    if not 2 <= W <= MAX or R not in (1, W) or n < 2 * W or cum_in.shape != (R,):
        raise ValueError("reference_step: 2 <= W <= 8, R in {1, W}, n >= 2W, one cum per row")
    rec = empty_record()
    cands = []                                                            # (score, r, place, token)
    for r in range(R):
        lp = row_logprobs(bits[r])
        if lp is None:                                                    # 1. the step fails
            rec[0], rec[1] = 1, 0
            return rec
        x = bf16_values(bits[r])
        order = np.lexsort((np.arange(n), -x))[:2 * W]                    # 2. larger value first, then the lower index
        for place, i in enumerate(order):
            with np.errstate(invalid="ignore"):
                cands.append((np.float32(cum_in[r] + lp[i]), r, place, int(i)))       # ONE fp32 addition
    cands.sort(key=lambda c: (-float(c[0]), c[1], c[2]))                  # 3. (scores are never NaN: cum <= 0, logprob <= 0)
    k = nf = 0
    for j, (score, r, _, token) in enumerate(cands[:2 * W]):              # 4.
        if k == W:
            break
        sbits = int(np.array(score, dtype=np.float32).view(np.int32))
        if token == eos:
            if j < W:
                rec[_FIN_PARENT + nf], rec[_FIN_SCORE + nf] = r, sbits
                nf += 1
            continue
        rec[_TOK + k], rec[_PARENT + k], rec[_CUM + k] = token, r, sbits
        k += 1
    assert k == W
    rec[0], rec[1] = 0, nf
    return rec


def unpack(rec, W):
    """One record (int32 [REC_INTS]) -> dict(status, tok, parent, cum, fin=[(parent, score)])."""
    rec = np.ascontiguousarray(np.asarray(rec, dtype=np.int32).reshape(REC_INTS))
    f = rec.view(np.float32)
    nf = max(0, min(int(rec[1]), MAX))
    return dict(status=int(rec[0]), tok=[int(t) for t in rec[_TOK:_TOK + W]], parent=[int(p) for p in rec[_PARENT:_PARENT + W]],
                cum=[float(c) for c in f[_CUM:_CUM + W]],
                fin=[(int(rec[_FIN_PARENT + i]), float(f[_FIN_SCORE + i])) for i in range(nf)])


class Search:
    """The host of one beam search: feed it record t after step t (`add`), stop when it says so, read `result()`.

    A hypothesis finished at step t has length l = t + 1 and final score sum / l ** length_penalty.  The pool keeps the W
    best: score descending, then the earlier step, then the earlier place in its step.  After a step the search is DONE when
    the pool holds W entries and max_k cum[k] / max_tokens ** length_penalty <= the worst pooled score: cum only falls and
    cum <= 0, so every descendant's score lies at or below that bound, and a tie loses to the earlier step.  At the budget
    (t + 1 == max_tokens) the live beams enter the pool unfinished with l = max_tokens.  Python floats throughout."""

    def __init__(self, W, max_tokens, eos, length_penalty=1.0, prune=True):
        self.W, self.eos, self.prune = check_width(W), int(eos), bool(prune)
        self.lp = check_length_penalty(length_penalty)
        if isinstance(max_tokens, bool) or not isinstance(max_tokens, numbers.Integral) or max_tokens < 1:
            raise ValueError(f"max_tokens must be a positive integer, got {max_tokens!r}")
        self.max_tokens = int(max_tokens)
        self.steps = []                # unpacked records
        self.pool = []                 # (key, entry)
        self.done = False

    def _final(self, s, l):
        return s / float(l) ** self.lp

    def _path(self, t, k):
        """tokens of beam k after step t"""
        out = []
        while t >= 0:
            out.append(self.steps[t]["tok"][k])
            k = self.steps[t]["parent"][k]
            t -= 1
        return out[::-1]

    def _pool_add(self, score, t, j, tokens, s, finished):
        self.pool.append(((-score, t, j), dict(token_ids=tokens, score=score, sum_logprob=s, finished=finished)))
        self.pool.sort(key=lambda e: e[0])
        del self.pool[self.W:]

    def add(self, rec):
        """Record t -> True when the search is done.  RuntimeError for a failed step, as the plain loop raises on a negative token."""
        if self.done:
            raise RuntimeError("beam search: a record after the end")
        r = unpack(rec, self.W) if not isinstance(rec, dict) else rec
        t = len(self.steps)
        if r["status"] != 0 or any(x < 0 for x in r["tok"]):
            raise RuntimeError(f"device step failed: beam step {t} met undefined logits (a NaN, a +inf or no finite value in a row)")
        self.steps.append(r)
        for j, (p, s) in enumerate(r["fin"]):
            head = self._path(t - 1, p) if t > 0 else []
            self._pool_add(self._final(s, t + 1), t, j, head + [self.eos], s, True)
        if t + 1 >= self.max_tokens:
            for k in range(self.W):
                s = r["cum"][k]
                self._pool_add(self._final(s, self.max_tokens), t, MAX + k, self._path(t, k), s, False)
            self.done = True
        elif self.prune and len(self.pool) == self.W:
            self.done = self._final(max(r["cum"]), self.max_tokens) <= self.pool[-1][1]["score"]
        return self.done

    def result(self):
        """The pooled hypotheses, best first."""
        return [e for _, e in self.pool]
