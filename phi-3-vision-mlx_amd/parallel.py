"""Host side of n completions per prompt: argument checking and the refusals, in one place for api.py, engine.py and server.py.

The rule (one prefill, KV fork, seeds s + j, best_of ranking) is written out in include/p3v.h above `p3v_kv_fork_t`; the
device copy is csrc/p3v_kv_fork.hip, the ranking is `logprobs.rank_best_of`.  A FAMILY is the m = best_of (default n) rows that
one prompt is forked into; n of them are returned.
"""
import numbers

MAX_N = 16                            # rows of one family: P3V_KV_FORK_MAX_DST destinations + the prefilled row


def _int(name, v):
    if isinstance(v, bool) or not isinstance(v, numbers.Integral):
        raise ValueError(f"{name} must be an integer in 1..{MAX_N}, got {type(v).__name__}")
    return int(v)


def check(n=1, best_of=None):
    """-> (n, m): n completions returned out of m generated (m = best_of, or n without one).  ValueError naming the limit for a
    bool, a float, a string, n outside 1..16 or best_of outside n..16."""
    n = _int("n", 1 if n is None else n)
    if not 1 <= n <= MAX_N:
        raise ValueError(f"n must be an integer in 1..{MAX_N}, got {n}")
    if best_of is None:
        return n, n
    m = _int("best_of", best_of)
    if not n <= m <= MAX_N:
        raise ValueError(f"best_of must be an integer in n..{MAX_N} (n = {n}), got {m}")
    return n, m


def refusal(m, batched=False, speculate=0, mlx4=False, device_step=True, sharded=False):
    """Why a family of m > 1 rows cannot run here, or None.  Each reason names its limit; callers raise it as a ValueError
    before anything runs."""
    if m <= 1:
        return None
    if batched:
        return "n > 1: one prompt (a string) per call; n completions of a list of prompts are not supported"
    if speculate:
        return "n > 1: not under speculative decoding (a verify step is B = 1; speculate must be 0)"
    if mlx4:
        return 'n > 1: not on cache_format="mlx4" (its 4-bit prompt codes are never forked; use the bf16 or the int8 cache)'
    if not device_step:
        return "n > 1 needs the device model's captured step and its KV fork (this model class has none)"
    if sharded:
        return "n > 1: not on the batch-sharded path (dist.generate_sharded runs one row per prompt); call generate per prompt"
    return None


def seeds(seed, m):
    """The seeds of a family's m rows from one concrete seed: (seed + j) mod 2^64, sampling.rows's batch rule."""
    from .sampling import SEED_MOD
    return [(int(seed) + j) % SEED_MOD for j in range(m)]
