"""Host side of n completions per prompt: argument checking and the refusals, in one place for api.py, engine.py and server.py.

The rule (one prefill, KV fork, seeds s + j, best_of ranking) is written out in include/p3v.h above `p3v_kv_fork_t`; the
device copy is csrc/p3v_kv_fork.hip, the ranking is `logprobs.rank_best_of`.  A FAMILY is the m = best_of (default n) rows that
one prompt is forked into; n of them are returned.
"""
import numbers

import numpy as np

FAMILY_INTS = 2 + 16                  # P3V_FAMILY_INTS: {lead, share_end, member[P3V_FAMILY_MAX]} per row of the family table
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


# ---- shared-prefix decode: the family table of p3v_attention_decode_family (include/p3v.h), as pure functions of host values
def family_table(B, families):
    """The family table for a state of B rows, int32 [B, 18] (numpy): row b = {lead, share_end, member[16]}.  families:
    [(rows, share_end), ...] -- the rows whose caches are identical up to column share_end, the leader (whose copy is read)
    first.  Rows in no family, and families of one row, are single rows {b, 0, b, -1, ...}.
    ValueError: a row outside the state, a row in two families or twice in one, more than 16 rows, a negative share_end."""
    tab = np.full((B, FAMILY_INTS), -1, dtype=np.int32)
    tab[:, 0] = tab[:, 2] = np.arange(B, dtype=np.int32)
    tab[:, 1] = 0
    taken = set()
    for rows, share_end in families:
        rows, share_end = [int(r) for r in rows], int(share_end)
        if any(not 0 <= r < B for r in rows):
            raise ValueError(f"family {rows}: rows of a state of {B}")
        if len(set(rows)) != len(rows) or taken & set(rows):
            raise ValueError(f"family {rows}: a row belongs to one family, once")
        if len(rows) > MAX_N:
            raise ValueError(f"family of {len(rows)} rows: at most {MAX_N} rows share a prefix (one forked row + {MAX_N - 1} copies)")
        if share_end < 0:
            raise ValueError(f"family {rows}: share_end {share_end} is negative")
        taken |= set(rows)
        if len(rows) < 2:
            continue
        tab[rows, 0], tab[rows, 1] = rows[0], share_end
        tab[rows, 2:] = -1                                       # (the list stands on the leader's row alone)
        tab[rows[0], 2:2 + len(rows)] = rows
    return tab


FAMILY_BREAK_EVEN = 4096              # (rows - 1) * shared keys from which sharing pays: profiles/share_prefix_step_time.txt


def family_pays(n_rows, share_end):
    """Does a family of n_rows rows that share share_end keys gain from the shared-prefix launch?  Its plan (single-wave
    workgroups over short splits, always a merge launch) costs 0.15 - 0.7 ms per step against the plain plan on the full model (cleared - unshared in the profile),
    and sharing saves (n_rows - 1) * shared keys * 393 KB of reads: measured with every family registered (profiles/share_prefix_step_time.txt, run 2), it
    loses at 2 rows x 512 keys, is level at 4, 8 and 16 x 512 and 2 x 2,531, and wins from 4 x 2,531 on."""
    return (int(n_rows) - 1) * int(share_end) >= FAMILY_BREAK_EVEN


def families_without(families, rows):
    """`families` after `rows` left: a leader that left hands its place to the next member (the copies are identical up to
    share_end), a family of one remaining row is dropped."""
    gone, out = set(int(r) for r in rows), []
    for members, share_end in families:
        left = tuple(r for r in members if r not in gone)
        if len(left) > 1:
            out.append((left, share_end))
    return out
