"""Prompt prefix cache: a store of prompt K/V and the rule that decides when a prefix may be reused (host logic only).

The most expensive request of a vision-language server is also its most repetitive one: every question about the same
picture starts with the same `<|user|>\\n` + image-slot run, and K is stored already rotated by its LOGICAL position, so a
row of K/V is valid in any column of any slot.  An entry holds the K/V of the first P tokens of a prompt, compact
(`[nl, nkv, P8, hd]` / `[nl, nkv, hd, P8]`, P8 = P rounded up to 8; codes + scales for the int8 cache); the device path
that moves it is `ops.kv_copy` (p3v_kv_copy), driven by `model.capture_prefix` / `model.prefill_slot(prefix=...)`.

Matching rule (`match_len`): over entries with an equal key -- (model.epoch, adapter name or None, RoPE regime, cache
kind) -- the longest common prefix of the token ids, cut back so that
  (a) at least one prompt token is left to compute (P <= S - 1),
  (b) the match does not end inside an image's slot run (negative ids): it covers all of that image's slots or none,
  (c) every image whose slots are covered has the same digest in request and entry.  The ids of two requests with
      different pictures of the same size are IDENTICAL: only the digest tells them apart.
A match shorter than `min_tokens` is a miss.  Entries are immutable; eviction is LRU by bytes.
"""
import collections
import hashlib
import threading

import numpy as np

KINDS = ("bf16", "int8")


def image_digest(img):
    """Digest of a SOURCE image (PIL): mode, size and raw bytes.  Computed next to the processor call -- never from
    `pixel_values`, which is a device tensor of tens of megabytes."""
    h = hashlib.blake2b(digest_size=16)
    h.update(f"{img.mode}|{img.size[0]}x{img.size[1]}|".encode())
    h.update(img.tobytes())
    return h.hexdigest()


def image_digests(images):
    """One digest per image of a request (None without images)."""
    if images is None:
        return None
    return [image_digest(i) for i in (images if isinstance(images, (list, tuple)) else [images])]


def slot_runs(ids):
    """Image slot runs of a prompt: [(start, end, image index)] in column order (slots of image i carry the id -(i + 1))."""
    ids = np.asarray(ids).reshape(-1)
    neg = np.nonzero(ids < 0)[0]
    runs = []
    if neg.size:
        cut = np.nonzero((np.diff(neg) != 1) | (np.diff(ids[neg]) != 0))[0] + 1
        for seg in np.split(neg, cut):
            runs.append((int(seg[0]), int(seg[-1]) + 1, int(-ids[seg[0]] - 1)))
    return runs


def _digest_of(digests, i):
    return digests[i] if digests is not None and 0 <= i < len(digests) else None


def match_len(ids, digests, e_ids, e_digests, leave=1):
    """Tokens of the entry (e_ids, e_digests) a request (ids, digests) may reuse: the rule of the module doc without the
    `min_tokens` threshold.  `leave`: prompt tokens that must stay to be computed (1 for a lookup, 0 for "is this range
    covered already")."""
    ids, e_ids = np.asarray(ids).reshape(-1), np.asarray(e_ids).reshape(-1)
    n = min(ids.size, e_ids.size)
    diff = np.nonzero(ids[:n] != e_ids[:n])[0]
    P = int(diff[0]) if diff.size else n
    P = min(P, ids.size - leave)
    if P <= 0:
        return 0
    for runs in (slot_runs(ids), slot_runs(e_ids)):             # (b): never end inside a slot run, the request's or the entry's
        for a, b, _ in runs:
            if a < P < b:
                P = a
    for a, b, i in slot_runs(ids):                              # (c): covered images are the same pictures
        if b <= P:
            d = _digest_of(digests, i)
            if d is None or d != _digest_of(e_digests, i):
                P = a
                break
    return max(P, 0)


def capture_len(ids, prefix_len=None):
    """Tokens a request's entry covers.  Default: through the last image slot if the prompt has images, else the whole
    prompt; an explicit `prefix_len` overrides it.  Never ends inside a slot run."""
    ids = np.asarray(ids).reshape(-1)
    runs = slot_runs(ids)
    if prefix_len is not None:
        P = max(0, min(int(prefix_len), ids.size))
        for a, b, _ in runs:
            if a < P < b:
                P = a
        return P
    return runs[-1][1] if runs else int(ids.size)


def kv_bytes(P, nl, nkv, hd, kind):
    """Bytes of an entry of P tokens (K + V^T at P8 columns; int8: codes + two fp32 scale rows)."""
    P8 = (int(P) + 7) // 8 * 8
    return 2 * nl * nkv * P8 * hd * 2 if kind == "bf16" else 2 * nl * nkv * P8 * (hd + 4)


def alloc_kv(P, nl, nkv, hd, kind, device):
    """The compact K/V tensors of an entry: (k [nl, nkv, P8, hd], vt [nl, nkv, hd, P8]) bf16, or uint8 codes of the same
    shapes + (k_scale, v_scale) fp32 [nl, nkv, P8].  Columns P .. P8 stay zero."""
    import torch
    P8 = (int(P) + 7) // 8 * 8
    dt = torch.bfloat16 if kind == "bf16" else torch.uint8
    kv = (torch.zeros((nl, nkv, P8, hd), dtype=dt, device=device), torch.zeros((nl, nkv, hd, P8), dtype=dt, device=device))
    if kind == "int8":
        kv += (torch.zeros((nl, nkv, P8), dtype=torch.float32, device=device), torch.zeros((nl, nkv, P8), dtype=torch.float32, device=device))
    return kv


class Entry:
    __slots__ = ("ids", "digests", "key", "kv", "P", "nbytes", "slot_counts")

    def __init__(self, ids, digests, key, kv):
        self.ids = np.array(np.asarray(ids).reshape(-1), dtype=np.int64)
        self.ids.setflags(write=False)
        self.P = int(self.ids.size)
        runs = slot_runs(self.ids)
        self.digests = tuple(_digest_of(digests, i) for i in range(max((i for _, _, i in runs), default=-1) + 1))
        self.slot_counts = tuple(b - a for a, b, _ in runs)      # each covered image's slot count
        self.key, self.kv = key, tuple(kv)
        self.nbytes = int(sum(t.numel() * t.element_size() for t in self.kv))


class PrefixCache:
    """Immutable entries under an LRU byte budget.  Thread-safe (a server's handler threads read the counters while the engine
    thread looks up and inserts)."""

    def __init__(self, max_bytes, min_tokens=64):
        self.max_bytes, self.min_tokens = int(max_bytes), int(min_tokens)
        if self.max_bytes < 0 or self.min_tokens < 1:
            raise ValueError("PrefixCache: max_bytes >= 0 and min_tokens >= 1")
        self._entries = collections.OrderedDict()                # id(entry) -> entry, least recently used first
        self._lock = threading.Lock()
        self.hits = self.misses = self.bypassed = self.tokens_reused = self.evictions = 0
        self.bytes = 0

    # ---- keys
    @staticmethod
    def key(epoch, adapter, long_rope, kind):
        if kind not in KINDS:
            raise ValueError(f"cache kind must be one of {KINDS}, got {kind!r}")
        return (int(epoch), adapter, "long" if long_rope else "short", kind)

    @property
    def entries(self):
        return len(self._entries)

    def counters(self):
        with self._lock:
            return {"hits": self.hits, "misses": self.misses, "bypassed": self.bypassed, "tokens_reused": self.tokens_reused,
                    "entries": len(self._entries), "bytes": self.bytes, "evictions": self.evictions,
                    "max_bytes": self.max_bytes, "min_tokens": self.min_tokens}

    def bypass(self):
        """A request that may not use the store (cache_format="mlx4", a batched prompt list): counted, nothing else."""
        with self._lock:
            self.bypassed += 1

    def _drop_stale(self, key):
        """Entries of an older model.epoch can never match again (set_adapters / set_adapter_bank changed the K/V numbers)."""
        for k in [k for k, e in self._entries.items() if e.key[0] < key[0]]:
            self.bytes -= self._entries.pop(k).nbytes

    # ---- lookup
    def lookup(self, ids, digests, key, count=True):
        """(entry, P) of the longest reusable prefix, or None.  A hit makes its entry the most recently used."""
        with self._lock:
            self._drop_stale(key)
            best, best_p = None, 0
            for e in self._entries.values():
                if e.key != key:
                    continue
                p = match_len(ids, digests, e.ids, e.digests)
                if p > best_p:
                    best, best_p = e, p
            if best is None or best_p < self.min_tokens:
                if count:
                    self.misses += 1
                return None
            self._entries.move_to_end(id(best))
            if count:
                self.hits += 1
                self.tokens_reused += best_p
            return best, best_p

    # ---- capture
    def wants(self, ids, digests, key, P, nbytes=None):
        """Should tokens [0, P) of this request be captured?  Not when the range is shorter than `min_tokens`, when an entry with
        the same key already covers it, or when it is larger than the whole budget."""
        if P < self.min_tokens or P > np.asarray(ids).size:
            return False
        if nbytes is not None and nbytes > self.max_bytes:
            return False
        head = np.asarray(ids).reshape(-1)[:P]
        with self._lock:
            return not any(e.key == key and match_len(head, digests, e.ids, e.digests, leave=0) >= P for e in self._entries.values())

    def insert(self, ids, digests, key, kv):
        """Store the K/V of tokens `ids` (already cut to the captured length).  Evicts least recently used entries until the new
        one fits; an entry larger than the budget is not stored.  Returns the entry or None."""
        e = Entry(ids, digests, key, kv)
        with self._lock:
            if e.nbytes > self.max_bytes:
                return None
            while self.bytes + e.nbytes > self.max_bytes and self._entries:
                _, old = self._entries.popitem(last=False)
                self.bytes -= old.nbytes
                self.evictions += 1
            self._entries[id(e)] = e
            self.bytes += e.nbytes
        return e

    def clear(self):
        with self._lock:
            self._entries.clear()
            self.bytes = 0
