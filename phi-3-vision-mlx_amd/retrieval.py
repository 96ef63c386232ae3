"""A vector store over the model's own embeddings: `VDB(items)(text, n_topk)` is the reference's contract (gte.py:189-203:
embed, multiply against the stored embeddings, arg-sort), here on one model and one kernel.  The index is a bf16 device tensor of
L2-normalised rows that grows by doubling; a query is the normalised fp32 embedding rounded to bf16; scores are fp32 and the
k best come from ONE pass over the index, the score matrix never written (include/p3v.h: p3v_sim_topk)."""
import numpy as np

from ._lib import SIM_TOPK_MAX, SIM_TOPK_MAX_Q


def _device_search(index, n, queries, k):
    """queries: np.float32 [Q <= 16, D] -> (idx [Q, k], score [Q, k]) through p3v_sim_topk."""
    import torch
    from . import ops
    q = torch.as_tensor(np.ascontiguousarray(queries, dtype=np.float32)).to(index.device).to(torch.bfloat16)
    idx, score = ops.sim_topk(index, q, k, n=n)
    return idx.cpu().numpy(), score.cpu().numpy()


class VDB:
    """VDB(items=None, preload=None, key=str, pooling="last", batch=8).  add(items) embeds key(item) in batches and appends;
    add_vectors(vectors, items) takes the caller's own vectors (normalised here); search(query, n_topk) takes a string, a list of
    strings or a [Q, D] array and returns (indices [Q, k], scores [Q, k]), -1 / -inf where the store holds fewer than k rows;
    __call__(text, n_topk) returns [[item, ...], ...], best first.  embed_fn(list of str) -> [n, D] replaces the model;
    search_fn(index, n, queries, k) replaces the device search (both: how the host logic is tested without a device)."""

    def __init__(self, items=None, preload=None, key=str, pooling="last", batch=8, embed_fn=None, search_fn=None, device=None):
        from .api import check_pooling
        self.key, self.pooling, self.batch = key, check_pooling(pooling), max(1, int(batch))
        self.preload, self.embed_fn, self.search_fn = preload, embed_fn, search_fn or _device_search
        self.device = device
        self.items, self.n, self.index = [], 0, None
        if items is not None:
            self.add(items)

    def __len__(self):
        return self.n

    @property
    def capacity(self):
        return 0 if self.index is None else int(self.index.shape[0])

    def _embed(self, texts):
        if self.embed_fn is not None:
            return np.asarray(self.embed_fn(list(texts)), dtype=np.float32).reshape(len(texts), -1)
        from . import api
        if self.preload is None:
            self.preload = api.load()
        out = [api.embed(list(texts[i:i + self.batch]), preload=self.preload, pooling=self.pooling, normalize=True)
               for i in range(0, len(texts), self.batch)]
        return np.concatenate(out, 0)

    def _rows(self, vectors):
        """fp32 [n, D], L2-normalised (a zero row stays zero), as the bf16 rows the index holds."""
        v = np.asarray(vectors, dtype=np.float32)
        v = v[None] if v.ndim == 1 else v
        if v.ndim != 2 or v.shape[1] % 8 or not 8 <= v.shape[1] <= 8192:
            raise ValueError(f"vectors must be [n, D] with D a multiple of 8 up to 8192, got {v.shape}")
        norm = np.sqrt((v.astype(np.float64) ** 2).sum(-1, keepdims=True))
        return (v / np.where(norm == 0, 1.0, norm)).astype(np.float32)

    def _reserve(self, n_new, D):
        import torch
        if self.index is not None and self.index.shape[1] != D:
            raise ValueError(f"vectors of width {D} for an index of width {self.index.shape[1]}")
        need = self.n + n_new
        cap = self.capacity
        if need <= cap:
            return
        new_cap = max(cap, 16)
        while new_cap < need:
            new_cap *= 2
        device = self.device or (self.preload[0].device if self.preload is not None and hasattr(self.preload[0], "device") else
                                 "cuda" if torch.cuda.is_available() else "cpu")
        grown = torch.zeros((new_cap, D), dtype=torch.bfloat16, device=device)
        if self.n:
            grown[:self.n] = self.index[:self.n]
        self.index = grown

    def add_vectors(self, vectors, items):
        import torch
        items = list(items)
        rows = self._rows(vectors)
        if len(items) != rows.shape[0]:
            raise ValueError(f"{rows.shape[0]} vectors for {len(items)} items")
        if not items:
            return self
        self._reserve(rows.shape[0], rows.shape[1])
        self.index[self.n:self.n + rows.shape[0]] = torch.as_tensor(rows).to(self.index.device).to(torch.bfloat16)
        self.items += items
        self.n += rows.shape[0]
        return self

    def add(self, items):
        items = list(items)
        for i in range(0, len(items), self.batch):
            chunk = items[i:i + self.batch]
            self.add_vectors(self._embed([self.key(it) for it in chunk]), chunk)
        return self

    def search(self, query, n_topk=1):
        k = int(n_topk)
        if not 1 <= k <= SIM_TOPK_MAX:
            raise ValueError(f"n_topk = {n_topk} outside 1..{SIM_TOPK_MAX} (P3V_SIM_TOPK_MAX)")
        if isinstance(query, str):
            query = [query]
        if isinstance(query, (list, tuple)) and all(isinstance(q, str) for q in query):
            qv = self._embed(list(query)) if len(query) else np.zeros((0, 8), dtype=np.float32)
        else:
            qv = query
        qv = self._rows(qv) if len(qv) else np.zeros((0, 8), dtype=np.float32)
        Q = qv.shape[0]
        idx, score = np.full((Q, k), -1, dtype=np.int32), np.full((Q, k), -np.inf, dtype=np.float32)
        if self.index is None or Q == 0:
            return idx, score
        if qv.shape[1] != self.index.shape[1]:
            raise ValueError(f"queries of width {qv.shape[1]} for an index of width {self.index.shape[1]}")
        for i in range(0, Q, SIM_TOPK_MAX_Q):                      # one launch per 16 queries
            idx[i:i + SIM_TOPK_MAX_Q], score[i:i + SIM_TOPK_MAX_Q] = self.search_fn(self.index, self.n, qv[i:i + SIM_TOPK_MAX_Q], k)
        return idx, score

    def __call__(self, text, n_topk=1):
        idx, _ = self.search(text, n_topk)
        return [[self.items[i] for i in row if i >= 0] for row in idx]
