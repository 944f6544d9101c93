"""TEST-ONLY engine: the CPU oracle behind the engine interface of rag_dpo_amd.collection / sharded.
Lets the host logic (ids, metadata, where filters, paging, sharded merge orchestration) run without a GPU.
The product never imports this file; its only engine is rag_dpo_amd.engine.HipIndex."""
import numpy as np

from oracle import oracle as O


class OracleEngine:
    def __init__(self, dim, device=0):
        self.dim = dim
        self.device = device
        self.rows = np.zeros((0, dim), dtype=np.float32)

    def __len__(self):
        return self.rows.shape[0]

    def _check(self, x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim != 2 or x.shape[1] != self.dim:
            raise ValueError("bad shape")
        if not np.isfinite(x).all():
            raise ValueError("embeddings contain NaN or Inf")
        return x

    def add(self, x):
        self.rows = np.concatenate([self.rows, O.normalize_rows(self._check(x))])

    def add_stored(self, x):
        self.rows = np.concatenate([self.rows, self._check(x)])

    def _check_ids(self, ids):
        """the ids of an update: rows the engine holds, each at most once (include/rdx.h rdx_index_update)"""
        ids = np.asarray(ids, dtype=np.int64)
        if ids.size and (ids.min() < 0 or ids.max() >= len(self)):
            raise ValueError(f"row id out of range [0, {len(self)})")
        uniq, times = np.unique(ids, return_counts=True)
        if (times > 1).any():
            raise ValueError(f"row id {int(uniq[times > 1][0])} is given more than once")
        return ids

    def update(self, ids, x):
        ids, y = self._check_ids(ids), O.normalize_rows(self._check(x))   # all or nothing: both judged before a row changes
        self.rows[ids] = y

    def get(self, ids):
        return self.rows[np.asarray(ids, dtype=np.int64)].copy()

    def compact(self, keep):
        self.rows = self.rows[np.asarray(keep, dtype=np.int64)].copy()

    def search(self, q, k, allow_bits=None):
        q = self._check(q)
        allow = None
        if allow_bits is not None:
            n = len(self)
            allow = np.unpackbits(np.asarray(allow_bits, dtype=np.uint32).view(np.uint8), bitorder="little")[:n].astype(bool)
        if len(self) == 0:
            B = q.shape[0]
            return (np.full((B, k), -np.inf, np.float32), np.full((B, k), -1, np.int64), np.zeros(B, np.int32))
        return O.cosine_topk(self.rows, q, k, allow)

    def close(self):
        pass


def factory(dim, device=0):
    return OracleEngine(dim, device)
