"""Near-duplicate clustering (Collection.near_duplicates): the definition, in numpy, and the host path.

With t = range_search.score_threshold(max_distance) and "allowed" as everywhere else (live rows, intersected with `where` and
`where_document`):

  edges   For an allowed row i, R(i) is the set of allowed rows that query_range returns for the embedding the collection itself
          returns for i (get(include=["embeddings"]): the stored normalised row) at that distance, with an unlimited max_results —
          the rows j whose engine-exact fp32 score against K1(stored row i) is >= t. There is an edge i -> j for every j in R(i),
          j != i; the graph is the undirected closure of those edges. Nothing assumes the score to be symmetric.
  labels  label[r] = the smallest row of r's connected component; -1 for a row that is not allowed.
  totals  total[r] = |R(r)| — query_range's `totals` for that row; the row itself counts when it is in range (a row's own score can
          be 0.99999994, a zero row scores 0). 0 for a row that is not allowed.

Labels and totals are functions of this definition alone: batch size, list length, path and thread schedule do not show.
near_dup_model states it over any source of exact scores; near_dup_host answers through range_search_host for engines without
librdx's rdx_index_near_dup.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Tuple

import numpy as np

from . import _lib as L
from . import range_search as RS

MAX_NEIGHBORS = L.RANGE_MAX_RESULTS      # the longest list rdx_index_range returns: the upper limit of max_neighbors
STAT_KEYS = ("calls", "rows", "listed", "dense", "batches", "host")


class UnionFind:
    """plain sequential union-find over rows 0..n-1; the larger root goes under the smaller, so a root is its set's smallest row"""

    def __init__(self, n: int):
        self.parent = list(range(n))

    def find(self, x: int) -> int:
        p = self.parent
        while p[x] != x:
            p[x] = p[p[x]]
            x = p[x]
        return x

    def union(self, a: int, b: int):
        a, b = self.find(a), self.find(b)
        if a != b:
            self.parent[max(a, b)] = min(a, b)


def labels_from_adjacency(adj: np.ndarray, allowed: Optional[np.ndarray] = None) -> np.ndarray:
    """adj bool [n][n] (adj[i][j]: an edge i -> j, directed or not; the diagonal is ignored) -> labels i64 [n]: the smallest row of
    the row's component in the undirected closure, over allowed rows only (edges from or to a row that is not allowed do not exist);
    -1 for a row that is not allowed"""
    adj = np.asarray(adj, dtype=bool)
    n = adj.shape[0]
    ok = np.ones(n, dtype=bool) if allowed is None else np.asarray(allowed, dtype=bool)
    uf = UnionFind(n)
    for i in np.flatnonzero(ok):
        for j in np.flatnonzero(adj[i] & ok):
            if j != i:
                uf.union(int(i), int(j))
    return np.array([uf.find(r) if ok[r] else -1 for r in range(n)], dtype=np.int64)


def near_dup_model(scores_of: Callable[[int], np.ndarray], n: int, t, allowed: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray]:
    """the definition over exact scores: scores_of(i) = fp32 [n], the engine-exact scores of every row against K1(stored row i)
    -> (labels i64 [n], totals i64 [n])"""
    ok = np.ones(n, dtype=bool) if allowed is None else np.asarray(allowed, dtype=bool)
    t = np.float32(t)
    uf = UnionFind(n)
    totals = np.zeros(n, dtype=np.int64)
    for i in np.flatnonzero(ok):
        s = np.asarray(scores_of(int(i)), dtype=np.float32)
        hit = np.flatnonzero((s >= t) & ok)
        totals[i] = len(hit)
        for j in hit:
            if j != i:
                uf.union(int(i), int(j))
    labels = np.array([uf.find(r) if ok[r] else -1 for r in range(n)], dtype=np.int64)
    return labels, totals


def labels_from_lists(n: int, allowed: Optional[np.ndarray], query_rows, lists) -> np.ndarray:
    """labels from neighbour lists (lists[k]: the rows listed for query_rows[k]) by the sequential union-find: what a caller did
    before near_duplicates existed (tools/dedup_bench.py's baseline)"""
    ok = np.ones(n, dtype=bool) if allowed is None else np.asarray(allowed, dtype=bool)
    uf = UnionFind(n)
    for i, rr in zip(query_rows, lists):
        for j in rr:
            if j >= 0 and j != i:
                uf.union(int(i), int(j))
    return np.array([uf.find(r) if ok[r] else -1 for r in range(n)], dtype=np.int64)


def clusters_of(labels: np.ndarray) -> List[List[int]]:
    """labels -> the components of at least two rows as ascending row lists, ordered by their first row"""
    lab = np.asarray(labels, dtype=np.int64)
    rows = np.flatnonzero(lab >= 0)
    if rows.size == 0:
        return []
    order = rows[np.argsort(lab[rows], kind="stable")]          # by label, rows ascending inside (stable over ascending rows)
    cuts = np.flatnonzero(np.diff(lab[order])) + 1
    return [g.tolist() for g in np.split(order, cuts) if len(g) >= 2]


def near_dup_host(engine, t, search_args: dict, allowed: Optional[np.ndarray] = None, batch: int = 256) -> Tuple[np.ndarray, np.ndarray]:
    """engines without rdx_index_near_dup: the definition through range_search_host with max_results = the engine's row count (every
    row in range is listed), the stored rows fetched with engine.get as the caller of query_range would -> (labels, totals)"""
    n = len(engine)
    ok = np.ones(n, dtype=bool) if allowed is None else np.asarray(allowed, dtype=bool)
    uf = UnionFind(n)
    totals = np.zeros(n, dtype=np.int64)
    rows = np.flatnonzero(ok)
    for a in range(0, len(rows), batch):
        qr = rows[a: a + batch]
        q = engine.get(qr)
        thr = np.full(len(qr), np.float32(t), dtype=np.float32)
        _, r, c, tt = RS.range_search_host(engine, q, thr, n, search_args)
        for k, i in enumerate(qr):
            totals[i] = int(tt[k])
            for j in r[k, : c[k]]:
                if j != i:
                    uf.union(int(i), int(j))
    labels = np.array([uf.find(r) if ok[r] else -1 for r in range(n)], dtype=np.int64)
    return labels, totals
