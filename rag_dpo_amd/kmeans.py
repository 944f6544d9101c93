"""Spherical k-means of the stored rows (Collection.kmeans): the definition, in numpy, and the host path.

"Allowed" as everywhere else: live rows, intersected with `where` and `where_document`. K1 = the engine's normalisation of a query or
an added row (x / max(|x|_2, 1e-12), the norm from the lane-order fp64 sum, each element rounded to fp32 once: `k1`).

  score(c, r)  the engine-exact fp32 score of stored row r against query c: 1 - distance of query(query_embeddings=[c]). K1 applied to
               c, then the lane-order fp64 sum against the stored row, rounded to fp32 once (mmr.pair_scores states that sum).
  assign(C)    for every allowed row r, label[r] = the centroid with the largest score, compared as fp32 values (-0 equals +0), ties
               to the smaller index; score[r] = that score. A row that is not allowed: label -1, score -inf.
  update(L, C) the members of cluster c are the rows with label c, ascending. They are cut into segments of SEGMENT = 256 consecutive
               members; per element a segment's total is the sequential fp64 sum of its members' stored fp32 values from +0.0, the
               cluster's sum the sequential fp64 sum of its segments' totals, in segment order, from +0.0. The new centroid is K1 of the
               sums rounded to fp32. A cluster without members keeps its centroid. SEGMENT is part of the definition.
  loop         C = K1(init); L, S = assign(C); n_iter = 0; converged = False
               while n_iter < max_iter:
                   C = update(L, C); n_iter += 1
                   L2, S = assign(C); same = (L2 == L); L = L2
                   if same: converged = True; break
               The returned labels and scores are always assign(returned centroids); max_iter = 0 is a pure assignment.
  init         an array [K][dim], or None: the stored rows of sample_rows(allowed rows, K, seed). Identical init centroids are legal:
               while two are identical the later one gets no row (and, without rows, stays where it is).

Labels, scores, centroids and counts are functions of this definition alone: batch and block sizes, the path and the thread schedule do
not show. kmeans_model states it over any source of exact scores; kmeans_host answers through engine.search for engines without
librdx's rdx_index_kmeans.
"""
from __future__ import annotations

from typing import Callable, Optional, Tuple

import numpy as np

from . import mmr as MM

SEGMENT = 256                              # members per segment of the ordered per-cluster sum: part of the definition
MAX_CLUSTERS, MAX_ITER = 4096, 1000        # include/rdx.h RDX_KMEANS_MAX_CLUSTERS, rdx_index_kmeans' max_iter
STAT_KEYS = ("calls", "rows", "iterations", "host")


def lane_sum(prod) -> np.ndarray:
    """prod fp64 [n][dim] (dim % 4 == 0) -> fp64 [n]: the lane-order sum of every row, the order of the engine's exact score and of K1's
    norm: lane l of 64 adds the float4 groups l, l + 64, ... (x, y, z, w within a group), the lanes meet by the xor butterfly 32 .. 1"""
    p = np.asarray(prod, dtype=np.float64)
    n, dim = p.shape
    n4 = dim // 4
    p = p.reshape(n, n4, 4)
    acc = np.zeros((n, 64), dtype=np.float64)
    for g0 in range(0, n4, 64):
        lanes = min(64, n4 - g0)
        for e in range(4):
            acc[:, :lanes] += p[:, g0: g0 + lanes, e]
    lane = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lane ^ m]
    return acc[:, 0]


def k1(x) -> np.ndarray:
    """K1 of every row of x fp32 [n][dim]: what the engine does to a query and to an added row, bit for bit"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim != 2 or x.shape[1] % 4:
        raise ValueError("k1 wants [n][dim] rows, dim a multiple of 4")
    x64 = x.astype(np.float64)
    den = np.maximum(np.sqrt(lane_sum(x64 * x64)), 1e-12)     # a product of two floats is exact in fp64
    return (x64 / den[:, None]).astype(np.float32)


def sample_rows(allowed_rows, n_clusters: int, seed: int) -> np.ndarray:
    """the init rule of init=None: K of the allowed rows, drawn without replacement by numpy's default generator, ascending"""
    rows = np.asarray(allowed_rows, dtype=np.int64)
    k = int(n_clusters)
    if k > rows.size:
        raise ValueError(f"n_clusters = {k} exceeds the {rows.size} rows the filters allow")
    return np.sort(np.random.default_rng(seed).choice(rows, k, replace=False))


def ordered_sum(members, segment: int = SEGMENT) -> np.ndarray:
    """members fp32 [m][dim], in member order -> fp64 [dim]: segments of `segment` members summed one by one from +0.0, the segments'
    totals summed one by one from +0.0 (`segment` differs from SEGMENT only in tests that show the order matters)"""
    x = np.asarray(members, dtype=np.float32)
    total = np.zeros(x.shape[1], dtype=np.float64)
    for a in range(0, x.shape[0], segment):
        part = np.zeros(x.shape[1], dtype=np.float64)
        for row in x[a: a + segment]:
            part += row
        total += part
    return total


def assign_from_scores(score_cols, n: int, allowed: Optional[np.ndarray]) -> Tuple[np.ndarray, np.ndarray]:
    """score_cols: per centroid, in index order, its fp32 scores of every row -> (labels i64 [n], scores f32 [n])"""
    ok = np.ones(n, dtype=bool) if allowed is None else np.asarray(allowed, dtype=bool)
    best = np.full(n, -np.inf, dtype=np.float32)
    lab = np.full(n, -1, dtype=np.int64)
    for c, s in enumerate(score_cols):
        s = np.asarray(s, dtype=np.float32)
        better = ok & ((s > best) | (lab < 0))                 # strictly larger as fp32 values: a tie stays with the smaller index
        best[better] = s[better]
        lab[better] = c
    return lab, best


def update(rows_hat, labels, centroids, segment: int = SEGMENT) -> np.ndarray:
    c_new = np.array(centroids, dtype=np.float32, copy=True)
    for c in range(c_new.shape[0]):
        members = np.flatnonzero(labels == c)                  # ascending
        if members.size:
            c_new[c] = k1(ordered_sum(rows_hat[members], segment).astype(np.float32)[None, :])[0]
    return c_new


def _loop(x, init, max_iter: int, assign, segment: int = SEGMENT):
    """the loop of the definition over an assign(C) -> (labels, scores)"""
    C = k1(init)
    L, S = assign(C)
    n_iter, converged = 0, False
    while n_iter < int(max_iter):
        C = update(x, L, C, segment)
        n_iter += 1
        L2, S = assign(C)
        same = bool((L2 == L).all())
        L = L2
        if same:
            converged = True
            break
    counts = np.bincount(L[L >= 0], minlength=C.shape[0]).astype(np.int64)
    return L, S, C, counts, n_iter, converged


def kmeans_model(rows_hat, init, max_iter: int, allowed: Optional[np.ndarray] = None,
                 scores_of: Optional[Callable[[np.ndarray], np.ndarray]] = None, segment: int = SEGMENT):
    """The definition. rows_hat fp32 [n][dim]: the stored rows; init fp32 [K][dim]; scores_of(qhat fp32 [dim]) = the exact fp32 scores of
    every stored row against the normalised query qhat (default: mmr.pair_scores).
    -> (labels i64 [n], scores f32 [n], centroids f32 [K][dim], counts i64 [K], n_iter, converged)"""
    x = np.ascontiguousarray(rows_hat, dtype=np.float32)
    n = x.shape[0]
    if scores_of is None:
        scores_of = lambda q: MM.pair_scores(x, q)             # noqa: E731

    def assign(C):
        qhat = k1(C)
        return assign_from_scores((scores_of(qhat[c]) for c in range(C.shape[0])), n, allowed)

    return _loop(x, init, max_iter, assign, segment)


def clusters_of(labels: np.ndarray, n_clusters: int):
    """labels -> per cluster its rows, ascending"""
    lab = np.asarray(labels, dtype=np.int64)
    return [np.flatnonzero(lab == c) for c in range(int(n_clusters))]


def kmeans_host(engine, init, max_iter: int, search_args: dict, allowed: Optional[np.ndarray] = None, chunk: int = 64):
    """engines without rdx_index_kmeans: the definition with the assignment through engine.search over the allowed rows (k = the
    engine's row count: every allowed row is listed with its exact score), the centroids `chunk` at a time; the stored rows fetched
    with engine.get -> kmeans_model's tuple"""
    n = len(engine)
    ok = np.ones(n, dtype=bool) if allowed is None else np.asarray(allowed, dtype=bool)
    x = engine.get(np.arange(n, dtype=np.int64))

    def assign(C):
        best = np.full(n, -np.inf, dtype=np.float32)
        lab = np.full(n, -1, dtype=np.int64)
        for a in range(0, C.shape[0], chunk):
            s, r, cn = engine.search(C[a: a + chunk], n, **search_args)
            for j in range(s.shape[0]):
                rows, sc = r[j, : cn[j]], s[j, : cn[j]]
                keep = ok[rows]
                rows, sc = rows[keep], sc[keep]
                better = (sc > best[rows]) | (lab[rows] < 0)
                best[rows[better]] = sc[better]
                lab[rows[better]] = a + j
        return lab, best

    return _loop(x, init, max_iter, assign)
