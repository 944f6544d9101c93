"""Threshold search (Collection.query_range): the definition, in numpy, and the host path.

Per query, with D = max_distance and m = max_results: the ranking is query()'s — the exact fp32 cosine scores s of the allowed rows, s
descending, row ascending — and the distance of a row is d = fl32(1 - s). A row is in range iff d <= D. s -> fl32(1 - s) is monotone
non-increasing, so "d <= D" is "s >= t" for ONE fp32 number t = score_threshold(D), the smallest fp32 whose distance is <= D: the
kernels compare s >= t and nothing else. `total` is the number of rows in range (exact; it may exceed m), the returned list the first
min(m, total) entries of the ranking. Therefore query_range(D, m) is the cut of query(n_results=m) at distance D, and total the length
of the same cut of query(n_results=count()). range_model states that cut; engines without librdx's rdx_index_range answer through it.
"""
from __future__ import annotations

import numpy as np

from . import _lib as L

MAX_RESULTS = L.RANGE_MAX_RESULTS
_ONE = np.float32(1.0)
_INF32 = np.float32(np.inf)


def _dist(t: np.float32) -> np.float32:
    return np.float32(_ONE - t)                     # fl32(1 - t): one fp32 subtraction, rounded once


def _key(t: np.float32) -> int:
    """the monotone map fp32 -> integer (ascending): what the radix selects order scores by (rdx_common.hpp f2key)"""
    u = int(np.float32(t).view(np.uint32))
    return (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)


def _unkey(k: int) -> np.float32:
    u = (k & 0x7FFFFFFF) if k & 0x80000000 else (~k & 0xFFFFFFFF)
    return np.uint32(u).view(np.float32)


_FMAX = np.float32(np.finfo(np.float32).max)


def score_threshold(max_distance) -> np.float32:
    """D -> the smallest fp32 t with fl32(1 - t) <= D (D = +inf: -inf, every allowed row; a D below every finite distance: +inf, none).
    fl32(1 - t) is monotone in t, so t is found by bisection over the ordered fp32 numbers: 32 steps, whatever D — near t = 0 a step
    of the distance spans 2^23 and more steps of t (fl32(1 - t) = 1 for every |t| < 2^-25), so walking by nextafter from 1 - D would not
    end. NaN is refused."""
    D = float(max_distance)
    if D != D:
        raise ValueError("max_distance must not be NaN")
    if D == np.inf:
        return np.float32(-np.inf)
    with np.errstate(over="ignore"):
        if float(_dist(_FMAX)) > D:
            return _INF32
        lo, hi = _key(-_FMAX), _key(_FMAX)           # the answer lies in [lo, hi]; hi is in range
        while lo < hi:
            mid = (lo + hi) // 2
            if float(_dist(_unkey(mid))) <= D:
                hi = mid
            else:
                lo = mid + 1
    t = _unkey(lo)
    return np.float32(0.0) if t == 0 else np.float32(t)   # (one zero: -0.0 and +0.0 compare equal, +0.0 is returned)


def range_model(scores, rows, t, m: int):
    """one query's ranking (scores f32 descending, rows i64; query()'s order, every allowed row or a prefix of them) -> (scores, rows,
    total): total = entries with score >= t, returned the first min(m, total). With a prefix of the ranking, total counts the prefix."""
    s = np.asarray(scores, dtype=np.float32)
    r = np.asarray(rows, dtype=np.int64)
    total = int(np.count_nonzero(s >= np.float32(t)))
    n = min(int(m), total)
    return s[:n].copy(), r[:n].copy(), total


def as_thresholds(max_distance, nq: int) -> np.ndarray:
    """a float, or one per query -> fp32 [nq] score thresholds"""
    a = np.asarray(max_distance, dtype=np.float64)
    if a.ndim == 0:
        return np.full(nq, score_threshold(float(a)), dtype=np.float32)
    if a.shape != (nq,):
        raise ValueError(f"Expected max_distance to be a number or one per query ({nq}), got shape {a.shape}")
    if np.isnan(a).any():
        raise ValueError("max_distance must not be NaN")
    known = {x: score_threshold(x) for x in set(a.tolist())}       # (a batch usually shares a few distances)
    return np.array([known[x] for x in a.tolist()], dtype=np.float32)


def range_search_host(engine, q: np.ndarray, thr: np.ndarray, max_results: int, search_args: dict):
    """engines without rdx_index_range: the model over engine.search(k = rows of the engine)
    -> (scores f32 [nq][m], rows i64 [nq][m], counts i32 [nq], totals i64 [nq]), padded -inf / -1"""
    nq, m = q.shape[0], int(max_results)
    sc = np.full((nq, m), -np.inf, dtype=np.float32)
    ro = np.full((nq, m), -1, dtype=np.int64)
    cn = np.zeros(nq, dtype=np.int32)
    tt = np.zeros(nq, dtype=np.int64)
    n_rows = len(engine)
    if n_rows == 0:
        return sc, ro, cn, tt
    s, r, c = engine.search(q, n_rows, **search_args)
    for b in range(nq):
        ps, pr, total = range_model(s[b, : c[b]], r[b, : c[b]], thr[b], m)
        cn[b], tt[b] = len(pr), total
        sc[b, : len(pr)], ro[b, : len(pr)] = ps, pr
    return sc, ro, cn, tt
