"""Diversity-aware top-k (maximal marginal relevance, MMR): `Collection.query_mmr` / `query_mmr_device`.

A plain search of a corpus of near-duplicate chunks returns the same passage k times. `query_groups` helps when the duplicates share a
metadata key; MMR needs none: it picks, one by one, the candidate that is close to the query and far from what is already picked.

Definition, per query, with lambda = lambda_mult in [0, 1], k = n_results, F = fetch_k >= k:
  candidates  the first F entries of the exact ranking of the allowed rows (cosine score descending, row ascending; fp32 scores s):
              what query(n_results=F) returns. n <= F entries; "position" = index in this list.
  p(i, j)     fp32: the engine's exact score with the stored (normalised) row of candidate j as the query and the row of candidate i
              as the corpus row. Lane l of 64 adds the products of float4 groups l, l + 64, ... (x, y, z, w within a group) into one
              fp64 accumulator, the lanes meet by the xor butterfly 32 .. 1, one rounding to fp32 (`pair_scores`). Symmetric bit for bit.
  picks       pick 0 is position 0, value lambda * (double)s_0. Every later pick is the unpicked position i with the largest
              v_i = a - b, a = lambda * (double)s_i, b = (1.0 - lambda) * (double)m_i, m_i = the fp32 maximum of p(i, j) over the
              picked j: three fp64 operations, each rounded once. Ties go to the smaller position. min(k, n) picks.
Results come in pick order, each with its row, its query score and its value v. lambda = 1 returns query(n_results=k); the result
depends on the candidate list alone. `mmr_model` states it in numpy; the host path and the tests use it. The device path is one
search_device with k = F and one launch of k_mmr (csrc/mmr_kernel.hpp), which returns the model's picks and floats bit for bit.
"""
from __future__ import annotations

import numpy as np

MAX_FETCH, MAX_K = 1024, 64               # include/rdx.h RDX_MMR_MAX_FETCH / RDX_MMR_MAX_K


def pair_scores(rows_hat, row_hat) -> np.ndarray:
    """p(i, j) for every row i of rows_hat [n][dim] against the row row_hat [dim] (both stored, normalised rows; dim % 4 == 0) -> fp32 [n],
    in the lane order of the engine's exact score (not spaces.ordered_sum, whose partial sums take elements, not float4 groups)"""
    c = np.ascontiguousarray(rows_hat, dtype=np.float32)
    q = np.ascontiguousarray(row_hat, dtype=np.float32)
    n, dim = c.shape
    if q.shape != (dim,) or dim % 4:
        raise ValueError("pair_scores wants [n][dim] rows and a [dim] row, dim a multiple of 4")
    n4 = dim // 4
    prod = (q.astype(np.float64)[None, :] * c.astype(np.float64)).reshape(n, n4, 4)   # a product of two floats is exact in fp64
    acc = np.zeros((n, 64), dtype=np.float64)
    for g0 in range(0, n4, 64):                                  # lane l's next group is g0 + l, where the row has one
        lanes = min(64, n4 - g0)
        for e in range(4):
            acc[:, :lanes] += prod[:, g0: g0 + lanes, e]
    lane = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lane ^ m]
    return acc[:, 0].astype(np.float32)


def mmr_model(cand_scores, cand_rows, rows_hat, n_results: int, lambda_mult: float):
    """The definition, for one query. cand_scores fp32 / cand_rows int64 [n]: the candidate list (entries with row < 0 are padding and
    are never picked); rows_hat [n][dim]: the stored row of every entry (anything for padding).
    -> (pos int32 [g], rows int64 [g], scores fp32 [g], values fp64 [g]) in pick order, g = min(n_results, live entries)."""
    s = np.asarray(cand_scores, dtype=np.float32)
    r = np.asarray(cand_rows, dtype=np.int64)
    lam = np.float64(lambda_mult)
    one_minus = np.float64(1.0) - lam
    free = r >= 0
    m = np.full(s.shape, -np.inf, dtype=np.float32)
    pos, val = [], []
    a = lam * s.astype(np.float64)
    while len(pos) < n_results and free.any():
        if not pos:
            pick = int(np.flatnonzero(free)[0])
            v_pick = a[pick]
        else:
            p = pair_scores(rows_hat, rows_hat[pos[-1]])
            m = np.where(p > m, p, m)
            v = a - one_minus * m.astype(np.float64)
            v_free = np.where(free, v, -np.inf)
            best = v_free[free].max()
            pick = int(np.flatnonzero(free & (v_free == best))[0])   # ties: the smaller position
            v_pick = v[pick]
        pos.append(pick)
        val.append(v_pick)
        free[pick] = False
    pos_a = np.asarray(pos, dtype=np.int32)
    return pos_a, r[pos_a], s[pos_a], np.asarray(val, dtype=np.float64)


def _padded(nq: int, k: int):
    return (np.full((nq, k), -np.inf, dtype=np.float32), np.full((nq, k), -1, dtype=np.int64),
            np.full((nq, k), -np.inf, dtype=np.float64), np.zeros(nq, dtype=np.int32))


def mmr_search_host(engine, q: np.ndarray, n_results: int, fetch_k: int, lambda_mult: float, search_args: dict):
    """engines without search_device: engine.search with k = fetch_k, engine.get of the candidates' rows, then the model
    -> (scores f32 [nq][k], rows i64 [nq][k], values f64 [nq][k], counts i32 [nq]), padded -inf / -1 / -inf"""
    nq, k = q.shape[0], int(n_results)
    sc, ro, va, cn = _padded(nq, k)
    if len(engine) == 0:
        return sc, ro, va, cn
    s, r, c = engine.search(q, int(fetch_k), **search_args)
    for b in range(nq):
        n = int(c[b])
        if n == 0:
            continue
        _, pr, ps, pv = mmr_model(s[b, :n], r[b, :n], engine.get(r[b, :n]), k, lambda_mult)
        g = len(pr)
        cn[b] = g
        sc[b, :g], ro[b, :g], va[b, :g] = ps, pr, pv
    return sc, ro, va, cn


def mmr_search_device(engine, q, n_results: int, fetch_k: int, lambda_mult: float, mask):
    """queries q fp32 [nq][dim] on the engine's device: one search with k = fetch_k, one launch of the selection; nothing visits the host,
    the lists' counts included -> (scores f32 [nq][k], rows i64 [nq][k], values f64 [nq][k], counts i32 [nq], bad i32 [1]) there, padded
    -inf / -1 / -inf. `bad` is the selection's flag for a listed row the index does not hold: the lists are this engine's own answers,
    so it stays 0; a caller that copies the results to the host anyway (query_mmr) reads it with them."""
    import torch
    from . import engine as E
    nq, F = int(q.shape[0]), int(fetch_k)
    dev = q.device
    s = torch.empty((nq, F), dtype=torch.float32, device=dev)
    r = torch.empty((nq, F), dtype=torch.int64, device=dev)
    c = torch.empty((nq,), dtype=torch.int32, device=dev)
    engine.search_device(q, F, s, r, c, mask=mask)
    out = E.mmr_select(engine, s, r, c, int(n_results), lambda_mult)
    return out["score"], out["row"], out["value"], out["count"], out["bad"]
