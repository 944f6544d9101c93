"""Exact value counts (Collection.facets / count(where=...) / query_facets): the definitions, in numpy, and the host path.

How many rows carry each value of a metadata key. The reference asks it with one full id list per value
(src/processing/create_chromadb_index.py:447-480: len(collection.get(where={...}, limit=100000)["ids"]), wrong above 100 000 rows) and
by counting fetched metadata in a Python dict (pages/3_Documents.py:97-137).

code[r] = groups.GroupTables(key).row_group[r]: the rank of the row's value by first appearance in row order, -1 for a row without the
key and for a deleted row; G = the number of distinct values. `allowed` = the rows that `where`, `where_document` and the tombstones leave.

Corpus facets (facet_counts_model): counts[c] = allowed rows with code c; missing = allowed rows with code -1; total = allowed rows =
counts.sum() + missing.

Query facets (query_facets_model): for a query with score threshold t (range_search.score_threshold(max_distance): the very float
query_range compares with) the rows in range are the allowed rows whose exact fp32 score is >= t — the rows query_range counts in
`totals`. counts[c] / missing count those rows by code, total is their number, n_values the codes with a non-zero count.

Listing order (facet_order), both forms: the values with a non-zero count, count descending, then code ascending (the value that
appears first in the rows first); `limit` cuts the list; padding is code -1, count 0.

Integers throughout: the results do not depend on the path, the batch, the chunking or the schedule, and are compared for equality.
"""
from __future__ import annotations

import numpy as np

from . import _lib as L

MAX_LIMIT = L.FACET_MAX_LIMIT
STAT_KEYS = ("calls", "calls_host", "queries", "mfma", "exact", "host")


def facet_counts_model(row_group, n_groups: int, allowed=None):
    """row_group int32 [rows] (-1 or a code < n_groups), allowed bool [rows] or None (every row) -> (counts int64 [n_groups], missing, total)"""
    code = np.asarray(row_group, dtype=np.int64)
    if allowed is not None:
        code = code[np.asarray(allowed, dtype=bool)[: code.shape[0]]]
    if code.size and (code.min() < -1 or code.max() >= n_groups):
        raise ValueError(f"row_group holds a code outside -1 .. n_groups - 1 = {n_groups - 1}")
    keyed = code[code >= 0]
    counts = np.bincount(keyed, minlength=int(n_groups)).astype(np.int64)
    return counts, int(code.size - keyed.size), int(code.size)


def facet_order(counts, limit=None):
    """counts int64 [G] -> (codes int32 [n], counts int64 [n], n_values): the non-zero cells by (count descending, code ascending), the
    first `limit` of them (None: all)"""
    c = np.asarray(counts, dtype=np.int64)
    codes = np.flatnonzero(c > 0)
    codes = codes[np.lexsort((codes, -c[codes]))]
    n_values = int(codes.size)
    if limit is not None:
        codes = codes[: int(limit)]
    return codes.astype(np.int32), c[codes], n_values


def query_facets_model(ranked_scores, ranked_rows, row_group, n_groups: int, t):
    """one query's ranking of the allowed rows (scores f32, rows i64; every allowed row, padding rows < 0 ignored) and its score
    threshold t -> (counts int64 [n_groups], missing, total) of the rows with score >= t"""
    s = np.asarray(ranked_scores, dtype=np.float32)
    r = np.asarray(ranked_rows, dtype=np.int64)
    rows = r[(r >= 0) & (s >= np.float32(t))]
    return facet_counts_model(np.asarray(row_group)[rows], n_groups)


def pad_listing(counts, limit: int):
    """counts int64 [G] -> (codes int32 [limit], counts int64 [limit], n_values): facet_order, padded with -1 / 0"""
    codes, cnt, n_values = facet_order(counts, limit)
    oc = np.full(int(limit), -1, dtype=np.int32)
    on = np.zeros(int(limit), dtype=np.int64)
    oc[: codes.size], on[: codes.size] = codes, cnt
    return oc, on, n_values


def query_facets_host(engine, q: np.ndarray, thr: np.ndarray, row_group, n_groups: int, limit: int, search_args: dict):
    """engines without librdx's rdx_index_range_facets: the model over engine.search(k = rows of the engine)
    -> (codes i32 [nq][limit], counts i64 [nq][limit], n_values i32 [nq], missing i64 [nq], totals i64 [nq]), padded -1 / 0"""
    nq, m = q.shape[0], int(limit)
    oc = np.full((nq, m), -1, dtype=np.int32)
    on = np.zeros((nq, m), dtype=np.int64)
    nv = np.zeros(nq, dtype=np.int32)
    mis = np.zeros(nq, dtype=np.int64)
    tot = np.zeros(nq, dtype=np.int64)
    n_rows = len(engine)
    if n_rows == 0:
        return oc, on, nv, mis, tot
    s, r, c = engine.search(q, n_rows, **search_args)
    for b in range(nq):
        counts, mis[b], tot[b] = query_facets_model(s[b, : c[b]], r[b, : c[b]], row_group, n_groups, thr[b])
        oc[b], on[b], nv[b] = pad_listing(counts, m)
    return oc, on, nv, mis, tot
