"""Exact top-k grouped by a metadata key: `Collection.query_groups` / `query_groups_device`.

The reference turns chunks into documents by fetching n_docs*10 chunks (src/rag/retriever.py:202) and deduplicating them by document on
the host (src/rag/retriever.py:539-578): when the best chunks crowd into a few documents the caller gets fewer documents than asked
for. Here the grouping is part of the search and exact.

Definition. A = the rows that pass `where` and `where_document` and are not deleted. Rows without the key belong to no group and are
ignored. Two rows share a group when their values are equal and of the same kind (where.py's K_STR / K_INT / K_FLOAT / K_BOOL: 1 and
True are two groups; +0.0 and -0.0 are one). Rank A by (exact cosine score descending, row ascending) — the engine's documented order,
with the score bits query() returns. The result is the first G distinct groups met while walking that ranking, in that order, each
with its first m rows of the ranking, in that order. `grouped_topk_model` states it in numpy; the host path and the tests use it.

The device path is a ladder whose every rung proves its answer or hands the query on, so results never depend on the path:
  1. search_device with k1 and k_group_select. The list is a prefix of the ranking, so the first G groups of the list are the first G
     of the ranking as soon as the list holds G groups or is not full (it then holds all of A), and a group's members are final when
     the list holds min(m, |group|) of its rows or is not full.
  2. queries whose full list holds fewer than G groups ("short") are searched again with k2 = 4096 and cut again.
  3. queries still short go to brute force: one fill job per group (every group's best m rows), then the first G groups by (best
     score descending, best row ascending) — the order in which the ranking meets the groups.
  4. a winning group of a query that was not short whose members are not proven final becomes a fill job (k_group_fill: the group's
     rows from the CSR table, masked, exact scores, best m); its output replaces the group's members.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np

from . import where as W

MAX_GROUPS, MAX_GROUP_SIZE = 64, 16       # include/rdx.h RDX_GROUP_MAX_GROUPS / RDX_GROUP_MAX_SIZE
FILL_SPAN = 4096                          # include/rdx.h RDX_GROUP_FILL_SPAN: rows one fill job walks
K_FAST_MAX = 256                          # csrc/search_plan.hpp: the largest k of the scan path
K_SECOND = 4096                           # csrc/rows_core.hpp SELECT_MAX_K: the second fetch (the exact scan path)
STAT_KEYS = ("queries", "proven_first_fetch", "second_fetch", "brute", "fill_jobs")


def first_fetch_k(n_groups: int, group_size: int) -> int:
    """k of the first fetch: four times what the answer holds, at least 64, on the scan path (DESIGN.md §21 measures the choice)"""
    return min(K_FAST_MAX, max(64, 4 * n_groups * group_size))


def grouped_topk_model(ranked_scores, ranked_rows, row_group, n_groups: int, group_size: int):
    """The definition, for one query. ranked_scores / ranked_rows: the WHOLE ranking of the allowed rows (score descending, row
    ascending; entries with row < 0 are padding); row_group[r] = the group code of row r or -1.
    -> (codes int32 [g], [(scores float32 [<= m], rows int64 [<= m])] * g), g <= n_groups, in the order the ranking meets the groups."""
    rows = np.asarray(ranked_rows, dtype=np.int64)
    scores = np.asarray(ranked_scores, dtype=np.float32)
    keep = rows >= 0
    rows, scores = rows[keep], scores[keep]
    codes = np.asarray(row_group)[rows] if rows.size else np.zeros(0, dtype=np.int32)
    has = codes >= 0
    rows, scores, codes = rows[has], scores[has], codes[has]
    uniq, first = np.unique(codes, return_index=True)
    win = uniq[np.argsort(first, kind="stable")][:n_groups]
    members = []
    for c in win.tolist():
        at = np.flatnonzero(codes == c)[:group_size]
        members.append((scores[at], rows[at]))
    return win.astype(np.int32), members


class GroupTables:
    """What the grouped search needs to know about one metadata key of a collection, valid for one `write_count`:
      row_group  int32 [rows]        the row's group code, numbered by first appearance in row order; -1 = no key (or deleted)
      group_off  int64 [groups + 1]  and
      group_rows int64 [keyed rows]  the CSR of group -> rows, rows ascending within a group
      values     [groups]            the key's value per code
    built from the Column arrays (kind, code, num), never from per-row dicts. device() keeps a copy in HBM."""

    def __init__(self, collection, key: str):
        self.write_count = collection.write_count
        self.key = key
        n = collection._rows
        col = collection._cols.get(key)
        self.row_group = np.full(n, -1, dtype=np.int32)
        self.values: list = []
        if col is not None and n:
            kind = col.kind[:n]
            keyed = np.flatnonzero((kind != W.K_MISSING) & collection._alive[:n])
            if keyed.size:
                kd = kind[keyed].astype(np.int64)
                # one number per value: a string's vocabulary index, or the numeric payload (+ 0.0 puts -0.0 onto +0.0)
                val = np.where(kd == W.K_STR, col.code[keyed].astype(np.float64), col.num[keyed] + 0.0)
                order = np.lexsort((val, kd))                    # stable: rows stay ascending inside a run of equal keys
                sk, sv = kd[order], val[order]
                new = np.ones(order.size, dtype=bool)
                new[1:] = (sk[1:] != sk[:-1]) | (sv[1:] != sv[:-1])
                run = np.cumsum(new) - 1                         # the run (= group) of each sorted entry
                first_row = keyed[order[new]]                    # a run's first entry is its lowest row
                rank = np.empty(first_row.size, dtype=np.int64)
                rank[np.argsort(first_row, kind="stable")] = np.arange(first_row.size)   # codes by first appearance in row order
                self.row_group[keyed[order]] = rank[run].astype(np.int32)
                self.values = [col.get(int(r)) for r in np.sort(first_row)]
        keyed_rows = np.flatnonzero(self.row_group >= 0)
        by_group = np.argsort(self.row_group[keyed_rows], kind="stable")
        self.group_rows = keyed_rows[by_group].astype(np.int64)
        self.n_groups = len(self.values)
        self.group_off = np.zeros(self.n_groups + 1, dtype=np.int64)
        np.cumsum(np.bincount(self.row_group[keyed_rows], minlength=self.n_groups), out=self.group_off[1:])
        self._dev = None

    def device(self, dev):
        """(row_group, group_off, group_rows) as torch tensors on `dev`, uploaded once"""
        if self._dev is None or self._dev[0] != dev:
            import torch
            self._dev = (dev, torch.from_numpy(self.row_group).to(dev), torch.from_numpy(self.group_off).to(dev),
                         torch.from_numpy(self.group_rows).to(dev))
        return self._dev[1:]


def group_tables(collection, key: str) -> GroupTables:
    """the collection's GroupTables for `key`, rebuilt after any write (as fusion.row_tables)"""
    cache = collection._group_tables
    t = cache.get(key)
    if t is None or t.write_count != collection.write_count:
        if cache and next(iter(cache.values())).write_count != collection.write_count:
            cache.clear()                                        # tables of an older state of the rows: none is valid any more
        t = cache[key] = GroupTables(collection, key)
    return t


def grouped_search_host(engine, q: np.ndarray, tables: GroupTables, n_groups: int, group_size: int, search_args: dict):
    """engines without search_device: the full ranking from engine.search, then the model
    -> (scores f32 [nq][G][m], rows i64 [nq][G][m], counts i32 [nq][G], codes i32 [nq][G], n_found i32 [nq]), padded -inf / -1 / 0"""
    nq, G, m = q.shape[0], n_groups, group_size
    sc = np.full((nq, G, m), -np.inf, dtype=np.float32)
    ro = np.full((nq, G, m), -1, dtype=np.int64)
    cn = np.zeros((nq, G), dtype=np.int32)
    cd = np.full((nq, G), -1, dtype=np.int32)
    nf = np.zeros(nq, dtype=np.int32)
    total = len(engine)
    if total == 0 or tables.n_groups == 0:
        return sc, ro, cn, cd, nf
    s, r, c = engine.search(q, total, **search_args)
    for b in range(nq):
        codes, members = grouped_topk_model(s[b, : c[b]], r[b, : c[b]], tables.row_group, G, m)
        nf[b] = len(codes)
        cd[b, : len(codes)] = codes
        for g, (ms, mr) in enumerate(members):
            cn[b, g] = len(mr)
            sc[b, g, : len(mr)] = ms
            ro[b, g, : len(mr)] = mr
    return sc, ro, cn, cd, nf


def _split_jobs(job_query: List[int], job_code: List[int], group_off: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """(query, group) pairs -> fill jobs of at most FILL_SPAN rows: (job_query i32, job_begin i64, job_end i64, job_pair i64 = which
    pair a job is a part of)"""
    jq = np.asarray(job_query, dtype=np.int64)
    jc = np.asarray(job_code, dtype=np.int64)
    begin, end = group_off[jc], group_off[jc + 1]
    parts = np.maximum(1, (end - begin + FILL_SPAN - 1) // FILL_SPAN)
    pair = np.repeat(np.arange(jq.size, dtype=np.int64), parts)
    part = np.arange(pair.size, dtype=np.int64) - np.repeat(np.cumsum(parts) - parts, parts)
    jb = begin[pair] + part * FILL_SPAN
    je = np.minimum(jb + FILL_SPAN, end[pair])
    return jq[pair].astype(np.int32), jb, je, pair


def _fill_pairs(engine, q, mask, job_query, job_code, tables: GroupTables, group_rows_dev, m: int, stats: dict):
    """the best m allowed rows of every (query, group) pair -> (score f32 [pairs][m], row i64 [pairs][m], count i32 [pairs]) on the device.
    A group longer than FILL_SPAN is several jobs whose lists are merged here: the best m of their union, in the same order."""
    import torch
    from . import engine as E
    jq, jb, je, pair = _split_jobs(job_query, job_code, tables.group_off)
    stats["fill_jobs"] += int(jq.size)
    sc, ro, cn = E.group_fill(engine, q, jq, jb, je, group_rows_dev, m, mask=mask)
    n_pairs = len(job_query)
    if jq.size == n_pairs:                                      # no group was split: a job is its pair
        return sc, ro, cn
    dev = sc.device
    key = torch.from_numpy(pair).to(dev).repeat_interleave(m)   # the pair of every list entry
    fs, fr = sc.reshape(-1), ro.reshape(-1)
    live = fr >= 0
    key, fs, fr = key[live], fs[live], fr[live]
    o = torch.sort(fr, stable=True).indices                     # row ascending,
    o = o[torch.sort(fs[o], descending=True, stable=True).indices]      # then score descending (stable: ties keep the row order),
    o = o[torch.sort(key[o], stable=True).indices]              # then by pair: every pair's entries in ranking order
    key, fs, fr = key[o], fs[o], fr[o]
    per = torch.bincount(key, minlength=n_pairs)
    start = torch.cumsum(per, 0) - per
    pos = torch.arange(key.numel(), device=dev) - start[key]
    take = pos < m
    out_s = torch.full((n_pairs, m), float("-inf"), dtype=torch.float32, device=dev)
    out_r = torch.full((n_pairs, m), -1, dtype=torch.int64, device=dev)
    out_s[key[take], pos[take]] = fs[take]
    out_r[key[take], pos[take]] = fr[take]
    return out_s, out_r, torch.clamp(per, max=m).to(torch.int32)


def grouped_search_device(collection, q, tables: GroupTables, n_groups: int, group_size: int, mask, stats: Dict[str, int],
                          k_first: Optional[int] = None):
    """The ladder (module docstring) for queries q fp32 [nq][dim] on the collection's device.
    -> (scores f32 [nq][G][m], rows i64 [nq][G][m], counts i32 [nq][G], codes i32 [nq][G], n_found i32 [nq]) there, padded -inf / -1 / 0"""
    import torch
    from . import engine as E
    from ._lib import RdxError
    eng = collection._engine
    nq, G, m = int(q.shape[0]), n_groups, group_size
    dev = q.device
    stats["queries"] += nq
    if tables.n_groups == 0:                                    # a key no (live) row carries: empty results
        stats["proven_first_fetch"] += nq
        return (torch.full((nq, G, m), float("-inf"), dtype=torch.float32, device=dev), torch.full((nq, G, m), -1, dtype=torch.int64, device=dev),
                torch.zeros((nq, G), dtype=torch.int32, device=dev), torch.full((nq, G), -1, dtype=torch.int32, device=dev),
                torch.zeros(nq, dtype=torch.int32, device=dev))
    row_group, group_off, group_rows = tables.device(dev)

    def fetch(qq, k):
        """search + cut; the flags the host decides on come back in ONE copy: (short [n], complete [n][G], code [n][G])"""
        n = qq.shape[0]
        s = torch.empty((n, k), dtype=torch.float32, device=dev)
        r = torch.empty((n, k), dtype=torch.int64, device=dev)
        c = torch.empty((n,), dtype=torch.int32, device=dev)
        eng.search_device(qq, k, s, r, c, mask=mask)
        sel = E.group_select(s, r, c, row_group, group_off, G, m)
        flags = torch.cat([sel["bad"], sel["short"], sel["complete"].reshape(-1), sel["code"].reshape(-1)]).cpu().numpy()
        if flags[0]:
            raise RdxError("grouped search: a search returned a row the group tables do not cover")
        return sel, flags[1: 1 + n], flags[1 + n: 1 + n + n * G].reshape(n, G).copy(), flags[1 + n + n * G:].reshape(n, G).copy()

    k1 = int(k_first) if k_first is not None else first_fetch_k(G, m)
    sel, short_h, complete_h, code_h = fetch(q, k1)
    o_s, o_r, o_c, o_code, o_found = sel["score"], sel["row"], sel["count"], sel["code"], sel["found"]
    short = np.flatnonzero(short_h)
    stats["proven_first_fetch"] += nq - int(short.size)
    still = short
    if short.size:                                              # rung 2: the short queries alone, with the exact scan's k
        stats["second_fetch"] += int(short.size)
        short_t = torch.from_numpy(short).to(dev)
        sel2, short2_h, complete_h[short], code_h[short] = fetch(q[short_t].contiguous(), K_SECOND)
        for name, dst in (("score", o_s), ("row", o_r), ("count", o_c), ("code", o_code), ("found", o_found)):
            dst[short_t] = sel2[name]
        still = short[np.flatnonzero(short2_h)]
    if still.size:                                              # rung 3: brute force over every group
        nb_, ng = int(still.size), tables.n_groups
        stats["brute"] += nb_
        still_t = torch.from_numpy(still).to(dev)
        fs, fr, fc = _fill_pairs(eng, q, mask, np.repeat(still, ng), np.tile(np.arange(ng, dtype=np.int64), nb_), tables, group_rows, m, stats)
        fs, fr, fc = fs.reshape(nb_, ng, m), fr.reshape(nb_, ng, m), fc.reshape(nb_, ng)
        best_s, best_r = fs[:, :, 0], fr[:, :, 0]               # a group is met at its best row (-inf / -1: no allowed row)
        far = torch.where(best_r >= 0, best_r, torch.full_like(best_r, 2 ** 62))
        o = torch.sort(far, dim=1, stable=True).indices                                                  # best row ascending,
        o = torch.gather(o, 1, torch.sort(torch.gather(best_s, 1, o), dim=1, descending=True, stable=True).indices)   # then best score descending
        top = o[:, : min(G, ng)]
        g = top.shape[1]
        cnt = torch.gather(fc, 1, top)
        o_s[still_t] = float("-inf")
        o_r[still_t] = -1
        o_c[still_t] = 0
        o_code[still_t] = -1
        o_s[still_t, :g] = torch.gather(fs, 1, top[:, :, None].expand(-1, -1, m))
        o_r[still_t, :g] = torch.gather(fr, 1, top[:, :, None].expand(-1, -1, m))
        o_c[still_t, :g] = cnt
        o_code[still_t, :g] = torch.where(cnt > 0, top.to(torch.int32), torch.full_like(cnt, -1))
        o_found[still_t] = (cnt > 0).sum(dim=1).to(torch.int32)
        complete_h[still] = 1
    nb, ng_ = np.nonzero(complete_h == 0)                       # rung 4: winning groups whose members the list did not prove
    if nb.size:
        fs, fr, fc = _fill_pairs(eng, q, mask, nb, code_h[nb, ng_].astype(np.int64), tables, group_rows, m, stats)
        at = torch.from_numpy(nb * G + ng_).to(dev)             # the (query, group) slots, flat
        o_s.view(nq * G, m)[at] = fs
        o_r.view(nq * G, m)[at] = fr
        o_c.view(nq * G)[at] = fc
    return o_s, o_r, o_c, o_code, o_found
