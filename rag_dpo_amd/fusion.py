"""Rank fusion on the GPU for batches of questions: the host half of `rdx_fuse_rankings` (include/rdx.h).

`DenseRetriever._fuse` joins the dense and the BM25 rankings of ONE question in Python, over objects built for every hit. Here the
rankings of a whole batch of questions are packed as arrays, fused by one kernel launch (one workgroup per question) and only the
winners come back: one device-to-host copy, and host objects for at most n_candidates chunks per question. `_fuse` is the model:
the kernel computes its order and every one of its floats, bit for bit. This module packs the lists, calls the kernel and unpacks
the winners; it does no arithmetic.

Keys. What identifies a chunk across lists is its collection row: a dense hit's row as `query_device` returns it, a BM25 hit's
`collection.rows_of([chunk id])`. A BM25 hit whose id the collection no longer holds (deleted since the index was built) cannot meet a
dense hit; it gets the negative key -2 - (its BM25 row), distinct from every other chunk's. -1 is padding.

The row -> document group table (what the summary pre-filter looks at) is the `document_path` column interned in first-appearance
order; it describes one state of the rows and is rebuilt whenever `collection.write_count` has moved."""
from __future__ import annotations

import ctypes
import json
from dataclasses import dataclass
from itertools import chain
from typing import Any, Dict, List, Optional, Sequence

import numpy as np

from . import _lib as L
from .retriever import RetrievedChunk

MAX_LISTS, MAX_LIST_ENTRIES, MAX_ENTRIES = L.FUSE_MAX_LISTS, L.FUSE_MAX_LIST_ENTRIES, L.FUSE_MAX_ENTRIES
DENSE, BM25 = L.FUSE_DENSE, L.FUSE_BM25
RRF_K = 60          # reference src/rag/retriever.py:66 (reciprocal_rank_fusion's k)


def fits(n_lists: int, list_stride: int, top_n: int) -> bool:
    """the kernel's limits (include/rdx.h): lists per question, entries per list, entries per question, winners per question"""
    return (1 <= n_lists <= MAX_LISTS and 1 <= list_stride <= MAX_LIST_ENTRIES and n_lists * list_stride <= MAX_ENTRIES
            and 1 <= top_n <= MAX_ENTRIES)


class PackedLists:
    """the ranked lists of nq questions in rdx_fuse_rankings' layout (host arrays): question q's lists are [q][0 .. n_lists) in the order
    _fuse visits them; a list that was never set is absent (count -1)"""

    def __init__(self, nq: int, n_lists: int, list_stride: int):
        if nq < 0 or not fits(n_lists, list_stride, 1):
            raise ValueError(f"{n_lists} lists of {list_stride} entries are beyond rdx_fuse_rankings' limits "
                             f"({MAX_LISTS} lists, {MAX_LIST_ENTRIES} entries per list, {MAX_ENTRIES} per question)")
        self.nq, self.n_lists, self.list_stride = nq, n_lists, list_stride
        self.kind = np.zeros((nq, n_lists), np.int32)
        self.weight = np.zeros((nq, n_lists), np.float64)
        self.count = np.full((nq, n_lists), -1, np.int32)
        self.keys = np.full((nq, n_lists, list_stride), -1, np.int64)
        self.dist = np.zeros((nq, n_lists, list_stride), np.float32)
        self.score = np.zeros((nq, n_lists, list_stride), np.float64)
        self.filter_on = np.zeros(nq, np.int32)
        self.group_words = 1
        self.allow = np.zeros((nq, 1), np.uint32)

    def set_list(self, q: int, l: int, kind: int, weight: float, keys: Sequence[int], values: Sequence[float]):
        """values: the fp32 distances of a dense list, the fp64 scores of a BM25 one"""
        n = len(keys)
        if n > self.list_stride or len(values) != n or kind not in (DENSE, BM25):
            raise ValueError("set_list: more entries than list_stride, or keys and values of different lengths, or an unknown kind")
        self.kind[q, l], self.weight[q, l], self.count[q, l] = kind, weight, n
        self.keys[q, l, :n] = keys
        (self.dist if kind == DENSE else self.score)[q, l, :n] = values

    def set_filter(self, q: int, allowed_groups: Sequence[int], n_groups: int):
        """question q's dense lists are filtered: only keys whose group is in allowed_groups pass"""
        self.set_filters({q: allowed_groups}, n_groups)

    def set_filters(self, allowed: Dict[int, Sequence[int]], n_groups: int):
        """set_filter for every question q of `allowed` (q -> its allowed groups), the bits of all of them OR-ed in at once"""
        if not allowed:
            return
        words = max(1, (int(n_groups) + 31) // 32)
        if words > self.group_words:
            grown = np.zeros((self.nq, words), np.uint32)
            grown[:, : self.group_words] = self.allow
            self.allow, self.group_words = grown, words
        qs = np.fromiter(allowed, dtype=np.int64, count=len(allowed))
        sizes = np.fromiter(map(len, allowed.values()), dtype=np.int64, count=len(allowed))
        groups = np.fromiter(chain.from_iterable(allowed.values()), dtype=np.int64, count=int(sizes.sum()))
        self.filter_on[qs] = 1
        self.allow[qs] = 0
        np.bitwise_or.at(self.allow, (np.repeat(qs, sizes), groups >> 5), np.left_shift(np.uint32(1), (groups & 31).astype(np.uint32)))

    def lists_of(self, q: int):
        """-> per list None (absent) or (kind, weight, keys, values): what set_list was given"""
        out = []
        for l in range(self.n_lists):
            n = int(self.count[q, l])
            if n < 0:
                out.append(None)
                continue
            kind = int(self.kind[q, l])
            vals = (self.dist if kind == DENSE else self.score)[q, l, :n]
            out.append((kind, float(self.weight[q, l]), self.keys[q, l, :n].tolist(), vals.tolist()))
        return out

    def allowed_groups_of(self, q: int) -> Optional[List[int]]:
        if not self.filter_on[q]:
            return None
        bits = np.unpackbits(self.allow[q].view(np.uint8), bitorder="little")
        return np.flatnonzero(bits).tolist()


@dataclass
class Winner:
    """one fused chunk as the kernel returns it: its key, _fuse's four floats and the input position of its first appearance"""
    key: int
    distance: float
    semantic_score: float
    bm25_score: float
    hybrid_score: float
    first_list: int
    first_rank: int


_OUT = (("key", np.int64), ("semantic", np.float64), ("bm25", np.float64), ("hybrid", np.float64), ("distance", np.float32),
        ("list", np.int32), ("rank", np.int32))


def _out_layout(nq: int, top_n: int):
    """byte offsets of the outputs inside one buffer (8-byte fields first): one device-to-host copy brings all of them"""
    off, lay = 0, {}
    for name, dt in _OUT:
        lay[name] = (off, np.dtype(dt), (nq, top_n))
        off += nq * top_n * np.dtype(dt).itemsize
    lay["count"] = (off, np.dtype(np.int32), (nq,))
    off += nq * 4
    return lay, off


def unpack(buf: np.ndarray, nq: int, top_n: int) -> List[List[Winner]]:
    """the output buffer of an rdx_fuse_rankings call (laid out by _out_layout) -> per question its winners, best first"""
    lay, _ = _out_layout(nq, top_n)
    a = {name: np.frombuffer(buf, dtype=dt, count=int(np.prod(shape)), offset=off).reshape(shape) for name, (off, dt, shape) in lay.items()}
    out = []
    for q in range(nq):
        c = int(a["count"][q])
        cols = [a[name][q, :c].tolist() for name in ("key", "distance", "semantic", "bm25", "hybrid", "list", "rank")]
        out.append([Winner(*t) for t in zip(*cols)])
    return out


def call_kernel(lib, device: int, nq: int, n_lists: int, stride: int, p: Dict[str, int], n_rows: int, group_words: int, min_semantic: int,
          bm25_keep_max: bool, top_n: int, out_base: int, space: int, stream: int):
    lay, _ = _out_layout(nq, top_n)
    o = {name: ctypes.c_void_p(out_base + off) for name, (off, _, _) in lay.items()}
    vp = lambda x: ctypes.c_void_p(x) if x else None
    L.check(lib.rdx_fuse_rankings(int(device), int(nq), int(n_lists), int(stride), vp(p["kind"]), vp(p["weight"]), vp(p["count"]),
                                  vp(p["keys"]), vp(p["dist"]), vp(p["score"]), vp(p.get("row_group")), int(n_rows),
                                  vp(p.get("filter_on")), vp(p.get("allow")), int(group_words), int(min_semantic),
                                  1 if bm25_keep_max else 0, RRF_K, int(top_n), o["key"], o["distance"], o["semantic"], o["bm25"],
                                  o["hybrid"], o["list"], o["rank"], o["count"], space, vp(stream)))


def fuse_host(packed: PackedLists, row_group: Optional[np.ndarray], min_semantic: int, bm25_keep_max: bool, top_n: int,
              device: int = 0) -> List[List[Winner]]:
    """rdx_fuse_rankings on host arrays (RDX_HOST: staged through the device by the library, complete on return)"""
    lib = L.load(require_gpu=True)
    lay, nbytes = _out_layout(packed.nq, top_n)
    out = np.zeros(max(nbytes, 8), np.uint8)
    if packed.nq == 0:
        return []
    rg = np.ascontiguousarray(row_group, np.int32) if row_group is not None else np.zeros(0, np.int32)
    filt = bool(packed.filter_on.any())
    p = {"kind": packed.kind.ctypes.data, "weight": packed.weight.ctypes.data, "count": packed.count.ctypes.data,
         "keys": packed.keys.ctypes.data, "dist": packed.dist.ctypes.data, "score": packed.score.ctypes.data}
    if filt:
        p.update(row_group=rg.ctypes.data if rg.size else 0, filter_on=packed.filter_on.ctypes.data, allow=packed.allow.ctypes.data)
    call_kernel(lib, device, packed.nq, packed.n_lists, packed.list_stride, p, rg.size, packed.group_words, min_semantic, bm25_keep_max,
          top_n, out.ctypes.data, L.RDX_HOST, 0)
    return unpack(out, packed.nq, top_n)


# ---- the tables derived from a collection's rows ---------------------------------------------------------------------------------
class RowTables:
    """what the fusion needs to know about a collection's rows, valid for one `write_count`: the row -> document group table (host
    and device) and, per BM25 index, the BM25 row -> key table"""

    def __init__(self, collection, device=None):
        self.write_count = collection.write_count
        paths = collection.column_values("document_path", "")
        self.group_of: Dict[Any, int] = {}
        for p in paths:                                         # first-appearance order
            if p not in self.group_of:
                self.group_of[p] = len(self.group_of)
        self.row_group = np.fromiter(map(self.group_of.__getitem__, paths), dtype=np.int32, count=len(paths))
        self.n_groups = len(self.group_of)
        self.row_group_device = None
        if device is not None:
            import torch
            self.row_group_device = torch.from_numpy(self.row_group).to(device)
        self._bm25_keys: Dict[int, np.ndarray] = {}

    def groups_allowed(self, doc_filter) -> List[int]:
        return [g for g in (self.group_of.get(p) for p in doc_filter) if g is not None]

    def bm25_keys(self, collection, index) -> np.ndarray:
        """int64 [BM25 rows]: the key of each chunk of a ChunkBM25Index"""
        ent = self._bm25_keys.get(id(index))
        if ent is None or ent.shape[0] != len(index.chunk_ids):
            ent = np.asarray(collection.rows_of(index.chunk_ids), dtype=np.int64).reshape(-1)
            gone = np.flatnonzero(ent < 0)
            ent[gone] = -2 - gone
            self._bm25_keys[id(index)] = ent
        return ent


def row_tables(collection, device=None) -> RowTables:
    """the collection's RowTables, rebuilt after any write"""
    t = getattr(collection, "_fusion_tables", None)
    if t is None or t.write_count != collection.write_count or (device is not None and t.row_group_device is None):
        t = RowTables(collection, device)
        collection._fusion_tables = t
    return t


# ---- DenseRetriever.retrieve_candidates_batch on the device ------------------------------------------------------------------------
def device_ready(retriever) -> bool:
    """whether the batch can run on the device at all: librdx with a GPU, a collection whose engine searches from device pointers"""
    try:
        L.load(require_gpu=True)
    except L.RdxUnavailable:
        return False
    col = retriever.collection
    eng = getattr(col, "_engine", None)
    return eng is not None and hasattr(eng, "search_device") and hasattr(col, "query_device") and hasattr(col, "rows_of")


def _where_key(where) -> str:
    return json.dumps(where, sort_keys=True, ensure_ascii=False, default=repr)


def _embed_device(provider, texts: List[str], device):
    """the vectors `provider.embed(texts)` returns, on the device: embed_device's raw rows normalised by the step embed() ends with
    (rdx_l2_normalize) — query_device then sees what query() sees — or, for a provider without embed_device, embed()'s rows uploaded"""
    import torch
    if hasattr(provider, "embed_device"):
        raw = provider.embed_device(texts).to(device=device, dtype=torch.float32).contiguous()
        out = torch.empty_like(raw)
        lib = L.load(require_gpu=True)
        stream = torch.cuda.current_stream(raw.device).cuda_stream
        L.check(lib.rdx_l2_normalize(raw.device.index or 0, ctypes.c_void_p(raw.data_ptr()), raw.shape[0], raw.shape[1],
                                     ctypes.c_void_p(out.data_ptr()), L.RDX_DEVICE, ctypes.c_void_p(stream)))
        return out
    return torch.tensor(np.asarray(provider.embed(texts), dtype=np.float32), device=device)


def dense_lists(col, vectors, sub_wheres: List[Any], n_fetch: int):
    """the dense lists of the batch's sub-queries (`vectors`, a tensor of one row each, sub-query t under sub_wheres[t]) -> (distances,
    rows, counts) on the vectors' device. One search for the whole batch: query_device when the sub-queries share their `where`, else
    query_filtered_device with every sub-query under its own; a collection without it is asked once per distinct `where`."""
    import torch
    by_where: Dict[str, List[int]] = {}
    for t, w in enumerate(sub_wheres):
        by_where.setdefault(_where_key(w), []).append(t)
    if len(by_where) == 1:
        return col.query_device(vectors, n_results=n_fetch, where=sub_wheres[0])
    if hasattr(col, "query_filtered_device"):
        try:
            return col.query_filtered_device(vectors, sub_wheres, n_results=n_fetch)
        except NotImplementedError:      # an "ip" / "l2" collection: refused before anything ran; the loop serves it as it always did
            pass
    device = vectors.device
    d_dist = torch.empty((len(sub_wheres), n_fetch), dtype=torch.float32, device=device)
    d_rows = torch.empty((len(sub_wheres), n_fetch), dtype=torch.int64, device=device)
    d_cnt = torch.empty((len(sub_wheres),), dtype=torch.int32, device=device)
    for ts in by_where.values():
        idx = torch.as_tensor(ts, dtype=torch.int64, device=device)
        dd, rr, cc = col.query_device(vectors.index_select(0, idx), n_results=n_fetch, where=sub_wheres[ts[0]])
        d_dist[idx], d_rows[idx], d_cnt[idx] = dd, rr, cc
    return d_dist, d_rows, d_cnt


def retrieve_candidates_device(r, expanded: List[tuple], n_candidates: int, wheres: List[Any]) -> List[List[RetrievedChunk]]:
    """retrieve_candidates of every question, given as DenseRetriever._expand's (main query, sub-queries) and all inside the kernel's
    limits, fused by one launch. Raises whatever the batched device calls raise: the caller falls back to the per-question path."""
    import torch
    nq = len(expanded)
    if nq == 0:
        return []
    col, lib = r.collection, L.load(require_gpu=True)
    n_fetch = max(n_candidates, 50)
    doc_filters = r._doc_filters([e for e, _ in expanded])
    hybrid = r._hybrid()
    per_sub = 2 if hybrid else 1
    n_lists = per_sub * max(len(subs) for _, subs in expanded)
    device = torch.device("cuda", col._engine.device)
    tables = row_tables(col, device)
    packed = PackedLists(nq, n_lists, n_fetch)

    # the sub-queries of the batch, flattened: sub-query t is question sub_q[t]'s sub_i[t]-th
    texts = [s for _, subs in expanded for s in subs]
    sub_q = [q for q, (_, subs) in enumerate(expanded) for _ in subs]
    sub_i = [i for _, subs in expanded for i in range(len(subs))]
    dense_slot = np.asarray([q * n_lists + per_sub * i for q, i in zip(sub_q, sub_i)], dtype=np.int64)
    for q, i in zip(sub_q, sub_i):
        packed.kind[q, per_sub * i], packed.weight[q, per_sub * i] = DENSE, (2.0 if i == 0 else 1.0)      # reference :209, :374

    with torch.cuda.device(device):
        vectors = _embed_device(r.embedding_provider, texts, device)
        d_dist, d_rows, d_cnt = dense_lists(col, vectors, [wheres[q] for q in sub_q], n_fetch)

        # BM25 of every sub-query, each under its question's summary filter: one device call; the hits stay arrays
        bm_rows = None
        if hybrid:
            bm_rows = np.full((nq * n_lists, n_fetch), -1, np.int64)
            keymap = tables.bm25_keys(col, r.chunk_bm25)
            keys2, score2, count1 = packed.keys.reshape(nq * n_lists, n_fetch), packed.score.reshape(nq * n_lists, n_fetch), packed.count.reshape(-1)
            slots = dense_slot + 1
            packed.kind.reshape(-1)[slots] = BM25
            packed.weight.reshape(-1)[slots] = [2.0 * 1.5 if i == 0 else 1.0 * 0.75 for i in sub_i]                 # reference :421, :430
            count1[slots] = 0                                                        # searched: present, maybe empty
            live, sc, ro, cn = r.chunk_bm25.search_batch_arrays(texts, top_k=n_fetch, doc_filters=[doc_filters[q] for q in sub_q])
            if len(live):
                ls, k = slots[live], ro.shape[1]
                bm_rows[ls, :k] = ro
                keys2[ls, :k] = np.where(ro >= 0, keymap[np.maximum(ro, 0)], -1)
                score2[ls, :k] = sc
                count1[ls] = cn
        # (an empty filter filters nothing: reference :226, :391)
        packed.set_filters({q: tables.groups_allowed(f) for q, f in enumerate(doc_filters) if f}, tables.n_groups)

        # one upload: every host array in one buffer (8-byte fields first)
        parts = [("keys", packed.keys), ("score", packed.score), ("weight", packed.weight), ("slot", dense_slot), ("kind", packed.kind),
                 ("count", packed.count), ("filter_on", packed.filter_on), ("allow", packed.allow)]
        offs, total = {}, 0
        for name, arr in parts:
            offs[name] = total
            total += (arr.nbytes + 7) & ~7
        host = np.zeros(total, np.uint8)
        for name, arr in parts:
            host[offs[name]: offs[name] + arr.nbytes] = np.ascontiguousarray(arr).reshape(-1).view(np.uint8)
        dev = torch.from_numpy(host).to(device)
        width = {torch.int64: 8, torch.int32: 4}
        view = lambda name, dt, n: dev[offs[name]: offs[name] + n * width[dt]].view(dt)
        keys_d = view("keys", torch.int64, packed.keys.size).view(nq * n_lists, n_fetch)
        count_d = view("count", torch.int32, packed.count.size)
        slot_d = view("slot", torch.int64, dense_slot.size)
        dist_d = torch.zeros((nq * n_lists, n_fetch), dtype=torch.float32, device=device)
        keys_d.index_copy_(0, slot_d, d_rows)                                       # the dense hits never leave the device
        dist_d.index_copy_(0, slot_d, d_dist)
        count_d.index_copy_(0, slot_d, d_cnt)

        top_n = min(n_candidates, MAX_ENTRIES)
        _, out_bytes = _out_layout(nq, top_n)
        out_d = torch.empty(out_bytes, dtype=torch.uint8, device=device)
        p = {k: dev.data_ptr() + offs[k] for k in ("keys", "score", "weight", "kind", "count")}
        p["dist"] = dist_d.data_ptr()
        if packed.filter_on.any():
            p.update(filter_on=dev.data_ptr() + offs["filter_on"], allow=dev.data_ptr() + offs["allow"],
                     row_group=tables.row_group_device.data_ptr() if tables.row_group.size else 0)
        call_kernel(lib, device.index, nq, n_lists, n_fetch, p, tables.row_group.size, packed.group_words, 10, True, top_n,
              out_d.data_ptr(), L.RDX_DEVICE, torch.cuda.current_stream(device).cuda_stream)
        winners = unpack(out_d.cpu().numpy(), nq, top_n)                            # the one device-to-host copy

    # host objects for the winners only
    dense_rows = [w.key for ws in winners for w in ws if not (hybrid and w.first_list % 2 == 1)]
    ids, docs, metas = col.payload_of(dense_rows)
    payload = dict(zip(dense_rows, zip(ids, docs, metas)))
    out: List[List[RetrievedChunk]] = []
    for q, ws in enumerate(winners):
        chunks = []
        for w in ws:
            if hybrid and w.first_list % 2 == 1:                                    # first seen by BM25: the index's text and metadata
                res = r.chunk_bm25.result_of(int(bm_rows[q * n_lists + w.first_list, w.first_rank]), w.bm25_score)
                chunk_id, meta = res.doc_key, dict(res.metadata)
                text = meta.pop("text", "")
            else:
                chunk_id, text, meta = payload[w.key]
                meta = dict(meta) if meta else {}
            chunks.append(RetrievedChunk(
                chunk_id=chunk_id, text=text, document_path=meta.get("document_path", ""),
                chunk_nature=meta.get("chunk_nature", "UNKNOWN"), chunk_index=meta.get("chunk_index", 0),
                confidence=meta.get("confidence", "unknown"), distance=w.distance, metadata=meta, bm25_score=w.bm25_score,
                semantic_score=w.semantic_score, hybrid_score=w.hybrid_score))
        out.append(chunks)
    return out
