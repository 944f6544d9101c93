"""Chroma-shaped `Collection` / `PersistentClient` whose vectors live in MI355X HBM (librdx).

Mirrors exactly the part of chromadb's API that RAG-DPO calls:
    collection.query(query_embeddings=, n_results=, where=, include=)   src/rag/retriever.py:215-220, 380-385
    collection.add(ids=, documents=, embeddings=, metadatas=)           src/processing/create_chromadb_index.py:374-379
    collection.get(limit=, offset=, where=, ids=, include=)             src/rag/bm25_index.py:211-215 and others
    collection.count() / delete(ids=) / update(ids=, metadatas=)        ingest_enterprise.py:272, tag_all_chunks.py:215
    client.get_collection / create_collection / delete_collection       app.py:58-59, create_chromadb_index.py:93-130
Everything that crosses this boundary is plain Python lists/dicts/strs/floats, as with chromadb.

`get`, `query`, `query_device` and `delete` also take chromadb's `where_document` ({"$contains": s}, {"$not_contains": s},
{"$and": [...]}, {"$or": [...]}; `$regex` is refused): a case-sensitive substring test of the UTF-8 text, intersected with
`where` (rag_dpo_amd/where_document.py states the rules). Trees of more than 1024 distinct patterns, 4096 compiled operations or
about 15 levels of nesting (16 stack entries) raise ValueError on every engine. On a librdx engine the test runs on the GPU over a copy of the
documents in HBM (engine.DocStore), built on the first where_document call and kept in step by every write after it; a
collection that never filters by document allocates nothing for it. The copy is not persisted: it is rebuilt after a load.
`query` / `query_device` evaluate a `where` they have not cached on the GPU as well, on a single-device librdx engine with at least
_WHERE_DEVICE_MIN_ROWS rows: the filter is compiled (rag_dpo_amd/where_device.py) and one kernel computes the row bitmap from the
metadata columns the filter names, kept in HBM (engine.MetaStore) from the first filter that names them and brought up to date
with the host's columns before every evaluation. rag_dpo_amd/where.py is the model and remains the path of get / delete, of
other engines, of smaller collections and of trees over the device's limits; results are the same on both. Not persisted.
`query_groups` / `query_groups_device` (not part of chromadb's API) return the exact top groups of a metadata key, each with its best
rows, instead of rows: what the reference approximates by over-fetching chunks and deduplicating them by document
(src/rag/retriever.py:202, 539-578); rag_dpo_amd/groups.py states the definition. Cosine collections on one device.
`query_mmr` / `query_mmr_device` (not part of chromadb's API either) return a diverse top-k: maximal marginal relevance over the
fetch_k best rows, for corpora whose near-duplicate chunks share no key; rag_dpo_amd/mmr.py states the definition. Same limits.
`query_range` / `query_range_device` (not part of chromadb's API either) return every allowed row within a distance of the query, counted
exactly, the best max_results of them listed: what the reference does by fetching a fixed 50 and cutting at distance 0.30 on the host
(src/rag/validators.py:64-81); rag_dpo_amd/range_search.py states the definition. Same limits.
`near_duplicates` / `near_duplicates_device` (not part of chromadb's API either) ask that question of the stored chunks themselves and
join the answers into clusters of near-copies on the device: what the reference can only do by content hash before ingest
(src/processing/deduplicate_corpus.py); rag_dpo_amd/dedup.py states the definition. Same limits.
`kmeans` / `kmeans_device` / `assign_clusters` (not part of chromadb's API either) cluster the stored chunks by spherical k-means on the
device, every step in a stated order, so that the clusters are a function of the rows and the arguments alone: which themes the corpus
holds, where the reference has one LLM call per chunk (tag_all_chunks.py); rag_dpo_amd/kmeans.py states the definition. Same limits.
ids/documents/metadata stay on the host; embeddings go to the device index (`engine`). The engine is
always librdx (rag_dpo_amd.engine.HipIndex): there is no CPU search path in this package.

Distances keep Chroma's cosine convention: distance = 1 - cos, ascending (so that
`similarity_score = 1/(1+distance)` reference retriever.py:39-42 and the 0.80 relevance threshold
reference validators.py:64-81 keep their meaning). The search itself is exact (brute force), not HNSW.
metadata={"hnsw:space": "ip"} / "l2" give Chroma's other two spaces (distance 1 - q.x, squared Euclidean distance) on the same
engine, exactly: rag_dpo_amd/spaces.py. Such a collection keeps its embeddings as given, runs on one device, and takes fp32 rows.
An absent "hnsw:space" means cosine here (chromadb's own default is l2).
"""
from __future__ import annotations

import json
import os
import threading
from typing import Any, Callable, Dict, List, Optional, Sequence

import numpy as np

from . import dedup as DD
from . import facets as FC
from . import groups as GR
from . import kmeans as KM
from . import mmr as MM
from . import range_search as RS
from . import where as W
from . import where_document as WD

DEFAULT_INCLUDE_QUERY = ["metadatas", "documents", "distances"]
DEFAULT_INCLUDE_GET = ["metadatas", "documents"]
_VALID_INCLUDE = {"embeddings", "documents", "metadatas", "distances", "uris", "data"}
_ROW_KEYS = ("embeddings", "documents", "metadatas", "distances")   # what query / query_mmr / query_range can put beside the ids


class DuplicateIDError(ValueError):
    pass


class NotFoundError(ValueError):
    pass


def _default_engine_factory(dim: int, device: int):
    from .engine import HipIndex   # raises RdxUnavailable when librdx / a gfx950 GPU is missing
    return HipIndex(dim, device)


def _devices_from_env() -> Optional[List[int]]:
    """RDX_DEVICES=all | "0,1,2,3": spread every collection of this process over these GPUs (rag_dpo_amd.multi_device)"""
    v = os.environ.get("RDX_DEVICES", "").strip()
    if not v:
        return None
    if v.lower() == "all":
        from .multi_device import visible_devices
        return visible_devices()
    return [int(x) for x in v.split(",") if x.strip() != ""]


def _fsync_dir(path: str):
    """make a rename / file creation in `path` durable (the directory entry itself)"""
    try:
        fd = os.open(path, os.O_RDONLY)
    except OSError:
        return
    try:
        os.fsync(fd)
    except OSError:
        pass
    finally:
        os.close(fd)


def _is_device_tensor(x) -> bool:
    import sys
    torch = sys.modules.get("torch")
    return torch is not None and isinstance(x, torch.Tensor) and x.is_cuda


def _check_unique(ids):
    """add's and update's rule, chromadb's wording: an id appears once in a call"""
    if len(set(ids)) != len(ids):
        seen, dups = set(), set()
        for s in ids:
            (dups if s in seen else seen).add(s)
        raise DuplicateIDError(f"Expected IDs to be unique, found duplicates of: {', '.join(sorted(dups))}")


def _as_matrix(embeddings, what: str):
    """-> contiguous fp32 [n][dim]: a numpy array, or the caller's torch CUDA tensor passed through untouched
    (EmbeddingProvider.embed_device -> add: the batch never becomes Python floats)"""
    if _is_device_tensor(embeddings):
        import torch
        t = embeddings if embeddings.dtype == torch.float32 else embeddings.float()
        if t.dim() != 2 or t.shape[0] == 0 or t.shape[1] == 0:
            raise ValueError(f"Expected {what} to be a non-empty [n][dim] tensor, got shape {tuple(t.shape)}")
        return t.contiguous()
    a = np.asarray(embeddings, dtype=np.float32)
    if a.ndim == 1 and a.size > 0:
        a = a[None, :]
    if a.ndim != 2 or a.shape[0] == 0 or a.shape[1] == 0:
        raise ValueError(f"Expected {what} to be a non-empty list of embeddings, got shape {a.shape}")
    return np.ascontiguousarray(a)


def _check_int(name: str, v, lo: int, hi: Optional[int] = None, message: Optional[str] = None):
    """a count argument: an int (not a bool, not a float) in [lo, hi], or >= lo where there is no hi; message: other words, around {}"""
    if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or v < lo or (hi is not None and v > hi):
        bounds = f">= {lo}" if hi is None else f"in [{lo}, {hi}]"
        raise ValueError(message.format(v) if message else f"Expected {name} to be an int {bounds}, got {v!r}")


class Collection:
    def __init__(self, name: str, metadata: Optional[dict] = None, device: int = 0,
                 engine_factory: Optional[Callable[[int, int], Any]] = None, _client=None,
                 devices: Optional[Sequence[int]] = None):
        """devices=[0, 1, ...] (or RDX_DEVICES in the environment): the rows of this ONE collection object are sharded over
        these GPUs and every query spans them (rag_dpo_amd.multi_device) — the reference's single shared `collection`
        (app.py:42-67) on up to 8 MI355X. Default: one GPU (`device`)."""
        self.name = name
        self.metadata = dict(metadata or {})
        space = self.metadata.get("hnsw:space", "cosine")
        if space not in ("cosine", "ip", "l2"):
            raise ValueError(f"hnsw:space must be 'cosine' (the reference's, and the default here), 'ip' or 'l2', got {space!r}")
        self._space_exp_hint: Optional[int] = None   # an "ip" / "l2" store's persisted scale (rag_dpo_amd/spaces.py)
        self._device = device
        if engine_factory is None:
            devs = list(devices) if devices is not None else _devices_from_env()
            if devs is not None and len(devs) > 1 and space != "cosine":
                raise ValueError(f"the {space!r} space runs on one device in this version: no devices= / RDX_DEVICES")
            if devs is not None and len(devs) > 1:
                from .multi_device import multi_device_factory
                engine_factory = multi_device_factory(devs)
            elif devs:
                self._device = device = int(devs[0])
        self._factory = engine_factory or _default_engine_factory
        self._engine = None
        self._dim: Optional[int] = None
        self._ids: List[str] = []              # row -> id ("" when tombstoned)
        self._docs: List[Optional[str]] = []
        self._row_of: Dict[str, int] = {}
        self._alive = np.zeros(0, dtype=bool)
        self._n_dead = 0
        self._cols: Dict[str, W.Column] = {}
        self._lock = threading.RLock()
        self._client = _client
        self._meta_cache: Dict[int, Optional[dict]] = {}   # row -> metadata dict as last assembled (dropped on any write)
        # `where` filters are a handful of fixed shapes re-sent with every question (reference src/rag/pipeline.py:35-71,
        # pages/1_Chat.py:245-247): canonical JSON of the filter -> (packed bitmap, the engine's HBM-resident copy or None).
        # Dropped on every write (add / update / delete / compaction): a bitmap describes one state of the rows.
        self._mask_cache: "Dict[str, tuple]" = {}
        self.mask_cache_hits = 0
        self._dir: Optional[str] = None        # set by PersistentClient: where the snapshot + journal live
        self._replaying = False
        self._doc_store = None                 # engine.DocStore: the documents in HBM, made by the first where_document call
        self._meta_store = None                # engine.MetaStore: the metadata columns filters have named, made by the first `where`
        self._meta_res: Dict[str, list] = {}   # key -> [slot in the store, rows [0, r) of the column that are on the device]
        self._writes = 0                       # bumped by every add / update / upsert / delete / compaction that changes a row: what tables
                                               # derived from the rows (rag_dpo_amd/fusion.py's row -> document group) are keyed on
        self._group_tables: Dict[str, Any] = {}    # groups.GroupTables per metadata key query_groups has grouped by (valid for one _writes)
        self._group_stats = {k: 0 for k in GR.STAT_KEYS}   # group_stats
        self._range_stats = {"queries": 0, "mfma": 0, "exact": 0, "host": 0}   # range_stats
        self._dedup_stats = {k: 0 for k in DD.STAT_KEYS}   # dedup_stats
        self._kmeans_stats = {k: 0 for k in KM.STAT_KEYS}  # kmeans_stats
        self._facet_stats = {k: 0 for k in FC.STAT_KEYS}   # facet_stats

    # ---- small helpers ----------------------------------------------------------------------
    @property
    def _rows(self) -> int:
        return len(self._ids)

    def _ensure_engine(self, dim: int):
        if self._engine is None:
            space = self.metadata.get("hnsw:space", "cosine")
            if space == "cosine":
                self._engine = self._factory(dim, self._device)
            else:       # the same engine over lifted rows, behind a wrapper that returns the space's exact distances
                from . import spaces as S
                if dim % 4 or S.lifted_dim(space, dim) > 4096:
                    raise ValueError(f"the {space!r} space needs a dimension that is a multiple of 4, at most {4096 - S.lifted_dim(space, 0)}")
                inner = self._factory(S.lifted_dim(space, dim), self._device)
                self._engine = S.SpaceEngine(space, inner, scale_exp=self._space_exp_hint,
                                             factory=lambda: self._factory(S.lifted_dim(space, dim), self._device))
            self._dim = dim
        elif dim != self._dim:
            raise ValueError(f"Embedding dimension {dim} does not match collection dimensionality {self._dim}")

    def _set_meta(self, row: int, meta: Optional[dict], replace: bool):
        self._meta_cache.pop(row, None)
        if self._mask_cache:
            self._drop_masks()
        if self._meta_res:                     # rows of resident columns changed in place: uploaded again from `row` on
            for k in (self._meta_res if replace else (meta or ())):
                ent = self._meta_res.get(k)
                if ent is not None and row < ent[1]:
                    ent[1] = row
        if replace:
            for col in self._cols.values():
                col.kind[row] = W.K_MISSING
        if not meta:
            return
        for k, v in meta.items():
            if not isinstance(k, str):
                raise ValueError(f"Expected metadata key to be a str, got {k!r}")
            col = self._cols.get(k)
            if col is None:
                col = self._cols[k] = W.Column(self._rows)
            col.set(row, v)

    def _meta_of(self, row: int) -> Optional[dict]:
        out = {}
        for k, col in self._cols.items():
            v = col.get(row)
            if v is not None:
                out[k] = v
        return out or None

    _META_CACHE_MAX = 200_000

    def _metas_of(self, rows) -> List[Optional[dict]]:
        """metadata dicts of the result rows. Rows seen before come out of a per-row cache (a RAG store answers with the
        same popular chunks again and again; rebuilding 50 dicts of 18 fields from the columns costs more than the GPU
        search at the reference's corpus size); the caller gets its own copies, as with chromadb."""
        rows = [int(r) for r in rows]
        cache = self._meta_cache
        miss = [r for r in rows if r not in cache]
        if miss:
            if len(cache) + len(miss) > self._META_CACHE_MAX:
                cache.clear()
            for r, m in zip(miss, self._metas_from_columns(miss)):
                cache[r] = m
        return [dict(m) if m else None for m in (cache[r] for r in rows)]

    def _metas_from_columns(self, rows) -> List[Optional[dict]]:
        """one vectorised gather per column instead of one Column.get per (row, key)"""
        rr = np.asarray(rows, dtype=np.int64)
        out: List[dict] = [{} for _ in range(rr.shape[0])]
        if rr.shape[0] == 0:
            return []
        for key, col in self._cols.items():
            kinds = col.kind[rr]
            if not kinds.any():
                continue
            vocab = col.vocab
            k0 = int(kinds[0])
            if k0 != W.K_MISSING and (kinds == k0).all():     # the usual case: one kind for the whole column
                if k0 == W.K_STR:
                    vals = [vocab[c] for c in col.code[rr].tolist()]
                elif k0 == W.K_INT:
                    vals = col.num[rr].astype(np.int64).tolist()
                elif k0 == W.K_FLOAT:
                    vals = col.num[rr].tolist()
                else:
                    vals = (col.num[rr] != 0).tolist()
                for d, v in zip(out, vals):
                    d[key] = v
                continue
            kl = kinds.tolist()
            nums = col.num[rr].tolist()
            codes = col.code[rr].tolist()
            for j, kd in enumerate(kl):
                if kd == W.K_STR:
                    out[j][key] = vocab[codes[j]]
                elif kd == W.K_INT:
                    out[j][key] = int(nums[j])
                elif kd == W.K_FLOAT:
                    out[j][key] = nums[j]
                elif kd == W.K_BOOL:
                    out[j][key] = bool(nums[j])
        return [d or None for d in out]

    def _grow_cols(self, n: int):
        for col in self._cols.values():
            col.resize(n)
        if self._alive.shape[0] < n:
            a = np.zeros(max(n, self._alive.shape[0] * 3 // 2 + 16), dtype=bool)
            a[: self._alive.shape[0]] = self._alive
            self._alive = a

    def _mask(self, where: Optional[dict]) -> Optional[np.ndarray]:
        """row bitmap source: `where` pre-filter AND not-deleted; None = everything passes"""
        n = self._rows
        m = W.evaluate(where, self._cols, n)
        if self._n_dead:
            m = self._alive[:n].copy() if m is None else (m & self._alive[:n])
        return m

    _MASK_CACHE_MAX = 32

    def _evict_mask(self, key: str):
        _, r0 = self._mask_cache.pop(key)
        if r0 is not None and hasattr(r0, "close"):
            r0.close()

    def _drop_masks(self):
        for key in list(self._mask_cache):
            self._evict_mask(key)

    # ---- where on the device --------------------------------------------------------------------
    # Below this many rows the host evaluator (0.1 ms at the reference's 16 919 rows) beats a set_query + launch + make_mask:
    # the smallest size at which tools/where_bench.py measured the device path faster (DESIGN.md §16 names the run).
    _WHERE_DEVICE_MIN_ROWS = 262_144

    def _meta_close(self):
        if self._meta_store is not None:
            try:
                self._meta_store.close()
            except Exception:
                pass
        self._meta_store = None
        self._meta_res = {}

    def _where_device(self, where: Optional[dict]):
        """`where` AND not deleted as a device bitmap (torch int32 [ceil(rows/32)]) computed by the predicate scan from the
        metadata columns in HBM, or None = evaluate on the host: no filter, an engine without a device store or with several
        devices, fewer rows than _WHERE_DEVICE_MIN_ROWS, a tree over the device's limits. The store (engine.MetaStore) is a
        cache of self._cols, built lazily: a column is uploaded the first time a filter names it and follows the host here —
        the tail added since, and everything from the lowest row a metadata update touched. If the device fails on the way
        (out of memory for a column, a HIP error) the store is closed, the next filter rebuilds it, and THIS filter is
        evaluated on the host as it was before there was a store: a failing cache never becomes the caller's error, and writes
        never wait on it. A column stays resident from the first filter that names it until a compaction or the collection's
        end: 9 bytes x rows per distinct key ever filtered on (the reference filters on a handful of keys)."""
        eng, n = self._engine, self._rows
        if where in (None, {}) or n == 0 or n < self._WHERE_DEVICE_MIN_ROWS or eng is None \
                or not getattr(eng, "has_device_meta", False) or hasattr(eng, "devices"):
            return None
        from . import where_device as WV
        prog = WV.compile_where(where, self._cols)     # raises what W.validate_where raises
        if prog is None:
            return None
        from . import _lib as L
        if len(set(self._meta_res) | set(prog.keys)) > L.META_MAX_COLUMNS:
            return None
        import torch
        try:
            if self._meta_store is None:
                from .engine import MetaStore
                self._meta_store, self._meta_res = MetaStore(eng.device), {}
            st = self._meta_store
            slots = []
            for key in prog.keys:
                ent = self._meta_res.get(key)
                if ent is None:
                    taken = {e[0] for e in self._meta_res.values()}
                    ent = self._meta_res[key] = [next(s for s in range(len(taken) + 1) if s not in taken), 0]
                if ent[1] < n:
                    col, a = self._cols[key], ent[1]
                    st.set_rows(ent[0], a, col.kind[a:n], col.num[a:n], col.code[a:n])
                    ent[1] = n
                slots.append(ent[0])
            leaves = prog.leaves.copy()
            named = leaves["col"] >= 0
            leaves["col"][named] = np.asarray(slots, dtype=np.int32)[leaves["col"][named]]
            st.set_query(leaves, prog.program)
            dev = torch.device("cuda", st.device)
            base = torch.from_numpy(W.pack_bits(self._alive[:n]).view(np.int32)).to(dev) if self._n_dead else None
            out = torch.empty((n + 31) // 32, dtype=torch.int32, device=dev)
            with torch.cuda.device(dev):
                st.filter_device(n, out, base)
            return out
        except (RuntimeError, MemoryError):             # RdxError / torch's out-of-memory: the device's failure, not the filter's
            self._meta_close()
            return None
        except Exception:
            self._meta_close()
            raise

    # ---- where_document ---------------------------------------------------------------------------
    def _docs_store(self):
        """the device document store (engines that have one: HipIndex, MultiDeviceIndex on its first device), built from
        self._docs on first use; None = evaluate on the host"""
        if self._doc_store is None and self._engine is not None and getattr(self._engine, "has_device_docs", False):
            from .engine import DocStore
            st = DocStore(self._engine.device)
            step = 65536
            for a in range(0, self._rows, step):
                st.append(self._docs[a: a + step])
            self._doc_store = st
        return self._doc_store

    def _docs_write(self, fn):
        """keep the device store in step with a write. The store is a cache of self._docs: if keeping it in step fails (device
        error, out of memory), it is dropped and rebuilt by the next where_document call, and the write itself goes on (its
        rows are already changed in memory and still have to reach the journal)."""
        if self._doc_store is None:
            return
        try:
            fn(self._doc_store)
        except Exception:
            try:
                self._doc_store.close()
            except Exception:
                pass
            self._doc_store = None

    def _wd_mask(self, where: Optional[dict], where_document: dict) -> np.ndarray:
        """bool[rows]: `where` AND `where_document` AND not deleted"""
        n = self._rows
        base = self._mask(where)
        if n == 0:
            return np.zeros(0, dtype=bool)
        store = self._docs_store()
        if store is None:
            m = WD.evaluate_host(where_document, self._docs)
            return m if base is None else (m & base)
        leaves, prog = WD.compile_tree(where_document)
        store.set_query(leaves, prog)
        words = store.filter(W.pack_bits(base) if base is not None else None)
        return np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(bool)

    def _wd_resident(self, where: Optional[dict], where_document: dict):
        """-> (host words or None, resident mask or None) of `where` AND `where_document` AND not deleted. On one device the
        bitmap goes from the document filter straight into the resident mask: it never crosses PCIe."""
        store = self._docs_store()
        eng = self._engine
        if store is not None and not hasattr(eng, "devices") and self._rows > 0:
            import torch
            dev = torch.device("cuda", store.device)
            words = (self._rows + 31) // 32
            base_t = self._where_device(where)       # the `where` half from the columns in HBM: nothing is packed or uploaded
            if base_t is None:
                base = self._mask(where)
                base_t = torch.from_numpy(W.pack_bits(base).view(np.int32)).to(dev) if base is not None else None
            out = torch.empty(words, dtype=torch.int32, device=dev)
            leaves, prog = WD.compile_tree(where_document)
            store.set_query(leaves, prog)
            with torch.cuda.device(dev):
                store.filter_device(out, base_t)
            return None, eng.make_mask(out)
        bits = W.pack_bits(self._wd_mask(where, where_document))
        return bits, (eng.make_mask(bits) if hasattr(eng, "make_mask") else None)

    def _search_args(self, where: Optional[dict], where_document: Optional[dict] = None) -> dict:
        """-> keyword arguments for engine.search: nothing (no filter, no tombstones), mask= (resident bitmap of a filter
        seen before or just uploaded) or allow_bits= (engines without resident masks)"""
        plan = self._filter_plan(where, where_document)
        return {} if plan is None else self._cached_args(*plan)

    def _filter_plan(self, where: Optional[dict], where_document: Optional[dict]):
        """-> _cached_args' arguments for the two filters (key prefix, what the key is made of, what computes the entry), or None:
        nothing filters and no row is dead"""
        if not WD.is_empty(where_document):             # a key of its own: "wd:" + both filters (where-only keys are unchanged)
            WD.validate(where_document)
            return "wd:", [where, where_document], lambda: self._wd_resident(where, where_document)
        if where in (None, {}) and not self._n_dead:
            return None
        return "", where, lambda: self._where_entry(where)

    @staticmethod
    def _filter_key(prefix: str, filters) -> Optional[str]:
        """the mask cache's key: the filters' canonical JSON; None = not canonicalisable (the evaluation will say what is wrong with it)"""
        try:
            return prefix + json.dumps(filters, sort_keys=True, ensure_ascii=False, allow_nan=False)
        except (TypeError, ValueError):
            return None

    def _where_entry(self, where: Optional[dict]):
        """-> the cache entry (host words or None, resident mask or None) of `where` AND not deleted; None = everything passes"""
        dev_bits = self._where_device(where)
        if dev_bits is not None:                        # computed in HBM and handed to the resident mask there
            return None, self._engine.make_mask(dev_bits)
        m = self._mask(where)
        if m is None:
            return None
        bits = W.pack_bits(m)
        return bits, (self._engine.make_mask(bits) if hasattr(self._engine, "make_mask") else None)

    def _cached_args(self, prefix: str, filters, compute, pin: Optional[dict] = None) -> dict:
        """_search_args' body: look the filters' canonical JSON up in the mask cache, else compute() the entry, bound the cache and
        store it. Entries are dropped on every write. pin (query_filtered: one call that uses several entries at once) = {"keys": the
        keys this call uses, never evicted while it runs; "own": the masks made beyond the cache's bound, which the call closes}."""
        key = self._filter_key(prefix, filters)
        ent = self._mask_cache.get(key) if key is not None else None
        if ent is not None:
            self.mask_cache_hits += 1
        else:
            ent = compute()
            if ent is None:
                return {}
            if key is not None and len(self._mask_cache) >= self._MASK_CACHE_MAX:
                # the oldest entry (insertion order) that the running call does not use
                victim = next((k for k in self._mask_cache if pin is None or k not in pin["keys"]), None)
                if victim is not None:
                    self._evict_mask(victim)
            if key is not None and len(self._mask_cache) < self._MASK_CACHE_MAX:
                self._mask_cache[key] = ent
            elif pin is not None:
                pin["own"].append(ent[1])
        if pin is not None and key is not None:
            pin["keys"].add(key)
        return {"mask": ent[1]} if ent[1] is not None else {"allow_bits": ent[0]}

    # ---- the stages every query shares -------------------------------------------------------------------------------
    def _derived_check(self, method: str, how: str, where_document):
        """the end of the four derived families' argument checks: a cosine collection on one device"""
        if not WD.is_empty(where_document):
            WD.validate(where_document)
        space = self.metadata.get("hnsw:space", "cosine")
        if space != "cosine":
            raise NotImplementedError(f"{method} {how}: not available in the {space!r} space")
        if self._engine is not None and hasattr(self._engine, "devices"):
            raise NotImplementedError(f"{method} runs on one device in this version: not on a collection spread over several")

    @staticmethod
    def _need_queries(query_embeddings, why: str = ""):
        if query_embeddings is None:
            raise ValueError("this collection has no embedding function: pass query_embeddings=" + why)

    def _host_queries(self, query_embeddings, keep_device: bool = False):
        """a host-list method's queries -> fp32 [nq][dim] on the host (keep_device: a device tensor stays where it is)"""
        self._need_queries(query_embeddings)
        q = _as_matrix(query_embeddings, "query_embeddings")
        if _is_device_tensor(q) and not keep_device:
            q = q.cpu().numpy()        # results are Python lists anyway; device callers use the *_device methods
        return q

    def _check_dim(self, dim: int, is_matrix: bool = True):
        if not is_matrix or dim != self._dim:
            raise ValueError(f"Embedding dimension {dim} does not match collection dimensionality {self._dim}")

    # What a *_device method refuses, one rule each; _device_args is their usual order. query_range_device, _grouped and _near_dup
    # call the rules one by one, because each of them reports two broken rules in an order of its own (kept as found).
    def _no_rows(self) -> bool:
        """nothing to answer from: nothing was ever added, or every row is deleted. Tombstones that no compaction has taken away yet
        do not count: what a caller sees depends on the content, never on whether a compaction or a reload has happened"""
        return self._engine is None or self._rows == self._n_dead

    def _judge_filters(self, where, where_document=None):
        """before an empty collection's answer: the filters a collection with rows refuses are refused all the same"""
        if where not in (None, {}):
            W.validate_where(where)
        if not WD.is_empty(where_document):
            WD.validate(where_document)

    def _refuse_empty(self, method: str):
        if self._no_rows():
            raise ValueError(f"{method}: the collection is empty")

    def _refuse_host_engine(self, always: bool = False):
        if always or not hasattr(self._engine, "search_device"):
            raise NotImplementedError("this collection's engine has no device-pointer search")

    @staticmethod
    def _resident(method: str, args: dict):
        """_search_args' answer -> the resident mask, or None, of a call that stays on the device"""
        if "allow_bits" in args:
            raise NotImplementedError(f"{method} needs an engine with resident masks")
        return args.get("mask")

    def _device_args(self, method: str, where, where_document):
        """the lock is held -> the resident mask or None"""
        self._refuse_empty(method)
        self._refuse_host_engine()
        return self._resident(method, self._search_args(where, where_document))

    def _on_device(self, args: dict) -> bool:
        """a host-list method's choice: the device path, or the host model over engine.search"""
        return hasattr(self._engine, "search_device") and "allow_bits" not in args

    def _distances(self, scores):
        if getattr(self._engine, "returns_distances", False):
            return scores                                               # "ip" / "l2": the wrapper's exact distances (spaces.py)
        return (np.float32(1.0) - scores).astype(np.float32)            # Chroma cosine distance, fp32 like chromadb

    @staticmethod
    def _empty_result(nq: int, include, keys, **extra) -> dict:
        """query()'s dict before any row is in it: per query an empty list under "ids" and under each of `keys` that is included"""
        out = {"ids": [[] for _ in range(nq)]}
        for key in keys:
            out[key] = [[] for _ in range(nq)] if key in include else None
        out["uris"] = out["data"] = None
        out["included"] = include
        out.update(extra)
        return out

    def _fill_rows(self, out: dict, rows, counts, dist):
        """the result lists: for every b the ids of rows[b, :counts[b]] into out["ids"][b], and beside them what `out` has a list for
        (None or no entry: not included). One call per search, not per query: at the reference's shape this loop is most of query()."""
        ids, docs = self._ids, self._docs
        o_ids, o_docs, o_meta, o_dist, o_emb = out["ids"], out.get("documents"), out.get("metadatas"), out.get("distances"), out.get("embeddings")
        for b in range(len(counts)):
            n = counts[b]
            rr = rows[b, :n].tolist()
            o_ids[b] = [ids[r] for r in rr]
            if o_docs is not None:
                o_docs[b] = [docs[r] for r in rr]
            if o_meta is not None:
                o_meta[b] = self._metas_of(rr)
            if o_dist is not None:
                o_dist[b] = [float(x) for x in dist[b, :n]]
            if o_emb is not None:
                o_emb[b] = self._engine.get(np.array(rr, dtype=np.int64)) if rr else np.zeros((0, self._dim), dtype=np.float32)

    @staticmethod
    def _check_include(include: Sequence[str], allowed: set):
        for inc in include:
            if inc not in _VALID_INCLUDE or inc not in allowed:
                raise ValueError(f"Expected include item to be one of {sorted(allowed)}, got {inc}")

    def _maybe_compact(self):
        if self._n_dead > max(1024, self._rows // 5):
            self._compact()

    def _compact(self):
        n = self._rows
        keep = np.flatnonzero(self._alive[:n])
        self._engine.compact(keep)
        self._docs_write(lambda st: st.compact(keep))
        self._meta_close()                              # rows are renumbered: rebuilt by the next `where`
        self._ids = [self._ids[i] for i in keep]
        self._docs = [self._docs[i] for i in keep]
        self._cols = {k: c.take(keep) for k, c in self._cols.items()}
        self._alive = np.ones(len(keep), dtype=bool)
        self._row_of = {s: i for i, s in enumerate(self._ids)}
        self._n_dead = 0
        self._meta_cache.clear()
        self._drop_masks()
        self._writes += 1

    # ---- chromadb.Collection API ---------------------------------------------------------------
    def count(self, where=None, where_document=None) -> int:
        """the live rows; with a filter, the live rows that pass it (the value counts' kernel with no table: no id list is built)"""
        with self._lock:
            if where in (None, {}) and WD.is_empty(where_document):
                return self._rows - self._n_dead
            if self._no_rows():
                self._judge_filters(where, where_document)
                return 0
            return self._facet_counts(None, where, where_document, False)[2]

    def add(self, ids, embeddings=None, metadatas=None, documents=None, _stored: bool = False, **_ignored):
        """reference create_chromadb_index.py:374-379, ingest_enterprise.py:241-246. Existing ids are skipped
        (chromadb's add never overwrites); duplicate ids inside one call raise DuplicateIDError."""
        if isinstance(ids, str):
            ids = [ids]
        ids = list(ids)
        if not ids:
            raise ValueError("Expected IDs to be a non-empty list, got 0 IDs")
        if embeddings is None:
            raise ValueError("this collection has no embedding function: pass embeddings= "
                             "(the reference always does, create_chromadb_index.py:374-379)")
        emb = _as_matrix(embeddings, "embeddings")
        n = len(ids)
        if emb.shape[0] != n:
            raise ValueError(f"Unequal lengths for fields: ids: {n}, embeddings: {emb.shape[0]}")
        for name, lst in (("metadatas", metadatas), ("documents", documents)):
            if lst is not None and len(lst) != n:
                raise ValueError(f"Unequal lengths for fields: ids: {n}, {name}: {len(lst)}")
        _check_unique(ids)
        for s in ids:
            if not isinstance(s, str) or not s:
                raise ValueError(f"Expected ID to be a non-empty str, got {s!r}")
        with self._lock:
            self._ensure_engine(emb.shape[1])
            fresh = [i for i, s in enumerate(ids) if s not in self._row_of]
            if not fresh:
                return
            if metadatas is not None:   # validate EVERYTHING before anything is stored (host and device rows stay in step)
                for i in fresh:
                    W.check_meta(metadatas[i])
            self._drop_masks()
            self._writes += 1
            sel = emb if len(fresh) == n else (emb[fresh].contiguous() if _is_device_tensor(emb) else np.ascontiguousarray(emb[fresh]))
            row0 = self._rows
            if _stored:             # snapshot reload: rows are the stored (already normalised) values, kept verbatim
                self._engine.add_stored(sel)
            else:
                self._engine.add(sel)   # raises ValueError on NaN/Inf: nothing stored
            self._grow_cols(row0 + len(fresh))
            for j, i in enumerate(fresh):
                row = row0 + j
                self._ids.append(ids[i])
                self._docs.append(documents[i] if documents is not None else None)
                self._row_of[ids[i]] = row
                self._alive[row] = True
                self._set_meta(row, metadatas[i] if metadatas is not None else None, replace=False)
            self._grow_cols(self._rows)   # a key first seen in this batch: its column is as long as the others (the rest is missing)
            self._docs_write(lambda st: st.append(self._docs[row0:]))
            self._log({"op": "add", "ids": [ids[i] for i in fresh],
                       "documents": None if documents is None else [documents[i] for i in fresh],
                       "metadatas": None if metadatas is None else [metadatas[i] for i in fresh]}, sel)

    def update(self, ids, embeddings=None, metadatas=None, documents=None, **_ignored):
        """reference tag_all_chunks.py:215,224 (metadatas only). Metadata updates MERGE into the stored dict,
        as chromadb does; ids that do not exist are ignored; duplicate ids inside one call raise DuplicateIDError."""
        if isinstance(ids, str):
            ids = [ids]
        ids = list(ids)
        n = len(ids)
        _check_unique(ids)           # as add does and as chromadb does: two rows for one id have no order, nothing is touched
        emb = _as_matrix(embeddings, "embeddings") if embeddings is not None else None
        if _is_device_tensor(emb):
            emb = emb.cpu().numpy()    # in-place row updates are rare and small: through the host path
        for name, lst in (("embeddings", emb), ("metadatas", metadatas), ("documents", documents)):
            if lst is not None and len(lst) != n:
                raise ValueError(f"Unequal lengths for fields: ids: {n}, {name}: {len(lst)}")
        if metadatas is not None:
            for m in metadatas:
                W.check_meta(m)
        with self._lock:
            hit = [(i, self._row_of[s]) for i, s in enumerate(ids) if s in self._row_of]
            if hit:
                self._writes += 1
            if emb is not None and hit:
                self._ensure_engine(emb.shape[1])
                self._engine.update(np.array([r for _, r in hit], dtype=np.int64),
                                    np.ascontiguousarray(emb[[i for i, _ in hit]]))
            for i, row in hit:
                if metadatas is not None and metadatas[i]:
                    self._set_meta(row, metadatas[i], replace=False)
                if documents is not None:
                    self._docs[row] = documents[i]
            if documents is not None and hit:
                for key in [k for k in self._mask_cache if k.startswith("wd:")]:   # where-only bitmaps do not read documents
                    self._evict_mask(key)
                self._docs_write(lambda st: st.replace([r for _, r in hit], [documents[i] for i, _ in hit]))
            if hit:
                idx = [i for i, _ in hit]
                self._log({"op": "update", "ids": [ids[i] for i in idx],
                           "documents": None if documents is None else [documents[i] for i in idx],
                           "metadatas": None if metadatas is None else [metadatas[i] for i in idx]},
                          None if emb is None else np.ascontiguousarray(emb[idx]))

    def upsert(self, ids, embeddings=None, metadatas=None, documents=None, **_ignored):
        if isinstance(ids, str):
            ids = [ids]
        ids = list(ids)
        with self._lock:
            old = [i for i, s in enumerate(ids) if s in self._row_of]
            new = [i for i, s in enumerate(ids) if s not in self._row_of]
            pick = lambda lst, idx: None if lst is None else [lst[i] for i in idx]
            emb = _as_matrix(embeddings, "embeddings") if embeddings is not None else None
            if _is_device_tensor(emb) and old:
                emb = emb.cpu().numpy()
            if old:
                self.update([ids[i] for i in old], None if emb is None else emb[old], pick(metadatas, old), pick(documents, old))
            if new:
                self.add([ids[i] for i in new], None if emb is None else emb[new], pick(metadatas, new), pick(documents, new))

    def delete(self, ids=None, where=None, where_document=None, **_ignored):
        """reference ingest_enterprise.py:272,304 (ids in batches of 5000). Rows are tombstoned (excluded from
        every search through the row bitmap) and compacted out of HBM once a fifth of the rows is dead.
        where_document narrows ids= / where=, or selects the rows alone."""
        wd = None if WD.is_empty(where_document) else where_document
        if wd is not None:
            WD.validate(wd)
        with self._lock:
            rows: List[int] = []
            if ids is not None:
                if isinstance(ids, str):
                    ids = [ids]
                rows = [self._row_of[s] for s in ids if s in self._row_of]
                if where is not None and rows:
                    m = W.evaluate(where, self._cols, self._rows)
                    rows = [r for r in rows if m is None or m[r]]
                if wd is not None and rows:
                    m = self._wd_mask(None, wd)
                    rows = [r for r in rows if m[r]]
            elif wd is not None:
                rows = np.flatnonzero(self._wd_mask(where, wd)).tolist()
            elif where is not None:
                m = self._mask(where)
                rows = np.flatnonzero(m).tolist() if m is not None else list(range(self._rows))
            else:
                raise ValueError("delete needs ids=, where= or where_document=")
            gone = [self._ids[r] for r in rows if self._alive[r]]
            if gone:
                self._drop_masks()
                self._writes += 1
                self._log({"op": "delete", "ids": gone}, None)
            for r in rows:
                if self._alive[r]:
                    self._alive[r] = False
                    self._meta_cache.pop(r, None)
                    self._n_dead += 1
                    del self._row_of[self._ids[r]]
                    self._ids[r] = ""
                    self._docs[r] = None
            if rows:
                self._maybe_compact()

    def get(self, ids=None, where=None, limit=None, offset=None, where_document=None, include=None, **_ignored):
        """reference bm25_index.py:211-215 (paging with limit/offset), create_chromadb_index.py:118,452-468,
        ingest_enterprise.py:142-145. Order = insertion order, like chromadb."""
        include = DEFAULT_INCLUDE_GET if include is None else list(include)
        self._check_include(include, {"embeddings", "documents", "metadatas", "uris", "data"})
        wd = None if WD.is_empty(where_document) else where_document
        if wd is not None:
            WD.validate(wd)
        with self._lock:
            if ids is not None:
                if isinstance(ids, str):
                    ids = [ids]
                rows = sorted(self._row_of[s] for s in set(ids) if s in self._row_of)
                if where is not None and rows:
                    m = W.evaluate(where, self._cols, self._rows)
                    rows = [r for r in rows if m is None or m[r]]
                if wd is not None and rows:
                    m = self._wd_mask(None, wd)
                    rows = [r for r in rows if m[r]]
            elif wd is not None:
                rows = np.flatnonzero(self._wd_mask(where, wd)).tolist()
            else:
                m = self._mask(where)
                rows = list(range(self._rows)) if m is None else np.flatnonzero(m).tolist()
            off = int(offset or 0)
            rows = rows[off: off + int(limit)] if limit is not None else rows[off:]
            out = {
                "ids": [self._ids[r] for r in rows],
                "embeddings": None,
                "documents": [self._docs[r] for r in rows] if "documents" in include else None,
                "metadatas": self._metas_of(rows) if "metadatas" in include else None,
                "uris": None,
                "data": None,
                "included": include,
            }
            if "embeddings" in include:
                dim = 0 if self._no_rows() else self._dim    # a collection without rows has no dimension, whatever it held before
                out["embeddings"] = self._engine.get(np.array(rows, dtype=np.int64)) if rows else np.zeros((0, dim), dtype=np.float32)
            return out

    def peek(self, limit: int = 10):
        return self.get(limit=limit, include=["embeddings", "metadatas", "documents"])

    def query(self, query_embeddings=None, n_results: int = 10, where=None, where_document=None, include=None,
              query_texts=None, **_ignored):
        """reference src/rag/retriever.py:215-220, 380-385 (one query, n_results=50, optional where, include
        documents+metadatas+distances) and create_chromadb_index.py:405-408 (no include/where)."""
        include = DEFAULT_INCLUDE_QUERY if include is None else list(include)
        self._check_include(include, _VALID_INCLUDE)
        self._need_queries(query_embeddings, " (the reference always does, retriever.py:215-220)")   # (before the two checks below, as found)
        if not WD.is_empty(where_document):
            WD.validate(where_document)
        _check_int("n_results", n_results, 1, None, "Number of requested results {}, cannot be negative, or zero.")
        q = self._host_queries(query_embeddings)
        nq = q.shape[0]
        with self._lock:
            out = self._empty_result(nq, include, _ROW_KEYS)
            if self._no_rows():        # (as found: "embeddings" is None here whatever include says)
                self._judge_filters(where, where_document)
                out["embeddings"] = None
                return out
            self._check_dim(q.shape[1])
            scores, rows, counts = self._engine.search(q, int(n_results), **self._search_args(where, where_document))
            self._fill_rows(out, rows, counts, self._distances(scores))
            return out

    def query_device(self, query_embeddings, n_results: int = 10, where=None, where_document=None):
        """Batch callers that already hold their query embeddings on the GPU (the provider's `embed_device`, reference
        src/utils/embedding_provider.py:139-145 feeding src/rag/retriever.py:215-220) and want the neighbours there too:
        `query_embeddings` a [nq][dim] fp32 torch CUDA tensor -> (distances f32[nq, n_results], rows i64[nq, n_results],
        counts i32[nq]) torch tensors on the collection's (first) device; `ids_of(rows)` maps rows to the Chroma ids. Same
        filter semantics and the same floats as query() — nothing crosses PCIe but the call itself."""
        import torch
        if not WD.is_empty(where_document):
            WD.validate(where_document)
        with self._lock:
            mask = self._device_args("query_device", where, where_document)
            q = query_embeddings.contiguous()
            nq, k = int(q.shape[0]), int(n_results)
            dev = q.device
            s = torch.empty((nq, k), dtype=torch.float32, device=dev)
            r = torch.empty((nq, k), dtype=torch.int64, device=dev)
            c = torch.empty((nq,), dtype=torch.int32, device=dev)
            self._engine.search_device(q, k, s, r, c, mask=mask)
            if getattr(self._engine, "returns_distances", False):
                return s, r, c
            return (1.0 - s), r, c            # Chroma cosine distance, fp32 (padding entries: distance +inf, row -1)

    # ---- one search, a filter per query --------------------------------------------------------------------------
    def _filters_check(self, nq: int, wheres, where_documents):
        """-> the two sequences as lists of nq entries; the refusals of the derived families"""
        out = []
        for name, seq in (("wheres", wheres), ("where_documents", where_documents)):
            if seq is None and name == "where_documents":
                seq = [None] * nq
            if isinstance(seq, (dict, str, bytes)) or not isinstance(seq, Sequence) or len(seq) != nq:
                raise ValueError(f"query_filtered: {name} must be a sequence with one entry per query ({nq}; None or {{}}: no filter), got "
                                 f"{type(seq).__name__}" + (f" of length {len(seq)}" if isinstance(seq, Sequence) else ""))
            out.append(list(seq))
        for wd in out[1]:
            self._derived_check("query_filtered", "searches the cosine engine with a filter per query", wd)
        if not out[1]:
            self._derived_check("query_filtered", "searches the cosine engine with a filter per query", None)
        return out

    def _resolve_filters(self, wheres, where_documents, pin: dict):
        """the lock is held -> (the distinct filters' _search_args answers, per query the index of its own or -1: nothing filters).
        Filters with the same cache key are one filter; each is resolved once, through the mask cache (pin: _cached_args)."""
        args, index_of, qf = [], {}, np.empty(len(wheres), dtype=np.int32)
        for i, (w, wd) in enumerate(zip(wheres, where_documents)):
            plan = self._filter_plan(w, wd)
            if plan is None:
                qf[i] = -1
                continue
            key = self._filter_key(plan[0], plan[1])
            f = index_of.get(key) if key is not None else None
            if f is None:
                a = self._cached_args(*plan, pin=pin)
                if not a:                                # the filter passes every row
                    f = -1
                else:
                    f = len(args)
                    args.append(a)
                if key is not None:
                    index_of[key] = f
            qf[i] = f
        return args, qf

    def _search_filtered(self, method: str, q, k: int, wheres, where_documents, device_out: bool):
        """the lock is held; q: host fp32 [nq][dim], or a CUDA tensor (device_out) -> (scores, rows, counts) on q's side. ONE
        engine.search_filtered where the engine has it and every filter is a resident mask; otherwise one search per distinct filter
        (host engines, engines without resident masks) — the same results."""
        import contextlib
        eng, nq = self._engine, int(q.shape[0])
        pin = {"keys": set(), "own": []}
        try:
            args, qf = self._resolve_filters(wheres, where_documents, pin)
            resident = all("mask" in a for a in args)
            if device_out:
                import torch
                if not resident:
                    raise NotImplementedError(f"{method} needs an engine with resident masks")
                s = torch.empty((nq, k), dtype=torch.float32, device=q.device)
                r = torch.empty((nq, k), dtype=torch.int64, device=q.device)
                c = torch.empty((nq,), dtype=torch.int32, device=q.device)
                if hasattr(eng, "search_filtered_device"):
                    eng.search_filtered_device(q, k, s, r, c, [a["mask"] for a in args], qf)
                    return s, r, c
                for f in np.unique(qf):                  # an engine with search_device alone: per distinct filter
                    sel = torch.from_numpy(np.flatnonzero(qf == f)).to(q.device)
                    n = int(sel.numel())
                    sf, rf, cf = s.new_empty((n, k)), r.new_empty((n, k)), c.new_empty((n,))
                    eng.search_device(q.index_select(0, sel).contiguous(), k, sf, rf, cf, mask=None if f < 0 else args[f]["mask"])
                    s[sel], r[sel], c[sel] = sf, rf, cf
                return s, r, c
            if resident and hasattr(eng, "search_filtered"):
                return eng.search_filtered(q, k, [a["mask"] for a in args], qf)
            s = np.empty((nq, k), dtype=np.float32)
            r = np.empty((nq, k), dtype=np.int64)
            c = np.empty((nq,), dtype=np.int32)
            for f in np.unique(qf):
                sel = np.flatnonzero(qf == f)
                s[sel], r[sel], c[sel] = eng.search(q[sel], k, **({} if f < 0 else args[f]))
            return s, r, c
        finally:
            for m in pin["own"]:                         # made for this call beyond the cache's bound
                if m is not None and hasattr(m, "close"):
                    with contextlib.suppress(Exception):
                        m.close()

    def query_filtered(self, query_embeddings, wheres, n_results: int = 10, where_documents=None, include=None):
        """query() for a batch of questions that each bring their own filters — the reference builds a `where` per user
        (src/rag/pipeline.py:35-71) over one shared collection (app.py:42-67) — in ONE search of the engine instead of one per
        distinct filter. wheres and where_documents: sequences with one entry per query (None or {}: no filter). Per query the
        result is query(..., where=wheres[q], where_document=where_documents[q])'s: the same dict, floats and order."""
        include = DEFAULT_INCLUDE_QUERY if include is None else list(include)
        self._check_include(include, _VALID_INCLUDE)
        self._need_queries(query_embeddings)
        _check_int("n_results", n_results, 1, None, "Number of requested results {}, cannot be negative, or zero.")
        q = self._host_queries(query_embeddings)
        nq = q.shape[0]
        wheres, where_documents = self._filters_check(nq, wheres, where_documents)
        with self._lock:
            out = self._empty_result(nq, include, _ROW_KEYS)
            if self._no_rows():                          # query()'s answer
                for w, wd in zip(wheres, where_documents):
                    self._judge_filters(w, wd)
                out["embeddings"] = None
                return out
            self._check_dim(q.shape[1])
            scores, rows, counts = self._search_filtered("query_filtered", q, int(n_results), wheres, where_documents, False)
            self._fill_rows(out, rows, counts, self._distances(scores))
            return out

    def query_filtered_device(self, query_embeddings, wheres, n_results: int = 10, where_documents=None):
        """query_device() with a filter per query (see query_filtered): the same tuple, per query what
        query_device(..., where=wheres[q], where_document=where_documents[q]) returns for it."""
        nq = int(query_embeddings.shape[0])
        wheres, where_documents = self._filters_check(nq, wheres, where_documents)
        with self._lock:
            self._refuse_empty("query_filtered_device")
            self._refuse_host_engine()
            s, r, c = self._search_filtered("query_filtered_device", query_embeddings.contiguous(), int(n_results), wheres,
                                            where_documents, True)
            return (1.0 - s), r, c            # Chroma cosine distance, fp32 (padding entries: distance +inf, row -1)

    # ---- grouped search (rag_dpo_amd/groups.py states the definition and the ladder) ---------------------------
    def _groups_check(self, group_by, n_groups, group_size, where_document):
        if not isinstance(group_by, str) or not group_by:
            raise ValueError(f"Expected group_by to be a non-empty str, got {group_by!r}")
        _check_int("n_groups", n_groups, 1, GR.MAX_GROUPS)
        _check_int("group_size", group_size, 1, GR.MAX_GROUP_SIZE)
        self._derived_check("query_groups", "ranks by the cosine score", where_document)

    @property
    def group_stats(self) -> Dict[str, int]:
        """counters of the grouped search since the collection was created: `queries`; how many of them were `proven_first_fetch`
        (the first list held the groups), took the `second_fetch`, went to `brute` force; and the `fill_jobs` given to the fill kernel"""
        return dict(self._group_stats)

    def group_values(self, group_by: str, codes) -> list:
        """the value of key `group_by` behind the group codes query_groups_device returned (any nesting of lists / an array; a negative
        code, padding, gives None). Codes belong to the state of the rows they were returned for: map them before the next write."""
        with self._lock:
            vals = GR.group_tables(self, group_by).values
            cc = codes.tolist() if hasattr(codes, "tolist") else codes
            walk = lambda x: [walk(y) for y in x] if isinstance(x, (list, tuple)) else (vals[x] if x >= 0 else None)
            return walk(cc)

    def _grouped(self, q, group_by, n_groups, group_size, where, where_document, device_out: bool):
        """-> (scores, rows, counts, codes, n_found): torch tensors on the device (device_out) or numpy arrays; the lock is held"""
        stats = self._group_stats
        tables = GR.group_tables(self, group_by)
        args = self._search_args(where, where_document)     # as found: the filters are judged before the engine, unlike in _device_args
        G, m = int(n_groups), int(group_size)
        if not hasattr(self._engine, "search_device"):
            if device_out:
                self._refuse_host_engine()
            stats["queries"] += q.shape[0]
            return GR.grouped_search_host(self._engine, q, tables, G, m, args)
        mask = self._resident("query_groups", args)         # as found: the host form refuses this too, and both under this name
        import torch
        if not _is_device_tensor(q):
            q = torch.from_numpy(q).to(torch.device("cuda", self._engine.device))
        with torch.cuda.device(q.device):
            out = GR.grouped_search_device(self, q.contiguous(), tables, G, m, mask, stats)
        return out if device_out else tuple(t.cpu().numpy() for t in out)

    def query_groups_device(self, query_embeddings, group_by: str, n_groups: int, group_size: int, where=None, where_document=None):
        """query_groups for callers that hold their query embeddings on the GPU ([nq][dim] fp32 torch CUDA tensor) -> (distances f32
        [nq, G, m], rows i64 [nq, G, m], counts i32 [nq, G], group_codes i32 [nq, G], n_found i32 [nq]) on the collection's device;
        padding is distance +inf, row -1, code -1. `group_values(group_by, codes)` maps the codes to the key's values, `ids_of` /
        `payload_of` the rows to ids and payloads. The same groups, rows and floats as query_groups."""
        self._groups_check(group_by, n_groups, group_size, where_document)
        with self._lock:
            self._refuse_empty("query_groups_device")
            s, r, c, codes, found = self._grouped(query_embeddings, group_by, n_groups, group_size, where, where_document, True)
            return (1.0 - s), r, c, codes, found

    def query_groups(self, query_embeddings, group_by: str, n_groups: int = 5, group_size: int = 3, where=None, where_document=None,
                     include=None):
        """Exact top-k grouped by metadata key `group_by`: per query the first n_groups distinct values of the key met while walking
        the ranking of the allowed rows (cosine score descending, row ascending — query()'s order and floats), each with its first
        group_size rows. It is what the reference approximates by fetching n_docs*10 chunks and deduplicating them by document
        (src/rag/retriever.py:202, 539-578). Rows without the key are ignored; 1 and True are different groups; fewer groups or rows
        come back only when the allowed rows hold no more. -> {"groups": [nq][<= G] the key's values, "ids": [nq][<= G][<= m], and per
        `include` "distances", "documents", "metadatas" of the same shape, "included"}."""
        include = DEFAULT_INCLUDE_QUERY if include is None else list(include)
        self._check_include(include, {"documents", "metadatas", "distances"})
        self._groups_check(group_by, n_groups, group_size, where_document)
        q = self._host_queries(query_embeddings, keep_device=True)      # as found: _grouped takes a device tensor as it is
        nq = q.shape[0]
        with self._lock:
            out = {"groups": [[] for _ in range(nq)], "ids": [[] for _ in range(nq)], "included": include}
            for inc in ("distances", "documents", "metadatas"):
                out[inc] = [[] for _ in range(nq)] if inc in include else None
            if self._no_rows():
                self._judge_filters(where, where_document)
                return out
            self._check_dim(q.shape[1])
            s, r, c, codes, found = self._grouped(q, group_by, n_groups, group_size, where, where_document, False)
            dist = self._distances(s)
            vals = GR.group_tables(self, group_by).values
            for b in range(nq):
                n = int(found[b])
                out["groups"][b] = [vals[int(x)] for x in codes[b, :n]]
                one = {key: [None] * n for key in ("ids", *include)}    # query b's groups: one level deeper than a query's rows
                self._fill_rows(one, r[b], c[b, :n], dist[b])
                for key, lists in one.items():
                    out[key][b] = lists
            return out

    # ---- diversity-aware search (rag_dpo_amd/mmr.py states the definition) ---------------------------------------
    def _mmr_check(self, n_results, fetch_k, lambda_mult, where_document):
        _check_int("n_results", n_results, 1, MM.MAX_K)
        _check_int("fetch_k", fetch_k, 1, MM.MAX_FETCH)
        if fetch_k < n_results:
            raise ValueError(f"Expected fetch_k >= n_results, got fetch_k={fetch_k!r}, n_results={n_results!r}")
        if not isinstance(lambda_mult, (int, float, np.integer, np.floating)) or isinstance(lambda_mult, bool) \
                or not 0.0 <= float(lambda_mult) <= 1.0:                      # (a NaN fails both comparisons)
            raise ValueError(f"Expected lambda_mult to be a number in [0, 1], got {lambda_mult!r}")
        self._derived_check("query_mmr", "ranks and compares by the cosine score", where_document)

    def query_mmr_device(self, query_embeddings, n_results: int = 10, fetch_k: int = 50, lambda_mult: float = 0.5, where=None,
                         where_document=None):
        """query_mmr for callers that hold their query embeddings on the GPU ([nq][dim] fp32 torch CUDA tensor) -> (distances f32
        [nq, n_results], rows i64 [nq, n_results], values f64 [nq, n_results], counts i32 [nq]) on the collection's device, in pick
        order; padding is distance +inf, row -1, value -inf. One search and one launch, nothing crosses PCIe but the call itself;
        `ids_of` / `payload_of` map the rows. The same picks and floats as query_mmr."""
        self._mmr_check(n_results, fetch_k, lambda_mult, where_document)
        with self._lock:
            mask = self._device_args("query_mmr_device", where, where_document)
            import torch
            q = query_embeddings.contiguous()                           # as found: its shape is not compared here (query_range_device does)
            with torch.cuda.device(q.device):
                s, r, v, c, _ = MM.mmr_search_device(self._engine, q, int(n_results), int(fetch_k), float(lambda_mult), mask)
            return (1.0 - s), r, v, c

    def query_mmr(self, query_embeddings, n_results: int = 10, fetch_k: int = 50, lambda_mult: float = 0.5, where=None,
                  where_document=None, include=None):
        """Diversity-aware top-k (maximal marginal relevance): of the fetch_k best allowed rows (query()'s ranking and floats) pick
        n_results one by one — first the best, then always the row with the largest lambda_mult * (its score) - (1 - lambda_mult) *
        (its largest exact cosine score with a row picked before), ties to the better-ranked. lambda_mult = 1 is query(n_results);
        smaller values trade relevance for diversity. -> query()'s dict in pick order, plus "mmr_scores": [nq][<= n_results], the value
        each row was picked with. rag_dpo_amd/mmr.py states the arithmetic; results are the same on every path."""
        include = DEFAULT_INCLUDE_QUERY if include is None else list(include)
        self._check_include(include, set(_ROW_KEYS))
        self._mmr_check(n_results, fetch_k, lambda_mult, where_document)
        q = self._host_queries(query_embeddings)
        nq = q.shape[0]
        k, F, lam = int(n_results), int(fetch_k), float(lambda_mult)
        with self._lock:
            out = self._empty_result(nq, include, _ROW_KEYS, mmr_scores=[[] for _ in range(nq)])
            if self._no_rows():
                self._judge_filters(where, where_document)
                return out
            self._check_dim(q.shape[1])
            args = self._search_args(where, where_document)
            if self._on_device(args):
                import torch
                qd = torch.from_numpy(q).to(torch.device("cuda", self._engine.device))
                with torch.cuda.device(qd.device):
                    res = MM.mmr_search_device(self._engine, qd, k, F, lam, args.get("mask"))
                s, r, v, c, bad = (t.cpu().numpy() for t in res)
                if bad[0]:                                              # as found: only this host form reads the flag
                    raise RuntimeError("query_mmr: the search returned a row the index does not hold")
            else:
                s, r, v, c = MM.mmr_search_host(self._engine, q, k, F, lam, args)
            self._fill_rows(out, r, c, self._distances(s))
            out["mmr_scores"] = [[float(x) for x in v[b, : c[b]]] for b in range(nq)]
            return out

    # ---- the score of named pairs (rag_dpo_amd/m3.py states the definition) -----------------------------------------
    def _pairs_check(self, method: str, pair_query, ids):
        self._derived_check(method, "returns the cosine score", None)
        ids = list(ids)
        pq = np.ascontiguousarray(pair_query, dtype=np.int32).reshape(-1)
        if pq.shape[0] != len(ids):
            raise ValueError(f"{method}: {pq.shape[0]} pair_query entries for {len(ids)} ids")
        return pq, ids

    def score_pairs_device(self, query_embeddings, pair_query, ids):
        """score_pairs for callers that hold their query embeddings on the GPU ([nq][dim] fp32 torch CUDA tensor) -> fp32 [n] on the
        collection's device: one launch (rdx_index_score_pairs), nothing synchronised; NaN for an id the collection does not hold
        and for a pair_query entry outside [0, nq). The same floats as score_pairs."""
        pq, ids = self._pairs_check("score_pairs_device", pair_query, ids)
        with self._lock:
            self._refuse_empty("score_pairs_device")
            self._refuse_host_engine()
            import torch
            from . import engine as E
            q = query_embeddings.contiguous()
            if q.dim() != 2:
                raise ValueError("score_pairs_device: query_embeddings must be [nq][dim]")
            self._check_dim(int(q.shape[1]))
            get = self._row_of.get
            rows = np.fromiter((get(s, -1) for s in ids), dtype=np.int64, count=len(ids))
            if not len(ids):
                return torch.empty((0,), dtype=torch.float32, device=q.device)
            with torch.cuda.device(q.device):
                return E.score_pairs(self._engine, q, torch.from_numpy(pq).to(q.device), torch.from_numpy(rows).to(q.device))

    def score_pairs(self, query_embeddings, pair_query, ids) -> np.ndarray:
        """The cosine score (1 - query()'s distance, the same bits) of each named pair: pair p is query pair_query[p] against the row
        of Chroma id ids[p] -> fp32 numpy [n]. NaN for an id the collection does not hold (never added, or deleted) and for a
        pair_query entry outside [0, nq). Cosine collections on one device; engines without the device call go through the numpy
        model over engine.get (rag_dpo_amd/m3.py dense_pairs_model)."""
        pq, ids = self._pairs_check("score_pairs", pair_query, ids)
        q = self._host_queries(query_embeddings)
        with self._lock:
            out = np.full((len(ids),), np.nan, dtype=np.float32)
            if self._no_rows() or not len(ids):
                return out
            self._check_dim(q.shape[1])
            get = self._row_of.get
            rows = np.fromiter((get(s, -1) for s in ids), dtype=np.int64, count=len(ids))
            if hasattr(self._engine, "search_device"):
                import torch
                from . import engine as E
                dev = torch.device("cuda", self._engine.device)
                with torch.cuda.device(dev):
                    return E.score_pairs(self._engine, torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).to(dev),
                                         torch.from_numpy(pq).to(dev), torch.from_numpy(rows).to(dev)).cpu().numpy()
            from . import m3 as M3
            return M3.dense_pairs_model(self._engine.get, len(self._engine), q, pq, rows)

    # ---- threshold search (rag_dpo_amd/range_search.py states the definition) ------------------------------------
    def _range_check(self, max_results, where_document):
        _check_int("max_results", max_results, 1, RS.MAX_RESULTS)
        self._derived_check("query_range", "cuts at a cosine distance", where_document)

    @property
    def range_stats(self) -> Dict[str, int]:
        """counters of the threshold search since the collection was created: `queries`, and how many of them the engine answered on its
        `mfma` path (threshold, main scan, exact re-score of the hits), by its `exact` full scan, or were answered on the `host`
        (engines without a threshold search)"""
        return dict(self._range_stats)

    def _range_count(self, nq: int, paths):
        st = self._range_stats
        st["queries"] += nq
        if paths is None:
            st["host"] += nq
        else:
            st["mfma"] += paths[0]
            st["exact"] += paths[1]

    def query_range_device(self, query_embeddings, max_distance, max_results: int = 100, where=None, where_document=None):
        """query_range for callers that hold their query embeddings on the GPU ([nq][dim] fp32 torch CUDA tensor) -> (distances f32
        [nq, max_results], rows i64 [nq, max_results], counts i32 [nq], totals i64 [nq]) on the collection's device; padding is distance
        +inf, row -1. `max_distance`: a float, or one per query (a sequence, an array or a tensor). `ids_of` / `payload_of` map the rows.
        The same rows and floats as query_range."""
        self._range_check(max_results, where_document)
        with self._lock:
            self._refuse_empty("query_range_device")
            self._refuse_host_engine()
            import torch
            from . import engine as E
            q = query_embeddings.contiguous()
            self._check_dim(tuple(q.shape)[-1], q.dim() == 2)           # as found: the shape and the distance are judged before the filters
            if _is_device_tensor(max_distance):
                max_distance = max_distance.cpu().numpy()
            thr = RS.as_thresholds(max_distance, int(q.shape[0]))
            mask = self._resident("query_range_device", self._search_args(where, where_document))
            with torch.cuda.device(q.device):
                if (thr == thr[0]).all():           # one distance for the batch: a fill on the stream instead of a pageable upload
                    thr_d = torch.full((thr.shape[0],), float(thr[0]), dtype=torch.float32, device=q.device)
                else:
                    thr_d = torch.from_numpy(thr).to(q.device)
                s, r, c, t, paths = E.range_search(self._engine, q, thr_d, int(max_results), mask)
            self._range_count(int(q.shape[0]), paths)
            return (1.0 - s), r, c, t

    def query_range(self, query_embeddings, max_distance, max_results: int = 100, where=None, where_document=None, include=None):
        """Threshold search: per query every allowed row whose cosine distance (query()'s floats) is <= max_distance, counted exactly,
        the best max_results of them in query()'s order. `max_distance`: a float, or one per query; +inf = every allowed row.
        -> query()'s dict for the rows in range, plus "totals": [rows in range per query] (it may exceed max_results). The entries are
        those of query(n_results=max_results) with distance <= max_distance; rag_dpo_amd/range_search.py states the definition."""
        include = DEFAULT_INCLUDE_QUERY if include is None else list(include)
        self._check_include(include, set(_ROW_KEYS))
        self._range_check(max_results, where_document)
        q = self._host_queries(query_embeddings)
        nq, m = q.shape[0], int(max_results)
        if _is_device_tensor(max_distance):
            max_distance = max_distance.cpu().numpy()
        thr = RS.as_thresholds(max_distance, nq)
        with self._lock:
            out = self._empty_result(nq, include, _ROW_KEYS, totals=[0] * nq)
            if self._no_rows():
                self._judge_filters(where, where_document)
                return out
            self._check_dim(q.shape[1])
            args = self._search_args(where, where_document)
            if self._on_device(args):
                import torch
                from . import engine as E
                dev = torch.device("cuda", self._engine.device)
                with torch.cuda.device(dev):
                    res = E.range_search(self._engine, torch.from_numpy(q).to(dev), torch.from_numpy(thr).to(dev), m, args.get("mask"))
                s, r, c, t = (x.cpu().numpy() for x in res[:4])
                self._range_count(nq, res[4])
            else:
                s, r, c, t = RS.range_search_host(self._engine, q, thr, m, args)
                self._range_count(nq, None)
            self._fill_rows(out, r, c, self._distances(s))
            out["totals"] = [int(x) for x in t]
            return out

    # ---- near-duplicate clustering (rag_dpo_amd/dedup.py states the definition) -----------------------------------
    def _dedup_check(self, max_neighbors, max_dense_rows, where_document):
        _check_int("max_neighbors", max_neighbors, 1, DD.MAX_NEIGHBORS)
        _check_int("max_dense_rows", max_dense_rows, 0)
        self._derived_check("near_duplicates", "cuts at a cosine distance", where_document)

    @property
    def dedup_stats(self) -> Dict[str, int]:
        """counters of near_duplicates since the collection was created: `calls`, the allowed `rows` they examined, how many of those
        the engine linked from their neighbour lists (`listed`) and from dense exact scores (`dense`: rows with more than
        max_neighbors rows in range), the engine's `batches`, and the rows answered on the `host` (engines without the clustering)"""
        return dict(self._dedup_stats)

    def _near_dup(self, max_distance, where, where_document, max_neighbors, max_dense_rows, device: bool):
        """-> (labels, totals): torch tensors on the engine's device (device engines), numpy arrays otherwise; the lock is held"""
        t = RS.score_threshold(max_distance)
        args = self._search_args(where, where_document)
        st = self._dedup_stats
        st["calls"] += 1
        if self._on_device(args):
            from . import engine as E
            lab, tot, stats = E.near_dup(self._engine, t, args.get("mask"), int(max_neighbors), int(max_dense_rows))
            for key, v in zip(("rows", "listed", "dense", "batches"), stats):
                st[key] += v
            return lab, tot
        if device:                                       # as found: after the distance and the filters, and in these words for an engine
            self._refuse_host_engine(always=True)        # that has the search but no resident masks as well
        allowed = self._mask(where) if WD.is_empty(where_document) else self._wd_mask(where, where_document)
        lab, tot = DD.near_dup_host(self._engine, t, args, allowed)
        n = int(self._rows if allowed is None else np.count_nonzero(allowed))
        st["rows"] += n
        st["host"] += n
        return lab, tot

    def near_duplicates_device(self, max_distance, where=None, where_document=None, max_neighbors: int = 1024, max_dense_rows: int = 4096):
        """near_duplicates for callers that stay on the GPU -> (labels i64 [rows], totals i64 [rows]) on the collection's device:
        labels[r] = the smallest row of r's cluster (r itself for a row without near-copies), -1 for a row that is deleted or filtered
        out; totals[r] = the rows within the distance of row r, itself included. `ids_of` / `payload_of` map the rows."""
        self._dedup_check(max_neighbors, max_dense_rows, where_document)
        with self._lock:
            self._refuse_empty("near_duplicates_device")
            return self._near_dup(max_distance, where, where_document, max_neighbors, max_dense_rows, True)

    def near_duplicates(self, max_distance, where=None, where_document=None, max_neighbors: int = 1024, max_dense_rows: int = 4096):
        """Near-duplicate clusters of the stored chunks themselves: two allowed rows belong together when one lies within the cosine
        distance `max_distance` (query()'s floats) of the other, directly or through a chain of such rows.
        -> {"clusters": [[id, ...], ...], "neighbors": [[total, ...], ...]}: the clusters of at least two rows, each in row order (its
        first id is the earliest-added row, the natural one to keep), ordered by their first row; beside every id the number of rows
        within the distance of it, itself included. `max_neighbors` (at most 1 024): rows with more rows than this in range are
        linked by an exact pass over the corpus instead of from their list; more than `max_dense_rows` such rows raise ValueError
        (the distance is too loose for duplicate detection). rag_dpo_amd/dedup.py states the definition."""
        self._dedup_check(max_neighbors, max_dense_rows, where_document)
        with self._lock:
            if self._no_rows():
                RS.score_threshold(max_distance)            # as found: a NaN distance is refused on an empty collection too
                self._judge_filters(where, where_document)
                return {"clusters": [], "neighbors": []}
            lab, tot = self._near_dup(max_distance, where, where_document, max_neighbors, max_dense_rows, False)
            if _is_device_tensor(lab):
                lab, tot = lab.cpu().numpy(), tot.cpu().numpy()
            groups = DD.clusters_of(lab)
            return {"clusters": [[self._ids[r] for r in g] for g in groups], "neighbors": [[int(tot[r]) for r in g] for g in groups]}

    # ---- k-means of the stored rows (rag_dpo_amd/kmeans.py states the definition) ------------------------------------
    def _kmeans_check(self, n_clusters, max_iter, seed, init, where_document):
        """-> init as a matrix (or None: sampled)"""
        _check_int("max_iter", max_iter, 0, KM.MAX_ITER)
        if init is None:
            _check_int("n_clusters", n_clusters, 1, KM.MAX_CLUSTERS)
            _check_int("seed", seed, 0)
        else:
            init = _as_matrix(init, "init")
            k = int(init.shape[0])
            if k > KM.MAX_CLUSTERS:
                raise ValueError(f"Expected init to hold at most {KM.MAX_CLUSTERS} centroids, got {k}")
            if n_clusters is not None and (isinstance(n_clusters, bool) or n_clusters != k):
                raise ValueError(f"n_clusters = {n_clusters!r} disagrees with the {k} centroids of init")
        self._derived_check("kmeans", "clusters by the cosine score", where_document)
        return init

    @property
    def kmeans_stats(self) -> Dict[str, int]:
        """counters of kmeans / kmeans_device / assign_clusters since the collection was created: `calls`, the allowed `rows` they
        clustered, the `iterations` (updates) they ran, and the calls answered on the `host` (engines without the clustering)"""
        return dict(self._kmeans_stats)

    def _kmeans(self, init, n_clusters, max_iter, seed, where, where_document, device: bool):
        """-> kmeans_model's tuple: torch tensors on the engine's device (device engines), numpy arrays otherwise; the lock is held"""
        self._refuse_empty("kmeans_device" if device else "kmeans")
        if init is not None:
            self._check_dim(int(init.shape[1]))
            if not (bool(init.isfinite().all()) if _is_device_tensor(init) else bool(np.isfinite(init).all())):
                raise ValueError("init contains NaN or Inf")
        args = self._search_args(where, where_document)
        on_device = self._on_device(args)
        allowed = None
        if init is None or not on_device:                # the host's bitmap: for the sample, and for the host path
            allowed = self._mask(where) if WD.is_empty(where_document) else self._wd_mask(where, where_document)
        if init is None:
            rows = np.arange(self._rows, dtype=np.int64) if allowed is None else np.flatnonzero(allowed)
            init = self._engine.get(KM.sample_rows(rows, n_clusters, seed))
        if device and not on_device:                     # after the arguments and the filters, in near_duplicates_device's words
            self._refuse_host_engine(always=True)
        st = self._kmeans_stats
        st["calls"] += 1
        if on_device:
            import torch
            from . import engine as E
            t = init if _is_device_tensor(init) else torch.from_numpy(init).to(f"cuda:{self._engine.device}")
            out = E.kmeans(self._engine, t, int(max_iter), args.get("mask"))
        else:
            out = KM.kmeans_host(self._engine, init.cpu().numpy() if _is_device_tensor(init) else init, int(max_iter), args, allowed)
            st["host"] += 1
        st["rows"] += int(out[3].sum())
        st["iterations"] += int(out[4])
        return out

    def kmeans_device(self, n_clusters: Optional[int] = None, max_iter: int = 20, seed: int = 0, init=None, where=None, where_document=None):
        """kmeans for callers that stay on the GPU -> (labels i64 [rows], scores f32 [rows], centroids f32 [K][dim], counts i64 [K], n_iter,
        converged), the tensors on the collection's device: labels[r] = the row's cluster, -1 for a row that is deleted or filtered out;
        scores[r] = its cosine score against that centroid (-inf there). `ids_of` / `payload_of` map the rows."""
        init = self._kmeans_check(n_clusters, max_iter, seed, init, where_document)
        with self._lock:
            return self._kmeans(init, n_clusters, max_iter, seed, where, where_document, True)

    def kmeans(self, n_clusters: Optional[int] = None, max_iter: int = 20, seed: int = 0, init=None, where=None, where_document=None):
        """Spherical k-means of the stored chunks: every allowed row goes to the centroid it is closest to by query()'s cosine distance,
        a centroid becomes the normalised sum of its rows, until no row moves or `max_iter` updates have run. Every sum is taken in a
        stated order: the same rows and arguments give the same answer, bit for bit, on every path.
        -> {"centroids": fp32 [K][dim], "clusters": [[id, ...], ...] per cluster in row order, "distances": beside every id its distance
        to its centroid, "counts": [members, ...], "n_iter": updates run, "converged": no row moved in the last assignment}.
        `init`: K starting centroids [K][dim]; None: the stored rows of K allowed rows drawn with `seed` (kmeans.sample_rows). A cluster
        that loses all its rows keeps its centroid. rag_dpo_amd/kmeans.py states the definition."""
        init = self._kmeans_check(n_clusters, max_iter, seed, init, where_document)
        with self._lock:
            lab, sc, cen, cnt, n_iter, conv = self._kmeans(init, n_clusters, max_iter, seed, where, where_document, False)
            if _is_device_tensor(lab):
                lab, sc, cen, cnt = lab.cpu().numpy(), sc.cpu().numpy(), cen.cpu().numpy(), cnt.cpu().numpy()
            dist = self._distances(sc)
            groups = KM.clusters_of(lab, cen.shape[0])
            return {"centroids": cen, "clusters": [[self._ids[r] for r in g.tolist()] for g in groups],
                    "distances": [[float(d) for d in dist[g]] for g in groups], "counts": [int(c) for c in cnt],
                    "n_iter": int(n_iter), "converged": bool(conv)}

    def assign_clusters(self, centroids, where=None, where_document=None):
        """kmeans' dict for given centroids, nothing moved (max_iter = 0): which allowed rows belong to which of them. The returned
        centroids are the given ones normalised."""
        return self.kmeans(init=centroids, max_iter=0, where=where, where_document=where_document)

    # ---- value counts (rag_dpo_amd/facets.py states the definitions) --------------------------------------------------
    @staticmethod
    def _facet_check(key, limit, limit_may_be_none: bool):
        if not isinstance(key, str) or not key:
            raise ValueError(f"Expected key to be a non-empty str, got {key!r}")
        if limit is not None or not limit_may_be_none:
            _check_int("limit", limit, 1, FC.MAX_LIMIT)

    @property
    def facet_stats(self) -> Dict[str, int]:
        """counters of the value counts since the collection was created: the corpus counts asked for (`calls`: facets, facets_device,
        count with a filter) and how many of them were answered on the host (`calls_host`); the `queries` of query_facets /
        query_facets_device and how many of them the engine answered on its `mfma` path, by its `exact` full scan, or were answered on
        the `host` (engines without the counting search)"""
        return dict(self._facet_stats)

    def _facet_counts(self, key: Optional[str], where, where_document, device_out: bool):
        """-> (counts int64 [G], missing, total) of the allowed rows by the code of `key` (None: no table, G = 0); counts is a torch tensor
        on the engine's device where the engine counted, a numpy array otherwise. The lock is held and the collection is not empty."""
        tables = GR.group_tables(self, key) if key is not None else None
        G = tables.n_groups if tables is not None else 0
        args = self._search_args(where, where_document)
        eng = self._engine
        st = self._facet_stats
        if self.metadata.get("hnsw:space", "cosine") == "cosine" and not hasattr(eng, "devices") and self._on_device(args):
            import torch
            from . import engine as E
            dev = torch.device("cuda", eng.device)
            st["calls"] += 1
            return E.facet_count(eng, tables.device(dev)[0] if G else None, G, args.get("mask"))
        if device_out:
            self._refuse_host_engine(always=True)
        st["calls"] += 1
        st["calls_host"] += 1
        allowed = self._mask(where) if WD.is_empty(where_document) else self._wd_mask(where, where_document)
        code = tables.row_group if tables is not None else np.full(self._rows, -1, dtype=np.int32)
        return FC.facet_counts_model(code, G, allowed)

    def facets_device(self, key: str, where=None, where_document=None):
        """facets for callers that stay on the GPU -> (counts i64 [G] on the collection's device, missing, total): counts[c] = the
        allowed rows that hold the value with code c (`group_values(key, codes)` maps codes to values: codes belong to the state of the
        rows they were counted in), `missing` those without the key, `total` all of them."""
        self._facet_check(key, None, True)
        with self._lock:
            self._refuse_empty("facets_device")
            self._refuse_host_engine()
            return self._facet_counts(key, where, where_document, True)

    def facets(self, key: str, where=None, where_document=None, limit: Optional[int] = None):
        """How many allowed rows carry each value of metadata key `key`, exactly: what the reference asks with one id list per value
        (src/processing/create_chromadb_index.py:447-480). -> {"key", "values": the values with a non-zero count, count descending and
        among equal counts the value that appears first in the rows first, "counts": beside them, "n_values": how many values have a
        non-zero count (`limit` cuts the two lists, not this), "missing": allowed rows without the key, "total": allowed rows}.
        1 and True are different values, as in query_groups. Works in every space and on every engine."""
        self._facet_check(key, limit, True)
        with self._lock:
            if self._no_rows():
                self._judge_filters(where, where_document)
                return {"key": key, "values": [], "counts": [], "n_values": 0, "missing": 0, "total": 0}
            counts, missing, total = self._facet_counts(key, where, where_document, False)
            if _is_device_tensor(counts):
                counts = counts.cpu().numpy()
            codes, cnt, n_values = FC.facet_order(counts, limit)
            vals = GR.group_tables(self, key).values
            return {"key": key, "values": [vals[c] for c in codes.tolist()], "counts": [int(x) for x in cnt], "n_values": n_values,
                    "missing": int(missing), "total": int(total)}

    def _query_facets_check(self, key, limit, where_document):
        self._facet_check(key, limit, False)
        self._derived_check("query_facets", "cuts at a cosine distance", where_document)

    def _facet_queries_count(self, nq: int, paths):
        st = self._facet_stats
        st["queries"] += nq
        if paths is None:
            st["host"] += nq
        else:
            st["mfma"] += paths[0]
            st["exact"] += paths[1]

    def query_facets_device(self, query_embeddings, key: str, max_distance, limit: int = 10, where=None, where_document=None):
        """query_facets for callers that hold their query embeddings on the GPU ([nq][dim] fp32 torch CUDA tensor) -> (codes i32
        [nq, limit], counts i64 [nq, limit], n_values i32 [nq], missing i64 [nq], totals i64 [nq]) on the collection's device; padding is
        code -1, count 0. `group_values(key, codes)` maps the codes. The same integers as query_facets."""
        self._query_facets_check(key, limit, where_document)
        with self._lock:
            self._refuse_empty("query_facets_device")
            self._refuse_host_engine()
            import torch
            from . import engine as E
            q = query_embeddings.contiguous()
            self._check_dim(tuple(q.shape)[-1], q.dim() == 2)
            if _is_device_tensor(max_distance):
                max_distance = max_distance.cpu().numpy()
            thr = RS.as_thresholds(max_distance, int(q.shape[0]))
            mask = self._resident("query_facets_device", self._search_args(where, where_document))
            tables = GR.group_tables(self, key)
            with torch.cuda.device(q.device):
                if (thr == thr[0]).all():           # one distance for the batch: a fill on the stream instead of a pageable upload
                    thr_d = torch.full((thr.shape[0],), float(thr[0]), dtype=torch.float32, device=q.device)
                else:
                    thr_d = torch.from_numpy(thr).to(q.device)
                res = E.range_facets(self._engine, q, thr_d, tables.device(q.device)[0], tables.n_groups, int(limit), mask)
            self._facet_queries_count(int(q.shape[0]), res[5])
            return res[:5]

    def query_facets(self, query_embeddings, key: str, max_distance, limit: int = 10, where=None, where_document=None):
        """Of the allowed rows within cosine distance `max_distance` of each query (query_range's rows and floats: `totals` is its
        `totals`), how many carry each value of metadata key `key`, exactly and however many rows are in range. `max_distance`: a
        float, or one per query. -> {"key", "values": [nq][<= limit] the values with a non-zero count in facets' order, "counts": beside
        them, "n_values": [values with a non-zero count per query], "missing": [rows in range without the key], "totals": [rows in
        range]}. rag_dpo_amd/facets.py states the definition."""
        self._query_facets_check(key, limit, where_document)
        q = self._host_queries(query_embeddings)
        nq, m = q.shape[0], int(limit)
        if _is_device_tensor(max_distance):
            max_distance = max_distance.cpu().numpy()
        thr = RS.as_thresholds(max_distance, nq)
        with self._lock:
            out = {"key": key, "values": [[] for _ in range(nq)], "counts": [[] for _ in range(nq)], "n_values": [0] * nq,
                   "missing": [0] * nq, "totals": [0] * nq}
            if self._no_rows():
                self._judge_filters(where, where_document)
                return out
            self._check_dim(q.shape[1])
            args = self._search_args(where, where_document)
            tables = GR.group_tables(self, key)
            if self._on_device(args):
                import torch
                from . import engine as E
                dev = torch.device("cuda", self._engine.device)
                with torch.cuda.device(dev):
                    res = E.range_facets(self._engine, torch.from_numpy(q).to(dev), torch.from_numpy(thr).to(dev), tables.device(dev)[0],
                                         tables.n_groups, m, args.get("mask"))
                codes, cnt, nv, mis, tot = (x.cpu().numpy() for x in res[:5])
                self._facet_queries_count(nq, res[5])
            else:
                codes, cnt, nv, mis, tot = FC.query_facets_host(self._engine, q, thr, tables.row_group, tables.n_groups, m, args)
                self._facet_queries_count(nq, None)
            vals = tables.values
            for b in range(nq):
                n = min(int(nv[b]), m)
                out["values"][b] = [vals[c] for c in codes[b, :n].tolist()]
                out["counts"][b] = [int(x) for x in cnt[b, :n]]
            out["n_values"] = [int(x) for x in nv]
            out["missing"] = [int(x) for x in mis]
            out["totals"] = [int(x) for x in tot]
            return out

    def ids_of(self, rows) -> List[List[str]]:
        """Chroma ids of row ids as returned by query_device (negative = padding, skipped)"""
        with self._lock:
            rr = rows.tolist() if hasattr(rows, "tolist") else rows
            return [[self._ids[x] for x in row if x >= 0] for row in rr]

    def rows_of(self, ids) -> List[int]:
        """the inverse of ids_of for a flat list of Chroma ids: the row query_device would return for each, -1 for an id the
        collection does not hold (never added, or deleted)"""
        with self._lock:
            get = self._row_of.get
            return [get(s, -1) for s in ids]

    def payload_of(self, rows):
        """-> (ids, documents, metadatas) of row ids as returned by query_device: what query() puts beside these rows"""
        with self._lock:
            rr = [int(r) for r in rows]
            return [self._ids[r] for r in rr], [self._docs[r] for r in rr], self._metas_of(rr)

    def column_values(self, key: str, default=None) -> list:
        """the value of metadata key `key` for every row, in row order (`default` where a row has none)"""
        with self._lock:
            col, n = self._cols.get(key), self._rows
            if col is None:
                return [default] * n
            out = [default] * n
            kinds = col.kind[:n]
            strs = np.flatnonzero(kinds == W.K_STR)
            vocab = col.vocab
            for r, c in zip(strs.tolist(), col.code[strs].tolist()):
                out[r] = vocab[c]
            for r in np.flatnonzero((kinds != W.K_STR) & (kinds != W.K_MISSING)).tolist():
                out[r] = col.get(r)
            return out

    @property
    def write_count(self) -> int:
        """how many writes (add / update / upsert / delete / compaction) have changed this collection's rows: a table derived from
        the rows is valid for the count it was built at"""
        return self._writes

    def modify(self, name: Optional[str] = None, metadata: Optional[dict] = None):
        with self._lock:
            if name is not None:
                if self._client is not None:
                    self._client._rename(self.name, name)
                self.name = name
            if metadata is not None:
                self.metadata = dict(metadata)
            if self._dir:
                self._write_header(self._dir, self._snap_rows)

    # ---- persistence: own shard format ------------------------------------------
    # <dir>/collection.json              name, metadata, dim, rows and GENERATION g of the current snapshot (format 3)
    # <dir>/snap<g>.embeddings.f32.npy   snapshot: the stored (normalised) fp32 rows, in row order; reloaded VERBATIM
    # <dir>/snap<g>.records.jsonl        snapshot: one {"id", "document", "metadata"} per row
    # <dir>/journal<g>.jsonl + .f32      every add/update/delete since snapshot g, appended (and fsync'ed) before the call
    #                                    returns: chromadb's PersistentClient is durable per call and the reference never
    #                                    calls persist() (create_chromadb_index.py writes, app.py reads in another process).
    # Crash consistency. A journal record is committed by its complete jsonl line, written AFTER its vectors; the line
    # carries the byte range of those vectors in journal.f32, so orphan floats of a writer killed between the two writes
    # are never read, and opening a store truncates both files to the last committed record (a torn last line, or floats
    # without a line, vanish). persist() writes snapshot g+1 under new names, then replaces collection.json atomically
    # (the commit point: it names the generation), then deletes generation g — a crash at any point leaves either g or
    # g+1 complete, and the files of the other one are removed at the next open.
    _snap_rows = 0
    _gen = 0

    def _names(self, gen: Optional[int]):
        pre = "" if gen is None else f"snap{gen}."
        jp = "journal" if gen is None else f"journal{gen}"
        return {"emb": pre + "embeddings.f32.npy", "rec": pre + "records.jsonl", "jl": jp + ".jsonl", "jf": jp + ".f32"}

    def _cur_names(self):
        return self._names(self._gen if self._snap_format >= 3 else None)   # format 2 stores (round 1) had one unnamed generation

    def _write_header(self, path: str, rows: int, fmt: Optional[int] = None, gen: Optional[int] = None):
        os.makedirs(path, exist_ok=True)
        tmp = os.path.join(path, "collection.json.tmp")
        with open(tmp, "w", encoding="utf-8") as f:
            hdr = {"name": self.name, "metadata": self.metadata, "dim": self._dim, "rows": rows,
                   "format": self._snap_format if fmt is None else fmt, "gen": self._gen if gen is None else gen}
            if self._engine is not None and hasattr(self._engine, "xcd_shares"):
                try:   # what the scan has learned about this GPU's XCDs travels with the store (speed only; include/rdx.h)
                    hdr["xcd_shares"] = [round(x, 5) for x in self._engine.xcd_shares()]
                except Exception:
                    pass
            if getattr(self._engine, "scale_exp", None) is not None:
                hdr["space_scale_exp"] = int(self._engine.scale_exp)   # speed only: the lift is redone from the raw rows at load
            json.dump(hdr, f)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, os.path.join(path, "collection.json"))
        _fsync_dir(path)

    def _log(self, rec: dict, emb):
        if not self._dir or self._replaying:
            return
        nm = self._cur_names()
        rec["n_emb"] = 0 if emb is None else int(emb.shape[0])
        rec["dim"] = None if emb is None else int(emb.shape[1])
        if _is_device_tensor(emb):
            emb = emb.cpu().numpy()
        if emb is not None:
            raw = np.ascontiguousarray(emb, dtype=np.float32).tobytes()
            with open(os.path.join(self._dir, nm["jf"]), "ab") as f:
                rec["f32_off"] = f.seek(0, os.SEEK_END)
                rec["f32_len"] = len(raw)
                f.write(raw)
                f.flush()
                os.fsync(f.fileno())
        with open(os.path.join(self._dir, nm["jl"]), "a", encoding="utf-8") as f:   # the complete line commits the op
            f.write(json.dumps(rec, ensure_ascii=False) + "\n")
            f.flush()
            os.fsync(f.fileno())

    def _save(self, path: str):
        with self._lock:
            if self._n_dead:
                self._compact()
            os.makedirs(path, exist_ok=True)
            old = self._cur_names()
            # The object moves to generation g+1 only AFTER the header naming it is on disk. Until then every add / update /
            # delete must keep going to journal<g>, which collection.json still names: a snapshot that fails half way (ENOSPC
            # in np.save, say) leaves the store exactly as it was, and the writes acknowledged afterwards are found again.
            new_gen = self._gen + 1
            nm = self._names(new_gen)
            n = self._rows
            try:
                if n:
                    emb = self._engine.get(np.arange(n, dtype=np.int64))   # the stored (normalised) fp32 rows
                    with open(os.path.join(path, nm["emb"]), "wb") as f:
                        np.save(f, emb)
                        f.flush()
                        os.fsync(f.fileno())
                with open(os.path.join(path, nm["rec"]), "w", encoding="utf-8") as f:
                    for r in range(n):
                        f.write(json.dumps({"id": self._ids[r], "document": self._docs[r], "metadata": self._meta_of(r)},
                                           ensure_ascii=False) + "\n")
                    f.flush()
                    os.fsync(f.fileno())
                _fsync_dir(path)                      # the new generation's files exist before the header can name them
                self._write_header(path, n, fmt=3, gen=new_gen)   # commit point: the header names generation g+1
            except BaseException:
                # os.replace(collection.json) IS the commit point: if the header on disk names generation g+1 (the replace
                # happened and something after it raised — the directory fsync, an interrupt), the new files are the store and
                # must stay; the object follows the header, so that later writes go to the journal the header names.
                committed = False
                try:
                    with open(os.path.join(path, "collection.json"), encoding="utf-8") as f:
                        committed = int(json.load(f).get("gen", -1)) == new_gen
                except (OSError, ValueError):
                    pass
                if committed:
                    self._snap_format, self._gen, self._snap_rows = 3, new_gen, n
                else:
                    for fn in (nm["emb"], nm["rec"], "collection.json.tmp"):   # partial files of the generation that never committed
                        try:
                            os.remove(os.path.join(path, fn))
                        except OSError:
                            pass
                raise
            self._snap_format, self._gen, self._snap_rows = 3, new_gen, n
            for fn in old.values():
                fp = os.path.join(path, fn)
                if os.path.exists(fp):
                    os.remove(fp)

    _snap_format = 3

    def _load(self, path: str):
        with open(os.path.join(path, "collection.json"), encoding="utf-8") as f:
            meta = json.load(f)
        self.metadata = meta.get("metadata") or {}
        if self.metadata.get("hnsw:space", "cosine") not in ("cosine", "ip", "l2"):
            raise ValueError(f"{path}: unknown hnsw:space {self.metadata.get('hnsw:space')!r}")
        if meta.get("space_scale_exp") is not None:
            self._space_exp_hint = int(meta["space_scale_exp"])
        n = int(meta.get("rows", 0))
        self._snap_rows = n
        self._snap_format = int(meta.get("format", 2))
        self._gen = int(meta.get("gen", 0))
        nm = self._cur_names()
        # files of another generation: a persist() that was killed before or after its commit point
        keep = set(nm.values()) | {"collection.json"}
        for fn in os.listdir(path):
            if fn not in keep and (fn.startswith("snap") or fn.startswith("journal") or fn == "collection.json.tmp"
                                   or (self._snap_format >= 3 and fn in self._names(None).values())):
                os.remove(os.path.join(path, fn))
        self._replaying = True
        try:
            if n:
                emb = np.load(os.path.join(path, nm["emb"]), mmap_mode="r", allow_pickle=False)
                ids, docs, metas = [], [], []
                with open(os.path.join(path, nm["rec"]), encoding="utf-8") as f:
                    for line in f:
                        rec = json.loads(line)
                        ids.append(rec["id"])
                        docs.append(rec.get("document"))
                        metas.append(rec.get("metadata"))
                step = 65536
                for a in range(0, n, step):
                    b = min(n, a + step)
                    self.add(ids=ids[a:b], embeddings=np.asarray(emb[a:b]), documents=docs[a:b], metadatas=metas[a:b],
                             _stored=True)   # verbatim: scores after a reload are bit-identical to those before
            jp, fp = os.path.join(path, nm["jl"]), os.path.join(path, nm["jf"])
            if os.path.exists(jp):
                with open(jp, "rb") as f:
                    blob = f.read()
                f32_size = os.path.getsize(fp) if os.path.exists(fp) else 0
                raw = np.memmap(fp, dtype=np.uint8, mode="r") if f32_size else None
                good, f32_end, pos, legacy_pos = 0, 0, 0, 0
                while pos < len(blob):
                    nl = blob.find(b"\n", pos)
                    if nl < 0:
                        break                      # torn last line of a killed writer: the op never committed
                    try:
                        rec = json.loads(blob[pos:nl].decode("utf-8"))
                    except ValueError:
                        break
                    emb = None
                    if rec.get("n_emb"):
                        cnt = rec["n_emb"] * rec["dim"] * 4
                        off = rec.get("f32_off", legacy_pos)      # format 2 journals carry no offsets: running position
                        if off + cnt > f32_size:
                            break                  # its vectors never reached the disk: not committed
                        emb = np.frombuffer(raw[off: off + cnt].tobytes(), dtype=np.float32).reshape(rec["n_emb"], rec["dim"])
                        legacy_pos = off + cnt
                        f32_end = max(f32_end, off + cnt)
                    if rec["op"] == "add":
                        self.add(ids=rec["ids"], embeddings=emb, documents=rec["documents"], metadatas=rec["metadatas"])
                    elif rec["op"] == "update":
                        self.update(ids=rec["ids"], embeddings=emb, documents=rec["documents"], metadatas=rec["metadatas"])
                    elif rec["op"] == "delete":
                        self.delete(ids=rec["ids"])
                    pos = good = nl + 1
                del raw
                if good < len(blob):               # drop the torn tail so that the next record starts on a fresh line
                    with open(jp, "r+b") as f:
                        f.truncate(good)
                if f32_size > f32_end:             # drop orphan vectors of an uncommitted record
                    with open(fp, "r+b") as f:
                        f.truncate(f32_end)
        finally:
            self._replaying = False
        sh = meta.get("xcd_shares")
        if sh and self._engine is not None and hasattr(self._engine, "xcd_shares"):
            try:
                self._engine.xcd_shares(sh)
            except Exception:      # (a header from another build: the shares are a hint, nothing more)
                pass


class PersistentClient:
    """chromadb.PersistentClient look-alike (reference app.py:58-59, create_chromadb_index.py:70-130,
    eval/run_eval.py:712-715): `PersistentClient(path).get_collection("rag_dpo_chunks")`.
    Collections are loaded into HBM on open; every add/update/delete is journalled when it returns, persist()/close()
    fold the journal into a snapshot."""

    def __init__(self, path: Optional[str] = None, device: int = 0, engine_factory=None, settings=None,
                 devices: Optional[Sequence[int]] = None, **_ignored):
        self.path = path
        self._device = device
        if engine_factory is None and devices is not None and len(devices) > 1:
            from .multi_device import multi_device_factory
            engine_factory = multi_device_factory(devices)
        self._factory = engine_factory
        self._cols: Dict[str, Collection] = {}
        if path and os.path.isdir(path):
            for name in sorted(os.listdir(path)):
                d = os.path.join(path, name)
                if os.path.exists(os.path.join(d, "collection.json")):
                    c = Collection(name, device=device, engine_factory=engine_factory, _client=self)
                    c._load(d)
                    c._dir = d
                    self._cols[name] = c

    def create_collection(self, name: str, metadata: Optional[dict] = None, get_or_create: bool = False, **_ignored):
        if name in self._cols:
            if get_or_create:
                return self._cols[name]
            raise ValueError(f"Collection {name} already exists")
        c = Collection(name, metadata=metadata, device=self._device, engine_factory=self._factory, _client=self)
        self._cols[name] = c
        if self.path:
            c._dir = os.path.join(self.path, name)
            c._write_header(c._dir, 0)
        return c

    def get_collection(self, name: str, **_ignored) -> Collection:
        if name not in self._cols:
            raise NotFoundError(f"Collection {name} does not exist.")
        return self._cols[name]

    def get_or_create_collection(self, name: str, metadata: Optional[dict] = None, **_ignored) -> Collection:
        return self.create_collection(name, metadata=metadata, get_or_create=True)

    def delete_collection(self, name: str):
        if name not in self._cols:
            raise NotFoundError(f"Collection {name} does not exist.")
        c = self._cols.pop(name)
        c._drop_masks()
        if c._doc_store is not None:
            c._doc_store.close()
            c._doc_store = None
        c._meta_close()
        if c._engine is not None and hasattr(c._engine, "close"):
            c._engine.close()
        if self.path:
            d = os.path.join(self.path, name)
            if os.path.isdir(d):
                for fn in os.listdir(d):
                    if fn.startswith(("collection.json", "snap", "journal", "records.jsonl", "embeddings.f32.npy")):
                        os.remove(os.path.join(d, fn))
                try:
                    os.rmdir(d)
                except OSError:
                    pass

    def list_collections(self):
        return list(self._cols.values())

    def _rename(self, old: str, new: str):
        if new in self._cols:
            raise ValueError(f"Collection {new} already exists")
        c = self._cols[new] = self._cols.pop(old)
        if self.path and c._dir and os.path.isdir(c._dir):
            nd = os.path.join(self.path, new)
            os.rename(c._dir, nd)
            c._dir = nd

    def persist(self):
        if not self.path:
            return
        os.makedirs(self.path, exist_ok=True)
        for name, c in self._cols.items():
            c._dir = os.path.join(self.path, name)
            c._save(c._dir)

    def close(self):
        self.persist()

    def heartbeat(self) -> int:
        import time
        return int(time.time() * 1e9)


def Client(**kw):   # chromadb.Client(): in-memory
    return PersistentClient(path=None, **kw)


def import_collection(src, client: PersistentClient, name: Optional[str] = None, page: int = 5000) -> Collection:
    """One-shot import of an existing Chroma collection. `src` is anything Chroma-shaped, e.g.
    `chromadb.PersistentClient(path="data/vectordb/chromadb").get_collection("rag_dpo_chunks")` on a machine that has
    chromadb: it is paged through `get(limit=, offset=, include=[embeddings, documents, metadatas])` (the paging the
    reference itself uses, bm25_index.py:211-215) and re-added here, insertion order kept. chromadb is not imported by
    this package."""
    name = name or getattr(src, "name", "rag_dpo_chunks")
    meta = dict(getattr(src, "metadata", None) or {"hnsw:space": "cosine"})
    dst = client.create_collection(name=name, metadata=meta)
    total, off = src.count(), 0
    while off < total:
        g = src.get(limit=page, offset=off, include=["embeddings", "documents", "metadatas"])
        if not g["ids"]:
            break
        dst.add(ids=g["ids"], embeddings=np.asarray(g["embeddings"], dtype=np.float32), documents=g.get("documents"),
                metadatas=g.get("metadatas"))
        off += len(g["ids"])
    client.persist()
    return dst
