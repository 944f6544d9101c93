"""BM25 sparse retrieval — the sparse half of the reference's hybrid retrieval (src/rag/bm25_index.py), scored on the GPU.

Two indexes with the reference's duck types, so that its unmodified `RAGRetriever` (and this repo's DenseRetriever) accept them:
- SummaryBM25Index: BM25 over the document summaries, the pre-filter that keeps the top documents of a question;
- ChunkBM25Index: BM25 over every chunk of the collection, the sparse ranking fused with the dense ones.

Scores are rank_bm25 0.2.2's BM25Okapi (k1 = 1.5, b = 0.75, epsilon = 0.25), bit for bit:
    doc_len[r] = tokens of row r (duplicates included), avgdl = sum(doc_len) / N, nd[t] = rows containing t
    idf[t] = log(N - nd + 0.5) - log(nd + 0.5), summed in the vocabulary's first-occurrence order; every idf < 0 becomes
             epsilon * (idf_sum / |V|)
    score[r] = 0.0, then for each query token q, in query order, duplicates kept:
             score[r] += idf(q) * ((tf * 2.5) / (tf + k1 * ((1 - b) + (b * doc_len[r]) / avgdl)))      (float64)
A row without q adds +-0.0, so out-of-vocabulary tokens are dropped here; duplicates are kept ((s + w) + w is not s + 2w).
The per-row denominator and the idf are computed on the host with exactly that operation order; the device adds the
postings (include/rdx.h rdx_bm25_*, csrc/bm25_kernel.hpp). Search result: rows with score > 0 (and, for chunks, whose
`document_path` is in `doc_filter` when it is not None: an empty set returns nothing), score descending, ties by
ascending row, cut to top_k (bm25_index.py:146-168, :265-292). A batch of chunk queries may give every query a doc_filter of its
own (`doc_filters`): still one device call (rdx_bm25_search_filtered), each query answered as if searched alone with its set.

The index is immutable, as in the reference: to refresh, build again. By default tokenisation is Python, as in the reference,
and the postings are built with numpy; build="device" does both on the GPU (rag_dpo_amd/bm25_build.py), for collections whose
tokens do not fit Python strings.
"""
from __future__ import annotations

import ctypes
import functools
import json
import logging
import math
import operator
import re
from dataclasses import dataclass
from itertools import accumulate, chain
from pathlib import Path
from typing import Callable, Dict, List, Optional, Sequence, Set

import numpy as np

from . import _lib as L
from .engine import _Handle

logger = logging.getLogger(__name__)

K1, B, EPSILON = 1.5, 0.75, 0.25
MAX_K = 4096          # include/rdx.h rdx_bm25_search: results per query
MAX_TERMS = 4096      # query terms per query (after dropping out-of-vocabulary ones)
MAX_TF = 65535        # the device stores tf as uint16
NOTHING = -2          # a query's entry in place of a filter row: its doc_filter names no indexed document

# French stop words of the reference's tokenizer (bm25_index.py FRENCH_STOPWORDS): a behavioural contract, pinned entry by
# entry by tests/golden/bm25_golden.json
STOPWORDS = frozenset("""
    à après ainsi alors assez au aussi autre autres aux avant avec avoir ayant bien c car ce ces cet cette chaque chez comme
    d dans de déjà depuis des donc dont du elle elles en encore entre est et été être fait faire il ils j jamais je l la le
    les leur leurs lors m ma mais mes même mon n ne ni notre nous on ou où par pas pendant peu peut plus pour quel quelle
    quelles quels que qui quoi rien s sa sans se ses si son sont sous sur t ta tes ton tous tout toute toutes très trop tu
    un une vers votre vous y
""".split())

_WORD = "[0-9a-zàâäçéèêëîïôùûüÿæœ]+"
_TOKEN = re.compile(f"{_WORD}(?:-{_WORD})*")


def tokenize_french(text: str) -> List[str]:
    """lowercase; words of letters (accented included) and digits, hyphen-joined; no stop words, no 1-character tokens"""
    return [t for t in _TOKEN.findall(text.lower()) if len(t) > 1 and t not in STOPWORDS]


@dataclass
class BM25Result:
    """reference bm25_index.py BM25Result: doc_key = document path (summaries) or chunk id (chunks)"""
    doc_key: str
    score: float
    metadata: Dict


@dataclass
class Bm25Arrays:
    """what the engine is built from (include/rdx.h rdx_bm25_create)"""
    n_rows: int
    idf: np.ndarray        # f64 [V]
    denom: np.ndarray      # f64 [N]  k1 * ((1 - b) + (b * doc_len) / avgdl)
    post_off: np.ndarray   # int64 [V+1]
    post_row: np.ndarray   # int32 [nnz], ascending inside a term
    post_tf: np.ndarray    # uint16 [nnz]
    row_group: Optional[np.ndarray] = None   # int32 [N] interned document_path, or None
    n_groups: int = 0


class Bm25Model:
    """the host half of an index: vocabulary, rank_bm25's statistics and the device arrays"""

    def __init__(self, corpus_tokens: Sequence[Sequence[str]]):
        n = len(corpus_tokens)
        doc_len = np.fromiter(map(len, corpus_tokens), dtype=np.int64, count=n)
        flat = list(chain.from_iterable(corpus_tokens))
        self._set_vocab(n, dict.fromkeys(flat))                       # first-occurrence order = rank_bm25's nd order
        ids = np.fromiter(map(self.term_id.__getitem__, flat), dtype=np.int64, count=len(flat))
        rows = np.repeat(np.arange(n, dtype=np.int64), doc_len)
        key, tf = np.unique(ids * max(n, 1) + rows, return_counts=True)   # sorted by (term, row)
        term = key // max(n, 1)
        if tf.size and int(tf.max()) > MAX_TF:
            raise ValueError(f"a token occurs {int(tf.max())} times in one text: the index stores tf in 16 bits (<= {MAX_TF})")
        self.post_row = (key % max(n, 1)).astype(np.int32)
        self.post_tf = tf.astype(np.uint16)
        self.post_off = np.zeros(self.n_terms + 1, dtype=np.int64)
        np.cumsum(np.bincount(term, minlength=self.n_terms), out=self.post_off[1:])
        self._set_statistics(doc_len)

    @classmethod
    def from_postings(cls, n_rows: int, doc_len: np.ndarray, vocab: Sequence[str], post_off: np.ndarray, post_row: np.ndarray,
                      post_tf: np.ndarray) -> "Bm25Model":
        """the model of postings built elsewhere (rag_dpo_amd/bm25_build.py builds them on the GPU): `vocab` = the terms in
        first-occurrence order, doc_len int64 [n_rows], the postings as in Bm25Arrays. The statistics are __init__'s own."""
        self = cls.__new__(cls)
        self._set_vocab(int(n_rows), vocab)
        self.post_off = np.ascontiguousarray(post_off, dtype=np.int64)
        self.post_row = np.ascontiguousarray(post_row, dtype=np.int32)
        self.post_tf = np.ascontiguousarray(post_tf, dtype=np.uint16)
        if self.post_off.shape != (self.n_terms + 1,) or len(doc_len) != self.n_rows or len(self.post_row) != len(self.post_tf):
            raise ValueError("from_postings: the arrays do not fit n_rows and the vocabulary")
        self._set_statistics(np.ascontiguousarray(doc_len, dtype=np.int64))
        return self

    def _set_vocab(self, n: int, vocab) -> None:
        self.term_id: Dict[str, int] = dict(zip(vocab, range(len(vocab))))
        self.n_rows, self.n_terms = n, len(self.term_id)

    def _set_statistics(self, doc_len: np.ndarray) -> None:
        """rank_bm25's statistics from doc_len and post_off, for both ways of building the postings"""
        n = self.n_rows
        self.doc_len = doc_len
        self.avgdl = int(doc_len.sum()) / n if n else 0.0
        self.idf, self.average_idf = idf_of(n, np.diff(self.post_off))
        # rank_bm25: self.k1 * (1 - self.b + self.b * doc_len / self.avgdl), doc_len an int64 array
        self.denom = K1 * (1 - B + B * doc_len / self.avgdl) if n else np.zeros(0)

    def arrays(self, row_group=None, n_groups=0) -> Bm25Arrays:
        return Bm25Arrays(self.n_rows, self.idf, np.ascontiguousarray(self.denom, dtype=np.float64), self.post_off, self.post_row,
                          self.post_tf, row_group, n_groups)

    def query_ids(self, tokens: Sequence[str]) -> List[int]:
        """query order, duplicates kept, out-of-vocabulary tokens dropped (they add +-0.0 to every row)"""
        get = self.term_id.get
        return [i for i in map(get, tokens) if i is not None]


def idf_of(n_rows: int, nd: np.ndarray):
    """rank_bm25 BM25Okapi._calc_idf: math.log per term, a plain left-to-right float sum (not sum(): Python >= 3.12 compensates)"""
    idf = [math.log(n_rows - f + 0.5) - math.log(f + 0.5) for f in nd.tolist()]
    if not idf:
        return np.zeros(0), 0.0
    average_idf = functools.reduce(operator.add, idf, 0) / len(idf)
    out = np.array(idf, dtype=np.float64)
    out[out < 0] = EPSILON * average_idf
    return out, average_idf


class HipBm25(_Handle):
    """one BM25 index in one MI355X's HBM, driven through include/rdx.h. No arithmetic happens in this class."""
    _destroy = "rdx_bm25_destroy"

    def __init__(self, arrays: Bm25Arrays, device: int = 0):
        out = self._new_handle()
        self.device = int(device)
        a = arrays
        self.n_groups = int(a.n_groups)
        self._keep = [np.ascontiguousarray(a.post_off, np.int64), np.ascontiguousarray(a.post_row, np.int32),
                      np.ascontiguousarray(a.post_tf, np.uint16), np.ascontiguousarray(a.idf, np.float64),
                      np.ascontiguousarray(a.denom, np.float64)]
        grp = np.ascontiguousarray(a.row_group, np.int32) if a.row_group is not None else None
        p = [ctypes.c_void_p(x.ctypes.data) for x in self._keep]
        L.check(self._lib.rdx_bm25_create(self.device, int(a.n_rows), int(len(a.idf)), *p,
                                          ctypes.c_void_p(grp.ctypes.data) if grp is not None else None, int(a.n_groups), out))
        self._keep = None   # copied to the device

    def search(self, term_offsets: np.ndarray, term_ids: np.ndarray, k: int, allow_bits: Optional[np.ndarray] = None):
        """-> scores f64 [nq, k], rows int64 [nq, k], counts int32 [nq]; on torch's current stream of the index's device"""
        import torch
        off = np.ascontiguousarray(term_offsets, np.int64)
        ids = np.ascontiguousarray(term_ids, np.int32)
        nq = off.shape[0] - 1
        sc = np.empty((nq, k), np.float64)
        ro = np.empty((nq, k), np.int64)
        cn = np.empty(nq, np.int32)
        ab = np.ascontiguousarray(allow_bits, np.uint32) if allow_bits is not None else None
        if ab is not None and ab.size < (self.n_groups + 31) // 32:
            raise ValueError("allow_bits must hold (n_groups + 31) // 32 words")
        stream = torch._C._cuda_getCurrentRawStream(self.device)
        L.check(self._lib.rdx_bm25_search(self._h, ctypes.c_void_p(off.ctypes.data), ctypes.c_void_p(ids.ctypes.data), nq, int(k),
                                          ctypes.c_void_p(ab.ctypes.data) if ab is not None else None,
                                          ctypes.c_void_p(sc.ctypes.data), ctypes.c_void_p(ro.ctypes.data),
                                          ctypes.c_void_p(cn.ctypes.data), L.RDX_HOST, ctypes.c_void_p(stream)))
        return sc, ro, cn

    def search_filtered(self, term_offsets: np.ndarray, term_ids: np.ndarray, k: int, filter_sets: Optional[np.ndarray],
                        query_filter: np.ndarray):
        """search with a filter per query (rdx_bm25_search_filtered): filter_sets uint32 [n_filters, (n_groups + 31) // 32] (None =
        no sets), query_filter int32 [nq] = the query's row of filter_sets, or -1 for no filter -> what search returns"""
        import torch
        off = np.ascontiguousarray(term_offsets, np.int64)
        ids = np.ascontiguousarray(term_ids, np.int32)
        nq = off.shape[0] - 1
        qf = np.ascontiguousarray(query_filter, np.int32).reshape(-1)
        if qf.shape[0] != nq:
            raise ValueError(f"query_filter has {qf.shape[0]} entries for {nq} queries")
        words = (self.n_groups + 31) // 32
        fs = np.ascontiguousarray(filter_sets, np.uint32) if filter_sets is not None else np.zeros((0, words), np.uint32)
        if fs.ndim != 2 or (fs.shape[0] and fs.shape[1] != words):
            raise ValueError(f"filter_sets must be [n_filters, (n_groups + 31) // 32 = {words}] words (got {fs.shape})")
        sc = np.empty((nq, k), np.float64)
        ro = np.empty((nq, k), np.int64)
        cn = np.empty(nq, np.int32)
        stream = torch._C._cuda_getCurrentRawStream(self.device)
        L.check(self._lib.rdx_bm25_search_filtered(self._h, ctypes.c_void_p(off.ctypes.data), ctypes.c_void_p(ids.ctypes.data), nq, int(k),
                                                   ctypes.c_void_p(fs.ctypes.data) if fs.shape[0] else None, int(fs.shape[0]),
                                                   ctypes.c_void_p(qf.ctypes.data), ctypes.c_void_p(sc.ctypes.data),
                                                   ctypes.c_void_p(ro.ctypes.data), ctypes.c_void_p(cn.ctypes.data), L.RDX_HOST,
                                                   ctypes.c_void_p(stream)))
        return sc, ro, cn


def _default_engine_factory(arrays: Bm25Arrays, device: int):
    return HipBm25(arrays, device)


def _resolve_build(build: str) -> str:
    """-> "host" or "device": where an index's postings are built ("auto" = the device when librdx loads with a GPU)"""
    if build not in ("host", "device", "auto"):
        raise ValueError(f'build must be "host", "device" or "auto" (got {build!r})')
    if build == "host":
        return build
    try:
        L.load(require_gpu=True)
    except L.RdxUnavailable:
        if build == "device":
            raise
        return "host"
    return "device"


class _Bm25Base:
    """build="host" tokenises in Python and builds the postings with numpy; build="device" does both on the GPU
    (rag_dpo_amd/bm25_build.py: the same model and engine arrays, bit for bit) and raises RuntimeError without librdx or a GPU;
    build="auto" takes the device when there is one. After a device build `corpus_tokens` stays []: the tokens never exist as
    Python strings."""

    def __init__(self, engine_factory: Optional[Callable[[Bm25Arrays, int], object]] = None, device: int = 0, build: str = "host"):
        self._factory = engine_factory or _default_engine_factory
        self.device = device
        self.build_mode = _resolve_build(build)
        self.model: Optional[Bm25Model] = None
        self.engine = None
        self.corpus_tokens: List[List[str]] = []
        self._is_built = False

    @property
    def is_built(self) -> bool:
        return self._is_built

    def _device_build(self, texts: Sequence[Optional[str]]):
        """-> (indexes of the texts that have a token, their Bm25Model), built on the GPU"""
        from .bm25_build import DeviceBm25Builder
        return DeviceBm25Builder(self.device).build(texts)

    def _install(self, row_group=None, n_groups=0, model: Optional[Bm25Model] = None):
        if self.engine is not None and hasattr(self.engine, "close"):
            self.engine.close()
        self.model = model if model is not None else Bm25Model(self.corpus_tokens)
        self.engine = self._factory(self.model.arrays(row_group, n_groups), self.device) if self.model.n_rows else None
        self._is_built = True

    def _search_arrays(self, queries: Sequence[str], top_k: int, allow_bits=None, filters=None):
        """-> (live, scores f64 [len(live), k], rows int64 [len(live), k], counts int32 [len(live)]): the engine's own arrays for the
        queries (indices `live`) that have a known token, the reference's order and cut; every other query finds nothing.
        allow_bits: one bitset for every query. filters = (filter_sets, which) instead: a bitset per row of filter_sets and, per
        query, its row, -1 (no filter) or NOTHING (its filter names no indexed document: the query finds nothing)"""
        if not self._is_built:
            raise RuntimeError("the BM25 index is not built")
        none = ([], np.zeros((0, 0), np.float64), np.zeros((0, 0), np.int64), np.zeros(0, np.int32))
        if top_k <= 0 or self.engine is None:
            return none
        k = min(int(top_k), self.model.n_rows)
        terms = [self.model.query_ids(tokenize_french(q)) for q in queries]
        sets, which = filters if filters is not None else (None, None)
        # a query without known tokens scores 0 everywhere: nothing
        live = [i for i, t in enumerate(terms) if t and (which is None or which[i] != NOTHING)]
        if not live:
            return none
        for i in live:
            if len(terms[i]) > MAX_TERMS:
                raise ValueError(f"a BM25 query has {len(terms[i])} known tokens; at most {MAX_TERMS} are supported")
        off = np.zeros(len(live) + 1, np.int64)
        np.cumsum([len(terms[i]) for i in live], out=off[1:])
        ids = np.fromiter(chain.from_iterable(terms[i] for i in live), dtype=np.int32, count=int(off[-1]))
        if sets is None or not len(sets):
            sc, ro, cn = self.engine.search(off, ids, k, allow_bits)
        else:
            sc, ro, cn = self._engine_search_filtered(off, ids, k, sets, np.asarray(which, np.int32)[live])
        return live, sc, ro, cn

    def _engine_search_filtered(self, off: np.ndarray, ids: np.ndarray, k: int, sets: np.ndarray, query_filter: np.ndarray):
        """the engine's search_filtered; an engine without one (a custom engine_factory's) is asked once per distinct set through
        search, with the same results"""
        if hasattr(self.engine, "search_filtered"):
            return self.engine.search_filtered(off, ids, k, sets, query_filter)
        nq = len(query_filter)
        sc, ro, cn = np.zeros((nq, k), np.float64), np.full((nq, k), -1, np.int64), np.zeros(nq, np.int32)
        lens = np.diff(off)
        for f in np.unique(query_filter).tolist():
            js = np.flatnonzero(query_filter == f)
            sub_off = np.zeros(len(js) + 1, np.int64)
            np.cumsum(lens[js], out=sub_off[1:])
            sub_ids = np.concatenate([ids[off[j]:off[j + 1]] for j in js.tolist()])
            sc[js], ro[js], cn[js] = self.engine.search(sub_off, sub_ids, k, None if f < 0 else sets[f])
        return sc, ro, cn

    def _search_rows(self, queries: Sequence[str], top_k: int, allow_bits=None, filters=None):
        """-> per query a list of (row, score), the reference's order and cut"""
        live, sc, ro, cn = self._search_arrays(queries, top_k, allow_bits, filters)
        out: List[list] = [[] for _ in queries]
        for j, i in enumerate(live):
            c = int(cn[j])
            out[i] = list(zip(ro[j, :c].tolist(), sc[j, :c].tolist()))
        return out


class SummaryBM25Index(_Bm25Base):
    """reference bm25_index.py SummaryBM25Index: BM25 over the document summaries (pre-filter of the documents)"""

    def __init__(self, summaries_path: Optional[Path] = None, engine_factory=None, device: int = 0, build: str = "host"):
        super().__init__(engine_factory, device, build)
        self.summaries_path = Path(summaries_path) if summaries_path else Path("data/keep/cnil/document_summaries.json")
        self.doc_keys: List[str] = []
        self.doc_metadata: List[Dict] = []

    def build(self, summaries_path: Optional[str] = None) -> None:
        if summaries_path:
            self.summaries_path = Path(summaries_path)
        if not self.summaries_path.exists():
            raise FileNotFoundError(f"summaries file not found: {self.summaries_path}")
        with open(self.summaries_path, "r", encoding="utf-8") as f:
            summaries = json.load(f)
        self.doc_keys, self.doc_metadata, self.corpus_tokens = [], [], []
        device = self.build_mode == "device"
        texts = []
        for doc_path, entry in summaries.items():
            summary = entry.get("summary", "")
            if not summary or summary.startswith("ERREUR"):
                continue
            title, url = entry.get("document_title", ""), entry.get("source_url", "")
            text = f"{title} {summary} {url}"
            if device:      # every entry goes to the GPU; the ones without a token are dropped below, by its count
                texts.append(text)
            else:
                tokens = tokenize_french(text)
                if not tokens:
                    continue
                self.corpus_tokens.append(tokens)
            self.doc_keys.append(doc_path)
            self.doc_metadata.append({"document_path": doc_path, "source_url": url, "document_title": title, "summary": summary})
        model = None
        if device:
            kept, model = self._device_build(texts)
            self.doc_keys, self.doc_metadata = ([col[i] for i in kept.tolist()] for col in (self.doc_keys, self.doc_metadata))
        self._install(model=model)
        logger.info("BM25 summaries index: %d documents (%d skipped)", len(self.doc_keys), len(summaries) - len(self.doc_keys))

    def search(self, query: str, top_k: int = 20) -> List[BM25Result]:
        (hits,) = self._search_rows([query], top_k)
        return [BM25Result(doc_key=self.doc_keys[r], score=s, metadata=self.doc_metadata[r]) for r, s in hits]

    def get_relevant_doc_paths(self, query: str, top_k: int = 20) -> Set[str]:
        return {r.doc_key for r in self.search(query, top_k=top_k)}

    def get_relevant_doc_paths_batch(self, queries: Sequence[str], top_k: int = 20) -> List[Set[str]]:
        """get_relevant_doc_paths of every query, in one device call"""
        return [{self.doc_keys[r] for r, _ in hits} for hits in self._search_rows(queries, top_k)]


class ChunkBM25Index(_Bm25Base):
    """reference bm25_index.py ChunkBM25Index: BM25 over the chunks of a collection (the sparse ranking of hybrid retrieval)"""

    def __init__(self, engine_factory=None, device: int = 0, build: str = "host"):
        super().__init__(engine_factory, device, build)
        self.chunk_ids: List[str] = []
        self.chunk_texts: List[str] = []
        self.chunk_metadatas: List[Dict] = []
        self._group_of: Dict[str, int] = {}

    def build_from_collection(self, collection, batch_size: int = 5000) -> None:
        total = collection.count()
        self.chunk_ids, self.chunk_texts, self.chunk_metadatas, self.corpus_tokens = [], [], [], []
        offset = 0
        device = self.build_mode == "device"
        while offset < total:
            batch = collection.get(limit=batch_size, offset=offset, include=["documents", "metadatas"])
            if device:      # every row goes to the GPU; the rows without a token are dropped below, by its count
                self.chunk_ids += batch["ids"]
                self.chunk_texts += batch["documents"]
                self.chunk_metadatas += batch["metadatas"]
                offset += batch_size
                continue
            for chunk_id, text, metadata in zip(batch["ids"], batch["documents"], batch["metadatas"]):
                if not text or not text.strip():
                    continue
                tokens = tokenize_french(text)
                if not tokens:
                    continue
                self.chunk_ids.append(chunk_id)
                self.chunk_texts.append(text)
                self.chunk_metadatas.append(metadata)
                self.corpus_tokens.append(tokens)
            offset += batch_size
        model = None
        if device:
            kept, model = self._device_build(self.chunk_texts)
            self.chunk_ids, self.chunk_texts, self.chunk_metadatas = ([col[i] for i in kept.tolist()] for col in
                                                                      (self.chunk_ids, self.chunk_texts, self.chunk_metadatas))
        paths = [(m or {}).get("document_path", "") for m in self.chunk_metadatas]
        self._group_of = dict(zip(dict.fromkeys(paths), range(len(paths))))
        groups = np.fromiter(map(self._group_of.__getitem__, paths), dtype=np.int32, count=len(paths))
        self._install(groups, len(self._group_of), model)
        logger.info("BM25 chunk index: %d chunks", len(self.chunk_ids))

    def _allow_bits(self, doc_filter: Set[str]):
        """-> bitset over document groups, or None when no indexed document is in the filter (nothing can pass)"""
        bits = np.zeros((len(self._group_of) + 31) // 32, np.uint32)
        hit = False
        for p in doc_filter:
            g = self._group_of.get(p)
            if g is not None:
                bits[g >> 5] |= np.uint32(1 << (g & 31))
                hit = True
        return bits if hit else None

    def _filter_table(self, queries: Sequence[str], doc_filter, doc_filters):
        """doc_filters (one Optional[Set[str]] per query) -> _search_arrays' `filters`: equal sets share one row of the table, a
        set that names no indexed document has none (its queries find nothing). None without doc_filters."""
        if doc_filters is None:
            return None
        if doc_filter is not None:
            raise ValueError("give doc_filter (one set for every query) or doc_filters (one per query), not both")
        if len(doc_filters) != len(queries):
            raise ValueError(f"doc_filters has {len(doc_filters)} entries for {len(queries)} queries")
        row_of: Dict[frozenset, int] = {}
        seen: Dict[int, int] = {}         # by identity first: the sub-queries of one question share one set object
        which = []
        for f in doc_filters:
            w = -1 if f is None else seen.get(id(f))
            if w is None:
                w = seen[id(f)] = row_of.setdefault(frozenset(f), len(row_of))
            which.append(w)
        # per distinct set the groups of its indexed documents; the sets that have one are the table's rows, in that order
        known = [[g for g in map(self._group_of.get, f) if g is not None] for f in row_of]
        row = list(accumulate(map(bool, known), initial=0))
        sets = np.zeros((row[-1], (len(self._group_of) + 31) // 32), np.uint32)
        if row[-1]:         # the bits of every set OR-ed in at once
            groups = np.fromiter(chain.from_iterable(known), dtype=np.int64)
            owner = np.repeat(np.arange(row[-1]), [len(gs) for gs in known if gs])
            np.bitwise_or.at(sets, (owner, groups >> 5), np.left_shift(np.uint32(1), (groups & 31).astype(np.uint32)))
        return sets, np.array([w if w < 0 else (row[w] if known[w] else NOTHING) for w in which], np.int32)

    def search_batch(self, queries: Sequence[str], top_k: int = 30, doc_filter: Optional[Set[str]] = None,
                     doc_filters: Optional[Sequence[Optional[Set[str]]]] = None) -> List[List[BM25Result]]:
        """search() of every query, in one device call; doc_filters gives every query a doc_filter of its own (None = unfiltered)"""
        if not self._is_built:
            raise RuntimeError("the BM25 index is not built")
        filters = self._filter_table(queries, doc_filter, doc_filters)
        if filters is not None:
            return [[self.result_of(r, s) for r, s in hits] for hits in self._search_rows(queries, top_k, filters=filters)]
        bits = None
        if doc_filter is not None:
            bits = self._allow_bits(doc_filter)
            if bits is None:
                return [[] for _ in queries]
        return [[self.result_of(r, s) for r, s in hits] for hits in self._search_rows(queries, top_k, bits)]

    def result_of(self, row: int, score: float) -> BM25Result:
        """the BM25Result of one hit: the index's own copy of the chunk's metadata, plus its text"""
        return BM25Result(doc_key=self.chunk_ids[row], score=score,
                          metadata={**(self.chunk_metadatas[row] or {}), "text": self.chunk_texts[row]})

    def search_batch_arrays(self, queries: Sequence[str], top_k: int = 30, doc_filter: Optional[Set[str]] = None,
                            doc_filters: Optional[Sequence[Optional[Set[str]]]] = None):
        """search_batch without the result objects, for callers that materialise a few of the hits (rag_dpo_amd/fusion.py):
        -> (live, scores f64 [len(live), k], rows int64 [len(live), k], counts int32 [len(live)]), rows = indexes into chunk_ids;
        a query that is not in `live` found nothing"""
        if not self._is_built:
            raise RuntimeError("the BM25 index is not built")
        filters = self._filter_table(queries, doc_filter, doc_filters)
        if filters is not None:
            return self._search_arrays(queries, top_k, filters=filters)
        bits = None
        if doc_filter is not None:
            bits = self._allow_bits(doc_filter)
            if bits is None:
                return [], np.zeros((0, 0), np.float64), np.zeros((0, 0), np.int64), np.zeros(0, np.int32)
        return self._search_arrays(queries, top_k, bits)

    def search(self, query: str, top_k: int = 30, doc_filter: Optional[Set[str]] = None) -> List[BM25Result]:
        return self.search_batch([query], top_k, doc_filter)[0]
