"""BGE-M3 lexical weights — learned-sparse retrieval over the encoder's own sub-word tokens.

The definition, stated once; `terms_model`, `score_model` and `ModelLexical` below are it, in numpy, and everything else (the kernels
`rdx_lex_reduce` / `rdx_lex_search` of include/rdx.h, `EmbeddingProvider.embed_lexical*`, `LexicalChunkIndex`) is tested against them
bit for bit. It is what FlagEmbedding's `_process_token_weights` and `compute_lexical_matching_score` compute, to our knowledge:
FlagEmbedding is not installed here and no BGE-M3 weights are offline, so that parity is a decision, not verified.

  Terms of a text. The encoder's last hidden states of every token except `<s>` go through the sparse head, w = relu(h . W + b) with
  W [1][hidden], b [1], in fp32 (torch operations, `EmbeddingProvider`). Each weight is paired with its token id. From there:
  the weight is rounded once to fp16, round to nearest even; the token is dropped when the fp16 value is not finite and greater than 0,
  or when its id is a special id (the tokenizer's cls / eos / pad / unk ids where it has them, else XLM-R's 0, 1, 2, 3); of the tokens
  left, one entry per distinct id carrying the largest weight; entries ordered by ascending id. A text may have no terms. An id
  outside [0, vocab) is an error of that text.

  Score of (question, chunk). s = 0.0 in float64; for each question term t in ascending id that the chunk also has:
  s = s + float64(wq[t]) * float64(wd[t]). The product of two fp16 values is exact in float64: only the order of the additions rounds.

  Search. Per question the rows with s > 0 that pass the question's document filter, score descending, ties by ascending row, the
  first k; scores f64, a count, and the slots past the count holding 0 / -1 (rdx_bm25_search_filtered's format).

`LexicalChunkIndex` has `ChunkBM25Index`'s interface: `DenseRetriever(chunk_bm25_index=LexicalChunkIndex(provider))` and
rag_dpo_amd/fusion.py take it unchanged, and its hits' scores travel where BM25 scores did (`bm25_score`)."""
from __future__ import annotations

import ctypes
import json
import logging
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _lib as L
from .bm25 import NOTHING, ChunkBM25Index
from .engine import _Handle

logger = logging.getLogger(__name__)

XLMR_SPECIAL_IDS = (0, 1, 2, 3)      # <s>, <pad>, </s>, <unk>
MAX_K = 4096                         # include/rdx.h rdx_lex_search: results per question
MAX_TERMS = 4096                     # terms per question
MAX_TOKENS = L.LEX_MAX_TOKENS        # tokens per text in one rdx_lex_reduce call (the encoder's cap)


def special_ids(tokenizer) -> tuple:
    """the ids that never become terms: the tokenizer's cls / eos / pad / unk ids where it has them, else XLM-R's"""
    found = [getattr(tokenizer, name, None) for name in ("cls_token_id", "eos_token_id", "pad_token_id", "unk_token_id")]
    found = sorted({int(i) for i in found if i is not None})
    return tuple(found) if found else XLMR_SPECIAL_IDS


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def terms_model(tok, w, vocab: int, skip=XLMR_SPECIAL_IDS):
    """the terms of one text: token ids [T] and fp32 weights [T] -> (ids int32 [n] ascending, weights fp16 [n])"""
    tok = np.asarray(tok, dtype=np.int64).reshape(-1)
    w32 = np.asarray(w, dtype=np.float32).reshape(-1)
    if tok.shape != w32.shape:
        raise ValueError("terms_model: one weight per token")
    if ((tok < 0) | (tok >= vocab)).any():
        raise ValueError(f"a token id outside [0, {vocab})")
    with np.errstate(over="ignore", invalid="ignore"):
        h = w32.astype(np.float16)                    # round to nearest even; 65520 and above become inf
        keep = np.isfinite(h) & (h > 0) & ~np.isin(tok, np.asarray(list(skip), dtype=np.int64))
    ids, inv = np.unique(tok[keep], return_inverse=True)
    best = np.zeros(ids.shape[0], dtype=np.float16)
    np.maximum.at(best, inv, h[keep])
    return ids.astype(np.int32), best


def terms_of_texts_model(tok, w, off, vocab: int, skip=XLMR_SPECIAL_IDS):
    """terms_model of every text [off[i], off[i + 1]) -> (ids int32 [nnz], weights fp16 [nnz], off int64 [n + 1]); a text with an id
    outside [0, vocab) raises ValueError naming it"""
    off = np.asarray(off, dtype=np.int64)
    ids, ws, counts = [], [], []
    for i in range(len(off) - 1):
        try:
            a, b = terms_model(tok[off[i]:off[i + 1]], w[off[i]:off[i + 1]], vocab, skip)
        except ValueError as e:
            raise ValueError(f"text {i}: {e}") from None
        ids.append(a)
        ws.append(b)
        counts.append(len(a))
    out_off = np.zeros(len(off), dtype=np.int64)
    np.cumsum(counts, out=out_off[1:])
    cat = lambda parts, dt: np.concatenate(parts).astype(dt, copy=False) if parts else np.zeros(0, dt)   # noqa: E731
    return cat(ids, np.int32), cat(ws, np.float16), out_off


def score_model(q_ids, q_w, d_ids, d_w) -> float:
    """score of one (question, chunk) pair from their terms (ids ascending, fp16 weights) -> float64"""
    d = dict(zip(np.asarray(d_ids).tolist(), np.asarray(d_w, dtype=np.float16).astype(np.float64).tolist()))
    s = 0.0
    for t, wq in zip(np.asarray(q_ids).tolist(), np.asarray(q_w, dtype=np.float16).astype(np.float64).tolist()):   # ascending id
        if t in d:
            s = s + wq * d[t]
    return s


@dataclass
class LexArrays:
    """what an engine is built from (include/rdx.h rdx_lex_create)"""
    n_rows: int
    n_terms: int           # the vocabulary's size
    post_off: np.ndarray   # int64 [n_terms + 1]
    post_row: np.ndarray   # int32 [nnz], strictly ascending inside a term
    post_w: np.ndarray     # uint16 [nnz], fp16 bits, finite and above 0
    row_group: Optional[np.ndarray] = None   # int32 [n_rows] interned document_path, or None
    n_groups: int = 0


def _as_bits(w) -> np.ndarray:
    w = np.ascontiguousarray(w)
    return w.view(np.uint16) if w.dtype == np.float16 else np.ascontiguousarray(w, dtype=np.uint16)


class ModelLexical:
    """HipLexical's interface on the CPU, and the oracle of the tests: every question's terms are added to a zero float64 vector in
    the order given (ascending id), one product and one sum per posting. order = -1 adds them in reverse: a mutant, for the tests
    that show the order matters."""

    def __init__(self, arrays: LexArrays, device: int = 0, order: int = 1):
        self.a, self.device, self.order = arrays, device, order
        self.n_groups = int(arrays.n_groups)

    def scores(self, ids, w) -> np.ndarray:
        a = self.a
        score = np.zeros(a.n_rows, dtype=np.float64)
        pw = _as_bits(a.post_w).view(np.float16)
        wq = _as_bits(w).view(np.float16).astype(np.float64)
        for j in range(len(ids))[::self.order]:
            b, e = int(a.post_off[ids[j]]), int(a.post_off[ids[j] + 1])
            rows = a.post_row[b:e].astype(np.int64)
            score[rows] = score[rows] + wq[j] * pw[b:e].astype(np.float64)
        return score

    def search(self, term_offsets, term_ids, term_w, k: int, filter_sets=None, query_filter=None):
        a = self.a
        if not 1 <= k <= MAX_K:
            raise ValueError(f"need 1 <= k <= {MAX_K} (got k = {k})")
        nq = len(term_offsets) - 1
        sc, ro, cn = np.zeros((nq, k)), np.full((nq, k), -1, np.int64), np.zeros(nq, np.int32)
        for q in range(nq):
            b, e = int(term_offsets[q]), int(term_offsets[q + 1])
            s = self.scores(np.asarray(term_ids[b:e]), np.asarray(term_w[b:e]))
            idx = np.nonzero(s > 0)[0]
            f = -1 if query_filter is None else int(query_filter[q])
            if f >= 0:
                gbits = np.unpackbits(np.ascontiguousarray(filter_sets[f], np.uint32).view(np.uint8), bitorder="little").astype(bool)
                idx = idx[gbits[a.row_group[idx]]]
            order = idx[np.argsort(-s[idx], kind="stable")][:k]
            cn[q] = len(order)
            ro[q, :len(order)] = order
            sc[q, :len(order)] = s[order]
        return sc, ro, cn

    def close(self):
        pass


def model_factory(arrays: LexArrays, device: int = 0) -> ModelLexical:
    """LexicalChunkIndex(provider, engine_factory=model_factory): the CPU path"""
    return ModelLexical(arrays, device)


# ---- the device engine ----------------------------------------------------------------------------------------------------------------
class HipLexical(_Handle):
    """one index of lexical weights in one MI355X's HBM, driven through include/rdx.h. No arithmetic happens in this class."""
    _destroy = "rdx_lex_destroy"

    def __init__(self, arrays: LexArrays, device: int = 0):
        out = self._new_handle()
        self.device = int(device)
        a = arrays
        self.n_groups = int(a.n_groups)
        keep = [np.ascontiguousarray(a.post_off, np.int64), np.ascontiguousarray(a.post_row, np.int32), _as_bits(a.post_w)]
        grp = np.ascontiguousarray(a.row_group, np.int32) if a.row_group is not None else None
        L.check(self._lib.rdx_lex_create(self.device, int(a.n_rows), int(a.n_terms), *[ctypes.c_void_p(x.ctypes.data) for x in keep],
                                         ctypes.c_void_p(grp.ctypes.data) if grp is not None else None, int(a.n_groups), out))

    def search(self, term_offsets, term_ids, term_w, k: int, filter_sets=None, query_filter=None):
        """term_offsets int64 [nq + 1], term_ids int32, term_w fp16 (or its uint16 bits); filter_sets uint32 [n_filters, (n_groups + 31)
        // 32] or None, query_filter int32 [nq] (None = no query is filtered) -> scores f64 [nq, k], rows int64 [nq, k], counts int32
        [nq]; on torch's current stream of the index's device"""
        import torch
        off = np.ascontiguousarray(term_offsets, np.int64)
        ids = np.ascontiguousarray(term_ids, np.int32)
        w = _as_bits(term_w)
        nq = off.shape[0] - 1
        if len(ids) != len(w):
            raise ValueError(f"{len(ids)} term ids for {len(w)} weights")
        qf = np.full(max(nq, 0), -1, np.int32) if query_filter is None else np.ascontiguousarray(query_filter, np.int32).reshape(-1)
        if qf.shape[0] != nq:
            raise ValueError(f"query_filter has {qf.shape[0]} entries for {nq} queries")
        words = (self.n_groups + 31) // 32
        fs = np.ascontiguousarray(filter_sets, np.uint32) if filter_sets is not None else np.zeros((0, words), np.uint32)
        if fs.ndim != 2 or (fs.shape[0] and fs.shape[1] != words):
            raise ValueError(f"filter_sets must be [n_filters, (n_groups + 31) // 32 = {words}] words (got {fs.shape})")
        k = int(k)
        sc = np.empty((nq, max(k, 0)), np.float64)
        ro = np.empty((nq, max(k, 0)), np.int64)
        cn = np.empty(max(nq, 0), np.int32)
        stream = torch._C._cuda_getCurrentRawStream(self.device)
        p = lambda x: ctypes.c_void_p(x.ctypes.data)   # noqa: E731
        L.check(self._lib.rdx_lex_search(self._h, p(off), p(ids), p(w), nq, k, p(fs) if fs.shape[0] else None, int(fs.shape[0]), p(qf),
                                         p(sc), p(ro), p(cn), L.RDX_HOST, ctypes.c_void_p(stream)))
        return sc, ro, cn


def _default_engine_factory(arrays: LexArrays, device: int):
    return HipLexical(arrays, device)


# ---- the index ------------------------------------------------------------------------------------------------------------------------
def csr_by_term(term, row, w, n_rows: int, n_terms: int):
    """(term id, row, weight) triples, torch tensors on one device with at most one triple per (term, row) -> the CSR by term as numpy
    (post_off int64 [n_terms + 1], post_row int32, post_w uint16): ONE sort of the keys term * n_rows + row"""
    import torch
    key = term.to(torch.int64) * max(int(n_rows), 1) + row.to(torch.int64)
    key, perm = torch.sort(key)
    post_row = (key % max(int(n_rows), 1)).to(torch.int32)
    post_w = w.to(torch.float16)[perm]
    counts = torch.bincount(term.to(torch.int64), minlength=int(n_terms))
    post_off = np.zeros(int(n_terms) + 1, dtype=np.int64)
    np.cumsum(counts.cpu().numpy(), out=post_off[1:])
    return post_off, post_row.cpu().numpy(), post_w.cpu().numpy().view(np.uint16)


class LexicalChunkIndex(ChunkBM25Index):
    """ChunkBM25Index's interface (search, search_batch, search_batch_arrays, result_of, chunk_ids, is_built, doc_filter / doc_filters
    with its semantics) over BGE-M3 lexical weights. `provider`: an EmbeddingProvider with a sparse head; it encodes the chunks at
    build time and all queries of a call in ONE embed_lexical_device call. engine_factory(LexArrays, device): None = HipLexical (the
    GPU); `model_factory` = the numpy model. The index is immutable: to refresh, build again. A row without terms is not indexed, a
    query without terms finds nothing."""

    FORMAT = 1

    def __init__(self, provider, engine_factory=None, device: int = 0):
        super().__init__(engine_factory or _default_engine_factory, device, "host")
        self.provider = provider
        self.arrays: Optional[LexArrays] = None

    # -- building -----------------------------------------------------------------------------------------------------------------
    def _vocab(self) -> int:
        return int(self.provider.lexical_vocab)

    def build_from_collection(self, collection, batch_size: int = 5000) -> None:
        import torch
        total = collection.count()
        ids_col, texts, metas = [], [], []
        terms, rows, ws = [], [], []
        offset = 0
        while offset < total:
            batch = collection.get(limit=batch_size, offset=offset, include=["documents", "metadatas"])
            offset += batch_size
            cand = [(c, t, m) for c, t, m in zip(batch["ids"], batch["documents"], batch["metadatas"]) if t and t.strip()]
            if not cand:
                continue
            t_ids, t_w, off = self.provider.embed_lexical_device([t for _, t, _ in cand])
            counts = np.diff(off)
            kept = np.flatnonzero(counts > 0)                                   # rows without terms are skipped
            new_row = np.full(len(cand), -1, dtype=np.int64)
            new_row[kept] = len(ids_col) + np.arange(len(kept))
            terms.append(t_ids)
            ws.append(t_w)
            rows.append(torch.from_numpy(np.repeat(new_row, counts)).to(t_ids.device))
            for i in kept.tolist():
                ids_col.append(cand[i][0])
                texts.append(cand[i][1])
                metas.append(cand[i][2])
        n = len(ids_col)
        if terms:
            post_off, post_row, post_w = csr_by_term(torch.cat(terms), torch.cat(rows), torch.cat(ws), n, self._vocab())
        else:
            post_off, post_row, post_w = np.zeros(self._vocab() + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.uint16)
        self._install_csr(ids_col, texts, metas, post_off, post_row, post_w)
        logger.info("lexical chunk index: %d chunks, %d postings", n, len(post_row))

    def build_from_weights(self, ids: Sequence[str], texts: Sequence[str], metadatas: Sequence[Optional[Dict]], terms) -> None:
        """for callers who computed the weights elsewhere: terms[i] = {token_id: weight} (or a pair (ids, weights)) of row i, put
        through the rule of terms_model (fp16 rounding, specials and non-positive weights dropped, the maximum per id); rows without
        terms are skipped"""
        import torch
        V = self._vocab()
        skip = self.provider.lexical_special_ids
        ids_col, tx, metas, t_parts, r_parts, w_parts = [], [], [], [], [], []
        for cid, text, meta, tm in zip(ids, texts, metadatas, terms):
            a, b = (list(tm.keys()), list(tm.values())) if isinstance(tm, dict) else tm
            t, w = terms_model(a, b, V, skip)
            if not len(t):
                continue
            t_parts.append(t)
            w_parts.append(w)
            r_parts.append(np.full(len(t), len(ids_col), dtype=np.int64))
            ids_col.append(cid)
            tx.append(text)
            metas.append(meta)
        if t_parts:
            post_off, post_row, post_w = csr_by_term(torch.from_numpy(np.concatenate(t_parts)), torch.from_numpy(np.concatenate(r_parts)),
                                                     torch.from_numpy(np.concatenate(w_parts)), len(ids_col), V)
        else:
            post_off, post_row, post_w = np.zeros(V + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.uint16)
        self._install_csr(ids_col, tx, metas, post_off, post_row, post_w)

    def _install_csr(self, ids, texts, metas, post_off, post_row, post_w) -> None:
        self.chunk_ids, self.chunk_texts, self.chunk_metadatas = list(ids), list(texts), list(metas)
        paths = [(m or {}).get("document_path", "") for m in self.chunk_metadatas]
        self._group_of = dict(zip(dict.fromkeys(paths), range(len(paths))))
        groups = np.fromiter(map(self._group_of.__getitem__, paths), dtype=np.int32, count=len(paths))
        if self.engine is not None and hasattr(self.engine, "close"):
            self.engine.close()
        self.arrays = LexArrays(len(self.chunk_ids), len(post_off) - 1, np.ascontiguousarray(post_off, np.int64),
                                np.ascontiguousarray(post_row, np.int32), _as_bits(post_w), groups, len(self._group_of))
        self.engine = self._factory(self.arrays, self.device) if self.arrays.n_rows else None
        self._row_of_id = {c: r for r, c in enumerate(self.chunk_ids)}
        self._is_built = True

    def rows_of(self, ids: Sequence[str]) -> np.ndarray:
        """int64 [len(ids)]: each chunk id's row in this index, -1 for an id it does not hold (a chunk without terms, or one added
        since the build)"""
        if not self._is_built:
            raise RuntimeError("the lexical index is not built")
        get = self._row_of_id.get
        return np.fromiter((get(c, -1) for c in ids), dtype=np.int64, count=len(ids))

    # -- files --------------------------------------------------------------------------------------------------------------------
    def save(self, path: str) -> None:
        """writes <path>/post_off.npy, post_row.npy, post_w.npy (uint16: fp16 bits) and index.json (the id / text / metadata columns)"""
        if not self._is_built:
            raise RuntimeError("the lexical index is not built")
        os.makedirs(path, exist_ok=True)
        a = self.arrays
        for name in ("post_off", "post_row", "post_w"):
            np.save(os.path.join(path, name + ".npy"), getattr(a, name))
        with open(os.path.join(path, "index.json"), "w", encoding="utf-8") as f:
            json.dump({"format": self.FORMAT, "n_rows": a.n_rows, "n_terms": a.n_terms, "ids": self.chunk_ids, "texts": self.chunk_texts,
                       "metadatas": self.chunk_metadatas}, f, ensure_ascii=False)

    @classmethod
    def load(cls, path: str, provider, engine_factory=None, device: int = 0) -> "LexicalChunkIndex":
        with open(os.path.join(path, "index.json"), encoding="utf-8") as f:
            meta = json.load(f)
        if meta.get("format") != cls.FORMAT:
            raise ValueError(f"LexicalChunkIndex.load: unknown format {meta.get('format')!r}")
        post_off, post_row, post_w = (np.load(os.path.join(path, n + ".npy")) for n in ("post_off", "post_row", "post_w"))
        if post_off.dtype != np.int64 or post_row.dtype != np.int32 or post_w.dtype != np.uint16 or len(post_off) != meta["n_terms"] + 1 \
                or len(post_row) != len(post_w) or int(post_off[-1]) != len(post_row) or len(meta["ids"]) != meta["n_rows"]:
            raise ValueError("LexicalChunkIndex.load: the files do not belong together")
        ix = cls(provider, engine_factory, device)
        ix._install_csr(meta["ids"], meta["texts"], meta["metadatas"], post_off, post_row, post_w)
        return ix

    # -- searching ----------------------------------------------------------------------------------------------------------------
    def _search_arrays(self, queries: Sequence[str], top_k: int, allow_bits=None, filters=None):
        """ChunkBM25Index._search_arrays over lexical terms: all queries are encoded in ONE embed_lexical_device call"""
        if not self._is_built:
            raise RuntimeError("the lexical index is not built")
        none = ([], np.zeros((0, 0), np.float64), np.zeros((0, 0), np.int64), np.zeros(0, np.int32))
        if top_k <= 0 or self.engine is None or not len(queries):
            return none
        k = min(int(top_k), self.arrays.n_rows)
        t_ids, t_w, off = self.provider.embed_lexical_device(list(queries))
        t_ids, t_w = t_ids.cpu().numpy(), t_w.cpu().numpy()
        counts = np.diff(off)
        sets, which = filters if filters is not None else (None, None)
        live = [i for i in range(len(queries)) if counts[i] > 0 and (which is None or which[i] != NOTHING)]
        if not live:
            return none
        if int(counts[live].max()) > MAX_TERMS:
            raise ValueError(f"a query has {int(counts[live].max())} terms; at most {MAX_TERMS} are supported")
        sub_off = np.zeros(len(live) + 1, np.int64)
        np.cumsum(counts[live], out=sub_off[1:])
        pick = np.concatenate([np.arange(off[i], off[i + 1]) for i in live])
        if allow_bits is not None:
            sets, qf = np.asarray(allow_bits, np.uint32).reshape(1, -1), np.zeros(len(live), np.int32)
        elif sets is not None and len(sets):
            qf = np.asarray(which, np.int32)[live]
        else:
            sets, qf = None, np.full(len(live), -1, np.int32)
        sc, ro, cn = self.engine.search(sub_off, t_ids[pick], t_w[pick], k, sets, qf)
        return live, sc, ro, cn
