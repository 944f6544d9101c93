"""The combined BGE-M3 score: one weighted dense + sparse + multi-vector score per (question, chunk) pair, and a reranker by it —
DESIGN.md §31.

The definition, stated once; `dense_pairs_model`, `sparse_pairs_model`, `combine_model` and `score_model` below are it, in numpy, and the
kernels (`rdx_index_score_pairs`, `rdx_lex_score_pairs`, `rdx_m3_combine` of include/rdx.h) are tested against them bit for bit. For one
pair (question q, chunk c) and weights (w_d, w_s, w_c), each finite and >= 0 with sum W = (w_d + w_s) + w_c > 0:

  dense    the search's exact fp32 score of q's dense vector against c's stored row: the bits query() returns for that row
           (`mmr.pair_scores` over engine.get's row and the query normalised as the search normalises it, `kmeans.k1`).
  sparse   `lexical.score_model`: float64, the products added in ascending term id from +0.0.
  colbert  `late_interaction.maxsim_model`: fp32. With an int8 `MultiVectorStore` the component's source is
           `late_interaction.maxsim_i8_model` over the quantised vectors instead; nothing else of the definition changes.
  value    ((w_d * float64(dense) + w_s * sparse) + w_c * float64(colbert)) / W: three products, two sums and one division in float64,
           each rounded once and never fused. A component whose weight is 0 is skipped: it is not read, and no 0 * x is added.
  final    float32(value). A NaN component gives a NaN value.

The default weights (0.4, 0.2, 0.4) are the model card's recommendation for 'colbert+sparse+dense'. This is what FlagEmbedding's
`compute_score` computes for that mode, to our knowledge: FlagEmbedding is not installed here and no BGE-M3 weights are offline, so that
parity is a decision, not verified (as DESIGN.md §29 and §30 say of their components).

`M3Reranker` has `CrossEncoderReranker`'s interface (`DenseRetriever.retrieve_reranked(_batch)` take it unchanged). Per scoring call it
encodes all distinct questions in ONE `embed_m3_device` call, asking only for the components with a non-zero weight."""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np
import torch

from . import kmeans as KM
from . import lexical as LX
from . import mmr as MM
from .late_interaction import LateInteractionReranker, MultiVectorStore, _MaxSimModel

DEFAULT_WEIGHTS = (0.4, 0.2, 0.4)
MAX_PAIRS = 1 << 20          # include/rdx.h: pairs per call of the three entry points
MAX_TERMS = LX.MAX_TERMS     # terms per question


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def check_weights(weights) -> tuple:
    """(w_dense, w_sparse, w_colbert) as floats: each finite and >= 0, their sum above 0; anything else is a ValueError"""
    try:
        w = tuple(float(x) for x in weights)
    except (TypeError, ValueError):
        raise ValueError(f"weights must be three numbers (dense, sparse, colbert), got {weights!r}") from None
    if len(w) != 3 or any(isinstance(x, bool) for x in weights):
        raise ValueError(f"weights must be three numbers (dense, sparse, colbert), got {weights!r}")
    if not all(math.isfinite(x) and x >= 0.0 for x in w):
        raise ValueError(f"every weight must be finite and at least 0, got {weights!r}")
    total = (w[0] + w[1]) + w[2]
    if not (total > 0.0 and math.isfinite(total)):
        raise ValueError(f"the weights' sum must be finite and above 0, got {weights!r}")
    return w


def combine_model(dense, sparse, colbert, weights):
    """-> (value float64 [n], final float32 [n]). dense fp32 / sparse f64 / colbert fp32 [n]; a component is None exactly when its
    weight is 0"""
    w = check_weights(weights)
    parts = ((dense, np.float32), (sparse, np.float64), (colbert, np.float32))
    for (x, _), wi, name in zip(parts, w, ("dense", "sparse", "colbert")):
        if (x is None) != (wi == 0.0):
            raise ValueError(f"combine_model: {name} is given exactly when its weight is not 0")
    total = np.float64((w[0] + w[1]) + w[2])
    value = None
    with np.errstate(invalid="ignore", over="ignore"):
        for (x, dt), wi in zip(parts, w):
            if x is None:
                continue
            term = np.float64(wi) * np.asarray(x, dtype=dt).astype(np.float64)      # one product, rounded once
            value = term if value is None else value + term                          # one sum, rounded once
        value = np.atleast_1d(value / total)
        return value, value.astype(np.float32)


def dense_pairs_model(get_rows, n_rows: int, queries, pair_q, pair_row) -> np.ndarray:
    """rdx_index_score_pairs in numpy: get_rows(rows) -> the stored rows (engine.get), queries fp32 [nq][dim] raw -> fp32 [n]; NaN for a
    pair whose query is outside [0, nq) or whose row is outside [0, n_rows), and for a query holding NaN or Inf"""
    q = np.ascontiguousarray(queries, dtype=np.float32)
    pq, pr = np.asarray(pair_q, dtype=np.int64), np.asarray(pair_row, dtype=np.int64)
    out = np.full((len(pq),), np.nan, dtype=np.float32)
    ok = (pq >= 0) & (pq < q.shape[0]) & (pr >= 0) & (pr < n_rows)
    if not ok.any():
        return out
    with np.errstate(invalid="ignore", over="ignore"):
        qhat = KM.k1(q)
    finite = np.isfinite(q.astype(np.float64)).all(axis=1)
    for qi in np.unique(pq[ok]).tolist():
        if not finite[qi]:
            continue
        at = np.flatnonzero(ok & (pq == qi))
        out[at] = MM.pair_scores(get_rows(pr[at]), qhat[qi])
    return out


def sparse_pairs_model(arrays: "LX.LexArrays", term_off, term_ids, term_w, pair_q, pair_row) -> np.ndarray:
    """rdx_lex_score_pairs in numpy over an index's arrays -> float64 [n]: lexical.score_model's sum of each pair (the chunk's weight
    of a term looked up in the term's postings); NaN for a pair out of range and for every pair of a bad question (ids not strictly
    ascending or outside [0, n_terms), weight bits outside [0x0001, 0x7BFF])"""
    off = np.asarray(term_off, dtype=np.int64)
    ids = np.asarray(term_ids, dtype=np.int64)
    bits = LX._as_bits(np.asarray(term_w))
    wq = bits.view(np.float16).astype(np.float64)
    pw = LX._as_bits(arrays.post_w).view(np.float16)
    nq = len(off) - 1
    out = np.full((len(pair_q),), np.nan, dtype=np.float64)
    for p, (qi, r) in enumerate(zip(np.asarray(pair_q).tolist(), np.asarray(pair_row).tolist())):
        if not (0 <= qi < nq and 0 <= r < arrays.n_rows):
            continue
        b, e = int(off[qi]), int(off[qi + 1])
        t = ids[b:e]
        if ((t < 0) | (t >= arrays.n_terms)).any() or (np.diff(t) <= 0).any() or ((bits[b:e] < 1) | (bits[b:e] > 0x7BFF)).any():
            continue
        s = 0.0
        for j in range(b, e):                                       # ascending term id
            lo, hi = int(arrays.post_off[ids[j]]), int(arrays.post_off[ids[j] + 1])
            at = lo + int(np.searchsorted(arrays.post_row[lo:hi], r))
            if at < hi and arrays.post_row[at] == r:
                s = s + wq[j] * float(pw[at])
        out[p] = s
    return out


def score_model(dense, q_terms, d_terms, q_vecs, d_vecs, weights=DEFAULT_WEIGHTS):
    """the definition for ONE pair from its parts -> (value float64, final float32): dense fp32 (the search's score), q_terms / d_terms
    (ids, fp16 weights) of the question and the chunk, q_vecs / d_vecs their fp16 token vectors; a part whose weight is 0 may be None"""
    from .late_interaction import maxsim_model
    w = check_weights(weights)
    d = np.asarray([dense], dtype=np.float32) if w[0] else None
    s = np.asarray([LX.score_model(*q_terms, *d_terms)], dtype=np.float64) if w[1] else None
    c = np.asarray([maxsim_model(q_vecs, d_vecs)], dtype=np.float32) if w[2] else None
    value, final = combine_model(d, s, c, w)
    return value[0], final[0]


# ---- the reranker ---------------------------------------------------------------------------------------------------------------------
class _M3Model:
    """What CrossEncoderReranker calls its model, scoring by the combined score: predict() -> float32 numpy (the CPU path, the numpy
    model throughout), predict_device_batch() -> an fp32 device tensor (four device calls: rdx_maxsim_f16 through _MaxSimModel,
    rdx_index_score_pairs through Collection.score_pairs_device, rdx_lex_score_pairs, rdx_m3_combine). A pair is (question,
    _Candidate). `last` keeps the components of the last scoring (for tests and tools)."""

    def __init__(self, provider, collection, lexical_index, store: Optional[MultiVectorStore], weights, on_gpu: bool, device: str):
        self.provider, self.collection, self.lexical_index, self.store = provider, collection, lexical_index, store
        self.weights, self.on_gpu, self.device = weights, on_gpu, device
        self._maxsim = _MaxSimModel(provider, store) if weights[2] else None
        self.last: dict = {}

    @property
    def path(self) -> str:
        return "m3" if self.on_gpu else "m3-model"

    @property
    def encoded(self) -> int:
        return self._maxsim.encoded if self._maxsim is not None else 0

    @encoded.setter
    def encoded(self, v: int):
        if self._maxsim is not None:
            self._maxsim.encoded = v

    def _sparse(self, lex, pair_q: np.ndarray, ids):
        """the sparse component of every pair; a candidate the lexical index does not hold scores +0.0"""
        ix = self.lexical_index
        t_ids, t_w, off = lex
        rows = ix.rows_of(ids)
        held = np.flatnonzero(rows >= 0)
        counts = np.diff(off)
        if len(counts) and int(counts.max()) > MAX_TERMS:
            raise ValueError(f"a question has {int(counts.max())} terms; at most {MAX_TERMS} are supported")
        if not self.on_gpu:
            out = np.zeros((len(ids),), dtype=np.float64)
            if len(held) and ix.engine is not None:
                out[held] = sparse_pairs_model(ix.arrays, off, t_ids.cpu().numpy(), t_w.cpu().numpy(), pair_q[held], rows[held])
            return out
        from . import engine as E
        dev = torch.device(self.device)
        out = torch.zeros((len(ids),), dtype=torch.float64, device=dev)
        if len(held) and ix.engine is not None:
            off_p = torch.from_numpy(np.ascontiguousarray(off, dtype=np.int64)).pin_memory()
            self._keep = off_p            # (read by the library and by the kernel: pinned, alive until the caller's copy has drained the stream)
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
            got = E.lex_score_pairs(ix.engine, off_p, t_ids.to(dev).contiguous(), t_w.to(dev).contiguous(), up(pair_q[held]), up(rows[held]))
            if len(held) == len(ids):
                return got
            out[up(held)] = got
        return out

    def _score(self, pairs):
        n = len(pairs)
        w = self.weights
        questions: dict = {}
        pair_q = np.fromiter((questions.setdefault(q, len(questions)) for q, _ in pairs), dtype=np.int32, count=n)
        ids = [c.chunk_id for _, c in pairs]
        missing = [c for c, r in zip(ids, self.collection.rows_of(ids)) if r < 0] if w[0] else []
        if missing:
            raise ValueError(f"the collection does not hold {len(missing)} of the candidates (first: {missing[0]!r})")
        m3 = self.provider.embed_m3_device(list(questions), dense=bool(w[0]), sparse=bool(w[1]), colbert=bool(w[2]))
        dense = sparse = colbert = None
        if w[2]:
            colbert = self._maxsim._score(pairs, q_tokens=m3["tokens"])
        if w[0]:
            if self.on_gpu:
                dense = self.collection.score_pairs_device(m3["dense"].to(torch.device(self.device)), pair_q, ids)
            else:
                dense = self.collection.score_pairs(m3["dense"].cpu().numpy(), pair_q, ids)
        if w[1]:
            sparse = self._sparse(m3["lex"], pair_q, ids)
        if self.on_gpu:
            from . import engine as E
            final, value = E.m3_combine(dense, sparse, colbert, w, want_value=True)
        else:
            value, final = combine_model(dense, sparse, colbert, w)
        self.last = {"dense": dense, "sparse": sparse, "colbert": colbert, "value": value, "final": final}
        return final

    def predict(self, pairs, batch_size: int = 32, show_progress_bar: bool = False) -> np.ndarray:
        if not pairs:
            return np.zeros((0,), dtype=np.float32)
        s = self._score(pairs)
        return s.cpu().numpy() if isinstance(s, torch.Tensor) else s

    def predict_device_batch(self, pairs, batch_size: int = 32) -> torch.Tensor:
        if not self.on_gpu:
            raise RuntimeError("predict_device_batch needs the reranker on a GPU")
        if not 1 <= len(pairs) <= MAX_PAIRS:
            raise ValueError(f"the pair calls score 1 to {MAX_PAIRS} pairs per call, got {len(pairs)}")
        return self._score(pairs)


class M3Reranker(LateInteractionReranker):
    """LateInteractionReranker's interface and flow (rerank, rerank_batch, the boosts, rdx_rerank_select(_batch), the fallback, the
    on-the-fly encoding of candidates the store lacks, last_rerank_stats["encoded"]) with the combined score in place of MaxSim alone.
    `collection`: the Collection holding the chunks' dense rows under their chunk ids (cosine, one device); `lexical_index`: a built
    LexicalChunkIndex; `store`: the MultiVectorStore. A source whose weight is 0 may be None; one that is None with a non-zero weight
    is a ValueError. A candidate the collection does not hold makes the scoring raise, and rerank / rerank_batch then take the
    reference's fallback, as for any scoring failure; a candidate the lexical index does not hold scores sparse +0.0 (a chunk without
    terms, or the index is stale: rebuild to refresh). All sources must live on the reranker's device. min_score=None means no cut."""

    def __init__(self, provider, collection, lexical_index, store: Optional[MultiVectorStore], weights: Sequence[float] = DEFAULT_WEIGHTS,
                 device: Optional[str] = None, min_score: Optional[float] = None, max_length: int = 512):
        w = check_weights(weights)
        for src, wi, name in ((collection, w[0], "collection"), (lexical_index, w[1], "lexical_index"), (store, w[2], "store")):
            if src is None and wi:
                raise ValueError(f"M3Reranker: {name} is None but its weight is {wi}")
        if device is None:
            device = store.device if store is not None and w[2] else "cpu"
            if (store is None or not w[2]) and w[1] and lexical_index is not None and isinstance(getattr(lexical_index, "engine", None), LX.HipLexical):
                device = f"cuda:{lexical_index.device}"
        device = str(device)
        on_gpu = device.startswith("cuda")
        index = torch.device(device).index or 0 if on_gpu else None
        if w[2] and (store.on_gpu != on_gpu or (on_gpu and (torch.device(store.device).index or 0) != index)):
            raise ValueError(f"M3Reranker: the store lives on {store.device}, the reranker was asked to run on {device}")
        if w[1] and on_gpu and int(lexical_index.device) != index:
            raise ValueError(f"M3Reranker: the lexical index lives on device {lexical_index.device}, the reranker was asked to run on {device}")
        if w[0] and on_gpu and int(getattr(collection, "_device", index)) != index:
            raise ValueError(f"M3Reranker: the collection lives on device {collection._device}, the reranker was asked to run on {device}")
        # (CrossEncoderReranker's constructor, through the late-interaction one's own arguments)
        super(LateInteractionReranker, self).__init__(model_name="m3", device=device, max_length=max_length,
                                                      min_score=float("-inf") if min_score is None else float(min_score))
        self.provider, self.store, self.collection, self.lexical_index, self.weights = provider, store, collection, lexical_index, w
        self._model = _M3Model(provider, collection, lexical_index, store if w[2] else None, w, on_gpu, device)
        self._on_gpu = on_gpu
        self._is_loaded = True
        self._nested = False

    def index_chunks(self, chunks, batch_size: int = 256) -> int:
        """encodes the chunks' texts (chunk_text) and stores their token vectors under chunk_id -> chunks stored (the store only: the
        collection and the lexical index are filled by their own builds)"""
        if self._model._maxsim is None:
            raise RuntimeError("M3Reranker.index_chunks: no store (the colbert weight is 0)")
        from .late_interaction import MAX_SLOT_TOKENS
        chunks = list(chunks)
        for a in range(0, len(chunks), batch_size):
            part = chunks[a:a + batch_size]
            vecs, off = self._model._maxsim._vectors([self.chunk_text(c) for c in part], MAX_SLOT_TOKENS)
            self.store.add([c.chunk_id for c in part], (vecs, off))
        return len(chunks)
