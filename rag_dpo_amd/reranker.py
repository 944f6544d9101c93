"""CrossEncoderReranker — same interface as reference src/rag/reranker.py:26-216, MI355X backend.

Reference behaviour mirrored (file:line in the reference's src/rag/reranker.py):
  RankedChunk fields                                                                   :26-34
  ctor kwargs model_name, device, batch_size, max_length, trust_remote_code, min_score  :47-70
  rerank(): [] -> []; pairs (heading + "\\n" + text, cut to max_length * 4 characters);   :112-144
            model.predict(pairs, batch_size=, show_progress_bar=False)                  :147-152
            on an exception: the first top_k candidates in input order, similarity as score :153-160
            final = float(score) (+ topic boost when > 0); stable sort, descending      :162-187
            the first top_k with final >= min_score; at least 3 when n >= 3            :197-206
  is_loaded                                                                            :214-216

What differs underneath. The reference scores with sentence-transformers' CrossEncoder on the CPU (8 ms per pair). Here the model is
an `XLMRobertaForSequenceClassification` checkpoint with one label (bge-reranker-v2-m3's architecture) loaded from a LOCAL directory,
and on a GPU:
  - the backbone runs as ONE packed forward over the pairs' real tokens (`_PackedEncoder`, the embedding provider's forward: fp16 with
    64-wide heads and a hidden size that is a multiple of 512 uses librdx's attention and add + LayerNorm kernels), or, for other
    shapes and dtypes, as transformers' module forward in padded batches of `batch_size`;
  - the classification head, the sigmoid and the selection are librdx kernels (`rdx_rerank_head_f16`, `rdx_rerank_select`, include/rdx.h);
  - a `topic_matcher` that has `topic_boosts_device` and lives on the same GPU (rag_dpo_amd/topics.py) is asked ONCE for all candidates
    and its device tensor goes to the selection as it is; any other matcher is called per candidate, as in the reference.
On the CPU the module forward scores and the selection is the Python below. Jina's reranker (the reference's default) needs remote
code and is not supported: `trust_remote_code` is accepted and never acted on.
`rerank_batch` takes SEVERAL questions: the pairs of all of them go through the packed forward together, so forwards
fill to MAX_FORWARD_TOKENS across questions, then one head call (`rdx_rerank_head_rows_f16`), one boost call
(`rdx_topic_boost_batch`), one selection launch (`rdx_rerank_select_batch`) and ONE copy to the host. What is equal and what is not:
the head, the boosts and the selection are bit for bit the single-question kernels, so with the same scores in, rerank_batch equals
[rerank(...)] exactly. The <s> rows are not promised equal: a batch groups pairs into forwards differently and the BLAS GEMMs may
round differently at another token count; with a real backbone the two agree wherever neighbouring scores differ by more than the
backbone's tolerance (the statement made against the module forward).
One deliberate difference: where the reference keeps nothing (n < 3 candidates, none above min_score, or top_k = 0 with n < 3) its
closing log line indexes the empty result and raises IndexError; here rerank() returns [].
"""
from __future__ import annotations

import logging
import time
from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import torch

from .packed_encoder import _XLMR_LARGE, _HashTokenizer, _PackedEncoder, _resolve_local_dir

logger = logging.getLogger(__name__)

DEFAULT_MODEL = "jinaai/jina-reranker-v2-base-multilingual"
KEEP_MIN = 3                     # reranker.py:204-205
MAX_GPU_CANDIDATES = 1024        # rdx_rerank_head_f16 / rdx_rerank_select
# pairs per device call of rerank_batch: a memory cap (the fp32 <s> rows of 65 536 pairs are 256 MB at H = 1024, the head's workspace 64 MB)
MAX_BATCH_PAIRS = 65536

# XLM-R-base: the Jina reranker's and most multilingual rerankers' width (its backbone takes the module forward: 768 is not a multiple of 512)
_XLMR_BASE = dict(_XLMR_LARGE, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072, max_position_embeddings=514)


@dataclass
class RankedChunk:
    """same fields as reference src/rag/reranker.py:26-34"""
    chunk_id: str
    text: str
    document_path: str
    rerank_score: float
    original_rank: int
    metadata: dict


def _ranked(chunk, score, original_rank: int) -> RankedChunk:
    return RankedChunk(chunk_id=chunk.chunk_id, text=chunk.text, document_path=chunk.document_path, rerank_score=score,
                       original_rank=original_rank, metadata=chunk.metadata)


def select_host(scores, boosts, top_k: int, min_score: float, keep_min: int = KEEP_MIN):
    """The selection of reranker.py:162-206 restated (what rdx_rerank_select computes):
    -> (order: every candidate, final descending, ties in input order; final fp64 per candidate in input order; count)"""
    final = [float(s) for s in scores]
    if boosts is not None:
        for i, b in enumerate(boosts):
            if b > 0:
                final[i] += b
    order = sorted(range(len(final)), key=lambda i: final[i], reverse=True)
    passing = sum(1 for i in order[:top_k] if final[i] >= min_score)
    count = passing
    if count < keep_min and len(final) >= keep_min:
        count = keep_min
    return order, final, count


class _CrossEncoderModel:
    """A loaded XLMRobertaForSequenceClassification (num_labels = 1) with sentence-transformers' CrossEncoder contract:
    predict(pairs, batch_size, show_progress_bar) -> float32 numpy sigmoid scores. predict_device() leaves them on the GPU."""

    # forwards of the packed backbone hold at most this many tokens (memory only: the packed forward pads nothing)
    MAX_FORWARD_TOKENS = 32768

    def __init__(self, model, tokenize, device: str, dtype: torch.dtype, packed: Optional[bool] = None):
        self.model = model
        self.tokenize = tokenize                     # (queries, texts) -> {"input_ids", "attention_mask"} right-padded, int64
        self.device = str(device)
        self.on_gpu = self.device.startswith("cuda")
        self.hidden = int(model.config.hidden_size)
        self.stats: dict = {}
        self._packed = None
        self._lib = None
        use_packed = self.on_gpu if packed is None else bool(packed)
        if use_packed:
            try:
                fused = self.on_gpu and dtype == torch.float16
                self._packed = _PackedEncoder(model.roberta, fused=fused, graphs=False)   # eager: graph capture of the rerank forward is not part of this path
                if self.on_gpu and not self._packed.fused:
                    self._packed = None              # another GPU shape or dtype: the module backbone, then the head kernel
            except ValueError as e:
                logger.info(f"packed forward not available for this reranker ({e}); using the module forward")
        if self.on_gpu:
            from . import _lib
            self._lib = _lib.load()                  # raises RdxUnavailable: the GPU path has no torch substitute
            c = model.classifier
            H = self.hidden
            if H % 64 or H > 4096:
                raise ValueError(f"rdx_rerank_head_f16 takes a hidden size that is a multiple of 64 up to 4096, not {H}")
            f16 = dict(dtype=torch.float16, device=self.device)
            self.w_d = c.dense.weight.detach().to(**f16).contiguous()
            self.b_d = c.dense.bias.detach().to(**f16).contiguous()
            self.w_o = c.out_proj.weight.detach().to(**f16).reshape(H).contiguous()
            self.b_o = c.out_proj.bias.detach().to(**f16).reshape(1).contiguous()

    @property
    def path(self) -> str:
        if not self.on_gpu:
            return "cpu-packed" if self._packed is not None else "cpu-module"
        return "fused" if self._packed is not None else "module+kernels"

    def _to_dev(self, name, t, out=None):
        return t.to(self.device) if out is None else out.copy_(t)

    @torch.no_grad()
    def _cls_rows(self, pairs, batch_size: int) -> torch.Tensor:
        """fp32 [n][hidden] final hidden states of the pairs' <s> tokens, in input order, on the model's device"""
        n = len(pairs)
        t0 = time.perf_counter()
        enc = self.tokenize([p[0] for p in pairs], [p[1] for p in pairs])
        ids, lens = enc["input_ids"], enc["attention_mask"].numpy().sum(axis=1)
        self.stats.update(tokens=int(lens.sum()), ms_tokenize=(time.perf_counter() - t0) * 1e3)
        out = torch.empty((n, self.hidden), dtype=torch.float32, device=self.device)
        if self._packed is not None:
            # length-sorted groups of at most MAX_FORWARD_TOKENS tokens, each one packed forward (short pairs land together: a group
            # whose pairs all fit 64 tokens takes the VALU attention kernel, any other the MFMA one)
            by = np.argsort(-lens, kind="stable")
            start = 0
            while start < n:
                stop, tok = start, 0
                while stop < n and (stop == start or tok + int(lens[by[stop]]) <= self.MAX_FORWARD_TOKENS):
                    tok += int(lens[by[stop]])
                    stop += 1
                rows = by[start:stop]
                width = int(lens[rows[0]])
                cls = self._packed.cls(torch.from_numpy(ids.numpy()[rows, :width]), lens[rows], self._to_dev)
                out[torch.from_numpy(rows).to(self.device)] = cls
                start = stop
            return out
        for a in range(0, n, batch_size):                    # the module forward, padded batches as sentence-transformers runs it
            lo, hi = a, min(n, a + batch_size)
            w = int(lens[lo:hi].max())
            feed = {"input_ids": ids[lo:hi, :w].to(self.device), "attention_mask": enc["attention_mask"][lo:hi, :w].to(self.device)}
            out[lo:hi] = self.model.roberta(**feed).last_hidden_state[:, 0].to(torch.float32)
        return out

    def _head(self, cls: torch.Tensor, head_fn: str) -> torch.Tensor:
        """the entry point head_fn (rdx_rerank_head_f16 or rdx_rerank_head_rows_f16) on fp32 CLS rows -> fp32 sigmoid scores on the device"""
        from . import _lib as L
        n, H = int(cls.shape[0]), self.hidden
        cls = cls.contiguous()
        ws = torch.empty(((H // L.RERANK_FEATURES) * n,), dtype=torch.float64, device=cls.device)
        scores = torch.empty((n,), dtype=torch.float32, device=cls.device)
        st = torch.cuda.current_stream(cls.device).cuda_stream
        L.check(getattr(self._lib, head_fn)(cls.device.index or 0, cls.data_ptr(), n, H, self.w_d.data_ptr(), self.b_d.data_ptr(), self.w_o.data_ptr(),
                        self.b_o.data_ptr(), ws.data_ptr(), scores.data_ptr(), st))
        return scores

    def head_device(self, cls: torch.Tensor) -> torch.Tensor:
        """rdx_rerank_head_f16 on fp32 CLS rows -> fp32 sigmoid scores on the device"""
        return self._head(cls, "rdx_rerank_head_f16")

    @torch.no_grad()
    def _predict_on_device(self, pairs, batch_size: int, head_fn: str, what: str, refusal) -> torch.Tensor:
        """the backbone's <s> rows, then head_fn on them, with the three events of the stats around the two steps. what: the caller's
        name; refusal: None, or why it does not take this many pairs"""
        if not self.on_gpu:
            raise RuntimeError(f"{what} needs the model on a GPU")
        if refusal:
            raise ValueError(refusal)
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        cls = self._cls_rows(pairs, batch_size)
        e1.record()
        scores = self._head(cls, head_fn)
        e2.record()
        self.stats["events"] = (e0, e1, e2)
        return scores

    def predict_device(self, pairs, batch_size: int = 32, show_progress_bar: bool = False) -> torch.Tensor:
        n = len(pairs)
        return self._predict_on_device(pairs, batch_size, "rdx_rerank_head_f16", "predict_device",
                                       n > MAX_GPU_CANDIDATES and f"the GPU reranker scores at most {MAX_GPU_CANDIDATES} candidates per call, got {n}")

    def predict_device_batch(self, pairs, batch_size: int = 32) -> torch.Tensor:
        """predict_device for the pairs of several questions (any number up to rdx_rerank_head_rows_f16's 2^20): _cls_rows sorts by
        length and groups across questions, the head runs once. A row's score has the bits rdx_rerank_head_f16 gives that <s> row."""
        from . import _lib as L
        n = len(pairs)
        return self._predict_on_device(pairs, batch_size, "rdx_rerank_head_rows_f16", "predict_device_batch",
                                       not 1 <= n <= L.RERANK_BATCH_MAX_ROWS and f"the GPU reranker scores 1 to {L.RERANK_BATCH_MAX_ROWS} pairs per call, got {n}")

    @torch.no_grad()
    def predict(self, pairs, batch_size: int = 32, show_progress_bar: bool = False) -> np.ndarray:
        if not pairs:
            return np.zeros((0,), dtype=np.float32)
        if self.on_gpu:
            return self.predict_device(pairs, batch_size).cpu().numpy()
        if self._packed is not None:
            cls = self._cls_rows(pairs, batch_size)
            return torch.sigmoid(self.model.classifier(cls[:, None, :]).reshape(-1)).to(torch.float32).numpy()
        out = []
        enc = self.tokenize([p[0] for p in pairs], [p[1] for p in pairs])
        lens = enc["attention_mask"].numpy().sum(axis=1)
        self.stats.update(tokens=int(lens.sum()))
        for a in range(0, len(pairs), batch_size):
            lo, hi = a, min(len(pairs), a + batch_size)
            w = int(lens[lo:hi].max())
            logits = self.model(input_ids=enc["input_ids"][lo:hi, :w], attention_mask=enc["attention_mask"][lo:hi, :w]).logits
            out.append(torch.sigmoid(logits.reshape(-1).to(torch.float32)))
        return torch.cat(out).numpy()


def _random_config(spec: str) -> dict:
    cfg = dict(_XLMR_LARGE, max_position_embeddings=514)        # bge-reranker-v2-m3: XLM-R-large, 512-token pairs
    if spec.startswith("tiny"):
        cfg.update(hidden_size=64, num_hidden_layers=2, num_attention_heads=4, intermediate_size=128, vocab_size=1000)
    elif spec.startswith("mid"):
        cfg.update(hidden_size=512, num_hidden_layers=3, num_attention_heads=8, intermediate_size=1024, vocab_size=1000)
    elif spec == "xlm-roberta-base":
        cfg = dict(_XLMR_BASE)
    elif spec != "xlm-roberta-large":
        raise ValueError(f"unknown random-init spec '{spec}': tiny, mid, xlm-roberta-base or xlm-roberta-large")
    return cfg


class CrossEncoderReranker:
    """Rescoring of retrieved candidates by a cross-encoder (question, chunk) -> relevance in [0, 1]."""

    def __init__(self, model_name: str = DEFAULT_MODEL, device: str = "cpu", batch_size: int = 32, max_length: int = 512,
                 trust_remote_code: bool = True, min_score: float = 0.08, dtype: Optional[torch.dtype] = None,
                 cache_dir: Optional[str] = None):
        self.model_name = model_name
        self.device = device
        self.batch_size = batch_size
        self.max_length = max_length
        self.trust_remote_code = trust_remote_code   # accepted for the reference's signature; remote code is never run
        self.min_score = min_score
        self.dtype = dtype if dtype is not None else (torch.float16 if str(device).startswith("cuda") else torch.float32)
        self.cache_dir = cache_dir
        self._model = None
        self._is_loaded = False
        self.last_rerank_stats: Optional[dict] = None

    # None: the packed backbone on a GPU, the module forward on the CPU; True: the packed forward on the CPU too (tests)
    packed_forward: Optional[bool] = None

    @property
    def is_loaded(self) -> bool:
        return self._is_loaded

    def _load_model(self):
        if self._is_loaded or self._model is not None:
            return
        t0 = time.time()
        from transformers import XLMRobertaConfig, XLMRobertaForSequenceClassification
        if self.model_name.startswith("random-init:"):
            cfg = _random_config(self.model_name.split(":", 1)[1])
            torch.manual_seed(0)
            model = XLMRobertaForSequenceClassification(XLMRobertaConfig(**cfg, num_labels=1))
            hash_tok = _HashTokenizer(cfg["vocab_size"])
            tokenize = lambda q, d: hash_tok.pairs(q, d, self.max_length)   # noqa: E731
        else:
            local = _resolve_local_dir(self.model_name, self.cache_dir)
            if local is None:
                raise RuntimeError(
                    f"CrossEncoderReranker: no local checkpoint for '{self.model_name}' (looked in the name itself and under "
                    f"cache_dir={self.cache_dir!r}). This build never downloads models; pass a directory holding an "
                    "XLMRobertaForSequenceClassification checkpoint with num_labels = 1 (e.g. bge-reranker-v2-m3).")
            from transformers import AutoConfig, AutoTokenizer
            supported = ("CrossEncoderReranker supports XLMRobertaForSequenceClassification checkpoints with num_labels = 1 "
                         "(bge-reranker-v2-m3 and its kind); checkpoints that need remote code are not supported")
            try:
                cfg = AutoConfig.from_pretrained(local, local_files_only=True, trust_remote_code=False)
            except Exception as e:  # noqa: BLE001  (e.g. a configuration class that only remote code defines)
                raise ValueError(f"{supported}: '{self.model_name}' has no loadable configuration ({e})") from e
            archs = list(getattr(cfg, "architectures", None) or [])
            if cfg.model_type != "xlm-roberta" or archs != ["XLMRobertaForSequenceClassification"] or int(cfg.num_labels) != 1:
                raise ValueError(f"{supported}: '{self.model_name}' is model_type={cfg.model_type!r}, architectures={archs}, "
                                 f"num_labels={cfg.num_labels}")
            model = XLMRobertaForSequenceClassification.from_pretrained(local, local_files_only=True)
            tok = AutoTokenizer.from_pretrained(local, local_files_only=True)
            max_length = self.max_length
            tokenize = lambda q, d: tok(list(q), list(d), padding=True, truncation="longest_first", max_length=max_length,   # noqa: E731
                                        return_tensors="pt")
        model = model.to(device=self.device, dtype=self.dtype).eval()
        self._model = _CrossEncoderModel(model, tokenize, self.device, self.dtype, packed=self.packed_forward)
        self._is_loaded = True
        logger.info(f"cross-encoder {self.model_name} loaded on {self.device} in {time.time() - t0:.1f}s ({self._model.path})")

    def _scores(self, pairs):
        """-> (scores: fp32 device tensor on the GPU path, else float32 numpy; path name). Exceptions propagate."""
        m = self._model
        gpu = str(self.device).startswith("cuda")
        if gpu and hasattr(m, "predict_device"):
            return m.predict_device(pairs, batch_size=self.batch_size, show_progress_bar=False), getattr(m, "path", "device")
        s = m.predict(pairs, batch_size=self.batch_size, show_progress_bar=False)
        return s, getattr(m, "path", "predict")

    def rerank(self, query: str, chunks: List, top_k: int = 8, topic_matcher=None,
               question_topics: Optional[List[str]] = None) -> List[RankedChunk]:
        if not chunks:
            return []
        self._load_model()
        pairs = self._pairs(query, chunks)
        stats = {"pairs": len(pairs), "tokens": None, "ms_forward": None, "ms_head_select": None}
        self.last_rerank_stats = stats
        t0 = time.perf_counter()
        try:
            scores, path = self._scores(pairs)
        except Exception as e:                                   # reranker.py:153-160
            logger.error(f"reranking failed: {e}")
            stats["path"] = "fallback"
            return [_ranked(c, c.similarity_score, i) for i, c in enumerate(chunks[:top_k])]
        stats["path"] = path
        n = min(len(chunks), len(scores))                        # (zip(chunks, scores), reranker.py:166)
        boosts = None
        if topic_matcher is not None and question_topics:
            if self._boosts_on_device(topic_matcher, n):
                # all candidates in one call, left where rdx_rerank_select reads them (rag_dpo_amd/topics.py): no host list, no upload
                boosts = topic_matcher.topic_boosts_device(question_topics, [c.metadata.get("rgpd_topics", "") for c in chunks[:n]])
            else:
                boosts = [topic_matcher.topic_boost(question_topics, c.metadata.get("rgpd_topics", "")) for c in chunks[:n]]
                hit = sum(1 for b in boosts if b > 0)
                if hit:
                    logger.info(f"topic boost applied to {hit}/{n} chunks")
        if str(self.device).startswith("cuda"):
            order, final, count = self._select_device(scores, boosts, n, top_k, stats)
        else:
            scores = scores.cpu().numpy() if isinstance(scores, torch.Tensor) else scores
            order, final, count = select_host(scores[:n], boosts, top_k, self.min_score)
        stats["ms_total"] = (time.perf_counter() - t0) * 1e3
        stats["kept"] = count
        m = self._model
        if isinstance(m, _CrossEncoderModel):
            stats["tokens"] = m.stats.get("tokens")
            stats["ms_tokenize"] = m.stats.get("ms_tokenize")
            ev = m.stats.pop("events", None)
            if ev is not None and "events" in stats:
                stats["ms_forward"] = ev[0].elapsed_time(ev[1])
                stats["ms_head_select"] = ev[1].elapsed_time(ev[2]) + stats["events"][0].elapsed_time(stats["events"][1])
            elif ev is not None:
                stats["ms_forward"] = ev[0].elapsed_time(ev[1])
        stats.pop("events", None)
        return [_ranked(chunks[i], final[i], i) for i in order[:count]]

    def _pairs(self, query: str, chunks) -> list:
        """the (question, text) pairs of rerank(): heading prefix, then the max_length * 4 character cut (reranker.py:131-144)"""
        pairs = []
        for chunk in chunks:
            text = chunk.text
            heading = chunk.metadata.get("heading", "")
            if heading:
                text = f"{heading}\n{text}"
            pairs.append((query, text[:self.max_length * 4]))
        return pairs

    def rerank_batch(self, queries, chunks_lists, top_k: int = 8, topic_matcher=None, question_topics=None) -> List[List[RankedChunk]]:
        """rerank() of every question: [rerank(queries[i], chunks_lists[i], top_k, topic_matcher, question_topics[i])].
        question_topics: None, or one list (or None) per question. On a GPU the pairs of all questions are scored together and the
        boosts and the selection of all questions run in one call each, with one copy to the host at the end (module docstring:
        the head, the boosts and the selection are the single-question kernels bit for bit; the backbone's <s> rows are equal up to
        its tolerance only, because pairs are grouped into forwards differently). Questions are cut into device calls of at most
        MAX_BATCH_PAIRS pairs. A question with more than 1024 candidates takes rerank(); one without candidates gives []. On the
        CPU this is the loop. If the batched scoring raises, every question of that call goes through rerank(), which has the
        reference's own fallback."""
        queries, chunks_lists = list(queries), [list(c) if c else [] for c in chunks_lists]
        nq = len(queries)
        if len(chunks_lists) != nq:
            raise ValueError(f"rerank_batch: {len(chunks_lists)} candidate lists for {nq} questions")
        topics = [None] * nq if question_topics is None else list(question_topics)
        if len(topics) != nq:
            raise ValueError(f"rerank_batch: question_topics has {len(topics)} entries for {nq} questions")
        one = lambda i: self.rerank(queries[i], chunks_lists[i], top_k=top_k, topic_matcher=topic_matcher, question_topics=topics[i])   # noqa: E731
        if not str(self.device).startswith("cuda"):
            return [one(i) for i in range(nq)]
        from . import _lib as L
        out: List[Optional[List[RankedChunk]]] = [None] * nq
        groups, group, held = [], [], 0
        for i, chunks in enumerate(chunks_lists):
            if not chunks:
                out[i] = []
            elif len(chunks) > MAX_GPU_CANDIDATES:
                out[i] = one(i)
            else:
                if group and (held + len(chunks) > MAX_BATCH_PAIRS or len(group) >= L.RERANK_BATCH_MAX_QUESTIONS):
                    groups.append(group)
                    group, held = [], 0
                group.append(i)
                held += len(chunks)
        if group:
            groups.append(group)
        if not groups:
            return out
        self._load_model()
        total = {"questions": 0, "pairs": 0, "tokens": None, "ms_forward": None, "ms_head_select": None, "path": None, "kept": 0, "device_calls": 0}
        t0 = time.perf_counter()
        for group in groups:
            ranked = self._rerank_group(group, queries, chunks_lists, topics, top_k, topic_matcher, total)
            if ranked is None:                                       # the scoring raised: the reference's fallback, question by question
                ranked = [one(i) for i in group]
                total["path"] = "loop"
            for i, r in zip(group, ranked):
                out[i] = r
        total["ms_total"] = (time.perf_counter() - t0) * 1e3
        self.last_rerank_stats = total
        return out

    def _rerank_group(self, group, queries, chunks_lists, topics, top_k, topic_matcher, total):
        """one device call of rerank_batch over the questions `group` (each 1 to 1024 candidates) -> their results, or None when the
        scoring raised"""
        from . import _lib as L
        lib = L.load()
        m = self._model
        dev = torch.device(self.device)
        pairs, cand_off = [], [0]
        for i in group:
            pairs.extend(self._pairs(queries[i], chunks_lists[i]))
            cand_off.append(len(pairs))
        n_total, nq = len(pairs), len(group)
        try:
            if hasattr(m, "predict_device_batch"):
                scores, path = m.predict_device_batch(pairs, batch_size=self.batch_size), getattr(m, "path", "device")
            else:
                s = np.asarray(m.predict(pairs, batch_size=self.batch_size, show_progress_bar=False), dtype=np.float32).reshape(-1)
                if len(s) != n_total:
                    raise ValueError(f"predict returned {len(s)} scores for {n_total} pairs")
                scores, path = torch.from_numpy(np.ascontiguousarray(s)).to(dev), getattr(m, "path", "predict")
        except Exception as e:  # noqa: BLE001
            logger.error(f"batched reranking failed ({e}): question by question")
            return None
        scores = scores.contiguous()
        dev = scores.device
        # boosts: the matcher's batched device call where it has one on this GPU, else the reference's call per candidate
        boosts, counted = None, [False] * nq
        wants = [topic_matcher is not None and bool(topics[i]) for i in group]
        if any(wants):
            tags = lambda i: [c.metadata.get("rgpd_topics", "") for c in chunks_lists[i]]   # noqa: E731
            if hasattr(topic_matcher, "topic_boosts_device_batch") and self._boosts_on_device(topic_matcher, 1):
                boosts = topic_matcher.topic_boosts_device_batch([topics[i] if w else [] for i, w in zip(group, wants)], [tags(i) for i in group])
                if boosts.dtype != torch.float64 or boosts.device != dev or boosts.numel() != n_total:
                    raise ValueError(f"topic_boosts_device_batch must return fp64 [{n_total}] on {dev}, got {boosts.dtype} [{boosts.numel()}] on {boosts.device}")
                boosts = boosts.contiguous()
                counted = wants
            else:
                host = np.zeros((n_total,), dtype=np.float64)
                for q, (i, w) in enumerate(zip(group, wants)):
                    if not w:
                        continue
                    b = [topic_matcher.topic_boost(topics[i], t) for t in tags(i)]
                    host[cand_off[q]:cand_off[q + 1]] = b
                    hit = sum(1 for x in b if x > 0)
                    if hit:
                        logger.info(f"topic boost applied to {hit}/{len(b)} chunks")
                boosts = torch.from_numpy(host).to(dev)
        # one output buffer, one copy back: final fp64 [n_total] | order int32 [n_total] | count int32 [nq] | boosted int32 [nq]
        buf = torch.empty((8 * n_total + 4 * n_total + 8 * nq,), dtype=torch.uint8, device=dev)
        base = buf.data_ptr()
        shape = torch.tensor(cand_off, dtype=torch.int32).pin_memory()   # (read by the library here and by the kernel: pinned; alive until the copy below has drained the stream)
        s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s0.record()
        L.check(lib.rdx_rerank_select_batch(dev.index or 0, scores.data_ptr(), boosts.data_ptr() if boosts is not None else None, nq,
                                            shape.data_ptr(), int(top_k), float(self.min_score), KEEP_MIN, base + 8 * n_total, base,
                                            base + 12 * n_total, base + 12 * n_total + 4 * nq, torch.cuda.current_stream(dev).cuda_stream))
        s1.record()
        host = buf.cpu().numpy()                                         # THE copy: it drains the stream
        final = host[:8 * n_total].view(np.float64)
        order = host[8 * n_total:12 * n_total].view(np.int32)
        count = host[12 * n_total:12 * n_total + 4 * nq].view(np.int32)
        boosted = host[12 * n_total + 4 * nq:].view(np.int32)
        ranked = []
        for q, i in enumerate(group):
            lo, chunks = cand_off[q], chunks_lists[i]
            if counted[q] and boosted[q]:
                logger.info(f"topic boost applied to {int(boosted[q])}/{len(chunks)} chunks")
            ranked.append([_ranked(chunks[p], float(final[lo + p]), p) for p in order[lo:lo + int(count[q])].tolist()])
        add = lambda k, v: total.__setitem__(k, v if total[k] is None else total[k] + v)   # noqa: E731
        total["questions"] += nq
        total["pairs"] += n_total
        total["kept"] += int(count.sum())
        total["device_calls"] += 1
        total["path"] = path
        ms_select = s0.elapsed_time(s1)
        if isinstance(m, _CrossEncoderModel):
            if m.stats.get("tokens") is not None:
                add("tokens", m.stats["tokens"])
            ev = m.stats.pop("events", None)
            if ev is not None:
                add("ms_forward", ev[0].elapsed_time(ev[1]))
                ms_select += ev[1].elapsed_time(ev[2])
        add("ms_head_select", ms_select)
        return ranked

    def _boosts_on_device(self, topic_matcher, n: int) -> bool:
        """a matcher with topic_boosts_device whose table lives on the GPU this reranker selects on"""
        if not str(self.device).startswith("cuda") or not hasattr(topic_matcher, "topic_boosts_device") or not 1 <= n <= MAX_GPU_CANDIDATES:
            return False
        mine, theirs = torch.device(self.device), getattr(topic_matcher, "device", None)
        if not isinstance(theirs, torch.device) or theirs.type != "cuda":
            return False
        index = lambda d: torch.cuda.current_device() if d.index is None else d.index   # noqa: E731
        return index(mine) == index(theirs)

    def _select_device(self, scores, boosts, n: int, top_k: int, stats: dict):
        """rdx_rerank_select on the GPU: scores from the head kernel (device tensor) or from a model's predict() (numpy); boosts None,
        a host list, or the fp64 device tensor of TopicMatcher.topic_boosts_device"""
        from . import _lib as L
        if n > MAX_GPU_CANDIDATES:
            raise ValueError(f"the GPU reranker selects among at most {MAX_GPU_CANDIDATES} candidates per call, got {n}")
        lib = L.load()
        dev = torch.device(self.device)
        if not isinstance(scores, torch.Tensor):
            scores = torch.from_numpy(np.ascontiguousarray(np.asarray(scores, dtype=np.float32)[:n])).to(dev)
        scores = scores[:n].contiguous()
        dev = scores.device
        b = None
        if isinstance(boosts, torch.Tensor):
            if boosts.dtype != torch.float64 or boosts.device != dev or boosts.numel() < n:
                raise ValueError(f"topic_boosts_device must return fp64 [{n}] on {dev}, got {boosts.dtype} [{boosts.numel()}] on {boosts.device}")
            b = boosts[:n].contiguous()
        elif boosts is not None:
            b = torch.from_numpy(np.asarray([float(x) for x in boosts], dtype=np.float64)).to(dev)
        order = torch.empty((n,), dtype=torch.int32, device=dev)
        final = torch.empty((n,), dtype=torch.float64, device=dev)
        count = torch.empty((1,), dtype=torch.int32, device=dev)
        s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s0.record()
        L.check(lib.rdx_rerank_select(dev.index or 0, scores.data_ptr(), b.data_ptr() if b is not None else None, n, int(top_k),
                                      float(self.min_score), KEEP_MIN, order.data_ptr(), final.data_ptr(), count.data_ptr(),
                                      torch.cuda.current_stream(dev).cuda_stream))
        s1.record()
        c = int(count.item())                                    # (synchronises the stream: the events below are complete)
        stats["events"] = (s0, s1)
        if isinstance(boosts, torch.Tensor):                     # (the stream is drained: the copy waits for nothing)
            hit = int((b.cpu().numpy() > 0).sum())
            if hit:
                logger.info(f"topic boost applied to {hit}/{n} chunks")
        return order[:c].cpu().tolist(), final.cpu().tolist(), c
