"""Host-side fusion either side of the dense hot path: the dense part of the reference's
`RAGRetriever.retrieve_candidates` / `.retrieve` (src/rag/retriever.py:156-470) restated so that the ≤ 4 queries
of one question are embedded in ONE batch and searched in ONE `collection.query` call (B = 4 instead of four
B = 1 round trips) while every per-query result, the rank fusion, the score merge and the
document de-duplication stay identical to the reference's.

Pinned by tests/golden/retriever_golden.json, captured by driving the IMPORTED reference retriever
(tests/golden/make_retriever_golden.py) with the same collection and embedder.
Hybrid retrieval: given the BM25 indexes of rag_dpo_amd/bm25.py (summary pre-filter and chunk index), both methods
follow the reference per method (retriever.py:187-285, :355-452): the summary pre-filter of the main query, the dense
list filtered by it and topped up to 5 (retrieve) / 10 (retrieve_candidates), the BM25 rankings interleaved with the
dense ones in the reference's order (RRF sums in ranking order), BM25-only chunks at distance 1.0. retrieve searches BM25
for the main query only; retrieve_candidates for every sub-query, all in ONE batched device call.
Pinned by tests/golden/bm25_golden.json. LLM query expansion stays out of scope: it is an injected callable.
"""
from __future__ import annotations

import logging
from collections import defaultdict
from dataclasses import dataclass
from typing import Any, Callable, Dict, List, Optional, Sequence


logger = logging.getLogger(__name__)


@dataclass
class RetrievedChunk:
    """same fields as reference src/rag/retriever.py:22-42"""
    chunk_id: str
    text: str
    document_path: str
    chunk_nature: str
    chunk_index: int
    confidence: str
    distance: float
    metadata: Dict[str, Any]
    bm25_score: float = 0.0
    semantic_score: float = 0.0
    hybrid_score: float = 0.0

    @property
    def similarity_score(self) -> float:
        return 1.0 / (1.0 + self.distance)          # reference retriever.py:39-42


@dataclass
class RetrievedDocument:
    """reference src/rag/retriever.py:45-63"""
    document_path: str
    chunks: List[RetrievedChunk]
    avg_similarity: float = 0.0
    primary_nature: str = ""

    def __post_init__(self):
        if self.chunks:
            self.avg_similarity = sum(c.similarity_score for c in self.chunks) / len(self.chunks)
            natures = [c.chunk_nature for c in self.chunks]
            self.primary_nature = max(set(natures), key=natures.count)
        else:
            self.avg_similarity = 0.0
            self.primary_nature = "UNKNOWN"


def reciprocal_rank_fusion(rankings: Sequence[Sequence[str]], k: int = 60,
                           weights: Optional[Sequence[float]] = None) -> Dict[str, float]:
    """score(id) = sum_i w_i / (k + rank_i + 1)   — reference src/rag/retriever.py:66-90"""
    if weights is None:
        weights = [1.0] * len(rankings)
    scores: Dict[str, float] = defaultdict(float)
    for ranking, weight in zip(rankings, weights):
        for rank, doc_id in enumerate(ranking):
            scores[doc_id] += weight / (k + rank + 1)
    return dict(scores)


def parse_query_results(results: Dict, b: int = 0) -> List[RetrievedChunk]:
    """reference src/rag/retriever.py:472-494 for the b-th query of a batched result"""
    chunks = []
    for chunk_id, text, metadata, distance in zip(results["ids"][b], results["documents"][b],
                                                  results["metadatas"][b], results["distances"][b]):
        metadata = metadata or {}
        chunks.append(RetrievedChunk(
            chunk_id=chunk_id, text=text, document_path=metadata.get("document_path", ""),
            chunk_nature=metadata.get("chunk_nature", "UNKNOWN"), chunk_index=metadata.get("chunk_index", 0),
            confidence=metadata.get("confidence", "unknown"), distance=distance, metadata=metadata))
    return chunks


class DenseRetriever:
    def __init__(self, collection, embedding_provider, query_expander: Optional[Callable[[str], List[str]]] = None,
                 query_preprocessor: Optional[Callable[[str], str]] = None, n_documents: int = 5,
                 n_chunks_per_doc: int = 3, fetch_multiplier: int = 10, summary_bm25_index=None, chunk_bm25_index=None,
                 summary_prefilter_k: int = 20, enable_hybrid: bool = True, enable_summary_prefilter: bool = True,
                 fusion: str = "auto"):
        if fusion not in ("auto", "device", "host"):
            raise ValueError(f"fusion must be 'auto', 'device' or 'host', got {fusion!r}")
        self.fusion = fusion                            # how retrieve_candidates_batch fuses: rag_dpo_amd/fusion.py, or the loop
        self.collection = collection
        self.embedding_provider = embedding_provider
        self.query_expander = query_expander            # reference: QueryExpander.expand (LLM, out of scope)
        self.query_preprocessor = query_preprocessor    # reference: expand_query_with_acronyms (string op, out of scope)
        self.n_documents = n_documents
        self.n_chunks_per_doc = n_chunks_per_doc
        self.fetch_multiplier = fetch_multiplier
        self.summary_bm25 = summary_bm25_index          # reference: SummaryBM25Index (pre-filter), rag_dpo_amd.bm25
        self.chunk_bm25 = chunk_bm25_index              # reference: ChunkBM25Index (sparse ranking), rag_dpo_amd.bm25
        self.summary_prefilter_k = summary_prefilter_k
        self.enable_hybrid = enable_hybrid
        self.enable_summary_prefilter = enable_summary_prefilter

    # one batched device round trip for all the queries of a question
    def _dense(self, all_queries: List[str], n_fetch: int, where_filter):
        """-> per sub-query its chunks, or None where `collection.query` raised for that sub-query: the reference calls
        query once per sub-query inside a try and skips a failing one (src/rag/retriever.py:215-223, 380-388; an embed
        failure is NOT caught there, :212, :377). Here the sub-queries go down as ONE batch; only when that batched call
        raises (e.g. one NaN embedding rejects the batch) they are re-issued one at a time, so one bad sub-query costs
        exactly that sub-query, as in the reference."""
        vectors = self.embedding_provider.embed(all_queries)       # reference: one embed([q]) per query (:212, :377)
        include = ["documents", "metadatas", "distances"]
        try:
            results = self.collection.query(query_embeddings=vectors, n_results=n_fetch, where=where_filter, include=include)
            return [parse_query_results(results, b) for b in range(len(all_queries))]
        except Exception as e:
            logger.error("collection.query failed for the batch of %d sub-queries (%s): retrying one by one", len(all_queries), e)
        out: List[Optional[List[RetrievedChunk]]] = []
        for q_idx, v in enumerate(vectors):
            try:
                res = self.collection.query(query_embeddings=[v], n_results=n_fetch, where=where_filter, include=include)
                out.append(parse_query_results(res, 0))
            except Exception as e:
                logger.error("collection.query failed (%s): %s", "principale" if q_idx == 0 else f"expansion #{q_idx}", e)
                out.append(None)                                   # reference: `continue` (:221-223, :386-388)
        return out

    def _queries(self, query: str) -> List[str]:
        return self._expand(query)[1]

    def _expand(self, query: str):
        """-> (the preprocessed main query, all sub-queries)"""
        expanded = self.query_preprocessor(query) if self.query_preprocessor else query
        return expanded, (list(self.query_expander(expanded)) if self.query_expander is not None else [expanded])

    def _doc_filter(self, expanded: str):
        """the summary pre-filter of the main query (reference :187-196, :355-363), or None"""
        if self.enable_summary_prefilter and self.summary_bm25 is not None and self.summary_bm25._is_built:
            return self.summary_bm25.get_relevant_doc_paths(expanded, top_k=self.summary_prefilter_k)
        return None

    def _doc_filters(self, expanded: Sequence[str]):
        """_doc_filter of every main query, the summary searches in one device call"""
        if self.enable_summary_prefilter and self.summary_bm25 is not None and self.summary_bm25._is_built:
            return self.summary_bm25.get_relevant_doc_paths_batch(list(expanded), top_k=self.summary_prefilter_k)
        return [None] * len(expanded)

    def _hybrid(self) -> bool:
        return self.enable_hybrid and self.chunk_bm25 is not None and self.chunk_bm25.is_built

    def _fuse(self, per_query: List[List[RetrievedChunk]], extra_rankings=(), extra_weights=(), bm25=None, doc_filter=None,
              min_semantic: int = 5, bm25_keep_max: bool = False):
        """bm25: per sub-query None or (its BM25 results, the ranking's weight); its ranking follows that sub-query's dense one"""
        all_rankings, weights = [], []
        chunk_map: Dict[str, RetrievedChunk] = {}
        for q_idx, chunks in enumerate(per_query):
            if chunks is None:                                     # skipped sub-query: no ranking, no weight, no BM25
                continue
            if doc_filter:                                         # reference :226-232, :391-397 (an empty filter filters nothing)
                filtered = [c for c in chunks if c.document_path in doc_filter]
                if len(filtered) < min_semantic:
                    kept = {id(c) for c in filtered}
                    filtered.extend([c for c in chunks if id(c) not in kept][:min_semantic - len(filtered)])
                chunks = filtered
            for c in chunks:
                c.semantic_score = c.similarity_score
            all_rankings.append([c.chunk_id for c in chunks])
            weights.append(2.0 if q_idx == 0 else 1.0)             # reference :209, :374
            for c in chunks:                                       # reference :246-256, :407-415
                old = chunk_map.get(c.chunk_id)
                if old is None:
                    chunk_map[c.chunk_id] = c
                else:
                    if c.distance < old.distance:
                        old.distance = c.distance
                    if c.semantic_score > old.semantic_score:
                        old.semantic_score = c.semantic_score
            if bm25 is not None and bm25[q_idx] is not None:       # reference :258-285, :417-452
                results, weight = bm25[q_idx]
                all_rankings.append([r.doc_key for r in results])
                weights.append(weight)
                for r in results:
                    c = chunk_map.get(r.doc_key)
                    if c is None:
                        meta = dict(r.metadata)
                        text = meta.pop("text", "")
                        c = chunk_map[r.doc_key] = RetrievedChunk(
                            chunk_id=r.doc_key, text=text, document_path=meta.get("document_path", ""),
                            chunk_nature=meta.get("chunk_nature", "UNKNOWN"), chunk_index=meta.get("chunk_index", 0),
                            confidence=meta.get("confidence", "unknown"), distance=1.0, metadata=meta)
                    c.bm25_score = max(c.bm25_score, r.score) if bm25_keep_max else r.score
        all_rankings += [list(r) for r in extra_rankings]
        weights += list(extra_weights)
        if len(all_rankings) > 1:                                  # reference :293-300, :455-462
            rrf = reciprocal_rank_fusion(all_rankings, weights=weights)
            for cid, c in chunk_map.items():
                c.hybrid_score = rrf.get(cid, 0.0)
        else:
            for c in chunk_map.values():
                c.hybrid_score = c.semantic_score
        out = list(chunk_map.values())
        out.sort(key=lambda c: c.hybrid_score, reverse=True)
        return out

    def retrieve_candidates(self, query: str, n_candidates: int = 100, where_filter=None) -> List[RetrievedChunk]:
        """reference src/rag/retriever.py:312-470: BM25 for every sub-query, weights 1.5 x / 0.75 x, bm25_score keeps the max"""
        n_fetch = max(n_candidates, 50)
        expanded, queries = self._expand(query)
        doc_filter = self._doc_filter(expanded)
        per_query = self._dense(queries, n_fetch, where_filter)
        bm25 = None
        if self._hybrid():
            live = [i for i, c in enumerate(per_query) if c is not None]
            found = self.chunk_bm25.search_batch([queries[i] for i in live], top_k=n_fetch, doc_filter=doc_filter) if live else []
            bm25 = [None] * len(queries)
            for i, res in zip(live, found):
                bm25[i] = (res, 2.0 * 1.5 if i == 0 else 1.0 * 0.75)
        return self._fuse(per_query, bm25=bm25, doc_filter=doc_filter, min_semantic=10, bm25_keep_max=True)[:n_candidates]

    def retrieve_candidates_batch(self, queries: Sequence[str], n_candidates: int = 100, where_filter=None) -> List[List[RetrievedChunk]]:
        """retrieve_candidates of every question — the same ids, order and floats — with the sub-queries of the whole batch encoded,
        searched and BM25-scored together and their rankings fused on the GPU by one launch (rag_dpo_amd/fusion.py).
        where_filter: one filter for every question, or a list / tuple with one filter (or None) per question.
        fusion="host" loops retrieve_candidates; "device" needs librdx and a GPU collection and refuses a question beyond the kernel's
        limits; "auto" takes the device where it can and the loop for the rest. If the batched device calls raise (a sub-query the
        index rejects), every question goes through retrieve_candidates, which skips exactly the failing sub-queries."""
        queries = list(queries)
        wheres = list(where_filter) if isinstance(where_filter, (list, tuple)) else [where_filter] * len(queries)
        if len(wheres) != len(queries):
            raise ValueError(f"where_filter: {len(wheres)} filters for {len(queries)} questions")
        loop = lambda idx: [self.retrieve_candidates(queries[i], n_candidates=n_candidates, where_filter=wheres[i]) for i in idx]
        if self.fusion == "host" or not queries:
            return loop(range(len(queries)))
        from . import fusion as F
        if self.fusion == "device":
            from . import _lib
            _lib.load(require_gpu=True)                             # raises RdxUnavailable: there is no quiet fall-back
            if not F.device_ready(self):
                raise RuntimeError("fusion='device' needs a collection on a GPU engine (query_device)")
        elif not F.device_ready(self):
            return loop(range(len(queries)))
        per_sub = 2 if self._hybrid() else 1
        n_fetch = max(n_candidates, 50)
        expanded = [self._expand(q) for q in queries]                # (expanded once: the expander may be a model)
        on_device = [i for i, (_, subs) in enumerate(expanded) if F.fits(per_sub * len(subs), n_fetch, n_candidates)]
        if self.fusion == "device" and len(on_device) < len(queries):
            raise ValueError("fusion='device': a question's rankings are beyond rdx_fuse_rankings' limits "
                             f"({F.MAX_LISTS} lists, {F.MAX_ENTRIES} entries per question)")
        out: List[Optional[List[RetrievedChunk]]] = [None] * len(queries)
        if on_device:
            try:
                got = F.retrieve_candidates_device(self, [expanded[i] for i in on_device], n_candidates, [wheres[i] for i in on_device])
            except Exception as e:
                logger.error("the batched device retrieval failed (%s): retrieving the %d questions one by one", e, len(on_device))
                got = loop(on_device)
            for i, g in zip(on_device, got):
                out[i] = g
        rest = [i for i in range(len(queries)) if out[i] is None]
        for i, g in zip(rest, loop(rest)):
            out[i] = g
        return out

    def retrieve_reranked(self, query: str, reranker, n_candidates: int = 40, top_k: int = 10, where_filter=None, topic_matcher=None,
                          question_topics: Optional[List[str]] = None) -> List[RetrievedDocument]:
        """Phases 1 and 1.5 of the reference's RAGPipeline.query with a reranker (src/rag/pipeline.py:221-262): retrieve_candidates,
        the cross-encoder rerank (rag_dpo_amd.reranker.CrossEncoderReranker, or any object with its rerank()), and the documents
        rebuilt from the reranked chunks. No candidates -> [] (the reference answers "nothing found" there)."""
        candidates = self.retrieve_candidates(query, n_candidates=n_candidates, where_filter=where_filter)
        if not candidates:
            return []
        ranked = reranker.rerank(query=query, chunks=candidates, top_k=top_k, topic_matcher=topic_matcher, question_topics=question_topics)
        return documents_from_ranked_chunks(ranked)

    def retrieve_reranked_batch(self, queries: Sequence[str], reranker, n_candidates: int = 40, top_k: int = 10, where_filter=None,
                                topic_matcher=None, question_topics=None) -> List[List[RetrievedDocument]]:
        """retrieve_reranked of every question: retrieve_candidates_batch, then the reranker's rerank_batch (a reranker without one is
        called question by question), then the documents rebuilt per question on the host (at most top_k winners each). A question
        without candidates gives []. question_topics: None, or one list (or None) per question. With a reranker whose scores do not
        depend on how pairs are grouped this equals [retrieve_reranked(...)] exactly; a real backbone's scores agree up to its
        tolerance (rag_dpo_amd/reranker.py)."""
        queries = list(queries)
        topics = [None] * len(queries) if question_topics is None else list(question_topics)
        if len(topics) != len(queries):
            raise ValueError(f"question_topics has {len(topics)} entries for {len(queries)} questions")
        candidates = self.retrieve_candidates_batch(queries, n_candidates=n_candidates, where_filter=where_filter)
        live = [i for i, c in enumerate(candidates) if c]
        out: List[List[RetrievedDocument]] = [[] for _ in queries]
        if not live:
            return out
        if hasattr(reranker, "rerank_batch"):
            ranked = reranker.rerank_batch([queries[i] for i in live], [candidates[i] for i in live], top_k=top_k, topic_matcher=topic_matcher,
                                           question_topics=[topics[i] for i in live])
        else:
            ranked = [reranker.rerank(query=queries[i], chunks=candidates[i], top_k=top_k, topic_matcher=topic_matcher,
                                      question_topics=topics[i]) for i in live]
        for i, r in zip(live, ranked):
            out[i] = documents_from_ranked_chunks(r)
        return out

    def retrieve(self, query: str, where_filter=None, n_documents: Optional[int] = None,
                 n_chunks_per_doc: Optional[int] = None) -> List[RetrievedDocument]:
        """reference src/rag/retriever.py:156-310: BM25 for the main query only, weight 2.0"""
        n_docs = n_documents or self.n_documents
        n_chunks = n_chunks_per_doc or self.n_chunks_per_doc
        n_fetch = n_docs * self.fetch_multiplier
        expanded, queries = self._expand(query)
        doc_filter = self._doc_filter(expanded)
        per_query = self._dense(queries, n_fetch, where_filter)
        bm25 = None
        if self._hybrid() and per_query and per_query[0] is not None:
            bm25 = [None] * len(queries)
            bm25[0] = (self.chunk_bm25.search(queries[0], top_k=n_fetch, doc_filter=doc_filter), 2.0)
        return deduplicate_by_document(self._fuse(per_query, bm25=bm25, doc_filter=doc_filter, min_semantic=5), n_docs, n_chunks)


def deduplicate_by_document(chunks: List[RetrievedChunk], n_documents: int, n_chunks_per_doc: int) -> List[RetrievedDocument]:
    """reference src/rag/retriever.py:539-578"""
    doc_chunks: Dict[str, List[RetrievedChunk]] = defaultdict(list)
    for c in chunks:
        doc_chunks[c.document_path].append(c)
    documents, seen_urls = [], set()
    for doc_path, lst in doc_chunks.items():
        ordered = sorted(lst, key=lambda c: c.hybrid_score if c.hybrid_score > 0 else c.similarity_score, reverse=True)
        selected = ordered[:n_chunks_per_doc]
        url = selected[0].metadata.get("source_url", "") if selected else ""
        if url:
            norm = url.lower().replace("https://", "").replace("http://", "").replace("www.", "")
            if norm in seen_urls:
                continue
            seen_urls.add(norm)
        documents.append(RetrievedDocument(document_path=doc_path, chunks=selected))
    documents.sort(key=lambda d: d.avg_similarity, reverse=True)
    return documents[:n_documents]


def documents_from_ranked_chunks(ranked_chunks, n_chunks_per_doc: Optional[int] = None) -> List[RetrievedDocument]:
    """reference src/rag/pipeline.py:805-878 (RAGPipeline._rebuild_documents_from_ranked_chunks): the reranked chunks grouped by
    document, documents by their best rerank score, chunks by score inside a document, every chunk kept (n_chunks_per_doc is
    ignored, as there). The agent graph's copy (src/rag/agent/nodes.py:1208-1252) computes the same without that argument.
    distance = 1 - rerank_score and hybrid_score = rerank_score; RetrievedDocument recomputes avg_similarity and primary_nature
    from the chunks, in both codebases."""
    doc_chunks: Dict[str, list] = defaultdict(list)
    doc_best: Dict[str, float] = {}
    for rc in ranked_chunks:
        doc_chunks[rc.document_path].append(rc)
        if rc.document_path not in doc_best or rc.rerank_score > doc_best[rc.document_path]:
            doc_best[rc.document_path] = rc.rerank_score
    documents = []
    for path in sorted(doc_best, key=lambda p: doc_best[p], reverse=True):
        lst = sorted(doc_chunks[path], key=lambda x: x.rerank_score, reverse=True)
        chunks = [RetrievedChunk(chunk_id=rc.chunk_id, text=rc.text, document_path=rc.document_path,
                                 chunk_nature=rc.metadata.get("chunk_nature", "UNKNOWN"), chunk_index=rc.metadata.get("chunk_index", 0),
                                 confidence=rc.metadata.get("confidence", "medium"), distance=1.0 - rc.rerank_score,
                                 metadata=rc.metadata, hybrid_score=rc.rerank_score) for rc in lst]
        natures = [rc.metadata.get("chunk_nature", "UNKNOWN") for rc in lst]
        documents.append(RetrievedDocument(document_path=path, chunks=chunks, avg_similarity=doc_best[path],
                                           primary_nature=max(set(natures), key=natures.count) if natures else "UNKNOWN"))
    return documents


def build_enterprise_where_filter(base_filter: Optional[Dict] = None, enterprise_tags: Optional[List[str]] = None) -> Optional[Dict]:
    """the `where` the pipeline sends down to collection.query — reference src/rag/pipeline.py:35-71:
    no tags -> base filter unchanged; tags -> $or[source != ENTREPRISE, tag_X = True, ...] AND-ed with the base."""
    if not enterprise_tags:
        return base_filter
    source_filter = {"$or": [{"source": {"$ne": "ENTREPRISE"}}] + [{f"tag_{t}": True} for t in enterprise_tags]}
    if base_filter:
        return {"$and": [base_filter, source_filter]}
    return source_filter
