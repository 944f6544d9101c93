#!/usr/bin/env python3
"""Captures tests/golden/reranker_golden.json by running the reference's OWN CrossEncoderReranker.rerank
(src/rag/reranker.py, imported from a reference checkout, never copied) with a fake `_model` that records the pairs and batch size
it is handed and returns scripted float32 scores (tests/golden/reranker_world.py), the reference's TopicMatcher
(src/utils/rgpd_topics.py) over a fake embedding provider, and RAGPipeline._rebuild_documents_from_ranked_chunks
(src/rag/pipeline.py:805-878) on every result. `rank_bm25` is not installed: it is stubbed with tests/bm25_oracle.py as in
make_bm25_golden.py. The JSON it writes is the committed fixture; the reference is needed only to regenerate it.

    python tests/golden/make_reranker_golden.py <reference checkout>
"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import bm25_oracle  # noqa: E402
import reranker_world as W  # noqa: E402


class FakeModel:
    """stands where sentence-transformers' CrossEncoder stands (predict(pairs, batch_size, show_progress_bar) -> float32 numpy)"""

    def __init__(self, scores, raises=False):
        self.scores, self.raises, self.calls = scores, raises, []

    def predict(self, pairs, batch_size=32, show_progress_bar=True):
        self.calls.append({"pairs": [list(p) for p in pairs], "batch_size": batch_size, "show_progress_bar": show_progress_bar})
        if self.raises:
            raise RuntimeError("scripted model failure")
        return np.asarray(self.scores, dtype=np.float32)


class FakeProvider:
    def __init__(self, vec):
        self.vec = vec

    def embed(self, texts):
        return [list(self.vec[t]) for t in texts]


class RecordingMatcher:
    """the reference's TopicMatcher, every topic_boost call and its result recorded"""

    def __init__(self, tm):
        self.tm, self.calls = tm, []

    def topic_boost(self, question_topics, chunk_tags_str):
        b = self.tm.topic_boost(question_topics, chunk_tags_str)
        self.calls.append([list(question_topics), chunk_tags_str, repr(float(b))])
        return b


def main(reference):
    stub = types.ModuleType("rank_bm25")
    stub.BM25Okapi = bm25_oracle.BM25Okapi
    sys.modules["rank_bm25"] = stub
    sys.path.insert(0, reference)
    from src.rag.pipeline import RAGPipeline          # the reference
    from src.rag.reranker import CrossEncoderReranker
    from src.rag.retriever import RetrievedChunk
    from src.utils.rgpd_topics import TopicMatcher

    pool = W.pool()
    tm = TopicMatcher(embedding_provider=FakeProvider(W.topic_vectors()))
    out = {"generator": "tests/golden/make_reranker_golden.py: the reference's CrossEncoderReranker.rerank with a scripted model, "
                        "its TopicMatcher and RAGPipeline._rebuild_documents_from_ranked_chunks",
           "query": W.QUERY, "defaults": {}, "cases": []}
    r0 = CrossEncoderReranker()
    out["defaults"] = {k: getattr(r0, k) for k in ("model_name", "device", "batch_size", "max_length", "trust_remote_code", "min_score")}
    for case in W.cases():
        chunks = [RetrievedChunk(chunk_id=pool[i]["chunk_id"], text=pool[i]["text"], document_path=pool[i]["document_path"],
                                 chunk_nature=pool[i]["metadata"]["chunk_nature"], chunk_index=pool[i]["metadata"]["chunk_index"],
                                 confidence=pool[i]["metadata"].get("confidence", "unknown"), distance=pool[i]["distance"],
                                 metadata=pool[i]["metadata"]) for i in case["idx"]]
        rr = CrossEncoderReranker(min_score=case["min_score"])
        rr._model = FakeModel(case["scores"], raises=case["raises"])
        rr._is_loaded = True
        matcher = RecordingMatcher(tm) if case["topics"] is not None else None
        rec = {"name": case["name"]}
        try:
            ranked = rr.rerank(W.QUERY, chunks, top_k=case["top_k"], topic_matcher=matcher, question_topics=case["topics"])
        except Exception as e:  # noqa: BLE001
            rec["raises"] = type(e).__name__
            ranked = None
        rec["model_calls"] = rr._model.calls
        rec["boosts"] = matcher.calls if matcher is not None else None
        if ranked is not None:
            rec["result"] = [{"chunk_id": r.chunk_id, "rerank_score": repr(float(r.rerank_score)), "original_rank": r.original_rank,
                              "document_path": r.document_path, "text_is_input": r.text == chunks[r.original_rank].text}
                             for r in ranked]
            docs = RAGPipeline._rebuild_documents_from_ranked_chunks(None, ranked, None)
            rec["documents"] = [{"document_path": d.document_path, "avg_similarity": repr(float(d.avg_similarity)),
                                 "primary_nature": d.primary_nature,
                                 "chunks": [[c.chunk_id, repr(float(c.hybrid_score)), repr(float(c.distance)), c.chunk_nature,
                                             c.chunk_index, c.confidence] for c in d.chunks]} for d in docs]
        out["cases"].append(rec)
    with open(os.path.join(HERE, "reranker_golden.json"), "w") as f:
        json.dump(out, f, indent=1, ensure_ascii=False)
    print(f"{len(out['cases'])} cases; raised: {[c['name'] for c in out['cases'] if 'raises' in c]}")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(os.path.abspath(sys.argv[1]))
