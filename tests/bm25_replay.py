"""Replays of tests/golden/bm25_golden.json (captured from the IMPORTED reference bm25_index.py / RAGRetriever by
tests/golden/make_bm25_golden.py) against this repo's BM25 indexes and hybrid DenseRetriever, for any pair of engines:
the CPU ones (test_bm25_host.py) or librdx (test_gpu_bm25.py). Nothing here reads the reference."""
import json
import os
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import bm25_world as W  # noqa: E402
from oracle_engine import factory as dense_cpu  # noqa: E402
from rag_dpo_amd.bm25 import ChunkBM25Index, SummaryBM25Index  # noqa: E402
from rag_dpo_amd.retriever import DenseRetriever  # noqa: E402

GOLD = json.load(open(os.path.join(HERE, "golden", "bm25_golden.json"), encoding="utf-8"))


def results(rs):
    return [[r.doc_key, repr(float(r.score))] for r in rs]


def doc_filter_of(flt):
    return None if flt is None else (set() if flt == "empty" else set(flt))


def chunk_index(bm25_factory):
    ix = ChunkBM25Index(engine_factory=bm25_factory)
    ix.build_from_collection(W.build_collection(dense_cpu), batch_size=700)
    return ix


def summary_index(bm25_factory, directory):
    ix = SummaryBM25Index(summaries_path=W.write_summaries(directory), engine_factory=bm25_factory)
    ix.build()
    return ix


def replay_chunk_search(ix):
    g = GOLD["chunk_index"]
    assert len(ix.chunk_ids) == g["rows"] and ix.chunk_ids[:5] == g["first_ids"]
    for case in GOLD["chunk_search"]:
        got = results(ix.search(case["query"], top_k=case["top_k"], doc_filter=doc_filter_of(case["doc_filter"])))
        assert got == case["results"], case["query"]
    assert [r.metadata for r in ix.search(W.CHUNK_CASES[0][0], top_k=3)] == GOLD["chunk_result_metadata"]


def replay_summary(ix):
    assert ix.doc_keys == GOLD["summary_index"]["doc_keys"]
    assert repr(ix.model.avgdl) == GOLD["summary_index"]["avgdl"]
    for case in GOLD["summary_search"]:
        assert results(ix.search(case["query"], top_k=case["top_k"])) == case["results"], case["query"]
        assert sorted(ix.get_relevant_doc_paths(case["query"], top_k=case["top_k"])) == case["doc_paths"]
    assert [r.metadata for r in ix.search(W.SUMMARY_QUERIES[0][0], top_k=2)] == GOLD["summary_result_metadata"]


def _same_chunk(c, g):
    assert c.chunk_id == g["chunk_id"], (c.chunk_id, g["chunk_id"])
    assert zlib.crc32(c.text.encode("utf-8")) == g["text_crc32"] and c.document_path == g["document_path"]
    assert c.chunk_nature == g["chunk_nature"] and c.chunk_index == g["chunk_index"] and c.confidence == g["confidence"]
    assert c.distance == g["distance"] and c.semantic_score == g["semantic_score"] and c.hybrid_score == g["hybrid_score"]
    assert repr(float(c.bm25_score)) == g["bm25_score"]


def replay_retriever(dense_factory, summ, chunk):
    """ids, order and every float of the reference's retrieve_candidates / retrieve, with both indexes; the dense sub-queries
    in one batched collection.query and, in retrieve_candidates, the BM25 searches of all sub-queries in one search_batch"""
    for case in GOLD["retriever"]:
        col = W.build_collection(dense_factory)
        emb = W.HashEmbedder(case["poison_sub"])
        batches = []
        real = chunk.search_batch

        def spy(queries, *a, **kw):
            batches.append(len(queries))
            return real(queries, *a, **kw)
        chunk.search_batch = spy
        try:
            r = DenseRetriever(col, emb, query_expander=W.expander if case["expand"] else None, summary_bm25_index=summ,
                               chunk_bm25_index=chunk, enable_summary_prefilter=case["prefilter"])
            cands = r.retrieve_candidates(case["query"], n_candidates=case["n_candidates"], where_filter=case["where"])
            assert len(batches) == 1
            assert len(cands) == len(case["candidates"])
            for c, g in zip(cands, case["candidates"]):
                _same_chunk(c, g)
            docs = r.retrieve(case["query"], where_filter=case["where"])
        finally:
            del chunk.search_batch
        assert [d.document_path for d in docs] == [g["document_path"] for g in case["documents"]]
        for d, g in zip(docs, case["documents"]):
            assert d.avg_similarity == g["avg_similarity"]
            nat = [c.chunk_nature for c in d.chunks]
            assert nat.count(d.primary_nature) == g["primary_nature_count"] == max(nat.count(x) for x in nat)
            assert [[c.chunk_id, c.hybrid_score, c.distance, repr(float(c.bm25_score))] for c in d.chunks] == g["chunks"]
