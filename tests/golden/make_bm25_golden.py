#!/usr/bin/env python3
"""Captures tests/golden/bm25_golden.json by driving the reference's
OWN bm25_index.py and RAGRetriever (/root/reference/src/rag/, imported here, never copied) over this repo's Chroma-shaped
Collection with the CPU oracle engine. `rank_bm25` is not installed: sys.modules["rank_bm25"] is set to the restatement of
BM25Okapi in tests/bm25_oracle.py, so the reference's classes score with rank_bm25 0.2.2's formulas. Runs only in the build
container (the reference does not travel to the GPU box); the JSON it writes is the committed fixture.

    python tests/golden/make_bm25_golden.py
"""
import json
import os
import sys
import tempfile
import types
import zlib
from pathlib import Path

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import bm25_oracle  # noqa: E402

stub = types.ModuleType("rank_bm25")
stub.BM25Okapi = bm25_oracle.BM25Okapi
sys.modules["rank_bm25"] = stub
sys.path.insert(0, "/root/reference")
from src.rag import bm25_index as REF  # noqa: E402  (the reference)
from src.rag.retriever import RAGRetriever  # noqa: E402
from src.utils.acronyms import expand_query_with_acronyms  # noqa: E402

import bm25_world as W  # noqa: E402
from oracle_engine import factory  # noqa: E402


class Expander:
    def expand(self, q):
        return W.expander(q)


def chunk_dict(c):
    return {"chunk_id": c.chunk_id, "distance": c.distance, "semantic_score": c.semantic_score, "hybrid_score": c.hybrid_score,
            "bm25_score": repr(float(c.bm25_score)), "document_path": c.document_path, "chunk_nature": c.chunk_nature,
            "chunk_index": c.chunk_index, "confidence": c.confidence, "text_crc32": zlib.crc32(c.text.encode("utf-8"))}


def doc_dict(d):
    # primary_nature is max(set(natures), key=natures.count) in the reference: a count tie is decided by string-hash order
    # (PYTHONHASHSEED), so only its count is recorded
    nat = [c.chunk_nature for c in d.chunks]
    return {"document_path": d.document_path, "avg_similarity": d.avg_similarity, "primary_nature_count": nat.count(d.primary_nature),
            "chunks": [[c.chunk_id, c.hybrid_score, c.distance, repr(float(c.bm25_score))] for c in d.chunks]}


def results(rs):
    return [[r.doc_key, repr(float(r.score))] for r in rs]


def main():
    out = {"generator": "tests/golden/make_bm25_golden.py driving /root/reference/src/rag/bm25_index.py and retriever.py",
           "stopwords": sorted(REF.FRENCH_STOPWORDS),
           "tokenizer": [[t, REF.tokenize_french(t)] for t in W.TOKENIZER_TEXTS + [" ".join(sorted(REF.FRENCH_STOPWORDS))]]}

    chunk = REF.ChunkBM25Index()
    chunk.build_from_collection(W.build_collection(factory), batch_size=700)
    bm = chunk.index
    out["chunk_index"] = {"rows": len(chunk.chunk_ids), "first_ids": chunk.chunk_ids[:5], "avgdl": repr(bm.avgdl),
                          "average_idf": repr(bm.average_idf), "vocabulary_head": list(bm.idf)[:40], "vocabulary_size": len(bm.idf)}
    out["chunk_search"] = []
    for query, top_k, flt in W.CHUNK_CASES:
        doc_filter = None if flt is None else (set() if flt == "empty" else set(flt))
        out["chunk_search"].append({"query": query, "top_k": top_k, "doc_filter": flt,
                                    "results": results(chunk.search(query, top_k=top_k, doc_filter=doc_filter))})
    r0 = chunk.search(W.CHUNK_CASES[0][0], top_k=3)
    out["chunk_result_metadata"] = [r.metadata for r in r0]

    summ = REF.SummaryBM25Index(summaries_path=Path(W.write_summaries(tempfile.mkdtemp())))
    summ.build()
    out["summary_index"] = {"doc_keys": summ.doc_keys, "avgdl": repr(summ.index.avgdl)}
    out["summary_search"] = [{"query": q, "top_k": k, "results": results(summ.search(q, top_k=k)),
                              "doc_paths": sorted(summ.get_relevant_doc_paths(q, top_k=k))} for q, k in W.SUMMARY_QUERIES]
    out["summary_result_metadata"] = [r.metadata for r in summ.search(W.SUMMARY_QUERIES[0][0], top_k=2)]

    out["retriever"] = []
    for case in W.RETRIEVER_QUERIES:
        assert expand_query_with_acronyms(case["query"]) == case["query"]    # the retriever's own acronym step is the identity here
        r = RAGRetriever(collection=W.build_collection(factory), llm_provider=None, embedding_provider=W.HashEmbedder(case["poison_sub"]),
                         summary_bm25_index=summ, chunk_bm25_index=chunk, query_expander=Expander() if case["expand"] else None,
                         enable_summary_prefilter=case["prefilter"])
        cands = r.retrieve_candidates(case["query"], n_candidates=case["n_candidates"], where_filter=case["where"])
        docs = r.retrieve(case["query"], where_filter=case["where"])
        out["retriever"].append(dict(case, candidates=[chunk_dict(c) for c in cands], documents=[doc_dict(d) for d in docs]))
    with open(os.path.join(HERE, "bm25_golden.json"), "w", encoding="utf-8") as f:
        json.dump(out, f, ensure_ascii=False, sort_keys=True)
    print("wrote", len(out["chunk_search"]), "chunk cases,", len(out["retriever"]), "retriever cases")


if __name__ == "__main__":
    main()
