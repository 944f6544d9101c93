"""Grouped search against the plain search it is built on: Collection.query_groups_device(G = 5, m = 3) and
Collection.query_device(n_results = k1), alternated call by call in one process on one GPU, at the reference's size and at bench size.

    python tools/group_bench.py [--out profiles/groups] [--cases ref1,ref4,uniform,embed] [--k-first 64[,256]] [--calls 30] [--rows 1000000]

Cases (dim 1024; the key is an int column `doc`, a document = a run of consecutive rows):
    ref1, ref4  16 919 rows (the reference's store), 1 and 4 queries; synth's N(0,1) corpus; documents of 8 chunks
    uniform     --rows rows x 256 queries of synth's N(0,1) corpus (10 % of the queries planted next to a row); 2 000 documents
    embed       --rows rows x 256 queries of synth's embedding-like corpus: 2 000 documents of near-duplicate chunks, every query
                placed near one document — the corpus on which the top chunks crowd into one document
Per case and first-fetch k: milliseconds per batch of both calls (median and minimum over --calls alternated turns after 3 unmeasured
ones; host clock around the call and a device synchronise: the grouped call reads its flags back in any case), the share of queries
proven at the first fetch, sent to the second fetch and to brute force, and the fill jobs per query (Collection.group_stats). The
collection's host-side fields are filled directly (vectorised), as tools/where_bench.py does: a million rows through Collection.add are
minutes of Python this tool does not measure. -> ab.txt + ab.json under --out."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DIM, G, M = 1024, 5, 3


def make_collection(name: str, n: int, chunks, doc_len: int):
    """chunks: iterable of [rows][DIM] arrays / device tensors in row order"""
    from rag_dpo_amd import where as W
    from rag_dpo_amd.collection import Collection
    col = Collection(name)
    col._ensure_engine(DIM)
    for c in chunks:
        col._engine.add(c)
    col._ids = [f"c{i}" for i in range(n)]
    col._docs = [None] * n
    col._row_of = {s: i for i, s in enumerate(col._ids)}
    col._alive = np.ones(n, dtype=bool)
    doc = W.Column(0)
    doc.kind = np.full(n, W.K_INT, dtype=np.int8)
    doc.num = (np.arange(n) // doc_len).astype(np.float64)
    doc.code = np.full(n, -1, dtype=np.int32)
    col._cols = {"doc": doc}
    col._writes += 1
    # the fields above are Collection's own: if they move, say so here instead of measuring something else
    one = col.get(ids=[f"c{n - 1}"])
    assert col.count() == n == len(col._engine) and one["metadatas"][0]["doc"] == (n - 1) // doc_len
    return col


def build_case(case: str, rows: int):
    import torch
    from rag_dpo_amd import synth
    dev = torch.device("cuda", 0)
    if case in ("ref1", "ref4"):
        n = 16919
        emb = synth.make_corpus(n, DIM)
        q = torch.from_numpy(synth.make_queries(int(case[3:]), DIM, emb)).to(dev)
        return make_collection(case, n, [emb], 8), q
    n, per = rows, synth.CHUNK
    doc_len = max(1, -(-n // synth.EMBED_DOCS))
    if case == "uniform":
        gen = (synth.torch_corpus_chunk(j, min(per, n - j * per), DIM, dev) for j in range(-(-n // per)))
        q = synth.torch_queries(256, DIM, dev, n)
    else:
        gen = (synth.torch_embedlike_chunk(j, min(per, n - j * per), DIM, dev, n) for j in range(-(-n // per)))
        q = synth.torch_embedlike_queries(256, DIM, dev)[0]
    return make_collection(case, n, gen, doc_len), q.contiguous()


def measure(col, q, k_first: int, calls: int):
    import torch
    from rag_dpo_amd import groups as GR
    GR.first_fetch_k = lambda n_groups, group_size: k_first          # the ladder's first k (developer override: this tool only)
    ms = {"groups": [], "plain": []}
    before = None
    for turn in range(calls + 3):
        if turn == 3:
            before = col.group_stats
        for path in ("groups", "plain"):
            torch.cuda.synchronize()
            t = time.perf_counter()
            if path == "groups":
                out = col.query_groups_device(q, "doc", G, M)
            else:
                out = col.query_device(q, n_results=k_first)
            torch.cuda.synchronize()
            if turn >= 3:
                ms[path].append((time.perf_counter() - t) * 1e3)
            del out
    d = {k: v - before[k] for k, v in col.group_stats.items()}
    nq = max(1, d["queries"])
    rec = {"k_first": k_first, "calls": calls, "proven_first_fetch": d["proven_first_fetch"] / nq, "second_fetch": d["second_fetch"] / nq,
           "brute": d["brute"] / nq, "fill_jobs_per_query": d["fill_jobs"] / nq}
    for path in ms:
        rec[path + "_median_ms"], rec[path + "_min_ms"] = float(np.median(ms[path])), float(np.min(ms[path]))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "groups"))
    ap.add_argument("--cases", default="ref1,ref4,uniform,embed", type=lambda s: s.split(","))
    ap.add_argument("--k-first", default="64", type=lambda s: [int(x) for x in s.split(",")])
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--slow-calls", type=int, default=5, help="turns of a case whose grouped call takes more than 50 ms")
    ap.add_argument("--rows", type=int, default=1_000_000)
    a = ap.parse_args()
    out = []
    lines = [f"{'case':>8} {'rows':>8} {'nq':>4} {'k1':>4} | {'groups med':>10} {'groups min':>10} | {'plain med':>9} {'plain min':>9} | {'over':>7} | "
             f"{'first':>6} {'second':>6} {'brute':>6} {'fill/q':>6}   (ms per batch; shares of queries)"]
    for case in a.cases:
        t0 = time.perf_counter()
        col, q = build_case(case, a.rows)
        print(f"# {case}: {col.count()} rows built in {time.perf_counter() - t0:.1f} s", flush=True)
        for k1 in a.k_first:
            probe = measure(col, q, k1, 1)
            rec = measure(col, q, k1, a.slow_calls if probe["groups_median_ms"] > 50 else a.calls)
            rec.update(case=case, rows=col.count(), nq=int(q.shape[0]), over_ms=rec["groups_median_ms"] - rec["plain_median_ms"])
            out.append(rec)
            lines.append(f"{case:>8} {rec['rows']:>8} {rec['nq']:>4} {k1:>4} | {rec['groups_median_ms']:10.3f} {rec['groups_min_ms']:10.3f} | "
                         f"{rec['plain_median_ms']:9.3f} {rec['plain_min_ms']:9.3f} | {rec['over_ms']:+7.3f} | {rec['proven_first_fetch']:6.3f} "
                         f"{rec['second_fetch']:6.3f} {rec['brute']:6.3f} {rec['fill_jobs_per_query']:6.2f}")
            print(lines[-1], flush=True)
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, "ab.json"), "w") as fh:
                json.dump({"dim": DIM, "n_groups": G, "group_size": M, "cases": out}, fh, indent=1)
            with open(os.path.join(a.out, "ab.txt"), "w") as fh:
                fh.write("\n".join(lines) + "\n")
        col._drop_masks()
        col._engine.close()
        del col, q


if __name__ == "__main__":
    main()
