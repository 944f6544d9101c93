"""BM25 sparse retrieval on the MI355X (rag_dpo_amd/bm25.py, csrc/bm25_kernel.hpp): one JSON line per shape.

- the reference's shape: ChunkBM25Index over 16,919 chunks (Zipf words, mean 120 tokens), top_k 50: search() per call with
  Python included, one query and four (search_batch), device time from events around the call, and the index build time;
- synthetic 1 M and 10 M rows (Zipf vocabulary of 200 k terms, mean 120 tokens per row): the device call, posting bytes per
  query (row int32 + tf uint16, + the f64 denominator gathered per posting) and that traffic's share of 8 TB/s;
- the CPU restatement of rank_bm25 (tests/bm25_oracle.py, NOT rank_bm25 itself) on the same shapes.

    python tools/bm25_bench.py [--reps N] [--skip-10m]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bm25_oracle as O  # noqa: E402
import bm25_synth as S  # noqa: E402
from rag_dpo_amd import bm25  # noqa: E402


def per_call_ms(f, reps, warm=5):
    for _ in range(warm):
        f()
    t = time.perf_counter()
    for _ in range(reps):
        f()
    return round((time.perf_counter() - t) / reps * 1e3, 4)


def event_ms(f, reps):
    s, e, st = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True), torch.cuda.current_stream()
    out = []
    for _ in range(reps):
        s.record(st)
        f()
        e.record(st)
        e.synchronize()
        out.append(s.elapsed_time(e))
    return round(float(np.median(out)), 4)


class Pages:
    """count() / get(limit, offset, include): what ChunkBM25Index.build_from_collection reads from a collection"""

    def __init__(self, texts):
        self.texts = texts

    def count(self):
        return len(self.texts)

    def get(self, limit, offset, include):
        ids = range(offset, min(offset + limit, len(self.texts)))
        return {"ids": [f"chunk_{i}" for i in ids], "documents": [self.texts[i] for i in ids],
                "metadatas": [{"document_path": f"doc_{i % 2000}"} for i in ids]}


def reference_shape(reps):
    rows, terms = S.tokens(16919, 40000, 120, seed=1)
    words = np.char.add("mot", np.arange(40000).astype(str))
    texts = [" ".join(x) for x in np.split(words[terms], np.cumsum(np.bincount(rows))[:-1])]
    t = time.perf_counter()
    ix = bm25.ChunkBM25Index()
    ix.build_from_collection(Pages(texts))
    build_s = round(time.perf_counter() - t, 3)
    queries = [" ".join(words[S.query(40000, 9, i)]) + " quelle est la durée" for i in range(64)]
    n = iter(range(10 ** 9))
    one = lambda: ix.search(queries[next(n) % 64], top_k=50)   # noqa: E731
    four = lambda: ix.search_batch([queries[(next(n) + j) % 64] for j in range(4)], top_k=50)   # noqa: E731
    cpu, ids = O.CpuBm25(ix.model.arrays()), ix.model.query_ids(bm25.tokenize_french(queries[0]))
    okapi = O.BM25Okapi(ix.corpus_tokens)
    print(json.dumps({"shape": "reference: 16919 chunks, top_k 50", "build_s": build_s, "search_1q_ms": per_call_ms(one, reps),
                      "search_batch_4q_ms": per_call_ms(four, reps), "device_events_1q_ms": event_ms(one, reps),
                      "device_events_4q_ms": event_ms(four, reps),
                      "host_tokenise_ms": per_call_ms(lambda: ix.model.query_ids(bm25.tokenize_french(queries[0])), reps),
                      "cpu_restatement_postings_1q_ms": per_call_ms(lambda: cpu.search([0, len(ids)], ids, 50), 20, 2),
                      "cpu_restatement_get_scores_1q_ms": per_call_ms(lambda: okapi.get_scores(bm25.tokenize_french(queries[0])), 3, 1),
                      "postings": int(ix.model.post_off[-1])}), flush=True)


def synthetic(n_rows, reps):
    t = time.perf_counter()
    a = S.make_by_term(n_rows, 200_000, 120, seed=n_rows)
    gen_s = round(time.perf_counter() - t, 2)
    t = time.perf_counter()
    eng = bm25.HipBm25(a, 0)
    create_s = round(time.perf_counter() - t, 3)
    qs = [S.query(200_000, 9, 100 + i) for i in range(16)]
    n = iter(range(10 ** 9))

    def run(nq):
        sel = [qs[(next(n) + i) % 16] for i in range(nq)]
        return eng.search(np.cumsum([0] + [len(q) for q in sel]), np.concatenate(sel), 50)
    ev1 = event_ms(lambda: run(1), reps)
    post = float(np.mean([np.diff(a.post_off)[q].sum() for q in qs]))
    cpu = O.CpuBm25(a)
    print(json.dumps({"shape": f"synthetic {n_rows} rows, 200k-term Zipf vocabulary, mean 120 tokens, top_k 50", "generate_s": gen_s,
                      "create_s": create_s, "postings": int(a.post_off[-1]), "search_1q_ms": per_call_ms(lambda: run(1), reps),
                      "device_events_1q_ms": ev1, "search_4q_ms": per_call_ms(lambda: run(4), reps),
                      "device_events_4q_ms": event_ms(lambda: run(4), reps), "postings_per_query": int(post),
                      "bytes_per_query": int(post * 14), "hbm_share_1q": round(post * 14 / (ev1 * 1e-3) / 8e12, 4),
                      "cpu_restatement_postings_1q_ms": per_call_ms(lambda: cpu.search([0, len(qs[0])], qs[0], 50), 3, 1)}), flush=True)
    eng.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--skip-10m", action="store_true")
    args = ap.parse_args()
    reference_shape(args.reps)
    for n_rows in (1_000_000,) if args.skip_10m else (1_000_000, 10_000_000):
        synthetic(n_rows, args.reps)
