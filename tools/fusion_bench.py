"""Hybrid retrieval for batches of questions: the per-question loop against DenseRetriever.retrieve_candidates_batch (rag_dpo_amd/fusion.py,
csrc/fuse_kernel.hpp) on the reference's shape — 16,919 chunks of 1,024 dimensions, 4 sub-queries per question (a scripted expander),
n_fetch 50, 40 candidates kept, both BM25 indexes (the summary pre-filter over 2,000 documents and the chunk index).

  loop    [r.retrieve_candidates(q, 40) for q in questions]: retrieve_candidates is the code every question took before there was a batch
          path (this file never measures the new code against itself)
  batch   r.retrieve_candidates_batch(questions, 40) with fusion="device"

Both run in one process on one GPU, alternating, at 1, 48 and 1,024 questions; the two results are compared in ids, order and every
float before anything is timed. Per size it also prints what the chunk-BM25 leg of ONE batch call is: the number of engine calls
(counted here, by wrapping the engine's search methods) and the wall time of its search_batch_arrays call or calls. The encoder's forward is not part of either side: the embedder serves vectors it holds on the GPU
through EmbeddingProvider's two doors — embed() = rdx_l2_normalize, device-to-host copy and the float lists, embed_device() = the raw
rows, left on the device.

    python tools/fusion_bench.py [--out profiles/fusion/ab.txt] [--sizes 1,48,1024] [--min-reps 9] [--label new] [--breakdown]
"""
import argparse
import ctypes
import gc
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bm25_synth as S  # noqa: E402
from rag_dpo_amd import _lib as L  # noqa: E402
from rag_dpo_amd import bm25, synth  # noqa: E402
from rag_dpo_amd.collection import Collection  # noqa: E402
from rag_dpo_amd.retriever import DenseRetriever  # noqa: E402

N, DIM, DOCS, VOCAB = 16919, 1024, 2000, 40000


class TableEmbedder:
    """vectors held on the GPU, one per known text (the encoder's forward is outside this measurement)"""
    model_name = "table"

    def __init__(self, texts, corpus):
        rng = np.random.default_rng(3)
        self.row = {t: i for i, t in enumerate(texts)}
        near = corpus[rng.integers(0, corpus.shape[0], len(texts))]
        raw = 3.0 * (near + 0.8 * rng.standard_normal((len(texts), DIM)).astype(np.float32) / np.sqrt(DIM) * 4)
        self.table = torch.from_numpy(raw.astype(np.float32)).to("cuda:0")
        self.lib = L.load()

    def embed_device(self, texts):
        return self.table.index_select(0, torch.tensor([self.row[t] for t in texts], device="cuda:0"))

    def embed(self, texts):
        raw = self.embed_device(texts)
        out = torch.empty_like(raw)
        L.check(self.lib.rdx_l2_normalize(0, ctypes.c_void_p(raw.data_ptr()), raw.shape[0], raw.shape[1], ctypes.c_void_p(out.data_ptr()),
                                          L.RDX_DEVICE, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return out.cpu().numpy().tolist()


def expander(q):
    return [q, q + " obligations employeur", "sanction " + q, q + " durée conservation"]


def world(n_questions):
    rows, terms = S.tokens(N, VOCAB, 120, seed=1)
    words = np.char.add("mot", np.arange(VOCAB).astype(str))
    texts = [" ".join(x) for x in np.split(words[terms], np.cumsum(np.bincount(rows))[:-1])]
    corpus = synth.make_corpus(N, DIM)
    col = Collection("chunks", metadata={"hnsw:space": "cosine"})
    nat = ["GUIDE", "DOCTRINE", "SANCTION", "TECHNIQUE"]
    for a in range(0, N, 4096):
        b = min(N, a + 4096)
        col.add(ids=[f"chunk_{i:05d}" for i in range(a, b)], embeddings=corpus[a:b], documents=texts[a:b],
                metadatas=[{"document_path": f"cnil/doc_{i % DOCS:04d}.html", "chunk_nature": nat[i % 4], "chunk_index": i % 9,
                            "confidence": "high" if i % 3 else "medium", "source": "CNIL", "source_url": f"https://cnil.fr/p{i % DOCS}",
                            "title": f"Titre {i % DOCS}", "section": f"s{i % 17}"} for i in range(a, b)])
    chunk = bm25.ChunkBM25Index()
    chunk.build_from_collection(col)
    summaries = {f"cnil/doc_{d:04d}.html": {"document_title": f"Fiche {d}", "source_url": f"https://cnil.fr/p{d}",
                                             "summary": " ".join(words[S.query(VOCAB, 40, 1000 + d)])} for d in range(DOCS)}
    tmp = tempfile.mkdtemp(prefix="fusion_bench_")
    path = os.path.join(tmp, "document_summaries.json")
    with open(path, "w", encoding="utf-8") as f:
        json.dump(summaries, f)
    summ = bm25.SummaryBM25Index(summaries_path=path)
    summ.build()
    questions = [" ".join(words[S.query(VOCAB, 9, 50_000 + i)]) + f" quelle est la durée {i}" for i in range(n_questions)]
    emb = TableEmbedder([s for q in questions for s in expander(q)], corpus)
    return col, chunk, summ, emb, questions


class Bm25Leg:
    """counts the chunk index's engine calls and times its search_batch_arrays calls, from outside the library"""

    def __init__(self, chunk):
        self.calls, self.ms = 0, 0.0
        for name in ("search", "search_filtered"):
            if hasattr(chunk.engine, name):
                setattr(chunk.engine, name, self._counted(getattr(chunk.engine, name)))
        real = chunk.search_batch_arrays

        def timed(*a, **kw):
            t = time.perf_counter()
            try:
                return real(*a, **kw)
            finally:
                self.ms += (time.perf_counter() - t) * 1e3
        chunk.search_batch_arrays = timed

    def _counted(self, real):
        def f(*a, **kw):
            self.calls += 1
            return real(*a, **kw)
        return f

    def reset(self):
        self.calls, self.ms = 0, 0.0


STAGES = (("r", "_doc_filters", "summary filters"), ("F", "_embed_device", "embed"), ("col", "query_device", "dense search"),
          ("chunk", "search_batch_arrays", "chunk BM25"), ("F", "call_kernel", "fuse launch"), ("F", "unpack", "unpack winners"),
          ("col", "payload_of", "payload_of"))


def breakdown(r, col, chunk, qs):
    """one batch call with the device synchronised before and after every stage -> ({stage: ms}, total ms); what the stages leave
    is the packing of the lists and the host objects of the winners"""
    from rag_dpo_amd import fusion as F
    where = {"r": r, "F": F, "col": col, "chunk": chunk}
    spans, saved = {}, []

    def staged(real, label):
        def f(*a, **kw):
            torch.cuda.synchronize()
            t = time.perf_counter()
            try:
                return real(*a, **kw)
            finally:
                torch.cuda.synchronize()
                spans[label] = spans.get(label, 0.0) + (time.perf_counter() - t) * 1e3
        return f
    for owner, name, label in STAGES:
        real = getattr(where[owner], name)
        saved.append((where[owner], name, real))
        setattr(where[owner], name, staged(real, label))
    try:
        t = time.perf_counter()
        r.retrieve_candidates_batch(qs, n_candidates=40)
        torch.cuda.synchronize()
        total = (time.perf_counter() - t) * 1e3
    finally:
        for obj, name, real in saved:
            setattr(obj, name, real)
    return spans, total


def values(c):
    return (c.chunk_id, c.text, c.document_path, np.float32(c.distance).tobytes(), np.float64(c.bm25_score).tobytes(),
            np.float64(c.semantic_score).tobytes(), np.float64(c.hybrid_score).tobytes(), json.dumps(c.metadata, sort_keys=True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fusion", "ab.txt"))
    ap.add_argument("--sizes", default="1,48,1024")
    ap.add_argument("--min-reps", type=int, default=3, help="repetitions per size at the least (the default gives 1,024 questions 3)")
    ap.add_argument("--breakdown", action="store_true", help="after each size, one more batch call timed stage by stage")
    ap.add_argument("--label", default="", help="printed in front of every line (which library the run is of)")
    args = ap.parse_args()
    sizes = [int(s) for s in args.sizes.split(",")]
    t0 = time.perf_counter()
    col, chunk, summ, emb, questions = world(max(sizes))
    leg = Bm25Leg(chunk)
    r = DenseRetriever(col, emb, query_expander=expander, summary_bm25_index=summ, chunk_bm25_index=chunk, fusion="device")
    lines = [f"fusion_bench: {N} chunks x {DIM}, 4 sub-queries, n_fetch 50, 40 candidates, summary pre-filter over {DOCS} documents + chunk BM25; "
             f"{torch.cuda.get_device_name(0)}; world built in {time.perf_counter() - t0:.1f} s",
             "loop = [retrieve_candidates(q) for q in questions]; batch = retrieve_candidates_batch(questions), fusion='device'; alternating, "
             "wall ms per call incl. Python, median (min .. max) over the repetitions; the encoder's forward is in neither side; "
             "bm25 = the chunk-BM25 leg of one batch call: engine calls, and the wall ms of its search_batch_arrays call(s)"]
    loop = lambda qs: [r.retrieve_candidates(q, n_candidates=40) for q in qs]      # noqa: E731
    batch = lambda qs: r.retrieve_candidates_batch(qs, n_candidates=40)          # noqa: E731
    for nq in sizes:
        qs = questions[:nq]
        a, b = loop(qs), batch(qs)                                               # warm-up, and the check
        same = [[values(c) for c in g] for g in a] == [[values(c) for c in g] for g in b]
        filtered = sum(1 for q in qs if r._doc_filter(q))
        reps = max(args.min_reps, min(40, 400 // nq))
        ta, tb, tl, calls = [], [], [], set()
        for _ in range(reps):
            gc.collect()                                                         # a call pays for its own garbage only
            t = time.perf_counter()
            loop(qs)
            ta.append((time.perf_counter() - t) * 1e3)
            leg.reset()
            gc.collect()
            t = time.perf_counter()
            batch(qs)
            torch.cuda.synchronize()
            tb.append((time.perf_counter() - t) * 1e3)
            tl.append(leg.ms)
            calls.add(leg.calls)
        ma, mb, ml = float(np.median(ta)), float(np.median(tb)), float(np.median(tl))
        lines.append(f"nq {nq:5d}  reps {reps:3d}  identical {same}  summary-filtered {filtered}/{nq}  candidates/question {np.mean([len(g) for g in b]):.1f}  "
                     f"loop {ma:10.2f} ms ({min(ta):.2f} .. {max(ta):.2f})  batch {mb:10.2f} ms ({min(tb):.2f} .. {max(tb):.2f})  "
                     f"per question {ma / nq:.3f} -> {mb / nq:.3f} ms  loop/batch {ma / mb:.2f}x  "
                     f"bm25 engine calls/batch {'/'.join(map(str, sorted(calls)))}  bm25 leg {ml:9.2f} ms ({min(tl):.2f} .. {max(tl):.2f})")
        print(lines[-1], flush=True)
        if args.breakdown:
            spans, total = breakdown(r, col, chunk, qs)
            rest = total - sum(spans.values())
            lines.append(f"nq {nq:5d}  one batch call, synchronised per stage: total {total:.2f} ms = "
                         + " + ".join(f"{label} {spans.get(label, 0.0):.2f}" for _, _, label in STAGES)
                         + f" + packing and the winners' host objects {rest:.2f}")
            print(lines[-1], flush=True)
    if args.label:
        lines = [f"[{args.label}] {l}" for l in lines]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[:2]))


if __name__ == "__main__":
    main()
