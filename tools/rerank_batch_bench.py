"""A/B of the rerank stage for batches of questions: the loop of CrossEncoderReranker.rerank (one question at a time: the code before
rerank_batch, the baseline) against CrossEncoderReranker.rerank_batch, alternating in one process.

Shapes: 1, 8 and 48 questions x 40 candidates; pair lengths as in tools/rerank_bench.py — every pair 128 tokens, and
tools/ingest_bench.py's log-normal chunk lengths cut at the 512-token pair limit; each with and without a warmed TopicMatcher on the
GPU and 3 topics per question. bge-reranker-v2-m3's architecture (XLM-R-large, one label), random-init fp16, hashing tokenizer; every
question has its own text and its own candidates.

Reported per row: wall ms per question of both sides (median, min and max over the alternations: the spread), the forward's GPU ms and
TF/s of both sides (2 x 303 M weights x tokens + 4 x hidden x length^2 per layer and pair for the attention, over the device events
around the packed forwards), head + select GPU us per question, and the share of questions whose kept ids agree.

    python tools/rerank_batch_bench.py [--reps 5] [--out profiles/rerank_batch/ab.txt]
"""
import argparse
import os
import statistics
import sys
import time
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from rag_dpo_amd.reranker import CrossEncoderReranker
from rag_dpo_amd.retriever import RetrievedChunk
from rag_dpo_amd.topics import TopicMatcher

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--questions", default="1,8,48")
ap.add_argument("--model", default="random-init:xlm-roberta-large")
ap.add_argument("--out", default=os.path.join("profiles", "rerank_batch", "ab.txt"))
args = ap.parse_args()

N_CAND, TOP_K = 40, 10
VOCAB = [a + b for a in "abcdefghijklmnopqrstuvwxyz" for b in "abcdefghijklmnopqrstuvwxyz"]
rng = np.random.default_rng(2026)
TAGS = [" ".join(rng.choice(VOCAB, 2)) for _ in range(60)]


class Embedder:
    """unit vectors around a common direction (cosines on both sides of the boost threshold), from the text's crc32"""
    device = "cuda:0"

    def embed(self, texts):
        base = np.random.default_rng(1).standard_normal(1024)
        out = []
        for t in texts:
            v = base / np.linalg.norm(base) + 0.75 * np.random.default_rng(zlib.crc32(t.encode())).standard_normal(1024) / 32.0
            out.append((v / np.linalg.norm(v)).astype(np.float32).tolist())
        return out


def question(lengths):
    query = " ".join(rng.choice(VOCAB, 12))                 # 12 pieces: a pair of L tokens has L - 16 text pieces
    chunks = [RetrievedChunk(chunk_id=f"c{i}", text=" ".join(rng.choice(VOCAB, max(1, int(L) - 16))), document_path=f"doc{i % 9}",
                             chunk_nature="GUIDE", chunk_index=i, confidence="high", distance=0.3,
                             metadata={"chunk_nature": "GUIDE", "rgpd_topics": ", ".join(rng.choice(TAGS, int(rng.integers(0, 4))))})
              for i, L in enumerate(lengths)]
    return query, chunks, [str(t) for t in rng.choice(TAGS, 3)]


def lengths_of(kind):
    if kind == "128":
        return [128] * N_CAND
    mix = np.clip(np.exp(rng.normal(5.5, 0.65, size=N_CAND)), 64, 1024).astype(np.int64)   # tools/ingest_bench.py's chunk lengths
    return list(np.minimum(mix + 14, 512))


r = CrossEncoderReranker(args.model, device="cuda", dtype=torch.float16, min_score=0.0)
r._load_model()
cfg = r._model.model.config
assert r._model.path == "fused", r._model.path
weights = sum(p.numel() for n, p in r._model.model.roberta.encoder.named_parameters() if n.endswith("weight") and p.dim() == 2)
tm = TopicMatcher(Embedder(), device="cuda:0")
tm.warm(TAGS)


def flops(toks):
    toks = np.asarray(toks, dtype=np.float64)
    return 2.0 * weights * toks.sum() + cfg.num_hidden_layers * 4.0 * cfg.hidden_size * float((toks ** 2).sum())


lines = [f"rerank_batch_bench: {args.model} fp16 ({weights / 1e6:.0f} M encoder weights), {N_CAND} candidates per question, top_k {TOP_K}; "
         f"{torch.cuda.get_device_name(0)}; loop = [rerank(q) for q in questions] (the code before rerank_batch), batch = rerank_batch(questions); "
         f"alternating in one process, {args.warmup} warm-up and {args.reps} timed alternations per row; wall ms include tokenising and the results on the host"]
print(lines[0], flush=True)
for nq in [int(x) for x in args.questions.split(",")]:
    for kind in ("128", "lognormal_cut512"):
        world = [question(lengths_of(kind)) for _ in range(nq)]
        queries, chunk_lists, topics = [w[0] for w in world], [w[1] for w in world], [w[2] for w in world]
        toks = [min(int(max(len(c.text.split()) + 16, 17)), 512) for cs in chunk_lists for c in cs]
        for boosted in (False, True):
            kw = dict(topic_matcher=tm) if boosted else {}

            def loop():
                out, fwd, hs = [], 0.0, 0.0
                for q, cs, t in zip(queries, chunk_lists, topics):
                    out.append(r.rerank(q, cs, top_k=TOP_K, question_topics=t if boosted else None, **kw))
                    fwd += r.last_rerank_stats["ms_forward"]
                    hs += r.last_rerank_stats["ms_head_select"]
                return out, fwd, hs, r.last_rerank_stats["tokens"]

            def batch():
                out = r.rerank_batch(queries, chunk_lists, top_k=TOP_K, question_topics=topics if boosted else None, **kw)
                st = r.last_rerank_stats
                return out, st["ms_forward"], st["ms_head_select"], st["tokens"]

            for _ in range(args.warmup):
                loop()
                batch()
            torch.cuda.synchronize()
            t = {"loop": [], "batch": []}
            f = {"loop": [], "batch": []}
            h = {"loop": [], "batch": []}
            for _ in range(args.reps):
                for name, fn in (("loop", loop), ("batch", batch)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    res, fwd, hs, tokens = fn()
                    t[name].append((time.perf_counter() - t0) * 1e3 / nq)
                    f[name].append(fwd)
                    h[name].append(hs * 1e3 / nq)
                    if name == "loop":
                        a = res
                    else:
                        b = res
                        assert tokens == int(np.sum(toks)), (tokens, int(np.sum(toks)))
            same = sum(1 for x, y in zip(a, b) if [c.chunk_id for c in x] == [c.chunk_id for c in y]) / nq
            med = {k: statistics.median(v) for k, v in t.items()}
            tf = {k: flops(toks) / (statistics.median(v) * 1e-3) / 1e12 for k, v in f.items()}
            line = (f"nq {nq:3d}  pairs {kind:>16s}  boosts {'yes' if boosted else 'no ':3s}  tokens {int(np.sum(toks)):7d}  "
                    f"loop {med['loop']:7.3f} ms/question (min {min(t['loop']):.3f} max {max(t['loop']):.3f})  "
                    f"batch {med['batch']:7.3f} ms/question (min {min(t['batch']):.3f} max {max(t['batch']):.3f})  loop/batch {med['loop'] / med['batch']:.2f}x  "
                    f"forward GPU ms {statistics.median(f['loop']):.2f} -> {statistics.median(f['batch']):.2f}  TF/s {tf['loop']:.0f} -> {tf['batch']:.0f}  "
                    f"head+select GPU us/question {statistics.median(h['loop']):.1f} -> {statistics.median(h['batch']):.1f}  same kept ids {same:.2f}")
            lines.append(line)
            print(line, flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
