"""Cost of the cross-encoder rerank stage: one question x 40 candidates (the reference's rerank_candidates, src/rag/pipeline.py:128),
bge-reranker-v2-m3's architecture (XLM-R-large, XLMRobertaForSequenceClassification, one label), random-init fp16, hashing tokenizer.

Per candidate shape — every pair 128, 256 or 512 tokens, and tools/ingest_bench.py's log-normal chunk lengths (mean ~300, clipped to
[64, 1024]) cut at the 512-token pair limit — two legs run alternately in one process:
  rerank    CrossEncoderReranker.rerank(top_k=10) on the GPU: packed forward, rdx_rerank_head_f16, rdx_rerank_select, results on the host
  baseline  what sentence-transformers' CrossEncoder.predict runs on the same GPU: transformers' module forward in fp16 over padded batches
            of 32 pairs in input order, sigmoid, scores to the host, a host sort (numpy, stable) and the top 10
Reported: ms per call (median, min) of both; for the rerank leg the host tokenise + pack ms, the forward's GPU ms, the head + select
GPU us and the forward's TF/s (2 x 303 M weights x tokens + 4 x hidden x length^2 per layer and pair for the attention).

    python tools/rerank_bench.py [--reps 15] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from rag_dpo_amd.reranker import CrossEncoderReranker
from rag_dpo_amd.retriever import RetrievedChunk

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()

N_CAND, TOP_K = 40, 10
VOCAB = [a + b for a in "abcdefghijklmnopqrstuvwxyz" for b in "abcdefghijklmnopqrstuvwxyz"]   # 3 characters a word: 512 tokens fit 2048
rng = np.random.default_rng(2026)
QUERY = " ".join(rng.choice(VOCAB, 12))                  # 12 pieces: a pair of L tokens has L - 16 text pieces


def candidates(lengths):
    return [RetrievedChunk(chunk_id=f"c{i}", text=" ".join(rng.choice(VOCAB, max(1, int(L) - 16))), document_path=f"doc{i % 9}",
                           chunk_nature="GUIDE", chunk_index=i, confidence="high", distance=0.3, metadata={"chunk_nature": "GUIDE"})
            for i, L in enumerate(lengths)]


mix = np.clip(np.exp(rng.normal(5.5, 0.65, size=N_CAND)), 64, 1024).astype(np.int64)   # tools/ingest_bench.py's chunk lengths
SHAPES = {"128": [128] * N_CAND, "256": [256] * N_CAND, "512": [512] * N_CAND, "lognormal_cut512": list(np.minimum(mix + 14, 512))}

r = CrossEncoderReranker("random-init:xlm-roberta-large", device="cuda", dtype=torch.float16, min_score=0.0)
r._load_model()
m = r._model
cfg = m.model.config
assert m.path == "fused", m.path


def baseline(chunks):
    """sentence-transformers' CrossEncoder.predict on the module forward, then the reference's sort and top_k"""
    pairs = [(QUERY, c.text[:r.max_length * 4]) for c in chunks]
    enc = m.tokenize([p[0] for p in pairs], [p[1] for p in pairs])
    out = []
    with torch.no_grad():
        for a in range(0, len(pairs), 32):
            att = enc["attention_mask"][a:a + 32]
            w = int(att.sum(1).max())
            feed = {"input_ids": enc["input_ids"][a:a + 32, :w].to("cuda"), "attention_mask": att[:, :w].to("cuda")}
            out.append(torch.sigmoid(m.model(**feed).logits.float()).reshape(-1))
    scores = torch.cat(out).cpu().numpy()
    order = np.argsort(-scores.astype(np.float64), kind="stable")
    return order[:TOP_K]


rows = []
for name, lengths in SHAPES.items():
    chunks = candidates(lengths)
    for _ in range(args.warmup):
        r.rerank(QUERY, chunks, top_k=TOP_K)
        baseline(chunks)
    torch.cuda.synchronize()
    t_ours, t_base, fwd, hs, tokz = [], [], [], [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        res = r.rerank(QUERY, chunks, top_k=TOP_K)
        t_ours.append((time.perf_counter() - t0) * 1e3)
        st = r.last_rerank_stats
        fwd.append(st["ms_forward"])
        hs.append(st["ms_head_select"] * 1e3)
        tokz.append(st["ms_tokenize"])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        top = baseline(chunks)
        t_base.append((time.perf_counter() - t0) * 1e3)
    assert len(res) == TOP_K and st["path"] == "fused"
    toks = np.asarray([min(int(L), 512) for L in lengths])
    assert st["tokens"] == int(toks.sum()), (st["tokens"], int(toks.sum()))
    flops = 2.0 * 303e6 * toks.sum() + cfg.num_hidden_layers * 4.0 * cfg.hidden_size * float((toks.astype(np.float64) ** 2).sum())
    padded = sum(len(toks[a:a + 32]) * int(toks[a:a + 32].max()) for a in range(0, len(toks), 32))
    row = {"shape": name, "candidates": N_CAND, "tokens": int(toks.sum()), "tokens_padded_baseline": int(padded),
           "rerank_ms_median": round(statistics.median(t_ours), 3), "rerank_ms_min": round(min(t_ours), 3),
           "baseline_ms_median": round(statistics.median(t_base), 3), "baseline_ms_min": round(min(t_base), 3),
           "speedup_median": round(statistics.median(t_base) / statistics.median(t_ours), 3),
           "tokenize_pack_ms_median": round(statistics.median(tokz), 3), "forward_gpu_ms_median": round(statistics.median(fwd), 3),
           "head_select_gpu_us_median": round(statistics.median(hs), 1), "head_select_gpu_us_min": round(min(hs), 1),
           "forward_tflops": round(flops / (statistics.median(fwd) * 1e-3) / 1e12, 1),
           "same_top1_as_baseline": bool(res[0].original_rank == int(top[0]))}
    rows.append(row)
    print(json.dumps(row), flush=True)

if args.out:
    with open(args.out, "w") as f:
        json.dump({"workload": "one question x 40 candidates, top_k 10; XLM-R-large sequence classifier (bge-reranker-v2-m3 shape), "
                               "random-init fp16, hashing tokenizer; rerank vs the module-forward baseline, alternated in one process",
                   "device": torch.cuda.get_device_name(0), "reps": args.reps, "rows": rows}, f, indent=1)
