"""Cost of late-interaction scoring: three arms alternated in one process, per shape.

  A  rdx_maxsim_f16 (engine.maxsim) on a MultiVectorStore-like arena: fp16 token vectors, ragged slots, one call for all pairs
  B  the torch formulation a user would write, on the same device tensors: pad the candidates' slots into [cands][L_max][dim] (one
     gather), einsum with the question's tokens, mask, amax over the chunk's tokens, sum over the question's — per question
  C  CrossEncoderReranker.rerank / rerank_batch on candidates of the same token counts, random weights of bge-reranker-v2-m3's shape
     (as tools/rerank_bench.py builds them): what the late-interaction rerank replaces. End to end (tokenise, forward, head, select).

Shapes: 1 question x 40 candidates, 48 x 40, 48 x 1024; ~300 chunk tokens (tools/ingest_bench.py's log-normal lengths, clipped to
[64, 600]), ~30 question tokens, dim 1024. Arm C is not run at 48 x 1024 (49 152 pairs of ~330 tokens through XLM-R-large: minutes).
A and B are timed with device events around `inner` back-to-back calls; C with a host clock around a call that ends in a copy to the
host. Reported: median and min per call, A's and B's largest score difference, A's GFLOP/s over 2 * dim * n_q * n_d per pair.

    python tools/maxsim_bench.py [--reps 9] [--out FILE] [--no-cross-encoder]
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

from rag_dpo_amd import engine

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--slots", type=int, default=4096)
ap.add_argument("--out", default=None)
ap.add_argument("--no-cross-encoder", action="store_true")
args = ap.parse_args()

DIM, TOP_K = 1024, 10
dev = torch.device("cuda")
rng = np.random.default_rng(2026)
g = torch.Generator(device="cuda").manual_seed(2026)


def unit_rows(n):
    v = torch.randn((n, DIM), generator=g, device=dev, dtype=torch.float32)
    return (v / v.norm(dim=1, keepdim=True)).to(torch.float16)


# the arena: args.slots chunks of ~300 token vectors
lens = np.clip(np.exp(rng.normal(5.5, 0.65, size=args.slots)), 64, 600).astype(np.int64)
start = np.cumsum(lens) - lens
arena = unit_rows(int(lens.sum()))
slot_start, slot_len = torch.from_numpy(start).to(dev), torch.from_numpy(lens.astype(np.int32)).to(dev)
L_MAX = int(lens.max())


def torch_formulation(q_vecs, q_off, cand):
    """arm B: per question pad -> einsum -> amax -> sum; cand: int64 [nq][n] slot numbers on the device -> fp32 [nq * n]"""
    out = []
    ar = torch.arange(L_MAX, device=dev)
    for qi in range(cand.shape[0]):
        q = q_vecs[q_off[qi]:q_off[qi + 1]]
        s0, sl = slot_start[cand[qi]], slot_len[cand[qi]]
        live = ar[None, :] < sl[:, None]                                            # [n][L_max]
        docs = arena[(s0[:, None] + ar[None, :]).clamp_(max=arena.shape[0] - 1)]    # the pad: one gather, [n][L_max][dim]
        sim = torch.einsum("qd,nld->nql", q, docs).float()
        sim.masked_fill_(~live[:, None, :], float("-inf"))
        out.append(sim.amax(dim=2).sum(dim=1) / q.shape[0])
    return torch.cat(out)


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner, r


cross = None
if not args.no_cross_encoder:
    from rag_dpo_amd.reranker import CrossEncoderReranker
    from rag_dpo_amd.retriever import RetrievedChunk
    cross = CrossEncoderReranker("random-init:xlm-roberta-large", device="cuda", dtype=torch.float16, min_score=0.0)
    cross._load_model()
    VOCAB = [a + b for a in "abcdefghijklmnopqrstuvwxyz" for b in "abcdefghijklmnopqrstuvwxyz"]

    def chunk_of(i, n_tokens):
        return RetrievedChunk(chunk_id=f"c{i}", text=" ".join(rng.choice(VOCAB, max(1, int(n_tokens)))), document_path=f"doc{i % 9}",
                              chunk_nature="GUIDE", chunk_index=i, confidence="high", distance=0.3, metadata={"chunk_nature": "GUIDE"})

rows = []
for nq, n_cand in ((1, 40), (48, 40), (48, 1024)):
    q_lens = rng.integers(24, 37, size=nq)
    q_off_np = np.zeros(nq + 1, dtype=np.int32)
    np.cumsum(q_lens, out=q_off_np[1:])
    q_vecs = unit_rows(int(q_off_np[-1]))
    q_off = torch.from_numpy(q_off_np).pin_memory()
    cand_np = np.stack([rng.choice(args.slots, size=n_cand, replace=n_cand > args.slots) for _ in range(nq)])
    cand = torch.from_numpy(cand_np).to(dev)
    pair_q = torch.arange(nq, dtype=torch.int32, device=dev).repeat_interleave(n_cand)
    pair_slot = cand.reshape(-1).contiguous()
    scores = torch.empty((nq * n_cand,), dtype=torch.float32, device=dev)
    arm_a = lambda: engine.maxsim(q_vecs, q_off, arena, slot_start, slot_len, pair_q, pair_slot, scores)   # noqa: E731
    arm_b = lambda: torch_formulation(q_vecs, q_off_np, cand)                                             # noqa: E731
    inner = 20 if nq * n_cand <= 2048 else 2
    run_c = cross is not None and nq * n_cand <= 2048
    if run_c:
        questions = [" ".join(rng.choice(VOCAB, int(n) - 1)) for n in q_lens]
        lists = [[chunk_of(i, lens[s] - 1) for i, s in enumerate(row)] for row in cand_np]
        arm_c = (lambda: cross.rerank(questions[0], lists[0], top_k=TOP_K)) if nq == 1 else (lambda: cross.rerank_batch(questions, lists, top_k=TOP_K))
    for _ in range(args.warmup):
        arm_a(), arm_b()
        if run_c:
            arm_c()
    torch.cuda.synchronize()
    ta, tb, tc = [], [], []
    for _ in range(args.reps):                                     # alternating: A, B, C, A, B, C, ...
        ms, sa = timed(arm_a, inner)
        ta.append(ms)
        ms, sb = timed(arm_b, max(1, inner // 4))
        tb.append(ms)
        if run_c:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            arm_c()
            tc.append((time.perf_counter() - t0) * 1e3)
    diff = float((sa - sb).abs().max())
    flops = 2.0 * DIM * float((q_lens[:, None] * lens[cand_np]).sum())
    med = statistics.median
    row = {"questions": nq, "candidates": n_cand, "pairs": nq * n_cand, "question_tokens_mean": round(float(q_lens.mean()), 1),
           "chunk_tokens_mean": round(float(lens[cand_np].mean()), 1), "dim": DIM,
           "maxsim_ms_median": round(med(ta), 4), "maxsim_ms_min": round(min(ta), 4),
           "torch_ms_median": round(med(tb), 4), "torch_ms_min": round(min(tb), 4), "torch_over_maxsim": round(med(tb) / med(ta), 2),
           "cross_encoder_ms_median": round(med(tc), 2) if tc else "not measured", "cross_encoder_ms_min": round(min(tc), 2) if tc else "not measured",
           "cross_encoder_over_maxsim": round(med(tc) / med(ta), 1) if tc else "not measured",
           "maxsim_gflops": round(flops / (med(ta) * 1e-3) / 1e9, 1), "max_abs_diff_maxsim_torch": diff}
    rows.append(row)
    print(json.dumps(row), flush=True)

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(f"# tools/maxsim_bench.py --reps {args.reps} --slots {args.slots}; {torch.cuda.get_device_name(0)}; arms alternated in one process\n")
        for row in rows:
            f.write(json.dumps(row) + "\n")
