"""Cost of the combined BGE-M3 score: two arms alternated in one process, per shape, and each of A's calls alone.

  A  the four device calls of M3Reranker's scoring: rdx_maxsim_f16 (engine.maxsim), rdx_index_score_pairs (engine.score_pairs),
     rdx_lex_score_pairs (engine.lex_score_pairs), rdx_m3_combine (engine.m3_combine)
  B  the torch formulation a user would write, on device tensors holding the same data: index_select of the normalised rows and a
     row-wise dot; per question a dense [V] float64 weight vector gathered at the candidates' term ids and summed per candidate
     (index_add_); §29's pad / einsum / amax; then three multiplies, two adds and a division

Shapes: 1 question x 40 candidates, 48 x 40, 48 x 1024; dim 1024 for the dense rows and the token vectors; ~300 chunk tokens, ~30
question tokens (tools/maxsim_bench.py's lengths); ~120 terms per chunk and ~12 per question over BGE-M3's vocabulary of 250 002.
Timed with device events around `inner` back-to-back runs of an arm; medians and minima per run. The encoder forward, the host work of
M3Reranker (id -> row lookups, the pinned shape arrays), the boosts and the selection are not part of either arm. There is no speed
threshold: the feature is the capability and the stated arithmetic.

    python tools/m3_bench.py [--reps 9] [--out profiles/m3/ab.txt]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from rag_dpo_amd import engine
from rag_dpo_amd import lexical as LX

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--slots", type=int, default=4096)
ap.add_argument("--out", default=None)
args = ap.parse_args()

DIM, VOCAB, W = 1024, 250002, (0.4, 0.2, 0.4)
dev = torch.device("cuda")
rng = np.random.default_rng(2026)
g = torch.Generator(device="cuda").manual_seed(2026)
N = args.slots


def unit_rows(n):
    v = torch.randn((n, DIM), generator=g, device=dev, dtype=torch.float32)
    return (v / v.norm(dim=1, keepdim=True)).to(torch.float16)


# the token-vector arena (tools/maxsim_bench.py's)
lens = np.clip(np.exp(rng.normal(5.5, 0.65, size=N)), 64, 600).astype(np.int64)
start = np.cumsum(lens) - lens
arena = unit_rows(int(lens.sum()))
slot_start, slot_len = torch.from_numpy(start).to(dev), torch.from_numpy(lens.astype(np.int32)).to(dev)
L_MAX = int(lens.max())
# the dense index and, for arm B, its normalised rows as a tensor
x = torch.randn((N, DIM), generator=g, device=dev, dtype=torch.float32)
index = engine.HipIndex(DIM)
index.add(x)
rows_hat = x / x.norm(dim=1, keepdim=True)
# the lexical index: ~120 terms per chunk, Zipf-like ids; arm B reads the same postings as a CSR by row
n_terms = np.clip(rng.normal(120, 30, size=N), 8, 400).astype(np.int64)
row_of = np.repeat(np.arange(N), n_terms)
term_of = np.minimum((rng.pareto(1.1, size=row_of.size) * 50).astype(np.int64), VOCAB - 1)
key = np.unique(term_of * N + row_of)
term_of, row_of = key // N, key % N
w_of = (rng.integers(1, 64, size=key.size) / 16.0).astype(np.float16)
post_off = np.zeros(VOCAB + 1, dtype=np.int64)
np.cumsum(np.bincount(term_of, minlength=VOCAB), out=post_off[1:])
lex = LX.HipLexical(LX.LexArrays(N, VOCAB, post_off, row_of.astype(np.int32), w_of.view(np.uint16).copy()))
by_row = np.argsort(row_of, kind="stable")
row_off_np = np.zeros(N + 1, dtype=np.int64)
np.cumsum(np.bincount(row_of, minlength=N), out=row_off_np[1:])
row_terms = torch.from_numpy(term_of[by_row]).to(dev)
row_w = torch.from_numpy(w_of[by_row].astype(np.float64)).to(dev)
row_off = torch.from_numpy(row_off_np).to(dev)


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner, r


rows = []
for nq, n_cand in ((1, 40), (48, 40), (48, 1024)):
    n = nq * n_cand
    q_lens = rng.integers(24, 37, size=nq)
    q_off_np = np.zeros(nq + 1, dtype=np.int32)
    np.cumsum(q_lens, out=q_off_np[1:])
    q_vecs, q_off = unit_rows(int(q_off_np[-1])), torch.from_numpy(q_off_np).pin_memory()
    q_dense = torch.randn((nq, DIM), generator=g, device=dev, dtype=torch.float32) * 3.0
    q_terms = [np.sort(rng.choice(2000, size=int(k), replace=False)).astype(np.int32) for k in rng.integers(8, 17, size=nq)]
    t_off_np = np.zeros(nq + 1, dtype=np.int64)
    np.cumsum([len(t) for t in q_terms], out=t_off_np[1:])
    t_off = torch.from_numpy(t_off_np).pin_memory()
    t_ids = torch.from_numpy(np.concatenate(q_terms)).to(dev)
    t_w = torch.from_numpy((rng.integers(1, 64, size=int(t_off_np[-1])) / 16.0).astype(np.float16)).to(dev)
    cand_np = np.stack([rng.choice(N, size=n_cand, replace=n_cand > N) for _ in range(nq)])
    cand = torch.from_numpy(cand_np).to(dev)
    pair_q = torch.arange(nq, dtype=torch.int32, device=dev).repeat_interleave(n_cand)
    pair_row = cand.reshape(-1).contiguous()
    out_c = torch.empty((n,), dtype=torch.float32, device=dev)
    out_d = torch.empty((n,), dtype=torch.float32, device=dev)
    out_s = torch.empty((n,), dtype=torch.float64, device=dev)

    call_maxsim = lambda: engine.maxsim(q_vecs, q_off, arena, slot_start, slot_len, pair_q, pair_row, out_c)     # noqa: E731
    call_dense = lambda: engine.score_pairs(index, q_dense, pair_q, pair_row, out_d)                             # noqa: E731
    call_lex = lambda: engine.lex_score_pairs(lex, t_off, t_ids, t_w, pair_q, pair_row, out_s)                   # noqa: E731
    call_combine = lambda: engine.m3_combine(out_d, out_s, out_c, W)                                             # noqa: E731

    def arm_a():
        call_maxsim(), call_dense(), call_lex()
        return call_combine()

    def arm_b():
        qhat = q_dense / q_dense.norm(dim=1, keepdim=True)
        dense = (rows_hat.index_select(0, pair_row) * qhat.index_select(0, pair_q.long())).sum(dim=1)
        sparse, colbert = [], []
        ar = torch.arange(L_MAX, device=dev)
        for qi in range(nq):
            qw = torch.zeros((VOCAB,), dtype=torch.float64, device=dev)
            qw[t_ids[t_off_np[qi]:t_off_np[qi + 1]].long()] = t_w[t_off_np[qi]:t_off_np[qi + 1]].double()
            b, e = row_off[cand[qi]], row_off[cand[qi] + 1]
            seg = torch.repeat_interleave(torch.arange(n_cand, device=dev), e - b)
            idx = torch.arange(seg.numel(), device=dev) - torch.repeat_interleave((e - b).cumsum(0) - (e - b), e - b) + b[seg]
            sparse.append(torch.zeros((n_cand,), dtype=torch.float64, device=dev).index_add_(0, seg, qw[row_terms[idx]] * row_w[idx]))
            q = q_vecs[q_off_np[qi]:q_off_np[qi + 1]]
            s0, sl = slot_start[cand[qi]], slot_len[cand[qi]]
            docs = arena[(s0[:, None] + ar[None, :]).clamp_(max=arena.shape[0] - 1)]
            sim = torch.einsum("qd,nld->nql", q, docs).float()
            sim.masked_fill_(~(ar[None, :] < sl[:, None])[:, None, :], float("-inf"))
            colbert.append(sim.amax(dim=2).sum(dim=1) / q.shape[0])
        value = (W[0] * dense.double() + W[1] * torch.cat(sparse) + W[2] * torch.cat(colbert).double()) / sum(W)
        return value.float()

    inner = 20 if n <= 2048 else 2
    for _ in range(args.warmup):
        arm_a(), arm_b()
    torch.cuda.synchronize()
    ta, tb = [], []
    alone = {"maxsim": [], "dense_pairs": [], "lex_pairs": [], "combine": []}
    for _ in range(args.reps):                                     # alternating: A, B, A's calls one by one, A, B, ...
        ms, fa = timed(arm_a, inner)
        ta.append(ms)
        ms, fb = timed(arm_b, max(1, inner // 4))
        tb.append(ms)
        for name, fn in (("maxsim", call_maxsim), ("dense_pairs", call_dense), ("lex_pairs", call_lex), ("combine", call_combine)):
            alone[name].append(timed(fn, inner)[0])
    med = statistics.median
    row = {"questions": nq, "candidates": n_cand, "pairs": n, "dim": DIM, "chunk_tokens_mean": round(float(lens[cand_np].mean()), 1),
           "chunk_terms_mean": round(float(n_terms[cand_np].mean()), 1), "question_terms_mean": round(float(np.diff(t_off_np).mean()), 1),
           "four_calls_ms_median": round(med(ta), 4), "four_calls_ms_min": round(min(ta), 4),
           "torch_ms_median": round(med(tb), 4), "torch_ms_min": round(min(tb), 4), "torch_over_four_calls": round(med(tb) / med(ta), 2),
           **{f"{k}_ms_median": round(med(v), 4) for k, v in alone.items()},
           "max_abs_diff_final": float((fa - fb).abs().max()), "pairs_with_a_common_term": int((out_s > 0).sum())}
    rows.append(row)
    print(json.dumps(row), flush=True)

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(f"# tools/m3_bench.py --reps {args.reps} --slots {args.slots}; {torch.cuda.get_device_name(0)}; arms alternated in one process\n")
        for row in rows:
            f.write(json.dumps(row) + "\n")
