"""Cost and error of the int8 token-vector store against the fp16 one, on the same vectors, in one process.

The corpus: --slots chunks of 64 ... 600 unit fp16 token vectors at dim 1024 (tools/maxsim_bench.py's lengths) in a MultiVectorStore on
the GPU, and its to_int8() twin. A question has 24 ... 36 tokens; each is a noisy copy (cosine about 0.7) of a random token of one of
the question's candidates, so that the candidates differ in score by more than noise. Shapes (§29's): 1 question x 40 candidates,
48 x 40, 48 x 1024.

Arms, alternated per repetition, timed by device events around `inner` back-to-back calls, medians of --reps:
  f16    rdx_maxsim_f16 on the fp16 store
  i8     rdx_maxsim_i8 on the int8 store, the questions' codes and scales made beforehand
  i8+q   rdx_maxsim_quantize_i8 of the questions' fp16 vectors, then rdx_maxsim_i8: what a rerank call pays
and, once, rdx_maxsim_quantize_i8 over a corpus batch of --batch-rows rows.

Reported besides: both stores' stats()["bytes"]; over a sample of pairs per shape (the first question's first 40 candidates; the numpy
models run on the CPU) the worst and mean |i8 kernel - fp16 model| and the worst ratio to quant_bound, and whether the kernel's bits are
the int8 model's; over every question, the overlap of the top 10 of its first 40 candidates between the two kernels' scores.

    python tools/maxsim_i8_bench.py [--reps 9] [--slots 4096] [--out FILE]
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
from rag_dpo_amd import late_interaction as LI

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--slots", type=int, default=4096)
ap.add_argument("--batch-rows", type=int, default=65536)
ap.add_argument("--out", default=None)
args = ap.parse_args()

DIM = 1024
dev = torch.device("cuda")
rng = np.random.default_rng(2026)
g = torch.Generator(device="cuda").manual_seed(2026)


def unit(v):
    return (v / v.norm(dim=1, keepdim=True)).to(torch.float16)


lens = np.clip(np.exp(rng.normal(5.5, 0.65, size=args.slots)), 64, 600).astype(np.int64)
off = np.zeros(args.slots + 1, dtype=np.int64)
np.cumsum(lens, out=off[1:])
rows_f16 = unit(torch.randn((int(off[-1]), DIM), generator=g, device=dev, dtype=torch.float32))
st16 = LI.MultiVectorStore(DIM, "cuda")
st16.add([f"c{i}" for i in range(args.slots)], (rows_f16, off))
st8 = st16.to_int8()
arena16, slot_start, slot_len = st16.tables()
(codes8, scales8), _, _ = st8.tables()
assert torch.equal(arena16, rows_f16)
bytes16, bytes8 = st16.stats()["bytes"], st8.stats()["bytes"]


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner, r


med = statistics.median
out_rows = []

# the quantiser over a corpus batch
batch = rows_f16[:min(args.batch_rows, rows_f16.shape[0])].contiguous()
bc = torch.empty(batch.shape, dtype=torch.int8, device=dev)
bs = torch.empty((batch.shape[0],), dtype=torch.float32, device=dev)
for _ in range(args.warmup):
    engine.maxsim_quantize(batch, bc, bs)
tq = [timed(lambda: engine.maxsim_quantize(batch, bc, bs), 20)[0] for _ in range(args.reps)]
row = {"quantize_rows": int(batch.shape[0]), "dim": DIM, "quantize_ms_median": round(med(tq), 4), "quantize_ms_min": round(min(tq), 4),
       "quantize_gb_per_s": round(batch.shape[0] * (3 * DIM + 4) / (med(tq) * 1e-3) / 1e9, 1),
       "store_bytes_f16": bytes16, "store_bytes_i8": bytes8, "store_bytes_ratio": round(bytes8 / bytes16, 4), "store_tokens": int(off[-1])}
out_rows.append(row)
print(json.dumps(row), flush=True)

for nq, n_cand in ((1, 40), (48, 40), (48, 1024)):
    q_lens = rng.integers(24, 37, size=nq)
    q_off_np = np.zeros(nq + 1, dtype=np.int32)
    np.cumsum(q_lens, out=q_off_np[1:])
    cand_np = np.stack([rng.choice(args.slots, size=n_cand, replace=n_cand > args.slots) for _ in range(nq)])
    # every question token: a noisy copy of a random token of one of the question's candidates
    src = np.concatenate([off[c] + rng.integers(0, lens[c]) for q in range(nq) for c in [rng.choice(cand_np[q], size=q_lens[q])]])
    base = rows_f16[torch.from_numpy(src).to(dev)].float()
    q_vecs = unit(base + torch.randn(base.shape, generator=g, device=dev) / DIM ** 0.5)
    q_off = torch.from_numpy(q_off_np).pin_memory()
    cand = torch.from_numpy(cand_np).to(dev)
    pair_q = torch.arange(nq, dtype=torch.int32, device=dev).repeat_interleave(n_cand)
    pair_slot = cand.reshape(-1).contiguous()
    n_pairs = nq * n_cand
    s16 = torch.empty((n_pairs,), dtype=torch.float32, device=dev)
    s8 = torch.empty((n_pairs,), dtype=torch.float32, device=dev)
    s8q = torch.empty((n_pairs,), dtype=torch.float32, device=dev)
    cq, sq = engine.maxsim_quantize(q_vecs)
    cq2, sq2 = torch.empty_like(cq), torch.empty_like(sq)
    arm_f16 = lambda: engine.maxsim(q_vecs, q_off, arena16, slot_start, slot_len, pair_q, pair_slot, s16)             # noqa: E731
    arm_i8 = lambda: engine.maxsim_i8(cq, sq, q_off, codes8, scales8, slot_start, slot_len, pair_q, pair_slot, s8)    # noqa: E731

    def arm_i8q():
        engine.maxsim_quantize(q_vecs, cq2, sq2)
        return engine.maxsim_i8(cq2, sq2, q_off, codes8, scales8, slot_start, slot_len, pair_q, pair_slot, s8q)

    inner = 20 if n_pairs <= 2048 else 2
    for _ in range(args.warmup):
        arm_f16(), arm_i8(), arm_i8q()
    torch.cuda.synchronize()
    t16, t8, t8q = [], [], []
    for _ in range(args.reps):                                     # alternating: f16, i8, i8+q, f16, ...
        t16.append(timed(arm_f16, inner)[0])
        t8.append(timed(arm_i8, inner)[0])
        t8q.append(timed(arm_i8q, inner)[0])
    torch.cuda.synchronize()
    h16, h8, h8q = s16.cpu().numpy().reshape(nq, n_cand), s8.cpu().numpy().reshape(nq, n_cand), s8q.cpu().numpy().reshape(nq, n_cand)
    assert h8.tobytes() == h8q.tobytes()
    # the error on a sample: the first question's first 40 candidates, against the numpy models on the CPU
    qh, cqh, sqh = q_vecs[:q_off_np[1]].cpu().numpy(), cq[:q_off_np[1]].cpu().numpy(), sq[:q_off_np[1]].cpu().numpy()
    errs, ratios, model_bits = [], [], True
    for j, s in enumerate(cand_np[0][:40]):
        a, b = int(off[s]), int(off[s + 1])
        d16, cd, sd = rows_f16[a:b].cpu().numpy(), codes8[a:b].cpu().numpy(), scales8[a:b].cpu().numpy()
        m = (qh.astype(np.float64) @ d16.astype(np.float64).T).max(axis=1)
        exact = float(np.sum(m) / len(m))                          # maxsim_model before its rounding to fp32
        errs.append(abs(float(h8[0, j]) - exact))
        ratios.append(errs[-1] / LI.quant_bound(cqh, sqh, cd, sd))
        model_bits &= h8[0, j].tobytes() == LI.maxsim_i8_model(cqh, sqh, cd, sd).tobytes()
    # the top 10 of each question's first 40 candidates under both scorings
    overlap = [len(set(np.argsort(-h16[q, :40], kind="stable")[:10]) & set(np.argsort(-h8[q, :40], kind="stable")[:10])) for q in range(nq)]
    slot_bytes = float(lens[cand_np].sum()) * DIM
    row = {"questions": nq, "candidates": n_cand, "pairs": n_pairs, "question_tokens_mean": round(float(q_lens.mean()), 1),
           "chunk_tokens_mean": round(float(lens[cand_np].mean()), 1), "dim": DIM,
           "f16_ms_median": round(med(t16), 4), "f16_ms_min": round(min(t16), 4), "i8_ms_median": round(med(t8), 4), "i8_ms_min": round(min(t8), 4),
           "i8_with_question_quantize_ms_median": round(med(t8q), 4), "i8_with_question_quantize_ms_min": round(min(t8q), 4),
           "f16_over_i8": round(med(t16) / med(t8), 3), "f16_over_i8_with_question_quantize": round(med(t16) / med(t8q), 3),
           "f16_slot_gb_per_s": round(2 * slot_bytes / (med(t16) * 1e-3) / 1e9, 1), "i8_slot_gb_per_s": round(slot_bytes / (med(t8) * 1e-3) / 1e9, 1),
           "sample_pairs": len(errs), "abs_err_vs_fp16_model_worst": max(errs), "abs_err_vs_fp16_model_mean": float(np.mean(errs)),
           "err_over_quant_bound_worst": max(ratios), "kernel_bits_equal_int8_model_on_sample": bool(model_bits),
           "max_abs_diff_i8_f16_kernels": float(np.abs(h8 - h16).max()),
           "top10_of_40_overlap_mean": round(float(np.mean(overlap)), 2), "top10_of_40_overlap_min": int(min(overlap))}
    out_rows.append(row)
    print(json.dumps(row), flush=True)

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(f"# tools/maxsim_i8_bench.py --reps {args.reps} --slots {args.slots} --batch-rows {args.batch_rows}; {torch.cuda.get_device_name(0)}; "
                "arms alternated in one process, device events\n")
        for row in out_rows:
            f.write(json.dumps(row) + "\n")
