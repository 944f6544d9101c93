"""Cost of the lexical-weight search and of the term reduction: arms alternated in one process, per shape.

Search, on the tests/bm25_synth.py Zipf corpus (every posting given a random fp16 weight), 1 / 4 / 48 questions of ~20 terms, top 30:
  A  rdx_lex_search (HipLexical.search): host arrays in, host arrays out, complete on return
  B  the torch formulation a user would write: a torch.sparse_csr [N][V] matrix of the weights times the dense question vectors
     [V][nq] (fp32), then topk over the rows — device tensors in and out, no copy to the host
  C  rdx_bm25_search on the same postings (their tf, rank_bm25's idf), for context
Reduce, 256 texts of ~300 tokens over BGE-M3's vocabulary:
  A  rdx_lex_reduce (engine.lex_reduce)
  B  torch: fp16 rounding and the drop rule as masks, torch.unique over (text, id) keys, scatter_reduce(amax)
Every arm is timed with device events around `inner` back-to-back calls on the current stream (A and C end in a stream synchronise of
their own, which the events include). Last, the share of one LexicalChunkIndex.search call that is the question's encode (XLM-R-large
architecture, random weights, a random sparse head), by a host clock.

    python tools/lexical_bench.py [--reps 9] [--out FILE] [--rows 16919,1000000] [--no-encode]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import bm25_synth as S
from rag_dpo_amd import bm25, engine
from rag_dpo_amd import lexical as LX

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--rows", default="16919,1000000")
ap.add_argument("--out", default=None)
ap.add_argument("--no-encode", action="store_true")
args = ap.parse_args()

dev = torch.device("cuda")
TOP_K, Q_TERMS = 30, 20
med = statistics.median
rows_out = []


def emit(row):
    rows_out.append(row)
    print(json.dumps(row), flush=True)


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner, r


def alternate(arms, inner):
    """arms: {name: callable or None} -> {name: [ms per call]}; A, B, C, A, B, C, ..."""
    live = {k: f for k, f in arms.items() if f is not None}
    for _ in range(args.warmup):
        for f in live.values():
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in live}
    for _ in range(args.reps):
        for k, f in live.items():
            t[k].append(timed(f, inner)[0])
    return t


def stats(t, name):
    return {f"{name}_ms_median": round(med(t[name]), 4), f"{name}_ms_min": round(min(t[name]), 4)} if name in t else {f"{name}_ms_median": "not run"}


# ---- search ---------------------------------------------------------------------------------------------------------------------------
for n_rows in [int(x) for x in args.rows.split(",") if x]:
    vocab, mean_len = (40_000, 200) if n_rows <= 100_000 else (50_000, 40)
    a = S.make(n_rows, vocab, mean_len, seed=n_rows) if n_rows <= 100_000 else S.make_by_term(n_rows, vocab, mean_len, seed=n_rows)
    nnz = len(a.post_row)
    w16 = (np.random.default_rng(n_rows).integers(1, 2048, nnz) / 1024.0).astype(np.float16)
    lex = LX.HipLexical(LX.LexArrays(n_rows, vocab, a.post_off, a.post_row, w16.view(np.uint16)))
    okapi = bm25.HipBm25(a)
    # arm B's matrix: the postings by row (one sort of (row, term) keys on the device)
    sparse_error = None
    try:
        term = torch.repeat_interleave(torch.arange(vocab, device=dev), torch.from_numpy(np.diff(a.post_off)).to(dev))
        key, perm = torch.sort(torch.from_numpy(a.post_row.astype(np.int64)).to(dev) * vocab + term)
        crow = torch.zeros(n_rows + 1, dtype=torch.int64, device=dev)
        crow[1:] = torch.cumsum(torch.bincount(key // vocab, minlength=n_rows), 0)
        M = torch.sparse_csr_tensor(crow, key % vocab, torch.from_numpy(w16.astype(np.float32)).to(dev)[perm], size=(n_rows, vocab))
        del term, key, perm
    except Exception as e:   # an arm that cannot be built is reported, not hidden
        M, sparse_error = None, f"{type(e).__name__}: {e}"
    for nq in (1, 4, 48):
        qs = [np.unique(S.query(vocab, Q_TERMS, 1000 * nq + i)) for i in range(nq)]
        off = np.zeros(nq + 1, np.int64)
        np.cumsum([len(q) for q in qs], out=off[1:])
        ids = np.concatenate(qs).astype(np.int32)
        qw = (np.random.default_rng(nq).integers(1, 2048, len(ids)) / 1024.0).astype(np.float16)
        Q = torch.zeros((vocab, nq), dtype=torch.float32, device=dev)
        Q[torch.from_numpy(ids.astype(np.int64)).to(dev), torch.repeat_interleave(torch.arange(nq), torch.from_numpy(np.diff(off))).to(dev)] = \
            torch.from_numpy(qw.astype(np.float32)).to(dev)
        k = min(TOP_K, n_rows)
        arm_a = lambda: lex.search(off, ids, qw, k)                                  # noqa: E731
        arm_c = lambda: okapi.search(off, ids, k)                                    # noqa: E731
        arm_b = None
        if M is not None:
            arm_b = lambda: torch.topk((M @ Q).t(), k, dim=1)                        # noqa: E731
            try:
                sb = arm_b()
            except Exception as e:
                arm_b, sparse_error = None, f"{type(e).__name__}: {e}"
        t = alternate({"lex": arm_a, "torch_sparse": arm_b, "bm25": arm_c}, 10 if n_rows <= 100_000 else 3)
        row = {"bench": "search", "rows": n_rows, "vocab": vocab, "postings": nnz, "questions": nq, "terms_mean": round(float(np.diff(off).mean()), 1),
               "k": k, **stats(t, "lex"), **stats(t, "torch_sparse"), **stats(t, "bm25")}
        if arm_b is not None:
            sa = lex.search(off, ids, qw, k)
            sb = arm_b()
            row["torch_over_lex"] = round(med(t["torch_sparse"]) / med(t["lex"]), 2)
            row["max_rel_diff_lex_torch_top_score"] = float(np.abs(sb.values[:, 0].double().cpu().numpy() / sa[0][:, 0] - 1).max())
        elif sparse_error:
            row["torch_sparse_error"] = sparse_error[:200]
        row["lex_over_bm25"] = round(med(t["lex"]) / med(t["bm25"]), 2)
        emit(row)
    lex.close()
    okapi.close()
    del M

# ---- reduce ---------------------------------------------------------------------------------------------------------------------------
V, N_TEXTS = 250002, 256
rng = np.random.default_rng(7)
lens = np.clip(np.exp(rng.normal(5.5, 0.5, size=N_TEXTS)), 16, 2000).astype(np.int64)
off_np = np.zeros(N_TEXTS + 1, np.int64)
np.cumsum(lens, out=off_np[1:])
T = int(off_np[-1])
tok = torch.from_numpy((rng.zipf(1.3, T) % V).astype(np.int32)).to(dev)
w = torch.from_numpy(np.maximum(rng.standard_normal(T), 0).astype(np.float32)).to(dev)
off_p = torch.from_numpy(off_np).pin_memory()
outs = (torch.empty(T, dtype=torch.int32, device=dev), torch.empty(T, dtype=torch.float16, device=dev), torch.empty(N_TEXTS, dtype=torch.int32, device=dev))
text_of = torch.repeat_interleave(torch.arange(N_TEXTS, device=dev), torch.from_numpy(lens).to(dev))


def torch_reduce():
    h = w.to(torch.float16)
    keep = torch.isfinite(h) & (h > 0) & (tok > 3)
    key = text_of[keep] * V + tok[keep]
    uniq, inv = torch.unique(key, return_inverse=True)
    best = torch.zeros(uniq.numel(), dtype=torch.float16, device=dev).scatter_reduce(0, inv, h[keep], "amax")
    return uniq, best


t = alternate({"lex_reduce": lambda: engine.lex_reduce(tok, w, off_p, V, (0, 1, 2, 3), *outs), "torch_unique": torch_reduce}, 10)
n_terms = int(outs[2].sum())
uniq, best = torch_reduce()
emit({"bench": "reduce", "texts": N_TEXTS, "tokens": T, "tokens_mean": round(T / N_TEXTS, 1), "terms": n_terms, "same_terms_as_torch": n_terms == int(uniq.numel()),
      **stats(t, "lex_reduce"), **stats(t, "torch_unique"), "torch_over_lex_reduce": round(med(t["torch_unique"]) / med(t["lex_reduce"]), 2)})

# ---- the encode's share of a search call ------------------------------------------------------------------------------------------------
if not args.no_encode:
    from rag_dpo_amd.embedding_provider import EmbeddingProvider
    g = torch.Generator().manual_seed(1)
    prov = EmbeddingProvider(model_name="random-init:xlm-roberta-large", device="cuda", dtype=torch.float16,
                             sparse_head=(torch.randn((1, 1024), generator=g) * 0.05, torch.zeros((1,)))).load()
    n_rows = 16919
    a = S.make(n_rows, prov.lexical_vocab, 200, seed=5)
    ix = LX.LexicalChunkIndex(prov)
    ix._install_csr([f"c{i}" for i in range(n_rows)], [""] * n_rows, [None] * n_rows, a.post_off, a.post_row,
                    (np.random.default_rng(5).integers(1, 2048, len(a.post_row)) / 1024.0).astype(np.float16))
    words = [f"mot{i}" for i in range(5000)]
    for nq in (1, 48):
        questions = [" ".join(np.random.default_rng(100 * nq + i).choice(words, 20)) for i in range(nq)]
        t_all, t_enc = [], []
        for r in range(args.warmup + args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hits = ix.search_batch(questions, top_k=TOP_K)
            t1 = time.perf_counter()
            ids_, w_, _ = prov.embed_lexical_device(questions)
            ids_.cpu(), w_.cpu()
            t2 = time.perf_counter()
            if r >= args.warmup:
                t_all.append((t1 - t0) * 1e3)
                t_enc.append((t2 - t1) * 1e3)
        emit({"bench": "search_call", "rows": n_rows, "questions": nq, "hits_first": len(hits[0]), "search_batch_ms_median": round(med(t_all), 3),
              "encode_ms_median": round(med(t_enc), 3), "encode_share": round(med(t_enc) / med(t_all), 3)})

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(f"# tools/lexical_bench.py --reps {args.reps} --rows {args.rows}; {torch.cuda.get_device_name(0)}; arms alternated in one process\n")
        for row in rows_out:
            f.write(json.dumps(row) + "\n")
