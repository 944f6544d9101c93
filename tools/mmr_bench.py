"""Diversity-aware search against the plain search it is built on and against the torch formulation a user would write:
Collection.query_mmr_device(k, fetch_k, lambda 0.5), Collection.query_device(n_results = fetch_k) and a torch MMR (query_device, get of
the candidates' vectors, a Gram matrix by bmm, a Python loop of k rounds), alternated call by call in one process on one GPU.

    python tools/mmr_bench.py [--out profiles/mmr] [--name ab] [--cases ref1,ref4,uniform,embed] [--shapes 10:50,10:256] [--calls 30] [--rows 1000000]

Cases (dim 1024):
    ref1, ref4  16 919 rows (the reference's store), 1 and 4 queries; synth's N(0,1) corpus
    uniform     --rows rows x 256 queries of synth's N(0,1) corpus (10 % of the queries planted next to a row)
    embed       --rows rows x 256 queries of synth's embedding-like corpus: 2 000 documents of near-duplicate chunks, every query
                placed near one document — the corpus on which a plain top-10 is ten copies of one paragraph
Per case and (k, fetch_k): milliseconds per batch of the three calls (median and minimum over --calls alternated turns after 3
unmeasured ones; host clock around the call and a device synchronise), the overhead of MMR over the plain search, the ratio of the
torch formulation to MMR, and how many of MMR's picks are not among the plain top-k (`new/q`, mean per query: what the call is for).
The torch arm's picks are compared with the kernel's and the share of queries with the same picks is printed (`same`): its floats
come from the BLAS, so near-ties may fall differently; it is a yardstick for time, not a reference. The library in use is named on
every line, so a run under RDX_LIB_PATH (a build with another RDX_MMR_WAVES) can be told apart. The collection's host-side fields are
filled directly, as tools/group_bench.py does. -> <name>.txt + <name>.json under --out."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DIM, LAMBDA = 1024, 0.5


def make_collection(name: str, n: int, chunks):
    """chunks: iterable of [rows][DIM] arrays / device tensors in row order"""
    from rag_dpo_amd.collection import Collection
    col = Collection(name)
    col._ensure_engine(DIM)
    for c in chunks:
        col._engine.add(c)
    col._ids = [f"c{i}" for i in range(n)]
    col._docs = [None] * n
    col._row_of = {s: i for i, s in enumerate(col._ids)}
    col._alive = np.ones(n, dtype=bool)
    col._writes += 1
    # the fields above are Collection's own: if they move, say so here instead of measuring something else
    assert col.count() == n == len(col._engine) and col.get(ids=[f"c{n - 1}"])["ids"] == [f"c{n - 1}"]
    return col


def build_case(case: str, rows: int):
    import torch
    from rag_dpo_amd import synth
    dev = torch.device("cuda", 0)
    if case in ("ref1", "ref4"):
        n = 16919
        emb = synth.make_corpus(n, DIM)
        q = torch.from_numpy(synth.make_queries(int(case[3:]), DIM, emb)).to(dev)
        return make_collection(case, n, [emb]), q
    n, per = rows, synth.CHUNK
    if case == "uniform":
        gen = (synth.torch_corpus_chunk(j, min(per, n - j * per), DIM, dev) for j in range(-(-n // per)))
        q = synth.torch_queries(256, DIM, dev, n)
    else:
        gen = (synth.torch_embedlike_chunk(j, min(per, n - j * per), DIM, dev, n) for j in range(-(-n // per)))
        q = synth.torch_embedlike_queries(256, DIM, dev)[0]
    return make_collection(case, n, gen), q.contiguous()


def torch_mmr(col, q, k: int, fetch_k: int):
    """what a user of query_device would write: -> picked rows i64 [nq][k] on the device"""
    import torch
    dist, rows, counts = col.query_device(q, n_results=fetch_k)
    nq = q.shape[0]
    s = 1.0 - dist
    vec = torch.empty((nq * fetch_k, DIM), dtype=torch.float32, device=q.device)
    col._engine.get_device(rows.reshape(-1).clamp(min=0).contiguous(), vec)
    vec = vec.view(nq, fetch_k, DIM)
    gram = torch.bmm(vec, vec.transpose(1, 2))
    live = rows >= 0
    at = torch.arange(nq, device=q.device)
    m = torch.full_like(s, float("-inf"))
    pick = torch.zeros(nq, dtype=torch.int64, device=q.device)
    picks = []
    for t in range(k):
        if t:
            m = torch.maximum(m, gram[at, :, pick])
            v = LAMBDA * s - (1.0 - LAMBDA) * m
            pick = torch.where(live, v, torch.full_like(v, float("-inf"))).argmax(dim=1)
        live[at, pick] = False
        picks.append(pick)
    return torch.gather(rows, 1, torch.stack(picks, dim=1))


def measure(col, q, k: int, fetch_k: int, calls: int):
    import torch
    arms = {"mmr": lambda: col.query_mmr_device(q, k, fetch_k, LAMBDA), "plain": lambda: col.query_device(q, n_results=fetch_k),
            "torch": lambda: torch_mmr(col, q, k, fetch_k)}
    ms = {a: [] for a in arms}
    for turn in range(calls + 3):
        for name, fn in arms.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            if turn >= 3:
                ms[name].append((time.perf_counter() - t) * 1e3)
            del out
    rec = {"k": k, "fetch_k": fetch_k, "calls": calls}
    for a in ms:
        rec[a + "_median_ms"], rec[a + "_min_ms"] = float(np.median(ms[a])), float(np.min(ms[a]))
    rows = col.query_mmr_device(q, k, fetch_k, LAMBDA)[1]
    top = col.query_device(q, n_results=k)[1]
    rec["new_per_query"] = float((rows[:, :, None] != top[:, None, :]).all(dim=2).sum(dim=1).float().mean())
    rec["torch_same"] = float((torch_mmr(col, q, k, fetch_k) == rows).all(dim=1).float().mean())
    return rec


def main():
    from rag_dpo_amd import _lib
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mmr"))
    ap.add_argument("--name", default="ab")
    ap.add_argument("--cases", default="ref1,ref4,uniform,embed", type=lambda s: s.split(","))
    ap.add_argument("--shapes", default="10:50,10:256", type=lambda s: [tuple(int(x) for x in p.split(":")) for p in s.split(",")])
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--rows", type=int, default=1_000_000)
    a = ap.parse_args()
    lib = os.path.basename(_lib.LIB_PATH)
    out = []
    lines = [f"{'case':>8} {'rows':>8} {'nq':>4} {'k':>3} {'F':>4} | {'mmr med':>8} {'mmr min':>8} | {'plain med':>9} {'plain min':>9} | {'over':>7} | "
             f"{'torch med':>9} {'torch min':>9} {'x mmr':>6} | {'new/q':>5} {'same':>5} | library   (ms per batch)"]
    for case in a.cases:
        t0 = time.perf_counter()
        col, q = build_case(case, a.rows)
        print(f"# {case}: {col.count()} rows built in {time.perf_counter() - t0:.1f} s", flush=True)
        for k, fetch_k in a.shapes:
            rec = measure(col, q, k, fetch_k, a.calls)
            rec.update(case=case, rows=col.count(), nq=int(q.shape[0]), library=lib, over_ms=rec["mmr_median_ms"] - rec["plain_median_ms"],
                       torch_over_mmr=rec["torch_median_ms"] / rec["mmr_median_ms"])
            out.append(rec)
            lines.append(f"{case:>8} {rec['rows']:>8} {rec['nq']:>4} {k:>3} {fetch_k:>4} | {rec['mmr_median_ms']:8.3f} {rec['mmr_min_ms']:8.3f} | "
                         f"{rec['plain_median_ms']:9.3f} {rec['plain_min_ms']:9.3f} | {rec['over_ms']:+7.3f} | {rec['torch_median_ms']:9.3f} "
                         f"{rec['torch_min_ms']:9.3f} {rec['torch_over_mmr']:6.1f} | {rec['new_per_query']:5.2f} {rec['torch_same']:5.2f} | {lib}")
            print(lines[-1], flush=True)
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, a.name + ".json"), "w") as fh:
                json.dump({"dim": DIM, "lambda_mult": LAMBDA, "cases": out}, fh, indent=1)
            with open(os.path.join(a.out, a.name + ".txt"), "w") as fh:
                fh.write("\n".join(lines) + "\n")
        col._drop_masks()
        col._engine.close()
        del col, q


if __name__ == "__main__":
    main()
