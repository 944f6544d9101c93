"""k-means of the stored rows against the route a user had before it: Collection.kmeans_device and the baseline — the rows fetched
through get (engine.get in batches, the host copy a caller of get(include=["embeddings"]) receives) into one device tensor, then a
Lloyd loop in torch: fp32 matmul + argmax + index_add_ + normalize — alternated call by call in one process on one GPU (the protocol
of tools/range_bench.py). The torch loop is a TIMING baseline only: its labels depend on the BLAS path and the reduction order and are
not the definition's; `agree` reports the share of rows both arms label alike after one update, for orientation.

One case per invocation, each GPU step under a time limit of its own:

    timeout -k 10 300 python tools/kmeans_bench.py --case ref   [--calls 5]
    timeout -k 10 900 python tools/kmeans_bench.py --case embed [--rows 1000000] [--calls 2]
    timeout -k 10 900 python tools/kmeans_bench.py --case iid   [--rows 1000000] [--calls 2]

Cases (dim 1024): ref = 16 919 rows of synth's embedding-like corpus with K = 64; embed / iid = --rows rows of the embedding-like /
the N(0,1) corpus with K = 256. Both arms start from the same K stored rows (kmeans.sample_rows, seed 0).
Per case, seconds per call (median and minimum over --calls alternated turns after one unmeasured): the device arm with max_iter = 0
(one assignment: `assign`), 1 and 10; the baseline's loop with 1 and 10 updates, and its fetch (`get`), which a caller pays once per
clustering. `GB/s` = the stored rows' bytes (rows x dim x 4) over the `assign` time: the assignment's rate against reading the corpus
once. -> <name>.txt (appended per case) + <name>_<case>.json under --out."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

DIM = 1024
HEAD = (f"{'case':>6} {'rows':>8} {'K':>4} | {'assign s':>9} {'GB/s':>7} | {'dev 1 s':>8} {'dev 10 s':>9} {'iters':>5} | {'get s':>7} {'base 1 s':>8} {'base 10 s':>9} | "
        f"{'base10/dev10':>12} {'(+get)':>7} | {'agree':>6} | library")


def build_case(case: str, rows: int):
    import torch
    from rag_dpo_amd import synth
    from mmr_bench import make_collection
    dev = torch.device("cuda", 0)
    n, per = (16919 if case == "ref" else rows), synth.CHUNK
    if case == "iid":
        gen = (synth.torch_corpus_chunk(j, min(per, n - j * per), DIM, dev) for j in range(-(-n // per)))
    else:
        gen = (synth.torch_embedlike_chunk(j, min(per, n - j * per), DIM, dev, n) for j in range(-(-n // per)))
    return make_collection(case, n, gen), (64 if case == "ref" else 256)


def fetch(col, batch: int = 65536):
    """the rows as a caller of get(include=["embeddings"]) has them, on the device"""
    import torch
    n = col.count()
    out = torch.empty((n, DIM), dtype=torch.float32, device="cuda")
    for a in range(0, n, batch):
        ids = np.arange(a, min(a + batch, n), dtype=np.int64)
        out[a: a + len(ids)] = torch.from_numpy(col._engine.get(ids)).cuda()
    return out


def torch_lloyd(x, init, iters: int):
    """what a user wrote by hand: labels by fp32 matmul + argmax, sums by index_add_, centroids normalised"""
    import torch
    C = torch.nn.functional.normalize(init, dim=1)
    lab = (x @ C.T).argmax(dim=1)
    for _ in range(iters):
        sums = torch.zeros_like(C).index_add_(0, lab, x)
        empty = sums.norm(dim=1) == 0
        C = torch.where(empty[:, None], C, torch.nn.functional.normalize(sums, dim=1))
        lab = (x @ C.T).argmax(dim=1)
    return lab, C


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def main():
    import torch
    from rag_dpo_amd import _lib, kmeans as KM
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans"))
    ap.add_argument("--name", default="ab")
    ap.add_argument("--case", default="ref", choices=["ref", "embed", "iid"])
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--calls", type=int, default=5)
    a = ap.parse_args()
    lib = os.path.basename(_lib.LIB_PATH)
    t0 = time.perf_counter()
    col, K = build_case(a.case, a.rows)
    n = col.count()
    init = torch.from_numpy(col._engine.get(KM.sample_rows(np.arange(n), K, 0))).cuda()
    print(f"# {a.case}: {n} rows built in {time.perf_counter() - t0:.1f} s; K = {K}", flush=True)
    sec = {k: [] for k in ("assign", "dev1", "dev10", "get", "base1", "base10")}
    iters = 0
    for turn in range(a.calls + 1):
        t_assign, _ = timed(lambda: col.kmeans_device(init=init, max_iter=0))
        t_get, x = timed(lambda: fetch(col))
        t_dev1, d1 = timed(lambda: col.kmeans_device(init=init, max_iter=1))
        t_base1, b1 = timed(lambda: torch_lloyd(x, init, 1))
        t_dev10, d10 = timed(lambda: col.kmeans_device(init=init, max_iter=10))
        t_base10, _ = timed(lambda: torch_lloyd(x, init, 10))
        iters = d10[4]
        agree = float((d1[0] == b1[0]).float().mean())
        del x
        if turn >= 1:
            for k, v in zip(sec, (t_assign, t_dev1, t_dev10, t_get, t_base1, t_base10)):
                sec[k].append(v)
        print(f"#   turn {turn}: assign {t_assign:.4f} s, device {t_dev1:.4f} / {t_dev10:.4f} s ({iters} updates), get {t_get:.3f} s, baseline {t_base1:.4f} / {t_base10:.4f} s", flush=True)
    med = {k: float(np.median(v)) for k, v in sec.items()}
    rec = dict(case=a.case, rows=n, dim=DIM, n_clusters=K, calls=a.calls, median_s=med, min_s={k: float(np.min(v)) for k, v in sec.items()},
               dev10_updates=int(iters), assign_gb_per_s=n * DIM * 4 / med["assign"] / 1e9, base10_over_dev10=med["base10"] / med["dev10"],
               base10_with_get_over_dev10=(med["base10"] + med["get"]) / med["dev10"], labels_agree_after_one_update=agree,
               stats=col.kmeans_stats, library=lib)
    line = (f"{a.case:>6} {n:>8} {K:>4} | {med['assign']:9.4f} {rec['assign_gb_per_s']:7.1f} | {med['dev1']:8.4f} {med['dev10']:9.4f} {iters:>5} | {med['get']:7.3f} "
            f"{med['base1']:8.4f} {med['base10']:9.4f} | {rec['base10_over_dev10']:12.3f} {rec['base10_with_get_over_dev10']:7.3f} | {agree:6.4f} | {lib}")
    print(HEAD + "\n" + line, flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, f"{a.name}_{a.case}.json"), "w") as fh:
        json.dump(rec, fh, indent=1)
    txt = os.path.join(a.out, a.name + ".txt")
    fresh = not os.path.exists(txt)
    with open(txt, "a") as fh:
        fh.write((HEAD + "   (median seconds per call)\n" if fresh else "") + line + "\n")
    col._drop_masks()
    col._engine.close()


if __name__ == "__main__":
    main()
