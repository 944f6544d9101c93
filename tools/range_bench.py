"""Threshold search against the route a user has today: Collection.query_range_device(D, max_results) and the baseline
Collection.query_device(n_results = max_results) followed by the cut at D on the device, alternated call by call in one process on one
GPU. The baseline lists at most max_results rows, so it cannot say how many rows are in range once that exceeds max_results; the
range search always does (`total`).

    python tools/range_bench.py [--out profiles/range] [--name ab] [--cases ref4,uniform,embed] [--shapes 10:100,100:100,1000:100,1000:1024]
                                [--calls 30] [--rows 1000000]

Cases (dim 1024):
    ref4        16 919 rows (the reference's store), 4 queries; synth's N(0,1) corpus
    uniform     --rows rows x 256 queries of synth's N(0,1) corpus (10 % of the queries planted next to a row)
    embed       --rows rows x 256 queries of synth's embedding-like corpus: 2 000 documents of near-duplicate chunks, every query
                placed near one document
A shape T:m is a target for the mean number of rows in range per query and max_results. ONE distance D per (case, T) serves all the
queries: the (T nq)-th smallest of the queries' pooled 4 096 best distances, taken from the engine's exact scores
(query_device(n_results = 4096): the exact full scan, the oracle's bits by the parity tests) — the oracle itself does not hold
a 1 M-row corpus that is generated on the device. On the embedding-like corpus the per-query totals under one D range from 0 to
thousands, which is the case the call exists for.
Per case and shape: milliseconds per batch of both calls (median and minimum over --calls alternated turns after 3 unmeasured ones;
host clock around the call and a device synchronise), the ratio baseline / range, the queries per path of one range call (MFMA
path / exact scan, from Collection.range_stats), and the rows in range per query (mean, max; `cut` = queries whose total exceeds
max_results: the baseline's count is wrong for them). The collection's host-side fields are filled directly, as tools/mmr_bench.py does.
-> <name>.txt + <name>.json under --out."""
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


def build_case(case: str, rows: int):
    import torch
    from rag_dpo_amd import synth
    from mmr_bench import make_collection
    dev = torch.device("cuda", 0)
    if case.startswith("ref"):
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


def distance_for(pool, target: int, nq: int) -> float:
    """the distance under which target * nq of the pooled best distances lie"""
    at = min(target * nq, pool.numel()) - 1
    return float(pool[at])


def measure(col, q, D: float, m: int, calls: int):
    import torch

    def baseline():
        dist, rows, counts = col.query_device(q, n_results=m)
        keep = dist <= D
        return dist, torch.where(keep, rows, torch.full_like(rows, -1)), keep.sum(dim=1)

    arms = {"range": lambda: col.query_range_device(q, D, m), "base": baseline}
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
    rec = {"max_distance": D, "max_results": m, "calls": calls}
    for a in ms:
        rec[a + "_median_ms"], rec[a + "_min_ms"] = float(np.median(ms[a])), float(np.min(ms[a]))
    before = col.range_stats
    dist, rows, counts, totals = col.query_range_device(q, D, m)
    after = col.range_stats
    rec["mfma_queries"], rec["exact_queries"] = after["mfma"] - before["mfma"], after["exact"] - before["exact"]
    rec["total_mean"], rec["total_max"] = float(totals.float().mean()), int(totals.max())
    rec["cut_queries"] = int((totals > m).sum())
    b = baseline()
    rec["same_rows"] = bool((b[1] == rows).all()) and bool((b[2] == counts).all())      # the identity the tests pin, seen once more
    return rec


def main():
    import torch
    from rag_dpo_amd import _lib
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "range"))
    ap.add_argument("--name", default="ab")
    ap.add_argument("--cases", default="ref4,uniform,embed", type=lambda s: s.split(","))
    ap.add_argument("--shapes", default="10:100,100:100,1000:100,1000:1024", type=lambda s: [tuple(int(x) for x in p.split(":")) for p in s.split(",")])
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--rows", type=int, default=1_000_000)
    a = ap.parse_args()
    lib = os.path.basename(_lib.LIB_PATH)
    out = []
    lines = [f"{'case':>8} {'rows':>8} {'nq':>4} {'T':>5} {'m':>5} {'D':>8} | {'range med':>9} {'range min':>9} | {'base med':>9} {'base min':>9} | "
             f"{'base/rng':>8} | {'mfma':>4} {'exact':>5} | {'tot mean':>8} {'tot max':>7} {'cut':>4} {'same':>5} | library   (ms per batch)"]
    for case in a.cases:
        t0 = time.perf_counter()
        col, q = build_case(case, a.rows)
        nq = int(q.shape[0])
        pool = torch.sort(col.query_device(q, n_results=4096)[0].reshape(-1))[0]
        print(f"# {case}: {col.count()} rows built in {time.perf_counter() - t0:.1f} s", flush=True)
        for target, m in a.shapes:
            rec = measure(col, q, distance_for(pool, target, nq), m, a.calls)
            rec.update(case=case, rows=col.count(), nq=nq, target=target, library=lib, base_over_range=rec["base_median_ms"] / rec["range_median_ms"])
            out.append(rec)
            lines.append(f"{case:>8} {rec['rows']:>8} {nq:>4} {target:>5} {m:>5} {rec['max_distance']:8.5f} | {rec['range_median_ms']:9.3f} "
                         f"{rec['range_min_ms']:9.3f} | {rec['base_median_ms']:9.3f} {rec['base_min_ms']:9.3f} | {rec['base_over_range']:8.2f} | "
                         f"{rec['mfma_queries']:>4} {rec['exact_queries']:>5} | {rec['total_mean']:8.1f} {rec['total_max']:>7} {rec['cut_queries']:>4} "
                         f"{str(rec['same_rows']):>5} | {lib}")
            print(lines[-1], flush=True)
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, a.name + ".json"), "w") as fh:
                json.dump({"dim": DIM, "cases": out}, fh, indent=1)
            with open(os.path.join(a.out, a.name + ".txt"), "w") as fh:
                fh.write("\n".join(lines) + "\n")
        col._drop_masks()
        col._engine.close()
        del col, q


if __name__ == "__main__":
    main()
