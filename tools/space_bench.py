"""The "ip" and "l2" spaces against the cosine search on the same synthetic corpus (synth.torch_corpus_chunk: N(0,1) rows, 1 %
duplicates), one process, one GPU, the three spaces taking turns batch by batch.

    python tools/space_bench.py [--out DIR] [--shapes 16919x4x50,1000000x256x10] [--dim 1024] [--calls 30]

Per shape rows x queries x k: ms per batch (host clock around search_device with device tensors in and out, synchronised; median and
p90 after 5 unmeasured turns each), for ip / l2 the share of the gather (rdx_index_get of the candidates, which waits for the
device) and of the re-score + select kernels (both timed by synchronising around the call in a second, instrumented series — the
synchronisation itself costs, so the shares are upper estimates and the ms figures come from the first series), and last_stats.
-> space_bench.json + ab.txt in --out (default profiles/spaces)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build(space: str, rows: int, dim: int, dev):
    from rag_dpo_amd import spaces as S, synth
    from rag_dpo_amd.engine import HipIndex
    eng = HipIndex(dim, dev.index) if space == "cosine" else S.SpaceEngine(space, HipIndex(S.lifted_dim(space, dim), dev.index))
    if space == "cosine":
        eng.reserve(rows)
    else:
        eng.inner.reserve(rows)
    for j, r0 in enumerate(range(0, rows, synth.CHUNK)):
        eng.add(synth.torch_corpus_chunk(j, min(synth.CHUNK, rows - r0), dim, dev))
    return eng


def run_shape(rows: int, nq: int, k: int, dim: int, calls: int, dev):
    import torch
    from rag_dpo_amd import engine as E, synth
    q = synth.torch_queries(nq, dim, dev, total_rows=rows)
    engines = {s: build(s, rows, dim, dev) for s in ("cosine", "ip", "l2")}
    out = (torch.empty((nq, k), dtype=torch.float32, device=dev), torch.empty((nq, k), dtype=torch.int64, device=dev),
           torch.empty(nq, dtype=torch.int32, device=dev))

    def once(space):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        engines[space].search_device(q, k, *out)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3

    times = {s: [] for s in engines}
    for turn in range(calls + 5):
        for s in engines:
            t = once(s)
            if turn >= 5:
                times[s].append(t)
    # second series: the gather and the re-score of the two spaces, each between two synchronisations
    parts = {s: {"gather": [], "rescore": []} for s in ("ip", "l2")}
    real_rescore = E.space_rescore
    for s in ("ip", "l2"):
        inner = engines[s].inner
        real_get = inner.get_device

        def timed(fn, bucket):
            def wrapped(*a, **kw):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                r = fn(*a, **kw)
                torch.cuda.synchronize(dev)
                bucket.append((time.perf_counter() - t0) * 1e3)
                return r
            return wrapped

        inner.get_device = timed(real_get, parts[s]["gather"])
        E.space_rescore = timed(real_rescore, parts[s]["rescore"])
        try:
            for _ in range(max(5, calls // 3)):
                once(s)
        finally:
            E.space_rescore = real_rescore
            del inner.get_device
    res = {"rows": rows, "queries": nq, "k": k, "dim": dim}
    for s, eng in engines.items():
        t = np.asarray(times[s])
        res[s] = {"ms_median": float(np.median(t)), "ms_p90": float(np.percentile(t, 90))}
        if s != "cosine":
            res[s]["gather_ms"] = float(np.median(parts[s]["gather"]))
            res[s]["rescore_ms"] = float(np.median(parts[s]["rescore"]))
            res[s]["last_stats"] = eng.last_stats
            res[s]["scale_exp"] = eng.scale_exp
            res[s]["inner"] = {kk: vv for kk, vv in eng.inner.last_stats().items() if kk in ("path", "coarse_bits", "k", "rescored")}
        else:
            res[s]["inner"] = {kk: vv for kk, vv in eng.last_stats().items() if kk in ("path", "coarse_bits", "k", "rescored")}
        eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spaces"))
    ap.add_argument("--shapes", default="16919x4x50,1000000x256x10")
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=30)
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    os.makedirs(a.out, exist_ok=True)
    results, lines = [], []
    for shape in a.shapes.split(","):
        rows, nq, k = (int(v) for v in shape.split("x"))
        with torch.cuda.device(dev):
            r = run_shape(rows, nq, k, a.dim, a.calls, dev)
        results.append(r)
        lines.append(f"{rows} rows x {a.dim}, {nq} queries, k = {k} ({a.calls} alternating batches per space)")
        for s in ("cosine", "ip", "l2"):
            e = r[s]
            line = f"  {s:6s} {e['ms_median']:8.3f} ms/batch (p90 {e['ms_p90']:.3f})  engine path {e['inner']}"
            if s != "cosine":
                line += (f"\n         gather {e['gather_ms']:.3f} ms, re-score + select {e['rescore_ms']:.3f} ms (each between two "
                         f"synchronisations), scale 2^{e['scale_exp']}, last_stats {e['last_stats']}")
            lines.append(line)
        print("\n".join(lines[-4:]), flush=True)
    with open(os.path.join(a.out, "space_bench.json"), "w") as f:
        json.dump(results, f, indent=1)
    with open(os.path.join(a.out, "ab.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
