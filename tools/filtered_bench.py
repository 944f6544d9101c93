"""One dense search with a filter per query against the route it replaces.

Arms, alternating in one process on one GPU, the queries on the device:
  loop      Collection.query_device once per distinct filter, with the queries that name it (fusion.py's route before §26)
  filtered  ONE Collection.query_filtered_device

The collection's rows carry an integer key u = row % 64; filter j is {"u": {"$gte": j}}, 0 <= j < F <= 32: it passes (64 - j) / 64 of
the rows, between half and all of them. Query q names filter q % F, so neighbouring queries of an MFMA block differ. Both arms are
warmed (the masks are then in the collection's cache: neither arm evaluates a filter inside the timed window), the results of the two
arms are compared (they must be equal), then each round times one arm after the other, a host clock around calls that end in a device
synchronise. Prints per shape the median and the range of both arms and the ratio of the medians.

    python tools/filtered_bench.py [--out FILE] [--rounds R] [--small-only]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build(rows: int, dim: int, seed: int):
    import torch
    from rag_dpo_amd.collection import Collection
    col = Collection("filtered_bench", metadata={"hnsw:space": "cosine"})
    g = torch.Generator(device="cuda").manual_seed(seed)
    step = 131_072
    for a in range(0, rows, step):
        n = min(step, rows - a)
        col.add(ids=[f"r{i}" for i in range(a, a + n)], embeddings=torch.randn((n, dim), generator=g, device="cuda"),
                metadatas=[{"u": i % 64} for i in range(a, a + n)])
    return col


def arms(col, q, wheres, k):
    import torch
    keys = sorted({w["u"]["$gte"] for w in wheres})
    idx = {j: torch.tensor([t for t, w in enumerate(wheres) if w["u"]["$gte"] == j], device=q.device) for j in keys}
    sub = {j: q.index_select(0, idx[j]).contiguous() for j in keys}

    def loop():
        out = [col.query_device(sub[j], n_results=k, where={"u": {"$gte": j}}) for j in keys]
        torch.cuda.synchronize()
        return out

    def filtered():
        out = col.query_filtered_device(q, wheres, n_results=k)
        torch.cuda.synchronize()
        return out

    def same():
        a, b = loop(), filtered()
        return all(torch.equal(x[i], b[i].index_select(0, idx[j])) for j, x in zip(keys, a) for i in range(3))
    return loop, filtered, same


def measure(col, rows, dim, nq, k, F, rounds, calls, seed, emit):
    import torch
    q = torch.randn((nq, dim), generator=torch.Generator(device="cuda").manual_seed(seed), device="cuda")
    wheres = [{"u": {"$gte": t % F}} for t in range(nq)]
    loop, filtered, same = arms(col, q, wheres, k)
    for _ in range(3):
        loop(), filtered()
    equal = same()
    t = {"loop": [], "filtered": []}
    for _ in range(rounds):
        for name, fn in (("loop", loop), ("filtered", filtered)):
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            t[name].append((time.perf_counter() - t0) / calls * 1e3)
    med = {n: statistics.median(v) for n, v in t.items()}
    bits = col._engine.last_stats()["coarse_bits"]
    emit(f"{rows:>9} x {dim:<5} nq {nq:<4} k {k:<3} F {F:<3} loop {med['loop']:8.3f} ms [{min(t['loop']):.3f} .. {max(t['loop']):.3f}]   "
         f"filtered {med['filtered']:8.3f} ms [{min(t['filtered']):.3f} .. {max(t['filtered']):.3f}]   loop / filtered {med['loop'] / med['filtered']:5.2f}   "
         f"equal {equal}   filtered coarse bits {bits}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--small-only", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("filtered_bench needs a GPU: nothing is measured without one")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    emit(f"# tools/filtered_bench.py: {torch.cuda.get_device_name(0)}; ms per batch, median [min .. max] of {a.rounds} rounds, arms alternating")
    col = build(16_919, 1024, 1)
    measure(col, 16_919, 1024, 48, 50, 8, a.rounds, 20, 2, emit)
    if not a.small_only:
        del col
        col = build(1_000_000, 1024, 3)
        for F in (1, 2, 8, 32):
            measure(col, 1_000_000, 1024, 256, 50, F, a.rounds, 3, 4 + F, emit)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
