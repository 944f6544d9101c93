"""`where` on the GPU: Collection.query(where=, n_results=50) with the mask cache dropped before every call, the device
predicate scan (engine.MetaStore, csrc/meta_kernel.hpp) against the host evaluator (rag_dpo_amd/where.py), alternated in one
process; and the kernel's own time from a rocprofv3 kernel trace.

    python tools/where_bench.py query  [--out DIR] [--sizes 16919,1000000,10000000] [--calls 200]
    rocprofv3 --kernel-trace --stats --output-format csv -d TRACE -- python tools/where_bench.py kernel [--out DIR] [--sizes ...] [--reps 30]
    python tools/where_bench.py trace --out DIR --csv TRACE/.../*_kernel_trace.csv

Filters: "five" = the reference's enterprise filter over five columns ($and of a 3-value $in on chunk_nature and a 4-way $or of
source $ne and three boolean tags), "one" = a single leaf, "in64" = a 64-value $in on an int column.

`query`: per (size, filter) the two paths take turns call by call (host, device, host, ...) after 5 unmeasured turns each; a
call is Collection.query with one query vector and the default include, timed on the host clock from call to return (the
results are Python lists: nothing is left running). The first device call of a size uploads the named columns; it is reported
on its own (cold_ms), not in the statistics. The collection's columns are filled directly (vectorised): ten million rows through
Collection.add are minutes of Python that this tool does not measure. -> where_query.json + where_query.txt.

`kernel` runs --reps back-to-back rdx_meta_filter calls per case (device pointers, one stream) and writes their order
(kernel_cases.json); `trace` assigns a kernel-trace CSV's k_meta_filter dispatches to the cases: GB/s = 9 bytes x rows x columns
named by the filter / kernel time, against 8 TB/s of HBM; the first 3 dispatches of a case are dropped. The dispatches of a case
read the same columns back to back: up to 1 M rows (9 - 45 MB) these stay in the 256 MB Infinity Cache, so only the 10 M-row
cases are HBM figures."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TBS = 8.0
DIM = 64
NAT = ["GUIDE", "DOCTRINE", "SANCTION", "TECHNIQUE"]
FILTERS = {
    "five": {"$and": [{"chunk_nature": {"$in": ["GUIDE", "DOCTRINE", "TECHNIQUE"]}},
                      {"$or": [{"source": {"$ne": "ENTREPRISE"}}, {"tag_rh": True}, {"tag_securite": True}, {"tag_cookies": True}]}]},
    "one": {"chunk_nature": "GUIDE"},
    "in64": {"doc_id": {"$in": list(range(0, 640, 10))}},
}


def make_columns(n: int, seed: int = 0):
    """the reference's shapes: two dictionary-coded string columns, three sparse boolean tags (missing where not set), an int"""
    from rag_dpo_amd import where as W
    rng = np.random.default_rng(seed)

    def column(kind, num=None, code=None, vocab=()):
        c = W.Column(0)
        c.kind = kind.astype(np.int8)
        c.num = np.zeros(n) if num is None else num.astype(np.float64)
        c.code = np.full(n, -1, dtype=np.int32) if code is None else code.astype(np.int32)
        c.vocab, c._lookup = list(vocab), {s: i for i, s in enumerate(vocab)}
        return c

    cols = {"chunk_nature": column(np.full(n, W.K_STR), code=rng.integers(0, 4, size=n), vocab=NAT),
            "source": column(np.full(n, W.K_STR), code=(rng.random(n) < 0.1), vocab=["CNIL", "ENTREPRISE"]),
            "doc_id": column(np.full(n, W.K_INT), num=rng.integers(0, 1000, size=n))}
    for tag in ("tag_rh", "tag_securite", "tag_cookies"):
        on = rng.random(n) < 0.1
        cols[tag] = column(np.where(on, W.K_BOOL, W.K_MISSING), num=on)
    return cols


def make_collection(n: int):
    from rag_dpo_amd.collection import Collection
    col = Collection(f"where_bench_{n}")
    col._ensure_engine(DIM)
    rng = np.random.default_rng(1)
    first = None
    for a in range(0, n, 1 << 20):
        e = rng.standard_normal((min(1 << 20, n - a), DIM), dtype=np.float32)
        first = e[:1].copy() if first is None else first
        col._engine.add(e)
    col._ids = [f"c{i}" for i in range(n)]
    col._docs = [None] * n
    col._row_of = {s: i for i, s in enumerate(col._ids)}
    col._alive = np.ones(n, dtype=bool)
    col._cols = make_columns(n)
    # the fields above are Collection's own: if they move, say so here instead of measuring something else
    one = col.get(ids=[f"c{n - 1}"])
    assert col.count() == n == len(col._engine) and one["ids"] == [f"c{n - 1}"] and one["metadatas"][0]["chunk_nature"] in NAT
    return col, first


def run_query(args):
    import torch
    out = []
    lines = [f"{'rows':>10} {'filter':>6} | {'host med':>9} {'host min':>9} | {'dev med':>9} {'dev min':>9} | {'host/dev':>8} | {'dev cold':>8}   (ms)"]
    for n in args.sizes:
        t0 = time.perf_counter()
        col, q = make_collection(n)
        print(f"# {n} rows built in {time.perf_counter() - t0:.1f} s", flush=True)
        for name, f in FILTERS.items():
            ms = {"host": [], "dev": []}
            cold = None
            ref = None
            for turn in range(args.calls + 5):
                if turn % 25 == 0:
                    print(f"# {n} {name}: turn {turn}", file=sys.stderr, flush=True)
                for path in ("host", "dev"):
                    col._WHERE_DEVICE_MIN_ROWS = 0 if path == "dev" else 1 << 62
                    col._drop_masks()
                    t = time.perf_counter()
                    r = col.query(query_embeddings=q, n_results=50, where=f)
                    dt = (time.perf_counter() - t) * 1e3
                    if path == "dev" and cold is None:
                        cold = dt
                    if turn >= 5:
                        ms[path].append(dt)
                    if ref is None:
                        ref = r["ids"]
                    assert r["ids"] == ref and len(ref[0]) == 50
            torch.cuda.synchronize()
            rec = {"rows": n, "filter": name, "calls": args.calls, "cold_dev_ms": cold}
            for path in ms:
                rec[path + "_median_ms"], rec[path + "_min_ms"] = float(np.median(ms[path])), float(np.min(ms[path]))
            rec["host_over_dev_median"] = rec["host_median_ms"] / rec["dev_median_ms"]
            out.append(rec)
            lines.append(f"{n:>10} {name:>6} | {rec['host_median_ms']:9.3f} {rec['host_min_ms']:9.3f} | {rec['dev_median_ms']:9.3f} "
                         f"{rec['dev_min_ms']:9.3f} | {rec['host_over_dev_median']:8.2f} | {cold:8.2f}")
            print(lines[-1], flush=True)
            os.makedirs(args.out, exist_ok=True)
            tag = "_".join(str(s) for s in args.sizes)
            with open(os.path.join(args.out, f"where_query_{tag}.json"), "w") as fh:
                json.dump({"calls": args.calls, "dim": DIM, "n_results": 50, "cases": out}, fh, indent=1)
            with open(os.path.join(args.out, f"where_query_{tag}.txt"), "w") as fh:
                fh.write("\n".join(lines) + "\n")
        col._meta_close()
        col._drop_masks()
        col._engine.close()
        del col


def run_kernel(args):
    import torch
    from rag_dpo_amd import where_device as WV
    from rag_dpo_amd.engine import MetaStore
    cases = []
    for n in args.sizes:
        cols = make_columns(n)
        keys = list(cols)
        st = MetaStore(0)
        for slot, k in enumerate(keys):
            st.set_rows(slot, 0, cols[k].kind, cols[k].num, cols[k].code)
        outs = torch.empty((n + 31) // 32, dtype=torch.int32, device="cuda")
        for name, f in FILTERS.items():
            c = WV.compile_where(f, cols)
            lv = c.leaves.copy()
            lv["col"] = np.array([keys.index(k) for k in c.keys], dtype=np.int32)[lv["col"]]
            st.set_query(lv, c.program)
            for _ in range(args.reps):
                st.filter_device(n, outs)
            torch.cuda.synchronize()
            cases.append({"rows": n, "filter": name, "dispatches": args.reps, "columns": len(c.keys), "leaves": int(lv.shape[0]),
                          "bytes": 9 * n * len(c.keys), "passing": int(np.unpackbits(outs.cpu().numpy().view(np.uint8)).sum())})
            print(cases[-1], flush=True)
        st.close()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "kernel_cases.json"), "w") as fh:
        json.dump(cases, fh, indent=1)


def run_trace(args):
    """per-case k_meta_filter time from a rocprofv3 kernel-trace CSV (dispatch order = case order of kernel_cases.json)"""
    import csv
    cases = json.load(open(os.path.join(args.out, "kernel_cases.json")))
    rows = [r for r in csv.DictReader(open(args.csv)) if "k_meta_filter" in r.get("Kernel_Name", "")]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    assert len(rows) == sum(c["dispatches"] for c in cases), (len(rows), sum(c["dispatches"] for c in cases))
    lines = [f"{'rows':>10} {'filter':>6} {'cols':>4} {'leaves':>6} | {'med us':>9} {'min us':>9} | {'GB/s (med)':>10} {'of 8 TB/s':>9}"]
    i = 0
    for c in cases:
        d = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0 for r in rows[i: i + c["dispatches"]]][3:]
        i += c["dispatches"]
        c["kernel_median_us"], c["kernel_min_us"] = float(np.median(d)), float(np.min(d))
        c["gbs_median"] = c["bytes"] / c["kernel_median_us"] / 1e3
        c["hbm_fraction"] = c["gbs_median"] / (PEAK_TBS * 1e3)
        lines.append(f"{c['rows']:>10} {c['filter']:>6} {c['columns']:>4} {c['leaves']:>6} | {c['kernel_median_us']:9.2f} {c['kernel_min_us']:9.2f} | "
                     f"{c['gbs_median']:10.1f} {100 * c['hbm_fraction']:8.1f}%")
    with open(os.path.join(args.out, "where_kernel.json"), "w") as fh:
        json.dump(cases, fh, indent=1)
    with open(os.path.join(args.out, "where_kernel.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["query", "kernel", "trace"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "where"))
    ap.add_argument("--sizes", default="16919,1000000,10000000", type=lambda s: [int(x) for x in s.split(",")])
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--csv", help="trace: the kernel-trace CSV of a rocprofv3 run of `kernel`")
    a = ap.parse_args()
    {"query": run_query, "kernel": run_kernel, "trace": run_trace}[a.mode](a)
