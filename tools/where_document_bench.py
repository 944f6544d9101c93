"""where_document on the GPU: (a) the substring scan through the C-ABI on numpy-generated arenas, (b) Collection.query with a
where_document at the reference's shape, device store against the host evaluator, alternated in one process.

    python tools/where_document_bench.py kernel [--out DIR] [--big-gb 4.2] [--reps 20]
    python tools/where_document_bench.py query  [--out DIR] [--calls 200]

`kernel` times each (arena, P) case with HIP events around --reps back-to-back rdx_docs_contains calls (device pointers, one
stream) and writes kernel_events.json plus the order of the cases (kernel_cases.json), so that the per-dispatch durations of a
`rocprofv3 --kernel-trace --stats` run of the same command can be assigned to the cases (`trace` below). GB/s = arena bytes
(the padded text the scan reads) per kernel time; peak HBM 8 TB/s. The 20 MB arena stays in the 256 MiB Infinity Cache.

    python tools/where_document_bench.py trace --out DIR --csv TRACE.csv     # per-case kernel time from a kernel-trace CSV
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TBS = 8.0
REF_ROWS = 16919
PATTERNS = ["article 28", "AIPD", "sous-traitant", "responsable de traitement", "durée de conservation", "CNIL", "RGPD",
            "consentement", "intérêt légitime", "transfert", "violation de données", "DPO", "cookies", "profilage",
            "minimisation", "pseudonymisation"]
WORDS = ("le la les des du de et à en un une pour par sur dans avec données personnelles traitement responsable finalité "
         "base légale personne concernée droit accès rectification effacement opposition sécurité mesure technique "
         "organisationnelle délai mois autorité contrôle sanction amende employeur salarié dossier registre analyse "
         "risque impact vie privée information transparence durée conservation sous-traitant contrat article").split()


def make_text(n_docs: int, seed: int, mean_len: int = 1200):
    """French-like chunk text, -> (uint8 bytes, int64 offsets[n + 1]); lengths 600..1800 B, a few keywords planted"""
    rng = np.random.default_rng(seed)
    vocab = [w.encode("utf-8") for w in WORDS]
    lens = rng.integers(mean_len // 2, mean_len * 3 // 2, size=n_docs)
    word_ids = rng.integers(0, len(vocab), size=int(lens.sum() // 6 + n_docs))
    pool = b" ".join(vocab[i] for i in word_ids)
    off = np.zeros(n_docs + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    buf = np.frombuffer(pool[: int(off[-1])], dtype=np.uint8).copy()
    pats = [p.encode("utf-8") for p in PATTERNS]
    for i in rng.choice(n_docs, size=n_docs // 20, replace=False):   # 5 % of the chunks quote a keyword
        p = pats[int(rng.integers(0, len(pats)))]
        s = int(off[i]) + int(rng.integers(0, max(1, int(lens[i]) - len(p))))
        buf[s: s + len(p)] = np.frombuffer(p, dtype=np.uint8)
    return buf, off


def tiled_arena(total_bytes: int, seed: int):
    """an arena past the L3: 64 MiB of chunk text repeated (the scan reads distinct addresses either way)"""
    b, off = make_text(56_000, seed)
    reps = int(np.ceil(total_bytes / b.shape[0]))
    big = np.tile(b, reps)
    n = off.shape[0] - 1
    offs = np.concatenate([off[:-1] + r * b.shape[0] for r in range(reps)] + [np.array([reps * b.shape[0]], dtype=np.int64)])
    return big, offs, n * reps


def store_from(buf, off, n):
    from rag_dpo_amd import _lib as L
    from rag_dpo_amd.engine import DocStore
    st = DocStore(0)
    step = 1 << 20
    for a in range(0, n, step):
        b = min(n, a + step)
        o = np.ascontiguousarray(off[a: b + 1] - off[a])
        seg = np.ascontiguousarray(buf[off[a]: off[b]])
        L.check(st._lib.rdx_docs_append(st._h, ctypes.c_void_p(seg.ctypes.data), ctypes.c_void_p(o.ctypes.data), b - a))
    return st


def kernel(args):
    import torch
    from rag_dpo_amd import _lib as L
    os.makedirs(args.out, exist_ok=True)
    arenas = [("ref_20MB_L3_resident", *make_text(REF_ROWS, 1), REF_ROWS)]
    if args.big_gb > 0:
        big, offs, n = tiled_arena(int(args.big_gb * (1 << 30)), 2)
        arenas.append((f"{args.big_gb:g}GB_past_L3", big, offs, n))
    cases, out = [], []
    for name, buf, off, n in arenas:
        t0 = time.perf_counter()
        st = store_from(buf, off, n)
        torch.cuda.synchronize()
        build_s = time.perf_counter() - t0
        stats = st.stats()
        del buf, off
        words = (n + 31) // 32
        for P in (1, 4, 16):
            st.set_query([p.encode("utf-8") for p in PATTERNS[:P]])
            bits = torch.empty(P * words, dtype=torch.int32, device="cuda")
            stream = torch.cuda.current_stream().cuda_stream

            def run():
                L.check(st._lib.rdx_docs_contains(st._h, ctypes.c_void_p(bits.data_ptr()), L.RDX_DEVICE, ctypes.c_void_p(stream)))
            for _ in range(3):
                run()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                run()
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1000.0 / args.reps
            hits = [int(np.unpackbits(bits[p * words:(p + 1) * words].cpu().numpy().view(np.uint8)).sum()) for p in range(P)]
            rec = {"arena": name, "rows": n, "arena_bytes": stats["arena_bytes"], "P": P, "call_us_events": round(us, 2),
                   "GBps_events": round(stats["arena_bytes"] / us / 1e3, 1),
                   "share_of_peak_events": round(stats["arena_bytes"] / us / 1e6 / PEAK_TBS, 3),
                   "rows_hit": hits, "store_build_s": round(build_s, 2)}
            print(json.dumps(rec), flush=True)
            out.append(rec)
            cases.append({"arena": name, "P": P, "arena_bytes": stats["arena_bytes"], "dispatches": 3 + args.reps})
        st.close()
    json.dump(out, open(os.path.join(args.out, "kernel_events.json"), "w"), indent=1)
    json.dump(cases, open(os.path.join(args.out, "kernel_cases.json"), "w"), indent=1)


def trace(args):
    """per-case k_docs_contains time from a rocprofv3 kernel-trace CSV (dispatch order = case order of kernel_cases.json)"""
    import csv
    cases = json.load(open(os.path.join(args.out, "kernel_cases.json")))
    rows = [r for r in csv.DictReader(open(args.csv)) if "k_docs_contains" in r.get("Kernel_Name", "")]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    res, i = [], 0
    for c in cases:
        d = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0 for r in rows[i: i + c["dispatches"]]][3:]
        i += c["dispatches"]
        med = float(np.median(d)) if d else float("nan")
        res.append({**c, "kernel_us_median": round(med, 2), "kernel_us_min": round(min(d), 2) if d else None,
                    "GBps": round(c["arena_bytes"] / med / 1e3, 1), "share_of_peak": round(c["arena_bytes"] / med / 1e6 / PEAK_TBS, 3)})
        print(json.dumps(res[-1]))
    json.dump(res, open(os.path.join(args.out, "kernel_trace.json"), "w"), indent=1)


def query(args):
    import torch
    from rag_dpo_amd import synth
    from rag_dpo_amd.collection import Collection
    os.makedirs(args.out, exist_ok=True)
    buf, off = make_text(REF_ROWS, 3)
    docs = [bytes(buf[off[i]: off[i + 1]]).decode("utf-8", errors="replace") for i in range(REF_ROWS)]
    emb = synth.make_corpus(REF_ROWS, 1024)
    q = synth.make_queries(args.calls, 1024, emb)
    ids = [f"chunk_{i}" for i in range(REF_ROWS)]
    metas = [{"chunk_nature": "GUIDE" if i % 2 else "DOCTRINE"} for i in range(REF_ROWS)]
    cols = {}
    for mode in ("device", "host"):
        c = Collection(f"wd_{mode}", metadata={"hnsw:space": "cosine"})
        for a in range(0, REF_ROWS, 5000):
            c.add(ids=ids[a:a + 5000], embeddings=emb[a:a + 5000], documents=docs[a:a + 5000], metadatas=metas[a:a + 5000])
        if mode == "host":
            c._engine.has_device_docs = False        # the host evaluator (the path of engines without a device store)
        cols[mode] = c
    wd = {"$or": [{"$contains": "article 28"}, {"$contains": "AIPD"}]}
    where = {"chunk_nature": "GUIDE"}
    res = {"rows": REF_ROWS, "where_document": wd, "where": where, "n_results": 50, "calls": args.calls}
    # cold: the first where_document call of the collection (device: includes building the store from the documents)
    for mode, c in cols.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = c.query(query_embeddings=[q[0]], n_results=50, where=where, where_document=wd)
        res[f"{mode}_cold_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        res[f"{mode}_ids0"] = r["ids"][0][:5]
    assert res["device_ids0"] == res["host_ids0"]
    # warm, filter evaluated every call (the bitmap cache dropped before each), and warm with the cached bitmap
    for label, drop in (("filter_each_call", True), ("cached_bitmap", False)):
        t = {m: [] for m in cols}
        for i in range(args.calls):
            for mode, c in cols.items():                 # alternated in the same process
                if drop:
                    c._drop_masks()
                t0 = time.perf_counter()
                r = c.query(query_embeddings=[q[i]], n_results=50, where=where, where_document=wd)
                t[mode].append((time.perf_counter() - t0) * 1e3)
        for mode in cols:
            a = np.array(t[mode])
            res[f"{mode}_{label}_ms_median"] = round(float(np.median(a)), 3)
            res[f"{mode}_{label}_ms_min"] = round(float(a.min()), 3)
    print(json.dumps(res, ensure_ascii=False), flush=True)
    json.dump(res, open(os.path.join(args.out, "query.json"), "w"), indent=1, ensure_ascii=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernel", "query", "trace"])
    ap.add_argument("--csv", help="trace: the kernel-trace CSV of a rocprofv3 run of `kernel`")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "where_document"))
    ap.add_argument("--big-gb", type=float, default=4.2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--calls", type=int, default=200)
    args = ap.parse_args()
    {"kernel": kernel, "query": query, "trace": trace}[args.mode](args)


if __name__ == "__main__":
    main()
