"""Near-duplicate clustering against the route a user had before it: Collection.near_duplicates_device(D) and the baseline — batches of
get(include=["embeddings"]) -> query_range_device(rows, D, 1024) -> the lists to the host -> the sequential union-find of
rag_dpo_amd/dedup.py (labels_from_lists) — alternated call by call in one process on one GPU (the protocol of tools/range_bench.py).
The baseline loses the edges of rows with more than 1 024 rows in range; the distances used here leave no such row, so both arms
compute the same labels where both run to the end.

One case per invocation, each GPU step under a time limit of its own:

    timeout -k 10 600  python tools/dedup_bench.py --case ref   [--calls 5]
    timeout -k 10 1100 python tools/dedup_bench.py --case embed [--rows 1000000] [--calls 2] [--base-batches 2]

Cases (dim 1024, synth's embedding-like corpus: 2 000 documents of near-duplicate chunks, a document's chunks stored together):
    ref      16 919 rows (the reference's store): 9 chunks per document
    embed    --rows rows: 500 chunks per document at 1 M
ONE distance D per case, from the engine's own exact scores (query_device of 256 stored rows spread over the corpus, n_results = two
documents' worth): halfway between the largest distance to a chunk of the row's own document and the smallest to any other
document's, so that the clusters are the documents' chunks (`sep` = whether the sample separates them; the labels are then checked
against row // chunks-per-document).
Per case: seconds per call of the device arm (median and minimum over --calls alternated turns after one unmeasured), and of the
baseline — whole calls where --base-batches is 0, otherwise only the first --base-batches batches of 4 096 rows are run per turn and
the whole call is EXTRAPOLATED from them (`base est`: the 1 M-row baseline spends minutes in the host union-find); the baseline's
share spent on the host (copies + union-find); clusters and rows clustered; dedup_stats of one device call; `same` = both arms gave the
same labels (whole baseline calls only). -> <name>.txt (appended per case) + <name>_<case>.json under --out."""
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
BATCH = 4096
HEAD = (f"{'case':>6} {'rows':>8} {'D':>8} {'sep':>5} | {'dev med s':>9} {'dev min s':>9} | {'base med s':>10} {'base min s':>10} {'base est':>8} {'host %':>6} | "
        f"{'base/dev':>8} | {'clusters':>8} {'clustered':>9} {'listed':>8} {'dense':>6} {'batches':>7} {'same':>5} {'docs ok':>7} | library")


def build_case(case: str, rows: int):
    import torch
    from rag_dpo_amd import synth
    from mmr_bench import make_collection
    dev = torch.device("cuda", 0)
    n, per = (16919 if case == "ref" else rows), synth.CHUNK
    gen = (synth.torch_embedlike_chunk(j, min(per, n - j * per), DIM, dev, n) for j in range(-(-n // per)))
    return make_collection(case, n, gen), max(1, -(-n // synth.EMBED_DOCS))


def pick_distance(col, doc_len: int):
    """-> (D, separated) from the exact distances of 256 stored rows to their 2 * doc_len nearest rows"""
    import torch
    n = col.count()
    rows = np.linspace(0, n - 1, 256).astype(np.int64)
    q = torch.from_numpy(col._engine.get(rows)).cuda()
    dist, got, counts = col.query_device(q, n_results=min(2 * doc_len, 4096, n))
    own = (got // doc_len) == torch.from_numpy(rows // doc_len).cuda()[:, None]
    inside, outside = float(dist[own].max()), float(dist[~own & (got >= 0)].min())
    return (inside + outside) / 2 if inside < outside else inside, inside < outside


def baseline(col, D: float, n_batches: int = 0):
    """the route of a user without near_duplicates -> (labels or None when only the first n_batches batches ran, seconds on the host)"""
    import torch
    from rag_dpo_amd import dedup as DD
    n = col.count()
    rows_q, lists, host = [], [], 0.0
    for b, a in enumerate(range(0, n, BATCH)):
        if n_batches and b >= n_batches:
            break
        ids = np.arange(a, min(a + BATCH, n), dtype=np.int64)
        emb = col._engine.get(ids)                                                  # get(include=["embeddings"]): the rows through the host
        dist, rows, counts, totals = col.query_range_device(torch.from_numpy(emb).cuda(), D, 1024)
        torch.cuda.synchronize()
        t = time.perf_counter()
        rows, counts = rows.cpu().numpy(), counts.cpu().numpy()
        rows_q += ids.tolist()
        lists += [rows[k, : counts[k]].tolist() for k in range(len(ids))]
        host += time.perf_counter() - t
    t = time.perf_counter()
    labels = DD.labels_from_lists(n, None, rows_q, lists)
    host += time.perf_counter() - t
    return (labels if len(rows_q) == n else None), host


def main():
    import torch
    from rag_dpo_amd import _lib, dedup as DD
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dedup"))
    ap.add_argument("--name", default="ab")
    ap.add_argument("--case", default="ref", choices=["ref", "embed"])
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--base-batches", type=int, default=0)
    a = ap.parse_args()
    lib = os.path.basename(_lib.LIB_PATH)
    t0 = time.perf_counter()
    col, doc_len = build_case(a.case, a.rows)
    n = col.count()
    D, sep = pick_distance(col, doc_len)
    print(f"# {a.case}: {n} rows built in {time.perf_counter() - t0:.1f} s; {doc_len} chunks per document; D = {D:.5f} (separated: {sep})", flush=True)
    n_batches = -(-n // BATCH)
    part = a.base_batches if 0 < a.base_batches < n_batches else 0
    sec = {"dev": [], "base": []}
    host_share, base_labels, labels = [], None, None
    for turn in range(a.calls + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        labels, totals = col.near_duplicates_device(D)
        torch.cuda.synchronize()
        dt_dev = time.perf_counter() - t
        t = time.perf_counter()
        base_labels, host = baseline(col, D, part)
        torch.cuda.synchronize()
        dt_base = time.perf_counter() - t
        if turn >= 1:
            sec["dev"].append(dt_dev)
            sec["base"].append(dt_base * (n_batches / part if part else 1.0))
            host_share.append(host / dt_base)
        print(f"#   turn {turn}: device {dt_dev:.3f} s, baseline {dt_base:.3f} s" + (f" for {part} of {n_batches} batches" if part else ""), flush=True)
    before = col.dedup_stats
    labels, totals = col.near_duplicates_device(D)
    st = {k: v - before[k] for k, v in col.dedup_stats.items()}
    lab = labels.cpu().numpy()
    groups = DD.clusters_of(lab)
    docs_ok = bool((lab == (np.arange(n) // doc_len) * doc_len).all())              # a document's chunks, labelled with its first row
    same = bool((base_labels == lab).all()) if base_labels is not None else None
    rec = dict(case=a.case, rows=n, dim=DIM, max_distance=D, separated=sep, calls=a.calls, base_batches=part, n_batches=n_batches,
               dev_median_s=float(np.median(sec["dev"])), dev_min_s=float(np.min(sec["dev"])), base_median_s=float(np.median(sec["base"])),
               base_min_s=float(np.min(sec["base"])), base_extrapolated=bool(part), base_host_share=float(np.median(host_share)),
               clusters=len(groups), clustered=int(sum(len(g) for g in groups)), stats=st, same_labels=same, documents_recovered=docs_ok,
               total_max=int(totals.max()), library=lib)
    rec["base_over_dev"] = rec["base_median_s"] / rec["dev_median_s"]
    line = (f"{a.case:>6} {n:>8} {D:8.5f} {str(sep):>5} | {rec['dev_median_s']:9.3f} {rec['dev_min_s']:9.3f} | {rec['base_median_s']:10.3f} "
            f"{rec['base_min_s']:10.3f} {('x%d/%d' % (n_batches, part)) if part else 'whole':>8} {100 * rec['base_host_share']:6.1f} | {rec['base_over_dev']:8.2f} | "
            f"{rec['clusters']:>8} {rec['clustered']:>9} {st['listed']:>8} {st['dense']:>6} {st['batches']:>7} {str(same):>5} {str(docs_ok):>7} | {lib}")
    print(HEAD + "\n" + line, flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, f"{a.name}_{a.case}.json"), "w") as fh:
        json.dump(rec, fh, indent=1)
    txt = os.path.join(a.out, a.name + ".txt")
    fresh = not os.path.exists(txt)
    with open(txt, "a") as fh:
        fh.write((HEAD + "   (seconds per call)\n" if fresh else "") + line + "\n")
    col._drop_masks()
    col._engine.close()


if __name__ == "__main__":
    main()
