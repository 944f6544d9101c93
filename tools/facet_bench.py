"""Value counts against the routes a user has today, alternated call by call in one process on one GPU.

    python tools/facet_bench.py [--out profiles/facets] [--name ab] [--cases ref4,uniform] [--targets 100,2000] [--calls 20] [--rows 1000000]

Cases (dim 1024, tools/range_bench.py's corpora): ref4 = 16 919 rows (the reference's store), 4 queries; uniform = --rows rows x 256
queries of synth's N(0,1) corpus. Two metadata keys are laid over the rows: `nature`, six values with shares 50 / 20 / 15 / 10 / 4 / 1 %
(a skewed key), and `doc`, one value per 8 consecutive rows (rows / 8 values: a wide table).

Corpus facets, per key: Collection.facets_device(key) against (a) the reference's route, len(get(where={key: v}, include=[])["ids"]) per
value (`nature` only: one id list per value) and (b) np.unique(column_values(key), return_counts=True). The host routes run --calls / 5
times (at least twice): they take seconds at 1 M rows.

Query facets, per key and target T (mean rows in range per query; ONE distance per target, range_bench.distance_for): the arms are
    facets   query_facets_device(q, key, D, limit=10)
    base     query_range_device(q, D, max_results=1024) + torch.bincount of the device row -> code table at the listed rows + topk
    range    query_range_device(q, D, max_results=1024) alone: facets - range is what the counting adds
`base` is complete only while every total <= 1024: `cut` = the queries for which it is not (its counts are then those of the best
1 024 rows, a truncated answer); `same` = base's counts equal facets' for the queries that are not cut.
The sub-chunk budget (option facet_table_kb) is timed for `doc` at the largest target, at 4 / 16 / 64 / 256 MiB.
-> <name>.txt + <name>.json under --out. Milliseconds per call: median and minimum, host clock around the call and a device synchronise."""
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

NATURES = ["DOCTRINE", "GUIDE", "SANCTION", "DELIBERATION", "FAQ", "OTHER"]
SHARES = [0.50, 0.20, 0.15, 0.10, 0.04, 0.01]


def str_column(codes: np.ndarray, vocab):
    """a where.Column of strings filled in one piece (Column.set row by row takes minutes at 1 M rows)"""
    from rag_dpo_amd import where as W
    c = W.Column(len(codes))
    c.kind[:] = W.K_STR
    c.code[:] = codes
    c.vocab = list(vocab)
    c._lookup = {s: i for i, s in enumerate(c.vocab)}
    return c


def add_keys(col):
    n = col.count()
    rng = np.random.default_rng(n)
    col._cols["nature"] = str_column(rng.choice(len(NATURES), n, p=SHARES).astype(np.int32), NATURES)
    col._cols["doc"] = str_column((np.arange(n) // 8).astype(np.int32), [f"doc{i:06d}" for i in range((n + 7) // 8)])
    col._writes += 1
    # the fields above are Collection's own: if they move, say so here instead of measuring something else
    assert col.get(ids=["c9"], include=["metadatas"])["metadatas"][0]["doc"] == "doc000001"


def timed(arms: dict, calls: int, sync):
    ms = {a: [] for a in arms}
    for turn in range(calls + 2):
        for name, fn in arms.items():
            sync()
            t = time.perf_counter()
            out = fn()
            sync()
            if turn >= 2:
                ms[name].append((time.perf_counter() - t) * 1e3)
            del out
    return {a: (float(np.median(v)), float(np.min(v))) for a, v in ms.items()}


def corpus_facets(col, key: str, calls: int):
    import torch
    values = col.facets(key)["values"]

    def per_value():
        return [len(col.get(where={key: v}, include=[])["ids"]) for v in values]

    def unique():
        return np.unique(np.asarray(col.column_values(key)), return_counts=True)

    rec = {"key": key, "n_values": len(values)}
    rec["facets"] = timed({"facets": lambda: col.facets_device(key)}, calls, torch.cuda.synchronize)["facets"]
    slow = {"np_unique": unique}
    if len(values) <= 16:
        slow["get_per_value"] = per_value
    rec.update(timed(slow, max(2, calls // 5), torch.cuda.synchronize))
    counts = col.facets_device(key)[0].cpu().numpy()
    u, c = unique()
    rec["same"] = sorted(c.tolist()) == sorted(counts[counts > 0].tolist())
    return rec


def query_facets(col, q, key: str, D: float, calls: int):
    import torch
    from rag_dpo_amd import groups as GR
    tables = GR.group_tables(col, key)
    code, G = tables.device(q.device)[0], tables.n_groups
    nq = int(q.shape[0])
    base_q = torch.arange(nq, device=q.device)[:, None] * G

    def base():
        dist, rows, counts, totals = col.query_range_device(q, D, 1024)
        c = code[rows.clamp(min=0)].long()
        ok = (rows >= 0) & (c >= 0)
        table = torch.bincount((base_q + c)[ok], minlength=nq * G).view(nq, G)
        top = torch.topk(table, min(10, G), dim=1)
        return table, top, totals

    arms = {"facets": lambda: col.query_facets_device(q, key, D, 10), "base": base, "range": lambda: col.query_range_device(q, D, 1024)}
    rec = {"key": key, "max_distance": D, "n_values": G}
    rec.update(timed(arms, calls, torch.cuda.synchronize))
    before = col.facet_stats
    codes, cnt, nv, mis, tot = col.query_facets_device(q, key, D, 10)
    after = col.facet_stats
    rec["mfma_queries"], rec["exact_queries"] = after["mfma"] - before["mfma"], after["exact"] - before["exact"]
    rec["total_mean"], rec["total_max"], rec["cut_queries"] = float(tot.float().mean()), int(tot.max()), int((tot > 1024).sum())
    table, top, totals = base()
    whole = tot <= 1024
    mine = torch.sort(cnt[whole], dim=1, descending=True)[0][:, : top[0].shape[1]]
    rec["same"] = bool((mine == top[0][whole]).all()) and bool((totals == tot).all())
    return rec


def main():
    import torch
    from rag_dpo_amd import _lib
    from range_bench import build_case, distance_for
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "facets"))
    ap.add_argument("--name", default="ab")
    ap.add_argument("--cases", default="ref4,uniform", type=lambda s: s.split(","))
    ap.add_argument("--targets", default="100,2000", type=lambda s: [int(x) for x in s.split(",")])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rows", type=int, default=1_000_000)
    a = ap.parse_args()
    lib = os.path.basename(_lib.LIB_PATH)
    out, lines = [], [f"# ms per call, median (minimum); library {lib}"]

    def save():
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, a.name + ".json"), "w") as fh:
            json.dump({"dim": 1024, "records": out}, fh, indent=1)
        with open(os.path.join(a.out, a.name + ".txt"), "w") as fh:
            fh.write("\n".join(lines) + "\n")

    def say(line):
        lines.append(line)
        print(line, flush=True)
        save()

    fmt = lambda v: f"{v[0]:10.3f} ({v[1]:9.3f})"   # noqa: E731
    for case in a.cases:
        t0 = time.perf_counter()
        col, q = build_case(case, a.rows)
        add_keys(col)
        nq = int(q.shape[0])
        say(f"# {case}: {col.count()} rows, {nq} queries, built in {time.perf_counter() - t0:.1f} s")
        say(f"{'corpus':>8} {'key':>7} {'values':>7} | {'facets_device':>22} | {'get per value':>22} | {'np.unique':>22} | same")
        for key in ("nature", "doc"):
            rec = corpus_facets(col, key, a.calls)
            rec.update(case=case, rows=col.count(), kind="corpus")
            out.append(rec)
            say(f"{case:>8} {key:>7} {rec['n_values']:>7} | {fmt(rec['facets'])} | {fmt(rec['get_per_value']) if 'get_per_value' in rec else '-':>22} | "
                f"{fmt(rec['np_unique'])} | {rec['same']}")
        pool = torch.sort(col.query_device(q, n_results=4096)[0].reshape(-1))[0]
        say(f"{'query':>8} {'key':>7} {'values':>7} {'T':>5} {'D':>8} | {'facets':>22} | {'base':>22} | {'range':>22} | {'mfma':>4} {'exact':>5} | "
            f"{'tot mean':>8} {'tot max':>7} {'cut':>4} same")
        for target in a.targets:
            D = distance_for(pool, target, nq)
            for key in ("nature", "doc"):
                rec = query_facets(col, q, key, D, a.calls)
                rec.update(case=case, rows=col.count(), nq=nq, target=target, kind="query")
                out.append(rec)
                say(f"{case:>8} {key:>7} {rec['n_values']:>7} {target:>5} {D:8.5f} | {fmt(rec['facets'])} | {fmt(rec['base'])} | {fmt(rec['range'])} | "
                    f"{rec['mfma_queries']:>4} {rec['exact_queries']:>5} | {rec['total_mean']:8.1f} {rec['total_max']:>7} {rec['cut_queries']:>4} {rec['same']}")
        D = distance_for(pool, a.targets[-1], nq)
        for mb in (4, 16, 64, 256):
            col._engine.set_option("facet_table_kb", mb * 1024)
            t = timed({"facets": lambda: col.query_facets_device(q, "doc", D, 10)}, a.calls, torch.cuda.synchronize)["facets"]
            out.append({"case": case, "kind": "budget", "facet_table_mb": mb, "facets": t})
            say(f"{case:>8} budget {mb:>4} MiB, key doc, T {a.targets[-1]} | {fmt(t)}")
        col._engine.set_option("facet_table_kb", 0)
        col._drop_masks()
        col._engine.close()
        del col, q


if __name__ == "__main__":
    main()
