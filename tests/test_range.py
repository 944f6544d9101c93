"""CPU: the threshold search's definition (rag_dpo_amd/range_search.py), Collection.query_range on the test-only oracle engine (the host
path) against the cut of query() at the same distance, the argument checks, and plan_range (rag_dpo_amd/csrc/search_plan.hpp) beside
plan_search as a stand-alone program (tests/c_abi/range_plan_dump.cpp, g++ under ASan and UBSan)."""
import os
import subprocess

import numpy as np
import pytest

from rag_dpo_amd import range_search as RS
from rag_dpo_amd.collection import Collection

from oracle_engine import OracleEngine, factory as oracle_factory
from test_sanitizers import ENV, ROOT, SAN

DIM = 64
N = 300
F32 = np.float32


def dist(t):
    return F32(F32(1.0) - F32(t))


# ---- score_threshold ---------------------------------------------------------------------------------------------------------------
def check_threshold(D):
    t = RS.score_threshold(D)
    assert isinstance(t, np.float32)
    assert float(dist(t)) <= float(D), (D, t)                                       # t itself is in range ...
    below = np.nextafter(t, F32(-np.inf))
    if np.isfinite(below):
        assert float(dist(below)) > float(D), (D, t)                                # ... and it is the smallest fp32 that is
    return t


def test_score_threshold_is_the_smallest_score_in_range():
    rng = np.random.default_rng(0)
    for D in [0.0, 1.0, 2.0, 0.3, float(F32(0.3)), 0.30000001192092896, 1e-8, -1e-8, 1.9999999, 2.0000002, -0.5, 3.0, 1e30]:
        check_threshold(D)
    for D in rng.uniform(-0.5, 2.5, 2000):
        check_threshold(float(D))
    for D in rng.uniform(0.0, 2.0, 2000).astype(np.float32):                        # distances that ARE fp32 numbers: some row may sit exactly there
        t = check_threshold(float(D))
        assert float(dist(t)) <= float(D)
    assert RS.score_threshold(np.inf) == -np.inf                                    # every allowed row
    assert RS.score_threshold(0.0) == F32(1.0) and RS.score_threshold(1.0) < 0.0    # fl32(1 - t) == 1 for a few t below 0
    with pytest.raises(ValueError):
        RS.score_threshold(float("nan"))


def test_score_threshold_is_monotone():
    Ds = np.sort(np.random.default_rng(1).uniform(-0.1, 2.1, 500))
    ts = [float(RS.score_threshold(float(D))) for D in Ds]
    assert all(a >= b for a, b in zip(ts, ts[1:]))


def test_as_thresholds():
    assert RS.as_thresholds(0.3, 3).tolist() == [RS.score_threshold(0.3)] * 3
    assert RS.as_thresholds([0.0, np.inf], 2).tolist() == [1.0, -np.inf]
    for bad in ([0.1, 0.2, 0.3], [[0.1, 0.2]], float("nan"), [0.1, float("nan")]):
        with pytest.raises(ValueError):
            RS.as_thresholds(bad, 2)


# ---- range_model against a literal loop --------------------------------------------------------------------------------------------
def literal_range(scores, rows, t, m):
    out_s, out_r, total = [], [], 0
    for s, r in zip(scores, rows):
        if s >= t:
            total += 1
            if len(out_r) < m:
                out_s.append(s)
                out_r.append(r)
    return out_s, out_r, total


@pytest.mark.parametrize("seed", range(6))
def test_range_model_matches_the_literal_loop(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(0, 80))
    s = -np.sort(-np.round(rng.standard_normal(n), 1).astype(np.float32))           # descending, many equal
    r = rng.permutation(1000)[:n].astype(np.int64)
    for t in [-np.inf, np.inf, -2.0, 0.0, -0.0, 0.5] + s[::7].tolist() + [np.nextafter(x, F32(np.inf)) for x in s[::9]]:
        for m in (1, 3, n + 1, 1024):
            gs, gr, gt = RS.range_model(s, r, F32(t), m)
            ws, wr, wt = literal_range(s.tolist(), r.tolist(), float(t), m)
            assert gs.dtype == np.float32 and gr.dtype == np.int64
            assert gs.tobytes() == np.asarray(ws, np.float32).tobytes() and gr.tolist() == wr and gt == wt


# ---- query_range on the oracle engine ----------------------------------------------------------------------------------------------
def make(factory=oracle_factory, space="cosine", n=N):
    """300 rows around a few centres; rows 40..47 are exact copies of row 7; metadata and documents to filter by"""
    rng = np.random.default_rng(5)
    centres = rng.standard_normal((6, DIM)).astype(np.float32)
    emb = (centres[rng.integers(0, 6, n)] + 0.35 * rng.standard_normal((n, DIM))).astype(np.float32)
    emb[40:48] = emb[7]
    col = Collection("c", metadata={"hnsw:space": space}, engine_factory=factory)
    col.add(ids=[f"id{i}" for i in range(n)], embeddings=emb, metadatas=[{"i": i, "nature": ["GUIDE", "DOCTRINE", "SANCTION"][i % 3]} for i in range(n)],
            documents=[f"text {i} {'even' if i % 2 == 0 else 'odd'}" for i in range(n)])
    return col, emb, centres


def cut(res, b, D):
    n = sum(1 for d in res["distances"][b] if d <= D)
    assert all(d <= D for d in res["distances"][b][:n])                             # the in-range entries are a prefix
    return n


def check_against_query(col, q, D, m, **filters):
    got = col.query_range(q, D, max_results=m, **filters)
    top = col.query(q, n_results=m, **filters)
    full = col.query(q, n_results=col.count(), **filters)
    Ds = np.broadcast_to(np.asarray(D, dtype=np.float64), (len(q),))
    for b in range(len(q)):
        n = cut(top, b, Ds[b])
        assert got["ids"][b] == top["ids"][b][:n]
        assert got["distances"][b] == top["distances"][b][:n]
        assert got["documents"][b] == top["documents"][b][:n] and got["metadatas"][b] == top["metadatas"][b][:n]
        assert got["totals"][b] == cut(full, b, Ds[b])
    return got


FILTERS = [{}, {"where": {"nature": "GUIDE"}}, {"where_document": {"$contains": "odd"}}]


@pytest.mark.parametrize("filters", FILTERS, ids=["all", "where", "where_document"])
def test_query_range_is_the_cut_of_query(filters):
    col, emb, centres = make()
    q = np.stack([emb[7], centres[1], emb[100] + 0.05]).astype(np.float32)          # query 0 is a stored row with eight exact copies
    m = 5
    full = col.query(q, n_results=col.count(), **filters)
    for b in range(len(q)):
        d = full["distances"][b]
        assert len(d) > m + 1
        below = float(np.nextafter(F32(d[0]), F32(-np.inf)))
        cases = {"none": below, "one or its ties": d[0], "exactly m or its ties": d[m - 1], "m + 1": d[m], "all": float(np.inf), "all rows": 2.5,
                 "between two rows": (d[2] + d[3]) / 2}
        for name, D in cases.items():
            got = check_against_query(col, q[b:b + 1], D, m, **filters)
            if name == "none":
                assert got["ids"] == [[]] and got["totals"] == [0] and got["distances"] == [[]]
            if name in ("all", "all rows"):
                assert got["totals"] == [len(d)] and len(got["ids"][0]) == m
            if name == "m + 1":
                assert got["totals"][0] >= m + 1 and len(got["ids"][0]) == m
    if not filters:                                                                 # the copies tie at the best distance: all of them, row ascending
        got = col.query_range(q[:1], full["distances"][0][0], max_results=20)
        assert got["ids"][0] == ["id7"] + [f"id{i}" for i in range(40, 48)] and got["totals"] == [9]
    # one threshold per query in one call
    d0, d1, d2 = (full["distances"][b] for b in range(3))
    check_against_query(col, q, [d0[3], float(np.nextafter(F32(d1[0]), F32(-np.inf))), d2[9]], m, **filters)


def test_query_range_follows_deletes_and_includes():
    col, emb, centres = make()
    q = centres[:2]
    best = col.query(q, n_results=6)["ids"]
    col.delete(ids=sorted({i for ids in best for i in ids[::2]}))
    check_against_query(col, q, 0.6, 7)
    check_against_query(col, q, 0.6, 7, where={"nature": "DOCTRINE"}, where_document={"$contains": "even"})
    res = col.query_range(q, 0.6, 7, include=["distances", "embeddings"])
    plain = col.query(q, n_results=7, include=["distances", "embeddings"])
    assert res["documents"] is None and res["metadatas"] is None and res["included"] == ["distances", "embeddings"]
    for b in range(2):
        n = cut(plain, b, 0.6)
        assert res["embeddings"][b].tobytes() == plain["embeddings"][b][:n].tobytes()
    assert col.range_stats == {"queries": 6, "mfma": 0, "exact": 0, "host": 6}
    res = col.query_range(q, 2.5, 3, where={"i": {"$lt": 0}})                       # a filter that allows nothing
    assert res["ids"] == [[], []] and res["totals"] == [0, 0]


def test_empty_collection_returns_empty_lists():
    empty = Collection("e", engine_factory=oracle_factory)
    res = empty.query_range([[0.0] * 8, [1.0] * 8], 0.3)
    assert res["ids"] == [[], []] and res["distances"] == [[], []] and res["totals"] == [0, 0]


def test_query_range_validation():
    col, emb, _ = make(n=40)
    q = emb[:1]
    for bad in (dict(max_distance=float("nan")), dict(max_distance=[0.1, 0.2]), dict(max_distance=[float("nan")]),
                dict(max_distance=0.3, max_results=0), dict(max_distance=0.3, max_results=1025), dict(max_distance=0.3, max_results=True),
                dict(max_distance=0.3, max_results=2.0), dict(max_distance=0.3, max_results=-1)):
        with pytest.raises(ValueError):
            col.query_range(q, **bad)
    for bad in (dict(max_results=0), dict(max_results=1025)):
        with pytest.raises(ValueError):
            col.query_range_device(q, 0.3, **bad)
    with pytest.raises(ValueError):
        col.query_range(q, 0.3, include=["uris"])
    with pytest.raises(ValueError):
        col.query_range(q, 0.3, where_document={"$regex": "x"})
    with pytest.raises(ValueError):
        col.query_range(np.zeros((1, DIM + 4), np.float32), 0.3)                    # wrong dim
    with pytest.raises(ValueError):
        col.query_range(None, 0.3)
    with pytest.raises(NotImplementedError):                                        # the host path has no device output
        col.query_range_device(q, 0.3)
    assert col.range_stats["queries"] == 0                                          # nothing ran


class TwoDeviceEngine(OracleEngine):
    devices = [0, 1]


@pytest.mark.parametrize("space", ["ip", "l2"])
def test_query_range_refuses_the_other_spaces(space):
    col = Collection("s", metadata={"hnsw:space": space}, engine_factory=oracle_factory)
    with pytest.raises(NotImplementedError):
        col.query_range([[1.0] * 8], 0.3)
    with pytest.raises(NotImplementedError):
        col.query_range_device(None, 0.3)


def test_query_range_refuses_a_collection_on_several_devices():
    col = Collection("c", engine_factory=lambda dim, device: TwoDeviceEngine(dim, device))
    col.add(ids=["a", "b"], embeddings=np.eye(2, 8, dtype=np.float32))
    with pytest.raises(NotImplementedError):
        col.query_range(np.ones((1, 8), np.float32), 0.3)


# ---- plan_range beside plan_search -------------------------------------------------------------------------------------------------
FIELDS = ("rc", "exact_only", "i8", "spill", "use_boot", "balance", "stamps", "bn", "nqt", "grid", "n_streams", "res", "fused", "use_small", "capw",
          "list_cap", "n_blocks32", "n_tiles", "k")


@pytest.fixture(scope="module")
def range_plans(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("range_plan") / "range_plan_dump")
    subprocess.check_call(["g++", "-std=c++17", *SAN, "-ffp-contract=off", "-Wall", "-Wextra",
                           os.path.join(ROOT, "tests", "c_abi", "range_plan_dump.cpp"), "-o", exe])

    def run(cases):
        r = subprocess.run([exe], input="\n".join(cases) + "\n", capture_output=True, text=True, timeout=300, env=ENV)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
        lines = r.stdout.splitlines()
        assert len(lines) == len(cases)
        out = []
        for line in lines:
            both = line.split(" => ")[1].split(" | ")
            out.append(tuple(dict(zip(FIELDS, (int(x) for x in part.split()[1:]))) for part in both))
        return out
    return run


ROWS = (0, 1, 600, 8229, 16919, 32768, 32769, 65536, 1000003, 10000000)
BATCH = (1, 3, 4, 64, 65, 128, 129, 130, 256, 257, 384, 385, 1024, 4096)
OPTS = ("", "force_fast=1", "force_exact=1", "force_bn=64", "force_bn=128", "force_bn=256", "small_scan=0", "cand_cap=32", "refine_list=32",
        "fuse_epilogue=0", "coarse_i8=1", "refine_spill=1", "coarse_i8=1 refine_spill=1 force_fast=1")


def test_plan_range_is_the_main_scan_half_of_plan_search(range_plans):
    cases = [f"{r} {b} {k} {d} 256 {o}".strip() for r in ROWS for b in BATCH for k in (1, 10, 100, 256) for d in (64, 320, 1024, 4096) for o in OPTS]
    n_fast = 0
    for case, (R, S) in zip(cases, range_plans(cases)):
        opts = case.split()[5:]
        assert R["rc"] == 0, case
        assert not R["i8"] and not R["spill"] and not R["use_boot"] and not R["balance"] and not R["stamps"], case   # never int8, spill, bootstrap
        if S["rc"] != 0:
            continue
        # int8 changes plan_search's tiling of 257..384 queries and its sizes: the range plan is the fp16 one, so compare with coarse_i8 = 0
        if S["i8"]:
            continue
        assert R["exact_only"] == S["exact_only"], case                            # the small / force_exact / force_fast rule, to the case
        if R["exact_only"]:
            continue
        n_fast += 1
        same = ("bn", "nqt", "grid", "n_streams", "res", "fused", "use_small", "capw", "n_blocks32", "n_tiles", "k")
        assert {f: R[f] for f in same} == {f: S[f] for f in same}, case            # the tiling and the segment size
        assert S["list_cap"] <= R["list_cap"] == (32 if "refine_list=32" in opts else 7168), case   # the whole LDS list, whatever k
        if "cand_cap=32" in opts:
            assert R["capw"] == 32
        if "refine_list=32" in opts:
            assert R["list_cap"] == 32
    assert n_fast > 1000


def test_plan_range_beyond_the_search_s_k_limit(range_plans):
    """max_results above K_FAST_MAX = 256 sends plan_search to the exact scan; plan_range keeps the MFMA path and only sizes its lists"""
    cases = [f"{r} {b} {k} 1024 256 {o}".strip() for r in (8229, 16919, 1000003) for b in (1, 65, 300) for k in (256, 257, 512, 1024)
             for o in ("", "force_fast=1", "force_exact=1", "cand_cap=32", "refine_list=32 force_fast=1")]
    got = dict(zip(cases, range_plans(cases)))
    for case, (R, S) in got.items():
        r, b, k = (int(x) for x in case.split()[:3])
        opts = " ".join(case.split()[5:])
        base = got[f"{r} {b} 256 1024 256 {opts}".strip()][0]
        assert R["rc"] == 0 and R["k"] == k
        if k > 256:
            assert S["exact_only"] == 1
        assert R["exact_only"] == base["exact_only"], case                          # k has no say in the path
        if R["exact_only"]:
            assert "force_exact=1" in opts or "force_fast=1" not in opts
            continue
        for f in ("bn", "nqt", "grid", "n_streams", "res", "fused", "use_small", "n_blocks32", "n_tiles"):
            assert R[f] == base[f], (case, f)
        mul = -(-k // 256)
        assert R["capw"] == (32 if "cand_cap=32" in opts else min(4096, base["capw"] * mul)), case
        assert R["list_cap"] == (32 if "refine_list=32" in opts else 7168), case
        assert 256 * 256 * R["capw"] < 1 << 29                                       # the scan's 32-bit slot index
