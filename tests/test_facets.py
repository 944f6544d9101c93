"""CPU: the value counts' definitions (rag_dpo_amd/facets.py) and Collection.facets / count(where=...) / query_facets on the test-only
oracle engine (the host path) against a brute-force Counter over column_values, against query_range's totals, and the argument checks."""
import os
from collections import Counter

import numpy as np
import pytest

from rag_dpo_amd import facets as FC
from rag_dpo_amd import groups as GR
from rag_dpo_amd import range_search as RS
from rag_dpo_amd.collection import Collection

from oracle_engine import OracleEngine, factory as oracle_factory

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIM = 32
N = 240
F32 = np.float32
MIXED = ["a", 1, True, 1.5, "b", 0, False, 1.0, "a", "a", 1, "c"]          # 1, True and 1.0 are three values; "a" is the most frequent


def tag(v):
    return (type(v).__name__, v)


def make(factory=oracle_factory, space="cosine", n=N, delete=True):
    """rows around a few centres; rows 40..47 are exact copies of row 7. `nature`: three values on every row; `mixed`: str / int / float /
    bool values, absent on every fifth row; `doc`: one value per four rows (a plateau of equal counts). Some rows are deleted."""
    rng = np.random.default_rng(9)
    centres = rng.standard_normal((5, DIM)).astype(np.float32)
    emb = (centres[rng.integers(0, 5, n)] + 0.35 * rng.standard_normal((n, DIM))).astype(np.float32)
    emb[40:48] = emb[7]
    metas = []
    for i in range(n):
        m = {"i": i, "nature": ["GUIDE", "DOCTRINE", "SANCTION"][(i * i) % 3], "doc": f"d{(i // 4 * 7) % 60:02d}"}
        if i % 5:
            m["mixed"] = MIXED[i % len(MIXED)]
        metas.append(m)
    col = Collection("c", metadata={"hnsw:space": space}, engine_factory=factory)
    col.add(ids=[f"id{i}" for i in range(n)], embeddings=emb, metadatas=metas,
            documents=[f"text {i} {'even' if i % 2 == 0 else 'odd'}" for i in range(n)])
    if delete:
        col.delete(ids=[f"id{i}" for i in (0, 3, 41, 77, 78, 200)])
    return col, emb, centres


def brute(col, key, rows):
    """the listing of `key` over `rows` (live rows that pass the filters): Counter over column_values, count descending, then the value
    that appears first among the LIVE rows"""
    vals = col.column_values(key, default=None)
    live = sorted(int(s[2:]) for s in col.get(include=[])["ids"])
    first = {}
    for r in live:
        if vals[r] is not None:
            first.setdefault(tag(vals[r]), r)
    cnt = Counter(tag(vals[r]) for r in rows if vals[r] is not None)
    order = sorted(cnt, key=lambda t: (-cnt[t], first[t]))
    return [t for t in order], [cnt[t] for t in order], sum(1 for r in rows if vals[r] is None), len(rows)


def rows_of(col, **filters):
    return sorted(int(s[2:]) for s in col.get(include=[], **filters)["ids"])


FILTERS = [{}, {"where": {"nature": "GUIDE"}}, {"where": {"i": {"$gte": 100}}}, {"where_document": {"$contains": "even"}},
           {"where": {"nature": {"$ne": "GUIDE"}}, "where_document": {"$contains": "odd"}}, {"where": {"i": {"$lt": 0}}}]


# ---- the model ---------------------------------------------------------------------------------------------------------------------
def test_the_model_counts_and_orders():
    code = np.array([0, 1, -1, 1, 2, 2, 2, -1, 0, 3], dtype=np.int32)
    counts, missing, total = FC.facet_counts_model(code, 5)
    assert counts.tolist() == [2, 2, 3, 1, 0] and (missing, total) == (2, 10) and counts.dtype == np.int64
    allowed = np.array([1, 1, 1, 0, 0, 1, 1, 0, 0, 0], dtype=bool)
    counts, missing, total = FC.facet_counts_model(code, 5, allowed)
    assert counts.tolist() == [1, 1, 2, 0, 0] and (missing, total) == (1, 5)
    codes, cnt, nv = FC.facet_order([2, 2, 3, 1, 0])
    assert codes.tolist() == [2, 0, 1, 3] and cnt.tolist() == [3, 2, 2, 1] and nv == 4          # zero cells never listed; ties by code
    for limit, want in ((1, [2]), (2, [2, 0]), (4, [2, 0, 1, 3]), (9, [2, 0, 1, 3])):
        codes, cnt, nv = FC.facet_order([2, 2, 3, 1, 0], limit)
        assert codes.tolist() == want and nv == 4
    oc, on, nv = FC.pad_listing(np.array([2, 2, 3, 1, 0]), 6)
    assert oc.tolist() == [2, 0, 1, 3, -1, -1] and on.tolist() == [3, 2, 2, 1, 0, 0] and oc.dtype == np.int32 and on.dtype == np.int64
    assert FC.facet_counts_model(np.zeros(0, np.int32), 0) [1:] == (0, 0)
    for bad in ([0, 5], [-2, 0]):
        with pytest.raises(ValueError, match="outside"):
            FC.facet_counts_model(np.array(bad, dtype=np.int32), 5)


def test_the_query_model_counts_the_rows_at_or_above_the_threshold():
    code = np.array([0, 1, -1, 1, 2], dtype=np.int32)
    s = np.array([0.9, 0.5, 0.5, 0.25, -np.inf], dtype=F32)
    r = np.array([3, 0, 2, 4, -1], dtype=np.int64)
    for t, want in ((0.5, ([1, 1, 0], 1, 3)), (np.nextafter(F32(0.5), F32(1)), ([0, 1, 0], 0, 1)), (-np.inf, ([1, 1, 1], 1, 4)), (np.inf, ([0, 0, 0], 0, 0))):
        counts, missing, total = FC.query_facets_model(s, r, code, 3, t)
        assert (counts.tolist(), missing, total) == want, t


# ---- Collection.facets / count on the host path --------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["nature", "mixed", "doc"])
@pytest.mark.parametrize("filters", FILTERS)
def test_facets_against_a_counter(key, filters):
    col, _, _ = make()
    rows = rows_of(col, **filters)
    tags, counts, missing, total = brute(col, key, rows)
    got = col.facets(key, **filters)
    assert got["key"] == key and [tag(v) for v in got["values"]] == tags and got["counts"] == counts
    assert (got["n_values"], got["missing"], got["total"]) == (len(tags), missing, total)
    assert sum(got["counts"]) + got["missing"] == got["total"]
    assert col.count(**filters) == total == len(rows)
    st = col.facet_stats
    assert st["calls"] == st["calls_host"] == (2 if filters else 1)                      # count() without a filter asks nothing


def test_one_and_true_and_one_point_zero_are_three_values():
    col, _, _ = make()
    got = col.facets("mixed")
    tags = [tag(v) for v in got["values"]]
    assert {("int", 1), ("bool", True), ("float", 1.0)} <= set(tags) and len(tags) == len(set(tags))
    assert tags[0] == ("str", "a")


def test_the_order_inside_a_plateau_and_the_limit():
    col, _, _ = make(delete=False)
    full = col.facets("doc")
    assert len(set(full["counts"])) < len(full["counts"])                                 # equal counts exist
    vals = col.column_values("doc")
    first = {}
    for r, v in enumerate(vals):
        first.setdefault(v, r)
    for a, b, ca, cb in zip(full["values"], full["values"][1:], full["counts"], full["counts"][1:]):
        assert ca > cb or (ca == cb and first[a] < first[b])
    n = full["n_values"]
    for limit in (1, 2, n - 1, n, n + 1, 1024):
        got = col.facets("doc", limit=limit)
        assert got["values"] == full["values"][:limit] and got["counts"] == full["counts"][:limit]
        assert (got["n_values"], got["missing"], got["total"]) == (n, full["missing"], full["total"])


def test_count_is_unchanged_without_a_filter_and_counts_with_one():
    col, _, _ = make()
    assert col.count() == N - 6 == len(col.get(include=[])["ids"])
    for filters in FILTERS[1:]:
        assert col.count(**filters) == len(col.get(include=[], **filters)["ids"])
    assert col.count(where={}) == N - 6


def test_a_write_moves_the_counts():
    col, _, _ = make()
    before = col.facets("nature")
    col.delete(ids=["id5"])
    col.update(ids=["id6"], metadatas=[{"nature": "NEW"}])
    after = col.facets("nature")
    assert after["total"] == before["total"] - 1 and "NEW" in after["values"] and after["counts"][after["values"].index("NEW")] == 1
    tags, counts, missing, total = brute(col, "nature", rows_of(col))
    assert [tag(v) for v in after["values"]] == tags and after["counts"] == counts


def test_the_empty_collection_and_a_key_no_row_has():
    col = Collection("e", engine_factory=oracle_factory)
    assert col.facets("nature") == {"key": "nature", "values": [], "counts": [], "n_values": 0, "missing": 0, "total": 0}
    assert col.count(where={"nature": "GUIDE"}) == 0 and col.count() == 0
    q = col.query_facets(np.ones((2, DIM), dtype=F32), "nature", 0.5)
    assert q == {"key": "nature", "values": [[], []], "counts": [[], []], "n_values": [0, 0], "missing": [0, 0], "totals": [0, 0]}
    col, emb, _ = make()
    got = col.facets("nobody")
    assert got["values"] == [] and got["counts"] == [] and got["n_values"] == 0 and got["missing"] == got["total"] == N - 6
    q = col.query_facets(emb[:2], "nobody", 0.4)
    assert q["values"] == [[], []] and q["n_values"] == [0, 0] and q["missing"] == q["totals"] and q["totals"][0] > 0


@pytest.mark.parametrize("space", ["ip", "l2"])
def test_facets_and_count_work_in_every_space(space):
    col, _, _ = make(space=space)
    tags, counts, missing, total = brute(col, "nature", rows_of(col, where={"i": {"$gte": 100}}))
    got = col.facets("nature", where={"i": {"$gte": 100}})
    assert [tag(v) for v in got["values"]] == tags and got["counts"] == counts and got["total"] == total
    assert col.count(where={"i": {"$gte": 100}}) == total


# ---- query_facets on the host path -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filters", FILTERS[:5])
def test_query_facets_against_the_model_and_query_range(filters):
    col, emb, centres = make()
    q = np.concatenate([centres[:3], emb[7:8]]).astype(F32)
    Ds = [0.25, 0.6, np.inf, 1e-6]
    G = GR.group_tables(col, "mixed").n_groups
    for key in ("nature", "mixed"):
        got = col.query_facets(q, key, Ds, limit=max(G, 3), **filters)
        rng = col.query_range(q, Ds, max_results=1024, include=[], **filters)
        assert got["totals"] == rng["totals"]
        vals = col.column_values(key, default=None)
        for b in range(len(q)):
            assert rng["totals"][b] <= 1024
            rows = [int(s[2:]) for s in rng["ids"][b]]
            tags, counts, missing, total = brute(col, key, rows)
            assert [tag(v) for v in got["values"][b]] == tags and got["counts"][b] == counts
            assert (got["n_values"][b], got["missing"][b], got["totals"][b]) == (len(tags), missing, total)
            assert sum(got["counts"][b]) + got["missing"][b] == got["totals"][b]
        cut = col.query_facets(q, key, Ds, limit=1, **filters)
        assert [v[:1] for v in got["values"]] == cut["values"] and cut["n_values"] == got["n_values"] and cut["totals"] == got["totals"]
    st = col.facet_stats
    assert st["queries"] == st["host"] == 16 and st["mfma"] == st["exact"] == 0


def test_the_copies_of_a_row_enter_together():
    col, emb, _ = make(delete=False)
    res = col.query_facets(emb[7:8], "nature", 1e-6, limit=5)
    assert res["totals"] == [9] and sum(res["counts"][0]) == 9                           # row 7 and rows 40..47
    vals = col.column_values("nature")
    cnt = Counter(vals[r] for r in [7] + list(range(40, 48)))
    assert dict(zip(res["values"][0], res["counts"][0])) == dict(cnt)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
class TwoDeviceEngine(OracleEngine):
    devices = [0, 1]


def test_refusals_and_their_messages():
    col, emb, _ = make()
    q = emb[:2]
    for key in ("", None, 3, b"nature"):
        for call in (lambda: col.facets(key), lambda: col.facets_device(key), lambda: col.query_facets(q, key, 0.3),
                     lambda: col.query_facets_device(q, key, 0.3)):
            with pytest.raises(ValueError, match="Expected key to be a non-empty str"):
                call()
    for limit in (0, -1, 1025, 2.0, True, "3"):
        with pytest.raises(ValueError, match=r"Expected limit to be an int in \[1, 1024\]"):
            col.facets("nature", limit=limit)
        with pytest.raises(ValueError, match=r"Expected limit to be an int in \[1, 1024\]"):
            col.query_facets(q, "nature", 0.3, limit=limit)
    with pytest.raises(ValueError, match=r"Expected limit to be an int in \[1, 1024\]"):
        col.query_facets(q, "nature", 0.3, limit=None)
    for bad in (float("nan"), [0.1, float("nan")]):
        with pytest.raises(ValueError, match="max_distance must not be NaN"):
            col.query_facets(q, "nature", bad)
    with pytest.raises(ValueError, match="one per query"):
        col.query_facets(q, "nature", [0.1, 0.2, 0.3])
    with pytest.raises(ValueError, match="does not match collection dimensionality"):
        col.query_facets(np.ones((1, DIM + 4), dtype=F32), "nature", 0.3)
    with pytest.raises(ValueError, match="query_embeddings"):
        col.query_facets(None, "nature", 0.3)
    with pytest.raises(ValueError):
        col.facets("nature", where={"i": {"$regex": "x"}})
    with pytest.raises(ValueError):
        col.count(where={"i": {"$regex": "x"}})
    for call in (lambda: col.facets_device("nature"), lambda: col.query_facets_device(q, "nature", 0.3)):
        with pytest.raises(NotImplementedError, match="no device-pointer search"):
            call()
    empty = Collection("e", engine_factory=oracle_factory)
    with pytest.raises(ValueError, match="facets_device: the collection is empty"):
        empty.facets_device("nature")
    with pytest.raises(ValueError, match="query_facets_device: the collection is empty"):
        empty.query_facets_device(q, "nature", 0.3)


@pytest.mark.parametrize("space", ["ip", "l2"])
def test_query_facets_refuses_the_other_spaces(space):
    col = Collection("s", metadata={"hnsw:space": space}, engine_factory=oracle_factory)
    for call in (lambda: col.query_facets(np.ones((1, DIM), F32), "k", 0.3), lambda: col.query_facets_device(np.ones((1, DIM), F32), "k", 0.3)):
        with pytest.raises(NotImplementedError, match="not available in the"):
            call()


def test_several_devices_count_on_the_host_and_refuse_query_facets():
    col = Collection("c", engine_factory=lambda dim, device: TwoDeviceEngine(dim, device))
    col.add(ids=["a", "b", "c"], embeddings=np.eye(3, 8, dtype=F32), metadatas=[{"k": "x"}, {"k": "y"}, {"k": "x"}])
    assert col.facets("k")["counts"] == [2, 1] and col.count(where={"k": "x"}) == 2
    with pytest.raises(NotImplementedError, match="one device"):
        col.query_facets(np.eye(1, 8, dtype=F32), "k", 0.3)


def test_the_bindings_are_declared():
    from rag_dpo_amd import _lib
    assert len(_lib.SYMBOLS["rdx_index_facet_count"][1]) == 8 and len(_lib.SYMBOLS["rdx_index_range_facets"][1]) == 15
    assert _lib.FACET_MAX_LIMIT == FC.MAX_LIMIT == 1024
    with open(os.path.join(ROOT, "include", "rdx.h")) as f:
        header = f.read()
    assert "#define RDX_FACET_MAX_LIMIT 1024" in header
    assert "int rdx_index_facet_count(rdx_index* h, const rdx_mask* mask, const int32_t* row_group, int64_t n_groups, int64_t* out_counts" in header
    assert "int rdx_index_range_facets(rdx_index* h, const float* queries, int64_t nq, const float* thresholds, const rdx_mask* mask" in header
    with open(os.path.join(ROOT, "rag_dpo_amd", "csrc", "facet_kernel.hpp")) as f:
        assert f"constexpr int FACET_MAX_LIMIT = {FC.MAX_LIMIT};" in f.read()
