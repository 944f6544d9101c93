"""GPU: Collection.facets / facets_device / count(where=...) / query_facets / query_facets_device end to end on 2 000 rows against the
host path (the same collection on the test-only oracle engine: rag_dpo_amd/facets.py's model over the oracle's ranking), with `where`,
`where_document` and deletes, facet_stats, and a write between two calls (the tables and the masks are rebuilt, the counts move)."""
import numpy as np
import pytest

from rag_dpo_amd import facets as FC
from rag_dpo_amd import groups as GR
from rag_dpo_amd.collection import Collection

from oracle_engine import factory as oracle_factory

pytestmark = pytest.mark.gpu

DIM, N = 64, 2000
F32 = np.float32
GONE = [f"id{i}" for i in (3, 17, 501, 777, 1999)]
FILTERS = [{}, {"where": {"even": True}}, {"where_document": {"$contains": "alpha"}},
           {"where": {"i": {"$gte": 100}}, "where_document": {"$contains": "beta"}}, {"where": {"i": {"$lt": 0}}}]
IDS = ["all", "where", "doc", "both", "nothing"]


def fill(c, emb):
    metas = []
    for i in range(N):
        m = {"i": i, "even": i % 2 == 0, "nature": ["GUIDE", "DOCTRINE", "SANCTION", "GUIDE"][(i * 7) % 4], "doc": f"d{i // 9:03d}"}
        if i % 6:
            m["mixed"] = ["a", 1, True, 2.5, "b", 1.0][(i // 2) % 6]
        metas.append(m)
    c.add(ids=[f"id{i}" for i in range(N)], embeddings=emb, metadatas=metas,
          documents=[f"row {i} {'alpha' if i % 3 == 0 else 'beta'}" for i in range(N)])
    c.delete(ids=GONE)


@pytest.fixture()
def cols():
    rng = np.random.default_rng(3)
    centres = rng.standard_normal((8, DIM)).astype(np.float32)
    emb = (centres[rng.integers(0, 8, N)] + 0.4 * rng.standard_normal((N, DIM))).astype(np.float32)
    emb[500:510] = emb[17]                                                          # exact copies
    dev, host = Collection("facets"), Collection("facets-host", engine_factory=oracle_factory)
    fill(dev, emb)
    fill(host, emb)
    yield dev, host, emb, centres
    dev._drop_masks()


def tags(values):
    return [[(type(v).__name__, v) for v in row] for row in values]


@pytest.mark.parametrize("filters", FILTERS, ids=IDS)
def test_facets_and_count_equal_the_host_path(cols, filters):
    import torch
    dev, host, _, _ = cols
    for key in ("nature", "mixed", "doc", "nobody"):
        want = host.facets(key, **filters)
        got = dev.facets(key, **filters)
        assert got == want and tags([got["values"]]) == tags([want["values"]])
        for limit in (1, 3, 1024):
            assert dev.facets(key, limit=limit, **filters) == host.facets(key, limit=limit, **filters)
        counts, missing, total = dev.facets_device(key, **filters)
        assert counts.is_cuda and counts.dtype == torch.int64 and counts.shape == (GR.group_tables(dev, key).n_groups,)
        codes, cnt, n_values = FC.facet_order(counts.cpu().numpy())
        assert (missing, total, n_values) == (want["missing"], want["total"], want["n_values"]) and int(cnt.sum()) + missing == total
        assert tags([dev.group_values(key, codes)]) == tags([want["values"]]) and cnt.tolist() == want["counts"]
    assert dev.count(**filters) == host.count(**filters) == len(dev.get(include=[], **filters)["ids"])
    assert dev.count() == N - len(GONE)
    st = dev.facet_stats
    assert st["calls_host"] == 0 and st["calls"] == 4 * 5 + (1 if filters else 0)


@pytest.mark.parametrize("filters", FILTERS[:4], ids=IDS[:4])
def test_query_facets_equals_the_host_path(cols, filters):
    import torch
    dev, host, emb, centres = cols
    q = np.stack([emb[500], centres[2], emb[1500] + 0.05, centres[5] + 0.2]).astype(np.float32)
    for D in (1e-6, 0.3, [0.2, 0.5, 0.1, 0.7], 0.9, np.inf):                          # few rows, some, one per query, most, every allowed row
        for key, limit in (("nature", 10), ("mixed", 2), ("doc", 1024), ("nobody", 3)):
            want = host.query_facets(q, key, D, limit=limit, **filters)
            got = dev.query_facets(q, key, D, limit=limit, **filters)
            assert got == want and tags(got["values"]) == tags(want["values"])
            assert got["totals"] == dev.query_range(q, D, max_results=1, include=[], **filters)["totals"]
            codes, cnt, nv, mis, tot = dev.query_facets_device(torch.from_numpy(q).cuda(), key, D, limit, **filters)
            assert all(t.is_cuda for t in (codes, cnt, nv, mis, tot))
            assert (codes.dtype, cnt.dtype, nv.dtype, mis.dtype, tot.dtype) == (torch.int32, torch.int64, torch.int32, torch.int64, torch.int64)
            assert codes.shape == cnt.shape == (4, limit)
            assert nv.tolist() == want["n_values"] and mis.tolist() == want["missing"] and tot.tolist() == want["totals"]
            for b in range(4):
                n = len(want["values"][b])
                assert tags([dev.group_values(key, codes[b, :n])]) == tags([want["values"][b]]) and cnt[b, :n].tolist() == want["counts"][b]
                assert (codes[b, n:] == -1).all() and (cnt[b, n:] == 0).all()
    if not filters:
        got = dev.query_facets(q[:1], "nature", 1e-6)
        assert got["totals"] == [9]                                                  # the copies of row 17 (itself deleted): rows 500..509 without the deleted 501


def test_facet_stats_count_the_queries_by_path(cols):
    dev, host, emb, centres = cols
    q = np.stack([centres[1], centres[3], centres[4]]).astype(np.float32)
    assert dev.facet_stats == {"calls": 0, "calls_host": 0, "queries": 0, "mfma": 0, "exact": 0, "host": 0}
    dev.query_facets(q, "nature", 0.5)
    st = dev.facet_stats
    assert st["queries"] == 3 and st["mfma"] + st["exact"] == 3 and st["host"] == 0
    dev._engine.set_option("force_fast", 1)
    try:
        dev.query_facets(q, "nature", 0.5)
    finally:
        dev._engine.set_option("force_fast", 0)
    assert dev.facet_stats["mfma"] == st["mfma"] + 3 and dev.facet_stats["queries"] == 6
    host.query_facets(q, "nature", 0.5)
    host.facets("nature")
    assert host.facet_stats == {"calls": 1, "calls_host": 1, "queries": 3, "mfma": 0, "exact": 0, "host": 3}


def test_a_write_between_two_calls_moves_the_counts(cols):
    dev, host, emb, centres = cols
    q = emb[600:601]
    where = {"even": True}
    before = dev.facets("nature", where=where)
    qb = dev.query_facets(q, "nature", 0.6, where=where)
    assert before == host.facets("nature", where=where) and qb == host.query_facets(q, "nature", 0.6, where=where)
    for c in (dev, host):
        c.delete(ids=["id600"])
        c.update(ids=["id602"], metadatas=[{"nature": "NEW", "even": True}])
        c.add(ids=["new0", "new1"], embeddings=emb[600:602], metadatas=[{"i": N, "even": True, "nature": "NEW"}, {"i": N + 1, "even": False, "nature": "NEW"}],
              documents=["row new alpha", "row new beta"])
    after = dev.facets("nature", where=where)
    qa = dev.query_facets(q, "nature", 0.6, where=where)
    assert after == host.facets("nature", where=where) and qa == host.query_facets(q, "nature", 0.6, where=where)
    assert after["total"] == before["total"] and after["counts"][after["values"].index("NEW")] == 2   # one row gone, one added, one renamed
    assert "NEW" in qa["values"][0] and "NEW" not in qb["values"][0] and qa["totals"] != [0]
    assert dev.count(where=where) == host.count(where=where) == after["total"]
