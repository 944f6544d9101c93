"""GPU: Collection.query_groups / query_groups_device end to end against the definition evaluated from the ORACLE's ranking
(tests/groups_model.py), bit for bit, on corpora planted so that every rung of the ladder runs — which `group_stats` then shows."""
import numpy as np
import pytest

from rag_dpo_amd.collection import Collection

import groups_model as GM

pytestmark = pytest.mark.gpu

DIM = 64


def unit(rng, n, dim=DIM):
    return rng.standard_normal((n, dim)).astype(np.float32)


def build(emb, metas, docs=None):
    col = Collection("groups", metadata={"hnsw:space": "cosine"})
    n = emb.shape[0]
    for a in range(0, n, 1000):
        col.add(ids=[f"id{i}" for i in range(a, min(n, a + 1000))], embeddings=emb[a:a + 1000], metadatas=metas[a:a + 1000],
                documents=None if docs is None else docs[a:a + 1000])
    return col


def moved(col, before):
    return {k: v - before[k] for k, v in col.group_stats.items()}


def check(col, oracle, emb, q, values, G=5, m=3, allow=None, **filters):
    """query_groups and query_groups_device against the definition; -> how the counters moved over the host-facing call"""
    import torch
    before = col.group_stats
    res = col.query_groups(q, "doc", n_groups=G, group_size=m, include=["distances"], **filters)
    delta = moved(col, before)
    want = GM.expected(oracle.normalize_rows(emb), q, values, G, m, allow)
    GM.same(GM.as_expected(res, col), want)
    dist, rows, counts, codes, found = col.query_groups_device(torch.from_numpy(q).cuda(), "doc", G, m, **filters)
    assert dist.shape == (len(q), G, m) and rows.dtype == torch.int64 and counts.dtype == codes.dtype == found.dtype == torch.int32
    dist, rows, counts, codes, found = (t.cpu().numpy() for t in (dist, rows, counts, codes, found))
    vals = col.group_values("doc", codes)
    for b, wq in enumerate(want):
        assert found[b] == len(wq)
        assert [(type(v), v) for v in vals[b][: len(wq)]] == [(type(v), v) for v, _, _, _ in wq] and all(v is None for v in vals[b][len(wq):])
        for g, (_, wr, _, wd) in enumerate(wq):
            assert counts[b, g] == len(wr) and rows[b, g, : len(wr)].tolist() == wr
            assert dist[b, g, : len(wr)].tobytes() == np.asarray(wd, dtype=np.float32).tobytes()
            assert (rows[b, g, len(wr):] == -1).all() and np.isposinf(dist[b, g, len(wr):]).all()
        assert (counts[b, len(wq):] == 0).all() and (codes[b, len(wq):] == -1).all() and (rows[b, len(wq):] == -1).all()
    return delta


def spread_world(n=2000, seed=0):
    """group sizes 1 .. 40, rows of a group scattered over the collection; every 50th row has no key"""
    rng = np.random.default_rng(seed)
    emb = unit(rng, n)
    emb[1500:1520] = emb[3]                                     # exact copies in several groups: ties by row id
    sizes, left = [], n
    while left > 0:
        sizes.append(min(left, 1 + len(sizes) % 40))
        left -= sizes[-1]
    owner = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))
    values = [None if i % 50 == 49 else f"doc{owner[i]}" for i in range(n)]
    metas = [({"doc": v} if v is not None else {}) | {"even": i % 2 == 0, "i": i} for i, v in enumerate(values)]
    docs = [f"row {i} {'alpha' if i % 3 == 0 else 'beta'}" for i in range(n)]
    return emb, values, metas, docs


@pytest.fixture(scope="module")
def spread():
    emb, values, metas, docs = spread_world()
    return build(emb, metas, docs), emb, values


@pytest.mark.parametrize("B", [1, 4, 65])
def test_spread_groups_are_proven_at_the_first_fetch(spread, oracle, B):
    col, emb, values = spread
    rng = np.random.default_rng(10 + B)
    q = unit(rng, B)
    q[0] = emb[3] + 0.05 * unit(rng, 1)[0]                      # next to the copies
    d = check(col, oracle, emb, q, values)
    assert d["queries"] == B and d["proven_first_fetch"] == B and d["second_fetch"] == 0 and d["brute"] == 0


@pytest.mark.parametrize("G,m", [(1, 1), (64, 16)])
def test_smallest_and_largest_answer(spread, oracle, G, m):
    col, emb, values = spread
    q = unit(np.random.default_rng(3), 2)
    check(col, oracle, emb, q, values, G=G, m=m)


def test_filters_on_the_host_and_on_the_device(spread, oracle):
    col, emb, values = spread
    n = len(values)
    q = unit(np.random.default_rng(4), 3)
    even = np.arange(n) % 2 == 0
    alpha = np.arange(n) % 3 == 0
    assert n < col._WHERE_DEVICE_MIN_ROWS
    check(col, oracle, emb, q, values, allow=even, where={"even": True})                      # below the threshold: the host's evaluator
    check(col, oracle, emb, q, values, allow=alpha, where_document={"$contains": "alpha"})
    check(col, oracle, emb, q, values, allow=even & alpha, where={"even": True}, where_document={"$contains": "alpha"})
    few = np.arange(n) < 40                                                                    # fewer allowed rows than k1: a list that is not full
    check(col, oracle, emb, q, values, allow=few, where={"i": {"$lt": 40}})
    col._WHERE_DEVICE_MIN_ROWS = 0                                                             # above it: the predicate scan in HBM
    try:
        col._drop_masks()
        check(col, oracle, emb, q, values, allow=~even, where={"even": False})
        check(col, oracle, emb, q, values, allow=np.arange(n) >= 1000, where={"i": {"$gte": 1000}})
    finally:
        del col._WHERE_DEVICE_MIN_ROWS
        col._drop_masks()


def test_second_fetch_when_one_group_owns_the_top(oracle):
    rng = np.random.default_rng(5)
    n = 2000
    emb = unit(rng, n)
    q = unit(rng, 2)
    big = rng.choice(n, 300, replace=False)
    emb[big] = q[0] + 0.2 * unit(rng, 300)                      # 300 rows next to query 0, all of one document
    values = [f"doc{i % 97}" for i in range(n)]
    for i in big:
        values[i] = "big"
    col = build(emb, [{"doc": v} for v in values])
    d = check(col, oracle, emb, q, values)
    assert d["second_fetch"] == 1 and d["proven_first_fetch"] == 1 and d["brute"] == 0


def test_brute_force_when_one_group_owns_more_than_the_second_fetch(oracle):
    rng = np.random.default_rng(6)
    n = 5000
    emb = unit(rng, n)
    q = unit(rng, 2)
    near = rng.choice(n, 4500, replace=False)
    emb[near] = q[1] + 0.05 * unit(rng, 4500)                   # 4 500 near-copies: longer than the second fetch and than one fill job
    values = [f"doc{i % 31}" for i in range(n)]
    for i in near:
        values[i] = "huge"
    col = build(emb, [{"doc": v} for v in values])
    d = check(col, oracle, emb, q, values)
    assert d["brute"] >= 1 and d["second_fetch"] >= d["brute"]   # (query 1 for certain; query 0 wherever the near-copies fall in its ranking)
    assert d["fill_jobs"] >= 31 + 2                              # every group once, the huge one in two spans
    d = check(col, oracle, emb, q, values, G=64, m=16)          # more groups asked for than exist
    assert d["brute"] >= 1


def test_fill_job_for_a_member_past_the_first_fetch(oracle):
    rng = np.random.default_rng(7)
    n = 2000
    emb = unit(rng, n)
    q = unit(rng, 1)
    emb[10] = q[0] + 0.01 * unit(rng, 1)[0]                     # the best row: document "pair" ...
    emb[1900] = -q[0]                                           # ... whose only other row is the worst of the collection
    values = [f"doc{i % 200}" for i in range(n)]
    values[10] = values[1900] = "pair"
    col = build(emb, [{"doc": v} for v in values])
    d = check(col, oracle, emb, q, values)
    assert d["fill_jobs"] >= 1 and d["second_fetch"] == 0 and d["brute"] == 0 and d["proven_first_fetch"] == 1
    res = col.query_groups(q, "doc", 5, 3)
    assert res["groups"][0][0] == "pair" and res["ids"][0][0] == ["id10", "id1900"]


def test_tombstones_and_key_updates(oracle):
    emb, values, metas, docs = spread_world(seed=8)
    col = build(emb, metas, docs)
    n = len(values)
    q = unit(np.random.default_rng(9), 3)
    best = col.query(q, n_results=8)["ids"]
    gone = sorted({i for ids in best for i in ids[::2]})         # delete every other of the best rows: tombstones, no compaction
    col.delete(ids=gone)
    assert col._n_dead == len(gone) and col._rows == n
    alive = np.ones(n, dtype=bool)
    alive[[int(s[2:]) for s in gone]] = False
    check(col, oracle, emb, q, values, allow=alive)
    keep = [i for ids in best for i in ids[1::2]][:6]            # move some of the remaining best rows into a new document
    col.update(ids=keep, metadatas=[{"doc": "moved"}] * len(keep))
    for s in keep:
        values[int(s[2:])] = "moved"
    d = check(col, oracle, emb, q, values, allow=alive)
    res = col.query_groups(q, "doc", 5, 3)
    assert any("moved" in g for g in res["groups"])
    col.update(ids=keep[:1], metadatas=[{"doc": 7}])             # a value of another kind is a group of its own
    values[int(keep[0][2:])] = 7
    check(col, oracle, emb, q, values, allow=alive)


def test_nobody_s_key_and_refusals(spread):
    import torch
    col, emb, _ = spread
    q = emb[:2]
    res = col.query_groups(q, "no_such_key")
    assert res["groups"] == [[], []] and res["ids"] == [[], []]
    dist, rows, counts, codes, found = col.query_groups_device(torch.from_numpy(q).cuda(), "no_such_key", 5, 3)
    assert found.tolist() == [0, 0] and (rows == -1).all() and torch.isinf(dist).all()
    with pytest.raises(ValueError):
        col.query_groups(q, "doc", n_groups=65)
    ip = Collection("ip", metadata={"hnsw:space": "ip"})
    ip.add(ids=["a"], embeddings=emb[:1], metadatas=[{"doc": "x"}])
    with pytest.raises(NotImplementedError):
        ip.query_groups(q, "doc")
