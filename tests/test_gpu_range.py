"""GPU: Collection.query_range / query_range_device end to end on 2 000 rows against query() on the same collection — the entries of
query(n_results = m) within the distance, totals from query(n_results = count()) — with `where` and `where_document`, after update()
and after delete() (the resident mask must follow writes), range_stats, and the refusals."""
import numpy as np
import pytest

from rag_dpo_amd.collection import Collection

pytestmark = pytest.mark.gpu

DIM, N = 64, 2000
F32 = np.float32


def make_world():
    rng = np.random.default_rng(3)
    centres = rng.standard_normal((8, DIM)).astype(np.float32)
    emb = (centres[rng.integers(0, 8, N)] + 0.4 * rng.standard_normal((N, DIM))).astype(np.float32)
    emb[500:510] = emb[17]                                                          # exact copies
    return emb, centres


@pytest.fixture()
def col():
    emb, centres = make_world()
    c = Collection("range", metadata={"hnsw:space": "cosine"})
    c.add(ids=[f"id{i}" for i in range(N)], embeddings=emb, metadatas=[{"i": i, "even": i % 2 == 0} for i in range(N)],
          documents=[f"row {i} {'alpha' if i % 3 == 0 else 'beta'}" for i in range(N)])
    yield c, emb, centres
    c._drop_masks()


def cut(dists, D):
    n = sum(1 for d in dists if d <= D)
    assert all(d <= D for d in dists[:n])
    return n


def check(c, q, D, m, **filters):
    """query_range and query_range_device against the cut of query() -> totals"""
    import torch
    nq = len(q)
    Ds = np.broadcast_to(np.asarray(D, dtype=np.float64), (nq,))
    top = c.query(q, n_results=m, **filters)
    full = [c.query(q[b:b + 1], n_results=min(c.count(), 4096), include=["distances"], **filters) for b in range(nq)]
    got = c.query_range(q, D, max_results=m, **filters)
    dist, rows, counts, totals = c.query_range_device(torch.from_numpy(q).cuda(), D, m, **filters)
    assert dist.shape == rows.shape == (nq, m) and counts.shape == totals.shape == (nq,)
    assert (dist.dtype, rows.dtype, counts.dtype, totals.dtype) == (torch.float32, torch.int64, torch.int32, torch.int64)
    assert all(t.is_cuda for t in (dist, rows, counts, totals))
    dist, rows, counts, totals = (t.cpu().numpy() for t in (dist, rows, counts, totals))
    for b in range(nq):
        n = cut(top["distances"][b], Ds[b])
        assert got["ids"][b] == top["ids"][b][:n] and got["distances"][b] == top["distances"][b][:n]
        assert got["documents"][b] == top["documents"][b][:n] and got["metadatas"][b] == top["metadatas"][b][:n]
        want_total = cut(full[b]["distances"][0], Ds[b])
        assert want_total < 4096 or c.count() <= 4096                               # (query() lists at most 4 096 rows)
        assert got["totals"][b] == want_total == int(totals[b])
        assert counts[b] == n and c.ids_of([rows[b, :n].tolist()])[0] == top["ids"][b][:n]
        assert dist[b, :n].tobytes() == np.asarray(top["distances"][b][:n], dtype=np.float32).tobytes()
        assert (rows[b, n:] == -1).all() and np.isposinf(dist[b, n:]).all()
    return got["totals"]


def thresholds(c, q, **filters):
    """per query, distances that cut its ranking at telling places: none, the best row (and its ties), 7 rows, 30, every row"""
    out = []
    for b in range(len(q)):
        d = c.query(q[b:b + 1], n_results=60, include=["distances"], **filters)["distances"][0]
        out.append([float(np.nextafter(F32(d[0]), F32(-np.inf))), d[0], d[6], (d[29] + d[30]) / 2, 2.5])
    return out


@pytest.mark.parametrize("filters", [{}, {"where": {"even": True}}, {"where_document": {"$contains": "alpha"}},
                                     {"where": {"i": {"$gte": 100}}, "where_document": {"$contains": "beta"}}], ids=["all", "where", "doc", "both"])
def test_query_range_is_the_cut_of_query(col, filters):
    c, emb, centres = col
    q = np.stack([emb[17], centres[2], emb[1500] + 0.05, centres[5] + 0.2]).astype(np.float32)
    th = thresholds(c, q, **filters)
    for j in range(5):
        totals = check(c, q, [th[b][j] for b in range(4)], 10, **filters)
        if j == 0:
            assert totals == [0, 0, 0, 0]
        if j == 4:
            assert totals == [len(c.get(include=[], **filters)["ids"])] * 4
    check(c, q, [th[0][1], th[1][0], th[2][3], th[3][4]], 40, **filters)             # a different distance per query, m above the cut and below
    check(c, q[:1], 0.3, 100, **filters)                                            # the reference's cut, one query
    if not filters:
        got = c.query_range(q[:1], th[0][1], 100)
        assert got["ids"][0] == ["id17"] + [f"id{i}" for i in range(500, 510)] and got["totals"] == [11]


def test_the_mask_follows_writes(col):
    c, emb, centres = col
    q = np.stack([centres[1], emb[17]]).astype(np.float32)
    f = {"where": {"even": True}}
    before = check(c, q, 0.5, 20, **f)
    best = c.query(q, n_results=8, **f)["ids"]
    moved = sorted({i for ids in best for i in ids[::2]})
    away = -(centres[1] / np.linalg.norm(centres[1]) + emb[17] / np.linalg.norm(emb[17]))       # far from both queries
    c.update(ids=moved, embeddings=np.stack([away] * len(moved)).astype(np.float32))            # rows leave the range ...
    after = check(c, q, 0.5, 20, **f)
    assert all(a < b for a, b in zip(after, before))
    c.update(ids=["id3", "id5"], embeddings=np.stack([centres[1]] * 2).astype(np.float32), metadatas=[{"i": 3, "even": True}, {"i": 5, "even": True}])
    assert check(c, q, 0.5, 20, **f)[0] == after[0] + 2                             # ... and rows enter it, by embedding and by metadata
    gone = c.query(q, n_results=6, **f)["ids"][0][:4]
    c.delete(ids=gone)
    assert check(c, q, 0.5, 20, **f)[0] == after[0] + 2 - 4
    check(c, q, 0.5, 20)
    check(c, q, 2.5, 20, where_document={"$contains": "alpha"})


def test_range_stats_count_queries_by_path(col):
    c, emb, centres = col
    assert c.range_stats == {"queries": 0, "mfma": 0, "exact": 0, "host": 0}
    q = np.tile(centres[:1], (70, 1)).astype(np.float32)
    c.query_range(q[:2], 0.4, 10)                                                   # a small problem: the exact scan
    assert c.range_stats == {"queries": 2, "mfma": 0, "exact": 2, "host": 0}
    c.query_range(q, 0.4, 10)                                                       # 70 queries on 2 000 rows: the MFMA path
    assert c.range_stats == {"queries": 72, "mfma": 70, "exact": 2, "host": 0}
    import torch
    c.query_range_device(torch.from_numpy(q).cuda(), 0.4, 10)
    assert c.range_stats == {"queries": 142, "mfma": 140, "exact": 2, "host": 0}


@pytest.mark.parametrize("space", ["ip", "l2"])
def test_other_spaces_are_refused(space):
    import torch
    c = Collection("s", metadata={"hnsw:space": space})
    c.add(ids=["a", "b"], embeddings=np.eye(2, 8, dtype=np.float32))
    with pytest.raises(NotImplementedError):
        c.query_range(np.ones((1, 8), np.float32), 0.3)
    with pytest.raises(NotImplementedError):
        c.query_range_device(torch.ones((1, 8)).cuda(), 0.3)
    c._drop_masks()


def test_bad_arguments_are_refused_before_anything_runs(col):
    import torch
    c, emb, centres = col
    q = torch.from_numpy(centres[:2]).cuda()
    for bad in (dict(max_distance=float("nan")), dict(max_distance=[0.1, 0.2, 0.3]), dict(max_distance=0.3, max_results=0),
                dict(max_distance=0.3, max_results=1025)):
        with pytest.raises(ValueError):
            c.query_range_device(q, **bad)
        with pytest.raises(ValueError):
            c.query_range(centres[:2], **bad)
    with pytest.raises(ValueError):
        c.query_range_device(torch.zeros((1, DIM + 4)).cuda(), 0.3)
    assert c.range_stats["queries"] == 0
