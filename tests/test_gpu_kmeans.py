"""GPU: Collection.kmeans / kmeans_device / assign_clusters end to end on 2 000 rows against the same calls on a collection over the
test-only oracle engine (the host path through the definition): the dicts and the device tuples must be identical — plain, with `where`
and `where_document`, after delete() / update() / add() (the resident mask and the stored rows must follow writes), with given and
with sampled centroids, kmeans_stats, and the refusals."""
import numpy as np
import pytest

from rag_dpo_amd import kmeans as KM
from rag_dpo_amd.collection import Collection

from oracle_engine import factory as oracle_factory

pytestmark = pytest.mark.gpu

DIM, N, THEMES = 64, 2000, 8
FILTERS = [{}, {"where": {"even": True}}, {"where_document": {"$contains": "alpha"}},
           {"where": {"i": {"$gte": 100}}, "where_document": {"$contains": "beta"}}]


def make_world(n=N, seed=5):
    """eight themes with a 30 % spread, stored interleaved"""
    rng = np.random.default_rng(seed)
    themes = rng.standard_normal((THEMES, DIM)).astype(np.float32)
    return (themes[np.arange(n) % THEMES] + 0.3 * rng.standard_normal((n, DIM))).astype(np.float32)


def fill(c, emb, first=0):
    n = len(emb)
    c.add(ids=[f"id{i}" for i in range(first, first + n)], embeddings=emb, metadatas=[{"i": i, "even": i % 2 == 0} for i in range(first, first + n)],
          documents=[f"row {i} {'alpha' if i % 3 == 0 else 'beta'}" for i in range(first, first + n)])


@pytest.fixture()
def cols():
    emb = make_world()
    got = Collection("kmeans", metadata={"hnsw:space": "cosine"})
    want = Collection("kmeans_oracle", metadata={"hnsw:space": "cosine"}, engine_factory=oracle_factory)
    fill(got, emb)
    fill(want, emb)
    yield got, want, emb
    got._drop_masks()


def same_dict(a, b, what):
    assert a.keys() == b.keys() == {"centroids", "clusters", "distances", "counts", "n_iter", "converged"}, what
    assert a["centroids"].dtype == b["centroids"].dtype == np.float32 and a["centroids"].shape == b["centroids"].shape, what
    assert a["centroids"].tobytes() == b["centroids"].tobytes(), (what, "centroids")
    for k in ("n_iter", "converged", "counts", "clusters", "distances"):
        assert a[k] == b[k], (what, k)


def check(got, want, what="", **kw):
    """the dict of the device collection against the oracle collection's, and the device variant's tensors against the dict"""
    import torch
    a = got.kmeans(**kw)
    same_dict(a, want.kmeans(**kw), (what, kw.keys()))
    labels, scores, cen, counts, n_iter, conv = got.kmeans_device(**kw)
    assert labels.is_cuda and scores.is_cuda and cen.is_cuda and counts.is_cuda
    assert (labels.dtype, scores.dtype, cen.dtype, counts.dtype) == (torch.int64, torch.float32, torch.float32, torch.int64)
    assert labels.shape == scores.shape == (got._rows,) and counts.shape == (cen.shape[0],) and cen.shape[1] == DIM
    labels, scores = labels.cpu().numpy(), scores.cpu().numpy()
    assert cen.cpu().numpy().tobytes() == a["centroids"].tobytes() and counts.cpu().tolist() == a["counts"] and (n_iter, conv) == (a["n_iter"], a["converged"])
    groups = KM.clusters_of(labels, cen.shape[0])
    assert got.ids_of(groups) == a["clusters"]
    assert [[float(np.float32(1.0) - scores[r]) for r in g] for g in groups] == a["distances"]
    filt = {k: v for k, v in kw.items() if k in ("where", "where_document")}
    allowed = set(got.get(include=[], **filt)["ids"])
    assert {got._ids[r] for r in np.flatnonzero(labels >= 0)} == allowed and np.isneginf(scores[labels < 0]).all()
    return a


@pytest.mark.parametrize("filters", FILTERS, ids=["all", "where", "doc", "both"])
def test_kmeans_is_the_definition(cols, filters):
    got, want, emb = cols
    a = check(got, want, "sampled", n_clusters=THEMES, seed=1, **filters)
    assert sum(a["counts"]) == len(got.get(include=[], **filters)["ids"]) and a["n_iter"] >= 1
    check(got, want, "one update", n_clusters=5, seed=2, max_iter=1, **filters)
    rng = np.random.default_rng(3)
    init = rng.standard_normal((THEMES, DIM)).astype(np.float32)
    b = check(got, want, "given", init=init, max_iter=30, **filters)
    assert b["converged"]
    same_dict(got.assign_clusters(b["centroids"], **filters), want.assign_clusters(b["centroids"], **filters), "assign")
    again = got.assign_clusters(b["centroids"], **filters)
    assert again["clusters"] == b["clusters"] and again["distances"] == b["distances"] and again["n_iter"] == 0
    st = got.kmeans_stats
    assert st["host"] == 0 and st["calls"] == 8 and st["iterations"] == 2 * (a["n_iter"] + 1 + b["n_iter"]) and want.kmeans_stats["host"] == 4


def test_init_on_the_device_and_the_seed(cols):
    import torch
    got, want, emb = cols
    init = np.random.default_rng(4).standard_normal((6, DIM)).astype(np.float32)
    a = got.kmeans(init=init)
    same_dict(got.kmeans(init=torch.from_numpy(init).cuda()), a, "device init")
    out = got.kmeans_device(init=torch.from_numpy(init).cuda(), n_clusters=6)
    assert out[2].cpu().numpy().tobytes() == a["centroids"].tobytes()
    same_dict(got.kmeans(6, seed=9), got.kmeans(6, seed=9), "seed")
    assert got.kmeans(6, seed=9)["clusters"] != got.kmeans(6, seed=10)["clusters"]


def test_the_answer_follows_writes(cols):
    got, want, emb = cols
    first = check(got, want, "before", n_clusters=THEMES, seed=1)
    gone = [c[0] for c in first["clusters"] if c] + [f"id{i}" for i in range(300, 340)]
    for c in (got, want):
        c.delete(ids=gone)
    after = check(got, want, "after delete", n_clusters=THEMES, seed=1)
    assert not set(gone) & {i for c in after["clusters"] for i in c} and sum(after["counts"]) == N - len(gone)
    moved = [f"id{i}" for i in (100, 101, 102, 900)]
    for c in (got, want):
        c.update(ids=moved, embeddings=np.stack([emb[17]] * 4).astype(np.float32))
    check(got, want, "after update", n_clusters=THEMES, seed=1)
    more = make_world(300, seed=6)
    for c in (got, want):
        fill(c, more, first=N)
    last = check(got, want, "after add", n_clusters=THEMES, seed=1, where={"even": True})
    assert any(int(i[2:]) >= N for c in last["clusters"] for i in c)


def test_refusals(cols):
    import torch
    got, want, emb = cols
    good = torch.eye(3, DIM, device="cuda")
    nan = good.clone()
    nan[1, 1] = float("nan")
    for bad in (dict(), dict(n_clusters=0), dict(n_clusters=4097), dict(n_clusters=N + 1), dict(n_clusters=3, max_iter=1001), dict(init=nan),
                dict(init=torch.eye(3, DIM + 4, device="cuda")), dict(init=good, n_clusters=4), dict(n_clusters=1001, where={"even": True}),
                dict(n_clusters=3, where_document={"$regex": "x"})):
        with pytest.raises(ValueError):
            got.kmeans(**bad)
        with pytest.raises(ValueError):
            got.kmeans_device(**bad)
    assert got.kmeans_stats == {"calls": 0, "rows": 0, "iterations": 0, "host": 0}
    assert got.kmeans(3)["counts"] and got.kmeans_stats["calls"] == 1 and got.kmeans_stats["rows"] == N   # and the collection goes on answering
