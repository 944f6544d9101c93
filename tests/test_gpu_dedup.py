"""GPU: Collection.near_duplicates / near_duplicates_device end to end on 2 000 rows against the same calls on a collection over the
test-only oracle engine (the host path through the definition): plain, with `where` and `where_document`, after delete() of the
clusters' representatives and after update() (the resident mask and the stored rows must follow writes), with lists shorter than the
clusters (the dense pass), dedup_stats, and the too-loose refusal with the library's message."""
import numpy as np
import pytest

from rag_dpo_amd import dedup as DD
from rag_dpo_amd.collection import Collection

from oracle_engine import factory as oracle_factory

pytestmark = pytest.mark.gpu

DIM, N, DOCS = 64, 2000, 250
TIGHT, LOOSE = 0.004, 0.02                                                          # inside the documents' spread, and beyond it


def make_world():
    """250 documents of 8 near-duplicate chunks each (chunk = document + 5 % noise), stored interleaved; ten exact copies of row 17"""
    rng = np.random.default_rng(5)
    docs = rng.standard_normal((DOCS, DIM)).astype(np.float32)
    emb = (docs[np.arange(N) % DOCS] + 0.05 * rng.standard_normal((N, DIM))).astype(np.float32)
    emb[500:510] = emb[17]
    return emb


def fill(c, emb):
    c.add(ids=[f"id{i}" for i in range(N)], embeddings=emb, metadatas=[{"i": i, "even": i % 2 == 0} for i in range(N)],
          documents=[f"row {i} {'alpha' if i % 3 == 0 else 'beta'}" for i in range(N)])


@pytest.fixture()
def cols():
    emb = make_world()
    got = Collection("dedup", metadata={"hnsw:space": "cosine"})
    want = Collection("dedup_oracle", metadata={"hnsw:space": "cosine"}, engine_factory=oracle_factory)
    fill(got, emb)
    fill(want, emb)
    yield got, want, emb
    got._drop_masks()


def check(got, want, D, **kw):
    """the dict of the device collection against the oracle collection's, and the device variant's tensors against the dict"""
    import torch
    a = got.near_duplicates(D, **kw)
    b = want.near_duplicates(D, **{k: v for k, v in kw.items() if k in ("where", "where_document")})
    assert a == b, (D, kw)
    labels, totals = got.near_duplicates_device(D, **kw)
    assert labels.is_cuda and totals.is_cuda and labels.dtype == totals.dtype == torch.int64 and labels.shape == totals.shape == (got._rows,)
    labels, totals = labels.cpu().numpy(), totals.cpu().numpy()
    groups = DD.clusters_of(labels)
    assert got.ids_of(groups) == a["clusters"] and [[int(totals[r]) for r in g] for g in groups] == a["neighbors"]
    allowed = set(got.get(include=[], **{k: v for k, v in kw.items() if k in ("where", "where_document")})["ids"])
    assert {got._ids[r] for r in np.flatnonzero(labels >= 0)} == allowed and not totals[labels < 0].any()
    assert (labels[labels >= 0] <= np.flatnonzero(labels >= 0)).all()               # a label is the smallest row of its component
    return a


@pytest.mark.parametrize("filters", [{}, {"where": {"even": True}}, {"where_document": {"$contains": "alpha"}},
                                     {"where": {"i": {"$gte": 100}}, "where_document": {"$contains": "beta"}}], ids=["all", "where", "doc", "both"])
def test_near_duplicates_is_the_definition(cols, filters):
    got, want, emb = cols
    loose = check(got, want, LOOSE, **filters)
    tight = check(got, want, TIGHT, **filters)
    if not filters:
        assert len(loose["clusters"]) == DOCS and all(len(c) >= 7 for c in loose["clusters"])    # the documents' chunks
        assert any({"id17", "id500", "id509"} <= set(c) for c in tight["clusters"])
        assert sum(len(c) for c in tight["clusters"]) < N                            # the tighter distance leaves rows alone
    check(got, want, 0.0, **filters)                                                 # score 1.0 and nothing less
    assert check(got, want, LOOSE, max_neighbors=4, **filters) == loose              # lists shorter than the clusters: the dense pass
    st = got.dedup_stats
    assert st["listed"] > 0 and st["host"] == 0 and st["rows"] == st["listed"] + st["dense"]
    if "where_document" not in filters:                                             # (a document filter leaves clusters of two or three)
        assert st["dense"] > 0


def test_the_answer_follows_writes(cols):
    got, want, emb = cols
    first = check(got, want, LOOSE)
    reps = [c[0] for c in first["clusters"][:40]]
    for c in (got, want):
        c.delete(ids=reps)                                                          # the representatives go: the next row takes over
    after = check(got, want, LOOSE)
    assert [c[0] for c in after["clusters"][:3]] != reps[:3] and not set(reps) & {i for c in after["clusters"] for i in c}
    moved = [f"id{i}" for i in (100, 101, 102, 900)]
    for c in (got, want):
        c.update(ids=moved, embeddings=np.stack([emb[17]] * 4).astype(np.float32))  # rows join the copies of row 17
    last = check(got, want, TIGHT)
    assert any({"id100", "id101", "id102", "id900", "id500"} <= set(c) for c in last["clusters"])
    check(got, want, LOOSE, where={"even": True})


def test_a_distance_too_loose_is_refused_with_the_library_s_message(cols):
    got, want, emb = cols
    with pytest.raises(ValueError, match=r"list_cap = 8.*too loose for duplicate detection"):
        got.near_duplicates(2.5, max_neighbors=8, max_dense_rows=10)
    assert check(got, want, LOOSE)["clusters"]                                      # and the collection goes on answering
    st = got.dedup_stats
    assert st["calls"] == 3 and st["batches"] >= 2
