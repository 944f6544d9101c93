"""Collection.query_filtered on the CPU: one search with a filter per query, against the loop of query().

The engine is the oracle behind resident masks and a search_filtered that loops the oracle once per query; it counts the masks it
makes and closes and the searches it runs. A second engine has neither masks nor search_filtered (a host-only engine: the method
answers by one search per distinct filter). The fusion stage is driven with a fake collection on CPU tensors."""
import numpy as np
import pytest
import torch

from rag_dpo_amd import fusion
from rag_dpo_amd.collection import Collection

from oracle_engine import OracleEngine

DIM, ROWS, NQ = 32, 300, 23
RNG = np.random.default_rng(26)
EMB = RNG.standard_normal((ROWS, DIM)).astype(np.float32)
Q = RNG.standard_normal((NQ, DIM)).astype(np.float32)
IDS = [f"id{i}" for i in range(ROWS)]
METAS = [{"source": ("ENTREPRISE" if i % 3 == 0 else "PUBLIC"), "tag": f"t{i % 5}", "n": i} for i in range(ROWS)]
DOCS = [f"chunk {i} about {'pensions' if i % 4 == 0 else 'contracts'} and topic{i % 7}" for i in range(ROWS)]
INCLUDE = ["documents", "metadatas", "distances"]


def user_where(tags):
    """the reference's per-user filter (src/rag/pipeline.py:35-71): public rows, or the company's rows with one of the user's tags"""
    return {"$or": [{"source": {"$ne": "ENTREPRISE"}}] + [{"tag": t} for t in tags]}


class Mask:
    def __init__(self, eng, bits):
        self.eng, self.bits, self.closed = eng, np.array(bits, dtype=np.uint32), False
        eng.made += 1

    def close(self):
        if not self.closed:
            self.closed = True
            self.eng.closed += 1


class FilteredEngine(OracleEngine):
    """resident masks and a search_filtered that is the oracle, once per query, with that query's bitmap"""
    made = closed = searches = filtered_calls = 0
    last_masks = None

    def make_mask(self, bits):
        return Mask(self, bits)

    def search(self, q, k, allow_bits=None, mask=None):
        self.searches += 1
        assert mask is None or not mask.closed
        return super().search(q, k, mask.bits if mask is not None else allow_bits)

    def search_filtered(self, q, k, masks, query_filter):
        self.filtered_calls += 1
        self.last_masks, self.last_qf = list(masks), np.array(query_filter)
        assert all(not m.closed for m in masks) and len(set(map(id, masks))) == len(masks)
        q = np.ascontiguousarray(q, dtype=np.float32)
        parts = [OracleEngine.search(self, q[i:i + 1], k, None if f < 0 else masks[f].bits) for i, f in enumerate(query_filter)]
        return tuple(np.concatenate([p[j] for p in parts]) for j in range(3))


def make(engine=FilteredEngine, rows=ROWS, space="cosine"):
    col = Collection("c", metadata={"hnsw:space": space}, engine_factory=lambda dim, device=0: engine(dim, device))
    if rows:
        col.add(ids=IDS[:rows], embeddings=EMB[:rows], metadatas=METAS[:rows], documents=DOCS[:rows])
    return col


def loop(col, q, wheres, wds, k, include=INCLUDE):
    """the model: query() per query with that query's filters, joined into one result dict"""
    parts = [col.query(query_embeddings=q[i:i + 1], n_results=k, where=wheres[i], where_document=wds[i], include=include) for i in range(len(q))]
    out = dict(parts[0]) if parts else col.query(query_embeddings=q, n_results=k, include=include)
    for key in ("ids", "documents", "metadatas", "distances", "embeddings"):
        if parts and parts[0].get(key) is not None:
            out[key] = [p[key][0] for p in parts]
    return out


def mixed_wheres(nq):
    pool = [user_where(["t1"]), user_where(["t2", "t4"]), None, {"source": "ENTREPRISE"}, {}, {"n": {"$lt": 4}}, {"tag": "none"}]
    return [pool[i % len(pool)] for i in range(nq)]


@pytest.mark.parametrize("engine", [FilteredEngine, OracleEngine])
def test_mixed_filters_equal_the_loop_of_query(engine):
    col = make(engine)
    wheres, wds = mixed_wheres(NQ), [None] * NQ
    got = col.query_filtered(Q, wheres, n_results=7, include=INCLUDE)
    assert got == loop(col, Q, wheres, wds, 7)
    assert [len(x) for x in got["ids"]][:7] == [7, 7, 7, 7, 7, 4, 0]      # {"n": < 4}: fewer than k rows; an unknown tag: none
    if engine is FilteredEngine:
        assert col._engine.filtered_calls == 1
        assert len(col._engine.last_masks) == 5                           # None and {} filter nothing: index -1
        assert (col._engine.last_qf[[2, 4]] == -1).all()


def test_where_documents_and_tombstones():
    col = make()
    col.delete(ids=IDS[5:40:3])
    wheres = mixed_wheres(NQ)
    wds = [None, {"$contains": "pensions"}, {"$contains": "topic3"}, {}, {"$not_contains": "contracts"}] * 5
    wds = wds[:NQ]
    eng = col._engine
    eng.filtered_calls = 0
    got = col.query_filtered(Q, wheres, n_results=9, where_documents=wds, include=INCLUDE)
    assert eng.filtered_calls == 1
    assert got == loop(col, Q, wheres, wds, 9)
    dead = set(IDS[5:40:3])
    assert not dead & {i for ids in got["ids"] for i in ids}
    assert (eng.last_qf >= 0).all()                                        # with dead rows "no filter" is the alive mask, not -1
    none_filter = col.query_filtered(Q[:3], [None, None, None], n_results=5)
    assert len(eng.last_masks) == 1 and (eng.last_qf == 0).all()           # (None and {} have a cache key each, as in query())
    assert none_filter == loop(col, Q[:3], [None] * 3, [None] * 3, 5, include=None)


def test_repeated_filters_share_one_mask():
    col = make()
    eng = col._engine
    a, b = user_where(["t1", "t3"]), {"tag": "t2"}
    same_a = {"$or": list(a["$or"])}                                       # another object, the same canonical JSON
    made = eng.made
    got = col.query_filtered(Q[:8], [a, b, same_a, b, a, None, b, same_a], n_results=5)
    assert eng.made - made == 2 and len(eng.last_masks) == 2
    assert got == loop(col, Q[:8], [a, b, a, b, a, None, b, a], [None] * 8, 5, include=None)
    hits = col.mask_cache_hits
    col.query_filtered(Q[:8], [a, b, same_a, b, a, None, b, same_a], n_results=5)
    assert eng.made - made == 2 and col.mask_cache_hits == hits + 2        # the second call finds both in the cache


def test_more_distinct_filters_than_the_cache_holds():
    """40 distinct filters against a cache of 32: no mask the call uses is evicted while it runs (the engine asserts none is closed), the
    eight beyond the bound are made for the call and closed after it, and the 32 cached ones stay open"""
    col = make()
    eng = col._engine
    old = {"tag": "t0"}
    col.query(query_embeddings=Q[:1], n_results=3, where=old)              # an older entry: the call may evict it
    nq = 40
    q = np.tile(Q, (2, 1))[:nq]
    wheres = [{"n": {"$gte": 3 * i}} for i in range(nq)]
    made, closed = eng.made, eng.closed
    got = col.query_filtered(q, wheres, n_results=6, include=INCLUDE)
    assert len(eng.last_masks) == nq and eng.filtered_calls == 1
    assert all(not m.closed for m in eng.last_masks[:32]) and all(m.closed for m in eng.last_masks[32:])
    assert eng.made - made == nq and eng.closed - closed == 1 + 8          # the older entry was evicted, the eight were the call's own
    assert len(col._mask_cache) == Collection._MASK_CACHE_MAX
    assert got == loop(col, q, wheres, [None] * nq, 6)                     # (the loop's own masks evict and re-make freely)


def test_empty_collections():
    never = make(rows=0)
    assert never.query_filtered(Q[:2], [None, {"tag": "t1"}], n_results=3) == never.query(query_embeddings=Q[:2], n_results=3)
    col = make()
    col.delete(ids=IDS)
    got = col.query_filtered(Q[:3], [None, {"tag": "t1"}, {}], n_results=3, include=INCLUDE)
    assert got == loop(col, Q[:3], [None, {"tag": "t1"}, {}], [None] * 3, 3)
    assert got["ids"] == [[], [], []]


@pytest.mark.parametrize("wheres,wds,words", [
    ([None] * (NQ - 1), None, ("wheres", f"({NQ};", "length 22")),
    ({"tag": "t1"}, None, ("wheres", "dict")),
    (None, None, ("wheres", "NoneType")),
    ([None] * NQ, [None], ("where_documents", "length 1")),
    ([None] * NQ, {"$contains": "x"}, ("where_documents", "dict")),
])
def test_sequence_length_errors(wheres, wds, words):
    col = make()
    for call in (lambda: col.query_filtered(Q, wheres, n_results=3, where_documents=wds),
                 lambda: col.query_filtered_device(torch.from_numpy(Q), wheres, n_results=3, where_documents=wds)):
        with pytest.raises(ValueError) as e:
            call()
        assert "one entry per query" in str(e.value) and all(w in str(e.value) for w in words), str(e.value)


def test_refusals():
    col = make()
    ok = [None] * NQ
    with pytest.raises(ValueError, match="Number of requested results 0"):
        col.query_filtered(Q, ok, n_results=0)
    with pytest.raises(ValueError, match="Expected include item"):
        col.query_filtered(Q, ok, include=["scores"])
    with pytest.raises(ValueError, match="pass query_embeddings"):
        col.query_filtered(None, ok)
    with pytest.raises(ValueError, match="does not match collection dimensionality"):
        col.query_filtered(np.zeros((NQ, 8), np.float32), ok)
    with pytest.raises(ValueError):                                        # a `where` operator that does not exist, in one entry
        col.query_filtered(Q, [None] * (NQ - 1) + [{"tag": {"$like": "t"}}])
    with pytest.raises(ValueError):                                        # $regex stays refused
        col.query_filtered(Q, ok, where_documents=[{"$regex": "x"}] + [None] * (NQ - 1))
    for space in ("ip", "l2"):
        other = make(rows=0, space=space)
        for call in (lambda: other.query_filtered(Q, ok), lambda: other.query_filtered_device(torch.from_numpy(Q), ok)):
            with pytest.raises(NotImplementedError) as e:
                call()
            assert str(e.value) == f"query_filtered searches the cosine engine with a filter per query: not available in the {space!r} space"

    class TwoDevices(OracleEngine):
        devices = [0, 1]

    two = make(TwoDevices)
    with pytest.raises(NotImplementedError) as e:
        two.query_filtered(Q, ok)
    assert str(e.value) == "query_filtered runs on one device in this version: not on a collection spread over several"
    with pytest.raises(NotImplementedError, match="no device-pointer search"):     # a host-only engine has no *_device form
        make(OracleEngine).query_filtered_device(torch.from_numpy(Q), ok)
    with pytest.raises(ValueError, match="query_filtered_device: the collection is empty"):
        make(rows=0).query_filtered_device(torch.from_numpy(Q), ok)


# ---- the fusion stage ------------------------------------------------------------------------------------------------------------------
class FakeCollection:
    """query_device / query_filtered_device over a Collection on the oracle, with CPU tensors; counts the calls"""

    def __init__(self, with_filtered: bool):
        self.col, self.calls = make(), []
        if with_filtered:
            self.query_filtered_device = self._query_filtered_device

    def _pack(self, res, k):
        n = len(res["ids"])
        dist = torch.full((n, k), float("inf"))
        rows = torch.full((n, k), -1, dtype=torch.int64)
        cnt = torch.zeros(n, dtype=torch.int32)
        for i, (ids, ds) in enumerate(zip(res["ids"], res["distances"])):
            cnt[i] = len(ids)
            rows[i, :len(ids)] = torch.tensor(self.col.rows_of(ids), dtype=torch.int64)
            dist[i, :len(ids)] = torch.tensor(ds, dtype=torch.float32)
        return dist, rows, cnt

    def query_device(self, vectors, n_results=10, where=None, where_document=None):
        self.calls.append(("query_device", int(vectors.shape[0])))
        return self._pack(self.col.query(query_embeddings=vectors.numpy(), n_results=n_results, where=where, include=["distances"]), n_results)

    def _query_filtered_device(self, vectors, wheres, n_results=10, where_documents=None):
        self.calls.append(("query_filtered_device", int(vectors.shape[0])))
        return self._pack(self.col.query_filtered(vectors.numpy(), wheres, n_results=n_results, include=["distances"]), n_results)


def test_fusion_makes_one_filtered_call_with_the_loops_results():
    vectors = torch.from_numpy(Q[:12])
    a, b = user_where(["t1"]), user_where(["t2", "t3"])
    sub_wheres = [a, a, b, None, b, b, a, None, {"tag": "t4"}, a, b, None]
    new, old = FakeCollection(True), FakeCollection(False)
    got = fusion.dense_lists(new, vectors, sub_wheres, 50)
    want = fusion.dense_lists(old, vectors, sub_wheres, 50)
    assert new.calls == [("query_filtered_device", 12)]
    assert sorted(old.calls) == sorted([("query_device", 4), ("query_device", 4), ("query_device", 3), ("query_device", 1)])
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and torch.equal(g, w)
    # one distinct `where`, and none: the call that was always made
    for same in ([a] * 12, [None] * 12):
        new.calls.clear()
        got = fusion.dense_lists(new, vectors, same, 50)
        assert new.calls == [("query_device", 12)]
        for g, w in zip(got, fusion.dense_lists(old, vectors, same, 50)):
            assert torch.equal(g, w)
