"""CPU: what Collection's five queries refuse, and in which words (tests/oracle_engine.py's engines, no GPU).

query / query_device and the four derived families (query_groups, query_mmr, query_range, near_duplicates), the host-list and the
*_device form of each, crossed with every refusal the method can raise: REFUSALS pins the exception's type and its whole message, PAIRS
which of two broken rules is reported. The literals are what the commit before the stages were given one helper each raised; the file
passes on that commit and on every one after it. Then the empty-collection results key by key, and the mask cache's size, hits and keys.
One rule has changed since: a collection whose rows are all deleted answers as one nothing was ever added to, compacted or not, and
an empty collection refuses the `where` a populated one refuses (tests/history_model.py found both by replaying write histories).
"""
import numpy as np
import pytest
import torch

from rag_dpo_amd.collection import Collection

from oracle_engine import OracleEngine

DIM, ROWS = 64, 24
EMB = np.random.default_rng(7).standard_normal((ROWS, DIM)).astype(np.float32)
IDS = [f"id{i}" for i in range(ROWS)]
Q = EMB[:2].copy()                       # the host forms' queries
QT = torch.from_numpy(Q)                 # the *_device forms': a CPU tensor has the methods the refusals before the first launch use
Q32 = np.zeros((2, 32), np.float32)      # a wrong dimension
QT32 = torch.from_numpy(Q32)
NAN = float("nan")
REGEX = {"$regex": "x"}                  # a where_document operator that is refused
NOT_A_WHERE = {"g": {"$like": "a"}}      # a `where` operator that is refused
WHERE = {"g": "a"}


class DeviceEngine(OracleEngine):
    """an engine with a device-pointer search and resident masks; a call that reaches it was not refused"""
    def search_device(self, *a, **k):
        raise AssertionError("the call was not refused: it reached search_device")

    def make_mask(self, bits):
        return object()


class BitsEngine(OracleEngine):
    """a device-pointer search but no resident masks: a filter comes back as allow_bits"""
    search_device = DeviceEngine.search_device


class TwoDeviceEngine(OracleEngine):
    devices = [0, 1]


ENGINES = {"device": DeviceEngine, "bits": BitsEngine, "two": TwoDeviceEngine}
_made = {}


def make(kind: str) -> Collection:
    """plain: OracleEngine (no search_device, no make_mask); device / bits / two: the engines above; ip / l2: that space, nothing added;
    never: nothing was ever added (no engine); drained: every row added, deleted and compacted away (an engine of 0 rows);
    tombstoned: every row added and deleted, no compaction yet (an engine whose rows are all dead)"""
    if kind in _made:
        return _made[kind]
    eng = ENGINES.get(kind, OracleEngine)
    col = Collection("c", metadata={"hnsw:space": kind if kind in ("ip", "l2") else "cosine"},
                     engine_factory=lambda dim, device=0: eng(dim, device))
    if kind not in ("ip", "l2", "never"):
        col.add(ids=IDS, embeddings=EMB, metadatas=[{"g": "ab"[i % 2], "i": i} for i in range(ROWS)], documents=[f"doc {i}" for i in range(ROWS)])
    if kind == "drained":
        col.delete(ids=IDS)
        col._compact()
        assert col._engine is not None and col._rows == 0
    if kind == "tombstoned":
        col.delete(ids=IDS)
        assert col._rows == col._n_dead == ROWS
    _made[kind] = col
    return col


BASE = {
    "query": dict(query_embeddings=Q, n_results=3),
    "query_device": dict(query_embeddings=QT, n_results=3),
    "query_groups": dict(query_embeddings=Q, group_by="g", n_groups=2, group_size=2),
    "query_groups_device": dict(query_embeddings=QT, group_by="g", n_groups=2, group_size=2),
    "query_mmr": dict(query_embeddings=Q, n_results=3, fetch_k=6, lambda_mult=0.5),
    "query_mmr_device": dict(query_embeddings=QT, n_results=3, fetch_k=6, lambda_mult=0.5),
    "query_range": dict(query_embeddings=Q, max_distance=0.3, max_results=5),
    "query_range_device": dict(query_embeddings=QT, max_distance=0.3, max_results=5),
    "near_duplicates": dict(max_distance=0.1),
    "near_duplicates_device": dict(max_distance=0.1),
}


def call(method: str, kind: str, changes: dict):
    return getattr(make(kind), method)(**{**BASE[method], **changes})


def refused(method, kind, changes, exc, message):
    with pytest.raises(exc) as e:
        call(method, kind, changes)
    assert type(e.value) is exc and str(e.value) == message


V, N = ValueError, NotImplementedError
M_REGEX = "where_document operator $regex is not implemented (only $contains, $not_contains, $and, $or)"
M_CONTAINS = "Expected where_document operand of $contains to be a non-empty str, got 5"
M_NO_EMB = "this collection has no embedding function: pass query_embeddings="
M_DIM = "Embedding dimension 32 does not match collection dimensionality 64"
M_NO_SEARCH = "this collection's engine has no device-pointer search"
M_NAN = "max_distance must not be NaN"
M_WHERE = "Expected where operator to be one of ('$eq', '$ne', '$gt', '$gte', '$lt', '$lte', '$in', '$nin'), got $like"
INC3 = "Expected include item to be one of ['distances', 'documents', 'metadatas'], got "
INC4 = "Expected include item to be one of ['distances', 'documents', 'embeddings', 'metadatas'], got "


def bad_int(name, rng, values):
    return [(dict([(name, v)]), V, f"Expected {name} to be an int {rng}, got {v!r}") for v in values]


def bad_filters():
    return [(dict(where_document=REGEX), V, M_REGEX), (dict(where_document={"$contains": 5}), V, M_CONTAINS)]


def derived(method, how):
    """the refusals every derived family ends its argument check with: (collection, changes, exception, message)"""
    return [("ip", {}, N, f"{method} {how}: not available in the 'ip' space"), ("l2", {}, N, f"{method} {how}: not available in the 'l2' space"),
            ("two", {}, N, f"{method} runs on one device in this version: not on a collection spread over several")]


def device_only(method, bits_message):
    """what only a *_device form refuses: (collection, changes, exception, message)"""
    return [("never", {}, V, f"{method}: the collection is empty"), ("drained", {}, V, f"{method}: the collection is empty"),
            ("plain", {}, N, M_NO_SEARCH), ("bits", dict(where=WHERE), N, bits_message)]


def table(*families):
    """(family, rows for both forms, rows for the host form, rows for the *_device form); a row is (changes, exception, message), judged
    on the form's usual collection (host: plain, *_device: device), or (collection, changes, exception, message)"""
    out = []
    for fam, both, host, dev in families:
        for method, usual, rows in ((fam, "plain", both + host), (fam + "_device", "device", both + dev)):
            for i, row in enumerate(rows):
                kind, changes, exc, message = row if len(row) == 4 else (usual,) + row
                out.append(pytest.param(method, kind, changes, exc, message, id=f"{method}-{i}-{kind}"))
    return out


GROUP_COUNTS = bad_int("n_groups", "in [1, 64]", [0, 65, True, 2.0]) + bad_int("group_size", "in [1, 16]", [0, 17, True, 2.0]) \
    + [(dict(group_by=v), V, f"Expected group_by to be a non-empty str, got {v!r}") for v in ("", None, 3)]
MMR_COUNTS = bad_int("n_results", "in [1, 64]", [0, 1025, True, 2.0]) + bad_int("fetch_k", "in [1, 1024]", [0, 100000, True, 2.0]) \
    + [(dict(n_results=3, fetch_k=2), V, "Expected fetch_k >= n_results, got fetch_k=2, n_results=3")] \
    + [(dict(lambda_mult=v), V, f"Expected lambda_mult to be a number in [0, 1], got {v!r}") for v in (NAN, -0.1, 1.1, True, "0.5")]
RANGE_COUNTS = bad_int("max_results", "in [1, 1024]", [0, 100000, True, 2.0]) \
    + [(dict(max_distance=NAN), V, M_NAN), (dict(max_distance=[0.1, NAN]), V, M_NAN),
       (dict(max_distance=[0.1, 0.2, 0.3]), V, "Expected max_distance to be a number or one per query (2), got shape (3,)")]
DEDUP_COUNTS = bad_int("max_neighbors", "in [1, 1024]", [0, 1025, True, 2.0]) + bad_int("max_dense_rows", ">= 0", [-1, True, 2.0]) \
    + [("plain", dict(max_distance=NAN), V, M_NAN),
       ("plain", dict(max_distance=[0.1, 0.2]), TypeError, "float() argument must be a string or a real number, not 'list'")]

REFUSALS = table(
    ("query", bad_filters(),
     [(dict(include=["bogus"]), V, "Expected include item to be one of ['data', 'distances', 'documents', 'embeddings', 'metadatas', 'uris'], got bogus"),
      (dict(query_embeddings=None), V, M_NO_EMB + " (the reference always does, retriever.py:215-220)"),
      (dict(query_embeddings=Q32), V, M_DIM)]
     + [(dict(n_results=v), V, f"Number of requested results {v}, cannot be negative, or zero.") for v in (0, -1, True, 2.5)],
     device_only("query_device", "query_device needs an engine with resident masks")),
    ("query_groups", GROUP_COUNTS + bad_filters() + derived("query_groups", "ranks by the cosine score"),
     [(dict(include=[x]), V, INC3 + x) for x in ("embeddings", "uris", "data", "bogus")]
     + [(dict(query_embeddings=None), V, M_NO_EMB), (dict(query_embeddings=Q32), V, M_DIM),
        ("bits", dict(where=WHERE), N, "query_groups needs an engine with resident masks")],       # (the host form refuses it too)
     device_only("query_groups_device", "query_groups needs an engine with resident masks")),      # (and names itself without _device)
    ("query_mmr", MMR_COUNTS + bad_filters() + derived("query_mmr", "ranks and compares by the cosine score"),
     [(dict(include=[x]), V, INC4 + x) for x in ("uris", "data", "bogus")]
     + [(dict(query_embeddings=None), V, M_NO_EMB), (dict(query_embeddings=Q32), V, M_DIM)],
     device_only("query_mmr_device", "query_mmr_device needs an engine with resident masks")),     # (no dimension check of its own)
    ("query_range", RANGE_COUNTS + bad_filters() + derived("query_range", "cuts at a cosine distance"),
     [(dict(include=[x]), V, INC4 + x) for x in ("uris", "data", "bogus")]
     + [(dict(query_embeddings=None), V, M_NO_EMB), (dict(query_embeddings=Q32), V, M_DIM)],
     device_only("query_range_device", "query_range_device needs an engine with resident masks") + [(dict(query_embeddings=QT32), V, M_DIM)]),
    ("near_duplicates", DEDUP_COUNTS + bad_filters() + derived("near_duplicates", "cuts at a cosine distance"), [],
     device_only("near_duplicates_device", M_NO_SEARCH)),       # (an engine without resident masks is reported as one without the search)
)

# two rules broken at once: (method, collection, changes, the exception reported, its message)
PAIRS = [
    ("query_groups", "ip", dict(n_groups=0), V, "Expected n_groups to be an int in [1, 64], got 0"),                     # a count before the space
    ("query_mmr", "plain", dict(include=["uris"], n_results=0), V, INC4 + "uris"),                                       # include before a count
    ("query_mmr", "l2", dict(where_document=REGEX), V, M_REGEX),                                                         # where_document before the space
    ("query_mmr", "ip", dict(query_embeddings=None), N, "query_mmr ranks and compares by the cosine score: not available in the 'ip' space"),
    ("query_mmr", "two", dict(n_results=3, fetch_k=2), V, "Expected fetch_k >= n_results, got fetch_k=2, n_results=3"),  # a count before the devices
    ("query_mmr", "plain", dict(query_embeddings=Q32, where=NOT_A_WHERE), V, M_DIM),                                     # the dimension before `where`
    ("query_range", "plain", dict(query_embeddings=None, max_results=0), V, "Expected max_results to be an int in [1, 1024], got 0"),
    ("query_range", "plain", dict(query_embeddings=Q32, max_distance=NAN), V, M_NAN),                                    # the distance before the dimension
    ("query_range", "never", dict(max_distance=NAN), V, M_NAN),                                                          # ... and before the empty result
    ("query", "plain", dict(query_embeddings=None, n_results=0), V, M_NO_EMB + " (the reference always does, retriever.py:215-220)"),
    ("query", "plain", dict(where_document=REGEX, n_results=0), V, M_REGEX),
    ("query", "plain", dict(query_embeddings=[], n_results=0), V, "Number of requested results 0, cannot be negative, or zero."),
    ("query_device", "never", dict(where_document=REGEX), V, M_REGEX),                                                   # where_document before "empty"
    ("query_device", "plain", dict(where=NOT_A_WHERE), N, M_NO_SEARCH),                                                  # the engine before `where`
    ("query_mmr_device", "plain", dict(where=NOT_A_WHERE), N, M_NO_SEARCH),
    ("query_range_device", "never", dict(max_distance=NAN), V, "query_range_device: the collection is empty"),
    ("query_range_device", "plain", dict(query_embeddings=QT32), N, M_NO_SEARCH),                                        # the engine before the dimension
    ("query_range_device", "device", dict(query_embeddings=QT32, where=NOT_A_WHERE), V, M_DIM),                          # the dimension before `where`
    ("query_range_device", "bits", dict(max_distance=NAN, where=WHERE), V, M_NAN),                                       # the distance before the masks
    ("query_groups_device", "plain", dict(where=NOT_A_WHERE), V, M_WHERE),                                               # here `where` before the engine
    ("query_groups_device", "never", dict(n_groups=0), V, "Expected n_groups to be an int in [1, 64], got 0"),
    ("near_duplicates", "plain", dict(max_distance=NAN, max_neighbors=0), V, "Expected max_neighbors to be an int in [1, 1024], got 0"),
    ("near_duplicates_device", "plain", dict(max_distance=NAN), V, M_NAN),                                               # the distance before the engine
    ("near_duplicates_device", "plain", dict(where=NOT_A_WHERE), V, M_WHERE),                                            # and `where` before it too
    ("near_duplicates_device", "never", dict(max_distance=NAN), V, "near_duplicates_device: the collection is empty"),
]


@pytest.mark.parametrize("method,kind,changes,exc,message", REFUSALS)
def test_refusal(method, kind, changes, exc, message):
    refused(method, kind, changes, exc, message)


@pytest.mark.parametrize("method,kind,changes,exc,message", PAIRS, ids=[f"{r[0]}-{i}-{r[1]}" for i, r in enumerate(PAIRS)])
def test_which_of_two_refusals_is_reported(method, kind, changes, exc, message):
    refused(method, kind, changes, exc, message)


def test_the_table_is_as_long_as_it_was_written():
    assert len(REFUSALS) == 171 and len(PAIRS) == 25


# ---- what the host-list methods return for an empty collection, key by key -----------------------------------------------------------
D = ["metadatas", "documents", "distances"]      # the default include
E2 = [[], []]
EMPTY = {
    "query": {"ids": E2, "embeddings": None, "documents": E2, "metadatas": E2, "distances": E2, "uris": None, "data": None, "included": D},
    "query_groups": {"groups": E2, "ids": E2, "distances": E2, "documents": E2, "metadatas": E2, "included": D},
    "query_mmr": {"ids": E2, "mmr_scores": E2, "embeddings": None, "documents": E2, "metadatas": E2, "distances": E2, "uris": None, "data": None,
                  "included": D},
    "query_range": {"ids": E2, "totals": [0, 0], "embeddings": None, "documents": E2, "metadatas": E2, "distances": E2, "uris": None,
                    "data": None, "included": D},
    "near_duplicates": {"clusters": [], "neighbors": []},
}


@pytest.mark.parametrize("kind", ["never", "drained", "tombstoned"])
@pytest.mark.parametrize("method", sorted(EMPTY))
def test_empty_collection_results(method, kind):
    res = call(method, kind, {})
    assert res == EMPTY[method] and sorted(res) == sorted(EMPTY[method])
    if method == "near_duplicates":
        return
    lists = [v for v in res.values() if isinstance(v, list) and v and isinstance(v[0], list)]
    assert len({id(x) for v in lists for x in v}) == 2 * len(lists)                  # every per-query list is the caller's own
    assert call(method, kind, dict(query_embeddings=Q32)) == EMPTY[method]           # an empty collection has no dimension to miss
    only = call(method, kind, dict(include=["distances"]))
    assert only["included"] == ["distances"] and only["distances"] == E2 and only["documents"] is None and only["metadatas"] is None
    assert only["ids"] == E2


def test_empty_collection_embeddings():
    """include=["embeddings"]: query_mmr / query_range give a list per query; query() gives None. Rows that are all gone answer as a
    collection nothing was ever added to: what a caller sees does not depend on whether a compaction or a reload has taken them away"""
    for kind in ("never", "drained", "tombstoned"):
        for method in ("query_mmr", "query_range"):
            res = call(method, kind, dict(include=["embeddings"]))
            assert res["embeddings"] == E2 and res["distances"] is None
        assert call("query", kind, dict(include=["embeddings"]))["embeddings"] is None
        got = make(kind).get(include=["embeddings"])["embeddings"]
        assert (type(got), got.shape, got.dtype) == (np.ndarray, (0, 0), np.float32)


OTHERS = {
    "query_filtered": lambda c, w: c.query_filtered(Q, [None, w]),
    "query_facets": lambda c, w: c.query_facets(Q, "g", 0.3, where=w),
    "facets": lambda c, w: c.facets("g", where=w),
    "count": lambda c, w: c.count(where=w),
    "get": lambda c, w: c.get(where=w),
}


@pytest.mark.parametrize("kind", ["never", "drained", "tombstoned", "plain"])
@pytest.mark.parametrize("method", sorted(EMPTY) + sorted(OTHERS))
def test_an_empty_collection_refuses_the_where_a_populated_one_refuses(method, kind):
    with pytest.raises(ValueError) as e:
        if method in OTHERS:
            OTHERS[method](make(kind), NOT_A_WHERE)
        else:
            call(method, kind, dict(where=NOT_A_WHERE))
    assert str(e.value) == M_WHERE


@pytest.mark.parametrize("kind", ["never", "drained", "tombstoned"])
def test_kmeans_and_the_device_forms_call_a_collection_without_live_rows_empty(kind):
    col = make(kind)
    for method, args in (("kmeans", dict(init=EMB[:2])), ("assign_clusters", dict(centroids=EMB[:2])), ("kmeans_device", dict(init=EMB[:2])),
                         ("query_device", dict(query_embeddings=QT)), ("facets_device", dict(key="g"))):
        with pytest.raises(ValueError) as e:
            getattr(col, method)(**args)
        assert str(e.value) == f"{'kmeans' if method == 'assign_clusters' else method}: the collection is empty"
    assert col.count() == 0 and col.facets("g") == {"key": "g", "values": [], "counts": [], "n_values": 0, "missing": 0, "total": 0}


# ---- the mask cache: size, hits and keys -----------------------------------------------------------------------------------------------
class ResidentEngine(OracleEngine):
    """resident masks that count how often they are made and closed"""
    def __init__(self, dim, device=0):
        super().__init__(dim, device)
        self.made = self.closed = 0

    def make_mask(self, bits):
        eng = self
        eng.made += 1

        class Mask:
            words = np.array(bits)

            def close(self):
                eng.closed += 1
        return Mask()

    def search(self, q, k, allow_bits=None, mask=None):
        return super().search(q, k, mask.words if mask is not None else allow_bits)


@pytest.mark.parametrize("engine", [OracleEngine, ResidentEngine])
def test_mask_cache_size_hits_and_keys(engine):
    col = Collection("c", engine_factory=lambda dim, device=0: engine(dim, device))
    col.add(ids=IDS, embeddings=EMB, metadatas=[{"g": "ab"[i % 2], "i": i} for i in range(ROWS)], documents=[f"doc {i}" for i in range(ROWS)])
    resident = engine is ResidentEngine
    counts = lambda: (col._engine.made, col._engine.closed) if resident else None
    k_where, k_both = '{"g": "a"}', 'wd:[{"g": "a"}, {"$contains": "doc 1"}]'
    wd = {"$contains": "doc 1"}
    a = col.query(Q, 3, where=WHERE)                                                  # 1. a `where`
    assert list(col._mask_cache) == [k_where] and col.mask_cache_hits == 0
    b = col.query(Q, 3, where=WHERE, where_document=wd)                               # 2. the same `where` plus a where_document
    assert list(col._mask_cache) == [k_where, k_both] and col.mask_cache_hits == 0
    assert all(int(s[2:]) % 2 == 0 and s[2] == "1" for ids in b["ids"] for s in ids)  # (rows 10, 12 .. 18: group "a", "doc 1...")
    assert col.query(Q, 3, where=WHERE) == a and col.query(Q, 3, where=WHERE, where_document=wd) == b
    assert col.mask_cache_hits == 2 and len(col._mask_cache) == 2 and counts() in (None, (2, 0))
    for bits, res in col._mask_cache.values():
        assert (res is not None) == resident and isinstance(bits, np.ndarray) and bits.dtype == np.uint32 and bits.shape == (1,)
    col.update(ids=["id3"], documents=["changed"])                                    # 3. drops only the entries that read documents
    assert list(col._mask_cache) == [k_where] and col.mask_cache_hits == 2 and counts() in (None, (2, 1))
    col.update(ids=["no such id"], documents=["x"])                                   # (a write that changes nothing drops nothing)
    assert list(col._mask_cache) == [k_where]
    many = Collection._MASK_CACHE_MAX + 5
    for i in range(many):                                                             # 4. more distinct filters than the cache holds
        col.query(Q, 1, where={"i": {"$gte": i}})
    assert Collection._MASK_CACHE_MAX == 32 and len(col._mask_cache) == 32 and col.mask_cache_hits == 2
    assert list(col._mask_cache) == ['{"i": {"$gte": %d}}' % i for i in range(5, many)]       # the oldest went first
    assert counts() in (None, (2 + many, 1 + 6))
    col.query(Q, 1, where={"i": {"$gte": many - 1}})
    assert col.mask_cache_hits == 3
    col.update(ids=["id3"], metadatas=[{"i": 99}])                                    # any other write drops every entry
    assert col._mask_cache == {} and col.mask_cache_hits == 3 and counts() in (None, (2 + many, 2 + many))
    assert col.query(Q, 3) == col.query(Q, 3, where={}) and col._mask_cache == {}     # no filter, no tombstone: no entry
    col.delete(ids=["id0"])
    col.query(Q, 3)
    col.query(Q, 3, where={})
    assert list(col._mask_cache) == ["null", "{}"]                                    # tombstones are part of every bitmap
