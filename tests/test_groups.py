"""CPU: the grouped search's model, its tables and Collection.query_groups on the test-only oracle engine (the host path), all against
the definition stated as a literal double loop over the ORACLE's ranking (tests/groups_model.py). Comparisons are bit for bit."""
import numpy as np
import pytest

from rag_dpo_amd import groups as GR
from rag_dpo_amd import synth
from rag_dpo_amd.collection import Collection

import groups_model as GM
from oracle_engine import OracleEngine, factory as oracle_factory

DIM = 32


# ---- the model against the literal statement ----------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("G,m", [(1, 1), (5, 3), (64, 16)])
def test_model_matches_the_literal_definition(seed, G, m):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 400))
    n_codes = int(rng.integers(1, 90))
    row_group = rng.integers(-1, n_codes, size=n).astype(np.int32)            # -1: rows without the key
    scores = np.round(rng.standard_normal(n), 1).astype(np.float32)             # one decimal: many planted ties
    allowed = np.flatnonzero(rng.random(n) < 0.8)
    order = allowed[np.lexsort((allowed, -scores[allowed].astype(np.float64)))]  # score descending, row ascending
    rs, rr = scores[order], order.astype(np.int64)
    pad = int(rng.integers(0, 5))                                               # padding entries are skipped
    rs_p, rr_p = np.concatenate([rs, np.full(pad, -np.inf, np.float32)]), np.concatenate([rr, np.full(pad, -1, np.int64)])
    codes, members = GR.grouped_topk_model(rs_p, rr_p, row_group, G, m)
    keys = [None if c < 0 else int(c) for c in row_group]
    want = GM.literal_groups(rs, rr, keys, G, m)
    assert codes.tolist() == [k for k, _ in want]
    for (ms, mr), (_, mem) in zip(members, want):
        assert mr.tolist() == [r for _, r in mem]
        assert ms.tobytes() == np.asarray([s for s, _ in mem], dtype=np.float32).tobytes()


def test_model_empty_inputs():
    codes, members = GR.grouped_topk_model(np.zeros(0, np.float32), np.zeros(0, np.int64), np.zeros(0, np.int32), 3, 2)
    assert codes.size == 0 and members == []
    codes, members = GR.grouped_topk_model(np.ones(2, np.float32), np.array([0, 1]), np.array([-1, -1], np.int32), 3, 2)
    assert codes.size == 0 and members == []


# ---- GroupTables ---------------------------------------------------------------------------------------------------------------
def make(metas, dim=DIM, factory=oracle_factory, space="cosine"):
    col = Collection("c", metadata={"hnsw:space": space}, engine_factory=factory)
    n = len(metas)
    emb = synth.make_corpus(n, dim)
    col.add(ids=[f"id{i}" for i in range(n)], embeddings=emb, metadatas=metas, documents=[f"text {i} {'even' if i % 2 == 0 else 'odd'}" for i in range(n)])
    return col, emb


def check_tables(col, key):
    """codes by first appearance in row order, -1 without the key or deleted; the CSR lists every group's rows ascending"""
    t = GR.group_tables(col, key)
    n = col._rows
    seen, want_code, want_vals = {}, [], []
    for r in range(n):
        meta = col._meta_of(r) if col._alive[r] else None
        k = GM.group_key((meta or {}).get(key))
        if k is None:
            want_code.append(-1)
            continue
        if k not in seen:
            seen[k] = len(seen)
            want_vals.append(k[1])
        want_code.append(seen[k])
    assert t.row_group.dtype == np.int32 and t.row_group.tolist() == want_code
    assert [(type(v), v) for v in t.values] == [(type(v), v) for v in want_vals]
    assert t.group_off.dtype == np.int64 and t.group_rows.dtype == np.int64 and t.group_off.shape == (len(seen) + 1,)
    assert t.group_off[0] == 0 and t.group_off[-1] == t.group_rows.shape[0] == sum(c >= 0 for c in want_code)
    for c in range(len(seen)):
        assert t.group_rows[t.group_off[c]: t.group_off[c + 1]].tolist() == [r for r in range(n) if want_code[r] == c]
    return t


def test_tables_for_every_kind_of_value():
    vals = ["b", "a", 1, True, 1.0, 2, "a", None, False, 0.0, -0.0, 1, True, "b", 2.5, 1.0, None, 0]
    metas = [({"k": v} if v is not None else {"other": 1}) for v in vals]
    col, _ = make(metas)
    t = check_tables(col, "k")
    # 1, True and 1.0 are three groups; 0.0 and -0.0 one; False and 0 two
    assert [(type(v), v) for v in t.values] == [(str, "b"), (str, "a"), (int, 1), (bool, True), (float, 1.0), (int, 2), (bool, False),
                                                 (float, 0.0), (float, 2.5), (int, 0)]
    assert GR.group_tables(col, "k") is t                                       # cached until a write
    assert GR.group_tables(col, "nobody").n_groups == 0 and GR.group_tables(col, "nobody").group_off.tolist() == [0]


def test_tables_follow_update_and_delete():
    col, _ = make([{"k": f"g{i % 4}"} for i in range(20)])
    t0 = check_tables(col, "k")
    col.update(ids=["id0", "id5"], metadatas=[{"k": "new"}, {"k": 7}])          # row 0 opened group 0: the numbering moves
    t1 = check_tables(col, "k")
    assert t1 is not t0 and t1.values[0] == "new" and 7 in t1.values
    col.delete(ids=["id1", "id2", "id5"])                                       # tombstones: no compaction at this size
    assert col._n_dead == 3
    t2 = check_tables(col, "k")
    assert t2.row_group[[1, 2, 5]].tolist() == [-1, -1, -1] and 7 not in t2.values


# ---- query_groups on the oracle engine --------------------------------------------------------------------------------------------
def world(n=300):
    metas = []
    for i in range(n):
        meta = {"chunk_index": i, "nature": ["GUIDE", "DOCTRINE", "SANCTION"][i % 3]}
        if i % 11:
            meta["document_path"] = f"p{(i * 7) % 23}"                          # groups of ~12 rows; every 11th row has no key
        metas.append(meta)
    col, emb = make(metas)
    return col, emb, metas


def hat(col):
    return col._engine.rows                                                     # the stored (normalised) rows: what the oracle ranks


@pytest.mark.parametrize("G,m", [(1, 1), (5, 3), (64, 16)])
def test_query_groups_matches_the_definition(G, m):
    col, emb, metas = world()
    q = synth.make_queries(3, DIM, emb)
    res = col.query_groups(q.tolist(), "document_path", n_groups=G, group_size=m)
    want = GM.expected(hat(col), q, [mt.get("document_path") for mt in metas], G, m)
    GM.same(GM.as_expected(res, col), want)
    if G == 64:                                                                 # more groups asked for than there are: all 23 come back
        assert [len(g) for g in res["groups"]] == [23, 23, 23]
    assert res["included"] == ["metadatas", "documents", "distances"]
    for b in range(3):
        for g, ids in enumerate(res["ids"][b]):
            assert len(ids) <= m and len(res["documents"][b][g]) == len(ids) == len(res["metadatas"][b][g])
            assert all(mt["document_path"] == res["groups"][b][g] for mt in res["metadatas"][b][g])
    assert col.group_stats["queries"] == 3 and set(col.group_stats) == set(GR.STAT_KEYS)


def test_query_groups_with_where_and_where_document():
    col, emb, metas = world()
    q = synth.make_queries(2, DIM, emb)
    vals = [mt.get("document_path") for mt in metas]
    allow = np.array([mt["nature"] == "GUIDE" for mt in metas])
    res = col.query_groups(q, "document_path", 5, 3, where={"nature": "GUIDE"})
    GM.same(GM.as_expected(res, col), GM.expected(hat(col), q, vals, 5, 3, allow))
    odd = np.array([i % 2 == 1 for i in range(len(metas))])
    res = col.query_groups(q, "document_path", 5, 3, where_document={"$contains": "odd"})
    GM.same(GM.as_expected(res, col), GM.expected(hat(col), q, vals, 5, 3, odd))
    res = col.query_groups(q, "document_path", 5, 3, where={"nature": "GUIDE"}, where_document={"$contains": "odd"}, include=["distances"])
    GM.same(GM.as_expected(res, col), GM.expected(hat(col), q, vals, 5, 3, allow & odd))
    assert res["documents"] is None and res["metadatas"] is None
    col.delete(ids=[f"id{i}" for i in range(0, 60, 2)])                         # tombstones
    alive = np.array([not (i < 60 and i % 2 == 0) for i in range(len(metas))])
    res = col.query_groups(q, "document_path", 5, 3)
    GM.same(GM.as_expected(res, col), GM.expected(hat(col), q, vals, 5, 3, alive))


def test_query_groups_by_keys_of_other_kinds_and_nobody_s_key():
    col, emb, metas = world(120)
    q = synth.make_queries(2, DIM, emb)
    res = col.query_groups(q, "chunk_index", 4, 2)                              # every row its own (int) group
    GM.same(GM.as_expected(res, col), GM.expected(hat(col), q, [mt["chunk_index"] for mt in metas], 4, 2))
    assert all(len(ids) == 1 for ids in res["ids"][0])
    res = col.query_groups(q, "no_such_key", 4, 2)
    assert res["groups"] == [[], []] and res["ids"] == [[], []] and res["distances"] == [[], []]
    empty = Collection("e", engine_factory=oracle_factory)
    assert empty.query_groups([[0.0] * 8], "k")["ids"] == [[]]


def test_query_groups_validation():
    col, emb, _ = world(40)
    q = emb[:1]
    for bad in (dict(n_groups=0), dict(n_groups=65), dict(n_groups=True), dict(n_groups=2.0), dict(group_size=0), dict(group_size=17)):
        with pytest.raises(ValueError):
            col.query_groups(q, "document_path", **bad)
    for key in ("", None, 3):
        with pytest.raises(ValueError):
            col.query_groups(q, key)
    with pytest.raises(ValueError):
        col.query_groups(q, "document_path", include=["embeddings"])
    with pytest.raises(ValueError):
        col.query_groups(q, "document_path", where={"nature": {"$regex": "x"}})
    with pytest.raises(ValueError):
        col.query_groups(q, "document_path", where_document={"$regex": "x"})
    with pytest.raises(ValueError):
        col.query_groups(np.zeros((1, DIM + 4), np.float32), "document_path")
    with pytest.raises(NotImplementedError):                                    # the host path has no device output
        col.query_groups_device(q, "document_path", 5, 3)


class TwoDeviceEngine(OracleEngine):
    devices = [0, 1]


@pytest.mark.parametrize("space", ["ip", "l2"])
def test_query_groups_refuses_the_other_spaces(space):
    col = Collection("s", metadata={"hnsw:space": space}, engine_factory=oracle_factory)
    with pytest.raises(NotImplementedError):
        col.query_groups([[1.0] * 8], "k")
    with pytest.raises(NotImplementedError):
        col.query_groups_device(None, "k", 5, 3)


def test_query_groups_refuses_a_collection_on_several_devices():
    col, emb = make([{"k": "a"}] * 4, factory=lambda dim, device: TwoDeviceEngine(dim, device))
    with pytest.raises(NotImplementedError):
        col.query_groups(emb[:1], "k")
    with pytest.raises(NotImplementedError):
        col.query_groups_device(emb[:1], "k", 5, 3)
