"""GPU: Collection.query_groups / query_groups_device end to end against the definition evaluated from the ORACLE's ranking
(tests/groups_model.py), bit for bit, on corpora planted so that every rung of the ladder runs — which `group_stats` then shows —
and on one with enough groups (12 000) that their codes collide in k_group_select's position table, which the table's model shows
from the oracle's ranking before the GPU is asked."""
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


# ---- many groups: k_group_select's table past the codes that never collide (tests/test_group_table_model.py) ----------------------
def dense_codes(values, alive=None):
    """GroupTables' numbering restated: codes by first appearance in row order among the live rows that carry the key"""
    seen, out = {}, np.full(len(values), -1, dtype=np.int64)
    for i, v in enumerate(values):
        if v is not None and (alive is None or alive[i]):
            out[i] = seen.setdefault(GM.group_key(v), len(seen))
    return out


def colliding_pairs(codes, n_pairs, taken, must=()):
    """pairs of codes whose groups share a home slot in k_group_select's table, none of them in `taken`; `must` come first"""
    n_groups = int(codes.max()) + 1
    pairs = [p for p in must]
    for slot in range(1, GM.GROUP_TABLE):
        if len(pairs) == n_pairs:
            break
        free = [int(c) for c in GM.codes_with_home(slot, n_groups) if c not in taken]
        if len(free) >= 2:
            pairs.append((free[0], free[1]))
    assert len(pairs) == n_pairs and all(GM.home_slot(a) == GM.home_slot(b) and a != b for a, b in pairs)
    return pairs


class ManyGroups:
    """20 000 rows in about 12 000 groups of 1 - 3 rows scattered over the collection (every 50th row without the key), and three
    queries: next to query 0 lie the rows of four pairs of groups whose codes collide (0 and 4181 among them); next to query 1 lie
    300 rows of one group, so its first fetch is short and the second one lists thousands of codes; next to query 2 lie four pairs
    that collide under the numbering AFTER `gone` (every other of the best 8 rows of queries 0 and 1) is deleted. `keep` is a
    metadata flag three rows in four carry, the planted ones among them."""

    def __init__(self, O):
        n, rng = 20_000, np.random.default_rng(21)
        self.emb = emb = unit(rng, n)
        sizes = np.resize([1, 1, 2, 1, 2, 3], 12_000)
        assert sizes.sum() == n
        owner = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))
        self.values = values = [None if i % 50 == 49 else f"doc{owner[i]}" for i in range(n)]
        self.q = q = unit(rng, 3)
        big = rng.choice(n, 300, replace=False)
        for i in big:
            values[i] = "big"
        emb[big] = q[1] + 0.2 * unit(rng, 300)
        planted = np.zeros(n, dtype=bool)
        planted[big] = True

        def plant(codes, pairs, query):
            rows = np.flatnonzero(np.isin(codes, [c for p in pairs for c in p]))
            assert not planted[rows].any() and 2 * len(pairs) <= len(rows) <= 6 * len(pairs)
            emb[rows] = query + 0.3 * unit(rng, len(rows))
            planted[rows] = True

        best8 = lambda: sorted({int(r) for rows in O.cosine_topk(O.normalize_rows(emb), q[:2], 8)[1] for r in rows[::2]})   # noqa: E731
        self.codes0 = dense_codes(values)
        big_code = int(self.codes0[big[0]])
        self.pairs0 = colliding_pairs(self.codes0, 4, {big_code}, must=[(0, 4181)])
        assert big_code not in (0, 4181)
        plant(self.codes0, self.pairs0, q[0])
        gone = best8()
        self.alive = np.ones(n, dtype=bool)
        self.alive[gone] = False
        self.codes1 = dense_codes(values, self.alive)
        assert (self.codes1 != self.codes0).any()                                     # the deletes renumber the groups
        touched = set(self.codes1[planted & self.alive].tolist()) | set(self.codes1[np.isin(self.codes0, self.codes0[gone])].tolist())
        self.pairs1 = colliding_pairs(self.codes1, 4, touched)
        plant(self.codes1, self.pairs1, q[2])
        assert best8() == gone                                                        # (query 2's rows did not change what is deleted)
        self.gone = [f"id{r}" for r in gone]
        self.keep = planted | (rng.random(n) < 0.75)
        self.metas = [({"doc": v} if v is not None else {}) | {"keep": bool(self.keep[i])} for i, v in enumerate(values)]

    def collection(self):
        from rag_dpo_amd.groups import group_tables
        col = build(self.emb, self.metas)
        assert group_tables(col, "doc").row_group.tolist() == self.codes0.tolist()
        return col

    def displaced(self, O, codes, query, k, allow=None):
        """codes of the table's model that leave their home slot when k_group_select cuts the oracle's best k rows of `query`"""
        _, rows, counts = O.cosine_topk(O.normalize_rows(self.emb), self.q[query: query + 1], k, allow)
        assert counts[0] == k
        return GM.table_walk(codes[rows[0]])[0]


@pytest.fixture(scope="module")
def many(oracle):
    return ManyGroups(oracle)


def check_many(col, oracle, w, codes, pairs, query, allow=None, **filters):
    """both fetches on colliding codes — shown from the oracle's ranking before the GPU is asked — then the two answers' bits"""
    from rag_dpo_amd import groups as GR
    G, m = 64, 4
    assert GR.first_fetch_k(G, m) == 256 and GR.K_SECOND == GM.GROUP_MAX_K
    assert w.displaced(oracle, codes, query, 256, allow) >= len(pairs) == 4          # a pair shares a home slot: one of the two leaves it
    assert w.displaced(oracle, codes, 1, GR.K_SECOND, allow) > 0                     # the second fetch's list: thousands of codes
    for G_, m_ in ((G, m), (5, 3)):
        d = check(col, oracle, w.emb, w.q, w.values, G=G_, m=m_, allow=allow, **filters)
        assert d["queries"] == 3 and d["proven_first_fetch"] == 2 and d["second_fetch"] == 1 and d["brute"] == 0, (G_, m_, d)


def test_many_groups_collide_in_the_first_and_the_second_fetch(many, oracle):
    check_many(many.collection(), oracle, many, many.codes0, many.pairs0, 0)


def test_many_groups_after_deletes_and_under_a_device_filter(many, oracle):
    from rag_dpo_amd.groups import group_tables
    w = many
    col = w.collection()
    col.delete(ids=w.gone)                                                            # tombstones: the rows stay, the codes are renumbered
    assert col._n_dead == len(w.gone) and col._rows == len(w.values)
    assert group_tables(col, "doc").row_group.tolist() == w.codes1.tolist()
    check_many(col, oracle, w, w.codes1, w.pairs1, 2, allow=w.alive)
    col._WHERE_DEVICE_MIN_ROWS = 0                                                    # the predicate scan in HBM
    try:
        col._drop_masks()
        check_many(col, oracle, w, w.codes1, w.pairs1, 2, allow=w.alive & w.keep, where={"keep": True})
    finally:
        del col._WHERE_DEVICE_MIN_ROWS
        col._drop_masks()


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
