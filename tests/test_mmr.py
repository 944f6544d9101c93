"""CPU: the diversity-aware search's numpy model (rag_dpo_amd/mmr.py) and Collection.query_mmr on the test-only oracle engine (the host
path), against the definition stated as a literal double loop over the ORACLE's exact scores (tests/mmr_model.py). Bit for bit."""
import numpy as np
import pytest

from rag_dpo_amd import mmr as MM
from rag_dpo_amd import synth
from rag_dpo_amd.collection import Collection

import mmr_model as LM
from oracle_engine import OracleEngine, factory as oracle_factory

DIM = 64


# ---- pair_scores against the oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [4, 60, 252, 256, 260, 1024, 1028])
def test_pair_scores_are_the_oracle_s_bits_and_symmetric(dim, oracle):
    rng = np.random.default_rng(dim)
    x = rng.standard_normal((40, dim)).astype(np.float32) * np.exp(rng.standard_normal((40, 1))).astype(np.float32)
    x[5] = 0.0                                                                    # a zero row
    x[6] = x[7]                                                                   # two identical rows
    hat = oracle.normalize_rows(x)
    for j in (0, 5, 6, 39):
        got = MM.pair_scores(hat, hat[j])
        assert got.dtype == np.float32 and got.tobytes() == oracle.scores(hat, hat[j]).tobytes(), (dim, j)
    full = np.stack([MM.pair_scores(hat, hat[j]) for j in range(40)])
    assert full.tobytes() == full.T.copy().tobytes()                              # p(i, j) == p(j, i), bit for bit
    with pytest.raises(ValueError):
        MM.pair_scores(hat, hat[0][:-4])


# ---- the model against the literal statement -------------------------------------------------------------------------------------
def check_model(scores, rows, hat, k, lam):
    pos, r, s, v = MM.mmr_model(scores, rows, hat[np.maximum(rows, 0)], k, lam)
    want = LM.literal_mmr(scores, rows, hat, k, lam)
    assert pos.dtype == np.int32 and r.dtype == np.int64 and s.dtype == np.float32 and v.dtype == np.float64
    assert pos.tolist() == [w[0] for w in want]
    assert r.tolist() == [w[1] for w in want]
    assert s.tobytes() == np.asarray([w[2] for w in want], dtype=np.float32).tobytes()
    assert v.tobytes() == np.asarray([w[3] for w in want], dtype=np.float64).tobytes()
    return pos


@pytest.mark.parametrize("seed", range(5))
@pytest.mark.parametrize("lam", [0.0, 0.3, 0.5, 1.0])
def test_model_matches_the_literal_definition_on_random_lists(seed, lam, oracle):
    rng = np.random.default_rng(seed)
    dim = int(rng.choice([4, 60, 256, 260]))
    n_rows = int(rng.integers(3, 120))
    x = rng.standard_normal((n_rows, dim)).astype(np.float32)
    x[n_rows // 2] = x[0]                                                         # an exact copy
    hat = oracle.normalize_rows(x)
    n = int(rng.integers(1, n_rows + 1))
    rows = rng.permutation(n_rows)[:n].astype(np.int64)
    scores = np.round(rng.standard_normal(n), 1).astype(np.float32)               # not sorted, many equal: the list is taken as it is
    rows[rng.random(n) < 0.1] = -1                                                # padding inside the list
    for k in (1, 5, n, 64):
        check_model(scores, rows, hat, k, lam)


@pytest.mark.parametrize("lam", [0.0, 0.5, 0.9, 1.0])
def test_model_on_the_planted_world(lam, oracle):
    emb, cluster, centres = LM.planted_world(n_clusters=12, paragraphs=2, copies=4, dim=DIM, seed=1)
    emb[3] = emb[2]                                                               # exact duplicates inside the world
    hat = oracle.normalize_rows(emb)
    s, r, c = oracle.cosine_topk(hat, centres[:3], 50)
    for b in range(3):
        pos = check_model(s[b], r[b], hat, 10, lam)
        if lam == 1.0:
            assert pos.tolist() == list(range(10))                                # no diversity asked for: the ranking itself


def test_model_edges():
    hat = np.eye(4, dtype=np.float32)
    pos, r, s, v = MM.mmr_model(np.zeros(0, np.float32), np.zeros(0, np.int64), hat[:0], 3, 0.5)
    assert pos.size == r.size == s.size == v.size == 0
    pos, r, s, v = MM.mmr_model(np.float32([0.5, 0.4]), np.int64([-1, -1]), hat[:2], 3, 0.5)      # padding only
    assert pos.size == 0
    # identical rows only: p = 1 for every pair, v = lam s - (1 - lam): the list's order stands
    same = np.tile(np.float32([0.6, 0.0, 0.8, 0.0]), (5, 1))
    pos, r, s, v = MM.mmr_model(np.full(5, 0.25, np.float32), np.arange(5), same, 5, 0.5)
    assert pos.tolist() == [0, 1, 2, 3, 4] and v[0] == 0.125 and (v[1:] == 0.125 - 0.5 * np.float64(MM.pair_scores(same, same[0])[0])).all()


# ---- query_mmr on the oracle engine ------------------------------------------------------------------------------------------------
def make(n=300, factory=oracle_factory, space="cosine", dim=DIM):
    col = Collection("c", metadata={"hnsw:space": space}, engine_factory=factory)
    emb, cluster, centres = LM.planted_world(n_clusters=n // 10, paragraphs=2, copies=5, dim=dim, seed=2)
    metas = [{"i": i, "nature": ["GUIDE", "DOCTRINE", "SANCTION"][i % 3]} for i in range(n)]
    col.add(ids=[f"id{i}" for i in range(n)], embeddings=emb, metadatas=metas,
            documents=[f"text {i} {'even' if i % 2 == 0 else 'odd'}" for i in range(n)])
    return col, emb, centres


def hat(col):
    return col._engine.rows                                                       # the stored (normalised) rows: what the oracle ranks


@pytest.mark.parametrize("k,F,lam", [(10, 50, 0.5), (1, 1, 0.5), (5, 5, 0.0), (64, 300, 0.3), (10, 1024, 0.7)])
def test_query_mmr_matches_the_definition(k, F, lam):
    col, emb, centres = make()
    q = centres[:3] + 0.01
    res = col.query_mmr(q.tolist(), n_results=k, fetch_k=F, lambda_mult=lam)
    LM.same(res, col, LM.expected(hat(col), q, k, F, lam))
    assert res["included"] == ["metadatas", "documents", "distances"] and res["embeddings"] is None
    for b in range(3):
        n = len(res["ids"][b])
        assert n == min(k, F, 300) and len(res["documents"][b]) == len(res["metadatas"][b]) == len(res["mmr_scores"][b]) == n
        assert [m["i"] for m in res["metadatas"][b]] == col.rows_of(res["ids"][b])


def test_lambda_one_is_query():
    col, emb, centres = make()
    q = synth.make_queries(4, DIM, emb)
    plain = col.query(q, n_results=10, include=["distances", "embeddings"])
    res = col.query_mmr(q, n_results=10, fetch_k=50, lambda_mult=1.0, include=["distances", "embeddings"])
    assert res["ids"] == plain["ids"] and res["distances"] == plain["distances"]
    for a, b in zip(res["embeddings"], plain["embeddings"]):
        assert a.tobytes() == b.tobytes()
    for b in range(4):                                                            # v = 1 * s - 0 * m = s
        assert res["mmr_scores"][b] == hat_scores(col, q[b], res["ids"][b])
    assert col.query_mmr(q, 10, 50, 1)["ids"] == plain["ids"]                     # an int is a number


def hat_scores(col, q_raw, ids):
    from oracle import oracle as O
    return O.scores(hat(col)[col.rows_of(ids)], O.normalize_rows(np.asarray(q_raw, dtype=np.float32)[None, :])[0]).astype(np.float64).tolist()


def test_mmr_spreads_over_clusters_where_query_does_not():
    col, emb, centres = make()
    cluster = LM.planted_world(n_clusters=30, paragraphs=2, copies=5, dim=DIM, seed=2)[1]
    q = centres[:4]
    plain = col.query(q, n_results=10)["ids"]
    div = col.query_mmr(q, n_results=10, fetch_k=50, lambda_mult=0.5)["ids"]
    for b in range(4):
        assert len({cluster[r] for r in col.rows_of(plain[b])}) == 1              # ten copies of one paragraph
        assert len({cluster[r] for r in col.rows_of(div[b])}) >= 4


def test_filters_tombstones_and_short_lists():
    col, emb, centres = make()
    n = 300
    q = centres[5:7]
    guide = np.arange(n) % 3 == 0
    odd = np.arange(n) % 2 == 1
    res = col.query_mmr(q, 10, 50, 0.5, where={"nature": "GUIDE"})
    LM.same(res, col, LM.expected(hat(col), q, 10, 50, 0.5, guide))
    res = col.query_mmr(q, 10, 50, 0.5, where_document={"$contains": "odd"})
    LM.same(res, col, LM.expected(hat(col), q, 10, 50, 0.5, odd))
    res = col.query_mmr(q, 10, 50, 0.5, where={"nature": "GUIDE"}, where_document={"$contains": "odd"}, include=["distances"])
    LM.same(res, col, LM.expected(hat(col), q, 10, 50, 0.5, guide & odd))
    assert res["documents"] is None and res["metadatas"] is None
    few = np.arange(n) < 4                                                        # n < k: n picks
    res = col.query_mmr(q, 10, 50, 0.5, where={"i": {"$lt": 4}})
    LM.same(res, col, LM.expected(hat(col), q, 10, 50, 0.5, few))
    assert [len(x) for x in res["ids"]] == [4, 4]
    res = col.query_mmr(q, 10, 50, 0.5, where={"i": {"$lt": 0}})                  # a filter that allows nothing
    assert res["ids"] == [[], []] and res["distances"] == [[], []] and res["mmr_scores"] == [[], []] and res["documents"] == [[], []]
    best = col.query(q, n_results=6)["ids"]
    gone = sorted({i for ids in best for i in ids[::2]})                          # tombstones among the best rows
    col.delete(ids=gone)
    assert col._n_dead == len(gone)
    alive = np.ones(n, dtype=bool)
    alive[[int(s[2:]) for s in gone]] = False
    res = col.query_mmr(q, 10, 50, 0.5)
    LM.same(res, col, LM.expected(hat(col), q, 10, 50, 0.5, alive))
    res = col.query_mmr(q, 10, 50, 0.5, where={"nature": "GUIDE"})
    LM.same(res, col, LM.expected(hat(col), q, 10, 50, 0.5, alive & guide))


def test_empty_collection_returns_empty_lists():
    empty = Collection("e", engine_factory=oracle_factory)
    res = empty.query_mmr([[0.0] * 8, [1.0] * 8])
    assert res["ids"] == [[], []] and res["distances"] == [[], []] and res["mmr_scores"] == [[], []]


def test_query_mmr_validation():
    col, emb, _ = make(40)
    q = emb[:1]
    for bad in (dict(n_results=0), dict(n_results=65, fetch_k=100), dict(n_results=True), dict(n_results=2.0), dict(fetch_k=1025),
                dict(fetch_k=9), dict(fetch_k=True, n_results=1), dict(fetch_k=50.0), dict(lambda_mult=-0.01), dict(lambda_mult=1.01),
                dict(lambda_mult=float("nan")), dict(lambda_mult=True), dict(lambda_mult="0.5"), dict(lambda_mult=None)):
        with pytest.raises(ValueError):
            col.query_mmr(q, **bad)
        with pytest.raises(ValueError):
            col.query_mmr_device(q, **bad)
    with pytest.raises(ValueError):
        col.query_mmr(q, include=["uris"])
    with pytest.raises(ValueError):
        col.query_mmr(q, where={"nature": {"$regex": "x"}})
    with pytest.raises(ValueError):
        col.query_mmr(q, where_document={"$regex": "x"})
    with pytest.raises(ValueError):
        col.query_mmr(np.zeros((1, DIM + 4), np.float32))
    with pytest.raises(ValueError):
        col.query_mmr(None)
    with pytest.raises(NotImplementedError):                                      # the host path has no device output
        col.query_mmr_device(q)


class TwoDeviceEngine(OracleEngine):
    devices = [0, 1]


@pytest.mark.parametrize("space", ["ip", "l2"])
def test_query_mmr_refuses_the_other_spaces(space):
    col = Collection("s", metadata={"hnsw:space": space}, engine_factory=oracle_factory)
    with pytest.raises(NotImplementedError):
        col.query_mmr([[1.0] * 8])
    with pytest.raises(NotImplementedError):
        col.query_mmr_device(None)


def test_query_mmr_refuses_a_collection_on_several_devices():
    col = Collection("c", engine_factory=lambda dim, device: TwoDeviceEngine(dim, device))
    col.add(ids=["a", "b"], embeddings=np.eye(2, 8, dtype=np.float32))
    with pytest.raises(NotImplementedError):
        col.query_mmr(np.ones((1, 8), np.float32))
    with pytest.raises(NotImplementedError):
        col.query_mmr_device(np.ones((1, 8), np.float32))
