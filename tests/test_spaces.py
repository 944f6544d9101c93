"""CPU: the "ip" and "l2" spaces (rag_dpo_amd/spaces.py) over the CPU oracle engine: the contract's distances, the
exactness of the ranking on every path of the fallback ladder, writes, persistence, and the guard G against the engine's own scores.
Every result is compared with spaces.brute_force, the contract restated over the raw rows, bit for bit."""
import ctypes
import json
import os

import numpy as np
import pytest

from rag_dpo_amd import _lib, spaces as S, synth
from rag_dpo_amd.collection import Collection, PersistentClient, import_collection

import space_model as M

SPACES = ("ip", "l2")


def _collection(space, x, ids=None, **kw):
    col = Collection("c", metadata={"hnsw:space": space}, engine_factory=M.factory)
    col.add(ids=ids or [f"r{i}" for i in range(x.shape[0])], embeddings=x, **kw)
    return col


def _query_arrays(col, q, k, **kw):
    res = col.query(query_embeddings=q, n_results=k, include=["distances"], **kw)
    return [np.asarray(d, dtype=np.float32) for d in res["distances"]], [[int(s[1:]) for s in ids] for ids in res["ids"]]


def _assert_collection_equals(col, space, q, raw, k, allow=None, **kw):
    bd, br, bc = S.brute_force(space, q, raw, k, allow)
    dist, rows = _query_arrays(col, q, k, **kw)
    for b in range(q.shape[0]):
        assert rows[b] == br[b, : bc[b]].tolist()
        assert (dist[b].view(np.uint32) == bd[b, : bc[b]].view(np.uint32)).all()


# ---- semantics ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("space", SPACES)
@pytest.mark.parametrize("dim", [4, 64, 100, 260])
def test_distances_are_the_contract(space, dim):
    rng = np.random.default_rng(dim)
    x = (rng.standard_normal((40, dim)) * 3).astype(np.float32)
    q = rng.standard_normal((3, dim)).astype(np.float32)
    plain = M.plain_distances(space, q, x)
    for b in range(3):
        d = S.distances(space, q[b], x)
        # within fp32 rounding of plain fp64 numpy (half an ulp of the result, and the fp64 sums' own error)
        assert (np.abs(d.astype(np.float64) - plain[b]) <= np.spacing(np.abs(d)) * 0.5 + 1e-12 * (1 + np.abs(plain[b]))).all()
        # and the ordered sum bit for bit, against a restatement that shares no code with it
        for r in (0, 7, 39):
            assert d[r].view(np.uint32) == M.scalar_distance(space, q[b], x[r]).view(np.uint32)
    col = _collection(space, x)
    _assert_collection_equals(col, space, q, x, 5)


def test_ip_ranks_by_inner_product_not_by_cosine():
    x = M.spread_rows(1500, 64, seed=3)
    q = np.random.default_rng(4).standard_normal((6, 64)).astype(np.float32)
    col = _collection("ip", x)
    _assert_collection_equals(col, "ip", q, x, 10)
    cos = Collection("c", metadata={"hnsw:space": "cosine"}, engine_factory=M.factory)
    cos.add(ids=[f"r{i}" for i in range(1500)], embeddings=x)
    ip_ids = col.query(query_embeddings=q, n_results=10)["ids"]
    cos_ids = cos.query(query_embeddings=q, n_results=10)["ids"]
    # norms over four decades: the largest inner products belong to the long rows, the largest cosines to any row
    assert all(a != b for a, b in zip(ip_ids, cos_ids))
    _, br, _ = S.brute_force("ip", q, x, 10)
    norms = np.linalg.norm(x.astype(np.float64), axis=1)
    assert np.median(norms[br]) > 10 * np.median(norms)


@pytest.mark.parametrize("space", SPACES)
def test_zero_row_zero_query_and_exact_hit(space):
    rng = np.random.default_rng(5)
    x = rng.standard_normal((300, 32)).astype(np.float32)
    x[17] = 0.0
    q = np.stack([np.zeros(32, np.float32), x[123], rng.standard_normal(32).astype(np.float32)])
    col = _collection(space, x)
    _assert_collection_equals(col, space, q, x, 8)
    assert col._engine.last_stats["brute"] == (1 if space == "ip" else 0)   # the zero ip query has no direction to normalise
    dist, rows = _query_arrays(col, q, 8)
    if space == "l2":
        assert rows[1][0] == 123 and dist[1][0] == 0.0 and not np.signbit(dist[1][0])
        assert dist[0][0] == S.distances("l2", q[0], x[17:18])[0] == 0.0 and rows[0][0] == 17
    else:
        assert (dist[0] == 1.0).all() and rows[0] == list(range(8))        # all tie at 1 - 0: ascending row id


@pytest.mark.parametrize("space", SPACES)
def test_duplicates_tie_by_row_and_overflowing_ties_take_the_brute_force(space):
    rng = np.random.default_rng(6)
    x = rng.standard_normal((5000, 16)).astype(np.float32)
    v = (rng.standard_normal(16) * 2).astype(np.float32)
    dup = np.sort(rng.choice(5000, size=S.MAX_FETCH + 150, replace=False))
    x[dup] = v
    q = np.stack([v, rng.standard_normal(16).astype(np.float32)])
    q[0] *= 3.0 if space == "ip" else 1.0        # the duplicates are query 0's nearest rows, in either space
    eng = M.make_engine(space, 16, x)
    got = eng.search(q, 10)
    M.assert_same(got, S.brute_force(space, q, x, 10), "duplicates")
    assert got[1][0].tolist() == dup[:10].tolist()
    # more identical rows at the k-th place than the largest fetch: nothing the engine returns can prove the cut
    assert eng.last_stats["brute"] >= 1 and eng.last_stats["proven_first"] <= 1
    assert eng.last_stats["fetched"] >= 26 + 1024                # ... and both fetches were tried before it


@pytest.mark.parametrize("space", SPACES)
def test_near_ties_are_ordered_by_distance_then_row(space):
    x = M.near_tie_rows(300, 64, seed=7)
    q = np.random.default_rng(8).standard_normal((8, 64)).astype(np.float32)
    eng = M.make_engine(space, 64, x)
    k = 40
    got = eng.search(q, k)
    M.assert_same(got, S.brute_force(space, q, x, k), "near ties")
    # the case is real: some twin pairs have equal or adjacent fp32 distances while the engine's scores order them the other way
    sc, ro, _ = eng.inner.search(S.lift_queries(space, q), 600)
    flipped = 0
    for b in range(q.shape[0]):
        d = S.distances(space, q[b], x)
        pos = np.empty(600, dtype=np.int64)
        pos[ro[b]] = np.arange(600)
        for i in range(0, 600, 2):
            close = abs(int(d[i].view(np.int32)) - int(d[i + 1].view(np.int32))) <= 1
            by_dist = (d[i], i) < (d[i + 1], i + 1)
            flipped += close and (pos[i] < pos[i + 1]) != by_dist
    assert flipped > 0


# ---- writes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("space", SPACES)
def test_update_upsert_delete_compaction_and_rescale(space):
    rng = np.random.default_rng(9)
    raw = rng.standard_normal((2600, 32)).astype(np.float32)
    q = rng.standard_normal((5, 32)).astype(np.float32)
    col = _collection(space, raw[:2500])
    new = (rng.standard_normal((40, 32)) * 0.5).astype(np.float32)
    col.update(ids=[f"r{i}" for i in range(100, 140)], embeddings=new)
    raw[100:140] = new
    col.upsert(ids=[f"r{i}" for i in (5, 2500, 2501)], embeddings=raw[[2600 - 1, 2500, 2501]])
    raw[5] = raw[2599]
    n = 2502
    _assert_collection_equals(col, space, q, raw[:n], 12)
    col.delete(ids=[f"r{i}" for i in range(0, 2000, 2)])                     # 1000 tombstones: below the compaction threshold
    allow = np.ones(n, dtype=bool)
    allow[0:2000:2] = False
    _assert_collection_equals(col, space, q, raw[:n], 12, allow)
    col.delete(ids=[f"r{i}" for i in range(1, 200, 2)])                      # 1100 > max(1024, n / 5): compacts
    assert col._n_dead == 0
    allow[1:200:2] = False
    keep = np.flatnonzero(allow)
    got_d, got_ids = _query_arrays(col, q, 12)
    bd, br, bc = S.brute_force(space, q, raw[:n][keep], 12)
    for b in range(5):
        assert got_ids[b] == keep[br[b]].tolist() and (got_d[b].view(np.uint32) == bd[b].view(np.uint32)).all()
    # a write that does not fit the scale in use: the stored rows are rescaled exactly, nothing else changes
    eng = col._engine
    e0 = eng.scale_exp
    big = (rng.standard_normal((1, 32)) * 1000).astype(np.float32)
    col.add(ids=["r9000"], embeddings=big)
    assert eng.rescales == 1 and eng.scale_exp < e0 and eng.last_stats["rescales"] == 0
    stored = col.get(ids=[f"r{i}" for i in keep[:50]] + ["r9000"], include=["embeddings"])["embeddings"]
    assert (stored.view(np.uint32) == np.concatenate([raw[keep[:50]], big]).view(np.uint32)).all()
    raw2 = np.concatenate([raw[:n][keep], big])
    got_d2, got_ids2 = _query_arrays(col, q, 12)
    bd2, br2, _ = S.brute_force(space, q, raw2, 12)
    ids2 = keep.tolist() + [9000]
    for b in range(5):
        assert got_ids2[b] == [ids2[r] for r in br2[b]] and (got_d2[b].view(np.uint32) == bd2[b].view(np.uint32)).all()
    assert col._engine.last_stats["rescales"] == 1
    # results that do not involve the new row are unchanged, bit for bit
    far = np.flatnonzero([9000 not in r for r in got_ids2])
    for b in far:
        assert got_ids2[b] == got_ids[b] and (got_d2[b].view(np.uint32) == got_d[b].view(np.uint32)).all()


@pytest.mark.parametrize("space", SPACES)
def test_rows_that_cannot_be_lifted_are_refused_and_nothing_is_added(space):
    x = np.random.default_rng(10).standard_normal((20, 8)).astype(np.float32)
    col = _collection(space, x)
    bad = x[:3].copy()
    bad[1, 2] = np.nan
    with pytest.raises(ValueError, match="NaN or Inf"):
        col.add(ids=["a", "b", "c"], embeddings=bad)
    tiny = x[:3].copy()
    tiny[2, 0] = 1e-44                          # a sub-normal element loses bits under the collection's scale
    tiny[2, 1] = 3e4
    with pytest.raises(ValueError, match="row 2 of the batch"):
        col.add(ids=["a", "b", "c"], embeddings=tiny)
    if space == "l2":
        huge = x[:2].copy()
        huge[1] = 3e19                          # |x|^2 / 2 is not finite in fp32
        with pytest.raises(ValueError, match="row 1 of the batch"):
            col.add(ids=["a", "b"], embeddings=huge)
    assert col.count() == 20 and len(col._engine) == 20


@pytest.mark.parametrize("space", SPACES)
def test_a_repeated_row_id_is_refused_before_the_lift_rescales(space):
    """the engine's refusal (include/rdx.h rdx_index_update_stored) comes ahead of the lift: rows 100 times longer than the stored
    ones would rescale every stored row first"""
    x = np.random.default_rng(12).standard_normal((20, 8)).astype(np.float32)
    col = _collection(space, x)
    eng = col._engine
    before = (eng.scale_exp, eng.rescales, eng.inner.get(np.arange(20)).tobytes())
    with pytest.raises(ValueError, match="row id 3 is given more than once"):
        eng.update(np.array([3, 5, 3]), 100 * x[:3])
    assert (eng.scale_exp, eng.rescales, eng.inner.get(np.arange(20)).tobytes()) == before
    from rag_dpo_amd.collection import DuplicateIDError
    with pytest.raises(DuplicateIDError):
        col.update(ids=["r3", "r5", "r3"], embeddings=100 * x[:3])
    assert (eng.scale_exp, eng.rescales, eng.inner.get(np.arange(20)).tobytes()) == before


# ---- persistence and import ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("space", SPACES)
def test_reload_gives_the_same_bits_and_import_keeps_the_space(space, tmp_path):
    x = M.spread_rows(700, 32, seed=11)
    q = np.random.default_rng(12).standard_normal((4, 32)).astype(np.float32)
    cl = PersistentClient(path=str(tmp_path / "db"), engine_factory=M.factory)
    col = cl.create_collection("c", metadata={"hnsw:space": space})
    ids = [f"r{i}" for i in range(700)]
    col.add(ids=ids[:600], embeddings=x[:600])
    cl.persist()
    col.add(ids=ids[600:], embeddings=x[600:])              # journalled behind the snapshot
    before = col.query(query_embeddings=q, n_results=9, include=["distances", "embeddings"])
    hdr = json.load(open(os.path.join(str(tmp_path / "db"), "c", "collection.json")))
    assert hdr["metadata"]["hnsw:space"] == space and isinstance(hdr["space_scale_exp"], int)
    again = PersistentClient(path=str(tmp_path / "db"), engine_factory=M.factory).get_collection("c")
    assert again._engine.space == space and again._engine.scale_exp == col._engine.scale_exp
    after = again.query(query_embeddings=q, n_results=9, include=["distances", "embeddings"])
    assert after["ids"] == before["ids"]
    assert np.asarray(after["distances"], np.float32).tobytes() == np.asarray(before["distances"], np.float32).tobytes()
    for a, b in zip(after["embeddings"], before["embeddings"]):
        assert a.tobytes() == b.tobytes()
    _assert_collection_equals(again, space, q, x, 9)
    dst = import_collection(col, PersistentClient(path=str(tmp_path / "db2"), engine_factory=M.factory), name="copy")
    assert dst.metadata["hnsw:space"] == space and dst._engine.space == space
    _assert_collection_equals(dst, space, q, x, 9)


# ---- independence from the path ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("space", SPACES)
def test_results_do_not_depend_on_the_pad_the_scale_or_the_batch(space):
    x = M.spread_rows(6000, 32, seed=13)
    q = np.random.default_rng(14).standard_normal((9, 32)).astype(np.float32)
    want = S.brute_force(space, q, x, 20)
    stats = []
    for pad in (1, S.MAX_FETCH - 20, None):
        eng = M.make_engine(space, 32, x, pad=pad)
        M.assert_same(eng.search(q, 20), want, f"pad {pad}")
        stats.append(eng.last_stats)
    assert stats[1]["fetched"] == 9 * S.MAX_FETCH and stats[1]["proven_first"] == 9
    assert stats[0]["fetched"] >= 9 * 21
    loose = S.SpaceEngine(space, M.factory(S.lifted_dim(space, 32)), scale_exp=-40)    # a scale far smaller than needed
    loose.add(x)
    assert loose.scale_exp == -40
    M.assert_same(loose.search(q, 20), want, "loose scale")
    one_by_one = [M.make_engine(space, 32, x).search(q[b: b + 1], 20) for b in range(9)]
    M.assert_same(tuple(np.concatenate([o[i] for o in one_by_one]) for i in range(3)), want, "one query at a time")
    bits = np.random.default_rng(15).random(6000) < 0.3
    eng = M.make_engine(space, 32, x)
    from rag_dpo_amd.where import pack_bits
    M.assert_same(eng.search(q, 20, allow_bits=pack_bits(bits)), S.brute_force(space, q, x, 20, bits), "allow_bits")
    M.assert_same(eng.search(q, 7000), S.brute_force(space, q, x, 7000), "k beyond the rows")


# ---- the guard ------------------------------------------------------------------------------------------------------------------
def _guard_use(space, x, q):
    """max over (query, row) of |engine score - 2^e g / |p|| / G, the exact value taken in extended precision"""
    eng = M.make_engine(space, x.shape[1], x)
    n = x.shape[0]
    sc, ro, _ = eng.inner.search(S.lift_queries(space, q), n)
    L = np.longdouble
    worst = 0.0
    for b in range(q.shape[0]):
        ql, xl = q[b].astype(L), x.astype(L)
        g = xl @ ql - ((xl * xl).sum(axis=1) / 2 if space == "l2" else 0)
        pn = np.sqrt((ql * ql).sum() + (1 if space == "l2" else 0))
        exact = np.ldexp(g, eng.scale_exp) / pn
        worst = max(worst, float(np.abs(sc[b].astype(L) - exact[ro[b]]).max()) / S.GUARD[space])
    return worst


@pytest.mark.parametrize("space", SPACES)
def test_engine_scores_stay_inside_the_guard(space):
    rng = np.random.default_rng(16)
    use = [_guard_use(space, M.spread_rows(400, 64, seed=17), rng.standard_normal((6, 64)).astype(np.float32)),
           _guard_use(space, rng.standard_normal((300, 1024)).astype(np.float32), rng.standard_normal((3, 1024)).astype(np.float32))]
    # adversarial: rows aligned with the rounding errors of the normalised query (the worst case of the guard's first term)
    from oracle import oracle as O
    q = rng.standard_normal((4, 256)).astype(np.float32)
    p = S.lift_queries(space, q)
    err = O.normalize_rows(p).astype(np.longdouble) - p.astype(np.longdouble) / np.sqrt((p.astype(np.longdouble) ** 2).sum(axis=1, keepdims=True))
    rows = (err[:, :256] / np.sqrt((err[:, :256] ** 2).sum(axis=1, keepdims=True))).astype(np.float64)
    x = np.concatenate([rows * s for s in (0.999, -0.999, 0.5)]).astype(np.float32)
    use.append(_guard_use(space, x, q))
    print(f"guard use ({space}): random d=64 {use[0]:.3f}, random d=1024 {use[1]:.3f}, aligned {use[2]:.3f} of G")
    assert max(use) < 1.0


# ---- the fallback cap -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("space", SPACES)
@pytest.mark.parametrize("source", ["normal", "embedlike"])
def test_ordinary_inputs_are_proven_by_the_first_fetch(space, source):
    import torch
    dim = 128
    if source == "normal":
        x = synth.make_corpus(3000, dim)
        batches = [synth.make_queries(16, dim, x), np.random.default_rng(18).standard_normal((16, dim)).astype(np.float32)]
    else:
        cpu = torch.device("cpu")
        x = synth.torch_embedlike_chunk(0, 3000, dim, cpu, 3000).numpy().astype(np.float32)
        batches = [synth.torch_embedlike_queries(16, dim, cpu)[0].numpy().astype(np.float32)]
    eng = M.make_engine(space, dim, x)
    for k in (1, 10, 50):
        for q in batches:
            M.assert_same(eng.search(q, k), S.brute_force(space, q, x, k), f"{source} k={k}")
            st = eng.last_stats
            assert st["proven_first"] == q.shape[0] and st["proven_second"] == 0 and st["brute"] == 0, st


# ---- the interface ----------------------------------------------------------------------------------------------------------------
def test_what_this_version_refuses():
    with pytest.raises(ValueError, match="hnsw:space"):
        Collection("c", metadata={"hnsw:space": "manhattan"})
    for space in SPACES:
        with pytest.raises(ValueError, match="one device"):
            Collection("c", metadata={"hnsw:space": space}, devices=[0, 1])
        eng = M.make_engine(space, 8)
        with pytest.raises(ValueError, match="compact_master"):
            eng.set_option("compact_master", 1)
        with pytest.raises(ValueError, match="bf16"):
            eng.add_bf16(np.zeros((1, 8), np.uint16))
        with pytest.raises(NotImplementedError):
            eng.search_device(None, 1, None, None, None)
        with pytest.raises(ValueError, match="multiple of 4"):
            _collection(space, np.ones((2, 6), np.float32))
    assert Collection("c")._factory is not None and Collection("c").metadata.get("hnsw:space", "cosine") == "cosine"


def test_environment_and_sharded_forms_are_refused_too(monkeypatch):
    from rag_dpo_amd.sharded import ShardedSearcher
    for space in SPACES:
        monkeypatch.setenv("RDX_DEVICES", "0,1")
        with pytest.raises(ValueError, match="one device"):
            Collection("c", metadata={"hnsw:space": space})
        monkeypatch.setenv("RDX_DEVICES", "0")                  # one device named in the environment is fine
        assert Collection("c", metadata={"hnsw:space": space})._device == 0
        monkeypatch.delenv("RDX_DEVICES")
        with pytest.raises(ValueError, match="cosine space only"):
            ShardedSearcher(M.make_engine(space, 8))
    with pytest.raises(ValueError, match="rdx_index_update_stored"):
        _lib.check(_lib.load(require_gpu=False).rdx_index_update_stored(None, None, None, 1, _lib.RDX_HOST))


def test_entry_points_validate_their_arguments_without_a_gpu():
    L = _lib.load(require_gpu=False)
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    INV = _lib.RDX_ERR_INVALID
    assert L.rdx_index_update_stored(None, p, p, 1, _lib.RDX_HOST) == INV
    assert L.rdx_space_measure(0, 2, p, 1, 8, p, p, None) == INV            # unknown space
    assert L.rdx_space_measure(0, 0, p, 1, 6, p, p, None) == INV            # dim not a multiple of 4
    assert L.rdx_space_measure(0, 1, p, 1, 4096, p, p, None) == INV         # l2: the lifted dim would be 4100
    assert L.rdx_space_measure(0, 0, None, 1, 8, p, p, None) == INV
    assert L.rdx_space_measure(-1, 0, p, 1, 8, p, p, None) == INV
    assert L.rdx_space_lift(0, 0, 1, p, 1, 8, 3, p, p, None) == INV          # queries are not scaled
    assert L.rdx_space_lift(0, 0, 0, p, 1, 8, 301, p, p, None) == INV
    assert L.rdx_space_lift(0, 0, 0, p, 1, 8, 0, None, p, None) == INV
    assert L.rdx_space_lift(0, 0, 0, ctypes.c_void_p(p.value + 4), 1, 8, 0, p, p, None) == INV
    args = lambda kp, k, guard=1e-7, q=p: (0, 0, q, 1, 8, p, p, p, p, kp, k, 0, guard, p, p, p, p, p, None)
    assert L.rdx_space_rescore(*args(4097, 10)) == INV
    assert L.rdx_space_rescore(*args(16, 17)) == INV
    assert L.rdx_space_rescore(*args(16, 0)) == INV
    assert L.rdx_space_rescore(*args(16, 4, guard=float("nan"))) == INV
    assert L.rdx_space_rescore(*args(16, 4, q=None)) == INV
    assert L.rdx_space_distances(0, 1, p, 65, 8, p, 10, 0, None, 0, p, 10, None) == INV
    assert L.rdx_space_distances(0, 1, p, 2, 8, p, 10, 0, None, 0, p, 9, None) == INV       # stride below the page
    assert L.rdx_space_distances(0, 1, p, 2, 8, p, 10, 0, None, -1, p, 10, None) == INV
    assert L.rdx_space_distances(0, 1, p, 2, 8, None, 10, 0, None, 0, p, 10, None) == INV
    assert b"rdx_space_distances" in L.rdx_last_error()
