"""GPU: the "ip" and "l2" spaces on librdx (csrc/space_kernel.hpp behind rag_dpo_amd/spaces.SpaceEngine) against the numpy model:
spaces.SpaceEngine over the CPU oracle engine, whose scores are bit-identical to librdx's, so distances, rows, counts AND the
proof decisions (last_stats) must be equal — there is no tolerance anywhere in this file.
Shapes: d = 64 and 1024 (l2: engine dims 68 and 1028 = 2 and 17 k-steps), 2 000 and 20 000 rows, 1 / 4 / 70 queries, k = 1 / 10 / 50,
each with the engine's default path and with force_fast (the exact scan and the MFMA scan both feed the re-score).
The kernels on their own — ragged dims, selection edges, the proof flag at its boundary, page addressing: tests/test_gpu_space_kernels.py."""
import numpy as np
import pytest

from rag_dpo_amd import spaces as S

import space_model as M

pytestmark = pytest.mark.gpu
SPACES = ("ip", "l2")


def _hip_engine(space, dim, rows=None, pad=None):
    from rag_dpo_amd.engine import HipIndex
    eng = S.SpaceEngine(space, HipIndex(S.lifted_dim(space, dim), 0))
    eng.pad = pad
    if rows is not None:
        eng.add(rows)
    return eng


def _corpus(n, dim, seed):
    """N(0,1) rows, a tenth of them with norms spread over 0.1 .. 10, 1 % exact duplicates of other rows"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    x[::10] *= (10.0 ** rng.uniform(-1, 1, size=(len(x[::10]), 1))).astype(np.float32)
    dst = rng.choice(n, size=n // 100, replace=False)
    x[dst] = x[rng.integers(0, n, size=n // 100)]
    return x


@pytest.fixture(scope="module", params=[(s, d, n) for s in SPACES for d in (64, 1024) for n in (2000, 20000)],
                ids=lambda p: f"{p[0]}-d{p[1]}-n{p[2]}")
def pair(request):
    space, dim, n = request.param
    x = _corpus(n, dim, seed=dim + n)
    rng = np.random.default_rng(1)
    q = rng.standard_normal((70, dim)).astype(np.float32)
    q[3] = x[n // 2]                                   # a query that is a stored row
    gpu, cpu = _hip_engine(space, dim, x), M.make_engine(space, dim, x)
    want = {}                                          # the model's answers, computed once per (nq, k)
    yield space, dim, x, q, gpu, cpu, want
    gpu.close()


@pytest.mark.parametrize("force_fast", [0, 1])
@pytest.mark.parametrize("nq", [1, 4, 70])
def test_search_equals_the_model(pair, nq, force_fast):
    space, dim, x, q, gpu, cpu, want = pair
    gpu.set_option("force_fast", force_fast)
    try:
        for k in (1, 10, 50):
            if (nq, k) not in want:
                want[(nq, k)] = (cpu.search(q[:nq], k), dict(cpu.last_stats))
            ref, stats = want[(nq, k)]
            M.assert_same(gpu.search(q[:nq], k), ref, f"{space} d={dim} nq={nq} k={k} force_fast={force_fast}")
            assert gpu.last_stats == stats
            assert stats["proven_first"] == nq and stats["brute"] == 0
    finally:
        gpu.set_option("force_fast", 0)


def test_stored_rows_come_back_bit_for_bit(pair):
    space, dim, x, q, gpu, cpu, want = pair
    ids = np.arange(0, x.shape[0], 7, dtype=np.int64)
    assert (gpu.get(ids).view(np.uint32) == x[ids].view(np.uint32)).all()
    assert gpu.scale_exp == cpu.scale_exp


@pytest.mark.parametrize("space", SPACES)
@pytest.mark.parametrize("dim", [64, 1024, 200])
def test_kernel_lift_equals_numpy_lift(space, dim):
    import torch
    from rag_dpo_amd import engine as E
    x = M.spread_rows(333, dim, seed=dim)
    x[5] = 0.0
    x[6, 0] = 1e-44                                     # loses bits when scaled down
    x[7] = (x[7].astype(np.float64) * (1e20 / np.linalg.norm(x[7].astype(np.float64)))).astype(np.float32)   # l2: -|x|^2 / 2 overflows fp32
    dev = torch.device("cuda", 0)
    xt = torch.from_numpy(x).to(dev)
    sq_t, bad_t = E.space_measure(S.KIND[space], xt)
    sq, bad = S.measure(space, x)
    assert (bad_t.cpu().numpy().astype(bool) == bad).all() and bad[7] == (space == "l2")
    ok = ~bad
    assert (sq_t.cpu().numpy()[ok].view(np.uint64) == sq[ok].view(np.uint64)).all()
    e = S.scale_exp_for(float(sq[ok].max()))
    for exp in (e, e - 9):
        y_t, lost_t = E.space_lift(S.KIND[space], xt, exp)
        y, lost = S.lift_rows(space, x, exp)
        keep = ok & ~lost
        assert (lost_t.cpu().numpy().astype(bool)[ok] == lost[ok]).all() and lost[6]
        assert (y_t.cpu().numpy()[keep].view(np.uint32) == y[keep].view(np.uint32)).all()
    p_t, _ = E.space_lift(S.KIND[space], xt[:40].contiguous(), 0, is_query=True)
    assert (p_t.cpu().numpy().view(np.uint32) == S.lift_queries(space, x[:40]).view(np.uint32)).all()
    # a device-tensor add takes the kernels, a host add numpy: the engines hold the same bits
    a, b = _hip_engine(space, dim), _hip_engine(space, dim)
    good = np.ascontiguousarray(x[8:])
    a.add(torch.from_numpy(good).to(dev))
    b.add(good)
    n = good.shape[0]
    assert a.scale_exp == b.scale_exp
    assert (a.inner.get(np.arange(n)).view(np.uint32) == b.inner.get(np.arange(n)).view(np.uint32)).all()
    a.close()
    b.close()


@pytest.mark.parametrize("space", SPACES)
def test_duplicates_near_ties_and_pads(space):
    rng = np.random.default_rng(6)
    x = np.concatenate([rng.standard_normal((4400, 64)).astype(np.float32), M.near_tie_rows(300, 64, seed=7)])
    v = (rng.standard_normal(64) * 2).astype(np.float32)
    dup = np.sort(rng.choice(4400, size=S.MAX_FETCH + 50, replace=False))
    x[dup] = v
    q = rng.standard_normal((6, 64)).astype(np.float32)
    q[0] = v * (3.0 if space == "ip" else 1.0)         # its k-th place lies inside more duplicates than any fetch holds
    gpu, cpu = _hip_engine(space, 64, x), M.make_engine(space, 64, x)
    for pad in (None, 1, S.MAX_FETCH - 40):
        gpu.pad = cpu.pad = pad
        ref = cpu.search(q, 40)
        M.assert_same(gpu.search(q, 40), ref, f"pad {pad}")
        assert gpu.last_stats == cpu.last_stats and cpu.last_stats["brute"] >= 1
        M.assert_same(ref, S.brute_force(space, q, x, 40), "the model itself")
    assert ref[1][0].tolist() == dup[:40].tolist()
    gpu.close()


@pytest.mark.parametrize("space", SPACES)
def test_collection_where_rescale_query_device_and_embeddings(space):
    import torch
    from rag_dpo_amd.collection import Collection
    rng = np.random.default_rng(21)
    n, dim = 3000, 64
    x = rng.standard_normal((n, dim)).astype(np.float32)
    q = rng.standard_normal((5, dim)).astype(np.float32)
    ids = [f"r{i}" for i in range(n)]
    col = Collection("c", metadata={"hnsw:space": space})
    col.add(ids=ids, embeddings=x, metadatas=[{"g": i % 3, "h": i} for i in range(n)])

    def check(raw, names, allow=None, **kw):
        res = col.query(query_embeddings=q, n_results=10, include=["distances", "embeddings"], **kw)
        bd, br, bc = S.brute_force(space, q, raw, 10, allow)
        for b in range(5):
            assert res["ids"][b] == [names[r] for r in br[b, : bc[b]]]
            assert np.asarray(res["distances"][b], np.float32).tobytes() == bd[b, : bc[b]].tobytes()
            assert res["embeddings"][b].tobytes() == raw[br[b, : bc[b]]].tobytes()      # the raw bits, not the lifted rows
        return bd

    check(x, ids)
    check(x, ids, allow=np.arange(n) % 3 == 1, where={"g": 1})
    check(x, ids, allow=np.arange(n) < 7, where={"h": {"$lt": 7}})       # fewer allowed rows than k: counts of 7, padding behind
    if space == "l2":      # an allowed row whose own distance overflows fp32 still ranks before every disallowed row (brute force)
        qh = np.full((1, dim), 3e19, dtype=np.float32)
        res = col.query(query_embeddings=qh, n_results=5, where={"g": 1}, include=["distances"])
        assert res["ids"][0] == ["r1", "r4", "r7", "r10", "r13"] and np.isinf(res["distances"][0]).all()
        assert col._engine.last_stats["brute"] == 1
    col.delete(ids=ids[:200])
    check(x, ids, allow=(np.arange(n) % 3 == 1) & (np.arange(n) >= 200), where={"g": 1})
    big = (rng.standard_normal((2, dim)) * 500).astype(np.float32)
    col.upsert(ids=["r7", "r9000", "r300"], embeddings=np.concatenate([big[:1], big[1:], x[301:302]]))   # r7 is deleted: added anew
    assert col._engine.rescales == 1
    raw = np.concatenate([x, big])
    raw[300] = x[301]
    alive = np.ones(n + 2, dtype=bool)
    alive[:200] = False
    bd = check(raw, ids + ["r7", "r9000"], allow=alive)
    qt = torch.from_numpy(q).to(torch.device("cuda", 0))
    stats = dict(col._engine.last_stats)
    d_t, r_t, c_t = col.query_device(qt, n_results=10)
    assert col._engine.last_stats == stats
    assert d_t.cpu().numpy().tobytes() == bd.tobytes() and (c_t.cpu().numpy() == 10).all()
    assert col.ids_of(r_t.cpu()) == col.query(query_embeddings=q, n_results=10)["ids"]
    got = col.get(ids=["r9000", "r300", "r299"], include=["embeddings"])["embeddings"]
    assert got.tobytes() == raw[[300 - 1, 300, n + 1]].tobytes()
