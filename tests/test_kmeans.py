"""CPU: k-means' definition (rag_dpo_amd/kmeans.py) against an independent brute-force restatement over the oracle's scores and
normalisation, Collection.kmeans / assign_clusters on the test-only oracle engine (the host path) against the definition, planted
clusters, ties, duplicate centroids, empty clusters, max_iter 0 and 1, filters and deleted rows, the seed, every refusal, and the
ordering core (rag_dpo_amd/csrc/km_order.hpp) as a stand-alone program (tests/c_abi/km_order_host.cpp) built by g++ with the address
and undefined-behaviour sanitizers."""
import functools
import os
import subprocess

import numpy as np
import pytest

from rag_dpo_amd import kmeans as KM
from rag_dpo_amd.collection import Collection

from oracle_engine import OracleEngine, factory as oracle_factory
from test_sanitizers import ENV, ROOT, SAN

DIM = 64
F32 = np.float32


# ---- the model against a brute-force restatement ---------------------------------------------------------------------------------
def brute(oracle, x, init, max_iter, allowed=None):
    """the issue's definition, written again without a line of kmeans.py: a score matrix per assignment, max and first index per row,
    members gathered by a scan over the rows, sums by folding rows left to right"""
    n, K = x.shape[0], init.shape[0]
    ok = [True] * n if allowed is None else [bool(a) for a in allowed]

    def assign(C):
        q = oracle.normalize_rows(C)
        S = np.stack([oracle.scores(x, q[c]) for c in range(K)])
        lab, sc = [-1] * n, [F32(-np.inf)] * n
        for r in range(n):
            if ok[r]:
                best = max(S[:, r])
                lab[r] = [c for c in range(K) if S[c, r] == best][0]
                sc[r] = best
        return lab, sc

    def fold(rows):
        return functools.reduce(lambda a, b: a + b, rows, np.zeros(x.shape[1], dtype=np.float64))

    C = oracle.normalize_rows(init)
    L, S = assign(C)
    n_iter, converged = 0, False
    while n_iter < max_iter:
        C = C.copy()
        for c in range(K):
            members = [r for r in range(n) if L[r] == c]
            if members:
                totals = [fold([x[r].astype(np.float64) for r in members[a: a + 256]]) for a in range(0, len(members), 256)]
                C[c] = oracle.normalize_rows(fold(totals).astype(F32)[None, :])[0]
        n_iter += 1
        L2, S = assign(C)
        same, L = L2 == L, L2
        if same:
            converged = True
            break
    return np.array(L, dtype=np.int64), np.array(S, dtype=F32), C, np.array([L.count(c) for c in range(K)], dtype=np.int64), n_iter, converged


def equal(a, b):
    return all(np.asarray(u).tobytes() == np.asarray(v).tobytes() and np.asarray(u).shape == np.asarray(v).shape for u, v in zip(a[:4], b[:4])) \
        and tuple(a[4:]) == tuple(b[4:])


@pytest.mark.parametrize("seed", range(12))
def test_the_model_is_the_definition(seed, oracle):
    rng = np.random.default_rng(seed)
    dim = (64, 260, 8)[seed % 3]
    n, K = 1 + (37 * seed) % 700, 1 + seed % 7
    x = oracle.normalize_rows(rng.standard_normal((n, dim)).astype(F32) + (seed % 2) * 2.0)
    if n > 300:
        x[: n // 2] = x[0]                                                          # more than a segment of identical rows
    init = rng.standard_normal((K, dim)).astype(F32)
    if K > 2:
        init[2] = init[0]                                                           # duplicate centroids
    allowed = rng.random(n) < 0.7 if seed % 4 == 1 else None
    max_iter = (0, 1, 3, 20)[seed % 4]
    want = brute(oracle, x, init, max_iter, allowed)
    assert equal(KM.kmeans_model(x, init, max_iter, allowed), want)                  # the scores stated in numpy (mmr.pair_scores)
    assert equal(KM.kmeans_model(x, init, max_iter, allowed, scores_of=lambda q: oracle.scores(x, q)), want)
    if K > 2 and max_iter == 0:
        assert want[3][2] == 0                                                       # of two identical centroids the later one gets no row
    assert KM.k1(init).tobytes() == oracle.normalize_rows(init).tobytes()


def test_the_sample_rule():
    rows = np.array([3, 5, 8, 13, 21, 34], dtype=np.int64)
    got = KM.sample_rows(rows, 4, 7)
    assert got.tolist() == sorted(np.random.default_rng(7).choice(rows, 4, replace=False).tolist()) and got.dtype == np.int64
    assert KM.sample_rows(rows, 6, 0).tolist() == rows.tolist()
    with pytest.raises(ValueError, match="exceeds"):
        KM.sample_rows(rows, 7, 0)


# ---- Collection.kmeans on the oracle engine ---------------------------------------------------------------------------------------
N, K_TRUE = 240, 4


def world_rows():
    """four well-separated themes on axes of their own, rows interleaved"""
    rng = np.random.default_rng(2)
    x = 0.05 * rng.standard_normal((N, DIM)).astype(F32)
    x[np.arange(N), 10 * (np.arange(N) % K_TRUE)] += 1.0
    return x


def make(rows=None):
    x = world_rows() if rows is None else rows
    n = len(x)
    col = Collection("km", metadata={"hnsw:space": "cosine"}, engine_factory=oracle_factory)
    col.add(ids=[f"id{i}" for i in range(n)], embeddings=x, metadatas=[{"k": i % 2, "i": i} for i in range(n)],
            documents=[f"text {i} {'keep' if i % 3 else 'drop'}" for i in range(n)])
    return col


def model_answer(col, oracle, init, max_iter, allowed=None):
    """the definition over the oracle's exact scores of the engine's stored rows -> kmeans' dict"""
    hat = col._engine.rows
    lab, sc, cen, cnt, n_iter, conv = KM.kmeans_model(hat, init, max_iter, allowed, scores_of=lambda q: oracle.scores(hat, q))
    groups = [np.flatnonzero(lab == c) for c in range(len(cnt))]
    return {"centroids": cen, "clusters": [[col._ids[r] for r in g] for g in groups],
            "distances": [[float(F32(1.0) - sc[r]) for r in g] for g in groups], "counts": cnt.tolist(), "n_iter": n_iter, "converged": conv}


def same_dict(a, b):
    assert a.keys() == b.keys() == {"centroids", "clusters", "distances", "counts", "n_iter", "converged"}
    assert a["centroids"].dtype == np.float32 and a["centroids"].tobytes() == b["centroids"].tobytes()
    assert all(a[k] == b[k] for k in a if k != "centroids"), [k for k in a if k != "centroids" and a[k] != b[k]]


def sampled_init(col, k, seed, allowed=None):
    rows = np.arange(col._rows) if allowed is None else np.flatnonzero(allowed)
    return col._engine.rows[KM.sample_rows(rows, k, seed)]


def test_planted_clusters_are_recovered(oracle):
    col = make()
    init = np.zeros((K_TRUE, DIM), dtype=F32)
    init[np.arange(K_TRUE), 10 * np.arange(K_TRUE)] = 1.0
    init += 0.2                                                                      # off the themes, closest to its own
    got = col.kmeans(init=init)
    same_dict(got, model_answer(col, oracle, init, 20))
    assert got["converged"] and got["counts"] == [N // K_TRUE] * K_TRUE
    assert got["clusters"] == [[f"id{i}" for i in range(c, N, K_TRUE)] for c in range(K_TRUE)]   # each in row order
    assert all(0 <= d < 0.2 for ds in got["distances"] for d in ds)
    assert col.kmeans_stats == {"calls": 1, "rows": N, "iterations": got["n_iter"], "host": 1}
    # the same through n_clusters and a seed: the stored rows of kmeans.sample_rows' pick
    got = col.kmeans(K_TRUE, seed=3)
    same_dict(got, model_answer(col, oracle, sampled_init(col, K_TRUE, 3), 20))
    same_dict(got, col.kmeans(K_TRUE, seed=3))                                       # the same seed, the same answer
    same_dict(col.kmeans(n_clusters=K_TRUE, init=init), col.kmeans(init=init))


def test_max_iter_0_and_1_and_assign_clusters(oracle):
    col = make()
    init = sampled_init(col, 3, 0)
    for it in (0, 1):
        got = col.kmeans(init=init, max_iter=it)
        same_dict(got, model_answer(col, oracle, init, it))
        assert got["n_iter"] == it and sum(got["counts"]) == N
    got = col.assign_clusters(init)
    same_dict(got, model_answer(col, oracle, init, 0))
    assert got["converged"] is False and got["centroids"].tobytes() == KM.k1(init).tobytes()
    done = col.kmeans(init=init)
    again = col.assign_clusters(done["centroids"])                                   # labels and scores are assign(returned centroids)
    assert again["clusters"] == done["clusters"] and again["distances"] == done["distances"]
    assert col.assign_clusters(init[0])["counts"] == [N]                             # one centroid as a plain vector


def test_ties_duplicates_and_empty_clusters(oracle):
    x = np.zeros((6, DIM), dtype=F32)
    x[0, [0, 1]] = 1.0                                                               # ties centroids 0 and 1
    x[1, 0] = x[2, 1] = x[3, 2] = 1.0
    x[4, 5] = 1.0                                                                    # orthogonal to every centroid: scores 0, ties all
    x[5, [1, 2]] = 1.0                                                               # ties centroids 1 and 2 (and 3, its copy)
    col = make(x)
    init = np.eye(3, DIM, dtype=F32)
    init = np.concatenate([init, init[1:2], 7.0 * np.eye(1, DIM, 9, dtype=F32)])    # 3 = a copy of 1; 4 = an axis without rows
    got = col.assign_clusters(init)
    same_dict(got, model_answer(col, oracle, init, 0))
    assert got["clusters"] == [["id0", "id1", "id4"], ["id2", "id5"], ["id3"], [], []]
    got = col.kmeans(init=init, max_iter=5)
    same_dict(got, model_answer(col, oracle, init, 5))
    assert got["counts"][4] == 0 and got["centroids"][4].tobytes() == KM.k1(init)[4].tobytes()   # an empty cluster keeps its centroid


def test_filters_and_deleted_rows(oracle):
    col = make()
    even = np.arange(N) % 2 == 0
    keep = np.arange(N) % 3 != 0
    for kw, allowed in (({"where": {"k": 0}}, even), ({"where_document": {"$contains": "keep"}}, keep),
                        ({"where": {"k": 0}, "where_document": {"$contains": "keep"}}, even & keep)):
        got = col.kmeans(3, seed=1, **kw)
        same_dict(got, model_answer(col, oracle, sampled_init(col, 3, 1, allowed), 20, allowed))
        assert {i for c in got["clusters"] for i in c} == {f"id{i}" for i in np.flatnonzero(allowed)}
    col.delete(ids=["id0", "id5", "id6"])
    alive = np.ones(N, dtype=bool)
    alive[[0, 5, 6]] = False
    got = col.kmeans(3, seed=1)
    same_dict(got, model_answer(col, oracle, sampled_init(col, 3, 1, alive), 20, alive))
    assert sum(got["counts"]) == N - 3
    col.update(ids=["id7"], embeddings=np.eye(1, DIM, 33, dtype=F32))
    same_dict(col.kmeans(3, seed=1), model_answer(col, oracle, sampled_init(col, 3, 1, alive), 20, alive))
    got = col.assign_clusters(np.eye(2, DIM, dtype=F32), where={"i": {"$lt": 0}})    # a filter that allows nothing
    assert got["counts"] == [0, 0] and got["clusters"] == [[], []]


def test_the_host_path_is_the_model(oracle):
    rng = np.random.default_rng(4)
    x = oracle.normalize_rows(rng.standard_normal((300, DIM)).astype(F32) + 0.5)
    e = OracleEngine(DIM)
    e.add_stored(x)
    init = rng.standard_normal((5, DIM)).astype(F32)
    allowed = rng.random(300) < 0.6
    bits = np.packbits(allowed, bitorder="little")
    bits = np.concatenate([bits, np.zeros(-len(bits) % 4, np.uint8)]).view(np.uint32)
    for chunk in (1, 2, 64):                                                         # the chunking does not show
        assert equal(KM.kmeans_host(e, init, 7, {}, None, chunk), KM.kmeans_model(x, init, 7))
        assert equal(KM.kmeans_host(e, init, 7, {"allow_bits": bits}, allowed, chunk), KM.kmeans_model(x, init, 7, allowed))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_argument_checks():
    col = make()
    good = np.eye(3, DIM, dtype=F32)
    nan, inf = good.copy(), good.copy()
    nan[1, 2], inf[0, 0] = np.nan, np.inf
    for bad in (dict(), dict(n_clusters=0), dict(n_clusters=4097), dict(n_clusters=2.0), dict(n_clusters=True), dict(n_clusters=N + 1),
                dict(n_clusters=3, max_iter=-1), dict(n_clusters=3, max_iter=1001), dict(n_clusters=3, max_iter=2.5), dict(n_clusters=3, seed=-1),
                dict(n_clusters=3, seed=1.5), dict(init=np.eye(3, DIM + 4, dtype=F32)), dict(init=nan), dict(init=inf), dict(init=good, n_clusters=4),
                dict(init=np.zeros((0, DIM), dtype=F32)), dict(init=np.zeros((4097, DIM), dtype=F32)), dict(n_clusters=3, where_document={"$regex": "x"}),
                dict(n_clusters=101, where={"i": {"$lt": 100}})):
        with pytest.raises(ValueError):
            col.kmeans(**bad)
        with pytest.raises(ValueError):
            col.kmeans_device(**bad)
    for bad in (nan, inf, np.eye(3, DIM + 4, dtype=F32)):
        with pytest.raises(ValueError):
            col.assign_clusters(bad)
    with pytest.raises(NotImplementedError):                                        # the host path has no device output
        col.kmeans_device(3)
    assert col.kmeans_stats == {"calls": 0, "rows": 0, "iterations": 0, "host": 0}   # nothing ran


def test_empty_collection():
    empty = Collection("e", engine_factory=oracle_factory)
    for call in (lambda: empty.kmeans(2), lambda: empty.kmeans_device(2), lambda: empty.assign_clusters(np.eye(2, DIM, dtype=F32))):
        with pytest.raises(ValueError, match="empty"):
            call()


class TwoDeviceEngine(OracleEngine):
    devices = [0, 1]


@pytest.mark.parametrize("space", ["ip", "l2"])
def test_the_other_spaces_are_refused(space):
    col = Collection("s", metadata={"hnsw:space": space}, engine_factory=oracle_factory)
    for call in (lambda: col.kmeans(2), lambda: col.kmeans_device(2), lambda: col.assign_clusters(np.eye(2, DIM, dtype=F32))):
        with pytest.raises(NotImplementedError, match="not available in the"):
            call()


def test_a_collection_on_several_devices_is_refused():
    col = Collection("c", engine_factory=lambda dim, device: TwoDeviceEngine(dim, device))
    col.add(ids=["a", "b"], embeddings=np.eye(2, 8, dtype=np.float32))
    with pytest.raises(NotImplementedError, match="one device"):
        col.kmeans(2)


def test_the_binding_is_declared():
    from rag_dpo_amd import _lib
    assert "rdx_index_kmeans" in _lib.SYMBOLS and len(_lib.SYMBOLS["rdx_index_kmeans"][1]) == 11
    assert (_lib.KMEANS_MAX_CLUSTERS, _lib.KMEANS_MAX_ITER) == (KM.MAX_CLUSTERS, KM.MAX_ITER) == (4096, 1000)
    with open(os.path.join(ROOT, "include", "rdx.h")) as f:
        header = f.read()
    assert "#define RDX_KMEANS_MAX_CLUSTERS 4096" in header and "int rdx_index_kmeans(rdx_index* h, const float* init, int n_clusters, int max_iter" in header
    with open(os.path.join(ROOT, "rag_dpo_amd", "csrc", "km_order.hpp")) as f:
        assert f"constexpr int KM_SEGMENT = {KM.SEGMENT};" in f.read()


# ---- the ordering core as a stand-alone program, under the sanitizers --------------------------------------------------------------
CASES = ["interleaved"] * 5 + ["random with gaps", "segment borders", "one cluster", "no row allowed", "more clusters than a tile"]


def test_the_ordering_core_under_the_sanitizers(tmp_path):
    """the rehearsal of k_km_hist / k_km_scan / k_km_place / k_km_seg_table: a rank or an offset that is off, or a read past a tile, shows here"""
    exe = str(tmp_path / "km_order_host")
    subprocess.check_call(["g++", "-std=c++17", *SAN, "-Wall", "-Wextra", os.path.join(ROOT, "tests", "c_abi", "km_order_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=ENV)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    for word in ("runtime error", "AddressSanitizer"):
        assert word not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok" and [line.split(":")[0] for line in lines[:-1]] == CASES
