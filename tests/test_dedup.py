"""CPU: near-duplicate clustering's definition (rag_dpo_amd/dedup.py) against a literal transitive closure, Collection.near_duplicates
on the test-only oracle engine (the host path) against the definition over the oracle's exact scores, the argument checks, and the
union core (rag_dpo_amd/csrc/dup_union.hpp) as a stand-alone program (tests/c_abi/dup_union_host.cpp) built by g++ twice — address +
undefined-behaviour sanitizers, and the thread sanitizer — with eight threads uniting shuffled edges, under a time limit."""
import os
import subprocess

import numpy as np
import pytest

from rag_dpo_amd import dedup as DD
from rag_dpo_amd import range_search as RS
from rag_dpo_amd.collection import Collection

from oracle_engine import OracleEngine, factory as oracle_factory
from test_sanitizers import ENV, ROOT, SAN

DIM = 64
F32 = np.float32


# ---- the model against a literal transitive closure ------------------------------------------------------------------------------
def closure_labels(adj, ok):
    """reachability by repeated squaring of the symmetrised adjacency matrix restricted to allowed rows; label = smallest reachable row"""
    n = adj.shape[0]
    a = (adj | adj.T) & ok[:, None] & ok[None, :]
    reach = a | np.eye(n, dtype=bool)
    for _ in range(max(1, int(np.ceil(np.log2(max(n, 2)))))):
        reach = (reach.astype(np.int32) @ reach.astype(np.int32)) > 0
    return np.array([int(np.flatnonzero(reach[r])[0]) if ok[r] else -1 for r in range(n)], dtype=np.int64)


@pytest.mark.parametrize("seed", range(60))
def test_the_model_is_the_transitive_closure(seed):
    rng = np.random.default_rng(seed)
    n = 1 + seed % 40
    density = (0.02, 0.08, 0.3)[seed % 3]
    adj = rng.random((n, n)) < density                                               # directed: adj[i][j] does not imply adj[j][i]
    if n > 4:
        adj[n // 2, :] = adj[:, n // 2] = False                                      # an isolated row
    ok = rng.random(n) < 0.8 if seed % 2 else np.ones(n, dtype=bool)                 # excluded rows
    want = closure_labels(adj, ok)
    assert DD.labels_from_adjacency(adj, ok).tolist() == want.tolist()
    # the same through scores: 1.0 where there is an edge, 0.0 elsewhere, t = 0.5; the diagonal counts in the totals when it is set
    sc = adj.astype(np.float32)
    labels, totals = DD.near_dup_model(lambda i: sc[i], n, 0.5, ok)
    assert labels.tolist() == want.tolist()
    assert totals.tolist() == [int((adj[r] & ok).sum()) if ok[r] else 0 for r in range(n)]
    groups = DD.clusters_of(labels)
    assert all(len(g) >= 2 and g == sorted(g) and len(set(want[g])) == 1 and want[g[0]] == g[0] for g in groups)
    assert [g[0] for g in groups] == sorted(g[0] for g in groups)
    assert sum(len(g) for g in groups) == sum(1 for r in range(n) if ok[r] and (want == want[r]).sum() >= 2)


def test_clusters_of_an_empty_answer():
    assert DD.clusters_of(np.zeros(0, np.int64)) == [] and DD.clusters_of(np.array([-1, -1])) == [] and DD.clusters_of(np.arange(5)) == []


# ---- Collection.near_duplicates on the oracle engine -----------------------------------------------------------------------------
CHAIN, COPIES, LONE = list(range(0, 10)), list(range(10, 15)), list(range(15, 30))


def unit(*ks):
    v = np.zeros(DIM, dtype=np.float32)
    v[list(ks)] = 1.0
    return v


def world_rows():
    """rows 0..9 a chain x_i = e_i + e_{i+1} (neighbours score 0.5, everything else 0), rows 10..14 five copies of one vector, scaled
    differently (the stored rows are normalised), rows 15..29 alone on axes of their own"""
    x = [unit(i, i + 1) for i in CHAIN]
    x += [(1.0 + 0.5 * k) * (unit(12) + 0.5 * unit(13)) for k in range(len(COPIES))]
    x += [unit(20 + k) for k in range(len(LONE))]
    return np.stack(x).astype(np.float32)


def make(rows=None):
    x = world_rows() if rows is None else rows
    n = len(x)
    col = Collection("dedup", metadata={"hnsw:space": "cosine"}, engine_factory=oracle_factory)
    col.add(ids=[f"id{i}" for i in range(n)], embeddings=x, metadatas=[{"k": i % 2, "i": i} for i in range(n)],
            documents=[f"text {i} {'keep' if i % 3 else 'drop'}" for i in range(n)])
    return col


def model_answer(col, oracle, D, allowed=None):
    """the definition over the oracle's exact scores of the engine's stored rows -> near_duplicates' dict"""
    hat = col._engine.rows
    n = hat.shape[0]
    labels, totals = DD.near_dup_model(lambda i: oracle.scores(hat, oracle.normalize_rows(hat[i:i + 1])[0]), n, RS.score_threshold(D), allowed)
    groups = DD.clusters_of(labels)
    return {"clusters": [[col._ids[r] for r in g] for g in groups], "neighbors": [[int(totals[r]) for r in g] for g in groups]}


def ids(rows):
    return [f"id{i}" for i in rows]


def test_some_rows_cluster(oracle):
    col = make()
    hat = col._engine.rows
    s0 = oracle.scores(hat, hat[0])
    assert abs(float(s0[1]) - 0.5) < 1e-6 and (s0[2:] == 0).all()                   # what the chain is built on
    got = col.near_duplicates(0.6)
    assert got == model_answer(col, oracle, 0.6)
    assert got["clusters"] == [ids(CHAIN), ids(COPIES)]
    assert got["neighbors"] == [[2] + [3] * 8 + [2], [5] * 5]                        # the row itself counts
    assert col.dedup_stats == {"calls": 1, "rows": 30, "listed": 0, "dense": 0, "batches": 0, "host": 30}
    # a tighter distance keeps the copies only; their first id is the earliest-added row
    got = col.near_duplicates(0.01)
    assert got == model_answer(col, oracle, 0.01) and got["clusters"] == [ids(COPIES)]
    # max_neighbors and max_dense_rows do not show on the host path either
    assert col.near_duplicates(0.6, max_neighbors=1, max_dense_rows=0)["clusters"] == [ids(CHAIN), ids(COPIES)]


def test_no_row_and_every_row_clusters(oracle):
    col = make(np.stack([unit(k) for k in range(12)]))
    assert col.near_duplicates(0.5) == {"clusters": [], "neighbors": []}
    got = col.near_duplicates(2.5)                                                   # every row is within 2.5 of every row
    assert got == model_answer(col, oracle, 2.5)
    assert got["clusters"] == [ids(range(12))] and got["neighbors"] == [[12] * 12]
    got = col.near_duplicates(1.0)                                                   # distance 1 = score 0: orthogonal rows are in range
    assert got == model_answer(col, oracle, 1.0) and got["clusters"] == [ids(range(12))]


def test_filters_remove_rows_and_their_edges(oracle):
    col = make()
    n = 30
    even = np.arange(n) % 2 == 0
    got = col.near_duplicates(0.6, where={"k": 0})
    assert got == model_answer(col, oracle, 0.6, even)
    assert got["clusters"] == [ids([10, 12, 14])] and got["neighbors"] == [[3, 3, 3]]   # every other chain row is gone: no chain
    keep = np.arange(n) % 3 != 0
    got = col.near_duplicates(0.6, where_document={"$contains": "keep"})
    assert got == model_answer(col, oracle, 0.6, keep)
    assert got["clusters"] == [ids([1, 2]), ids([4, 5]), ids([7, 8]), ids([10, 11, 13, 14])]
    both = even & keep
    got = col.near_duplicates(0.6, where={"k": 0}, where_document={"$contains": "keep"})
    assert got == model_answer(col, oracle, 0.6, both) and got["clusters"] == [ids([10, 14])]
    assert col.near_duplicates(0.6, where={"i": {"$lt": 0}}) == {"clusters": [], "neighbors": []}   # a filter that allows nothing


def test_a_tombstone_inside_a_chain_splits_it(oracle):
    col = make()
    col.delete(ids=["id4", "id10"])
    alive = np.ones(30, dtype=bool)
    alive[[4, 10]] = False
    got = col.near_duplicates(0.6)
    assert got == model_answer(col, oracle, 0.6, alive)
    assert got["clusters"] == [ids([0, 1, 2, 3]), ids([5, 6, 7, 8, 9]), ids([11, 12, 13, 14])]   # the copies' representative is the next one
    assert got["neighbors"][0] == [2, 3, 3, 2] and got["neighbors"][2] == [4] * 4


def test_updates_move_rows_between_clusters(oracle):
    col = make()
    col.update(ids=["id7", "id20"], embeddings=np.stack([unit(50), 3.0 * (unit(12) + 0.5 * unit(13))]))
    got = col.near_duplicates(0.6)
    assert got == model_answer(col, oracle, 0.6)
    assert got["clusters"] == [ids(range(0, 7)), ids([8, 9]), ids(COPIES + [20])]


def test_empty_collection():
    empty = Collection("e", engine_factory=oracle_factory)
    assert empty.near_duplicates(0.3) == {"clusters": [], "neighbors": []}
    with pytest.raises(ValueError):
        empty.near_duplicates(float("nan"))
    with pytest.raises(ValueError):
        empty.near_duplicates_device(0.3)


def test_argument_checks():
    col = make()
    for bad in (dict(max_distance=float("nan")), dict(max_distance=0.3, max_neighbors=0), dict(max_distance=0.3, max_neighbors=1025),
                dict(max_distance=0.3, max_neighbors=True), dict(max_distance=0.3, max_neighbors=8.0), dict(max_distance=0.3, max_dense_rows=-1),
                dict(max_distance=0.3, max_dense_rows=1.5), dict(max_distance=0.3, where_document={"$regex": "x"})):
        with pytest.raises(ValueError):
            col.near_duplicates(**bad)
        with pytest.raises(ValueError):
            col.near_duplicates_device(**bad)
    with pytest.raises(NotImplementedError):                                        # the host path has no device output
        col.near_duplicates_device(0.3)
    assert col.dedup_stats["rows"] == 0                                             # nothing ran


class TwoDeviceEngine(OracleEngine):
    devices = [0, 1]


@pytest.mark.parametrize("space", ["ip", "l2"])
def test_the_other_spaces_are_refused(space):
    col = Collection("s", metadata={"hnsw:space": space}, engine_factory=oracle_factory)
    with pytest.raises(NotImplementedError, match="not available in the"):
        col.near_duplicates(0.3)
    with pytest.raises(NotImplementedError, match="not available in the"):
        col.near_duplicates_device(0.3)


def test_a_collection_on_several_devices_is_refused():
    col = Collection("c", engine_factory=lambda dim, device: TwoDeviceEngine(dim, device))
    col.add(ids=["a", "b"], embeddings=np.eye(2, 8, dtype=np.float32))
    with pytest.raises(NotImplementedError, match="one device"):
        col.near_duplicates(0.3)


def test_the_binding_is_declared():
    from rag_dpo_amd import _lib
    assert "rdx_index_near_dup" in _lib.SYMBOLS and len(_lib.SYMBOLS["rdx_index_near_dup"][1]) == 9


# ---- the union core as a stand-alone program, under the sanitizers ---------------------------------------------------------------
GRAPHS = ("chain", "star", "cliques", "sparse", "chain with gaps", "sparse with gaps", "clique")
TSAN = ["-fsanitize=thread", "-pthread", "-fno-omit-frame-pointer", "-g", "-O1"]


@pytest.mark.parametrize("flags", [SAN + ["-pthread"], TSAN], ids=["asan_ubsan", "tsan"])
def test_the_union_core_with_eight_threads(flags, tmp_path):
    """the rehearsal of the device loops: a loop that can spin, a write that breaks parent[x] <= x or a data race shows up here"""
    exe = str(tmp_path / "dup_union_host")
    subprocess.check_call(["g++", "-std=c++17", *flags, "-Wall", "-Wextra", os.path.join(ROOT, "tests", "c_abi", "dup_union_host.cpp"), "-o", exe])
    env = dict(ENV, TSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    for word in ("runtime error", "AddressSanitizer", "ThreadSanitizer", "data race"):
        assert word not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok" and [line.split(":")[0] for line in lines[:-1]] == list(GRAPHS)
