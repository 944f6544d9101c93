"""GPU: the BM25 kernels (csrc/bm25_kernel.hpp through include/rdx.h rdx_bm25_*) return the same rows and bit-identical
float64 scores as the CPU restatement of rank_bm25 (tests/bm25_oracle.py), and the hybrid DenseRetriever on librdx replays
the fixture captured from the reference."""
import numpy as np
import pytest

import bm25_oracle as O
import bm25_replay as R
import bm25_synth as S
from rag_dpo_amd import bm25

pytestmark = pytest.mark.gpu
TILE = 4096


def offsets(qs):
    off = np.zeros(len(qs) + 1, np.int64)
    np.cumsum([len(q) for q in qs], out=off[1:])
    ids = np.concatenate([np.asarray(q, np.int32) for q in qs]) if off[-1] else np.zeros(0, np.int32)
    return off, ids


def same(arrays, qs, k, allow_bits=None, gpu=None):
    gpu = gpu or bm25.HipBm25(arrays, 0)
    off, ids = offsets(qs)
    g = gpu.search(off, ids, k, allow_bits)
    c = O.CpuBm25(arrays).search(off, ids, k, allow_bits)
    assert (g[2] == c[2]).all(), (g[2], c[2])
    for q in range(len(qs)):
        n = int(c[2][q])
        assert (g[1][q, :n] == c[1][q, :n]).all()
        assert (g[0][q, :n].view(np.int64) == c[0][q, :n].view(np.int64)).all()   # float64 bit equality
        assert (g[1][q, n:] == -1).all()
    return g


@pytest.fixture(scope="module")
def chunk():
    return R.chunk_index(None)          # librdx


@pytest.fixture(scope="module")
def summ(tmp_path_factory):
    return R.summary_index(None, str(tmp_path_factory.mktemp("summaries")))


def test_fixture_chunk_search(chunk):
    assert isinstance(chunk.engine, bm25.HipBm25)
    R.replay_chunk_search(chunk)
    rng = np.random.default_rng(1)
    words = list(chunk.model.term_id)
    qs = [chunk.model.query_ids(rng.choice(words, size=n)) for n in (1, 2, 5, 17, 300)]
    same(chunk.model.arrays(), qs, 50, gpu=chunk.engine)


def test_fixture_summary_search(summ):
    R.replay_summary(summ)


def test_fixture_hybrid_retriever_on_librdx(summ, chunk):
    R.replay_retriever(None, summ, chunk)


def test_reference_shape():
    a = S.make(16919, 30000, 120, seed=2)
    same(a, [S.query(30000, 9, 3)], 50)


@pytest.mark.parametrize("n", [TILE - 1, TILE, TILE + 1, 3 * TILE + 7])
def test_tile_edges(n):
    a = S.make(n, 500, 30, seed=n, every_row_term=0)
    same(a, [S.query(500, 6, n), [0], [499, 0, 0], [7]], 20)
    same(a, [[0]], 4096)                 # a term in every row: every row passes, ties everywhere, k = 4096 (= one whole tile)


def test_long_query_and_k_edges():
    a = S.make(20000, 3000, 60, seed=4)
    q600 = S.query(3000, 600, 5)
    same(a, [q600], 50)
    same(a, [S.query(3000, 4096, 6)], 10)          # the longest query accepted
    same(a, [q600[:3]], 1)
    rare = [2999, 2998]
    g = same(a, [rare], 4096)                      # k above the rows with a positive score
    assert g[2][0] < 4096


def test_group_filter():
    a = S.make(30000, 2000, 50, seed=8, groups=300)
    gpu = bm25.HipBm25(a, 0)
    rng = np.random.default_rng(9)
    for n_allowed in (1, 7, 150, 300):
        bits = np.zeros((300 + 31) // 32, np.uint32)
        for gid in rng.choice(300, n_allowed, replace=False):
            bits[gid >> 5] |= np.uint32(1 << (gid & 31))
        same(a, [S.query(2000, 5, n_allowed), S.query(2000, 40, n_allowed + 1)], 64, bits, gpu)
    same(a, [S.query(2000, 5, 0)], 64, np.zeros(10, np.uint32), gpu)   # nothing allowed


def test_batched_equals_single_and_is_deterministic():
    a = S.make(40000, 5000, 80, seed=12)
    gpu = bm25.HipBm25(a, 0)
    qs = [S.query(5000, n, 20 + n) for n in (1, 4, 12, 33)]
    b = same(a, qs, 100, gpu=gpu)
    for i, q in enumerate(qs):
        s = gpu.search(*offsets([q]), 100)
        assert (s[2][0] == b[2][i]) and (s[1][0] == b[1][i]).all() and (s[0][0].view(np.int64) == b[0][i].view(np.int64)).all()
    again = gpu.search(*offsets(qs), 100)
    assert all((x.view(np.uint8) == y.view(np.uint8)).all() for x, y in zip(again, b))


def test_one_million_rows():
    a = S.make(1_000_000, 50000, 40, seed=13)
    same(a, [S.query(50000, 8, 14), S.query(50000, 3, 15)], 50)
    same(a, [S.query(50000, 4, 16)], 4096)


def test_argument_errors_are_clean():
    a = S.make(5000, 300, 20, seed=30)
    gpu = bm25.HipBm25(a, 0)
    good = gpu.search(*offsets([[1, 2]]), 10)
    for qs, k, msg in (([[1, 300]], 10, "term id"), ([[-1]], 10, "term id"), ([[1]], 0, "k"), ([[1]], 4097, "k"),
                       ([list(range(300)) * 14], 10, "terms")):
        with pytest.raises(ValueError, match=msg):
            gpu.search(*offsets(qs), k)
    with pytest.raises(ValueError, match="group"):
        gpu.search(*offsets([[1]]), 10, np.zeros(1, np.uint32))    # a group filter on an index without groups
    after = gpu.search(*offsets([[1, 2]]), 10)                    # nothing was launched with the bad arguments
    assert all((x.view(np.uint8) == y.view(np.uint8)).all() for x, y in zip(after, good))
