"""The slot claims of the scan's emit path (scan_kernel.hpp emit_block): a lane tests its eight accumulators of a
block and claims a slot of the (query, stream) segment from an LDS counter for every hit; the four lanes of a query column claim
on the same counter. The cases are placed by the kernel's lane layout: lane group g of a wave's 32-row block owns rows
4g .. 4g + 3 (accumulator half 0) and 16 + 4g .. 16 + 4g + 3 (half 1). (Written with a form of emit_block that counted a lane's
hits first and claimed them with one atomic; that form measured slower and was not kept — DESIGN.md §4 — the cases hold for any.)

One corpus per dim holds three constructions, each an EXACT copy of a query direction at chosen rows of one 32-row block:
  A  all 8 rows of lane group 2 of a block;
  B  all 32 rows of a block (the four lanes of a query column claim on the same counter);
  C  one row in each half of lane group 1: exactly one accumulator of each half.
Each direction also has 12 "anchor" rows, identical copies of direction + 0.3 |direction| noise (cosine 0.96), 257 rows apart, so
each in a 32-row block — a threshold set — of its own: the k = 10 threshold lies at the anchors' score, every other row of the
corpus scores below 0.5, and a query's hits are exactly its construction's rows and its anchors. The 129 queries are the three
directions in turn (more than 128: the int8 pass), so every query column of the tile claims.

Each case runs on fp16 and int8 (coarse_i8 = 1), with fuse_epilogue 0 and 1, and with a `where` bitmap that masks some of the
constructed rows; ids, score bits and counts are the C oracle's and `emitted` is the number of constructed rows the bitmap lets
through. The last case makes a segment hold 5 slots (cand_cap): A's eight rows cross it in the middle of one lane's claims, B's 32
cross it too; both are flagged and answered by the fallback pass."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROWS = 12_400
NQ = 129
N_ANCH = 12
BASE = {"A": 2048, "B": 4096 + 64, "C": 6144 + 96}          # first rows of the three 32-row blocks
MASKED = {"A": [9, 26], "B": [0, 5, 17, 30, 31], "C": [20]}    # rows of the block (offsets) the bitmap case takes out
_cache = {}


def _rows(kind):
    if kind == "A":
        off = [4 * 2 + r for r in range(4)] + [16 + 4 * 2 + r for r in range(4)]
    elif kind == "B":
        off = list(range(32))
    else:
        off = [4 * 1 + 3, 16 + 4 * 1 + 0]
    return np.array(off)


@pytest.fixture(scope="module")
def eng():
    from rag_dpo_amd import engine
    return engine


def _data(oracle, d, masked):
    key = (d, masked)
    if key not in _cache:
        rng = np.random.default_rng([77, d])
        corpus = rng.standard_normal((ROWS, d), dtype=np.float32)
        dirs = rng.standard_normal((3, d), dtype=np.float32)
        allow = np.ones(ROWS, dtype=bool)
        hits = {}
        for j, kind in enumerate("ABC"):
            rows = BASE[kind] + _rows(kind)
            corpus[rows] = dirs[j]
            noise = rng.standard_normal(d).astype(np.float32)
            anchor = dirs[j] + 0.3 * np.linalg.norm(dirs[j]) * noise / np.linalg.norm(noise)
            arows = 7000 + 257 * np.arange(N_ANCH) + j
            corpus[arows] = anchor
            if masked:
                allow[BASE[kind] + np.array(MASKED[kind])] = False
            hits[kind] = int(allow[rows].sum()) + N_ANCH
        q = np.stack([dirs[i % 3] for i in range(NQ)])
        want = sum(hits["ABC"[i % 3]] for i in range(NQ))
        a = allow if masked else None
        _cache[key] = (corpus, q, a, want, oracle.cosine_topk(oracle.normalize_rows(corpus), q, 10, a))
    return _cache[key]


def _index(eng, corpus, i8, fuse, **opts):
    ix = eng.HipIndex(corpus.shape[1])
    ix.set_option("coarse_i8", 1 if i8 else 0)
    if not i8:
        ix.set_option("force_fast", 1)
    ix.set_option("spec_tau", 0)              # the proven threshold (k-th sampled score minus the slack), whatever the history
    ix.set_option("fuse_epilogue", fuse)
    for name, v in opts.items():
        ix.set_option(name, v)
    ix.add(corpus)
    return ix


def _search(oracle, ix, data, i8):
    corpus, q, allow, want, (es, er, ec) = data
    gs, gr, gc = ix.search(q, 10, None if allow is None else oracle.pack_mask(allow, ROWS))
    st = ix.last_stats()
    print(f"i8 {i8}: emitted {st['emitted']} (constructed {want}) rescored {st['rescored']} retried {st['retried_queries']} "
          f"exact {st['exact_queries']}")
    np.testing.assert_array_equal(gc, ec)
    np.testing.assert_array_equal(gr, er)
    np.testing.assert_array_equal(gs, es)
    assert st["coarse_bits"] == (8 if i8 else 16) and st["path"] == 0, st
    return st


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("fuse", [0, 1])
@pytest.mark.parametrize("i8", [False, True])
@pytest.mark.parametrize("d", [128, 1024])
def test_one_lane_one_block_one_accumulator_per_half(eng, oracle, d, i8, fuse, masked):
    data = _data(oracle, d, masked)
    ix = _index(eng, data[0], i8, fuse)
    st = _search(oracle, ix, data, i8)
    ix.close()
    assert st["retried_queries"] == 0 and st["exact_queries"] == 0, st
    assert st["emitted"] == data[3], (st["emitted"], data[3])


@pytest.mark.parametrize("fuse", [0, 1])
@pytest.mark.parametrize("i8", [False, True])
@pytest.mark.parametrize("d", [128, 1024])
def test_capacity_crossed_inside_one_claim(eng, oracle, d, i8, fuse):
    """segments of 5 slots: the lane of A claims 8 (slots 0 .. 7: the stores at 5, 6, 7 are dropped), the block of B 32; the queries
    of A and B are flagged and the fallback pass answers them, the queries of C (two hits in that segment) are not"""
    data = _data(oracle, d, False)
    ix = _index(eng, data[0], i8, fuse, cand_cap=5)
    st = _search(oracle, ix, data, i8)
    ix.close()
    assert st["retried_queries"] == 2 * (NQ // 3) and st["exact_queries"] == 0, st
