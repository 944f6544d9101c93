"""k_refine answers a spilling query in its own launch (DESIGN.md §5 "Spill list"): after the segment prefix a block with more
hits than the LDS list holds goes on with its row of the HBM spill buffer as the list; there is no second kernel and no queue.

Every query here is CONSTRUCTED, so that the number of its hits is known: query i is a random direction, and c_i near copies of
it (direction + 0.002 * noise) are stored at rows j * nq + i, j < c_i — consecutive copies lie in different 32-row blocks, so each
is a threshold set of its own, and with c_i >= 12 > k = 10 the threshold sits at the copies' level (cosine ~ 1; every other row of
the corpus scores below 0.5): the query has exactly c_i hits. With refine_list = 32 a query of 12 copies fits the LDS list and one
of 40 copies spills. All checks are ids, score bits and counts against the C oracle, plus the counters of the search.

Two things the wording of the cases could not be met by, and what is tested instead:
- "one over spill_cap (the spill_cap = 32 developer option)": with refine_list = 32 (the option's minimum) and spill_cap = 32 no
  query can spill at all (a spilling query has 32 < m <= spill_cap). The search of four kinds runs with spill_cap = 64: 12 copies
  fit the list, 40 spill, 70 exceed the spill list, and a query with six extra copies inside one 256-row tile overflows a segment
  of cand_cap = 4 slots.
- "a query with zero hits": no search through the API has one next to a query with hits — the threshold is a sampled score (minus
  a slack), and the row that set it is emitted, so m >= 1 whenever any row is allowed; and k = 0 is answered by the exact path
  before any plan is made. Both are searched here (k = 0, and a bitmap that allows no row of the corpus: m = 0 for every query of
  a plan that spills), the m == 0 / k == 0 statement of the kernel being shared by the two routes."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROWS = 12_400
FIT, SPILL, OVER = 12, 40, 70       # copies: <= refine_list = 32 < SPILL <= spill_cap = 64 < OVER
_cache = {}


@pytest.fixture(scope="module")
def eng():
    from rag_dpo_amd import engine
    return engine


@pytest.fixture(autouse=True)
def _debug_hits(monkeypatch):
    monkeypatch.setenv("RDX_DEBUG_HITS", "1")


def _build(d, nq, sizes, extra=()):
    """corpus and queries: sizes[i] near copies of query i at rows j * nq + i; extra: (query, rows) more copies at the given rows"""
    assert max(sizes) * nq <= ROWS
    rng = np.random.default_rng([d, nq, sum(sizes)])
    corpus = rng.standard_normal((ROWS, d), dtype=np.float32)
    q = rng.standard_normal((nq, d), dtype=np.float32)
    for i, c in enumerate(sizes):
        rows = np.arange(c) * nq + i
        corpus[rows] = q[i] + 0.002 * rng.standard_normal((c, d), dtype=np.float32)
    for i, rows in extra:
        corpus[rows] = q[i] + 0.002 * rng.standard_normal((len(rows), d), dtype=np.float32)
    return corpus, q


def _case(oracle, tag, d, nq, sizes, extra=(), k=10):
    """(corpus, queries, the oracle's answer), built once per case and shared by the fp16 and the int8 run"""
    key = (tag, d, nq, k)
    if key not in _cache:
        corpus, q = _build(d, nq, sizes, extra)
        _cache[key] = (corpus, q, oracle.cosine_topk(oracle.normalize_rows(corpus), q, k, None))
    return _cache[key]


def _index(eng, corpus, i8, **opts):
    ix = eng.HipIndex(corpus.shape[1])
    ix.set_option("coarse_i8", 1 if i8 else 0)
    if not i8:
        ix.set_option("force_fast", 1)
    ix.set_option("spec_tau", 0)             # the proven threshold: the k-th sampled score minus the slack, whatever the history
    for name, v in opts.items():
        ix.set_option(name, v)
    ix.add(corpus)
    return ix


def _search(capfd, ix, ref, q, k, i8, allow_bits=None):
    capfd.readouterr()
    gs, gr, gc = ix.search(q, k, allow_bits)
    st = ix.last_stats()
    found = re.findall(r"hits max (\d+) spilled (\d+)", capfd.readouterr().err)
    assert found, "the library did not print its RDX_DEBUG_HITS line"
    longest, spilled = max(int(a) for a, _ in found), sum(int(b) for _, b in found)
    print(f"nq {q.shape[0]} k {k} i8 {i8}: emitted {st['emitted']} rescored {st['rescored']} retried {st['retried_queries']} "
          f"exact {st['exact_queries']} longest {longest} spilled {spilled}")
    if ref is not None:
        es, er, ec = ref
        np.testing.assert_array_equal(gc, ec)
        np.testing.assert_array_equal(gr, er)
        np.testing.assert_array_equal(gs, es)
        assert st["coarse_bits"] == (8 if i8 else 16) and st["path"] == 0, st
    return st, longest, spilled, (gs, gr, gc)


def _two_runs(eng, oracle, capfd, tag, d, nq, sizes, i8):
    """refine_spill = 0 with the automatic list, then refine_spill = 1 with refine_list = 32, on one index"""
    corpus, q, ref = _case(oracle, tag, d, nq, sizes)
    ix = _index(eng, corpus, i8, refine_spill=0, refine_list=0)
    a, _, sp_a, _ = _search(capfd, ix, ref, q, 10, i8)
    ix.set_option("refine_spill", 1)
    ix.set_option("refine_list", 32)
    b, longest, sp_b, _ = _search(capfd, ix, ref, q, 10, i8)
    ix.close()
    assert sp_a == 0 and a["retried_queries"] == 0 and a["exact_queries"] == 0, (sp_a, a)
    assert b["retried_queries"] == 0 and b["exact_queries"] == 0, b
    assert a["emitted"] == b["emitted"] == sum(sizes), (a, b, sum(sizes))
    assert a["rescored"] == b["rescored"], (a, b)
    assert sp_b == sum(1 for c in sizes if c > 32) and longest == max(sizes), (sp_b, longest)
    return b


@pytest.mark.parametrize("i8", [True, False])
@pytest.mark.parametrize("d,nq", [(128, 129), (128, 257), (1024, 129), (1024, 257)])
def test_spilling_and_fitting_queries_alternate(eng, oracle, capfd, d, nq, i8):
    _two_runs(eng, oracle, capfd, "alt", d, nq, [SPILL if i % 2 == 0 else FIT for i in range(nq)], i8)


@pytest.mark.parametrize("i8", [True, False])
@pytest.mark.parametrize("d,nq", [(128, 257), (1024, 129)])
@pytest.mark.parametrize("which", ["first", "last"])
def test_one_query_spills(eng, oracle, capfd, which, d, nq, i8):
    at = 0 if which == "first" else nq - 1
    _two_runs(eng, oracle, capfd, which, d, nq, [SPILL if i == at else FIT for i in range(nq)], i8)


@pytest.mark.parametrize("i8", [True, False])
@pytest.mark.parametrize("d,nq", [(128, 257), (1024, 129)])
@pytest.mark.parametrize("size", [SPILL, FIT])
def test_every_query_spills_or_none_and_the_search_is_finished(eng, oracle, capfd, size, d, nq, i8):
    """the end-of-search work runs in k_refine's last block for every plan: counts, results and the stats struct are there"""
    b = _two_runs(eng, oracle, capfd, f"all{size}", d, nq, [size] * nq, i8)
    assert b["emitted"] == size * nq and b["rescored"] >= 10 * nq, b


@pytest.mark.parametrize("i8", [True, False])
@pytest.mark.parametrize("d", [128, 1024])
def test_four_routes_in_one_search(eng, oracle, capfd, d, i8):
    """list, spill, fallback (more hits than the spill list), fallback (a segment overflowed): one query each, the others fit"""
    nq = 129
    sizes = [FIT] * nq
    sizes[3], sizes[64] = SPILL, OVER
    tile = 10_240 + 5                           # six more copies of query 128 in six 32-row blocks of ONE 256-row tile
    extra = [(128, tile + 32 * np.arange(6))]
    corpus, q, ref = _case(oracle, "four", d, nq, sizes, extra)
    ix = _index(eng, corpus, i8, refine_spill=1, refine_list=32, spill_cap=64, cand_cap=4)
    st, longest, spilled, _ = _search(capfd, ix, ref, q, 10, i8)
    ix.close()
    assert spilled == 1, (spilled, st)
    assert st["retried_queries"] == 2, st      # (what the second pass does with the two is its own plan's business)
    assert longest >= OVER, longest


@pytest.mark.parametrize("i8", [True, False])
def test_k_zero_and_no_allowed_row(eng, oracle, capfd, i8):
    d, nq = 128, 129
    corpus, q, ref = _case(oracle, "alt", d, nq, [SPILL if i % 2 == 0 else FIT for i in range(nq)])
    ix = _index(eng, corpus, i8, refine_spill=1, refine_list=32)
    gs, gr, gc = ix.search(q, 0)
    assert gs.shape == (nq, 0) and gr.shape == (nq, 0) and not gc.any()
    none = np.zeros(ROWS, dtype=bool)
    st, longest, spilled, (gs, gr, gc) = _search(capfd, ix, None, q, 10, i8, oracle.pack_mask(none, ROWS))
    assert not gc.any() and (gr == -1).all() and st["emitted"] == 0 and (longest, spilled) == (0, 0), (st, longest, spilled)
    _search(capfd, ix, ref, q, 10, i8)          # and the index answers the spilling search afterwards
    ix.close()
