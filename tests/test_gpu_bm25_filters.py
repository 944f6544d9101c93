"""GPU: a filter per query in one BM25 search (rdx_bm25_search_filtered through rag_dpo_amd.bm25.HipBm25.search_filtered). Every
comparison is bit equality of rows, counts and float64 score bits: with rdx_bm25_search called for the query alone with its one set
(the path tests/test_gpu_bm25_edges.py pins) and with bm25_oracle.CpuBm25. What is new and can be wrong is the table's address
arithmetic (row * allow_words, the word of a group) and the offset of query_filter in the second and third launch of one search;
the shapes are the smallest that reach them.

One property the cases cannot have: under the set of all ones a query's result IS its unfiltered result, so for that set the CPU
pre-check asserts equality with the unfiltered result (and a difference from every other set) instead of a difference."""
import ctypes
import dataclasses

import numpy as np
import pytest

import bm25_model as M
import bm25_oracle as O
import bm25_replay as R
import bm25_synth as S
from bm25_replay import W
from rag_dpo_amd import _lib as L
from rag_dpo_amd import bm25
from rag_dpo_amd.retriever import DenseRetriever

pytestmark = pytest.mark.gpu

# ---- words and sets: 2 tiles (the second ragged), 70 groups = 3 words (the last ragged) ---------------------------------------------
N_ROWS, GROUPS, WORDS = M.TILE + 37, 70, 3
SETS = np.stack([M.bits_of([31], WORDS), M.bits_of([32], WORDS), M.bits_of([63, 64, 69], WORDS), M.bits_of([], WORDS),
                 np.full(WORDS, 0xFFFFFFFF, np.uint32)])
ALL_ONES = 4
QUERY_FILTER = np.array([-1, 0, 1, 0, 2, -1, 3, 4, 1], np.int32)
# every query holds a term of thousands of rows: each group has more than 3 passing rows in tile 0
QS = [[2, 7, 2], [3, 30], [4, 59, 12, 4], [2, 5], [9, 3, 9, 20], [15, 4], [6, 11, 5], [8, 2, 40], [13, 3]]


def cpu_search(a, qs, k, sets, query_filter):
    """CpuBm25 per query under its own set -> (scores, rows, counts) as one search returns them; the scores are computed once"""
    cpu = O.CpuBm25(a)
    nq = len(qs)
    sc, ro, cn = np.zeros((nq, k)), np.full((nq, k), -1, np.int64), np.zeros(nq, np.int32)
    allow = [np.unpackbits(s.view(np.uint8), bitorder="little").astype(bool)[a.row_group] for s in sets]
    for q, ids in enumerate(qs):
        f = int(query_filter[q])
        rows, s = O.topk(cpu.scores(ids), k, None if f < 0 else allow[f])
        cn[q], ro[q, :len(rows)], sc[q, :len(rows)] = len(rows), rows, s
    return sc, ro, cn


def same(got, want, what):
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape, what
    bad = np.flatnonzero(got[2] != want[2])
    assert bad.size == 0, (what, "counts", bad[:8], got[2][bad[:8]], want[2][bad[:8]])
    bad = np.flatnonzero((got[1] != want[1]).any(axis=1))
    assert bad.size == 0, (what, "rows", bad[:8])
    bad = np.flatnonzero((got[0].view(np.int64) != want[0].view(np.int64)).any(axis=1))
    assert bad.size == 0, (what, "score bits", bad[:8])


@pytest.fixture(scope="module")
def small():
    a = S.make(N_ROWS, 60, 12, seed=61, groups=GROUPS)
    assert M.n_tiles(a.n_rows) == 2 and a.n_rows % M.TILE == 37 and (a.n_groups + 31) // 32 == WORDS and a.n_groups % 32
    gpu = bm25.HipBm25(a, 0)
    yield a, gpu
    gpu.close()


@pytest.mark.parametrize("k", [3, M.MAX_K])
def test_each_query_has_its_own_set(small, k):
    a, gpu = small
    want = cpu_search(a, QS, k, SETS, QUERY_FILTER)
    # first, on the CPU: these inputs tell a wrong set from the right one
    for q, f in enumerate(QUERY_FILTER.tolist()):
        if f < 0:
            continue
        mine = M.result_of(want, q)
        free = M.result_of(cpu_search(a, [QS[q]], k, SETS, [-1]), 0)
        assert (mine == free) if f == ALL_ONES else (mine != free), (q, f)
        for other in range(len(SETS)):
            if other != f:
                assert M.result_of(cpu_search(a, [QS[q]], k, SETS, [other]), 0) != mine, (q, f, other)
    passing = [int((O.CpuBm25(a).scores(ids) > 0).sum()) for ids in QS]
    if k == 3:     # tiles with more than k passing rows: the tile top-k and the merge cut
        assert want[2][QUERY_FILTER != 3].min() == 3 and want[2][6] == 0
        in_tile0 = [(O.topk(O.CpuBm25(a).scores(QS[q]), N_ROWS, np.unpackbits(SETS[f].view(np.uint8), bitorder="little").astype(bool)[a.row_group])[0]
                     < M.TILE).sum() for q, f in enumerate(QUERY_FILTER.tolist()) if f in (0, 1, 2)]
        assert min(in_tile0) > 3
    else:          # every passing row of every query is compared
        assert max(passing) <= k and (want[2] < k).all() and want[2][7] == passing[7]

    got = gpu.search_filtered(*M.offsets(QS), k, SETS, QUERY_FILTER)
    same(got, want, "CpuBm25")
    past = np.arange(k)[None, :] >= want[2][:, None]
    assert (got[1][past] == -1).all() and (got[0].view(np.int64)[past] == 0).all()
    for q, f in enumerate(QUERY_FILTER.tolist()):       # the single-set path, the query alone
        alone = gpu.search(*M.offsets([QS[q]]), k, None if f < 0 else SETS[f])
        same([x[q:q + 1] for x in got], alone, ("rdx_bm25_search alone", q, f))


def test_no_sets_is_the_unfiltered_search(small):
    a, gpu = small
    off, ids = M.offsets(QS)
    want = gpu.search(off, ids, 50, None)
    assert want[2].min() > 3
    same(gpu.search_filtered(off, ids, 50, None, np.full(len(QS), -1, np.int32)), want, "n_filters = 0")
    same(gpu.search_filtered(off, ids, 50, SETS, np.full(len(QS), -1, np.int32)), want, "a table nobody uses")
    sc, ro, cn = gpu.search_filtered(np.zeros(1, np.int64), np.zeros(0, np.int32), 5, SETS, np.zeros(0, np.int32))
    assert sc.shape == (0, 5) and ro.shape == (0, 5) and cn.shape == (0,)


def raw_call(gpu, qs, k, sets, n_filters, query_filter):
    """rdx_bm25_search_filtered itself, on outputs filled with a sentinel -> (rc, message, the outputs are untouched)"""
    off, ids = M.offsets(qs)
    nq = len(qs)
    sc, ro, cn = np.full((nq, k), 7.5), np.full((nq, k), 77, np.int64), np.full(nq, 777, np.int32)
    ptr = lambda x: ctypes.c_void_p(x.ctypes.data) if x is not None else None      # noqa: E731
    rc = gpu._lib.rdx_bm25_search_filtered(gpu._h, ptr(off), ptr(ids), nq, k, ptr(sets), n_filters, ptr(query_filter), ptr(sc), ptr(ro),
                                           ptr(cn), L.RDX_HOST, None)
    return rc, L.last_error(), bool((sc == 7.5).all() and (ro == 77).all() and (cn == 777).all())


def test_refusals_write_nothing(small):
    a, gpu = small
    qs = QS[:3]
    i32 = lambda *v: np.array(v, np.int32)      # noqa: E731
    for what, sets, n_filters, qf, words in (
            ("an entry equal to n_filters", SETS, 5, i32(0, 5, -1), ("query_filter[1]", "5")),
            ("an entry of -2", SETS, 5, i32(4, 0, -2), ("query_filter[2]", "-2")),
            ("a null table", None, 1, i32(0, 0, 0), ("filter_sets", "n_filters = 1")),
            ("a null query_filter", SETS, 5, None, ("query_filter", "nq = 3"))):
        rc, msg, untouched = raw_call(gpu, qs, 4, sets, n_filters, qf)
        assert rc == L.RDX_ERR_INVALID and untouched, what
        assert msg.startswith("rdx_bm25_search_filtered:") and all(w in msg for w in words), (what, msg)
    plain = bm25.HipBm25(dataclasses.replace(a, row_group=None, n_groups=0), 0)
    try:
        rc, msg, untouched = raw_call(plain, qs, 4, SETS, 1, i32(-1, -1, -1))
        assert rc == L.RDX_ERR_INVALID and untouched and "without groups" in msg, msg
        rc, msg, untouched = raw_call(plain, qs, 4, None, 0, i32(-1, -1, -1))           # no table: the group-less index answers
        assert rc == L.RDX_OK and not untouched
    finally:
        plain.close()
    with pytest.raises(ValueError, match="query_filter has 2 entries for 3 queries"):
        gpu.search_filtered(*M.offsets(qs), 4, SETS, i32(0, 0))
    with pytest.raises(ValueError, match="filter_sets must be"):
        gpu.search_filtered(*M.offsets(qs), 4, SETS[:, :2], i32(0, 0, 0))
    same(gpu.search_filtered(*M.offsets(qs), 4, SETS, i32(0, 4, -1)), cpu_search(a, qs, 4, SETS, [0, 4, -1]), "after the refusals")


def test_query_filter_follows_the_launches():
    """64 tiles at k = 4096: 85 queries per launch, 2 * 85 + 3 queries = three launches. query_filter[i] and query_filter[i + 85]
    always differ, so a launch that read query_filter from the start again returns another query's set"""
    case = M.case("workspace-chunks")
    (run,) = case.runs
    chunk, nq, k = case.facts["chunk"], len(run.qs), run.k
    assert chunk == 85 and nq == 2 * 85 + 3 and M.plan(case.a.n_rows, k, nq) == [(0, 85), (85, 85), (170, 3)]
    a = dataclasses.replace(case.a, row_group=np.random.default_rng(62).integers(0, GROUPS, case.a.n_rows).astype(np.int32), n_groups=GROUPS)
    rng = np.random.default_rng(63)
    sets = np.stack([M.bits_of(rng.choice(GROUPS, n, replace=False).tolist(), WORDS) for n in (9, 30, 50)])
    i = np.arange(nq)
    qf = ((i + 2 * (i // chunk)) % 4 - 1).astype(np.int32)
    assert set(qf.tolist()) == {-1, 0, 1, 2} and (qf[:-chunk] != qf[chunk:]).all() and (qf[:3] != qf[2 * chunk:]).all()
    want = cpu_search(a, run.qs, k, sets, qf)
    rewound = cpu_search(a, run.qs, k, sets, qf[i % chunk])       # what a launch without the offset would return
    differ = np.array([M.result_of(want, q) != M.result_of(rewound, q) for q in range(nq)])
    assert (np.flatnonzero(~differ[chunk:]) + chunk).tolist() == sorted(case.facts["empty"])      # all but the queries without terms
    gpu = bm25.HipBm25(a, 0)
    try:
        same(gpu.search_filtered(*M.offsets(run.qs), k, sets, qf), want, "three launches")
    finally:
        gpu.close()


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def test_the_batch_path_makes_one_bm25_call(tmp_path):
    """six questions with pairwise different summary filters: one chunk-BM25 engine call for the batch, and the loop's candidates"""
    from test_gpu_fusion import DeviceHashEmbedder, chunk_values
    col = W.build_collection(None)
    chunk = R.chunk_index(None)
    summ = R.summary_index(None, str(tmp_path))
    queries = [W.Q0, "registre des traitements du sous-traitant article 28", "notification d'une violation en 72 heures",
               "biométrie badge salariés", "consentement cookies prospection", "transfert union européenne"]
    r = DenseRetriever(col, DeviceHashEmbedder(), query_expander=W.expander, summary_bm25_index=summ, chunk_bm25_index=chunk, fusion="device")
    filters = [r._doc_filter(r._expand(q)[0]) for q in queries]
    assert all(filters) and len({frozenset(f) for f in filters}) == len(queries) == 6
    calls = []
    eng = chunk.engine
    for name in ("search", "search_filtered"):
        def counted(*args, _real=getattr(eng, name), _name=name, **kw):
            calls.append((_name, len(args[0]) - 1))
            return _real(*args, **kw)
        setattr(eng, name, counted)
    try:
        got = r.retrieve_candidates_batch(queries, n_candidates=40)
        assert calls == [("search_filtered", 24)]                      # 6 questions x 4 sub-queries, 6 sets, one call
        calls.clear()
        loop = [r.retrieve_candidates(q, n_candidates=40) for q in queries]
        assert len(calls) == 6
    finally:
        del eng.search, eng.search_filtered
    assert all(len(g) > 0 for g in got)
    for g, l in zip(got, loop):
        assert [chunk_values(c) for c in g] == [chunk_values(c) for c in l]
