"""GPU: the threshold search called directly (rag_dpo_amd.engine.range_search -> rdx_index_range -> k_range_tau, the main scan,
k_range_refine / k_range_select_dense) on a HipIndex, scores, rows, counts and totals byte for byte against the definition over the
oracle's exact scores.

Shapes. dims 64, 260, 1024 (1, 5 and 16 k-steps; 260 pads its last k-step). 600 rows: the main scan is k_scan<EPI_EMIT> (fewer 32-row
blocks than workgroups), with 64, 128 and 256 queries per workgroup at 1 / 3, 65 and 130 queries. 8 229 rows = 258 blocks: under
force_fast 1 and 3 queries run k_scan_small, 65 and 130 k_scan again. Every case runs as planned, with force_exact and with force_fast,
and the three must give the same bytes; the test restates the plan's small-problem rule to know which path "as planned" is.

World (tests/test_gpu_mmr_kernel.py's): a common component, ten tight clusters (rows 200..399), eleven exact copies of row 7 (rows
100..110), two zero rows. Thresholds, each computed from the oracle's scores and CHECKED on the CPU before anything runs (combos()):
a row's own score (the row and every copy of it are in, row ascending) and the next float above it (all out); the median score of a
cluster (rows within E on both sides); above the best score (nothing in range); the m-th, (m + 1)-th and 3 m-th best score (total > count); the copies'
score with m = 5 (the cut falls inside the tie); -2 (every allowed row); a mask that removes the best rows and some copies.
MFMA-path cases keep every query's possible hits — allowed rows with exact score >= t - 2E - 1e-6: the scan may emit those — at or below
4 096 and assert paths == [nq, 0]. Overflow cases assert the number of queries that fell back: cand_cap = 32 and refine_list = 32
(queries with more than 32 rows IN range overflow for certain, queries with at most 32 possible hits certainly do not, and no other
kind is in the batch), and -2 at 8 229 rows (more hits than the list's 7 168)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32 = np.float32
TWIN, COPIES, ZEROS = 7, list(range(100, 111)), [20, 21]
DIMS = [64, 260, 1024]
ROWS = [600, 8229]
BATCHES = [1, 3, 65, 130]


def two_e(dim):
    dim_pad = (dim + 63) // 64 * 64
    return F32(2.0) * (F32(1.0e-3) + F32(2.5e-7) * F32(dim_pad))                    # rdx_index::two_e()


def world(dim, n_rows):
    rng = np.random.default_rng(dim * 100003 + n_rows)
    common = rng.standard_normal(dim).astype(np.float32)
    x = (0.7 * common[None, :] + rng.standard_normal((n_rows, dim))).astype(np.float32)
    x[200:400] = x[200:400:20].repeat(20, axis=0) + 0.05 * rng.standard_normal((200, dim)).astype(np.float32)   # ten tight clusters
    x[COPIES] = x[TWIN]
    x[ZEROS] = 0.0
    q = (0.7 * common[None, :] + rng.standard_normal((3, dim))).astype(np.float32)
    q[1] = x[TWIN] + 0.1 * rng.standard_normal(dim).astype(np.float32)              # the copies are this query's best rows
    q[2] = x[205] + 0.1 * rng.standard_normal(dim).astype(np.float32)               # a cluster is this one's
    return x, q


def mask_for(sc, n_rows):
    """allow bitmap: every third row gone, and query 0's ten best rows, the twin and every other copy with them; five copies stay"""
    allow = np.arange(n_rows) % 3 != 1
    allow[np.argsort(-sc[0], kind="stable")[:10]] = False
    allow[COPIES[1::2]] = True
    allow[[TWIN] + COPIES[::2]] = False
    return allow


def expected(sc, allow, t, m):
    """the definition: allowed rows with score >= t, (score descending, row ascending), total, the first m"""
    ok = sc >= F32(t)
    if allow is not None:
        ok &= allow
    rows = np.flatnonzero(ok)
    rows = rows[np.lexsort((rows, -sc[rows].astype(np.float64)))]
    n = min(m, len(rows))
    s = np.full(m, -np.inf, dtype=np.float32)
    r = np.full(m, -1, dtype=np.int64)
    s[:n], r[:n] = sc[rows[:n]], rows[:n]
    return s, r, n, len(rows)


def possible_hits(sc, allow, t, dim):
    """allowed rows the scan may emit for threshold t: coarse >= fl_down(t - E) and |coarse - exact| <= E"""
    ok = sc.astype(np.float64) >= float(t) - float(two_e(dim)) - 1e-6
    if allow is not None:
        ok &= allow
    return int(np.count_nonzero(ok))


def up(x):
    return np.nextafter(F32(x), F32(np.inf))


def combos(sc, allow, m, dim, n_rows):
    """[(query, threshold, kind)] — the distinct (query, threshold) pairs of a case, their claims checked here on the CPU"""
    def ranked(b):
        rows = np.flatnonzero(allow) if allow is not None else np.arange(n_rows)
        return rows[np.lexsort((rows, -sc[b][rows].astype(np.float64)))]

    def total(b, t):
        return expected(sc[b], allow, t, m)[3]

    out = []
    E = float(two_e(dim)) / 2
    live_copies = [r for r in [TWIN] + COPIES if allow is None or allow[r]]
    t_copy = sc[1][live_copies[0]]
    assert all(sc[1][r] == t_copy for r in live_copies)                             # identical rows, identical bits
    r1 = ranked(1)
    assert r1[: len(live_copies)].tolist() == live_copies                           # query 1's best rows, row ascending
    out.append((1, t_copy, "a row's own score: it and its copies"))
    assert total(1, t_copy) == len(live_copies) >= 5
    out.append((1, up(t_copy), "the next float above: all out"))
    assert total(1, up(t_copy)) == 0
    cl = np.asarray([r for r in range(200, 220) if allow is None or allow[r]])
    t_cl = np.sort(sc[2][cl])[len(cl) // 2]
    near = sc[2][cl].astype(np.float64) - float(t_cl)
    assert ((near < 0) & (near > -E)).any() and ((near > 0) & (near < E)).any(), "the cluster has rows within E on both sides of t"
    out.append((2, t_cl, "inside a cluster"))
    r0 = ranked(0)
    out.append((0, up(sc[0][r0[0]]), "above the best score: nothing"))
    assert total(0, out[-1][1]) == 0
    for rank, kind in ((m, "exactly m"), (m + 1, "m + 1"), (3 * m, "3 m")):
        # the rank-th best score of the first query whose ranking has no tie across that cut (the copies tie wherever they stand)
        fit = [(b, sc[b][ranked(b)[rank - 1]]) for b in (0, 2, 1)]
        fit = [(b, t) for b, t in fit if total(b, t) == rank]
        assert fit, kind
        out.append((fit[0][0], fit[0][1], kind))
    if n_rows <= 4096:
        out.append((2, F32(-2.0), "every allowed row"))
        assert total(2, -2.0) == (n_rows if allow is None else int(allow.sum()))
    for b, t, kind in out:
        assert possible_hits(sc[b], allow, t, dim) <= 4096, kind
    return out


def planned_exact(n_rows, nq):
    """plan_search's small-problem rule (search_plan.hpp), which plan_range keeps: the exact scan alone"""
    return n_rows <= 32768 and ((nq + 3) // 4) * (n_rows * 1.28e-3 + 10.0) <= 60.0


@pytest.fixture(scope="module")
def worlds(oracle):
    from rag_dpo_amd import engine as E
    made = {}

    def get(dim, n_rows):
        if (dim, n_rows) not in made:
            x, q = world(dim, n_rows)
            ix = E.HipIndex(dim)
            ix.add(x)
            hat, qhat = oracle.normalize_rows(x), oracle.normalize_rows(q)
            sc = [oracle.scores(hat, qhat[b]) for b in range(3)]
            allow = mask_for(sc, n_rows)
            bits = np.packbits(allow, bitorder="little")
            bits = np.concatenate([bits, np.zeros(-len(bits) % 4, np.uint8)]).view(np.uint32)
            made[(dim, n_rows)] = (ix, q, sc, allow, ix.make_mask(bits))
        return made[(dim, n_rows)]

    yield get
    for ix, _, _, _, mask in made.values():
        mask.close()
        ix.close()


def run(ix, q, order, m, mask=None, **options):
    import torch
    from rag_dpo_amd import engine as E
    dev = torch.device("cuda", 0)
    qs = np.stack([q[b] for b, _ in order]).astype(np.float32)
    thr = np.asarray([t for _, t in order], dtype=np.float32)
    for name, v in options.items():
        ix.set_option(name, v)
    try:
        s, r, c, t, paths = E.range_search(ix, torch.from_numpy(qs).to(dev), torch.from_numpy(thr).to(dev), m, mask)
    finally:
        for name in options:
            ix.set_option(name, 0)
    return s.cpu().numpy(), r.cpu().numpy(), c.cpu().numpy(), t.cpu().numpy(), paths


def check(got, order, sc, allow, m, what):
    s, r, c, t, _ = got
    assert s.dtype == np.float32 and r.dtype == np.int64 and c.dtype == np.int32 and t.dtype == np.int64
    assert s.shape == r.shape == (len(order), m)
    for i, (b, thr) in enumerate(order):
        ws, wr, wc, wt = expected(sc[b], allow, thr, m)
        assert (int(t[i]), int(c[i])) == (wt, wc), (what, i, b, float(thr))
        assert r[i].tolist() == wr.tolist(), (what, i, b, float(thr))
        assert s[i].tobytes() == ws.tobytes(), (what, i, b, float(thr))


def batch(distinct, nq, shift=0):
    """nq (query, threshold) pairs: the distinct ones over and over — a different threshold per query, the same pair at several places"""
    return [distinct[(i + shift) % len(distinct)][:2] for i in range(nq)]


@pytest.mark.parametrize("nq", BATCHES)
@pytest.mark.parametrize("n_rows", ROWS)
@pytest.mark.parametrize("dim", DIMS)
def test_three_ways_agree_with_the_definition(dim, n_rows, nq, worlds):
    ix, q, sc, allow, mask = worlds(dim, n_rows)
    for m in (5, 40):
        for al, mk in ((None, None), (allow, mask)):
            distinct = combos(sc, al, m, dim, n_rows)
            shifts = range(len(distinct)) if nq == 1 else (0, 3)                    # one pair alone: every distinct pair in turn
            for shift in shifts:
                order = batch(distinct, nq, shift)
                what = (dim, n_rows, nq, m, al is not None, shift)
                got = run(ix, q, order, m, mk)
                check(got, order, sc, al, m, what + ("planned",))
                assert got[4] == ([0, nq] if planned_exact(n_rows, nq) else [nq, 0]), what
                ex = run(ix, q, order, m, mk, force_exact=1)
                check(ex, order, sc, al, m, what + ("force_exact",))
                assert ex[4] == [0, nq], what
                fa = run(ix, q, order, m, mk, force_fast=1)
                check(fa, order, sc, al, m, what + ("force_fast",))
                assert fa[4] == [nq, 0], what                                       # the kernels' own answer: nobody fell back
                for a, b in zip(got[:4], ex[:4]):
                    assert a.tobytes() == b.tobytes()
                for a, b in zip(fa[:4], ex[:4]):
                    assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("n_rows", ROWS)
@pytest.mark.parametrize("dim", DIMS)
def test_a_list_longer_than_the_search_s_k_limit(dim, n_rows, worlds):
    """max_results = 300 > K_FAST_MAX: the MFMA path still answers; at 600 rows -2 returns more than 256 rows of one query"""
    ix, q, sc, allow, mask = worlds(dim, n_rows)
    m = 300
    distinct = [(b, t) for b, t, _ in combos(sc, allow, 40, dim, n_rows)]
    order = batch(distinct, 3, 5) + [(0, sc[0][np.argsort(-sc[0], kind="stable")[280]])]
    for al, mk in ((None, None), (allow, mask)):
        assert all(possible_hits(sc[b], al, t, dim) <= 4096 for b, t in order)
        fa = run(ix, q, order, m, mk, force_fast=1)
        check(fa, order, sc, al, m, (dim, n_rows, "m=300", al is not None))
        assert fa[4] == [len(order), 0]
        ex = run(ix, q, order, m, mk, force_exact=1)
        for a, b in zip(fa[:4], ex[:4]):
            assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("nq", [3, 65, 130])
@pytest.mark.parametrize("n_rows", ROWS)
@pytest.mark.parametrize("dim", DIMS)
def test_overflowing_queries_fall_back_and_nobody_else(dim, n_rows, nq, worlds):
    ix, q, sc, allow, mask = worlds(dim, n_rows)
    m = 40
    # few: at most 32 possible hits, spread or not, fit a segment of 32 slots and a list of 32; many: more than 32 rows in range
    few = [(b, t) for b, t, kind in combos(sc, None, 5, dim, n_rows) if possible_hits(sc[b], None, t, dim) <= 32]
    assert len(few) >= 3
    low = [(0, F32(-2.0)), (1, F32(-2.0))]                                          # every row: a 256-row tile / two 32-row blocks in one segment
    t120 = sc[0][np.argsort(-sc[0], kind="stable")[119]]
    assert expected(sc[0], None, t120, m)[3] == 120
    order = [(low + few)[i % (len(few) + 2)] for i in range(nq)]
    n_low = sum(1 for _, t in order if t == F32(-2.0))
    assert 0 < n_low < nq
    got = run(ix, q, order, m, None, force_fast=1, cand_cap=32)                     # segment overflow
    check(got, order, sc, None, m, (dim, n_rows, nq, "cand_cap"))
    assert got[4] == [nq - n_low, n_low]
    order2 = [([(0, t120)] + few)[i % (len(few) + 1)] for i in range(nq)]
    n_many = sum(1 for _, t in order2 if t == t120)
    got = run(ix, q, order2, m, None, force_fast=1, refine_list=32)                 # list overflow: 120 rows in range > 32 entries
    check(got, order2, sc, None, m, (dim, n_rows, nq, "refine_list"))
    assert got[4] == [nq - n_many, n_many]
    if n_rows > 7168:                                                               # more hits than the LDS list holds, nothing forced but the path
        got = run(ix, q, order, m, None, force_fast=1)
        check(got, order, sc, None, m, (dim, n_rows, nq, "list"))
        assert got[4] == [nq - n_low, n_low]
    else:                                                                           # 600 hits: the kernel answers -2 itself
        got = run(ix, q, order, m, None, force_fast=1)
        check(got, order, sc, None, m, (dim, n_rows, nq, "all rows"))
        assert got[4] == [nq, 0]


def test_more_identical_rows_than_the_ranking_arrays(oracle):
    """1 500 exact copies of one row tie at the threshold: total counts them all, the list is the m lowest rows of the tie (the radix
    select by row, as for k_refine's crowded band); the same with better rows above the tie"""
    from rag_dpo_amd import engine as E
    rng = np.random.default_rng(11)
    dim, n = 64, 2100
    x = rng.standard_normal((n, dim)).astype(np.float32)
    x[300:1800] = x[299]
    q = np.stack([x[299] + 0.3 * rng.standard_normal(dim).astype(np.float32)] * 2).astype(np.float32)
    q[1] = x[50] + 0.6 * x[299]                                                     # row 50 scores above the copies' tie for this one
    hat, qhat = oracle.normalize_rows(x), oracle.normalize_rows(q)
    sc = [oracle.scores(hat, qhat[b]) for b in range(2)]
    order = [(0, sc[0][299]), (1, sc[1][299]), (0, sc[0][299])]
    assert expected(sc[0], None, sc[0][299], 40)[3] == 1501 and expected(sc[1], None, sc[1][299], 40)[1][:2].tolist() == [50, 299]
    ix = E.HipIndex(dim)
    try:
        ix.add(x)
        for m in (1, 40, 1024):
            fa = run(ix, q, order, m, None, force_fast=1)
            check(fa, order, sc, None, m, ("ties", m))
            assert fa[4] == [3, 0]
            ex = run(ix, q, order, m, None, force_exact=1)
            check(ex, order, sc, None, m, ("ties exact", m))
    finally:
        ix.close()
