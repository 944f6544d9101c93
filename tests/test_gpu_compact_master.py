"""GPU: the searches derived from the master (rdx_index_range, rdx_index_group_fill, rdx_index_near_dup, rdx_index_kmeans and
rdx_search_filtered) on the COMPACT master (option compact_master: the raw bf16 rows + one double divisor per row, every normalised
element recomputed where it is read, k_rows.hpp master_row), and rdx_search_filtered on a shard (row_base / a row-id map).

Every case runs on two indexes given the same add_bf16 calls (two of them: the second one grows the index) — `ix` with
compact_master = 1, `ref` in the default fp32 form — and asserts (1) every output array of ix equals ref's byte for byte, padding
included, and (2) ix's output equals the family's definition over oracle.normalize_rows(wide), wide = the bf16 rows widened, compared
the way the family's own kernel test compares (whose helpers are imported from those modules). (2) keeps the test from passing when
both forms are wrong together. Every comparison is exact.

Worlds (class World; every claim asserted on CPU values before anything is launched). Row r is a unit direction times
0.37 (1 + r % 17), the last row times 0.37 * 29, rounded to bf16; the model's divisor den[r] = max(lane-order |row|, 1e-12) gives
the oracle's normalised rows bit for bit (asserted), den[r] != den[r - 1], den[r] != den[last], and neighbouring divisors differ
by a factor of at least 1.05: a kernel that takes the divisor of a neighbouring, clamped or shuffled row moves a score in its second
digit. One all-zero row (divisor 1e-12, every score 0), one row of bf16 subnormal patterns (divisor 1e-12 too), one row at 1e18, and
exact copies of one row TWO rows apart (contiguous copies would share a divisor with their neighbour). Rows of the last ragged 32-row
block are part of every family's expected answer (asserted on the model's output).

Dims 64 / 260 / 1024 / 1028 = 1, 2 (ragged), 4 float4 groups per lane and the re-read path (U = 0)."""
import numpy as np
import pytest

import test_gpu_dedup_kernel as DK
import test_gpu_group_kernels as GK
import test_gpu_kmeans_kernel as KK
import test_gpu_range_kernel as RK
import test_gpu_search_filtered as SF
from rag_dpo_amd import kmeans as KM
from rag_dpo_amd import synth

pytestmark = pytest.mark.gpu

F32 = np.float32
DIMS = [64, 260, 1024, 1028]
TWIN = 7


@pytest.fixture(scope="module")
def eng():
    from rag_dpo_amd import engine
    return engine


# ---- the world ---------------------------------------------------------------------------------------------------------------------
def row_scales(n, first_row=0, last=29):
    s = 0.37 * (1 + (first_row + np.arange(n)) % 17)
    s[-1] = 0.37 * last                                                             # the last row's divisor is nobody else's
    return s


def copy_rows(src, first, count):
    """`count` rows from `first` on, two apart, none beside a row of src's own factor"""
    out, r = [], first
    while len(out) < count:
        if (r - 1) % 17 != src % 17 and (r + 1) % 17 != src % 17:
            out.append(r)
        r += 2
    return out


def widen(u16):
    return (np.ascontiguousarray(u16, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def dress(x, copies=(), zero=None, sub=None, big=None, first_row=0, last=29):
    """directions x [n][dim] -> the bf16 patterns uint16 [n][dim] of: unit rows times row_scales, `big` at 1e18, `zero` all zero, the
    rows of copies = [(src, rows)] equal to their src, `sub` the bf16 subnormal patterns 0x0001 .. 0x007F of both signs"""
    import torch
    x = np.array(x, dtype=np.float64)
    n, dim = x.shape
    s = row_scales(n, first_row, last)
    x *= (s / np.sqrt((x * x).sum(axis=1)))[:, None]
    if big is not None:
        x[big] *= 1e18 / s[big]
    x = x.astype(F32)
    if zero is not None:
        x[zero] = 0.0
    for src, rows in copies:
        x[rows] = x[src]
    u = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16).copy()
    assert (widen(u) == torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()).all()
    if sub is not None:
        u[sub] = (np.arange(dim) % 0x7F + 1).astype(np.uint16) | ((np.arange(dim) % 2) << 15).astype(np.uint16)
    return u


class World:
    """bf16 patterns u -> wide, the model's divisors, the reference rows hat = oracle.normalize_rows(wide); the preconditions"""

    def __init__(self, oracle, u, copies=(), zero=None, sub=None, big=None):
        self.u = np.ascontiguousarray(u, dtype=np.uint16)
        self.n, self.dim = self.u.shape
        self.wide = widen(self.u)
        w64 = self.wide.astype(np.float64)
        self.den = d = np.maximum(np.sqrt(KM.lane_sum(w64 * w64)), 1e-12)
        self.hat = oracle.normalize_rows(self.wide)
        assert self.hat.tobytes() == (w64 / d[:, None]).astype(F32).tobytes()        # den is the divisor behind the reference's rows
        assert (d[1:] != d[:-1]).all(), np.flatnonzero(d[1:] == d[:-1])[:8]
        assert (d[:-1] != d[-1]).all()
        ratio = np.maximum(d[1:], d[:-1]) / np.minimum(d[1:], d[:-1])
        assert ratio.min() >= 1.05, (int(ratio.argmin()), float(ratio.min()))
        self.last0 = (self.n - 1) // 32 * 32
        assert self.n % 32 != 0                                                     # the last 32-row block is ragged
        if zero is not None:
            assert d[zero] == 1e-12 and not self.hat[zero].any()
        if sub is not None:
            a = np.abs(self.wide[sub])
            assert (a > 0).all() and (a < F32(2.0 ** -126)).all() and d[sub] == 1e-12 and (self.hat[sub] != 0).all()
        if big is not None:
            assert 0.9e18 < d[big] < 1.1e18
        for src, rows in copies:
            assert all(self.u[r].tobytes() == self.u[src].tobytes() for r in rows) and self.hat[src].any()
        self.zero, self.sub, self.big, self.copies = zero, sub, big, list(copies)

    def in_last_block(self, rows):
        return bool((np.asarray(rows) >= self.last0).any())


class Pair:
    """ix (compact master) and ref (default master) given the same two add_bf16 calls"""

    def __init__(self, eng, w):
        self.ix, self.ref = eng.HipIndex(w.dim), eng.HipIndex(w.dim)
        self._masks = []
        try:
            self.ix.set_option("compact_master", 1)
            cut = max(1, w.n * 3 // 5)
            for a, b in ((0, cut), (cut, w.n)):
                self.ix.add_bf16(w.u[a:b])
                self.ref.add_bf16(w.u[a:b])
            self.witness(w)
        except BaseException:
            self.close()
            raise

    def witness(self, w):
        """ix really is compact: fp32 rows cannot enter it, and the refusal changes nothing"""
        n = len(self.ix)
        with pytest.raises(Exception, match="compact"):
            self.ix.add(np.ascontiguousarray(w.wide[:1]))
        assert len(self.ix) == len(self.ref) == n

    def both(self):
        return (self.ix, self.ref)

    def masks(self, allow):
        """(ix's, ref's) resident mask of allow, or (None, None)"""
        if allow is None:
            return (None, None)
        made = tuple(x.make_mask(DK.pack(allow)) for x in self.both())
        self._masks += made
        return made

    def close(self):
        for m in self._masks:
            m.close()
        self._masks = []
        self.ix.close()
        self.ref.close()


def same_bytes(a, b, what):
    """every output array of the compact index equals the fp32 index's, byte for byte; host values equal"""
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        if isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (what, "output", i)
        else:
            assert x == y, (what, "output", i)


def cached(build):
    """a module-scoped fixture body: get(key) builds once; everything built is closed at the end"""
    made = {}

    def get(*key):
        if key not in made:
            made[key] = build(*key)
        return made[key]

    return made, get


# ---- range ----------------------------------------------------------------------------------------------------------------------------
R_ROWS, R_M = 8229, 8
R_SPECIAL = dict(zero=20, sub=40, big=60)
R_LAST = 8225                                                                       # query 2's row, in the last ragged block; 8225 % 3 != 1


def range_directions(dim, n):
    rng = np.random.default_rng(dim * 100003 + n)
    common = rng.standard_normal(dim)
    x = 0.7 * common[None, :] + rng.standard_normal((n, dim))
    x[200:400] = x[200:400:20].repeat(20, axis=0) + 0.05 * rng.standard_normal((200, dim))   # ten tight clusters
    return x, common, rng


def range_queries(x, common, rng, last_row):
    dim = x.shape[1]
    q = 0.7 * common[None, :] + rng.standard_normal((3, dim))
    q[1] = x[TWIN] + 0.1 * rng.standard_normal(dim)                                 # the copies are this query's best rows
    q[2] = x[last_row] + 0.1 * rng.standard_normal(dim)                             # a row of the last block is this one's
    return q.astype(F32)


def range_mask(sc, n, keep_row):
    """every third row gone, query 0's ten best rows, the twin"""
    allow = np.arange(n) % 3 != 1
    allow[np.argsort(-sc[0], kind="stable")[:10]] = False
    allow[TWIN] = False
    assert allow[keep_row]
    return allow


def range_pairs(w, sc, allow, m):
    """(query, threshold): the best, the 6th and the 30th best allowed score of each query; every list non-empty and shorter than the
    corpus, within the MFMA path's reach, and query 2's made of the last block's row"""
    rows = np.flatnonzero(allow) if allow is not None else np.arange(w.n)
    out = []
    for b in range(3):
        best = np.sort(sc[b][rows])[::-1]
        for rank in (1, 6, 30):
            t = best[rank - 1]
            total = RK.expected(sc[b], allow, t, m)[3]
            assert rank <= total < len(rows), (b, rank, total)
            assert RK.possible_hits(sc[b], allow, t, w.dim) <= 4096
            out.append((b, t))
    assert w.in_last_block(RK.expected(sc[2], allow, out[6][1], m)[1][:1])
    assert any(RK.expected(sc[b], allow, t, m)[3] > m for b, t in out) and any(RK.expected(sc[b], allow, t, m)[3] < m for b, t in out)
    return out


def range_three_ways(pair, q, order, m, masks, sc, allow, what):
    """the plan's choice, force_exact, force_fast on both indexes: the definition's bytes, the same bytes from both, the paths"""
    nq, n = len(order), len(pair.ix)
    exact = None
    for forced, paths in (({}, [0, nq] if RK.planned_exact(n, nq) else [nq, 0]), ({"force_exact": 1}, [0, nq]), ({"force_fast": 1}, [nq, 0])):
        got = [RK.run(x, q, order, m, mk, **forced) for x, mk in zip(pair.both(), masks)]
        where = what + (tuple(forced),)
        same_bytes(got[0], got[1], where)
        RK.check(got[0], order, sc, allow, m, where)
        assert got[0][4] == paths, where
        if exact is None and forced:
            exact = got[0]
        if exact is not None:
            same_bytes(got[0][:4], exact[:4], where + ("against force_exact",))


def range_case(oracle, dim):
    """the CPU side of a range world: (world, queries, the oracle's scores, the mask, the (query, threshold) pairs without / with it)"""
    x, common, rng = range_directions(dim, R_ROWS)
    copies = [(TWIN, copy_rows(TWIN, 101, 11))]
    w = World(oracle, dress(x, copies, **R_SPECIAL), copies, **R_SPECIAL)
    q = range_queries(x, common, rng, R_LAST)
    qhat = oracle.normalize_rows(q)
    sc = [oracle.scores(w.hat, qhat[b]) for b in range(3)]
    allow = range_mask(sc, w.n, R_LAST)
    assert all(sc[1][r] == sc[1][TWIN] for r in copies[0][1]) and int(np.argmax(sc[1])) == TWIN   # identical rows, identical bits
    pairs = {False: range_pairs(w, sc, None, R_M), True: range_pairs(w, sc, allow, R_M)}
    return w, q, sc, allow, pairs


@pytest.fixture(scope="module")
def range_worlds(eng, oracle):
    def build(dim):
        w, q, sc, allow, pairs = range_case(oracle, dim)
        p = Pair(eng, w)
        return w, p, q, sc, allow, pairs, p.masks(allow)

    made, get = cached(build)
    yield get
    for v in made.values():
        v[1].close()


@pytest.mark.parametrize("nq", [3, 65])
@pytest.mark.parametrize("dim", DIMS)
def test_range(dim, nq, range_worlds):
    w, pair, q, sc, allow, pairs, masks = range_worlds(dim)
    for al, mk in ((None, (None, None)), (allow, masks)):
        distinct = pairs[al is not None]
        for shift in (0, 3, 6):                                                     # with three queries: each query's three thresholds in turn
            order = RK.batch(distinct, nq, shift)
            range_three_ways(pair, q, order, R_M, mk, sc, al, ("range", dim, nq, al is not None, shift))


@pytest.mark.parametrize("dim", DIMS)
def test_range_overflow_falls_back_for_that_query_alone(dim, range_worlds):
    """refine_list = 32 and max_results = 5: a query with 120 rows in range overflows its list for certain and is answered by the exact
    scan (k_exact_scores* + k_range_select_dense), queries with at most 32 possible hits certainly are not"""
    w, pair, q, sc, allow, pairs, _ = range_worlds(dim)
    m, nq = 5, 65
    few = [(b, t) for b, t in pairs[False] if RK.possible_hits(sc[b], None, t, dim) <= 32]
    assert len(few) >= 3
    t120 = sc[0][np.argsort(-sc[0], kind="stable")[119]]
    assert RK.expected(sc[0], None, t120, m)[3] == 120
    order = [([(0, t120)] + few)[i % (len(few) + 1)] for i in range(nq)]
    n_many = sum(1 for _, t in order if t == t120)
    assert 0 < n_many < nq
    got = [RK.run(x, q, order, m, None, force_fast=1, refine_list=32) for x in pair.both()]
    same_bytes(got[0], got[1], ("overflow", dim))
    RK.check(got[0], order, sc, None, m, ("overflow", dim))
    assert got[0][4] == [nq - n_many, n_many]


# ---- group fill -----------------------------------------------------------------------------------------------------------------------
G_ROWS = GK.N_ROWS                                                                   # 4 300 = 134 blocks of 32 + 12
G_LAST = 4296                                                                        # query 2's row: even, in the last block


def fill_spans(m):
    return [(0, 0), (5, 5), (0, 1), (10, 10 + m - 1), (10, 10 + m), (10, 10 + m + 1), (60, 60 + 64), (60, 60 + 65), (200, 200 + 255),
            (200, 200 + 256), (200, 200 + 257), (90, 150), (4190, 4215), (4096, G_ROWS), (0, 4096)]


@pytest.mark.parametrize("dim", DIMS)
def test_group_fill(dim, eng, oracle):
    import torch
    rng = np.random.default_rng(dim)
    x = rng.standard_normal((G_ROWS, dim))
    copies = [(TWIN, copy_rows(TWIN, 101, 20) + copy_rows(TWIN, 4201, 5))]           # equal scores: the row id decides
    special = dict(zero=20, sub=41, big=62)
    w = World(oracle, dress(x, copies, **special), copies, **special)
    q = rng.standard_normal((3, dim))
    q[1] = x[TWIN] + 0.01 * rng.standard_normal(dim)
    q[2] = x[G_LAST] + 0.01 * rng.standard_normal(dim)
    q = q.astype(F32)
    qhat = oracle.normalize_rows(q)
    scores = [oracle.scores(w.hat, qhat[b]) for b in range(3)]
    assert all(scores[1][r] == scores[1][TWIN] for r in copies[0][1]) and int(np.argmax(scores[1])) == TWIN
    group_rows = np.arange(G_ROWS, dtype=np.int64)
    alternate = np.arange(G_ROWS) % 2 == 0
    cases = []
    for allow in (None, alternate):
        for m in (5, 16):
            spans = fill_spans(m)
            jq = [b for b in range(3) for _ in spans]
            jb = [a for _ in range(3) for a, _ in spans]
            je = [e for _ in range(3) for _, e in spans]
            want = [GK.want_fill(scores[jq[j]], group_rows[jb[j]: je[j]], allow, m) for j in range(len(jq))]
            j_last = 2 * len(spans) + spans.index((4096, G_ROWS))
            assert want[j_last][0] == G_LAST >= w.last0                            # the last block's row leads query 2's list there
            if allow is None:
                j_dup = len(spans) + spans.index((90, 150))
                assert want[j_dup] == ([r for r in copies[0][1] if 90 <= r < 150])[:m]   # inside the tie the row id decides
            cases.append((allow, m, jq, jb, je, want))
    pair = Pair(eng, w)
    try:
        dev = torch.device("cuda", 0)
        gq, gr = torch.from_numpy(q).to(dev), torch.from_numpy(group_rows).to(dev)
        for allow, m, jq, jb, je, want in cases:
            masks = pair.masks(allow)
            got = [tuple(t.cpu().numpy() for t in eng.group_fill(ix, gq, jq, jb, je, gr, m, mask=mk)) for ix, mk in zip(pair.both(), masks)]
            same_bytes(got[0], got[1], ("group fill", dim, m, allow is not None))
            sc, ro, cn = got[0]
            assert sc.shape == ro.shape == (len(jq), m)
            for j in range(len(jq)):
                k = len(want[j])
                assert cn[j] == k, (dim, m, j)
                assert ro[j, :k].tolist() == want[j], (dim, m, j, jb[j], je[j])
                assert sc[j, :k].tobytes() == scores[jq[j]][want[j]].tobytes(), (dim, m, j)   # the oracle's bits
                assert (ro[j, k:] == -1).all() and np.isneginf(sc[j, k:]).all()
    finally:
        pair.close()


# ---- near duplicates -------------------------------------------------------------------------------------------------------------------
DUP_T = F32(0.9)
DUP_STEP = float(np.arccos(0.95))                                                   # neighbours of a chain score 0.95, second neighbours 0.805


def dup_world(oracle, dim, n, chains, copies, seed):
    """random directions (no two of them anywhere near DUP_T) and chains: rows turning by DUP_STEP in a plane of their own"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, dim))
    for rows in chains:
        a, b = rng.standard_normal((2, dim))
        a /= np.linalg.norm(a)
        b -= (b @ a) * a
        b /= np.linalg.norm(b)
        for k, r in enumerate(rows):
            x[r] = np.cos(k * DUP_STEP) * a + np.sin(k * DUP_STEP) * b
    special = dict(zero=20, sub=41, big=62)
    return World(oracle, dress(x, copies, **special), copies, **special)


def dup_mask(n, gone):
    allow = np.arange(n) % 3 != 1
    allow[gone] = False
    return allow


def dup_three_ways(pair, t, masks, allow, list_cap, want, what, batch=0):
    """DK.three_ways on both indexes: the definition's bytes and the exact statistics from the compact index, the same from the other"""
    labels, totals = want
    n = len(labels)
    n_allowed = n if allow is None else int(allow.sum())
    heavy = int(np.count_nonzero(totals > list_cap))
    b = batch or DK.BATCH
    extra = {"dup_batch": batch} if batch else {}
    for forced in ({}, {"force_exact": 1}, {"force_fast": 1}):
        got = [DK.run(ix, t, mk, list_cap, **forced, **extra) for ix, mk in zip(pair.both(), masks)]
        where = what + (tuple(forced),)
        same_bytes(got[0], got[1], where)
        lab, tot, stats = got[0]
        assert lab.dtype == np.int64 and tot.dtype == np.int64 and lab.shape == tot.shape == (n,)
        assert tot.tobytes() == totals.tobytes(), (where, np.flatnonzero(tot != totals)[:8].tolist())
        assert lab.tobytes() == labels.tobytes(), (where, np.flatnonzero(lab != labels)[:8].tolist())
        assert stats == [n_allowed, n_allowed - heavy, heavy, (n_allowed + b - 1) // b], where
    return heavy


def dup_claims(w, sc, chains, copies, allow):
    """what the model says of the world: each chain one component (split where the mask removes a member), the copies one, ends of a
    chain 2 rows in range and its inner rows 3, the zero and the subnormal row alone with nobody in range"""
    labels, totals = sc.model(DUP_T, allow)
    ok = np.ones(w.n, dtype=bool) if allow is None else allow
    for rows in chains:
        runs, cur = [], []
        for r in rows:
            if ok[r]:
                cur.append(r)
            elif cur:
                runs.append(cur)
                cur = []
        if cur:
            runs.append(cur)
        for run in runs:
            assert labels[run].tolist() == [min(run)] * len(run), (run, labels[run])
            if len(run) == len(rows) > 2:
                assert totals[run].tolist() == [2] + [3] * (len(run) - 2) + [2]
    src, rows = copies[0]
    live = [r for r in [src] + rows if ok[r]]
    assert labels[live].tolist() == [live[0]] * len(live) and (totals[live] == len(live)).all() and len(live) >= 5
    for r in (w.zero, w.sub):
        if ok[r]:
            assert labels[r] == r and totals[r] == 0                                # scores 0 (or next to it) against itself
    return labels, totals


@pytest.mark.parametrize("dim", [64, 1028])
def test_near_dup(dim, eng, oracle):
    n = 600
    chains = [[300, 302, 303, 305, 306, 308], [50, 590, 51, 450], [581, 585, 597]]   # one apart, one across the corpus, one in the last block
    copies = [(TWIN, copy_rows(TWIN, 101, 11))]
    w = dup_world(oracle, dim, n, chains, copies, 7 * dim)
    sc = DK.Scores(oracle, w.wide, F32(-np.inf))
    assert sc.hat.tobytes() == w.hat.tobytes()
    allow = dup_mask(n, [303])                                                       # the mask cuts the first chain in two
    assert all(allow[r] for c in chains for r in c if r != 303)
    wants = [dup_claims(w, sc, chains, copies, al) for al in (None, allow)]
    assert all(want[0][597] == 581 for want in wants) and w.in_last_block([581, 597])
    pair = Pair(eng, w)
    try:
        for al, want in zip((None, allow), wants):
            masks = pair.masks(al)
            # batches of 7 rows: every chain crosses batch borders. list_cap 1024: every row linked from its list; 2: the inner rows of
            # the chains and the copies go through the dense pass
            assert dup_three_ways(pair, DUP_T, masks, al, 1024, want, ("near_dup", dim, al is not None, "lists"), batch=7) == 0
            heavy = dup_three_ways(pair, DUP_T, masks, al, 2, want, ("near_dup", dim, al is not None, "dense"), batch=7)
            assert heavy == int((want[1] > 2).sum()) > 0
    finally:
        pair.close()


def test_near_dup_across_the_batch_border(eng, oracle):
    """4 200 rows: two batches without a mask; a chain over rows 4 092 .. 4 100, copies of row 7 more than 4 096 rows away"""
    dim, n = 64, 4200
    chains = [[4092, 4094, 4095, 4097, 4098, 4100], [4194, 4196]]
    copies = [(TWIN, copy_rows(TWIN, 101, 5) + copy_rows(TWIN, 4151, 3))]
    assert copies[0][1][-1] - TWIN > 4096
    w = dup_world(oracle, dim, n, chains, copies, 11)
    sc = DK.Scores(oracle, w.wide, DUP_T)
    assert sc.best_other < F32(0.96) and sc.hat.tobytes() == w.hat.tobytes()
    allow = dup_mask(n, [4095])
    assert all(allow[r] for c in chains for r in c if r != 4095)
    wants = [dup_claims(w, sc, chains, copies, al) for al in (None, allow)]
    assert all(want[0][4196] == 4194 for want in wants) and w.in_last_block([4194])
    assert wants[0][0][4100] == 4092                                                 # one component on both sides of row 4 096
    pair = Pair(eng, w)
    try:
        for al, want in zip((None, allow), wants):
            masks = pair.masks(al)
            assert dup_three_ways(pair, DUP_T, masks, al, 1024, want, ("near_dup 4200", al is not None, "lists")) == 0
            assert dup_three_ways(pair, DUP_T, masks, al, 2, want, ("near_dup 4200", al is not None, "dense")) == int((want[1] > 2).sum()) > 0
    finally:
        pair.close()


# ---- k-means --------------------------------------------------------------------------------------------------------------------------
def km_run(eng, ix, init, max_iter, mask):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(init, dtype=np.float32)).to(f"cuda:{ix.device}")
    lab, sc, cen, cnt, n_iter, conv = eng.kmeans(ix, t, max_iter, mask)
    return lab.cpu().numpy(), sc.cpu().numpy(), cen.cpu().numpy(), cnt.cpu().numpy(), n_iter, conv


def km_both(eng, pair, init, max_iter, masks, want, what):
    got = [km_run(eng, ix, init, max_iter, mk) for ix, mk in zip(pair.both(), masks)]
    same_bytes(got[0], got[1], what)
    KK.same(got[0], want, what)


@pytest.mark.parametrize("dim", DIMS)
def test_kmeans(dim, eng, oracle):
    rows, K = 700, 37
    rng = np.random.default_rng(1000003 * dim + rows)
    dirs = rng.standard_normal((K, dim))
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    x = dirs[np.arange(rows) % K] + 0.02 * rng.standard_normal((rows, dim)) / np.sqrt(dim)
    special = dict(zero=20, sub=41, big=62)
    w = World(oracle, dress(x, **special), **special)
    init = (dirs + 0.3 * rng.standard_normal((K, dim)) / np.sqrt(dim)).astype(F32)
    no_zero = np.arange(rows) % 3 != 1
    no_zero[w.zero] = False
    only_zero = np.zeros(rows, dtype=bool)
    only_zero[w.zero] = True
    cases = []
    for allow in (None, no_zero, only_zero):
        for k in (5, 37):                                                            # 37: not a multiple of the four centroids scored at a time
            for max_iter in (0, 3):
                want = KK.model(oracle, w.hat, init[:k], max_iter, allow)
                if allow is None:
                    assert (want[0][w.last0:] >= 0).all() and want[3].sum() == rows   # the last block's rows are labelled and counted
                    if k == 37 and max_iter == 0:
                        regular = np.setdiff1d(np.arange(rows), [w.zero, w.sub])
                        assert (want[0][regular] == regular % K).all()               # every row to its own direction: labels interleaved
                elif allow is only_zero:
                    assert want[3].tolist() == [1] + [0] * (k - 1) and want[0][w.zero] == 0 and want[1][w.zero] == 0
                else:
                    assert want[0][w.zero] == -1 and want[3].sum() == allow.sum() and (want[0][w.last0:][allow[w.last0:]] >= 0).all()
                cases.append((allow, k, max_iter, want))
    pair = Pair(eng, w)
    try:
        masks = {id(allow): pair.masks(allow) for allow in (None, no_zero, only_zero)}
        for allow, k, max_iter, want in cases:
            km_both(eng, pair, init[:k], max_iter, masks[id(allow)], want, ("kmeans", dim, k, max_iter, allow is not None and int(allow.sum())))
    finally:
        pair.close()


KM_SIZES = [255, 256, 257, 513]


@pytest.mark.parametrize("dim", [64, 1028])
def test_kmeans_clusters_at_the_segment_borders(dim, eng, oracle):
    """clusters of 255 / 256 / 257 / 513 members (k_km_segment_sums' segments of 256): every member's divisor enters the sum. The big
    row is a member; a zero or a subnormal row would change the sizes, and test_kmeans holds them"""
    rng = np.random.default_rng(dim)
    K = len(KM_SIZES)
    owner = rng.permutation(np.repeat(np.arange(K), KM_SIZES))
    rows = len(owner)
    x = np.zeros((rows, dim))
    x[np.arange(rows), 2 * owner] = 1.0                                              # cluster c lives around axis 2 c ...
    x[:, 20:40] = 0.2 * rng.standard_normal((rows, 20))                              # ... with a spread on axes of their own
    w = World(oracle, dress(x, big=62), big=62)
    init = np.zeros((K, dim), dtype=F32)
    init[np.arange(K), 2 * np.arange(K)] = 1.0
    want, want1 = KK.model(oracle, w.hat, init, 4), KK.model(oracle, w.hat, init, 1)
    assert want[3].tolist() == KM_SIZES and want[0].tolist() == owner.tolist() and want[5]
    pair = Pair(eng, w)
    try:
        km_both(eng, pair, init, 4, (None, None), want, ("kmeans sizes", dim))
        km_both(eng, pair, init, 1, (None, None), want1, ("kmeans sizes", dim, 1))
    finally:
        pair.close()


# ---- a filter per query ------------------------------------------------------------------------------------------------------------------
class Filtered(SF.Index):
    """SF.Index over an index that exists already"""

    def __init__(self, ix, oracle, n, allows, **opts):
        self.ix, self.n = ix, n
        self.masks = [ix.make_mask(oracle.pack_mask(a, n)) for a in allows]
        self.set(**opts)

    def close(self):                                                                # (the index is the pair's)
        for m in self.masks:
            m.close()


def filtered_world(oracle, n, dim, nq, plant=False):
    """synth's corpus, dressed; plant: rows [64 i, 64 i + 64) are near copies of query i (test_fallbacks' world)"""
    x = synth.make_corpus(n, dim).astype(np.float64)
    q = synth.make_queries(nq, dim, x.astype(F32))
    if plant:
        rng = np.random.default_rng(n)
        q = rng.standard_normal((nq, dim)).astype(F32)
        for i in range(nq):
            x[64 * i: 64 * i + 64] = q[i] + 1e-3 * rng.standard_normal((64, dim))
    special = dict(zero=n - 20, sub=n - 41, big=n - 62)                              # (behind the planted rows)
    return World(oracle, dress(x, **special), **special), q


def filtered_ref(oracle, w, q, k, qf):
    """the oracle per bitmap; the queries held to the last block's rows are answered from them"""
    qf = np.asarray(qf, dtype=np.int32)
    ref = SF.oracle_per_query(oracle, w.wide, q, k, SF.mask_set(w.n, k), qf)
    last = np.flatnonzero(qf == 5)
    assert len(last) and all(ref[2][i] == min(k, w.n - w.last0) and (ref[1][i][: ref[2][i]] >= w.last0).all() for i in last)
    return k, qf, ref


def filtered_both(oracle, pair, w, q, case, what, path, **opts):
    """ix against the oracle per bitmap, against search_device(mask) per mask on ix itself, and against ref"""
    k, qf, ref = case
    allows = SF.mask_set(w.n, k)
    a, b = Filtered(pair.ix, oracle, w.n, allows, **opts), Filtered(pair.ref, oracle, w.n, allows, **opts)
    try:
        st = SF.check_both(a, q, k, qf, ref, what, path=path)
        got = a.filtered(q, k, qf)
        same_bytes(got, b.filtered(q, k, qf), (what, "against the fp32 master"))
        assert b.ix.last_stats()["path"] == path
    finally:
        a.set()
        b.set()
        a.close()
        b.close()
    return st


@pytest.mark.parametrize("dim", [64, 200, 1280])
def test_filtered_exact_path(dim, eng, oracle):
    """k_exact_scores_reg<U, true> at dims 64 / 200, k_exact_scores<true> at 1 280; five queries: a group of four and a group of one"""
    w, q = filtered_world(oracle, 1317, dim, 5)
    cases = [filtered_ref(oracle, w, q, k, qf) for k, qf in ((10, [0, 1, 4, 5, -1]), (1, [1, 3, 5, -1, 0]))]
    pair = Pair(eng, w)
    try:
        for case in cases:
            st = filtered_both(oracle, pair, w, q, case, f"exact dim {dim} k {case[0]}", 1, force_exact=1)
            assert st["coarse_bits"] == 0
    finally:
        pair.close()


def test_filtered_small_path_and_its_fallback(eng, oracle):
    """k_boot + k_scan_small + k_refine's per-query mode; then cand_cap = 8: every query whose mask allows more than eight of its 64
    near copies overflows its segment, and the second-chance batch answers it"""
    w, q = filtered_world(oracle, 9000, 64, 40, plant=True)
    qf = SF.assignment(40)
    case = filtered_ref(oracle, w, q, 10, qf)
    pair = Pair(eng, w)
    try:
        st = filtered_both(oracle, pair, w, q, case, "small path", 0, force_fast=1)
        assert st["coarse_bits"] == 16
        st = filtered_both(oracle, pair, w, q, case, "small path, cand_cap 8", 0, force_fast=1, cand_cap=8)
        assert st["retried_queries"] >= int(np.isin(qf, (-1, 0, 1, 2)).sum()), st
    finally:
        pair.close()


def test_filtered_streaming_path(eng, oracle):
    """k_scan<SETMAX> + k_scan<EMIT> and k_refine's per-query mode on the streaming path: 130 queries, a 128-query tile and a rest"""
    w, q = filtered_world(oracle, SF.N_STREAM, SF.D_STREAM, 130)
    case = filtered_ref(oracle, w, q, 10, SF.assignment(130))
    pair = Pair(eng, w)
    try:
        st = filtered_both(oracle, pair, w, q, case, "streaming", 0, force_fast=1, small_scan=0, split_boot=0)
        assert st["coarse_bits"] == 16
    finally:
        pair.close()


# ---- after compaction ------------------------------------------------------------------------------------------------------------------
def test_after_compaction_and_an_add(eng, oracle):
    """compact(keep) with half the rows (raw rows and divisors move as they are, k_gather_raw), one add behind it, then the range and
    the k-means case on the shrunken world; the masks are remade (a mask does not outlive a write)"""
    dim, extra = 260, 300
    x, common, rng = range_directions(dim, R_ROWS)
    rows = copy_rows(TWIN, 101, 11)
    w0 = World(oracle, dress(x, [(TWIN, rows)], **R_SPECIAL), [(TWIN, rows)], **R_SPECIAL)
    keep = np.asarray(sorted(set(range(0, R_ROWS, 2)) | {TWIN, rows[0], rows[-1]}), dtype=np.int64)   # every second row, the twin, two copies
    xe = rng.standard_normal((extra, dim))
    xe[-2] = x[R_LAST]                                                              # query 2's row comes back, in the new last block
    ue = dress(xe, first_row=len(keep), last=31)
    place = {int(r): i for i, r in enumerate(keep)}
    copies = [(place[TWIN], [place[rows[0]], place[rows[-1]]])]
    special = {name: place[r] for name, r in R_SPECIAL.items()}
    w = World(oracle, np.concatenate([w0.u[keep], ue]), copies, **special)
    last_row = w.n - 2
    assert last_row >= w.last0 and last_row % 3 != 1
    q = range_queries(x, common, rng, R_LAST)
    qhat = oracle.normalize_rows(q)
    sc = [oracle.scores(w.hat, qhat[b]) for b in range(3)]
    assert int(np.argmax(sc[2])) == last_row
    allow = range_mask(sc, w.n, last_row)
    init = rng.standard_normal((5, dim)).astype(F32)
    no_zero = np.arange(w.n) % 3 != 1
    no_zero[w.zero] = False
    orders = [RK.batch(range_pairs(w, sc, al, R_M), 3, shift) for al, shift in ((None, 3), (allow, 6))]   # query 1's copies, query 2's last block
    wants = [KK.model(oracle, w.hat, init, 3, al) for al in (None, no_zero)]
    assert (wants[0][0][w.last0:] >= 0).all() and (wants[1][0][w.last0:][no_zero[w.last0:]] >= 0).all() and wants[1][0][w.zero] == -1
    pair = Pair(eng, w0)
    try:
        for ix in pair.both():
            ix.compact(keep)
            ix.add_bf16(ue)
        pair.witness(w)
        assert len(pair.ix) == w.n
        for al, order in zip((None, allow), orders):
            range_three_ways(pair, q, order, R_M, pair.masks(al), sc, al, ("range after compaction", al is not None))
        for al, want in zip((None, no_zero), wants):
            km_both(eng, pair, init, 3, pair.masks(al), want, ("kmeans after compaction", al is not None))
    finally:
        pair.close()


# ---- a filter per query on a shard (default master: this one is about the returned ids) ---------------------------------------------------
def shard_index(eng, corpus, mapped):
    """-> (index, ids): local row r is returned as ids[r]"""
    n = corpus.shape[0]
    ix = eng.HipIndex(corpus.shape[1])
    if mapped:
        ix.add(corpus)
        ids = 3 * np.arange(n, dtype=np.int64) + 7
        ix.set_row_ids(0, ids)
    else:
        ix.set_option("row_base", 1000)
        ix.add(corpus)
        ids = 1000 + np.arange(n, dtype=np.int64)
    return ix, ids


SHARD_CASES = [("exact 64", 1317, 64, 5, 1, dict(force_exact=1)), ("exact 200", 1317, 200, 5, 1, dict(force_exact=1)),
               ("exact 1280", 1317, 1280, 5, 1, dict(force_exact=1)), ("small", 9000, 64, 40, 0, dict(force_fast=1)),
               ("streaming", SF.N_STREAM, SF.D_STREAM, 130, 0, dict(force_fast=1, small_scan=0, split_boot=0))]


@pytest.mark.parametrize("mapped", [True, False], ids=["id_map", "row_base"])
@pytest.mark.parametrize("case", SHARD_CASES, ids=[c[0] for c in SHARD_CASES])
def test_filtered_on_a_shard(case, mapped, eng, oracle):
    """RowIds::of in the per-query kernels: returned ids = ids[oracle rows] (-1 in the padding), scores and counts the oracle's, the
    same arrays from search_device(mask) per mask"""
    what, n, dim, nq, path, opts = case
    corpus = synth.make_corpus(n, dim)
    q = synth.make_queries(nq, dim, corpus)
    k = 10
    allows = SF.mask_set(n, k)
    qf = np.array([0, 1, 4, 5, -1], dtype=np.int32) if nq == 5 else SF.assignment(nq)
    es, er, ec = SF.oracle_per_query(oracle, corpus, q, k, allows, qf)
    ix, ids = shard_index(eng, corpus, mapped)
    I = Filtered(ix, oracle, n, allows, **opts)
    try:
        assert (er >= 0).any() and (er < 0).any() and (ids[er[er >= 0]] != er[er >= 0]).all()   # ids and padding both occur; no id is its row
        ref = (es, np.where(er >= 0, ids[np.maximum(er, 0)], -1), ec)
        SF.check_both(I, q, k, qf, ref, what, path=path)
    finally:
        I.close()
        ix.close()
