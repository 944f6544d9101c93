"""GPU: near-duplicate clustering called directly (rag_dpo_amd.engine.near_dup -> rdx_index_near_dup -> k_gather_rows, the threshold
search, k_dup_link_lists, the exact scores + k_dup_link_dense, k_dup_labels) on a HipIndex, labels and totals byte for byte against
the definition (rag_dpo_amd/dedup.py near_dup_model) over the oracle's exact scores oracle.scores(hat, oracle.normalize_rows(hat)[i]).

Every case runs as planned, with force_exact and with force_fast, and the three must give the same bytes; the statistics are exact
too: allowed rows examined, rows linked from their lists, rows linked by the dense pass (= allowed rows with total > list_cap, exact by
definition), batches. Every claim about a world is asserted on the CPU from the oracle's scores before anything runs.

Worlds. (1) tests/test_gpu_range_kernel.py's: a common component, ten tight clusters (rows 200..399), eleven copies of row 7, two zero
rows; 600 rows at dims 64 / 260 / 1024, and 8 229 rows at dim 64 (three batches, the last of 37 queries: k_scan_small under
force_fast). (2) Chains x_i = e_i + e_{i+1} with batches of 7 rows: edges cross batch borders. (3) Two hubs whose only bridge lies
beyond the first list_cap entries of either hub's list: linking from lists alone would give two components. (4) 1 500 identical rows:
all heavy, and the max_dense refusal."""
import numpy as np
import pytest

from rag_dpo_amd import dedup as DD

pytestmark = pytest.mark.gpu

F32 = np.float32
TWIN, COPIES, ZEROS = 7, list(range(100, 111)), [20, 21]
BATCH = 4096                                                                        # rdx_index_near_dup's batch (the range chunk)


def up(x):
    return np.nextafter(F32(x), F32(np.inf))


def pack(allow):
    bits = np.packbits(allow, bitorder="little")
    return np.concatenate([bits, np.zeros(-len(bits) % 4, np.uint8)]).view(np.uint32)


class Scores:
    """the oracle's exact scores of every stored row against K1(stored row i), kept sparsely: per row the entries >= t_base"""

    def __init__(self, oracle, x, t_base):
        self.hat = oracle.normalize_rows(x)
        self.n = n = self.hat.shape[0]
        self.t_base = F32(t_base)
        _, group = np.unique(self.hat, axis=0, return_inverse=True)                 # identical stored rows share a group
        group = group.reshape(-1)
        qhat = oracle.normalize_rows(self.hat)                                      # K1 of the stored rows, as a search applies it
        self.hits, self.best_other, self.top = [], F32(-np.inf), F32(-np.inf)
        for i in range(n):
            s = oracle.scores(self.hat, qhat[i])
            rows = np.flatnonzero(s >= self.t_base)
            self.hits.append((rows, s[rows].copy()))
            self.top = max(self.top, s.max())
            other = s[group != group[i]]
            if other.size:
                self.best_other = max(self.best_other, other.max())

    def row(self, i):
        s = np.full(self.n, -np.inf, dtype=np.float32)
        rows, sc = self.hits[i]
        s[rows] = sc
        return s

    def model(self, t, allow=None):
        assert F32(t) >= self.t_base
        return DD.near_dup_model(self.row, self.n, t, allow)


def run(ix, t, mask, list_cap, max_dense=4096, **options):
    from rag_dpo_amd import engine as E
    for name, v in options.items():
        ix.set_option(name, v)
    try:
        lab, tot, stats = E.near_dup(ix, t, mask, list_cap, max_dense)
    finally:
        for name in options:
            ix.set_option(name, 0)
    return lab.cpu().numpy(), tot.cpu().numpy(), stats


def three_ways(ix, t, mask, allow, list_cap, want, what, batch=0):
    """as planned, force_exact, force_fast: the definition's bytes and the exact statistics, three times"""
    labels, totals = want
    n = len(labels)
    n_allowed = n if allow is None else int(allow.sum())
    heavy = int(np.count_nonzero(totals > list_cap))
    b = batch or BATCH
    extra = {"dup_batch": batch} if batch else {}
    for forced in ({}, {"force_exact": 1}, {"force_fast": 1}):
        lab, tot, stats = run(ix, t, mask, list_cap, **forced, **extra)
        where = what + (tuple(forced),)
        assert lab.dtype == np.int64 and tot.dtype == np.int64 and lab.shape == tot.shape == (n,)
        assert tot.tobytes() == totals.tobytes(), (where, np.flatnonzero(tot != totals)[:8].tolist())
        assert lab.tobytes() == labels.tobytes(), (where, np.flatnonzero(lab != labels)[:8].tolist())
        assert stats == [n_allowed, n_allowed - heavy, heavy, (n_allowed + b - 1) // b], where
    return heavy


# ---- 1. the range tests' world ---------------------------------------------------------------------------------------------------
def world(dim, n_rows):
    rng = np.random.default_rng(dim * 100003 + n_rows)
    common = rng.standard_normal(dim).astype(np.float32)
    x = (0.7 * common[None, :] + rng.standard_normal((n_rows, dim))).astype(np.float32)
    x[200:400] = x[200:400:20].repeat(20, axis=0) + 0.05 * rng.standard_normal((200, dim)).astype(np.float32)   # ten tight clusters
    x[COPIES] = x[TWIN]
    x[ZEROS] = 0.0
    return x


def mask_for(n_rows):
    """every third row gone, the twin and every other copy with them; five copies stay"""
    allow = np.arange(n_rows) % 3 != 1
    allow[COPIES[1::2]] = True
    allow[[TWIN] + COPIES[::2]] = False
    return allow


def two_e(dim):
    dim_pad = (dim + 63) // 64 * 64
    return F32(2.0) * (F32(1.0e-3) + F32(2.5e-7) * F32(dim_pad))                    # rdx_index::two_e()


@pytest.mark.parametrize("dim,n_rows", [(64, 600), (260, 600), (1024, 600), (64, 8229)])
def test_the_range_tests_world(dim, n_rows, oracle):
    from rag_dpo_amd import engine as E
    x = world(dim, n_rows)
    hat = oracle.normalize_rows(x)
    qhat = oracle.normalize_rows(hat)
    # the median intra-cluster score of rows 200..219 against row 200: rows within E on both sides of it
    s200 = oracle.scores(hat, qhat[200])
    t_cl = np.sort(s200[200:220])[10]
    near = s200[200:220].astype(np.float64) - float(t_cl)
    half_e = float(two_e(dim)) / 2
    assert ((near < 0) & (near > -half_e)).any() and ((near > 0) & (near < half_e)).any()
    small = n_rows <= 4096
    sc = Scores(oracle, x, F32(-np.inf) if small else t_cl)
    allow = mask_for(n_rows)
    copies = [TWIN] + COPIES
    # the next float above the best score between non-identical rows: only the twelve copies cluster, and their label is 7
    t_up = up(sc.best_other)
    assert t_up >= t_cl
    labels, totals = sc.model(t_up)
    want = np.arange(n_rows)
    want[copies] = TWIN
    assert labels.tolist() == want.tolist() and (totals[copies] == 12).all()
    assert all(totals[r] == 0 for r in ZEROS) and labels[ZEROS].tolist() == ZEROS    # a zero row scores 0 against itself: alone, total 0
    # above every score: every label its own row, totals 0 — zero rows included
    t_above = up(sc.top)
    labels, totals = sc.model(t_above)
    assert labels.tolist() == list(range(n_rows)) and not totals.any()
    # inside the clusters: components of more than one row beside the copies
    labels, totals = sc.model(t_cl)
    assert len(DD.clusters_of(labels)) >= 2 and totals.max() > 8
    ix = E.HipIndex(dim)
    mask = None
    try:
        ix.add(x)
        mask = ix.make_mask(pack(allow))
        for al, mk in ((None, None), (allow, mask)):
            for name, t in (("cluster median", t_cl), ("copies only", t_up), ("above all", t_above)):
                want = sc.model(t, al)
                for list_cap in (8, 1024):
                    heavy = three_ways(ix, t, mk, al, list_cap, want, (dim, n_rows, name, al is not None, list_cap))
                    if name == "copies only":                                       # 12 (5 under the mask) copies each: heavy at 8 without the mask
                        assert heavy == (12 if al is None and list_cap == 8 else 0)
                    if name == "above all":
                        assert heavy == 0
            if small:                                                               # -2: every row is heavy, one component
                want = sc.model(F32(-2.0), al)
                first = 0 if al is None else int(np.flatnonzero(al)[0])
                n_al = n_rows if al is None else int(al.sum())
                assert set(want[0].tolist()) <= {first, -1} and (want[1][want[0] >= 0] == n_al).all()
                assert three_ways(ix, F32(-2.0), mk, al, 64, want, (dim, n_rows, "-2", al is not None)) == n_al
    finally:
        if mask is not None:
            mask.close()
        ix.close()


# ---- 2. chains -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [64, 1024])
def test_chains_across_batch_borders(dim, oracle):
    from rag_dpo_amd import engine as E
    n = dim - 1
    x = np.zeros((n, dim), dtype=np.float32)
    x[np.arange(n), np.arange(n)] = 1.0
    x[np.arange(n), np.arange(n) + 1] = 1.0
    t = F32(0.4)
    sc = Scores(oracle, x, F32(-np.inf))
    for i in range(n):                                                              # neighbours score 0.5, the row itself 1, everything else 0
        s = sc.row(i)
        nb = [j for j in (i - 1, i + 1) if 0 <= j < n]
        assert all(abs(float(s[j]) - 0.5) < 1e-6 for j in nb) and abs(float(s[i]) - 1.0) < 1e-6
        rest = np.ones(n, dtype=bool)
        rest[nb + [i]] = False
        assert (s[rest] == 0).all()
    gaps = [20, 21, 22, 40] if dim == 64 else list(range(500, 521)) + [700]
    allow = np.ones(n, dtype=bool)
    allow[gaps] = False
    ix = E.HipIndex(dim)
    mask = None
    try:
        ix.add(x)
        mask = ix.make_mask(pack(allow))
        for al, mk in ((None, None), (allow, mask)):
            want = sc.model(t, al)
            if al is None:
                assert not want[0].any() and want[1].tolist() == [2] + [3] * (n - 2) + [2]
            else:                                                                   # the labels restart after each gap; removed rows get -1
                starts = [0] + [g + 1 for g in gaps if g + 1 not in gaps]
                exp = np.full(n, -1)
                for a in starts:
                    b = a
                    while b < n and al[b]:
                        exp[b] = a
                        b += 1
                assert want[0].tolist() == exp.tolist() and len(set(exp.tolist())) == len(starts) + 1
            heavy = three_ways(ix, t, mk, al, 3, want, (dim, "all light", al is not None), batch=7)
            assert heavy == 0
            heavy = three_ways(ix, t, mk, al, 2, want, (dim, "interior heavy", al is not None), batch=7)
            assert heavy == int((want[1] == 3).sum()) > 0
    finally:
        if mask is not None:
            mask.close()
        ix.close()


# ---- 3. two hubs -----------------------------------------------------------------------------------------------------------------
def test_two_hubs_whose_bridge_is_beyond_both_lists(oracle):
    from rag_dpo_amd import engine as E
    dim = 64

    def e(k):
        v = np.zeros(dim, dtype=np.float32)
        v[k] = 1.0
        return v

    h1, h2 = e(0), 0.8 * e(0) + 0.6 * e(1)
    x = np.stack([h1 + 0.6 * e(k) for k in range(2, 8)] + [h1, h2] + [h2 + 0.6 * e(k) for k in range(8, 14)]).astype(np.float32)
    H1, H2, S1, S2 = 6, 7, list(range(0, 6)), list(range(8, 14))
    t = F32(0.75)
    sc = Scores(oracle, x, F32(-np.inf))
    near = lambda a, b: abs(float(a) - b) < 2e-3   # noqa: E731
    s1, s2 = sc.row(H1), sc.row(H2)
    assert all(near(s1[r], 0.857) for r in S1) and all(near(s2[r], 0.857) for r in S2) and near(s1[H2], 0.8) and near(s2[H1], 0.8)
    assert all(near(s1[r], 0.686) for r in S2) and all(near(s2[r], 0.686) for r in S1)
    assert near(sc.row(0)[1], 0.735) and near(sc.row(8)[9], 0.735)
    labels, totals = sc.model(t)
    assert totals.tolist() == [2] * 6 + [8, 8] + [2] * 6 and not labels.any()      # degrees 8 and 2; one component of 14
    # the bridge is in neither hub's first four entries (score descending, row ascending) ...
    lists = []
    for i in range(14):
        s = sc.row(i)
        rows = np.flatnonzero(s >= t)
        lists.append(rows[np.lexsort((rows, -s[rows].astype(np.float64)))][:4].tolist())
    assert H2 not in lists[H1] and H1 not in lists[H2]
    # ... so linking from the lists alone gives two components
    alone = DD.labels_from_lists(14, None, range(14), lists)
    assert sorted(set(alone.tolist())) == [0, 7]
    ix = E.HipIndex(dim)
    try:
        ix.add(x)
        assert three_ways(ix, t, None, None, 4, (labels, totals), ("hubs", 4)) == 2
        assert three_ways(ix, t, None, None, 8, (labels, totals), ("hubs", 8)) == 0
    finally:
        ix.close()


# ---- 4. 1 500 identical rows -----------------------------------------------------------------------------------------------------
def test_identical_rows_beyond_the_longest_list(oracle):
    from rag_dpo_amd import engine as E
    rng = np.random.default_rng(11)
    dim, n = 64, 2100
    x = rng.standard_normal((n, dim)).astype(np.float32)
    x[300:1800] = x[299]
    t = F32(0.9)
    hat = oracle.normalize_rows(x)
    qhat = oracle.normalize_rows(hat)
    S = np.stack([oracle.scores(hat, qhat[i]) for i in range(n)])
    A = S >= t
    tie = np.zeros(n, dtype=bool)
    tie[299:1800] = True
    assert A[np.ix_(tie, tie)].all() and not A[np.ix_(tie, ~tie)].any() and not A[np.ix_(~tie, tie)].any()
    assert (A[np.ix_(~tie, ~tie)] == np.eye(int((~tie).sum()), dtype=bool)).all()  # everybody else: itself and nobody else
    labels = np.where(tie, 299, np.arange(n)).astype(np.int64)                      # one component of 1 501, labelled with the first copy
    totals = np.where(tie, 1501, 1).astype(np.int64)
    ix = E.HipIndex(dim)
    try:
        ix.add(x)
        assert three_ways(ix, t, None, None, 1024, (labels, totals), ("ties",)) == 1501
        with pytest.raises(ValueError, match=r"1501 rows .*list_cap = 1024.*too loose for duplicate detection"):
            run(ix, t, None, 1024, max_dense=100)
        q = (x[[5, 299, 2000]] + 0.1 * rng.standard_normal((3, dim))).astype(np.float32)
        s, r, c = ix.search(q, 10)                                                  # the index answers a plain search afterwards
        ref = oracle.cosine_topk(hat, q, 10)
        assert (r == ref[1]).all() and (s == ref[0]).all() and (c == ref[2]).all()
    finally:
        ix.close()


def test_argument_checks_and_an_empty_index():
    from rag_dpo_amd import engine as E
    ix = E.HipIndex(64)
    other = E.HipIndex(64)
    mask = None
    try:
        lab, tot, stats = E.near_dup(ix, 0.5)
        assert lab.numel() == 0 and tot.numel() == 0 and stats == [0, 0, 0, 0]
        ix.add(np.eye(8, 64, dtype=np.float32))
        other.add(np.eye(9, 64, dtype=np.float32))
        mask = other.make_mask(pack(np.ones(9, dtype=bool)))
        for bad in (dict(list_cap=0), dict(list_cap=1025), dict(t=float("nan")), dict(max_dense=-1), dict(mask=mask)):
            with pytest.raises(ValueError):
                E.near_dup(ix, **{"t": 0.5, **bad})
        with pytest.raises(ValueError):
            ix.set_option("dup_batch", 4097)
        lab, tot, stats = E.near_dup(ix, 0.5)
        assert lab.cpu().tolist() == list(range(8)) and tot.cpu().tolist() == [1] * 8 and stats == [8, 8, 0, 1]
    finally:
        if mask is not None:
            mask.close()
        other.close()
        ix.close()
