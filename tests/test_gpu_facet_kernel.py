"""GPU: the value counts called directly (rag_dpo_amd.engine.facet_count -> rdx_index_facet_count -> k_facet_count;
engine.range_facets -> rdx_index_range_facets -> the threshold search with k_range_refine<true> / k_range_select_dense<true>, then
k_facet_top) on a HipIndex, every output equal to the definition (rag_dpo_amd/facets.py) over the oracle's exact scores. Integers: every
comparison is exact.

k_facet_count: 1 / 31 / 32 / 33 rows (a mask word and its neighbours), 1 025 (more than one workgroup), 70 001 (workgroups that walk
several tiles of 256 rows); 1 / 2 codes, FACET_LDS_GROUPS and one more (the table in LDS / straight to global memory), one code per row;
random codes with -1 among them and every row in one group; no mask, a random one, an all-zero one.

rdx_index_range_facets: the world, thresholds and masks of tests/test_gpu_range_kernel.py (imported). Codings: row % 7 with -1 where
row % 11 == 0; one group; one group per row (every count 1: the listing is the lowest codes). Every case as planned, with force_exact
and with force_fast: equal bytes. Overflow cases assert the number of queries that fell back, as the range kernel's test does."""
import numpy as np
import pytest

import test_gpu_range_kernel as RK
from rag_dpo_amd import facets as FC

pytestmark = pytest.mark.gpu

F32 = np.float32
LDS_CAP = 4096                                                                       # facet_kernel.hpp FACET_LDS_GROUPS


def pack(allow):
    bits = np.packbits(allow, bitorder="little")
    return np.concatenate([bits, np.zeros(-len(bits) % 4, np.uint8)]).view(np.uint32)


def test_the_cap_is_the_kernel_s():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "rag_dpo_amd", "csrc", "facet_kernel.hpp")) as f:
        assert f"constexpr int FACET_LDS_GROUPS = {LDS_CAP};" in f.read()


# ---- k_facet_count --------------------------------------------------------------------------------------------------------------------
def count(ix, code, G, mask=None):
    import torch
    from rag_dpo_amd import engine as E
    t = torch.from_numpy(np.ascontiguousarray(code, dtype=np.int32)).to("cuda:0") if code is not None else None
    counts, missing, total = E.facet_count(ix, t, G, mask)
    assert counts.dtype == torch.int64 and counts.shape == (G,)
    return counts.cpu().numpy(), missing, total


@pytest.mark.parametrize("rows", [1, 31, 32, 33, 1025, 70001])
def test_facet_count(rows):
    from rag_dpo_amd import engine as E
    rng = np.random.default_rng(rows)
    ix = E.HipIndex(64)
    masks = []
    try:
        ix.add(rng.standard_normal((rows, 64)).astype(F32))
        allows = [None, rng.random(rows) < 0.6, np.zeros(rows, dtype=bool)]
        masks = [ix.make_mask(pack(a)) if a is not None else None for a in allows]
        for G in (1, 2, LDS_CAP, LDS_CAP + 1, rows):
            random = rng.integers(-1, G, rows).astype(np.int32)                     # -1 among the codes
            random[rng.integers(0, rows)] = G - 1                                   # the last cell is used
            skewed = np.full(rows, G - 1, dtype=np.int32)                           # every row in one group
            for name, code in (("random", random), ("one group", skewed)):
                for allow, mask in zip(allows, masks):
                    want = FC.facet_counts_model(code, G, allow)
                    got = count(ix, code, G, mask)
                    what = (rows, G, name, None if allow is None else int(allow.sum()))
                    assert got[0].tobytes() == want[0].tobytes(), what
                    assert got[1:] == want[1:], what
                    assert int(got[0].sum()) + got[1] == got[2], what
        for allow, mask in zip(allows, masks):                                       # no table: the rows of a mask
            got = count(ix, None, 0, mask)
            assert got[0].shape == (0,) and got[1] == got[2] == (rows if allow is None else int(allow.sum()))
    finally:
        for m in masks:
            if m is not None:
                m.close()
        ix.close()


@pytest.mark.parametrize("G", [3, LDS_CAP + 5])
def test_a_code_outside_the_table_fails_the_call(G):
    """refused by the flag: the kernel compares the code with n_groups before it would index with it"""
    from rag_dpo_amd import engine as E
    rows = 1000
    ix = E.HipIndex(64)
    try:
        ix.add(np.random.default_rng(1).standard_normal((rows, 64)).astype(F32))
        good = (np.arange(rows) % G).astype(np.int32)
        for bad_code in (G, G + 1000, 2 ** 31 - 1, -2, -(2 ** 31)):
            code = good.copy()
            code[777] = bad_code
            with pytest.raises(ValueError, match="outside -1 .. n_groups - 1"):
                count(ix, code, G)
        got = count(ix, good, G)                                                     # the index is as it was
        assert got[0].tobytes() == np.bincount(good, minlength=G).astype(np.int64).tobytes() and got[1:] == (0, rows)
    finally:
        ix.close()


# ---- rdx_index_range_facets -------------------------------------------------------------------------------------------------------------
def codings(n_rows):
    r = np.arange(n_rows)
    return {"mod 7": (np.where(r % 11 == 0, -1, r % 7).astype(np.int32), 7), "one group": (np.zeros(n_rows, dtype=np.int32), 1),
            "a group per row": (r.astype(np.int32), n_rows)}


@pytest.fixture(scope="module")
def worlds(oracle):
    import torch
    from rag_dpo_amd import engine as E
    made = {}

    def get(dim, n_rows):
        if (dim, n_rows) not in made:
            x, q = RK.world(dim, n_rows)
            ix = E.HipIndex(dim)
            ix.add(x)
            hat, qhat = oracle.normalize_rows(x), oracle.normalize_rows(q)
            sc = [oracle.scores(hat, qhat[b]) for b in range(3)]
            allow = RK.mask_for(sc, n_rows)
            tabs = {name: (code, G, torch.from_numpy(code).to("cuda:0")) for name, (code, G) in codings(n_rows).items()}
            made[(dim, n_rows)] = (ix, q, sc, allow, ix.make_mask(pack(allow)), tabs)
        return made[(dim, n_rows)]

    yield get
    for ix, _, _, _, mask, _ in made.values():
        mask.close()
        ix.close()


def run(ix, q, order, tab, limit, mask=None, **options):
    import torch
    from rag_dpo_amd import engine as E
    dev = torch.device("cuda", 0)
    qs = np.stack([q[b] for b, _ in order]).astype(np.float32)
    thr = np.asarray([t for _, t in order], dtype=np.float32)
    for name, v in options.items():
        ix.set_option(name, v)
    try:
        res = E.range_facets(ix, torch.from_numpy(qs).to(dev), torch.from_numpy(thr).to(dev), tab[2], tab[1], limit, mask)
    finally:
        for name in options:
            ix.set_option(name, 0)
    return tuple(t.cpu().numpy() for t in res[:5]) + (res[5],)


def expected(sc, allow, thr, code, G, limit):
    ok = sc >= F32(thr)
    if allow is not None:
        ok = ok & allow
    counts, missing, total = FC.facet_counts_model(code, G, ok)
    oc, on, nv = FC.pad_listing(counts, limit)
    return oc, on, nv, missing, total


def check(got, order, sc, allow, tab, limit, what):
    codes, cnt, nv, mis, tot, _ = got
    assert (codes.dtype, cnt.dtype, nv.dtype, mis.dtype, tot.dtype) == (np.int32, np.int64, np.int32, np.int64, np.int64)
    assert codes.shape == cnt.shape == (len(order), limit)
    for i, (b, thr) in enumerate(order):
        oc, on, n, m, t = expected(sc[b], allow, thr, tab[0], tab[1], limit)
        where = (what, i, b, float(thr))
        assert (int(tot[i]), int(mis[i]), int(nv[i])) == (t, m, n), where
        assert codes[i].tolist() == oc.tolist() and cnt[i].tolist() == on.tolist(), where


def same(a, b):
    for x, y in zip(a[:5], b[:5]):
        assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("nq", RK.BATCHES)
@pytest.mark.parametrize("n_rows", RK.ROWS)
@pytest.mark.parametrize("dim", RK.DIMS)
def test_three_ways_agree_with_the_definition(dim, n_rows, nq, worlds):
    ix, q, sc, allow, mask, tabs = worlds(dim, n_rows)
    limit = 9
    for al, mk in ((None, None), (allow, mask)):
        # a row's own score and the next float above it (the copies of row 7 enter or leave their cells), a cluster's median, above
        # the best score, the ranks, and -2 (every allowed row) where the MFMA path holds that many hits
        distinct = RK.combos(sc, al, 5, dim, n_rows)
        order = RK.batch(distinct, nq)                                              # (one query: the row's own score)
        for name, tab in tabs.items():
            what = (dim, n_rows, nq, al is not None, name)
            got = run(ix, q, order, tab, limit, mk)
            check(got, order, sc, al, tab, limit, what + ("planned",))
            assert got[5] == ([0, nq] if RK.planned_exact(n_rows, nq) else [nq, 0]), what
            ex = run(ix, q, order, tab, limit, mk, force_exact=1)
            assert ex[5] == [0, nq], what
            fa = run(ix, q, order, tab, limit, mk, force_fast=1)
            assert fa[5] == [nq, 0], what                                            # the kernels' own answer: nobody fell back
            same(got, ex)
            same(fa, ex)
        totals = RK.run(ix, q, order, 1, mk)[3]                                      # rdx_index_range's out_total for the same call
        assert got[4].tobytes() == totals.tobytes()


@pytest.mark.parametrize("n_rows", RK.ROWS)
@pytest.mark.parametrize("dim", RK.DIMS)
def test_each_distinct_threshold_alone(dim, n_rows, worlds):
    """one query at a time, every distinct (query, threshold) pair in turn: the copies enter at their own score and leave one float above"""
    ix, q, sc, allow, mask, tabs = worlds(dim, n_rows)
    tab = tabs["mod 7"]
    for al, mk in ((None, None), (allow, mask)):
        distinct = RK.combos(sc, al, 5, dim, n_rows)
        live = [r for r in [RK.TWIN] + RK.COPIES if al is None or al[r]]
        own = expected(sc[1], al, distinct[0][1], *tab[:2], 9)
        above = expected(sc[1], al, distinct[1][1], *tab[:2], 9)
        assert own[4] == len(live) and above[4] == 0 and own[3] == sum(1 for r in live if r % 11 == 0)
        for b, t, kind in distinct:
            for forced in ({"force_exact": 1}, {"force_fast": 1}):
                got = run(ix, q, [(b, t)], tab, 9, mk, **forced)
                check(got, [(b, t)], sc, al, tab, 9, (dim, n_rows, kind, tuple(forced)))


@pytest.mark.parametrize("nq", [3, 65])
@pytest.mark.parametrize("n_rows", RK.ROWS)
@pytest.mark.parametrize("dim", RK.DIMS)
def test_overflowing_queries_are_counted_once_by_the_dense_stage(dim, n_rows, nq, worlds):
    ix, q, sc, allow, mask, tabs = worlds(dim, n_rows)
    limit = 9
    few = [(b, t) for b, t, kind in RK.combos(sc, None, 5, dim, n_rows) if RK.possible_hits(sc[b], None, t, dim) <= 32]
    assert len(few) >= 3
    low = [(0, F32(-2.0)), (1, F32(-2.0))]
    t120 = sc[0][np.argsort(-sc[0], kind="stable")[119]]
    order = [(low + few)[i % (len(few) + 2)] for i in range(nq)]
    n_low = sum(1 for _, t in order if t == F32(-2.0))
    order2 = [([(0, t120)] + few)[i % (len(few) + 1)] for i in range(nq)]
    n_many = sum(1 for _, t in order2 if t == t120)
    assert 0 < n_low < nq and 0 < n_many < nq
    for name in ("mod 7", "a group per row"):
        tab = tabs[name]
        got = run(ix, q, order, tab, limit, None, force_fast=1, cand_cap=32)         # segment overflow
        check(got, order, sc, None, tab, limit, (dim, n_rows, nq, name, "cand_cap"))
        assert got[5] == [nq - n_low, n_low]
        got = run(ix, q, order2, tab, limit, None, force_fast=1, refine_list=32)     # list overflow: 120 rows in range > 32 entries
        check(got, order2, sc, None, tab, limit, (dim, n_rows, nq, name, "refine_list"))
        assert got[5] == [nq - n_many, n_many]
        got = run(ix, q, order, tab, limit, None, force_fast=1)                      # -2: more hits than the list holds at 8 229 rows
        check(got, order, sc, None, tab, limit, (dim, n_rows, nq, name, "all rows"))
        assert got[5] == ([nq - n_low, n_low] if n_rows > 7168 else [nq, 0])


@pytest.mark.parametrize("n_rows", RK.ROWS)
def test_sub_chunks_of_one_and_of_two_queries(n_rows, worlds):
    """a group per row: a table row is 4 B x rows. The budget holds one query, then two of three / five: the passes give the same bytes"""
    dim = 64
    ix, q, sc, allow, mask, tabs = worlds(dim, n_rows)
    tab = tabs["a group per row"]
    row_kb = -(-4 * n_rows // 1024)                                                 # KiB that hold one table row, rounded up
    assert row_kb * 1024 // (4 * n_rows) == 1 and 2 * row_kb * 1024 // (4 * n_rows) in (2, 3)
    distinct = RK.combos(sc, allow, 5, dim, n_rows)
    for nq in (3, 5):
        order = RK.batch(distinct, nq, 2) [:-1] + [(2, F32(-2.0))]
        for forced in ({"force_exact": 1}, {"force_fast": 1}):
            whole = run(ix, q, order, tab, 40, mask, **forced)
            check(whole, order, sc, allow, tab, 40, (n_rows, nq, tuple(forced)))
            for kb in (row_kb, 2 * row_kb):
                got = run(ix, q, order, tab, 40, mask, facet_table_kb=kb, **forced)
                same(got, whole)
                assert got[5] == whole[5]


@pytest.mark.parametrize("n_rows", RK.ROWS)
def test_the_limit_inside_a_plateau_above_the_values_and_a_wide_table(n_rows, worlds):
    import torch
    dim = 260
    ix, q, sc, allow, mask, tabs = worlds(dim, n_rows)
    order = [(0, F32(-2.0)), (1, sc[1][RK.TWIN]), (2, F32(-2.0))]
    per_row = tabs["a group per row"]
    for al, mk in ((None, None), (allow, mask)):
        live = np.flatnonzero(al) if al is not None else np.arange(n_rows)
        for limit in (1, 5, 1024):                                                  # every count 1: the lowest codes, whatever the cut
            for forced in ({"force_exact": 1}, {"force_fast": 1}):
                got = run(ix, q, order, per_row, limit, mk, **forced)
                check(got, order, sc, al, per_row, limit, (n_rows, limit, tuple(forced)))
                n = min(limit, len(live))
                assert got[0][0, :n].tolist() == live[:n].tolist() and (got[1][0, :n] == 1).all() and got[2][0] == len(live)
        got = run(ix, q, order, tabs["mod 7"], 1024, mk)                             # limit above n_values: padding behind 7 cells
        check(got, order, sc, al, tabs["mod 7"], 1024, (n_rows, "limit above"))
        assert got[2].max() <= 7 and (got[0][:, 7:] == -1).all() and (got[1][:, 7:] == 0).all()
    G = 100_000                                                                     # a wide table with seven non-zero cells at its end
    code = (np.arange(n_rows) % 7 + G - 7).astype(np.int32)
    wide = (code, G, torch.from_numpy(code).to("cuda:0"))
    for forced in ({"force_exact": 1}, {"force_fast": 1}):
        got = run(ix, q, order, wide, 10, mask, **forced)
        check(got, order, sc, allow, wide, 10, (n_rows, "G = 100 000", tuple(forced)))
        assert got[2][0] == 7 and got[0][0, :7].min() >= G - 7


def test_a_code_outside_the_table_fails_the_search(worlds):
    import torch
    ix, q, sc, allow, mask, tabs = worlds(64, 600)
    code = tabs["mod 7"][0].copy()
    code[RK.TWIN] = 7                                                               # query 1's best row
    bad = (code, 7, torch.from_numpy(code).to("cuda:0"))
    for forced in ({"force_exact": 1}, {"force_fast": 1}):
        with pytest.raises(ValueError, match="outside -1 .. n_groups - 1"):
            run(ix, q, [(1, sc[1][RK.TWIN])], bad, 5, None, **forced)
    got = run(ix, q, [(1, sc[1][RK.TWIN])], tabs["mod 7"], 5)
    check(got, [(1, sc[1][RK.TWIN])], sc, None, tabs["mod 7"], 5, "after the refusal")


def test_on_the_compact_master_against_its_fp32_twin(oracle):
    """the rows in range on the compact bf16 master (the exact re-score and the exact scan recompute every element) are its fp32 twin's"""
    import torch
    import test_gpu_compact_master as CM
    from rag_dpo_amd import engine as E
    dim = 260
    w, q, sc, allow, pairs = CM.range_case(oracle, dim)
    code, G = codings(w.n)["mod 7"]
    pair = CM.Pair(E, w)
    try:
        for al in (None, allow):
            masks = pair.masks(al)
            order = RK.batch(pairs[al is not None], 65, 3)
            for forced in ({"force_exact": 1}, {"force_fast": 1}):
                got = [run(ix, q, order, (code, G, torch.from_numpy(code).to("cuda:0")), 9, mk, **forced) for ix, mk in zip(pair.both(), masks)]
                same(got[0], got[1])
                assert got[0][5] == got[1][5]
                check(got[0], order, sc, al, (code, G), 9, ("compact", al is not None, tuple(forced)))
    finally:
        pair.close()
