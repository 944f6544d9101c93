"""GPU: the top-k selection kernels against the documented order at its edges (tests/selection_landscapes.py).

Every search ends in select_dense_query (K5b), one of k_refine's endings or a merge, and all of them end in rank_and_write.
include/rdx.h promises ONE order for them: score descending (compared as floats: +0.0 and -0.0 tie), ties by ascending row id.
The landscapes put signed zeros, plateaus of 1 .. 3000 identical scores, negative lists and k up to SELECT_MAX_K at the k-th place,
on either side of EQ_CAP, REFINE_PMAX, MERGE_MAX and of the 32 768 rows K5b keeps in registers. The bar for every case: out_count
and out_row equal the oracle's exactly, scores equal as values AND as bits (a returned zero carries the sign of the row's exact
score), tails hold (-inf, -1). Every case asserts its landscape's precondition on `facts` (the oracle's own scores) first."""
import numpy as np
import pytest

import selection_landscapes as SL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from rag_dpo_amd import engine
    return engine


def _index(eng, corpus, before_add=(), **opts):
    ix = eng.HipIndex(corpus.shape[1])
    for k, v in before_add:
        ix.set_option(k, v)
    ix.add(corpus)
    for k, v in opts.items():
        ix.set_option(k, v)
    return ix


def _same(got, want, what=""):
    gs, gr, gc = got
    es, er, ec = want
    np.testing.assert_array_equal(gc, ec, err_msg=f"counts {what}")
    np.testing.assert_array_equal(gr, er, err_msg=f"row ids {what}")
    assert np.array_equal(gs, es), f"scores {what}"
    nz = es != 0
    np.testing.assert_array_equal(gs.view(np.uint32)[nz], es.view(np.uint32)[nz], err_msg=f"score bits {what}")
    np.testing.assert_array_equal(np.signbit(gs[~nz]), np.signbit(es[~nz]), err_msg=f"sign of the returned zeros {what}")
    for b in range(ec.shape[0]):
        assert (gr[b, gc[b]:] == -1).all() and np.isneginf(gs[b, gc[b]:]).all(), f"tail {what}"


def _check(oracle, ix, corpus, q, k, allow=None, path=None, what=""):
    want = oracle.cosine_topk(oracle.normalize_rows(corpus), q, k, allow)
    got = ix.search(q, k, oracle.pack_mask(allow, corpus.shape[0]))
    st = ix.last_stats()
    _same(got, want, f"{what} k={k} nq={q.shape[0]} {st}")
    if path is not None:
        assert st["path"] == path, st
    return st, got, want


# ---- 1. signed zeros on the exact path ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["zeros_3000", "zeros_3000_few", "zeros_tiled", "zeros_tiled_few"])
def test_signed_zeros_on_the_exact_path(eng, oracle, name):
    """the k-th place inside a zero plateau holding both signs, at its first place, a few places in, half way and at its last place;
    the plateau above EQ_CAP (the in-order walk) and below it (the eq_idx ranking), the score row in registers and in global
    memory, with and without a bitmap hiding some of the low-row zeros, 1 / 5 / 6 queries (a partial group, a full group of four
    plus one, plus two). A select that orders ties by f2key takes every +0.0 row ahead of every -0.0 row: on the smallest
    instance ids [143 653 1474 1969 0 1 2 9 10 11] (selection_landscapes.order_by_keys) against [143 653 1474 1969 0 1 2 3 4 5]."""
    corpus, queries, facts = SL.catalogue()[name][0](oracle)
    n = corpus.shape[0]
    assert queries.shape[0] >= 6
    assert (n <= SL.REG_ROWS) == ("tiled" not in name)               # register form / global form of K5b
    ix = _index(eng, corpus, force_exact=1)
    m = SL.masks(n)
    for mask in (None, "low"):
        allow = m[mask]
        s0 = facts.scores[0] if allow is None else facts.scores[0][allow]
        top, zeros = int((s0 > 0).sum()), int((s0 == 0).sum())
        assert (zeros > SL.EQ_CAP) == ("few" not in name), zeros   # which of the two tie routines runs
        ks = sorted({top + 1, top + 6, min(top + zeros // 2, SL.SELECT_MAX_K), min(top + zeros, SL.SELECT_MAX_K)})
        for k in ks:
            fs = facts.at(k, allow)
            for f in fs:
                assert f["kth"] == 0.0 and f["n_gt"] == top and f["plateau"] == zeros and f["need_eq"] == k - top, f
                assert f["pos_zero"] > 0 and f["neg_zero"] > 0 and f["pos_zero"] + f["neg_zero"] == zeros, f
            # a -0.0 row below the lowest +0.0 row that the order of f2key would take: for some query at the plateau's first place
            # (the lowest zero row is +0.0 for every second query), for every query a few places in; at the last place every zero
            # is taken and the ids agree either way
            if k < top + zeros:
                assert any(f["key_order_differs"] for f in fs), fs
            if top + 6 <= k < top + zeros:
                assert all(f["key_order_differs"] for f in fs), fs
            for nq in (1, 5, 6):
                st, got, want = _check(oracle, ix, corpus, queries[:nq], k, allow, path=1, what=f"{name} mask={mask}")
                if name == "zeros_3000" and mask is None and k == 10 and nq == 1:
                    print(f"\n{name} k=10: gpu ids {got[1][0].tolist()} oracle ids {want[1][0].tolist()} "
                          f"gpu scores {got[0][0].tolist()} (+0.0 rows {f['pos_zero']}, -0.0 rows {f['neg_zero']})")
    ix.close()


# ---- 2. signed zeros behind the MFMA scan --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [8, 200])
@pytest.mark.parametrize("plateau", [40, 1500])
def test_signed_zeros_behind_the_mfma_scan(eng, oracle, plateau, B):
    """40 000 rows: 4 positives, a zero plateau of mixed sign, everything else near -0.66; k = 10 ends inside the plateau.
    40 zeros: the ordinary ending of k_refine (rank_and_write over the whole band). 1 500 zeros: the band is wider than REFINE_PMAX,
    the in-place ending runs (exact_queries == 0, rescored > 1024) — its k-th key is a zero, and the 1 500 rows that tie there are
    more than the ranking arrays hold: the lowest rows among them are selected by row id. B = 8 and 200: the two bootstrap forms."""
    corpus, q8, facts = SL.mfma_zeros(oracle, 40_000, plateau, nq=8)
    for f in facts.at(10):
        assert f["kth"] == 0.0 and f["n_gt"] == 4 and f["plateau"] == plateau and f["key_order_differs"], f
        assert min(f["pos_zero"], f["neg_zero"]) > plateau // 3, f
    assert (plateau > SL.REFINE_PMAX) == (plateau == 1500)
    q = q8[np.arange(B) % 8]
    ix = _index(eng, corpus, force_fast=1)
    st, _, _ = _check(oracle, ix, corpus, q, 10, path=0, what=f"mfma plateau {plateau}")
    print(f"\nplateau {plateau} B {B}: {st}")
    if plateau > SL.REFINE_PMAX:
        assert st["exact_queries"] == 0 and st["rescored"] > 1024, st
    ix.close()


@pytest.mark.parametrize("pilot", [0, 4])
def test_signed_zeros_behind_the_int8_scan(eng, oracle, pilot):
    """the 1 500-zero landscape at B = 300 on the int8 scan, one band (refine_pilot 0) and two rounds (4). d = 128, not 64: the
    int8 scan's shape gate wants the padded dimension to be a multiple of 128 (rdx_index.hip, i8_shape)."""
    corpus, q8, facts = SL.mfma_zeros(oracle, 40_000, 1500, nq=8, d=128)
    for f in facts.at(10):
        assert f["kth"] == 0.0 and f["n_gt"] == 4 and f["plateau"] == 1500 and f["key_order_differs"], f
    q = q8[np.arange(300) % 8]
    ix = _index(eng, corpus, before_add=[("coarse_i8", 1), ("refine_pilot", pilot)], force_fast=1)
    st, _, _ = _check(oracle, ix, corpus, q, 10, path=0, what=f"int8 pilot {pilot}")
    print(f"\nint8 pilot {pilot}: {st}")
    assert st["coarse_bits"] == 8, st
    ix.close()


# ---- 3. plateau sizes at the k-th place on the exact path -----------------------------------------------------------------------------

@pytest.mark.parametrize("level", [0.35, -0.35])
@pytest.mark.parametrize("n", SL.PLATEAU_ROWS)
def test_plateau_sizes_at_the_kth_place(eng, oracle, n, level):
    """plateaus of 1, 2, 1023, 1024, 1025 and 3000 identical scores around EQ_CAP = 1024, k-th place at depth 1, size / 2 and size
    of the plateau; the plateau's rows at high row ids, every second row of the corpus' tail; 32 768 rows (registers), 32 769
    (global) and 20 011 (a ragged last chunk of 1024); positive and negative plateau level."""
    for size in SL.PLATEAU_SIZES:
        corpus, queries, facts = SL.plateau_at_kth(oracle, n, size, level)
        ix = _index(eng, corpus, force_exact=1)
        for e in SL.need_eqs(size):
            f = facts.at(7 + e)[0]
            assert (f["n_gt"], f["plateau"], f["need_eq"]) == (7, size, e) and (f["kth"] < 0) == (level < 0), (size, e, f)
            assert f["rows"][-1] >= n - 2 * size                     # the k-th row sits in the corpus' tail
            _check(oracle, ix, corpus, queries, 7 + e, path=1, what=f"plateau n={n} size={size} level={level}")
        ix.close()


# ---- 4. k range on the exact path ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [5000, 40_000])
def test_k_range_through_tie_groups(eng, oracle, n):
    """k = 1 .. SELECT_MAX_K over many small tie groups (register form at 5 000 rows, global form at 40 000); k above what a bitmap
    leaves: the k-th key is -inf and the tie walk runs over masked entries; an all-zero bitmap"""
    corpus, queries, facts = SL.tie_groups(oracle, n)
    assert np.unique(facts.scores[0]).shape[0] < 0.6 * n             # many tie groups
    ix = _index(eng, corpus, force_exact=1)
    for k in SL.K_RANGE:
        assert k <= SL.SELECT_MAX_K
        _check(oracle, ix, corpus, queries, k, path=1, what=f"ties n={n}")
    assert any(f["plateau"] > 1 for k in SL.K_RANGE for f in facts.at(k))   # a k-th place inside a tie group
    m = SL.masks(n)
    f = facts.at(257, m["few"])[0]
    assert f["valid"] == 100 and f["kk"] == 100                      # fewer allowed rows than k
    st, got, _ = _check(oracle, ix, corpus, queries, 257, m["few"], path=1, what=f"ties n={n} few")
    assert (got[2] == 100).all()
    st, got, _ = _check(oracle, ix, corpus, queries, 10, m["none"], what=f"ties n={n} none")
    assert (got[2] == 0).all()
    ix.close()


def test_k_above_the_row_count_and_the_largest_k(eng, oracle):
    corpus, queries, facts = SL.tie_groups(oracle, 3000)
    ix = _index(eng, corpus, force_exact=1)
    assert facts.at(SL.SELECT_MAX_K)[0]["kk"] == 3000
    st, got, _ = _check(oracle, ix, corpus, queries, SL.SELECT_MAX_K, path=1, what="k above the row count")
    assert (got[2] == 3000).all()
    # rdx_search's argument check: "k larger than SELECT_MAX_K is not supported" -> RDX_ERR_INVALID (ValueError in _lib.check)
    with pytest.raises(ValueError):
        ix.search(queries, SL.SELECT_MAX_K + 1)
    ix.close()
    corpus, queries, facts = SL.tie_groups(oracle, 5000, d=256)      # d = 256: four times the row bytes per K5a wave
    ix = _index(eng, corpus, force_exact=1)
    _check(oracle, ix, corpus, queries, 257, path=1, what="ties d=256")
    ix.close()


# ---- 5. all-negative and mixed lists ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,opt,path", [(5000, "force_exact", 1), (40_000, "force_exact", 1), (40_000, "force_fast", 0)])
def test_negative_and_crossing_lists(eng, oracle, n, opt, path):
    """every row on the far side of the query (the whole list negative, ties among the negatives), and a list that runs from
    positive through -0.0 and +0.0 rows (the -0.0 rows at the lower ids) into the negatives; exact and MFMA path"""
    corpus, queries, facts = SL.negatives(oracle, n)
    for k in (10, 200):
        for f in facts.at(k):
            assert f["negative_in_list"] == k and f["pos_zero"] == 0 and f["neg_zero"] == 0, f
    assert np.unique(facts.scores[0]).shape[0] <= n // 2             # ties among the negatives
    ix = _index(eng, corpus, **{opt: 1})
    for k in (10, 200):
        _check(oracle, ix, corpus, queries, k, path=path, what=f"negatives n={n} {opt}")
    ix.close()
    corpus, queries, facts = SL.negatives(oracle, n, crossing=True)
    f = facts.at(12)[0]
    assert (f["pos_zero"], f["neg_zero"], f["negative_in_list"], f["n_gt"]) == (3, 3, 3, 9) and f["key_order_differs"], f
    assert facts.at(4)[0]["kth"] == 0.0 and facts.at(8)[0]["kth"] == 0.0 and facts.at(8)[0]["key_order_differs"]
    ix = _index(eng, corpus, **{opt: 1})
    for k in (4, 8, 12, 200):
        _check(oracle, ix, corpus, queries, k, path=path, what=f"crossing n={n} {opt}")
    ix.close()


# ---- 6. merges ---------------------------------------------------------------------------------------------------------------------------

def _merge_inputs(oracle, P, k, nq):
    """part lists cut from a landscape's per-shard answers (rows dealt round-robin): signed zeros and plateaus spread over the
    parts, negative tails; then counts of 0, k / 2, and values outside [0, k] (the kernels clamp them)"""
    if k >= 64:
        corpus, queries, _ = SL.mfma_zeros(oracle, 40_000, 1500, nq=5)
    else:                                                            # short lists: the crossing rows reach every part's top
        corpus, queries, _ = SL.negatives(oracle, 40_000, nq=5, crossing=True)
    assert corpus.shape[0] // P >= k
    ps, pr, pc = SL.shard_parts(oracle, corpus, queries, P, k)
    assert (pc == k).all() and ((ps == 0) & np.signbit(ps)).any() and ((ps == 0) & ~np.signbit(ps)).any() and (ps < 0).any()
    if nq != 5:
        reps = -(-nq // 5)
        ps, pr, pc = (np.tile(a, (1, reps) + (1,) * (a.ndim - 2))[:, :nq].copy() for a in (ps, pr, pc))
    if nq == 1:
        pc[P - 1, 0] = k + 5                                         # above k: means k
    else:
        pc[0, 0] = 0                                                 # an empty part
        pc[P - 1, 1] = k + 5                                         # above k: means k
        pc[P // 2, 2] = -3                                           # below 0: means 0
        pc[0, 3] = k // 2                                            # a truncated list
        pc[:, 4] = 0                                                 # nothing at all
    return ps, pr, pc, np.clip(pc, 0, k).astype(np.int32)


@pytest.mark.parametrize("P,k,nq", [(64, 64, 5), (8, 512, 5), (2, 2048, 1), (1, 4096, 5), (5, 7, 5000), (5, 7, 1),
                                    (2, 2049, 5), (3, 1366, 1)])
def test_merge_of_landscape_parts(eng, oracle, P, k, nq):
    """rdx_merge_topk: one k_merge launch up to n_parts * k = MERGE_MAX exactly, the pairwise fold (k_merge_pair) from 4097 on"""
    assert (P * k <= SL.MERGE_MAX) == ((P, k) not in [(2, 2049), (3, 1366)])
    ps, pr, pc, clamped = _merge_inputs(oracle, P, k, nq)
    want = oracle.merge_topk(ps, pr, clamped, k)
    got = eng.merge_topk(ps, pr, pc, k)
    _same(got, want, f"merge P={P} k={k} nq={nq}")
    np.testing.assert_array_equal(want[2], np.minimum(clamped.sum(axis=0), k))


@pytest.mark.parametrize("P,k,nq", [(64, 64, 5), (8, 512, 5), (1, 4096, 5), (5, 7, 5), (5, 7, 5000), (5, 7, 1)])
def test_packed_merge_of_landscape_parts(eng, oracle, P, k, nq):
    """rdx_merge_topk_packed over the all-gather layout (rows | scores | counts | flags per part), up to n_parts * k = MERGE_MAX"""
    import ctypes
    import torch
    from rag_dpo_amd import _lib as L
    from rag_dpo_amd.sharded import ShardedSearcher, packed_bytes
    lib = L.load()
    ps, pr, pc, clamped = _merge_inputs(oracle, P, k, nq)
    want = oracle.merge_topk(ps, pr, clamped, k)
    stride = (packed_bytes(nq, k) + 15) // 16 * 16
    buf = torch.zeros(P * stride, dtype=torch.uint8, device="cuda")
    parts = [ShardedSearcher.views(buf[p * stride:(p + 1) * stride], nq, k) for p in range(P)]
    for p in range(P):
        parts[p][0].copy_(torch.from_numpy(ps[p])); parts[p][1].copy_(torch.from_numpy(pr[p])); parts[p][2].copy_(torch.from_numpy(pc[p]))
    os_ = torch.empty((nq, k), dtype=torch.float32, device="cuda"); or_ = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    oc = torch.empty((nq,), dtype=torch.int32, device="cuda")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(lib.rdx_merge_topk_packed(0, ptr(buf), stride, P, nq, k, ptr(os_), ptr(or_), ptr(oc), None, stream))
    torch.cuda.synchronize()
    _same((os_.cpu().numpy(), or_.cpu().numpy(), oc.cpu().numpy()), want, f"packed merge P={P} k={k} nq={nq}")


def test_packed_merge_refuses_more_than_merge_max(eng):
    """n_parts * k = 4097 = 17 * 241: the packed merge has no fold, rdx_merge_topk_packed states RDX_ERR_INVALID"""
    import ctypes
    import torch
    from rag_dpo_amd import _lib as L
    from rag_dpo_amd.sharded import packed_bytes
    lib = L.load()
    P, k, nq = 17, 241, 2
    assert P * k == SL.MERGE_MAX + 1
    stride = (packed_bytes(nq, k) + 15) // 16 * 16
    buf = torch.zeros(P * stride, dtype=torch.uint8, device="cuda")
    os_ = torch.empty((nq, k), dtype=torch.float32, device="cuda"); or_ = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    oc = torch.empty((nq,), dtype=torch.int32, device="cuda")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    with pytest.raises(ValueError):
        L.check(lib.rdx_merge_topk_packed(0, ptr(buf), stride, P, nq, k, ptr(os_), ptr(or_), ptr(oc), None, stream))
    torch.cuda.synchronize()


# ---- 7. one index against shards -----------------------------------------------------------------------------------------------------

def test_shards_equal_one_index_on_the_zero_plateau(eng, oracle):
    """the 40 000-row landscape through MultiDeviceIndex with three HipIndex shards on device 0, rows dealt round-robin in pieces of
    100 (batches of 300: the water-filling cuts each into one piece per shard): per-shard selection, set_row_ids and the merge on
    the same edge together == one HipIndex == the oracle, on the MFMA and on the exact path"""
    from rag_dpo_amd.multi_device import MultiDeviceIndex
    corpus, queries, facts = SL.mfma_zeros(oracle, 40_000, 1500, nq=8)
    for f in facts.at(10):
        assert f["kth"] == 0.0 and f["key_order_differs"], f
    md, one = MultiDeviceIndex(64, [0, 0, 0]), eng.HipIndex(64)
    for a in range(0, 40_000, 300):
        md.add(corpus[a:a + 300])
    one.add(corpus)
    sizes = [len(s) for s in md._shards]
    assert sum(sizes) == 40_000 and max(sizes) - min(sizes) <= 2, sizes
    assert md._dev_of[:300].tolist() == [0] * 100 + [1] * 100 + [2] * 100
    want = {k: oracle.cosine_topk(oracle.normalize_rows(corpus), queries, k) for k in (10, 300)}
    for opt in ("force_fast", "force_exact"):
        for ix in (one, md):
            ix.set_option(opt, 1)
        for k in (10, 300) if opt == "force_exact" else (10,):
            _same(one.search(queries, k), want[k], f"one index {opt} k={k}")
            _same(md.search(queries, k), want[k], f"three shards {opt} k={k}")
        for ix in (one, md):
            ix.set_option(opt, 0)
    md.close(); one.close()
