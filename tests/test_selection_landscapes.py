"""CPU: the reference order itself on the selection landscapes (tests/selection_landscapes.py), and the kernels' edges they aim at.

oracle.cosine_topk (heap + qsort over `before`, oracle/rdx_oracle.c) must equal an independent numpy restatement of the documented
order — np.lexsort((rows, -scores)) over the oracle's own scores, masked rows removed — on every landscape the GPU tests run:
ids and counts, signed zeros included (lexsort compares floats: the two zeros tie, the row id decides). A second test reads the
selectors' constants out of the sources: a kernel change that moves an edge fails here instead of un-aiming the GPU tests."""
import os
import re

import numpy as np
import pytest

import selection_landscapes as SL

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rag_dpo_amd", "csrc")
CAT = SL.catalogue()


@pytest.mark.parametrize("name", sorted(CAT))
def test_oracle_order_equals_lexsort(oracle, name):
    build, cases = CAT[name]
    corpus, queries, facts = build(oracle)
    n = corpus.shape[0]
    ch = oracle.normalize_rows(corpus)
    m = SL.masks(n)
    rows = np.arange(n, dtype=np.int64)
    for k, mask in cases:
        allow = m[mask]
        es, er, ec = oracle.cosine_topk(ch, queries, k, allow)
        keep = rows if allow is None else rows[allow]
        for b in range(queries.shape[0]):
            want = SL.order_documented(facts.scores[b, keep], keep)[:k]
            assert ec[b] == want.shape[0], (name, k, mask, b)
            np.testing.assert_array_equal(er[b, :ec[b]], want, err_msg=f"{name} k={k} mask={mask} query {b}")
            np.testing.assert_array_equal(es[b, :ec[b]].view(np.uint32), facts.scores[b, want].view(np.uint32))
            assert (er[b, ec[b]:] == -1).all() and np.isneginf(es[b, ec[b]:]).all()


def test_landscapes_hold_what_they_are_built_for(oracle):
    """the headline landscapes, against the figures they were designed to (the GPU tests assert their own preconditions as well)"""
    _, _, facts = SL.signed_zeros(oracle, 3000, nq=2)
    f = facts.at(10)[0]
    assert (f["n_gt"], f["pos_zero"], f["neg_zero"], f["plateau"], f["need_eq"]) == (4, 1563, 1433, 2996, 6)
    assert f["kth"] == 0.0 and f["key_order_differs"]
    np.testing.assert_array_equal(f["rows"], [143, 653, 1474, 1969, 0, 1, 2, 3, 4, 5])
    np.testing.assert_array_equal(SL.order_by_keys(facts.scores[0], np.arange(3000))[:10], [143, 653, 1474, 1969, 0, 1, 2, 9, 10, 11])
    f = facts.at(10)[1]                                   # the flipped query: every zero changes its sign
    assert (f["pos_zero"], f["neg_zero"]) == (1433, 1563) and f["key_order_differs"]
    for plateau in (40, 1500):
        _, _, facts = SL.mfma_zeros(oracle, 40_000, plateau, nq=2)
        for f in facts.at(10):
            assert f["n_gt"] == 4 and f["plateau"] == plateau and f["kth"] == 0.0 and f["key_order_differs"]
            assert f["pos_zero"] + f["neg_zero"] == plateau and min(f["pos_zero"], f["neg_zero"]) > plateau // 3
    for size in SL.PLATEAU_SIZES:
        for level in (0.35, -0.35):
            _, _, facts = SL.plateau_at_kth(oracle, SL.REG_ROWS + 1, size, level)
            for e in SL.need_eqs(size):
                f = facts.at(7 + e)[0]
                assert (f["n_gt"], f["plateau"], f["need_eq"]) == (7, size, e), (size, level, e, f)
                assert (f["kth"] < 0) == (level < 0)
    _, _, facts = SL.negatives(oracle, 5000, crossing=True)
    f = facts.at(12)[0]
    assert f["pos_zero"] == 3 and f["neg_zero"] == 3 and f["negative_in_list"] == 3 and f["key_order_differs"]
    f = SL.negatives(oracle, 5000)[2].at(200)[0]
    assert f["negative_in_list"] == 200 and f["plateau"] >= 1


@pytest.mark.parametrize("name,file,value", [("EQ_CAP", "k_rows.hpp", SL.EQ_CAP), ("RN", "k_rows.hpp", SL.RN),
                                             ("SELECT_MAX_K", "rows_core.hpp", SL.SELECT_MAX_K),
                                             ("REFINE_PMAX", "rdx_limits.hpp", SL.REFINE_PMAX),
                                             ("MERGE_MAX", "merge_kernel.hpp", SL.MERGE_MAX)])
def test_selector_constants_are_where_the_landscapes_aim(name, file, value):
    src = open(os.path.join(CSRC, file)).read()
    found = re.findall(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", src)
    assert found == [str(value)], (name, file, found)
    assert (SL.EQ_CAP, SL.RN, SL.SELECT_MAX_K, SL.REFINE_PMAX, SL.MERGE_MAX, SL.REG_ROWS) == (1024, 32, 4096, 1024, 4096, 32768)
    # the sizes around the edges are really in the catalogue
    assert {SL.EQ_CAP - 1, SL.EQ_CAP, SL.EQ_CAP + 1} <= set(SL.PLATEAU_SIZES)
    assert {SL.REG_ROWS, SL.REG_ROWS + 1} <= set(SL.PLATEAU_ROWS) and any(n % 1024 for n in SL.PLATEAU_ROWS)
    assert {SL.SELECT_MAX_K - 1, SL.SELECT_MAX_K} <= set(SL.K_RANGE)
