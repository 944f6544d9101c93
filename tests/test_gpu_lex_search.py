"""GPU: rdx_lex_create / rdx_lex_search (HipLexical; csrc/bm25_kernel.hpp k_lex_score + k_bm25_merge) against the model engine of
rag_dpo_amd/lexical.py, on bits: scores viewed as uint64, rows, counts, and the 0 / -1 slots past each count."""
import numpy as np
import pytest

import lexical_world as LW
from rag_dpo_amd import lexical as LX

pytestmark = pytest.mark.gpu

TILE = 4096


def both(arrays):
    return LX.HipLexical(arrays), LX.ModelLexical(arrays)


def check(arrays, queries, k, sets=None, qf=None):
    hip, model = both(arrays)
    off, ids, w = LW.pack(queries)
    got = hip.search(off, ids, w, k, sets, qf)
    LW.same_bits(got, model.search(off, ids, w, k, sets, qf))
    hip.close()
    return got


@pytest.mark.parametrize("rows", [1, 4095, 4096, 4097, 8193])
def test_every_row_of_a_dense_corpus(rows):
    groups = 3 if rows > TILE else 0                      # more rows than k can return: three filtered searches cover them all
    arrays = LW.dense_corpus(rows, 40, seed=rows, groups=groups)
    qs = [LW.query(40, n, seed=10 * rows + n) for n in (1, 7, 40)]
    qs[0] = (np.array([0], np.int32), qs[0][1])           # term 0 is in every row
    qs[1] = (np.union1d(qs[1][0], [0]).astype(np.int32), np.resize(qs[1][1], len(np.union1d(qs[1][0], [0]))))
    for k in (1, min(rows, TILE)):
        if not groups:
            sc, ro, cn = check(arrays, qs, k)
            assert cn.tolist() == [k] * 3
            continue
        sets = np.array([[1], [2], [4]], np.uint32)
        seen = []
        for f in range(3):
            sc, ro, cn = check(arrays, qs, k, sets, np.full(3, f, np.int32))
            seen.append(ro[0, :cn[0]])
        if k > 1:
            assert sorted(np.concatenate(seen).tolist()) == list(range(rows))          # every row's bits were compared


def test_the_summation_order_in_both_tiles():
    big, sq, sd = 32768.0, 2.0 ** -12, 2.0 ** -11
    terms, rows, w = [], [], []
    for r in (7, TILE + 1):
        terms += [10, 20, 30, 11, 21, 31]
        rows += [r] * 6
        w += [big, sd, sd, sd, sd, big]                   # the big product at the smallest id (10, 20, 30) and at the largest (11, 21, 31)
    arrays = LW.arrays_from_triples(TILE + 4, 40, terms, rows, w)
    qs = [(np.array([10, 20, 30], np.int32), np.array([big, sq, sq], np.float16)), (np.array([11, 21, 31], np.int32), np.array([sq, sq, big], np.float16))]
    sc, ro, cn = check(arrays, qs, 4)
    assert cn.tolist() == [2, 2] and ro[:, :2].tolist() == [[7, TILE + 1]] * 2
    assert sc[0, :2].tolist() == [2.0 ** 30] * 2 and sc[1, :2].tolist() == [2.0 ** 30 + 2.0 ** -22] * 2
    off, ids, wq = LW.pack(qs)
    mutant = LX.ModelLexical(arrays, order=-1).search(off, ids, wq, 4)[0]
    assert mutant[0, 0] != sc[0, 0] and mutant[1, 0] != sc[1, 0]                        # a scorer adding in another order would show


def test_a_plateau_across_the_tile_edge():
    n = 2 * TILE + 1
    arrays = LW.arrays_from_triples(n, 8, [3] * n, np.arange(n), [1.0] * n)
    q = [(np.array([3], np.int32), np.array([0.5], np.float16))]
    for k in (1, TILE - 1, TILE):
        sc, ro, cn = check(arrays, q, k)
        assert cn.tolist() == [k] and ro[0].tolist() == list(range(k)) and (sc[0] == 0.5).all()   # ties by ascending row


def widen(a: LX.LexArrays, extra: int) -> LX.LexArrays:
    """the same index over a vocabulary with `extra` more terms, none of which has a posting"""
    return LX.LexArrays(a.n_rows, a.n_terms + extra, np.concatenate([a.post_off, np.full(extra, a.post_off[-1])]), a.post_row, a.post_w,
                        a.row_group, a.n_groups)


def test_question_lengths_empty_terms_and_no_questions():
    arrays = widen(LW.dense_corpus(500, 300, seed=4), 5)
    qs = [LW.query(300, n, seed=n) for n in (1, 255, 256, 257)]                         # around the 256-term chunk of phase A
    qs.append((np.array([302], np.int32), np.array([1.0], np.float16)))                 # a term with no postings
    qs.append((np.zeros(0, np.int32), np.zeros(0, np.float16)))                         # a question with no terms
    qs.append((np.array([0, 300, 304], np.int32), np.array([1.0, 2.0, 3.0], np.float16)))
    sc, ro, cn = check(arrays, qs, 500)
    assert cn.tolist()[4:] == [0, 0, 500] and (ro[4:6] == -1).all() and (sc[4:6] == 0).all()
    check(arrays, qs[::-1], 10)
    hip = LX.HipLexical(arrays)
    sc, ro, cn = hip.search(np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float16), 5)   # nq == 0
    assert sc.shape == (0, 5) and ro.shape == (0, 5) and cn.shape == (0,)


def test_the_smallest_and_the_largest_products():
    tiny, huge = 2.0 ** -24, 65504.0
    arrays = LW.arrays_from_triples(3, 8, [1, 2, 1, 2], [0, 0, 2, 2], [tiny, huge, huge, tiny])
    qs = [(np.array([1], np.int32), np.array([tiny], np.float16)), (np.array([2], np.int32), np.array([huge], np.float16)),
          (np.array([1, 2], np.int32), np.array([tiny, huge], np.float16))]
    sc, ro, cn = check(arrays, qs, 3)
    assert cn.tolist() == [2, 2, 2]
    assert ro[0, :2].tolist() == [2, 0] and sc[0, :2].tolist() == [huge * tiny, 2.0 ** -48]   # 2^-48 passes score > 0
    assert ro[1, :2].tolist() == [0, 2] and sc[1, :2].tolist() == [huge * huge, huge * tiny]
    assert sc[2, 0] == 2.0 ** -48 + huge * huge


def test_filters():
    rng = np.random.default_rng(8)
    n, G = 5000, 33                                        # two words per set, the last one ragged
    base = LW.dense_corpus(n, 40, seed=8)
    groups = rng.integers(0, G, n).astype(np.int32)
    groups[:40] = np.arange(40) % G
    arrays = LX.LexArrays(n, 40, base.post_off, base.post_row, base.post_w, groups, G)
    sets = np.zeros((5, 2), np.uint32)
    sets[0, 0] = 1 << 31                                   # {31}
    sets[1, 1] = 1                                         # {32}
    sets[2] = [0xFFFFFFFF, 1]                              # all
    sets[4] = [0x0F0F0F0F, 0]                              # (row 3 stays a set of zeros)
    qs = [LW.query(40, 5, seed=s) for s in range(9)]
    qs = [(np.union1d(i, [0]).astype(np.int32), np.resize(w, len(np.union1d(i, [0])))) for i, w in qs]
    qf = np.array([0, 1, -1, 2, 3, 0, 4, -1, 1], np.int32)  # neighbouring questions differ
    sc, ro, cn = check(arrays, qs, 300, sets, qf)
    assert cn[4] == 0 and cn[2] == 300 == cn[3] and 0 < cn[0] < 300 and 0 < cn[1] < 300
    assert set(groups[ro[0, :cn[0]]].tolist()) == {31} and set(groups[ro[1, :cn[1]]].tolist()) == {32}
    check(arrays, qs, TILE, sets, qf)
    check(arrays, qs, 7, None, None)
    check(arrays, qs[:3], 7, sets[:0], np.full(3, -1, np.int32))


def test_more_questions_than_one_launch_holds():
    # 20 tiles at k = 4096: the tile partials of 273 questions fill the 256 MiB workspace, so 276 questions take two launches; the
    # filters differ on either side of the cut
    n, G, nq = 20 * TILE, 4, 276
    arrays = LW.dense_corpus(n, 6, seed=3, groups=G)
    sets = np.array([[0b0001], [0b0110], [0b1000]], np.uint32)
    qs = [LW.query(6, 1 + q % 3, seed=q) for q in range(nq)]
    qf = (np.arange(nq) % 4 - 1).astype(np.int32)
    assert qf[272] != qf[273]
    check(arrays, qs, TILE, sets, qf)


def test_refusals_name_the_query_and_the_value():
    arrays = LW.dense_corpus(100, 40, seed=1, groups=3)
    hip = LX.HipLexical(arrays)
    one = np.array([0, 2], np.int64)
    w2 = np.array([1.0, 1.0], np.float16)
    cases = [
        (one, [7, 5], w2, 3, None, None, "query 0: term id 5 after 7"),
        (one, [5, 5], w2, 3, None, None, "query 0: term id 5 after 5"),
        (np.array([0, 1, 3], np.int64), [1, 9, 8], np.ones(3, np.float16), 3, None, None, "query 1: term id 8 after 9"),
        (one, [5, 7], np.array([1.0, 0.0], np.float16), 3, None, None, "query 0: term id 7 has weight bits 0 "),
        (one, [5, 7], np.array([np.inf, 1.0], np.float16), 3, None, None, "query 0: term id 5 has weight bits 31744"),
        (one, [5, 7], np.array([1.0, np.nan], np.float16), 3, None, None, "query 0: term id 7 has weight bits"),
        (one, [5, 7], np.array([1.0, -1.0], np.float16), 3, None, None, "query 0: term id 7 has weight bits 48128"),
        (one, [5, 40], w2, 3, None, None, r"term id 40 out of \[0, 40\)"),
        (one, [-1, 4], w2, 3, None, None, r"term id -1 out of \[0, 40\)"),
        (one, [5, 7], w2, 0, None, None, r"k = 0\)"),
        (one, [5, 7], w2, 4097, None, None, r"k = 4097\)"),
        (one, [5, 7], w2, 3, np.ones((2, 1), np.uint32), [2], r"query_filter\[0\] = 2 out of \[-1, 2\)"),
        (one, [5, 7], w2, 3, np.ones((2, 1), np.uint32), [-2], r"query_filter\[0\] = -2 out of \[-1, 2\)"),
    ]
    for off, ids, w, k, sets, qf, msg in cases:
        with pytest.raises(ValueError, match=msg):
            hip.search(off, np.array(ids, np.int32), w, k, sets, None if qf is None else np.array(qf, np.int32))
    with pytest.raises(ValueError, match="query 0 has 4097 terms"):
        hip.search(np.array([0, 4097], np.int64), np.zeros(4097, np.int32), np.ones(4097, np.float16), 3)
    # after the refusals the index still answers
    LW.same_bits(hip.search(one, np.array([5, 7], np.int32), w2, 3), LX.ModelLexical(arrays).search(one, np.array([5, 7], np.int32), w2, 3))
    # 4096 terms are admitted
    big = LX.HipLexical(LW.arrays_from_triples(3, 5000, np.arange(0, 5000, 7), np.arange(0, 5000, 7) % 3, np.ones(len(range(0, 5000, 7)), np.float16)))
    sc, ro, cn = big.search(np.array([0, 4096], np.int64), np.arange(4096, dtype=np.int32), np.ones(4096, np.float16), 3)
    assert cn.tolist() == [3]
    import ctypes
    from rag_dpo_amd import _lib as L
    with pytest.raises(ValueError, match="space must be RDX_HOST"):
        z = ctypes.c_void_p(one.ctypes.data)
        L.check(hip._lib.rdx_lex_search(hip._h, z, z, z, 1, 3, None, 0, z, z, z, z, L.RDX_DEVICE, None))


def test_create_refuses_bad_postings():
    good = LW.arrays_from_triples(4, 6, [1, 1, 2], [0, 3, 2], [1.0, 2.0, 3.0])
    LX.HipLexical(good).close()

    def with_(**kw):
        return LX.LexArrays(**{**good.__dict__, **kw})
    with pytest.raises(ValueError, match="term 1: rows must be strictly ascending and < n_rows"):
        LX.HipLexical(with_(post_row=np.array([3, 0, 2], np.int32)))
    with pytest.raises(ValueError, match="term 1: rows must be strictly ascending"):
        LX.HipLexical(with_(post_row=np.array([3, 3, 2], np.int32)))
    with pytest.raises(ValueError, match="term 2: rows must be strictly ascending and < n_rows"):
        LX.HipLexical(with_(post_row=np.array([0, 3, 4], np.int32)))
    for bad in (0.0, np.inf, np.nan, -1.0):
        with pytest.raises(ValueError, match="term 2: a weight that is not a finite fp16 above 0"):
            LX.HipLexical(with_(post_w=np.array([1.0, 2.0, bad], np.float16).view(np.uint16)))
    with pytest.raises(ValueError, match="row_group and n_groups"):
        LX.HipLexical(with_(row_group=np.zeros(4, np.int32), n_groups=0))
