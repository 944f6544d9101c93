"""GPU: the lexical score of named (question, row) pairs (rag_dpo_amd.engine.lex_score_pairs -> rdx_lex_score_pairs ->
k_lex_score_pairs) on bits (uint64) against rag_dpo_amd/lexical.py's ModelLexical / score_model, against the numpy
restatement of the call (m3.sparse_pairs_model) and against what rdx_lex_search returns for the same (question, row)."""
import ctypes

import numpy as np
import pytest
import torch

import lexical_world as LW
from rag_dpo_amd import lexical as LX
from rag_dpo_amd import m3 as M3

pytestmark = pytest.mark.gpu

TILE = 4096


def u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def call(hip, queries, pq, pr):
    from rag_dpo_amd import engine as E
    off, ids, w = LW.pack(queries)
    dev = torch.device("cuda", hip.device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    off_p = torch.from_numpy(off).pin_memory()
    out = E.lex_score_pairs(hip, off_p, up(ids), up(w), up(np.asarray(pq, np.int32)), up(np.asarray(pr, np.int64)))
    return out.cpu().numpy()


def all_pairs(nq, rows):
    return np.repeat(np.arange(nq, dtype=np.int32), rows), np.tile(np.arange(rows, dtype=np.int64), nq)


def check_against_everything(arrays, queries, pq, pr):
    """the call's bits = ModelLexical's score of (question, row) = the numpy restatement = rdx_lex_search's where it lists the row"""
    hip, model = LX.HipLexical(arrays), LX.ModelLexical(arrays)
    try:
        got = call(hip, queries, pq, pr)
        table = np.stack([model.scores(ids, w) for ids, w in queries])         # [nq][rows] float64
        want = table[np.asarray(pq), np.asarray(pr)]
        assert np.array_equal(u64(got), u64(want))
        off, ids, w = LW.pack(queries)
        assert np.array_equal(u64(got), u64(M3.sparse_pairs_model(arrays, off, ids, w, pq, pr)))
        k = min(arrays.n_rows, TILE)
        sc, ro, cn = hip.search(off, ids, w, k, None, None)
        listed = np.zeros_like(table)
        for b in range(len(queries)):
            listed[b, ro[b, :cn[b]]] = sc[b, :cn[b]]
        if arrays.n_rows <= TILE:                                               # the search lists every row with a score above 0
            assert np.array_equal(u64(got), u64(listed[np.asarray(pq), np.asarray(pr)]))
        else:
            seen = listed[np.asarray(pq), np.asarray(pr)] > 0
            assert np.array_equal(u64(got[seen]), u64(listed[np.asarray(pq), np.asarray(pr)][seen]))
        return got
    finally:
        hip.close()


def test_a_dense_corpus_every_pair():
    arrays = LW.dense_corpus(70, 40, seed=70)
    qs = [LW.query(40, n, seed=n) for n in (1, 7, 40)] + [(np.zeros(0, np.int32), np.zeros(0, np.float16))]
    pq, pr = all_pairs(len(qs), 70)
    got = check_against_everything(arrays, qs, pq, pr)
    assert (u64(got[pq == 3]) == 0).all()                                       # a question without terms: +0.0, not -0.0, not NaN
    for n in (1, 3, 4, 5, 64, 65, 1000):                                        # around a workgroup of four waves, and many of them
        rng = np.random.default_rng(n)
        a, b = rng.integers(0, len(qs), n).astype(np.int32), rng.integers(0, 70, n).astype(np.int64)
        sub = check_against_everything(arrays, qs, a, b)
        assert np.array_equal(u64(sub), u64(got.reshape(len(qs), 70)[a, b]))    # a pair's bits do not depend on the call it is in


def test_the_directory_tile_edge():
    n = TILE + 4                                                                # 4 100 rows: two tiles
    arrays = LW.dense_corpus(n, 12, seed=4100)
    qs = [LW.query(12, k, seed=40 + k) for k in (1, 5, 12)]
    qs = [(np.union1d(ids, [0]).astype(np.int32), np.resize(w, len(np.union1d(ids, [0])))) for ids, w in qs]   # term 0 is in every question
    rows = [0, 1, TILE - 2, TILE - 1, TILE, TILE + 1, TILE + 3]
    pq, pr = np.repeat(np.arange(3, dtype=np.int32), len(rows)), np.tile(np.asarray(rows, np.int64), 3)
    got = check_against_everything(arrays, qs, pq, pr)
    assert (got > 0).all()                                                      # term 0 is in every row: both tiles' entries were found


def test_question_lengths_up_to_the_limit():
    vocab, rows = 5000, 9
    rng = np.random.default_rng(5)
    has = rng.random((vocab, rows)) < 0.3
    terms, rws = np.nonzero(has)
    arrays = LW.arrays_from_triples(rows, vocab, terms, rws, (rng.integers(1, 64, terms.size) / 16.0).astype(np.float16))
    qs = [LW.query(vocab, n, seed=n) for n in (0, 1, 63, 64, 65, 4096)]
    pq, pr = all_pairs(len(qs), rows)
    check_against_everything(arrays, qs, pq, pr)
    hip = LX.HipLexical(arrays)
    try:
        with pytest.raises(ValueError, match="4097 terms"):
            call(hip, qs + [LW.query(vocab, 4097, seed=1)], [0], [0])
        # a fault in the first lane of the second round of 64 terms (it is compared with the term before it), and in its last lane
        ids, w = LW.query(vocab, 128, seed=3)
        twice, neg = ids.copy(), w.copy()
        twice[64] = twice[63]
        neg[127] = -neg[127]
        got = call(hip, [(ids, w), (twice, w), (ids, neg)], [0, 1, 2, 0], [4, 4, 4, 4])
        assert np.isnan(got[1:3]).all() and got[0] == got[3] == LX.ModelLexical(arrays).scores(ids, w)[4]
    finally:
        hip.close()


def test_posting_lists_of_every_length_with_the_row_first_last_and_absent():
    n = 2 * TILE + 10
    long_rows = np.arange(3, n, 3)                                              # a long list over three tiles; rows 3 .. are in it
    lists = {0: [], 1: [5], 2: [5, TILE + 7], 3: long_rows.tolist(), 4: [0, n - 1], 5: list(range(TILE - 1, TILE + 2))}
    terms = np.concatenate([np.full(len(v), t) for t, v in lists.items()]).astype(np.int64)
    rws = np.concatenate([np.asarray(v, np.int64) for v in lists.values()])
    w = (np.random.default_rng(8).integers(1, 64, terms.size) / 16.0).astype(np.float16)
    arrays = LW.arrays_from_triples(n, 7, terms, rws, w)                        # term 6 has no postings either
    qs = [(np.arange(7, dtype=np.int32), (np.arange(1, 8) / 4.0).astype(np.float16)), (np.array([3], np.int32), np.array([1.5], np.float16)),
          (np.array([0, 6], np.int32), np.array([1.0, 2.0], np.float16))]
    rows = [0, 1, 3, 4, 5, 6, TILE - 1, TILE, TILE + 1, TILE + 7, TILE + 8, int(long_rows[-1]), n - 2, n - 1]
    pq, pr = np.repeat(np.arange(3, dtype=np.int32), len(rows)), np.tile(np.asarray(rows, np.int64), 3)
    got = check_against_everything(arrays, qs, pq, pr).reshape(3, len(rows))
    assert (u64(got[2]) == 0).all()                                             # only terms without postings: +0.0 everywhere
    assert got[1, rows.index(3)] > 0 and got[1, rows.index(int(long_rows[-1]))] > 0 and got[1, rows.index(4)] == 0   # first, last, absent between
    assert got[0, rows.index(0)] > 0 and got[0, rows.index(n - 1)] > 0 and got[0, rows.index(1)] == 0


def test_the_order_probe():
    """three terms in ascending id whose products are [2^-22, 2^-22, 65504^2]: fp16 2^-11, 2^-11 and 65504 on both sides, the question's
    and the chunk's. Ascending: (2^-22 + 2^-22) + 65504^2 = 0x1.ff80080000001p+31, one ulp (2^-21) above the big product; reversed, each
    2^-22 is half an ulp of the big product, a tie that goes to even: 0x1.ff80080000000p+31."""
    small, big = np.float16(2.0 ** -11), np.float16(65504.0)
    asc, rev = float.fromhex("0x1.ff80080000001p+31"), float.fromhex("0x1.ff80080000000p+31")
    # checked here in numpy first
    p = [float(small) * float(small), float(small) * float(small), float(big) * float(big)]
    assert (p[0] + p[1]) + p[2] == asc and (p[2] + p[1]) + p[0] == rev and asc != rev
    arrays = LW.arrays_from_triples(TILE + 2, 40, [10, 20, 30, 10, 20, 30], [7, 7, 7, TILE + 1, TILE + 1, TILE + 1], [small, small, big] * 2)
    qs = [(np.array([10, 20, 30], np.int32), np.array([small, small, big], np.float16))]
    off, ids, wq = LW.pack(qs)
    assert LX.ModelLexical(arrays).scores(ids, wq)[7] == asc and LX.ModelLexical(arrays, order=-1).scores(ids, wq)[7] == rev
    assert LX.score_model(ids, wq, [10, 20, 30], [small, small, big]) == asc
    got = check_against_everything(arrays, qs, [0, 0, 0], [7, TILE + 1, 8])
    assert got.tolist() == [asc, asc, 0.0]


def test_bad_questions_and_pairs_get_nan_and_leave_their_neighbours():
    arrays = LW.dense_corpus(70, 40, seed=1)
    good = LW.query(40, 9, seed=2)
    w9 = good[1]
    h = lambda bits: np.array([bits], np.uint16).view(np.float16)[0]   # noqa: E731
    qs = [good,
          (np.array([3, 3, 5], np.int32), w9[:3]),                              # not strictly ascending (equal)
          (np.array([5, 3], np.int32), w9[:2]),                                 # descending
          (np.array([1, 40], np.int32), w9[:2]),                                # an id outside [0, n_terms)
          (np.array([-1, 2], np.int32), w9[:2]),
          (np.array([1, 2], np.int32), np.array([1.0, h(0x0000)], np.float16)),  # weight bits 0
          (np.array([1, 2], np.int32), np.array([h(0x7C00), 1.0], np.float16)),  # inf
          (np.array([1, 2], np.int32), np.array([1.0, h(0x8001)], np.float16)),  # negative
          (np.concatenate([np.arange(0, 39), [39, 39]]).astype(np.int32), np.resize(w9, 41)),   # the fault is the last of 41 terms
          good]
    hip, model = LX.HipLexical(arrays), LX.ModelLexical(arrays)
    try:
        pq, pr = all_pairs(len(qs), 70)
        got = call(hip, qs, pq, pr).reshape(len(qs), 70)
        want = model.scores(*good)
        assert np.array_equal(u64(got[0]), u64(want)) and np.array_equal(u64(got[9]), u64(want))
        assert np.isnan(got[1:9]).all()
        off, ids, w = LW.pack(qs)
        assert np.array_equal(u64(got.reshape(-1)), u64(M3.sparse_pairs_model(arrays, off, ids, w, pq, pr)))
        # pairs out of range, among good ones
        pq = np.array([0, -1, 0, len(qs), 0, 0, 9], np.int32)
        pr = np.array([0, 3, -1, 3, 70, 2 ** 40, 69], np.int64)
        got = call(hip, qs, pq, pr)
        assert np.isnan(got[1:6]).all() and got[0] == want[0] and got[6] == want[69]
    finally:
        hip.close()


def test_limits_and_refusals():
    from rag_dpo_amd import _lib as L
    arrays = LW.dense_corpus(70, 40, seed=1)
    hip = LX.HipLexical(arrays)
    try:
        dev = torch.device("cuda", hip.device)
        off = torch.tensor([0, 2], dtype=torch.int64).pin_memory()
        ids = torch.tensor([1, 2], dtype=torch.int32, device=dev)
        w = torch.tensor([1.0, 2.0], dtype=torch.float16, device=dev)
        pq, pr = torch.zeros(4, dtype=torch.int32, device=dev), torch.zeros(4, dtype=torch.int64, device=dev)
        out = torch.full((4,), 7.0, dtype=torch.float64, device=dev)
        p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
        f = hip._lib.rdx_lex_score_pairs
        for nq, n in ((1, 0), (1, (1 << 20) + 1), (0, 4), (65536, 4)):
            assert f(hip._h, p(off), p(ids), p(w), nq, p(pq), p(pr), n, p(out), None) == L.RDX_ERR_INVALID, (nq, n)
        assert f(None, p(off), p(ids), p(w), 1, p(pq), p(pr), 4, p(out), None) == L.RDX_ERR_INVALID
        off_d = off.cuda()
        assert f(hip._h, p(off_d), p(ids), p(w), 1, p(pq), p(pr), 4, p(out), None) == L.RDX_ERR_INVALID          # a shape array lies in pinned host memory
        dec = torch.tensor([2, 0], dtype=torch.int64).pin_memory()
        assert f(hip._h, p(dec), p(ids), p(w), 1, p(pq), p(pr), 4, p(out), None) == L.RDX_ERR_INVALID            # decreasing offsets
        torch.cuda.synchronize()
        assert out.cpu().tolist() == [7.0] * 4                                   # nothing was launched
        assert f(hip._h, p(off), p(ids), p(w), 1, p(pq), p(pr), 4, p(out), None) == L.RDX_OK
        torch.cuda.synchronize()
        assert out.cpu().tolist() == [float(LX.ModelLexical(arrays).scores(np.array([1, 2]), np.array([1.0, 2.0], np.float16))[0])] * 4
    finally:
        hip.close()
