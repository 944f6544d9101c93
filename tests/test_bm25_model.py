"""CPU tests of tests/bm25_model.py, the cases tests/test_gpu_bm25_edges.py replays through the BM25 kernels.

  * the constants the cases aim at are the ones in csrc/bm25_kernel.hpp and csrc/rdx_bm25.hip, read out of the sources: a
    kernel change that moves an edge fails here instead of un-aiming the GPU tests;
  * per case, the branch it is built for is really taken (number of launches, n_tiles > BM25_MERGE_THREADS, a non-positive idf, a
    tile with postings and no passing row, ...), asserted from those constants;
  * where a case is built from token lists (all of them have at most 5000 rows), CpuBm25.scores equals the dense restatement of
    rank_bm25, bm25_oracle.BM25Okapi.get_scores, as int64 bit patterns, on every distinct query of the case; the other cases say
    why they are exempt (idf overridden, written as arrays, or too many rows for the dense loop);
  * every mutant a run names returns (rows, score bits, counts) that differ from the truth on that run's own queries and k —
    which is what shows that the GPU file's bit equality bites there."""
import os
import re

import numpy as np
import pytest

import bm25_model as M
import bm25_oracle as O

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rag_dpo_amd", "csrc")
TILE = M.TILE


def test_constants_are_where_the_cases_aim():
    src = open(os.path.join(CSRC, "bm25_kernel.hpp")).read()
    for name, value in (("BM25_TILE", M.TILE), ("BM25_THREADS", M.THREADS), ("BM25_TERM_CHUNK", M.TERM_CHUNK),
                        ("BM25_MAX_TERMS", M.MAX_TERMS), ("BM25_MAX_K", M.MAX_K), ("BM25_MERGE_THREADS", M.MERGE_THREADS),
                        ("BM25_MERGE_CAP", M.MERGE_CAP)):
        found = re.findall(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", src)
        assert found == [str(value)], (name, found)
    assert (M.TILE, M.TERM_CHUNK, M.MAX_K, M.MERGE_THREADS, M.MERGE_CAP) == (4096, 256, 4096, 512, 8192)
    host = re.sub(r"\s+", " ", open(os.path.join(CSRC, "rdx_bm25.hip")).read())
    # bytes of partials per query, and the queries of one launch
    assert "const size_t per_query = (size_t)h->n_tiles * k * 12 + (size_t)h->n_tiles * 4;" in host
    m = re.search(r"const int64_t chunk = std::max<int64_t>\(1, std::min<int64_t>\(\{nq, \(int64_t\)\(\(size_t\)(\d+) << (\d+)\) / "
                  r"\(int64_t\)per_query, (\d+)\}\)\);", host)
    assert m, "the chunk formula of rdx_bm25_search changed: re-aim bm25_model.plan"
    assert (int(m.group(1)) << int(m.group(2)), int(m.group(3))) == (M.WORKSPACE, M.GRID_Y)
    assert M.chunk_of(M.CHUNK_ROWS, M.CHUNK_K, 10 ** 6) == (256 << 20) // (64 * (12 * 4096 + 4)) == 85
    assert M.plan(50, 1, M.GRID_NQ) == [(0, 65535), (65535, 6)]
    assert M.plan(1_000_000, 4096, 1) == [(0, 1)] and M.plan(5, 3, 0) == []


def passing(a, ids, allow=None):
    s = O.CpuBm25(a).scores(ids)
    return s, np.flatnonzero(s > 0)


def check_workspace_chunks(c):
    (run,) = c.runs
    chunk, nq = c.facts["chunk"], len(run.qs)
    assert M.n_tiles(c.a.n_rows) == 64 and run.k == M.MAX_K
    assert chunk == M.WORKSPACE // (64 * (12 * run.k + 4)) and nq == 2 * chunk + 3 > 2 * chunk
    assert M.plan(c.a.n_rows, run.k, nq) == [(0, chunk), (chunk, chunk), (2 * chunk, 3)]
    launch = lambda i: i // chunk
    assert sorted(launch(i) for i in c.facts["empty"]) == [1, 2] and all(len(run.qs[i]) == 0 for i in c.facts["empty"])
    assert sorted(launch(i) for i in c.facts["long"]) == [1, 2] and all(len(run.qs[i]) > M.TERM_CHUNK for i in c.facts["long"])
    assert sorted(launch(i) for i in c.facts["alone"]) == [0, 1, 2]
    t = c.truth(run)
    # a launch that read another launch's queries, or wrote into another launch's slots, shows: the queries at one position of
    # the three launches never have the same answer
    for i in range(chunk):
        same_pos = [M.result_of(t, j) for j in range(i, nq, chunk)]
        assert len(set(same_pos)) == len(same_pos), i
    assert t[2].max() == run.k and 0 < np.sort(t[2])[nq // 2] < run.k     # cut answers and short ones
    s, p = passing(c.a, run.qs[2 * chunk])
    assert (np.bincount(p // TILE, minlength=64) > 0).all() and len(p) > M.MERGE_CAP   # third launch: the merge cuts with tau


def check_grid_cap(c):
    (run,) = c.runs
    nq = len(run.qs)
    assert nq == M.GRID_Y + 6 and M.WORKSPACE // (1 * (12 * run.k + 4)) > nq      # the workspace is not what splits it
    assert M.plan(c.a.n_rows, run.k, nq) == [(0, M.GRID_Y), (M.GRID_Y, 6)]
    assert {len(q) for q in run.qs} == {0, 1, 2, 3}
    t = c.truth(run)
    assert all(M.result_of(t, M.GRID_Y + i) != M.result_of(t, i) for i in range(6))
    assert 0 < (t[2] == 0).sum() < nq


def check_merge_rounds(c):
    a = c.a
    assert M.n_tiles(a.n_rows) == M.MERGE_THREADS + 1 and a.n_rows - M.MERGE_THREADS * TILE == 1
    p0, p511, p512 = c.facts["plant"]
    assert (p0 // TILE, p511 // TILE, p512 // TILE) == (0, 511, 512)
    for run in c.runs:
        t = c.truth(run)
        for q in (0, 1):
            assert set(t[1][q, :3]) == {p0, p511, p512}, (run.name, q)        # the planted rows head both answers
    common, rare = c.runs[0].qs[:2]
    s, p = passing(a, common)
    per_tile = np.bincount(p // TILE, minlength=513)
    assert len(p) > 100 * M.MERGE_CAP and (per_tile[:512] > 2000).all() and per_tile[512] == 1    # many cuts, then the second round
    s, p = passing(a, rare)
    per_tile = np.bincount(p // TILE, minlength=513)
    assert 500 < len(p) < M.MAX_K and np.median(per_tile) <= 3 and (per_tile > 0).sum() > 300      # most tiles send 0 to 3


def check_idf_zero(c):
    a = c.a
    assert a.n_rows % 2 == 0 and a.post_off[1] - a.post_off[0] == a.n_rows // 2
    assert a.idf[0] == 0.0 and not np.signbit(a.idf[0]) and (a.idf[1:20] > 0).all()
    alone = c.truth(c.runs[0])
    assert (alone[2] == 0).all()                                                      # postings in the tile, nothing passes
    assert (c.truth(c.runs[1])[2] > 0).all()


def check_negative_floor(c):
    a = c.a
    assert (a.idf[:10] < 0).all() and (a.idf[10:] > 0).all() and len(set(a.idf[:10])) == 1     # the floor, of a negative average
    s, p = passing(a, c.runs[0].qs[0])
    assert len(p) > 50 and (s < 0).sum() > 50
    neg = c.truth(c.runs[1])
    assert (neg[2] == 0).all() and (neg[1] == -1).all() and (neg[0].view(np.int64) == 0).all()


def check_negative_tile(c):
    a = c.a
    assert M.n_tiles(a.n_rows) == 3 and (a.idf[:10] < 0).all()
    for q in c.runs[0].qs:
        s, p = passing(a, q)
        per_tile = np.bincount(p // TILE, minlength=3)
        assert per_tile[0] > 0 and per_tile[2] > 0 and per_tile[1] == 0
        assert (s[TILE:2 * TILE] <= 0).all() and (s[TILE:2 * TILE] < 0).sum() > TILE // 2   # tile 1: postings, nothing above zero


def check_cancellation(c):
    a = c.a
    both = a.post_row[a.post_off[0]:a.post_off[1]]
    for q in c.runs[0].qs:
        s = O.CpuBm25(a).scores(q)
        assert (s[both].view(np.int64) == 0).all()                                    # +0.0, bit for bit
    assert (c.truth(c.runs[0])[2] == 0).all()
    late = c.facts["late"]
    assert late.index(2) >= M.TERM_CHUNK and late.count(2) == 1
    t = c.truth(c.runs[1])
    first = O.CpuBm25(a).scores(late[:M.TERM_CHUNK])
    assert first[M.KEPT_ROW] == 0.0 and M.KEPT_ROW in t[1][0]                          # positive again only past position 256
    assert M.CANCEL_ROW not in t[1][0] and t[2][0] == 102                              # (the filler's 100 rows, 6000 and the kept one)
    neg = c.truth(c.runs[2])
    assert (neg[2] == 0).all() and (neg[1] == -1).all() and (neg[0].view(np.int64) == 0).all()
    assert a.post_tf.max() == 65535


def check_dense(c):
    n = c.a.n_rows
    q300 = c.runs[1].qs[0]
    assert len(q300) > M.TERM_CHUNK and q300[M.TERM_CHUNK - 1] == q300[M.TERM_CHUNK]
    for run in c.runs:
        t = c.truth(run)
        for i, q in enumerate(run.qs):
            s, p = passing(c.a, q)
            if n < TILE:
                assert t[2][i] == len(p) <= run.k                                    # every passing row's bits are compared
            else:
                assert t[2][i] == min(len(p), run.k)
        if n > TILE:
            assert passing(c.a, run.qs[0])[1].size == n > run.k                      # both tiles pass every row; one row is cut
    if n > TILE:
        assert len(c.runs[2].qs[0]) == M.MAX_TERMS


def check_tf_extremes(c):
    a = c.a
    tf3 = a.post_tf[a.post_off[3]:a.post_off[4]]
    assert tf3.max() == 65535 and tf3.min() == 1
    assert a.denom.max() / a.denom.min() > 300 and a.denom.min() < 0.4              # the denominators span orders of magnitude
    assert (a.idf[3:7] > 0).all()
    t = c.truth(c.runs[0])
    assert (t[2] > 40).all() and t[2].max() < c.runs[0].k                            # every passing row's bits are compared


def check_plateau(c):
    assert M.n_tiles(c.a.n_rows) == 5
    assert [r.k for r in c.runs] == [1, M.MAX_K - 1, M.MAX_K]
    for run in c.runs:
        t = c.truth(run)
        assert (t[1][0] == np.arange(run.k)).all() and len(set(t[0][0].tolist())) == 1


def check_plateau_mid_tile(c):
    assert 0 < M.PLATEAU_FROM < TILE
    top = c.facts["top"]
    want_top = list(top)
    for run in c.runs:
        t = c.truth(run)
        m = min(run.k, 3)
        assert t[1][0, :m].tolist() == want_top[:m]
        assert (t[1][0, 3:] == M.PLATEAU_FROM + np.arange(run.k - 3)[:max(run.k - 3, 0)]).all()
        assert (t[1][1] == M.PLATEAU_FROM + np.arange(run.k)).all()


def check_groups(c):
    g, words = c.a.n_groups, c.facts["words"]
    by = {r.name: r for r in c.runs}
    for r in c.runs:
        if r.allow is not None:
            assert len(r.allow) == words + 2 and (r.allow[words:] == 0xFFFFFFFF).all()       # longer than needed, garbage behind
    assert (c.truth(by["none"])[2] == 0).all()
    assert not M.differs(c.truth(by["all"]), c.truth(by["no filter"]))
    last = c.truth(by["last"])
    assert (last[2] > 0).all() and all((c.a.row_group[last[1][q, :last[2][q]]] == g - 1).all() for q in range(3))
    for only in (31, 32):
        if only < g:
            t = c.truth(by[f"only {only}"])
            assert (t[2] > 0).all() and all((c.a.row_group[t[1][q, :t[2][q]]] == only).all() for q in range(3))
    assert {"only 31": g > 31, "only 32": g > 32} == {"only 31": "only 31" in by, "only 32": "only 32" in by}


def check_one_row(c):
    assert c.a.n_rows == 1 and (c.a.idf < 0).all()
    assert all((c.truth(r)[2] == 0).all() for r in c.runs)


def check_one_row_positive(c):
    assert c.a.n_rows == 1
    t = c.truth(c.runs[0])
    assert t[2].tolist() == [1, 1, 0] and c.truth(c.runs[1])[2].tolist() == [1]


def check_no_terms(c):
    assert len(c.a.idf) == 0 and len(c.a.post_row) == 0 and all(len(q) == 0 for q in c.runs[0].qs)


def check_shapes(c):
    a = c.a
    post = lambda t: a.post_row[a.post_off[t]:a.post_off[t + 1]]
    nnz = len(a.post_row)
    assert post(1).tolist() == [TILE - 1, TILE]
    assert (post(2) == np.arange(TILE, 2 * TILE)).all()
    assert len(a.idf) == 8 and len(post(7)) == 0 and len(post(5)) == 0
    assert a.post_off[7] == a.post_off[8] == nnz and a.post_off[6] < nnz          # term 6's last directory entry ends at nnz
    assert post(6).tolist() == [7, 4000, 2 * TILE + 9]
    t = c.truth(c.runs[0])
    assert t[2].tolist()[:4] == [2, TILE, 3, 0] and t[2][5] == 0


CHECKS = {"workspace-chunks": check_workspace_chunks, "grid-cap": check_grid_cap, "merge-rounds": check_merge_rounds,
          "idf-zero": check_idf_zero, "negative-floor": check_negative_floor, "negative-tile": check_negative_tile,
          "cancellation": check_cancellation, "dense": check_dense, "tf-extremes": check_tf_extremes, "plateau": check_plateau,
          "plateau-mid-tile": check_plateau_mid_tile, "groups": check_groups, "one-row": check_one_row,
          "one-row-positive": check_one_row_positive, "no-terms": check_no_terms, "shapes": check_shapes}


def check_of(name):
    return CHECKS[name] if name in CHECKS else CHECKS[name.rsplit("-", 1)[0]]


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_case_reaches_its_branch(name):
    check_of(name)(M.case(name))


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_case_agrees_with_rank_bm25(name):
    c = M.case(name)
    if c.docs is None:
        assert c.exempt, name
        return
    assert not c.exempt and len(c.docs) == c.a.n_rows <= 5000
    dense, sparse = O.BM25Okapi(c.docs), O.CpuBm25(c.a)
    seen = set()
    for run in c.runs:
        for q in run.qs:
            key = tuple(int(t) for t in q)
            if key in seen:
                continue
            seen.add(key)
            np.testing.assert_array_equal(sparse.scores(q).view(np.int64), dense.get_scores(list(key)).view(np.int64),
                                          err_msg=f"{name} {run.name} {key[:12]}")


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_named_mutants_differ(name):
    c = M.case(name)
    for run in c.runs:
        t = c.truth(run)
        for m in run.mutants:
            assert M.differs(t, M.mutant_search(c.a, run.qs, run.k, run.allow, m)), (name, run.name, m)


def test_every_mutant_is_named_somewhere():
    named = {m for name in M.CASES for run in M.case(name).runs for m in run.mutants}
    assert named == set(range(1, 11))


def test_unmutated_model_is_the_truth():
    """mutant_search with no mutant selected restates CpuBm25.search: the mutants differ by their one change alone"""
    for name in ("dense-4095", "groups-33", "cancellation"):
        c = M.case(name)
        for run in c.runs:
            if sum(len(q) for q in run.qs) < 1000:
                assert not M.differs(c.truth(run), M.mutant_search(c.a, run.qs, run.k, run.allow, 0))
