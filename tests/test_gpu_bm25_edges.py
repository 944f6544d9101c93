"""GPU: the BM25 kernels (csrc/bm25_kernel.hpp, rdx_bm25_search of csrc/rdx_bm25.hip) replay the named cases of tests/bm25_model.py
through rag_dpo_amd.bm25.HipBm25 and return the truth's rows, counts and float64 score BITS — no tolerance anywhere. The truth is
bm25_oracle.CpuBm25 with bm25_oracle.topk; tests/test_bm25_model.py shows, without a GPU, that every case reaches the branch it
names (a second and third launch of the query-chunk loop, the merge's second round of tiles, idf <= 0, a tile with postings and no
passing row, ...) and that the wrong kernels it lists would be told from the truth by exactly these comparisons.

Beyond tests/test_gpu_bm25.py's same(): the slots past `count` hold row -1 AND score +0.0 bitwise, as the merge kernel promises."""
import threading

import numpy as np
import pytest

import bm25_model as M
from rag_dpo_amd import bm25

pytestmark = pytest.mark.gpu


def equal_bits(x, y):
    return all((a.view(np.uint8) == b.view(np.uint8)).all() for a, b in zip(x, y))


def same(gpu, case, run):
    """the whole answer, slot by slot: counts, rows (-1 past the count), score bits (+0.0 past the count)"""
    want = case.truth(run)
    got = gpu.search(*M.offsets(run.qs), run.k, run.allow)
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape
    bad = np.flatnonzero(got[2] != want[2])
    assert bad.size == 0, (run.name, "counts", bad[:8], got[2][bad[:8]], want[2][bad[:8]])
    bad = np.flatnonzero((got[1] != want[1]).any(axis=1))
    assert bad.size == 0, (run.name, "rows", bad[:8])
    bad = np.flatnonzero((got[0].view(np.int64) != want[0].view(np.int64)).any(axis=1))
    assert bad.size == 0, (run.name, "score bits", bad[:8])
    past = np.arange(run.k)[None, :] >= want[2][:, None]
    assert (got[1][past] == -1).all() and (got[0].view(np.int64)[past] == 0).all()
    return got


@pytest.mark.parametrize("name", sorted(n for n in M.CASES if n != "workspace-chunks"))
def test_case(name):
    case = M.case(name)
    gpu = bm25.HipBm25(case.a, 0)
    try:
        for run in case.runs:
            same(gpu, case, run)
    finally:
        gpu.close()


def test_workspace_chunks():
    """three launches in one search; a query of each launch searched alone equals its row of the batch"""
    case = M.case("workspace-chunks")
    (run,) = case.runs
    assert len(M.plan(case.a.n_rows, run.k, len(run.qs))) == 3
    gpu = bm25.HipBm25(case.a, 0)
    try:
        batch = same(gpu, case, run)
        for i in case.facts["alone"]:
            one = gpu.search(*M.offsets([run.qs[i]]), run.k)
            assert equal_bits(one, [x[i:i + 1] for x in batch]), i
    finally:
        gpu.close()


@pytest.fixture(scope="module")
def dense():
    case = M.case("dense-4097")
    gpu = bm25.HipBm25(case.a, 0)
    yield case, gpu
    gpu.close()


def test_no_queries_is_a_success(dense):
    case, gpu = dense
    sc, ro, cn = gpu.search(np.zeros(1, np.int64), np.zeros(0, np.int32), 5)
    assert sc.shape == (0, 5) and ro.shape == (0, 5) and cn.shape == (0,)
    same(gpu, case, case.runs[0])                      # and the index still answers


def test_side_stream_gives_the_same_bits(dense):
    import torch
    case, gpu = dense
    run = case.runs[0]
    here = same(gpu, case, run)
    side = torch.cuda.Stream(device=0)
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream(0) == side
        there = gpu.search(*M.offsets(run.qs), run.k)
    assert equal_bits(here, there)


def test_two_threads_on_one_index(dense):
    case, gpu = dense
    runs = case.runs[:2]
    want = [same(gpu, case, r) for r in runs]
    wrong, errors = [], []

    def work(i):
        try:
            for _ in range(10):
                got = gpu.search(*M.offsets(runs[i].qs), runs[i].k)
                if not equal_bits(got, want[i]):
                    wrong.append(i)
        except Exception as e:                         # a thread's exception would otherwise be lost
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors and not wrong, (errors, wrong)
