"""GPU: the exact dense score of named (query, row) pairs (rag_dpo_amd.engine.score_pairs -> rdx_index_score_pairs -> k_score_pairs,
DESIGN.md §31) on bits against rdx_search(k = rows)'s score of the same (query, row) and against the oracle's.

dims: one float4 group (4), two (8), the edges of one and of four groups per lane (252, 256, 260, 1024). A 70-row index (more than
one wave's worth of rows, no multiple of anything). n_pairs around a workgroup of four waves (1, 3, 4, 5), around 64 (64, 65) and
many workgroups (1000); every list holds repeated pairs, row 0 and the last row. The queries are raw (not normalised): one is scaled
by 1e3, one by 1e-3."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS, NQ = 70, 5
DIMS = [4, 8, 252, 256, 260, 1024]
N_PAIRS = [1, 3, 4, 5, 64, 65, 1000]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def world(dim):
    rng = np.random.default_rng(100 + dim)
    x = rng.standard_normal((ROWS, dim)).astype(np.float32)
    q = rng.standard_normal((NQ, dim)).astype(np.float32)
    q[1] *= 1e3
    q[2] *= 1e-3
    q[3] = x[ROWS - 1] * 0.5           # the last row's own direction
    return x, q


def pair_list(n, seed):
    rng = np.random.default_rng(seed)
    pq = rng.integers(0, NQ, n).astype(np.int32)
    pr = rng.integers(0, ROWS, n).astype(np.int64)
    pr[0] = 0
    pr[-1] = ROWS - 1
    if n >= 4:
        pq[1], pr[1] = pq[0], pr[0]    # a repeated pair
        pr[2] = ROWS - 1
    return pq, pr


def call(E, ix, q, pq, pr):
    dev = torch.device("cuda", ix.device)
    return E.score_pairs(ix, torch.from_numpy(q).to(dev), torch.from_numpy(pq).to(dev), torch.from_numpy(pr).to(dev)).cpu().numpy()


def search_table(ix, q):
    """[nq][rows] fp32: rdx_search(k = rows)'s score of every (query, row)"""
    sc, ro, cn = ix.search(q, ROWS)
    assert cn.tolist() == [ROWS] * len(q)
    table = np.empty((len(q), ROWS), dtype=np.float32)
    for b in range(len(q)):
        table[b, ro[b]] = sc[b]
    return table


@pytest.fixture(scope="module")
def worlds(oracle):
    from rag_dpo_amd import engine as E
    made = {}

    def get(dim):
        if dim not in made:
            x, q = world(dim)
            ix = E.HipIndex(dim)
            ix.add(x)
            hat, qhat = oracle.normalize_rows(x), oracle.normalize_rows(q)
            want = np.stack([oracle.scores(hat, qhat[b]) for b in range(NQ)])
            table = search_table(ix, q)
            assert np.array_equal(bits(table), bits(want))       # the reference, computed once: the search IS the oracle here
            made[dim] = (ix, q, table)
        return made[dim]

    yield get
    for ix, _, _ in made.values():
        ix.close()


@pytest.mark.parametrize("dim", DIMS)
def test_pairs_have_the_bits_of_the_search_and_of_the_oracle(worlds, dim):
    from rag_dpo_amd import engine as E
    ix, q, table = worlds(dim)
    for n in N_PAIRS:
        pq, pr = pair_list(n, 7 * n + dim)
        got = call(E, ix, q, pq, pr)
        assert got.shape == (n,) and np.array_equal(bits(got), bits(table[pq, pr])), (dim, n)
    # every (query, row) once
    pq, pr = np.repeat(np.arange(NQ, dtype=np.int32), ROWS), np.tile(np.arange(ROWS, dtype=np.int64), NQ)
    assert np.array_equal(bits(call(E, ix, q, pq, pr)), bits(table.reshape(-1)))


@pytest.mark.parametrize("dim", [8, 260, 1024])
def test_out_of_range_pairs_get_nan_and_leave_their_neighbours(worlds, dim):
    from rag_dpo_amd import engine as E
    ix, q, table = worlds(dim)
    pq, pr = pair_list(65, dim)
    bad = {3: (-1, 5), 4: (NQ, 5), 10: (0, -1), 11: (0, ROWS), 63: (2, 2 ** 40), 64: (-2 ** 31, ROWS - 1)}
    for p, (a, b) in bad.items():
        pq[p], pr[p] = a, b
    got = call(E, ix, q, pq, pr)
    ok = np.array([p not in bad for p in range(65)])
    assert np.isnan(got[~ok]).all()
    assert np.array_equal(bits(got[ok]), bits(table[pq[ok], pr[ok]]))
    # a query holding NaN or Inf, which a search refuses as a whole: NaN for its pairs alone
    q2 = q.copy()
    q2[4, dim // 2] = np.inf
    got = call(E, ix, q2, *pair_list(64, dim + 1))
    pq, pr = pair_list(64, dim + 1)
    assert np.isnan(got[pq == 4]).all() and (pq == 4).any()
    assert np.array_equal(bits(got[pq != 4]), bits(table[pq[pq != 4], pr[pq != 4]]))


def test_two_calls_and_a_second_stream_give_the_same_bits(worlds):
    from rag_dpo_amd import engine as E
    ix, q, table = worlds(260)
    pq, pr = pair_list(1000, 3)
    first = call(E, ix, q, pq, pr)
    assert np.array_equal(bits(call(E, ix, q, pq, pr)), bits(first))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = call(E, ix, q, pq, pr)
    side.synchronize()
    assert np.array_equal(bits(other), bits(first))
    # a pair's bits do not depend on its position or on n_pairs
    assert np.array_equal(bits(call(E, ix, q, pq[::-1].copy(), pr[::-1].copy())), bits(first[::-1]))
    assert np.array_equal(bits(call(E, ix, q, pq[500:501], pr[500:501])), bits(first[500:501]))


@pytest.mark.parametrize("dim", [8, 256, 260])
def test_a_compact_master_twin_and_an_update(oracle, dim):
    from rag_dpo_amd import engine as E
    x, q = world(dim)
    u = torch.from_numpy(x).to(torch.bfloat16)                     # the same bf16 rows for both forms
    wide = u.to(torch.float32).numpy()
    ix, ref = E.HipIndex(dim), E.HipIndex(dim)
    try:
        ix.set_option("compact_master", 1)
        ix.add_bf16(u)
        ref.add_bf16(u)
        hat = oracle.normalize_rows(wide)
        qhat = oracle.normalize_rows(q)
        want = np.stack([oracle.scores(hat, qhat[b]) for b in range(NQ)])
        pq, pr = pair_list(65, dim)
        a, b = call(E, ix, q, pq, pr), call(E, ref, q, pq, pr)
        assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(want[pq, pr]))
        # after update of one row its score is the new row's; the others keep theirs
        new = (3.0 * np.random.default_rng(dim).standard_normal((1, dim))).astype(np.float32)
        ref.update([ROWS - 1], new)
        hat[ROWS - 1] = oracle.normalize_rows(new)[0]
        want = np.stack([oracle.scores(hat, qhat[b]) for b in range(NQ)])
        got = call(E, ref, q, pq, pr)
        assert np.array_equal(bits(got), bits(want[pq, pr])) and (pr == ROWS - 1).sum() >= 2
        assert not np.array_equal(bits(got), bits(b))
    finally:
        ix.close()
        ref.close()


def test_limits_and_refusals(worlds):
    from rag_dpo_amd import _lib as L
    from rag_dpo_amd import engine as E
    ix, q, _ = worlds(8)
    dev = torch.device("cuda", ix.device)
    qd = torch.from_numpy(q).to(dev)
    pq = torch.zeros(4, dtype=torch.int32, device=dev)
    pr = torch.zeros(4, dtype=torch.int64, device=dev)
    out = torch.full((4,), 7.0, dtype=torch.float32, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    f = ix._lib.rdx_index_score_pairs
    for nq, n in ((NQ, 0), (NQ, -1), (NQ, (1 << 20) + 1), (0, 4), (65536, 4)):
        assert f(ix._h, p(qd), nq, p(pq), p(pr), n, p(out), None) == L.RDX_ERR_INVALID, (nq, n)
    assert f(None, p(qd), NQ, p(pq), p(pr), 4, p(out), None) == L.RDX_ERR_INVALID
    assert f(ix._h, None, NQ, p(pq), p(pr), 4, p(out), None) == L.RDX_ERR_INVALID
    assert f(ix._h, ctypes.c_void_p(qd.data_ptr() + 4), NQ, p(pq), p(pr), 4, p(out), None) == L.RDX_ERR_INVALID   # 16-byte alignment
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [7.0] * 4                         # nothing was launched
    with pytest.raises(ValueError):
        E.score_pairs(ix, qd[:, :4].contiguous(), pq, pr)          # another dim
    with pytest.raises(ValueError):
        E.score_pairs(ix, qd, pq, pr[:3])
    # a shard (mapped row ids) is refused, as rdx_index_mmr refuses it
    sh = E.HipIndex(8)
    try:
        sh.add(world(8)[0])
        sh.set_row_ids(0, np.arange(ROWS, dtype=np.int64) * 2)
        assert sh._lib.rdx_index_score_pairs(sh._h, p(qd), NQ, p(pq), p(pr), 4, p(out), None) == L.RDX_ERR_STATE
    finally:
        sh.close()
