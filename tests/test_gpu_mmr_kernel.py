"""GPU: the diversity-aware selection kernel called directly (rag_dpo_amd.engine.mmr_select -> rdx_index_mmr -> k_mmr) on hand-made
candidate lists over a small index, all five outputs byte for byte against the definition as a literal double loop over the oracle's
exact scores (tests/mmr_model.py).

dims: one float4 group (4), the edges of one and of four groups per lane (252, 256, 260, 1024) and the long-row path (1028). List
lengths around a wave (63, 64, 65), around the widest list of the engine's scan path (256, 257), the smallest (1, 2) and the largest
(1024: every lane of every wave owns a position). Every case runs a batch of 130 lists (a handful of distinct ones, repeated: the same list gives the same bits wherever it
stands), three lists with k = 1 and one list alone."""
import json

import numpy as np
import pytest

import mmr_model as LM

pytestmark = pytest.mark.gpu

N_ROWS = 1500
TWIN, COPIES, ZEROS = 7, list(range(100, 111)), [20, 21]      # rows 100..110 are exact copies of row 7; rows 20 and 21 are zero
LAMBDAS = [0.0, 0.3, 0.5, 1.0]
DIMS = [4, 252, 256, 260, 1024, 1028]
FETCH = [1, 2, 63, 64, 65, 256, 257, 1024]


def world(dim):
    rng = np.random.default_rng(dim)
    common = rng.standard_normal(dim).astype(np.float32)
    x = (0.7 * common[None, :] + rng.standard_normal((N_ROWS, dim))).astype(np.float32)
    x[200:400] = x[200:400:20].repeat(20, axis=0) + 0.05 * rng.standard_normal((200, dim)).astype(np.float32)   # ten tight clusters
    x[COPIES] = x[TWIN]
    x[ZEROS] = 0.0
    q = (0.7 * common[None, :] + rng.standard_normal((3, dim))).astype(np.float32)
    q[1] = x[TWIN] + 0.1 * rng.standard_normal(dim).astype(np.float32)          # the copies are this query's best rows
    q[2] = x[205] + 0.1 * rng.standard_normal(dim).astype(np.float32)           # a cluster is this one's
    return x, q


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
            made[dim] = (ix, hat, [oracle.scores(hat, qhat[b]) for b in range(3)])
        return made[dim]

    yield get
    for ix, _, _ in made.values():
        ix.close()


def ranked(rows, sc):
    rows = np.asarray(sorted(rows, key=lambda r: (-float(sc[r]), r)), dtype=np.int64)
    return sc[rows], rows


def make_lists(F, K, scores, rng):
    """-> [(score f32 [F], row i64 [F], count)]: a handful of distinct lists of width F for picks of K"""
    special = [TWIN] + COPIES[:3] + ZEROS if F >= 16 else []
    lists = []

    def put(s, r, count):
        ps = np.full(F, -np.inf, dtype=np.float32)
        pr = np.full(F, N_ROWS + 5, dtype=np.int64)              # past a list's count: a row the index does not hold, never looked at
        ps[: len(s)], pr[: len(r)] = s, r
        lists.append((ps, pr, count))

    def pick_rows(b):
        rest = np.setdiff1d(np.arange(N_ROWS), special)
        top = rest[np.argsort(-scores[b][rest], kind="stable")][: 4 * F]    # drawn among the query's better rows: clusters meet again
        return np.concatenate([np.asarray(special, dtype=np.int64), rng.choice(top, F - len(special), replace=False)])

    s, r = ranked(pick_rows(1), scores[1])                       # 0: a search's list (sorted), the copies of row 7 tie at its top
    put(s, r, F)
    r = rng.permutation(pick_rows(2))                            # 1: not sorted, and a count beyond the width (clamped)
    put(scores[2][r], r, F + 7)
    put(*ranked(pick_rows(0), scores[0]), 0)                     # 2: an empty list
    s, r = ranked(pick_rows(0), scores[0])                       # 3: fewer entries than picks
    put(s[: K - 1], r[: K - 1], K - 1)
    s, r = ranked(pick_rows(2), scores[2])                       # 4: padding rows of -1 inside the list, the first entry among them
    hole = rng.random(F) < 0.25
    hole[0] = F > 1
    s, r = s.copy(), r.copy()
    s[hole], r[hole] = -np.inf, -1
    put(s, r, F)
    same = np.asarray(([TWIN] + COPIES)[:F], dtype=np.int64)     # 5: identical rows only
    put(scores[1][same], same, len(same))
    return lists


def run(ix, lists, order, k, lam):
    import torch
    from rag_dpo_amd import engine as E
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    s = np.stack([lists[i][0] for i in order])
    r = np.stack([lists[i][1] for i in order])
    c = np.asarray([lists[i][2] for i in order], dtype=np.int32)
    out = E.mmr_select(ix, t(s), t(r), t(c), k, lam)
    return {name: v.cpu().numpy() for name, v in out.items()}


def check(out, order, want, k):
    """every query of a call against the model of its list (picked with K >= k: a greedy selection's first k picks are its k picks)"""
    assert out["pos"].dtype == np.int32 and out["row"].dtype == np.int64 and out["score"].dtype == np.float32 and out["value"].dtype == np.float64
    assert out["pos"].shape == (len(order), k) and out["count"].shape == (len(order),)
    for b, i in enumerate(order):
        pos, row, sc, va, n = LM.as_arrays(want[i][:k], k)
        assert out["count"][b] == n, (b, i)
        assert out["pos"][b].tobytes() == pos.tobytes(), (b, i, out["pos"][b].tolist(), pos.tolist())
        assert out["row"][b].tobytes() == row.tobytes(), (b, i)
        assert out["score"][b].tobytes() == sc.tobytes(), (b, i)
        assert out["value"][b].tobytes() == va.tobytes(), (b, i, out["value"][b].tolist(), va.tolist())


@pytest.mark.parametrize("F", FETCH)
@pytest.mark.parametrize("dim", DIMS)
def test_select_matches_the_definition(dim, F, worlds):
    ix, hat, scores = worlds(dim)
    rng = np.random.default_rng(1000 * dim + F)
    K = min(F, 64)                                               # k = F up to 64 entries, k = 64 beyond
    lists = make_lists(F, K, scores, rng)
    # every lambda on the short lists; the long ones (a second of model per list and lambda) take two, by turns over the cases
    turn = DIMS.index(dim) + FETCH.index(F)
    lams = LAMBDAS if F <= 65 else [LAMBDAS[turn % 4], LAMBDAS[(turn + 2) % 4]]
    for lam in lams:
        want = [LM.literal_mmr(s[: min(c, F)], r[: min(c, F)], hat, K, lam) for s, r, c in lists]
        if F >= 16 and lam < 1.0:
            # list 0 holds row 7 and three exact copies of it, side by side: they tie in v, so they are picked in the order of their
            # positions; and once one of them is picked the others, now next to a picked copy of themselves (m = p of identical
            # rows), fall behind a zero row (v = 0) that is still to be had
            twins = [t for t, (_, row, _, _) in enumerate(want[0]) if row in [TWIN] + COPIES]
            assert [want[0][t][0] for t in twins] == sorted(want[0][t][0] for t in twins)
            if twins and twins[0] + 1 < len(want[0]) and not any(row in ZEROS for _, row, _, _ in want[0][: twins[0] + 1]):
                assert twins[0] + 1 not in twins
        big = [b % len(lists) for b in range(130)]
        out130 = run(ix, lists, big, K, lam)
        assert out130["bad"].tolist() == [0]
        check(out130, big, want, K)
        out3 = run(ix, lists, [0, 1, 4], 1, lam)
        check(out3, [0, 1, 4], want, 1)
        for i in (0, 1):
            out1 = run(ix, lists, [i], K, lam)
            check(out1, [i], want, K)
            for name in ("pos", "row", "score", "value", "count"):      # alone and inside the batch of 130: the same bits
                assert out1[name][0].tobytes() == out130[name][i].tobytes() == out130[name][i + 126].tobytes(), (name, i)
    if F < 64:
        with pytest.raises(ValueError):
            run(ix, lists, [0], 64, 0.5)                         # k beyond the list's width


def test_a_row_the_index_does_not_hold_is_skipped_and_reported(worlds):
    dim, F, K = 256, 64, 10
    ix, hat, scores = worlds(dim)
    lists = make_lists(F, K, scores, np.random.default_rng(5))
    clean = run(ix, lists, [0, 1, 4], K, 0.5)
    assert clean["bad"].tolist() == [0]
    for wild in (N_ROWS, 1 << 40):
        s, r, c = lists[0]
        r = r.copy()
        r[1], r[9] = wild, wild
        dirty = [(s, r, c), lists[1], lists[4]]
        out = run(ix, dirty, [0, 1, 2], K, 0.5)
        assert out["bad"].tolist() == [1]
        want = [LM.literal_mmr(ls[: min(lc, F)], lr[: min(lc, F)], hat, K, 0.5, n_rows=N_ROWS) for ls, lr, lc in dirty]
        check(out, [0, 1, 2], want, K)                           # the entries were skipped as padding is ...
        assert 1 not in out["pos"][0] and 9 not in out["pos"][0]
        for name in ("pos", "row", "score", "value", "count"):   # ... and the other queries' answers are what they were
            assert out[name][1:].tobytes() == clean[name][1:].tobytes(), name


@pytest.mark.parametrize("dim", [260, 1028])
def test_compact_master_gives_its_fp32_twin_s_bits(dim, oracle):
    import torch
    from rag_dpo_amd import engine as E
    x, q = world(dim)
    xb = torch.from_numpy(x).to(torch.bfloat16)
    wide = xb.to(torch.float32).numpy()
    hat = oracle.normalize_rows(wide)
    scores = [oracle.scores(hat, qh) for qh in oracle.normalize_rows(q)]
    ix, ref = E.HipIndex(dim), E.HipIndex(dim)
    ix.set_option("compact_master", 1)
    ix.add_bf16(xb)
    ref.add_bf16(xb)
    F, K = 65, 64
    lists = make_lists(F, K, scores, np.random.default_rng(dim))
    order = [0, 1, 3, 4, 5]
    a, b = run(ix, lists, order, K, 0.3), run(ref, lists, order, K, 0.3)
    for name in a:
        assert a[name].tobytes() == b[name].tobytes(), name
    check(a, order, [LM.literal_mmr(s[: min(c, F)], r[: min(c, F)], hat, K, 0.3) for s, r, c in lists], K)
    ix.close()
    ref.close()


def test_limits_and_refusals(worlds):
    import torch
    from rag_dpo_amd import engine as E
    from rag_dpo_amd._lib import RdxError
    ix, hat, scores = worlds(256)
    lists = make_lists(64, 10, scores, np.random.default_rng(6))
    for k, lam in ((0, 0.5), (65, 0.5), (10, -0.01), (10, 1.01), (10, float("nan"))):
        with pytest.raises(ValueError):
            run(ix, lists, [0], k, lam)
    dev = torch.device("cuda", 0)
    wide = (torch.zeros((1, 1025), dtype=torch.float32, device=dev), torch.zeros((1, 1025), dtype=torch.int64, device=dev),
            torch.zeros(1, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        E.mmr_select(ix, *wide, 10, 0.5)                          # fetch_k beyond RDX_MMR_MAX_FETCH
    with pytest.raises(ValueError):
        E.mmr_select(ix, wide[0][:, :64].contiguous(), wide[1][:, :64].contiguous().to(torch.int32), wide[2], 10, 0.5)   # rows must be int64
    none = E.mmr_select(ix, wide[0][:0, :64].contiguous(), wide[1][:0, :64].contiguous(), wide[2][:0], 10, 0.5)        # no queries: nothing to do
    assert none["pos"].shape == (0, 10)
    shard = E.HipIndex(8)
    shard.add(np.eye(4, 8, dtype=np.float32))
    shard.set_row_ids(0, [10, 20, 30, 40])
    with pytest.raises(RdxError):                                 # mapped row ids: the lists would not name the index's own rows
        E.mmr_select(shard, wide[0][:, :4].contiguous(), wide[1][:, :4].contiguous(), wide[2], 2, 0.5)
    shard.close()


def test_the_kernel_keeps_its_registers():
    from rag_dpo_amd import build
    build.build_lib()
    res = json.load(open(build.RESOURCES))
    mine = {k: v for k, v in res.items() if "k_mmr" in k}
    assert len(mine) == 5, sorted(mine)                           # U = 0 .. 4
    for k, v in mine.items():
        assert v["spill_vgprs"] == 0 and v["scratch_bytes"] == 0, (k, v)
