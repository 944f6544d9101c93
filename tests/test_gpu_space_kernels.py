"""GPU: the kernels of the "ip" / "l2" spaces (csrc/space_kernel.hpp) called DIRECTLY — engine.space_measure, space_lift,
space_rescore, space_distances on synthetic tensors, no HipIndex and no SpaceEngine — against tests/space_model.py. Everything is
compared bit for bit; there is no tolerance in this file. tests/test_space_kernel_model.py (CPU) pins the references used here and
asserts the conditions that give these tests their teeth.

  a. every dimension edge of space_sum (fewer elements than partial sums, a float4 group short of / past a 64-lane row and the
     256-element chunk, the engine's MAX_DIM), both modes, all four users of the sum. ip inputs are cancelling_pairs, whose fp32
     distance changes with the fp64 summation order; l2 has no such input (its terms are non-negative): there the ragged dims
     catch dropped, doubled or misplaced terms, not the order.
  b. k_space_select: counts 0 .. kp in one call, k = 1 / middle / kp, kp across the 64-lane and 256-thread steps up to 4096, ties
     by int64 row id (also ids that differ in the high word only), distances that overflow to +inf, NaN in every slot the
     kernels must not read.
  c. the proof flag at its boundary: the largest fp32 score that proves, the next float and the one after -> 1, 0, 0; both sides of
     U = 0; other guards; query norms outside the guard's range; fewer candidates than slots.
  d. k_space_page's addressing: allow bits by first_row + r across 32-bit word edges, column offset and stride, nothing written
     outside the page.
  e. the same inputs give the same bits, on any stream."""
import numpy as np
import pytest

from rag_dpo_amd import spaces as S

import space_model as M

pytestmark = pytest.mark.gpu
SPACES = ("ip", "l2")
DIMS = (4, 60, 64, 68, 252, 256, 260, 508, 516, 1020, 1024, 1028, 4092, 4096)
DIM_CASES = [(s, d) for s in SPACES for d in DIMS if S.lifted_dim(s, d) <= 4096]
SENTINEL = 0x7FC12345       # a NaN no kernel produces: what must stay in the columns outside a page


def _dev():
    import torch
    return torch.device("cuda", 0)


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _nan_like(shape, rng):
    """fp32 NaNs of both signs with random payloads"""
    b = rng.integers(1, 1 << 22, size=shape, dtype=np.uint32) | np.uint32(0x7FC00000) | (rng.integers(0, 2, size=shape, dtype=np.uint32) << np.uint32(31))
    return b.view(np.float32)


def _lift(space, x, e):
    """engine rows by spaces.lift_rows; the kernels under test read the raw columns only, which must scale back exactly (the
    lifted coordinate of the 3e19 rows overflows: it is never read)"""
    with np.errstate(all="ignore"):
        y, _ = S.lift_rows(space, x, e)
    back = np.ldexp(y[..., : x.shape[-1]], np.int32(-e))
    assert (back.view(np.uint32) == np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)).all()    # the scaling is exact
    return y


def _engine_cands(space, x, counts, e, rng):
    """raw candidates x [nq][kp][dim] -> engine rows [nq * kp][engine dim] with NaN in every slot at or past the count"""
    nq, kp, dim = x.shape
    y = _lift(space, x.reshape(nq * kp, dim), e).reshape(nq, kp, -1).copy()
    for b in range(nq):
        y[b, counts[b]:] = _nan_like(y[b, counts[b]:].shape, rng)
    return y.reshape(nq * kp, -1)


def _rescore(space, q, y, rows, scores, counts, k, e, guard):
    from rag_dpo_amd import engine as E
    out = E.space_rescore(S.KIND[space], _t(q), _t(y), _t(rows), _t(scores), _t(np.asarray(counts, dtype=np.int32)), k, e, guard)
    return tuple(_np(o) for o in out)


def _assert_rescore(got, want, what):
    (gd, gr, gc, gp), (wd, wr, wc, wp) = got, want
    assert (gc == wc).all(), f"{what}: counts differ"
    assert (gr == wr).all(), f"{what}: rows differ at {np.argwhere(gr != wr)[:5].tolist()}"
    assert (_bits(gd) == _bits(wd)).all(), f"{what}: distance bits differ at {np.argwhere(_bits(gd) != _bits(wd))[:5].tolist()}"
    assert (gp == wp).all(), f"{what}: proof flags differ at {np.flatnonzero(gp != wp)[:10].tolist()}: {gp[gp != wp][:10].tolist()}"


# ---- a. every dimension edge ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("space,dim", DIM_CASES, ids=[f"{s}-d{d}" for s, d in DIM_CASES])
def test_measure_and_lift_at_every_dim_edge(space, dim):
    from rag_dpo_amd import engine as E
    x = M.wide_rows(41, dim, seed=3)                      # 41 rows: the last block has one live wave
    xt = _t(x)
    sq, bad = S.measure(space, x)
    sq_t, bad_t = E.space_measure(S.KIND[space], xt)
    assert not bad.any() and (_np(bad_t) == 0).all()
    assert (_np(sq_t).view(np.uint64) == sq.view(np.uint64)).all()
    e0 = S.scale_exp_for(float(sq.max()))
    for e in (e0, e0 - 9):
        y, lost = S.lift_rows(space, x, e)
        y_t, lost_t = E.space_lift(S.KIND[space], xt, e)
        assert not lost.any() and (_np(lost_t) == 0).all()
        assert (_np(y_t).view(np.uint32) == y.view(np.uint32)).all()
    p_t, lost_t = E.space_lift(S.KIND[space], xt, 0, is_query=True)
    assert (_np(p_t).view(np.uint32) == S.lift_queries(space, x).view(np.uint32)).all() and (_np(lost_t) == 0).all()


def _pairs_for(space, dim):
    if space == "ip":
        q, x = M.cancelling_pairs(37, dim, seed=dim)
        return q[:3].copy(), x
    return M.spread_rows(3, dim, seed=dim + 1), M.spread_rows(37, dim, seed=dim)


@pytest.mark.parametrize("space,dim", DIM_CASES, ids=[f"{s}-d{d}" for s, d in DIM_CASES])
def test_distances_and_rescore_at_every_dim_edge(space, dim):
    import torch
    from rag_dpo_amd import engine as E
    q, x = _pairs_for(space, dim)                          # 3 x 37 = 111 pairs: the last block has three live waves
    want = M.model_page(space, q, x, None, 0)
    assert np.isfinite(want).all()
    rng = np.random.default_rng(dim)
    nq, kp, k = 3, 37, 10
    rows = np.stack([rng.permutation(1 << 20)[:kp] for _ in range(nq)]).astype(np.int64)
    counts = np.asarray([kp, kp - 1, 5], dtype=np.int32)
    scores = _nan_like((nq, kp), rng)
    scores[:, kp - 1] = 0.0
    rows_in = rows.copy()
    for b in range(nq):
        rows_in[b, counts[b]:] = -1
        scores[b, counts[b]:] = np.nan
    xs = np.broadcast_to(x, (nq, kp, dim))
    for e in (0, 7):
        out = torch.full((nq, kp), SENTINEL, dtype=torch.int32, device=_dev()).view(torch.float32)
        E.space_distances(S.KIND[space], _t(q), _t(_lift(space, x, e)), e, None, 0, out, 0)
        got = _np(out)
        assert (_bits(got) == _bits(want)).all(), f"{space} d={dim} e={e}: {int((_bits(got) != _bits(want)).sum())} of 111 distances differ"
        ref = M.model_rescore(space, q, xs, rows, scores, counts, k, e, S.GUARD[space])
        y = _engine_cands(space, np.ascontiguousarray(xs), counts, e, rng)
        _assert_rescore(_rescore(space, q, y, rows_in, scores, counts, k, e, S.GUARD[space]), ref, f"{space} d={dim} e={e}")


# ---- b. selection edges ---------------------------------------------------------------------------------------------------------
def _selection_world(space, kp):
    """7 queries x kp candidates at dim 64 (7 kp is not a multiple of the block's 4 waves whenever kp is odd; no nq can do that for
    kp = 64, 1000, 4096). Duplicated vectors make tie groups whose row ids come in descending order, shuffled, and differing in the
    high 32 bits only; the last l2 query is full of 3e19: candidates equal to it (distance 0), a few ulps off (finite) and
    ordinary ones, whose distances overflow to +inf and rank by row, before the padding."""
    rng = np.random.default_rng([S.KIND[space], kp])
    dim, nq = 64, 7
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    x = (0.05 * rng.standard_normal((nq, kp, dim))).astype(np.float32)
    rows = np.stack([rng.permutation(1 << 20)[:kp] + 7 for _ in range(nq)]).astype(np.int64)
    if space == "l2":
        q[6] = 3e19
        third = kp // 3
        x[6, :third] = q[6]
        for j in range(third, 2 * third):
            x[6, j] = q[6]
            c = rng.integers(0, dim, size=2)
            x[6, j, c] = M.f32_of_key(M.f32_key(x[6, j, c]) + rng.integers(-3, 4, size=2))
        perm = rng.permutation(kp)
        x[6] = x[6, perm]
    if kp >= 63:
        for b in range(nq):
            pos = rng.permutation(kp)[:12]
            a, s, h = pos[:5], pos[5:9], pos[9:]
            x[b, a], x[b, s], x[b, h] = x[b, a[0]], x[b, s[0]], x[b, h[0]]
            rows[b, np.sort(a)] = np.sort(rows[b, a])[::-1]                      # descending in slot order
            rows[b, h] = (rows[b, h[0]] & 0xFFFFFFFF) | (np.asarray([5, 1, 3], dtype=np.int64) << 32)
    assert all(len(set(r.tolist())) == kp for r in rows)
    return q, x, rows


def _boundary_scores(space, q, x, counts, kp, k, e, flip):
    """NaN everywhere but [b][kp - 1] of the full queries: the largest score that proves (b + flip even) or the next float (odd)"""
    nq = q.shape[0]
    scores = np.full((nq, kp), np.nan, dtype=np.float32)
    n2q = S.sq_norms(q)
    for b in np.flatnonzero(np.asarray(counts) == kp):
        with np.errstate(all="ignore"):
            kth = np.sort(S.distances(space, q[b], x[b]))[k - 1: k]
            e_lo, found = M.bracket_score(lambda s: S.lower_bound32(space, s, n2q[b: b + 1], e), kth)
        scores[b, kp - 1] = (e_lo[0] if (b + flip) % 2 == 0 else M.f32_of_key(M.f32_key(e_lo) + 1)[0]) if found[0] else 0.25
    return scores


@pytest.mark.parametrize("kp", [1, 63, 64, 65, 257, 1000, 4096])
@pytest.mark.parametrize("space", SPACES)
def test_selection_edges(space, kp):
    q, x, rows = _selection_world(space, kp)
    e, nq = 3, q.shape[0]
    proven_seen = set()
    for flip, k in enumerate(sorted({1, (kp + 1) // 2, kp})):
        rng = np.random.default_rng(k)
        last = kp - 1 if space == "l2" else kp                                # l2: the overflowing query is followed by padding
        counts = np.clip(np.asarray([0, 1, k - 1, k, kp - 1, kp, last]), 0, kp).astype(np.int32)
        scores = _boundary_scores(space, q, x, counts, kp, k, e, flip)
        rows_in = rows.copy()
        for b in range(nq):
            rows_in[b, counts[b]:] = -1
            scores[b, counts[b]:] = np.nan
        with np.errstate(all="ignore"):
            ref = M.model_rescore(space, q, x, rows, scores, counts, k, e, S.GUARD[space])
            y = _engine_cands(space, x, counts, e, rng)
        _assert_rescore(_rescore(space, q, y, rows_in, scores, counts, k, e, S.GUARD[space]), ref, f"{space} kp={kp} k={k}")
        proven_seen |= {(int(c) == kp, int(p)) for c, p in zip(counts, ref[3])}
        if space == "l2" and kp >= 63 and k == kp:          # the overflowing group ranks by row, then one slot of padding
            d, r, c = ref[0][6], ref[1][6], int(ref[2][6])
            assert c == kp - 1 and np.isposinf(d[c - 5:]).all() and (np.diff(r[c - 5: c]) > 0).all() and r[c] == -1 and np.isfinite(d[0])
    if kp > 1:
        assert (True, 1) in proven_seen and (True, 0) in proven_seen and (False, 1) in proven_seen


# ---- c. the proof's boundary ----------------------------------------------------------------------------------------------------
def _three_scores(e_lo, kp):
    """[3 m][kp] scores: NaN but the last slot, which holds e_lo, the next float above it and the one after, case by case"""
    m = e_lo.shape[0]
    scores = np.full((3 * m, kp), np.nan, dtype=np.float32)
    scores[:, kp - 1] = M.f32_of_key(M.f32_key(e_lo)[:, None] + np.arange(3)[None, :]).reshape(-1)
    return scores


def _boundary_call(g, idx, e_lo, guard, what):
    space, kp, k, se = g["space"], g["kp"], g["k"], g["scale_exp"]
    q, x, rows = np.repeat(g["q"][idx], 3, axis=0), np.repeat(g["x"][idx], 3, axis=0), np.repeat(g["rows"][idx], 3, axis=0)
    scores = _three_scores(e_lo, kp)
    rng = np.random.default_rng(0)
    for counts, proven in ((np.full(q.shape[0], kp, dtype=np.int32), np.tile([1, 0, 0], len(idx))),
                           (np.full(q.shape[0], kp - 1, dtype=np.int32), np.ones(q.shape[0], dtype=int))):
        ref = M.model_rescore(space, q, x, rows, scores, counts, k, se, guard)
        assert (ref[3] == proven).all()
        y = _engine_cands(space, x, counts, se, rng)
        got = _rescore(space, q, y, rows, scores, counts, k, se, guard)
        _assert_rescore(got, ref, f"{what} counts={int(counts[0])}")


_GROUPS = M.boundary_cases()


@pytest.mark.parametrize("gi", range(len(_GROUPS)), ids=[f"{g['space']}-e{g['scale_exp']}-k{g['k']}of{g['kp']}" for g in _GROUPS])
def test_proof_flag_at_its_boundary(gi):
    g = _GROUPS[gi]
    idx = np.arange(g["kth"].shape[0])
    _boundary_call(g, idx, g["e_lo"], S.GUARD[g["space"]], f"{g['space']} e={g['scale_exp']} k={g['k']}")


@pytest.mark.parametrize("guard", [0.0, 1.0])
@pytest.mark.parametrize("space", SPACES)
def test_proof_flag_under_other_guards(space, guard):
    g = next(x for x in _GROUPS if x["space"] == space and x["scale_exp"] == 0 and x["k"] == x["kp"])
    idx = M.guard_case_indices(g)
    e_lo, found = M.guard_brackets(g, idx, guard)
    assert found.all()
    _boundary_call(g, idx, e_lo, guard, f"{space} guard={guard}")


@pytest.mark.parametrize("space", SPACES)
def test_query_norms_outside_the_guards_range_prove_nothing(space):
    """the score is -1 (with 1e-10 in l2: +1), where a bound that is computed anyway lies far ABOVE the k-th distance: only NaN, or
    for l2's small side (|p|^2 = |q|^2 + 1 is in range) the bound itself, gives 0. With a free slot the flag is 1 regardless."""
    rng = np.random.default_rng(17)
    dim, kp, k = 64, 6, 4
    u = M.unit(rng.standard_normal(dim))
    frac = rng.uniform(0.5, 1.0, size=(kp, 1))
    if space == "ip":
        cases = [(u * 1e-10, u * 1e9 * frac, -1.0, 0, True), (u * 1e16, u * 1e-17 * frac, -1.0, 0, True)]
    else:
        cases = [(u * 1e-10, 0.1 * rng.standard_normal((kp, dim)), 1.0, 0, False), (u * 1e16, u * frac, -1.0, -40, True)]
    for q, x, score, se, is_nan in cases:
        q, x = q[None, :].astype(np.float32), x[None, :, :].astype(np.float32)
        n2q = S.sq_norms(q)[0]
        assert np.isnan(M.scalar_lower_bound(space, score, n2q, se, S.GUARD[space])) == is_nan
        rows = rng.permutation(100)[:kp][None, :].astype(np.int64)
        scores = np.full((1, kp), np.nan, dtype=np.float32)
        scores[0, kp - 1] = score
        if is_nan:      # the teeth: the same arithmetic without the range check would prove the query
            kth = np.sort(S.distances(space, q[0], x[0]))[k - 1]
            gain = (1.0 - S.GUARD[space]) * np.sqrt(n2q) * 2.0 ** -se * (1 - 2.0 ** -29)       # |B| at a score of -1, from below
            unchecked = 1.0 + gain if space == "ip" else n2q * (1 - 2.0 ** -39) + 2.0 * gain
            assert np.float32(unchecked) > kth
        for c, proven in ((kp, 0), (kp - 1, 1)):
            counts = np.asarray([c], dtype=np.int32)
            ref = M.model_rescore(space, q, x, rows, scores, counts, k, se, S.GUARD[space])
            assert ref[3].tolist() == [proven]
            y = _engine_cands(space, x, counts, se, rng)
            _assert_rescore(_rescore(space, q, y, rows, scores, counts, k, se, S.GUARD[space]), ref, f"{space} |q|={np.sqrt(n2q):.0e} count={c}")


# ---- d. the page's addressing -----------------------------------------------------------------------------------------------------
def _allow_pattern(n_bits, rng):
    """random bits; around every 32-bit word edge the bits (.., 1 | 0, ..) and (.., 0 | 1, ..) alternate"""
    allow = rng.random(n_bits) < 0.5
    for w in range(1, n_bits // 32 + 1):
        if 32 * w < n_bits:
            allow[32 * w - 1], allow[32 * w] = (w % 2 == 0), (w % 2 == 1)
    return allow


@pytest.mark.parametrize("space", SPACES)
def test_page_addressing(space):
    import torch
    from rag_dpo_amd import engine as E
    from rag_dpo_amd import where as W
    dim, e, col0, tail = 64, 2, 2, 3
    rng = np.random.default_rng(31)
    q = rng.standard_normal((64, dim)).astype(np.float32)
    x = M.spread_rows(257, dim, seed=32)
    x[11] = q[2]
    full = M.model_page(space, q, x, None, 0)                   # computed once; every case below is a slice of it
    yt, qt = _t(_lift(space, x, e)), _t(q)
    seen_inf = seen_kept = 0
    for first_row in (0, 31, 32, 16389):
        allow = _allow_pattern(first_row + 257 + 40, rng)
        bits_t = _t(W.pack_bits(allow).view(np.int32))
        assert (S.unpack_bits(W.pack_bits(allow), allow.size) == allow).all()
        for nq in (1, 3, 64):
            for n in (1, 5, 257):
                for use_bits in (True, False):
                    out = torch.full((nq, col0 + n + tail), SENTINEL, dtype=torch.int32, device=_dev()).view(torch.float32)
                    E.space_distances(S.KIND[space], qt[:nq].contiguous(), yt[:n].contiguous(), e, bits_t if use_bits else None, first_row, out, col0)
                    got = _bits(_np(out))
                    want = full[:nq, :n].copy()
                    if use_bits:
                        want[:, ~allow[first_row: first_row + n]] = np.inf
                    what = f"{space} first_row={first_row} nq={nq} n={n} bits={use_bits}"
                    assert (got[:, col0: col0 + n] == _bits(want)).all(), what
                    assert (got[:, :col0] == SENTINEL).all() and (got[:, col0 + n:] == SENTINEL).all(), f"{what}: written outside the page"
                    seen_inf += int(np.isposinf(want).sum())
                    seen_kept += int(np.isfinite(want).sum())
    assert seen_inf > 1000 and seen_kept > 1000


# ---- e. the same inputs, the same bits --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("space", SPACES)
def test_same_inputs_same_bits_on_any_stream(space):
    import torch
    from rag_dpo_amd import engine as E
    dim, e, nq, kp, k = 260, 4, 5, 300, 40
    rng = np.random.default_rng(41)
    if space == "ip":
        q, x = M.cancelling_pairs(kp, dim, seed=9)
        q = q[:nq].copy()
    else:
        q, x = M.spread_rows(nq, dim, seed=10), M.spread_rows(kp, dim, seed=9)
    yt, qt = _t(_lift(space, x, e)), _t(q)
    cand = _t(np.tile(_lift(space, x, e), (nq, 1)))
    rows = _t(np.stack([rng.permutation(1 << 20)[:kp] for _ in range(nq)]).astype(np.int64))
    scores = _t(rng.uniform(-0.5, 0.5, size=(nq, kp)).astype(np.float32))
    counts = _t(np.asarray([kp, kp, kp - 1, 7, 0], dtype=np.int32))

    def run():
        out = torch.full((nq, kp), SENTINEL, dtype=torch.int32, device=_dev()).view(torch.float32)
        E.space_distances(S.KIND[space], qt, yt, e, None, 0, out, 0)
        return (out,) + tuple(E.space_rescore(S.KIND[space], qt, cand, rows, scores, counts, k, e, S.GUARD[space]))

    torch.cuda.synchronize(_dev())
    runs = [run(), run()]
    torch.cuda.synchronize(_dev())
    side = torch.cuda.Stream(device=_dev())
    with torch.cuda.stream(side):
        runs.append(run())
    side.synchronize()
    first = [_np(t).tobytes() for t in runs[0]]
    assert (_bits(_np(runs[0][0])) != SENTINEL).all()
    for other in runs[1:]:
        assert [_np(t).tobytes() for t in other] == first
    want = M.model_page(space, q, x, None, 0)
    assert (_bits(_np(runs[0][0])) == _bits(want)).all()
