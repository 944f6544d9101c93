"""CPU: the references and the inputs of tests/test_gpu_space_kernels.py, held to things that share no code with them, and the
conditions that file's GPU tests rest on — computed from the model (rag_dpo_amd/spaces.py, tests/space_model.py) alone:
  * scalar_lower_bound (the proof's bound, one Python float at a time) equals spaces.lower_bound32 bit for bit, the bound falls
    monotonically with the engine score (the boundary search is a bisection), and it is sound on small worlds;
  * model_rescore / model_page give the contract's distances (scalar_distance bit for bit);
  * cancelling_pairs makes the ip distance depend on the fp64 summation order: the floors asserted here are what gives the GPU
    test its teeth against a kernel that sums in another order. l2 HAS NO SUCH INPUT: its terms (q_j - x_j)^2 are non-negative, so
    a different order moves the fp64 sum by a few 2^-53 relative, which reaches the fp32 result only when the sum lies within
    that of a rounding boundary (a chance of about 2^-27 per pair). At ragged dims the GPU test's l2 cases catch dropped, doubled
    or misplaced terms, not the order; the order itself is pinned by ip, by k_space_measure's fp64 output, and by the code being
    one function (space_sum) for both modes;
  * every case of boundary_cases() has a bracket of two adjacent fp32 scores, cases sit on both sides of U = 0, the bound EQUALS
    the k-th distance on the unproven side, and the plausible wrong bounds (>=, UP30 / DN30 swapped, the other branch at U < 0,
    a guard that is dropped, doubled or subtracted, a bound that ignores the scale) each get some case of the list wrong."""
import math

import numpy as np
import pytest

from rag_dpo_amd import spaces as S

import space_model as M

SPACES = ("ip", "l2")
GPU_DIMS = (4, 60, 64, 68, 252, 256, 260, 508, 516, 1020, 1024, 1028, 4092, 4096)   # test_gpu_space_kernels.DIMS (4096: ip only)


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def _score_grid(space):
    g = np.float32(-S.GUARD[space])            # U = e + G changes sign here
    vals = [-1.0, 1.0, 0.0, -0.0, g, np.nextafter(g, np.float32(-2)), np.nextafter(g, np.float32(2)), np.float32(-g),
            1e-30, -1e-30, 0.25, -0.25, 0.9999999, -0.9999999, 3e-7, -3e-7]
    return np.asarray(vals, dtype=np.float32)


@pytest.mark.parametrize("space", SPACES)
def test_scalar_lower_bound_is_the_numpy_bound(space):
    norms = [1e-10, 1.00001e-9, 3e-5, 0.5, 1.0, 7.25, 1e4, 1e9, 0.99999e15, 1e16]
    n2q = np.asarray([x * x for x in norms] + [0.0, 1e-30, 0.9e-18, 1.1e30, 1e40, 1e-18, 1e30])   # the last four: the sides and the edges
    scores = _score_grid(space)
    seen_nan = 0
    for se in (-20, -1, 0, 9, 40):
        want = np.stack([S.lower_bound32(space, scores, n, se) for n in n2q])
        got = np.asarray([[M.scalar_lower_bound(space, e, n, se, S.GUARD[space]) for e in scores] for n in n2q], dtype=np.float32)
        assert (_bits(got) == _bits(want)).all(), f"scale_exp {se}"
        seen_nan += int(np.isnan(got).sum())
        pn2 = n2q + (1.0 if space == "l2" else 0.0)
        assert (np.isnan(got).all(axis=1) == ~((pn2 >= 1e-18) & (pn2 <= 1e30))).all()
        assert not np.isnan(got[(pn2 >= 1e-18) & (pn2 <= 1e30)]).any()
    assert seen_nan


@pytest.mark.parametrize("space", SPACES)
def test_lower_bound_never_rises_with_the_score(space):
    g = S.GUARD[space]
    keys = [np.arange(-40, 41)]                                                      # around +-0
    for c in (-1.0, 1.0, -g, g, 0.25, -0.25, -3e-7, 1e-3):
        k0 = int(M.f32_key(np.float32(c)))
        keys.append(np.arange(k0 - 40, k0 + 41))
    keys.append(np.linspace(int(M.f32_key(np.float32(-1.0))), int(M.f32_key(np.float32(1.0))), 20001).astype(np.int64))
    lo, hi = int(M.f32_key(np.float32(-1.0))), int(M.f32_key(np.float32(1.0)))
    e = M.f32_of_key(np.unique(np.clip(np.concatenate(keys), lo, hi)))
    assert (np.diff(e.astype(np.float64)) >= 0).all() and (e.astype(np.float64) + g < 0).any() and (e.astype(np.float64) + g > 0).any()
    for se in (-6, 0, 9):
        for n2q in (1e-6, 0.3, 1.0, 50.0, 1e7):
            lb = S.lower_bound32(space, e, n2q, se).astype(np.float64)
            assert not np.isnan(lb).any() and (np.diff(lb) <= 0).all(), (se, n2q)


@pytest.mark.parametrize("space", SPACES)
def test_lower_bound_is_sound_on_small_worlds(space):
    dim, n = 64, 300
    for seed, spread in ((1, False), (2, True)):
        rng = np.random.default_rng(seed)
        x = M.spread_rows(n, dim, seed) if spread else rng.standard_normal((n, dim)).astype(np.float32)
        q = np.concatenate([rng.standard_normal((6, dim)), 0.05 * rng.standard_normal((3, dim)), x[:2] * 1.0]).astype(np.float32)
        eng = M.make_engine(space, dim, x)
        sc, ro, cn = eng.inner.search(S.lift_queries(space, q), n)
        assert (cn == n).all()
        n2q = S.sq_norms(q)
        d = np.stack([S.distances(space, q[b], x[ro[b]]) for b in range(q.shape[0])])      # in the engine's order
        for kp in (1, 2, 17, 150, n - 1):
            lb = S.lower_bound32(space, sc[:, kp - 1], n2q, eng.scale_exp)
            assert not np.isnan(lb).any()
            assert (d[:, kp:] >= lb[:, None]).all(), f"{space} seed {seed} kp {kp}: a row outside the fetch lies below the bound"


@pytest.mark.parametrize("space", SPACES)
def test_model_rescore_and_page_give_the_contract(space):
    rng = np.random.default_rng(5)
    dim, nq, kp, k = 68, 4, 9, 4
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    x = M.spread_rows(nq * kp, dim, seed=8).reshape(nq, kp, dim)
    x[1, 5] = x[1, 2]                                  # a tie: the lower row id first
    rows = np.stack([rng.permutation(50)[:kp] for _ in range(nq)]).astype(np.int64)
    scores = np.full((nq, kp), np.nan, dtype=np.float32)
    scores[:, kp - 1] = [-1.0, 1.0, -1.0, 0.0]
    counts = np.asarray([kp, kp, 2, 0], dtype=np.int32)
    od, orow, oc, pv = M.model_rescore(space, q, x, rows, scores, counts, k, 0, S.GUARD[space])
    assert oc.tolist() == [k, k, 2, 0] and pv.tolist() == [1, 0, 1, 1]          # (a score of -1 proves, a score of 1 cannot)
    for b in range(nq):
        c = int(counts[b])
        want = sorted((float(M.scalar_distance(space, q[b], x[b, j])), int(rows[b, j])) for j in range(c))[:k]
        assert [(float(a), int(r)) for a, r in zip(od[b, : oc[b]], orow[b, : oc[b]])] == want
        assert np.isposinf(od[b, oc[b]:]).all() and (orow[b, oc[b]:] == -1).all()
    # the page: scalar_distance bit for bit, plain fp64 to fp32 rounding of a well-conditioned sum, the allow bits by first_row + r
    flat = x.reshape(-1, dim)
    allow = rng.random(100 + flat.shape[0]) < 0.5
    page = M.model_page(space, q, flat, allow, 100)
    free = M.model_page(space, q, flat, None, 100)
    assert (np.isposinf(page) == ~allow[100:][None, :].repeat(nq, 0)).all() and (page[:, allow[100:]] == free[:, allow[100:]]).all()
    for b in range(nq):
        for r in range(0, flat.shape[0], 5):
            assert _bits(free[b, r]) == _bits(M.scalar_distance(space, q[b], flat[r]))
    plain = M.plain_distances(space, q, flat)
    size = 1.0 + np.abs(q.astype(np.float64)) @ np.abs(flat.astype(np.float64)).T if space == "ip" else plain
    assert (np.abs(free.astype(np.float64) - plain) <= 2.0 ** -24 * np.abs(plain) + 2.0 ** -45 * size).all()


@pytest.mark.parametrize("dim", GPU_DIMS)
def test_cancelling_pairs_show_the_summation_order(dim):
    q, x = M.cancelling_pairs(200, dim, seed=1)
    right = np.stack([S.distances("ip", q[i], x[i: i + 1])[0] for i in range(200)])
    wrong = M.left_to_right_ip(q, x)
    assert np.isfinite(right).all() and np.isfinite(wrong).all()
    differ = float((_bits(right) != _bits(wrong)).mean())
    assert differ >= 0.5 if dim >= 60 else differ > 0.0, differ
    # every (query, row) combination cancels, not only the pairs made together: the GPU test takes 3 queries x 37 rows
    cross = S.distances("ip", q[0], x[:37])
    assert np.isfinite(cross).all() and (_bits(cross) != _bits(M.left_to_right_ip(np.repeat(q[:1], 37, 0), x[:37]))).mean() >= (0.5 if dim >= 60 else 0.0)
    # the rows of the measure test: the squared norm's fp64 bits depend on the order as well
    w = M.wide_rows(41, dim, seed=3).astype(np.float64)
    lr = np.zeros(41)
    for j in range(dim):
        lr = lr + w[:, j] * w[:, j]
    assert (lr != S.sq_norms(w)).mean() >= (0.5 if dim >= 60 else 0.0)


def test_ordered_keys_walk_the_floats():
    v = np.asarray([-1.0, -1e-45, -0.0, 0.0, 1e-45, 0.5, 1.0], dtype=np.float32)
    k = M.f32_key(v)
    assert k.tolist() == sorted(k.tolist()) and k[2] == k[3] == 0 and k[1] == -1 and k[4] == 1
    assert (M.f32_of_key(k + 1)[[0, 5]] == np.nextafter(v[[0, 5]], np.float32(2))).all()
    assert (_bits(M.f32_of_key(M.f32_key(v[[0, 1, 4, 5, 6]]))) == _bits(v[[0, 1, 4, 5, 6]])).all()


# the bound as a wrong kernel might compute it: scalar_lower_bound with one deliberate fault each
def _wrong_bound(fault, space, e_last, n2q, scale_exp, guard):
    e32, n2q = float(np.float32(e_last)), float(n2q)
    up30, dn30, t40 = 1.0 + 2.0 ** -30, 1.0 - 2.0 ** -30, 2.0 ** -40
    if fault == "swapped":
        up_b, dn_b = dn30, up30
    else:
        up_b, dn_b = up30, dn30
    guard = {"no guard": 0.0, "guard twice": 2.0 * guard, "guard subtracted": -guard}.get(fault, guard)
    se = 0 if fault == "no scale" else int(scale_exp)
    p = math.sqrt(n2q + 1.0 if space == "l2" else n2q)
    u = e32 + guard
    if fault == "one branch":
        pb = p * up_b
    else:
        pb = p * up_b if u >= 0.0 else p * dn_b
    b = math.ldexp(u * pb, -se)
    if space == "l2":
        bup = b + abs(b) * t40
        lb = n2q * (1.0 - t40) - 2.0 * bup
    else:
        bup = b + math.ldexp(p * up30 * t40, -se)
        bup = bup + abs(bup) * t40
        lb = 1.0 - bup
    lb = lb - abs(lb) * t40
    return np.float32(lb)


@pytest.fixture(scope="module")
def groups():
    return M.boundary_cases()


def test_boundary_cases_bracket_the_proof(groups):
    assert {(g["space"], g["scale_exp"], g["k"] == g["kp"]) for g in groups} == \
        {(s, e, full) for s in SPACES for e in (-6, 0, 9) for full in (True, False)}
    equal = {s: 0 for s in SPACES}
    for g in groups:
        space, se, G = g["space"], g["scale_exp"], S.GUARD[g["space"]]
        m = g["kth"].shape[0]
        assert (g["side"] > 0).sum() >= M.BOUNDARY_PER_GROUP // 2 and (g["side"] < 0).sum() >= M.BOUNDARY_PER_GROUP // 2
        assert g["q"].shape == (m, M.BOUNDARY_DIM) and g["x"].shape == (m, g["kp"], M.BOUNDARY_DIM)
        lo, hi = S.lower_bound32(space, g["e_lo"], g["n2q"], se), S.lower_bound32(space, g["e_hi"], g["n2q"], se)
        assert (lo > g["kth"]).all() and (hi <= g["kth"]).all()
        assert (M.f32_key(g["e_hi"]) - M.f32_key(g["e_lo"]) == 1).all()                 # adjacent fp32 values
        assert (np.abs(g["e_hi"]) < 1).all() and (np.abs(g["e_lo"]) < 1).all()
        u = g["e_lo"].astype(np.float64) + G
        assert (np.sign(u) == g["side"]).all() and (np.sign(g["e_hi"].astype(np.float64) + G) == g["side"]).all()
        assert (np.abs(g["e_lo"][g["side"] < 0]) > G).all()                              # a negative last score beyond the guard
        equal[space] += int((hi == g["kth"]).sum())
        # the k-th distance is what model_rescore ranks k-th, and the scalar bound takes the same decisions
        for i in range(0, m, 7):
            d = sorted(float(M.scalar_distance(space, g["q"][i], g["x"][i, j])) for j in range(g["kp"]))
            assert np.float32(d[g["k"] - 1]) == g["kth"][i]
            assert M.scalar_lower_bound(space, g["e_lo"][i], g["n2q"][i], se, G) > g["kth"][i]
            assert M.scalar_lower_bound(space, g["e_hi"][i], g["n2q"][i], se, G) == hi[i]
    assert all(v >= 5 for v in equal.values()), equal       # bound == k-th distance on the unproven side: `>=` would prove these


@pytest.mark.parametrize("fault", ["swapped", "one branch", "no guard", "guard twice", "guard subtracted", "no scale"])
def test_boundary_cases_tell_a_wrong_bound(groups, fault):
    """each fault changes proven = (1, 0, 0) at the scores (e_lo, e_hi, the next) of some case — of BOTH spaces for the faults of the
    guard. (`swapped` and `one branch` move the bound by 2^-29 relative, so they show in about one case in 40: that is why the
    list is this long.)"""
    hit = {s: 0 for s in SPACES}
    for g in groups:
        space, se, G = g["space"], g["scale_exp"], S.GUARD[g["space"]]
        for i in range(g["kth"].shape[0]):
            if fault == "one branch" and g["side"][i] > 0:
                continue
            e3 = M.f32_of_key(M.f32_key(g["e_lo"][i]) + np.arange(3))
            got = [bool(_wrong_bound(fault, space, e, g["n2q"][i], se, G) > g["kth"][i]) for e in e3]
            hit[space] += got != [True, False, False]
    assert sum(hit.values()) >= 1 and (fault in ("swapped", "one branch") or all(hit.values())), hit


@pytest.mark.parametrize("guard", [0.0, 1.0])
@pytest.mark.parametrize("space", SPACES)
def test_other_guards_have_a_boundary_too(groups, space, guard):
    """the GPU test passes guard = 0 and guard = 1 (the ABI's range) on the positive-side cases at scale_exp 0: their boundary
    under those guards, found with scalar_lower_bound, lies inside [-1, 1] and elsewhere than the product guard's"""
    g = next(x for x in groups if x["space"] == space and x["scale_exp"] == 0 and x["k"] == x["kp"])
    idx = M.guard_case_indices(g)
    assert len(idx) >= 4
    e_lo, found = M.guard_brackets(g, idx, guard)
    assert found.all() and (e_lo != g["e_lo"][idx]).all()
    for j, i in enumerate(idx):
        nxt = M.f32_of_key(M.f32_key(e_lo[j]) + 1)
        assert M.scalar_lower_bound(space, e_lo[j], g["n2q"][i], 0, guard) > g["kth"][i]
        assert not M.scalar_lower_bound(space, nxt, g["n2q"][i], 0, guard) > g["kth"][i]
