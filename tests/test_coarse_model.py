"""The coarse-pass model of tests/coarse_model.py and its constructions (CPU, no GPU): every construction reaches the fraction of
the error bound E it is built for, the model stays within E everywhere, §5's inequality chain holds for every dimension the
library accepts, and each plausible regression of the scan's numerics changes a prediction tests/test_gpu_coarse_bound.py asserts
on the GPU — the gap those GPU tests close (the old suite's N(0,1) inputs use 3.6 % of E)."""
import numpy as np
import pytest

import coarse_model as M

DIMS = (64, 100, 1024, 4096)


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle):
    return oracle


def _err(q, rows, dim):
    qh = M.normalize(q)[0]
    ch = M.normalize(rows)
    cs = M.coarse(qh, ch, dim)
    return cs, M.exact(qh, ch)


@pytest.mark.parametrize("dim", DIMS)
def test_aligned_worst_case_fraction_of_e(dim):
    """the row equal to the query, every scaled element just past an fp16 midpoint: coarse - exact = 0.999 * 2^-10 (up) and
    -0.94 * 2^-10 (down) after the library's own normalisation — 0.78 E at d = 1024, 0.96 E at d = 64"""
    e = float(M.e_bound(dim))
    want = {64: 0.955, 100: 0.94, 1024: 0.775, 4096: 0.48}[dim]
    for sign in (+1, -1):
        q, r = M.aligned(dim, list(range(16)), sign)
        cs, ex = _err(q, r[None], dim)
        frac = (cs.value[0] - ex[0]) / e
        assert sign * frac >= want * (0.985 if sign < 0 else 1.0), (sign, frac)
        assert abs(frac) + cs.bound[0] / e <= 1.0
        assert (sign > 0) == (cs.value[0] > ex[0])
    q, r = M.aligned(dim, list(range(16)), +1)
    assert abs(_err(q, r[None], dim)[0].value[0] - 1.0 - 0.999 * 2.0 ** -10) < 2e-6


@pytest.mark.parametrize("dim", DIMS)
def test_split_pair(dim):
    """exact(A) > exact(B) by ~1e-5, coarse(B) - coarse(A) ~ 4/3 2^-10 = 1.28e-3: more than E at d <= 1024 (0.51 of 2E at
    d = 1024), inside 2E everywhere"""
    q, a, b = M.split_pair(dim, list(range(34)))
    cs, ex = _err(q, np.stack([a, b]), dim)
    from oracle import oracle as O
    s32 = O.scores(M.normalize(np.stack([a, b])), M.normalize(q)[0])
    assert s32[0] > s32[1] and 0 < ex[0] - ex[1] < 2e-5
    gap = (cs.lo[1] - cs.hi[0])
    e = float(M.e_bound(dim))
    assert gap >= 1.28e-3
    assert cs.hi[1] - cs.lo[0] < 2 * e
    if dim <= 1024:
        assert gap > e
    assert gap / (2 * e) >= {64: 0.63, 100: 0.62, 1024: 0.51, 4096: 0.31}[dim]


@pytest.mark.parametrize("dim", DIMS)
def test_model_within_e(dim):
    """|coarse - exact| + the accumulation bound <= E over every construction and a random sweep (N(0,1) rows, planted
    neighbours, rows whose elements fall into fp16's subnormal range)"""
    e = float(M.e_bound(dim))
    worst = 0.0
    for sign in (+1, -1):
        q, r = M.aligned(dim, list(range(16)), sign)
        cs, ex = _err(q, r[None], dim)
        worst = max(worst, float(np.max(np.abs(cs.value - ex) + cs.bound)))
    q, a, b = M.split_pair(dim, list(range(34)))
    cs, ex = _err(q, np.stack([a, b]), dim)
    worst = max(worst, float(np.max(np.abs(cs.value - ex) + cs.bound)))
    for side in ("row", "query"):
        q, anc, pr, _ = M.subnormal_ladder(dim, list(range(17)), side)
        cs, ex = _err(q, np.vstack([anc[None], pr]), dim)
        worst = max(worst, float(np.max(np.abs(cs.value - ex) + cs.bound)))
    rng = np.random.default_rng(dim)
    x = rng.standard_normal((600, dim)).astype(np.float32)
    x[300:] *= np.exp(rng.uniform(-14, 0, size=(300, dim))).astype(np.float32)   # many elements in the subnormal range
    qs = x[:8] + 0.05 * rng.standard_normal((8, dim)).astype(np.float32)
    for q in qs:
        cs, ex = _err(q, x, dim)
        worst = max(worst, float(np.max(np.abs(cs.value - ex) + cs.bound)))
    assert worst <= e, (worst, e)


def test_inequality_chain_every_dim():
    """§5: fp16 term + subnormal term + accumulation term <= E(dim_pad) for every dim the library accepts"""
    for dim in range(4, M.MAX_DIM + 1, 4):
        f, s, a = M.e_terms(dim)
        assert f + s + a <= float(M.e_bound(dim)), dim
    # the margin E leaves at d = 1024 (what a restated subnormal term could use)
    f, s, a = M.e_terms(1024)
    assert 1.5e-4 < float(M.e_bound(1024)) - (f + s + a) < 1.7e-4


@pytest.mark.parametrize("dim", DIMS)
def test_ladder_is_pinned_and_rtz_moves_it(dim):
    """the dyadic ladder: anchor and probes exact in fp32 (the kernel's coarse scores are the model's to the bit), probes on both
    sides of t2 (the nearest in-band one within 2.5e-6, the nearest outside within 6e-6); a round-toward-zero conversion moves the predicted `rescored` count"""
    cols = list(range(14))
    q = M.dyadic_query(dim, cols)
    t2 = M.ladder_prediction(q, q[None], 1, dim)["t2"]
    rows, above = M.ladder_probes(q, t2, dim, cols, np.random.default_rng(1))
    allr = np.vstack([q[None], rows])
    p = M.ladder_prediction(q, allr, 1, dim, use_boot=True, use_small=True)
    cs = p["coarse"]
    assert cs.exact.all() and p["c_k"] == np.float32(1.0)
    assert p["rescored"] == 1 + above.sum() and p["emitted"] == p["rescored"]
    d = cs.value[1:] - float(t2)
    assert np.all(d[above] >= 0) and np.all(d[~above] < 0) and np.max(np.abs(d)) < 1e-5
    assert d[above].min() < 2.5e-6 and -d[~above].max() < 6e-6
    assert M.ladder_prediction(q, allr, 1, dim, rtz=True)["rescored"] < p["rescored"]
    # the slack without its factor 2 (E instead of 2E): the proven threshold lies above t2, so k_refine's verification c_k - 2E >= T
    # fails for every query — the GPU tests see it as retried queries with spec_tau = 0
    bad_t = np.float32(p["c_k"] - M.e_bound(dim))
    assert M.band_edge(p["c_k"], dim) < bad_t


@pytest.mark.parametrize("dim", (64, 100, 1024))
def test_split_pair_kills_a_narrow_band(dim):
    """k_refine with E (or E/2) instead of 2E ranks B first: the wrong top-1"""
    q, a, b = M.split_pair(dim, list(range(34)))
    rows = np.stack([a, b])
    assert list(M.band_top(q, rows, 1, dim)) == [0]
    assert list(M.band_top(q, rows, 1, dim, band=M.e_bound(dim))) == [1]
    assert list(M.band_top(q, rows, 1, dim, band=M.e_bound(dim) / 2)) == [1]


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("side", ["row", "query"])
def test_subnormal_ladder_sees_flushing(dim, side):
    """band membership of probes that rest on fp16 subnormal products: a conversion or an MFMA that flushed them to zero moves
    the predicted `rescored` count; everything is exact in fp32"""
    q, anc, pr, sub = M.subnormal_ladder(dim, list(range(17)), side)
    allr = np.vstack([anc[None], pr])
    p = M.ladder_prediction(q, allr, 1, dim)
    assert p["coarse"].exact.all()
    assert M.ladder_prediction(q, allr, 1, dim, flush=True)["rescored"] < p["rescored"]
    assert 0 < float(p["t2"]) < float(p["c_k"])
