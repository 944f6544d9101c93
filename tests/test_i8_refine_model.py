"""CPU model of the two-round exact re-score of int8 searches (DESIGN.md §5 "two-round re-score", refine_kernel.hpp), on the
quantiser of test_i8_bound_model.py. The hits of a query carry a coarse score with |coarse - exact| <= E_q. Round one re-scores
S1 = the hits that reach the k1-th largest coarse score (k1 = min(m, pilot k)) and takes X1, the k-th largest exact score in S1;
round two re-scores S2 = {coarse >= t3} \\ S1 with t3 = X1 - E_q rounded toward -inf in fp32. Claims checked here:
  * the oracle top-k of the hits (score desc, row asc) is the top-k of S1 u S2 — for pilot 1, 4 and "all", with exact ties at the
    k-th score and with fewer hits than k1, on random, embedding-like and adversarial rows;
  * t3 >= c_k - 2 E_q: the band is never wider than the single band it replaces;
  * a band of E_q / 4 in place of E_q drops a true top-k row in a construction made for it: the first check bites.
The kernel's fallback (more than REFINE_PMAX rows tie at the k1-th coarse score: the single band) is not modelled."""
import numpy as np

from test_i8_bound_model import F32, normalize, quant_query, quant_rows


def sub_down(a, b):
    """a - b in float32, rounded toward -inf (refine_kernel.hpp sub_down)"""
    d = F32(F32(a) - F32(b))
    if np.float64(d) > np.float64(a) - np.float64(b):
        d = np.nextafter(d, F32(-np.inf))
    return d


def e_q(e, n, eps_max):
    """k_tau8: E_q = e_q (1 + 1e-6) + n_q eps_max + 1e-6 in fp64, rounded up to float32"""
    E = np.float64(e) * (1.0 + 1e-6) + np.float64(n) * np.float64(eps_max) + 1e-6
    f = F32(E)
    return np.nextafter(f, F32(np.inf)) if np.float64(f) < E else f


def kth_largest(v, k):
    return np.sort(v)[::-1][k - 1]


def two_rounds(coarse, exact, Eq, k, pilot, band=1.0):
    """(member mask of S1 u S2, t3, c_k) over the hits; pilot = "all": S1 is every hit; band: the multiple of E_q subtracted
    (1 unless a mutant is modelled)"""
    m = len(coarse)
    k1 = m if pilot == "all" else min(m, pilot * k)
    c_k1 = kth_largest(coarse, k1)
    S1 = coarse >= c_k1
    t3 = F32(-np.inf)
    if S1.sum() >= k:
        t3 = sub_down(kth_largest(exact[S1], k), F32(band) * Eq)
    S2 = (coarse >= t3) & ~S1
    c_k = kth_largest(coarse, min(k, m))
    return S1 | S2, t3, c_k


def topk(exact, rows, k):
    order = np.lexsort((rows, -exact.astype(np.float64)))[:k]
    return rows[order], exact[order]


def corpus_scores(q, blocks):
    """coarse, exact (float32) of every row of the 32-row blocks and the query's E_q with the corpus-wide eps_max"""
    t, q8, e, n = quant_query(q)
    coarse, exact, eps_max = [], [], F32(0)
    for b in blocks:
        s, c8, eps = quant_rows(b)
        D = c8.astype(np.int64) @ q8.astype(np.int64)
        coarse.append(((D.astype(F32) * s).astype(F32) * t).astype(F32))
        exact.append((b.astype(np.float64) * q.astype(np.float64)[None, :]).sum(axis=1).astype(F32))   # (row by row: equal rows, equal bits)
        eps_max = max(eps_max, eps)
    return np.concatenate(coarse), np.concatenate(exact), e_q(e, n, eps_max)


def make_blocks(kind, q, rng, nb, d):
    out = []
    for _ in range(nb):
        if kind == "random":                             # with a pull toward the query: a populated top of the score range
            b = normalize(rng.standard_normal((32, d)) + 3 * q[None, :] * np.sqrt(d) * rng.random((32, 1)) ** 4)
        elif kind == "embed":                            # a document's chunks: near-duplicates around a shared direction
            mu = rng.standard_normal(d) + 2 * q * np.sqrt(d) * rng.random()
            b = normalize(mu + 0.05 * rng.standard_normal((32, d)))
        else:                                            # adversarial: every row's rounding error aligned with the query
            base = normalize(rng.standard_normal((32, d)) + 2 * q[None, :] * np.sqrt(d) * rng.random((32, 1)))
            s = np.abs(base).max() / 127
            grid = np.rint(base / s) * s
            b = normalize(grid + 0.49 * s * np.sign(q)[None, :] * (np.abs(base) < 126 * s))
        out.append(b)
    return out


def check(coarse, exact, Eq, k, rows=None):
    rows = np.arange(len(coarse)) if rows is None else rows
    assert (np.abs(coarse.astype(np.float64) - exact.astype(np.float64)) <= np.float64(Eq)).all()   # the premise (test_i8_bound_model)
    want = topk(exact, rows, k)
    sizes = []
    for pilot in (1, 4, "all"):
        S, t3, c_k = two_rounds(coarse, exact, Eq, k, pilot)
        got = topk(exact[S], rows[S], k)
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])
        if len(coarse) >= k:
            assert t3 >= sub_down(c_k, F32(2) * Eq), (pilot, t3, c_k, Eq)
        sizes.append(int(S.sum()))
    return sizes


def test_two_rounds_keep_the_top_k():
    rng = np.random.default_rng(5)
    d, k = 256, 10
    narrower = 0
    for trial in range(30):
        kind = ("random", "embed", "adversarial")[trial % 3]
        q = normalize(rng.standard_normal((1, d)))[0]
        blocks = make_blocks(kind, q, rng, 24, d)
        if trial % 2:                                    # exact ties at the k-th score: copies of that row in three blocks
            _, exact, _ = corpus_scores(q, blocks)
            r = int(np.argsort(-exact.astype(np.float64), kind="stable")[k - 1])
            row = blocks[r // 32][r % 32].copy()
            for b, i in ((0, 3), (7, 31), (23, 0)):
                blocks[b][i] = row
        coarse, exact, Eq = corpus_scores(q, blocks)
        if trial % 2:
            assert (exact == kth_largest(exact, k)).sum() >= 2
        sizes = check(coarse, exact, Eq, k)
        one_band = int((coarse >= F32(kth_largest(coarse, k) - F32(2) * Eq)).sum())
        assert sizes[0] <= one_band                      # pilot 1: S1 lies inside the single band, so never more rows than it re-scores
        narrower += sizes[0] < one_band
        print(kind, 'rows re-scored at pilot 1 / 4 / all:', sizes, 'single band:', one_band)
        # the hits of a search: what a threshold let through, down to fewer than k1 and fewer than k of them
        for m in (k - 3, k, k + 5, 4 * k - 1, 200):
            hit = np.argsort(-coarse.astype(np.float64), kind="stable")[:m]
            hit = np.sort(hit)
            check(coarse[hit], exact[hit], Eq, k, rows=hit)
    assert narrower >= 20                                # and usually fewer


def test_a_quarter_band_drops_a_true_top_row():
    """k = 1, two hits. B's rounding error is aligned with the query, which sits on its own grid (e_q ~ 0): coarse(B) lies most
    of E_q below exact(B). A is a plain row (a small error), its exact score between coarse(B) + E_q / 4 and exact(B), its coarse
    score above coarse(B): A is the pilot, X1 = exact(A). With the band E_q the second round re-scores B and B wins; with E_q / 4
    it does not, and A is returned: the wrong row."""
    rng = np.random.default_rng(11)
    d = 256
    q = normalize(np.sign(rng.standard_normal((1, d))))[0]
    base = normalize(rng.standard_normal((32, d)) + 0.5 * q[None, :] * np.sqrt(d))
    s = np.abs(base).max() / 127
    grid = np.rint(base / s) * s
    adv = normalize(grid + 0.49 * s * np.sign(q)[None, :] * (np.abs(base) < 126 * s))
    plain = normalize(rng.standard_normal((32 * 200, d)) + 0.5 * q[None, :] * np.sqrt(d) * (0.9 + 0.2 * rng.random((32 * 200, 1))))
    blocks = [adv] + [plain[32 * i:32 * i + 32] for i in range(200)]
    coarse, exact, Eq = corpus_scores(q, blocks)
    gap = exact[:32].astype(np.float64) - coarse[:32]
    b = int(np.argmax(gap))
    assert gap[b] > 0.5 * Eq, (gap[b], Eq)               # the aligned row uses more than half the bound
    lo, hi = coarse[b] + 0.25 * np.float64(Eq) + 1e-6, exact[b]
    cand = [a for a in range(32, len(coarse)) if lo < exact[a] < hi and coarse[a] > coarse[b]]
    assert cand, "no row between coarse(B) + E_q / 4 and exact(B)"
    hit = np.array([b, cand[0]])
    c, x = coarse[hit], exact[hit]
    S, _, _ = two_rounds(c, x, Eq, 1, 1)
    assert S.all() and topk(x[S], hit[S], 1)[0][0] == b
    S, _, _ = two_rounds(c, x, Eq, 1, 1, band=0.25)
    assert not S[0] and topk(x[S], hit[S], 1)[0][0] != b  # the mutant loses the true top row
