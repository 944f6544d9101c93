"""CPU model of the int8 scan's classes of block error (tests/i8_class_model.py; DESIGN.md §5 "classes of eps_b"). A block is charged
the edge of its class of eps_b instead of the corpus' largest; the claims, on random, embedding-like and adversarial blocks:

  * every row whose exact score reaches T is emitted, with 1, 2, 4 and 8 classes;
  * a row that is not emitted scores below taus8 + E_q — what keeps k_refine's verification X - E_q >= taus8 sufficient — on the rows
    of the corpus and at the proof's own edge (a row of class c with the largest coarse score that is not emitted, coarse < tau_c, and
    the whole of E_{q,c} on top);
  * the hits with 8 classes are a subset of those with 4, those of those with 2, those of those with one class, and there are fewer;
  * the adversarial case: a flat block in the lowest class holds one row whose rounding error is aligned with the query and uses more
    than half of E_{q,0}; it is emitted;
  * each of four mistakes loses a row, or fails the bound, in a case built for it: a class charged the next lower class's edge, an
    edge taken one order statistic too low, a top edge not refreshed after an append raised eps_max, taus8 left at the top class's
    tau."""
import numpy as np

import i8_class_model as CM
import i8_model as M
from test_i8_bound_model import F32, normalize

D, NB, K = 256, 64, 10


def _spike(rng, d, z):
    """a row with one element z and little else: it sets its block's scale s_b = z / 127, and with it the block's eps_b"""
    v = (0.3 * normalize(rng.standard_normal((1, d)))[0]).astype(F32)
    v[int(rng.integers(d))] = z
    return v


def _corpus(kind, rng, q, nb=NB, d=D, zs=None):
    """nb 32-row blocks of rows with norm <= 1 (the bound's premise); row 0 of every block is a spike row of size zs[b] (a 2x spread of
    scales: every class is populated)"""
    zs = 0.2 * 2.0 ** rng.permutation(np.arange(nb) / nb) if zs is None else zs
    blocks = []
    for b in range(nb):
        if kind == "random":
            rows = 0.5 * normalize(rng.standard_normal((32, d)) + 4 * q[None, :] * np.sqrt(d) * rng.random((32, 1)) ** 4)
        elif kind == "embed":                            # a document's chunks around a shared direction
            mu = rng.standard_normal(d) + 2 * q * np.sqrt(d) * rng.random()
            rows = 0.5 * normalize(mu + 0.05 * rng.standard_normal((32, d)))
        else:                                            # adversarial: row 1's rounding error is aligned with the query
            rows = 0.5 * normalize(rng.standard_normal((32, d)) + 2 * q[None, :] * np.sqrt(d) * rng.random((32, 1)))
            s = F32(F32(zs[b]) / F32(127))
            grid = (np.rint(rows[1] / s) * s).astype(F32)
            rows[1] = (grid + F32(0.49) * s * np.sign(q)).astype(F32)
        rows = rows.astype(F32)
        rows[0] = _spike(rng, d, zs[b])
        assert np.abs(rows[1:]).max() < 0.98 * zs[b] and (np.linalg.norm(rows.astype(np.float64), axis=1) <= 1.0).all()
        blocks.append(rows)
    return np.concatenate(blocks), zs


def _state(y):
    cc = CM.ClassCopy()
    return cc, cc.prepare(y)


def _search(st, cc, y, qs, T, C, edges=None, cls=None):
    """(hit mask [nq, n], thr, tau, E, taus8, exact [nq, n] float64) of queries qs (normalised rows) at thresholds T with C classes"""
    t, q8, e, nn = M.quant_queries(qs)
    edges = CM.class_edges(cc.e7, st.eps_max, C) if edges is None else edges
    thr, tau, E, taus8 = CM.thresholds(T, t, e, nn, edges)
    acc = CM.acc_units(st.c8, st.s, q8, len(y))
    exact = qs.astype(np.float64) @ y.astype(np.float64).T
    return CM.emitted_mask(acc, cc.cls if cls is None else cls, thr), thr, tau, E, taus8, exact


def _proof_edge(tau, E, taus8):
    """a row of class c that is not emitted has coarse < tau_c, so at most the float below it, and exact <= coarse + E_{q,c}: that
    must lie below taus8 + E_q. True where it does, per class and query."""
    worst = np.nextafter(tau, F32(-np.inf)).astype(np.float64) + E.astype(np.float64)
    return worst < (taus8.astype(np.float64) + E[-1].astype(np.float64))[None, :]


def test_edges_are_exact_order_statistics_and_classes_nest():
    rng = np.random.default_rng(3)
    for nb in (1, 2, 3, 7, 8, 9, 64, 1000, 4097):
        eps = rng.random(nb).astype(F32)
        eps[rng.integers(nb, size=nb // 3)] = eps[0]                       # ties
        e7 = CM.edges7(eps)
        s = np.sort(eps)
        for c in range(7):
            rank = int(np.ceil((1 - 2.0 ** -(c + 1)) * nb))                # 1-based, the issue's statement
            assert 1 <= rank <= nb and e7[c] == s[rank - 1]
            assert (eps <= e7[c]).sum() >= rank                           # at least that share of the blocks lies at or below the edge
        assert (np.diff(e7) >= 0).all()                                   # (with fewer blocks than classes: duplicate edges)
        cls = CM.classify(eps, e7)
        for b in range(nb):
            want = next((c for c in range(7) if eps[b] <= e7[c]), 7)
            assert cls[b] == want
            for C in (1, 2, 4, 8):                                        # the class a search with C classes uses, and what it charges
                assert eps[b] <= CM.class_edges(e7, s[-1], C)[min(cls[b], C - 1)]


def test_every_top_row_is_emitted_and_the_rest_stays_below_the_bound():
    rng = np.random.default_rng(5)
    fewer = 0
    for trial in range(9):
        kind = ("random", "embed", "adversarial")[trial % 3]
        qs = normalize(rng.standard_normal((8, D)))
        if kind == "adversarial":
            qs[0] = normalize(np.sign(rng.standard_normal((1, D))))[0]     # sits on its own grid: e_q ~ 0
        y, _ = _corpus(kind, rng, qs[0])
        cc, st = _state(y)
        exact = qs.astype(np.float64) @ y.astype(np.float64).T
        kth = np.sort(exact, axis=1)[:, -K]
        for drop in (0.0, 2e-3, 0.03):                                    # T at the k-th score, and below it as a sample leaves it
            T = (kth - drop).astype(F32)
            T = np.where(T.astype(np.float64) > kth, np.nextafter(T, F32(-np.inf)), T).astype(F32)
            hits = {}
            for C in (1, 2, 4, 8):
                hit, thr, tau, E, taus8, ex = _search(st, cc, y, qs, T, C)
                assert hit[ex >= T.astype(np.float64)[:, None]].all(), (kind, C, drop)
                bound = (taus8.astype(np.float64) + E[-1].astype(np.float64))[:, None]
                assert (ex[~hit] < np.broadcast_to(bound, ex.shape)[~hit]).all(), (kind, C, drop)
                assert _proof_edge(tau, E, taus8).all(), (kind, C, drop)
                hits[C] = hit
            one = _search(st, cc, y, qs, T, 1)[1:]
            # one class: today's threshold, E_q and tau_s, to the bit (test_i8_bound_model's statement of them)
            t, q8, e, nn = M.quant_queries(qs)
            Eq = M.e_q(e, nn, st.eps_max)
            assert (one[2][0] == Eq).all() and (one[3] == one[1][0]).all()
            for lo, hi in ((8, 4), (4, 2), (2, 1)):
                assert not (hits[lo] & ~hits[hi]).any(), (kind, lo, hi, drop)
            fewer += int(hits[8].sum() < hits[1].sum())
            print(kind, "drop", drop, "hits with 1 / 2 / 4 / 8 classes:", [int(hits[C].sum()) for C in (1, 2, 4, 8)])
    assert fewer >= 18                                                    # the classes do narrow the band


def _adversarial(seed, nb=NB):
    rng = np.random.default_rng(seed)
    q = normalize(np.sign(rng.standard_normal((1, D))))[0]
    y, zs = _corpus("adversarial", rng, q, nb=nb)
    return rng, q, y, zs


def _aligned(b):
    return 32 * b + 1


def test_adversarial_row_in_the_lowest_class_uses_half_its_bound():
    rng, q, y, zs = _adversarial(11)
    cc, st = _state(y)
    flat = [b for b in range(NB) if cc.cls[b] == 0]
    assert len(flat) == NB // 2
    used = 0.0
    for b in flat:
        r = _aligned(b)
        T = np.array([F32(np.float64(q) @ np.float64(y[r]))])
        T = np.where(T.astype(np.float64) > np.float64(q) @ np.float64(y[r]), np.nextafter(T, F32(-np.inf)), T).astype(F32)
        hit, thr, tau, E, taus8, ex = _search(st, cc, y, q[None, :], T, 8)
        coarse = M.coarse_scores(st.c8, st.s, *M.quant_queries(q[None, :])[:2], len(y))[0]
        gap = ex[0, r] - np.float64(coarse[r])
        assert 0 < gap <= E[0, 0]                                          # within its class's bound ...
        used = max(used, gap / np.float64(E[0, 0]))
        assert hit[0, r] and hit[0][ex[0] >= np.float64(T[0])].all()      # ... and emitted, like every row that reaches T
    assert used > 0.5, used


def _lost(st, cc, y, q, b, C=8, edges=None, cls=None):
    """is block b's aligned row — the row T is put at — missing from the hits?"""
    r = _aligned(b)
    x = np.float64(q) @ np.float64(y[r])
    T = np.array([F32(x)])
    T = np.where(T.astype(np.float64) > x, np.nextafter(T, F32(-np.inf)), T).astype(F32)
    hit = _search(st, cc, y, q[None, :], T, C, edges=edges, cls=cls)[0]
    return not hit[0, r]


def test_mistake_next_lower_edge_loses_a_row():
    rng, q, y, zs = _adversarial(13)
    cc, st = _state(y)
    true = CM.class_edges(cc.e7, st.eps_max, 8)
    wrong = np.concatenate([true[:1], true[:-1]]).astype(F32)             # class c charged edge[c - 1]
    lost = 0
    for c in range(1, 7):                                                 # (64 blocks: edge[6] is the largest eps_b, class 7 is empty)
        at_edge = [b for b in range(NB) if cc.cls[b] == c and cc.eps[b] == true[c]]
        assert at_edge
        assert not _lost(st, cc, y, q, at_edge[0])
        lost += _lost(st, cc, y, q, at_edge[0], edges=wrong)
    assert lost >= 4, lost


def test_mistake_edge_one_order_statistic_too_low_loses_a_row():
    rng, q, y, zs = _adversarial(17)
    cc, st = _state(y)
    s = np.sort(cc.eps)
    true = CM.class_edges(cc.e7, st.eps_max, 8)
    wrong = true.copy()
    for c in range(7):
        rank = NB - (NB >> (c + 1))
        assert s[rank - 1] == true[c]
        wrong[c] = s[rank - 2]                                            # blocks are classed by the right edges, charged the wrong ones
    lost = 0
    for c in range(7):
        b = int(np.flatnonzero(cc.eps == true[c])[0])
        assert cc.cls[b] == c and not _lost(st, cc, y, q, b)
        lost += _lost(st, cc, y, q, b, edges=wrong)
    assert lost >= 4, lost


def test_mistake_stale_top_edge_after_an_append_loses_a_row():
    rng, q, y, zs = _adversarial(19)
    n0 = 32 * 48 + 13                                                     # the first search ends inside block 48
    zs2 = zs.copy()
    zs2[60] = 0.6                                                         # an appended block above every edge and the old eps_max
    rng2 = np.random.default_rng(19)
    q2 = normalize(np.sign(rng2.standard_normal((1, D))))[0]
    y2, _ = _corpus("adversarial", rng2, q2, zs=zs2)
    assert (q2 == q).all()
    cc = CM.ClassCopy()
    st0 = cc.prepare(y2[:n0])
    e7 = cc.e7.copy()
    cc.appended(n0)
    st1 = cc.prepare(y2)
    assert (cc.e7 == e7).all()                                            # an append keeps the edges ...
    assert st1.eps_max > st0.eps_max and st1.eps_before == st0.eps_max and cc.eps[60] == st1.eps_max and cc.cls[60] == 7
    fresh = CM.ClassCopy()
    fresh.prepare(y2)
    assert (cc.eps == fresh.eps).all()                                    # ... re-quantises the partial block, and classifies the new ones
    assert all(cc.eps[b] <= CM.class_edges(e7, st1.eps_max, 8)[cc.cls[b]] for b in range(NB))
    assert not _lost(st1, cc, y2, q, 60)
    stale = CM.class_edges(e7, st1.eps_before, 8)                         # the top edge as it stood before the append
    assert _lost(st1, cc, y2, q, 60, edges=stale)


def test_mistake_taus8_left_at_the_top_class_fails_the_bound():
    """tau_c + E_{q,c} differs from class to class only by the roundings of thr_c, tau_c and E_{q,c}, but it does differ: with taus8
    left at tau_{C-1} the proof's edge row of some class reaches taus8 + E_q."""
    rng, q, y, zs = _adversarial(23)
    cc, st = _state(y)
    qs = normalize(rng.standard_normal((64, D)))
    t, q8, e, nn = M.quant_queries(qs)
    edges = CM.class_edges(cc.e7, st.eps_max, 8)
    broken = 0
    for T0 in np.linspace(0.05, 0.45, 41):
        T = np.full(len(qs), T0, F32)
        thr, tau, E, taus8 = CM.thresholds(T, t, e, nn, edges)
        assert _proof_edge(tau, E, taus8).all()
        assert (taus8 >= tau[-1]).all()
        broken += int((~_proof_edge(tau, E, tau[-1])).sum())
    assert broken > 0
