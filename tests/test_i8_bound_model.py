"""CPU model of the int8 coarse pass (DESIGN.md §5 "int8 coarse pass"): block-scaled quantisation of the corpus (one scale per
32-row block), per-query quantisation, the exact int32 dot product D, the coarse score (float)D * s_b * t_q and the bound
E_q,b = e_q (1 + 1e-6) + n_q eps_b + 1e-6. The bound must hold on random, embedding-like and adversarial rows, the adversarial
rows must use a stated part of it, and the emit threshold must never drop a row whose upper bound reaches T."""
import numpy as np

F32 = np.float32


def quant_rows(y):
    """y: [32, d] float32 block -> (s_b, c8, eps_b) as k_quant8_corpus computes them"""
    mx = F32(np.abs(y).max())
    s = F32(mx / F32(127))
    inv = F32(1) / s if mx > 0 else F32(0)
    c8 = np.clip(np.rint(y * inv), -127, 127).astype(np.int8)
    err = y.astype(np.float64) - np.float64(s) * c8.astype(np.float64)
    eps = np.sqrt((err * err).sum(axis=1).max()) * (1 + 1e-12)
    return s, c8, F32(np.nextafter(F32(eps), F32(np.inf)))


def quant_query(q):
    mx = F32(np.abs(q).max())
    t = F32(mx / F32(127)) if mx > 0 else F32(1)
    inv = F32(1) / t if mx > 0 else F32(0)
    q8 = np.clip(np.rint(q * inv), -127, 127).astype(np.int8)
    a = np.float64(t) * q8.astype(np.float64)
    e = np.sqrt(((q.astype(np.float64) - a) ** 2).sum()) * (1 + 1e-12)
    n = np.sqrt((a * a).sum()) * (1 + 1e-12)
    return t, q8, F32(np.nextafter(F32(e), F32(np.inf))), F32(np.nextafter(F32(n), F32(np.inf)))


def normalize(x):
    x = x.astype(np.float32)
    den = np.maximum(np.sqrt((x.astype(np.float64) ** 2).sum(axis=1)), 1e-12)
    return (x.astype(np.float64) / den[:, None]).astype(np.float32)


def coarse_and_bound(qn, block):
    s, c8, eps = quant_rows(block)
    t, q8, e, n = quant_query(qn)
    D = c8.astype(np.int64) @ q8.astype(np.int64)
    assert np.abs(D).max() < 2 ** 24
    coarse = ((D.astype(F32) * s).astype(F32) * t).astype(F32)
    exact = (block.astype(np.float64) @ qn.astype(np.float64)).astype(F32)
    E = np.float64(e) * (1 + 1e-6) + np.float64(n) * np.float64(eps) + 1e-6
    return coarse, exact, E, (t, s)


def test_bound_holds_on_random_embedlike_and_adversarial_rows():
    rng = np.random.default_rng(0)
    d = 1024
    worst = 0.0
    for trial in range(40):
        q = normalize(rng.standard_normal((1, d)))[0]
        kind = trial % 3
        if kind == 0:
            block = normalize(rng.standard_normal((32, d)))
        elif kind == 1:                                  # embedding-like: a shared mean direction, a document's chunks
            mu = rng.standard_normal(d)
            block = normalize(mu + 0.3 * rng.standard_normal((32, d)))
        else:                                            # adversarial: every row's rounding error aligned with the query
            base = normalize(rng.standard_normal((32, d)))
            s = np.abs(base).max() / 127
            grid = np.rint(base / s) * s
            block = normalize(grid + 0.49 * s * np.sign(q)[None, :] * (np.abs(base) < 126 * s))
        coarse, exact, E, _ = coarse_and_bound(q, block)
        r = np.abs(coarse.astype(np.float64) - exact.astype(np.float64)) / E
        assert r.max() <= 1.0, (kind, r.max())
        if kind == 2:
            worst = max(worst, r.max())
    assert worst > 0.25, worst                           # the adversarial rows use a quarter of E and more: the bound is not vacuous


def test_threshold_rounding_never_drops_a_row():
    """thr = (T - E) / t_q rounded down; a row is emitted iff (float)D * s_b >= thr. Every row whose coarse + E reaches T (and so
    every row whose exact score reaches T) must be emitted."""
    rng = np.random.default_rng(1)
    d = 256
    for _ in range(20):
        q = normalize(rng.standard_normal((1, d)))[0]
        block = normalize(rng.standard_normal((32, d)) + 2 * q[None, :] * rng.random((32, 1)))
        coarse, exact, E, (t, s) = coarse_and_bound(q, block)
        s_b, c8, _ = quant_rows(block)
        _, q8, _, _ = quant_query(q)
        acc = (c8.astype(np.int64) @ q8.astype(np.int64)).astype(F32) * s_b
        for T in np.sort(exact)[::4]:
            Ef = F32(np.nextafter(F32(E), F32(np.inf)))
            thr = F32((np.float64(T) - np.float64(Ef)) / np.float64(t))
            if np.float64(thr) * np.float64(t) > np.float64(T) - np.float64(Ef):
                thr = np.nextafter(thr, F32(-np.inf))
            emitted = acc >= thr
            assert emitted[exact >= T].all()
            assert emitted[coarse.astype(np.float64) + E >= np.float64(T) + 1e-6].all()
