"""A numpy restatement of the reranker head (k_rerank_head + k_rerank_combine) and of the selection's order (K_R3), written from the
comment block of rag_dpo_amd/csrc/rerank_kernel.hpp and independent of the product code (which never imports it).

reference()     the head in fp64 and the derived worst-case bound on |kernel score - fp64 score| (any inputs)
kernel_order()  the scores of the documented order of operations, and of named mutants of it: what a plausible regression computes
exact_probe()   inputs on a grid on which every partial sum of that order is exact in fp32, so that z is the fp64 value in ANY correct
                order and the bound collapses to tight_reference()'s: the one fp32 rounding of the score plus the fp64 tail
select_model()  the selection's order with NaN finals stated independently of the kernel and of reranker.select_host

One rounding per fma is modelled as an fp64 multiply-add rounded to fp32. The product (11 x 24 bits) is exact in fp64; the sum is
rounded twice (fp64, then fp32), which differs from the single rounding only where the fp64 sum lands on an fp32 tie: never on
exact_probe's grid (nothing rounds there), and one ulp of one partial sum elsewhere, which both bounds hold with room."""
import numpy as np

U32 = 2.0 ** -24
MUTANTS = ("fp16_acc", "fp16_lanes", "drop_round", "swap_features", "pair_rows", "skip_bd")
FEATURES, ROWS_PER_BLOCK, KU = 8, 64, 16                                     # RERANK_FEATURES, RERANK_ROWS_PER_BLOCK, RERANK_KU
SWAP = (2, 5)                                                                # swap_features: these two w_o entries of the LAST feature block
GRID = 2.0 ** -10                                                            # exact_probe: every product and partial sum is a multiple of it


def _f64(t):
    """torch tensor (any device) or array -> numpy fp64 (exact for fp16 and fp32 inputs)"""
    if hasattr(t, "detach"):
        return t.detach().double().cpu().numpy()
    return np.asarray(t, dtype=np.float64)


def reference(cls, wd, bd, wo, bo):
    """fp64 of the fp16 weights: (score, the derived bound on |kernel score - score|)"""
    h = _f64(cls)
    W_, b_, w_, c_ = (_f64(t) for t in (wd, bd, wo, bo))
    H = h.shape[1]
    z = h @ W_.T + b_
    logit = np.tanh(z) @ w_ + c_[0]
    score = 1.0 / (1.0 + np.exp(-logit))
    # z: per lane an fma chain of H / 64 terms, then a 6-level butterfly, then + b_d: m = H / 64 + 7 roundings of partial sums
    m = H // 64 + 7
    gamma = m * U32 / (1 - m * U32)
    dz = gamma * (np.abs(h) @ np.abs(W_).T) + gamma * np.abs(b_)
    # tanh is 1-Lipschitz; the rest is fp64 (tanh, the products and at most H / 8 + 7 sums): 1e-12 relative covers it
    dlogit = dz @ np.abs(w_) + 1e-12 * (np.abs(np.tanh(z)) @ np.abs(w_) + abs(c_[0]))
    bound = dlogit / 4 + U32 * score + 1e-15                                               # sigmoid is 1/4-Lipschitz; one fp32 rounding
    return score, bound


def random_head(H, seed, scale=3.0):
    """the random head of the GPU tests (LayerNorm-scale inputs, 1 / sqrt(H) weights) as CPU torch tensors: W_d, b_d, w_o, b_o in fp16"""
    import torch
    g = torch.Generator().manual_seed(seed)
    wd = (torch.randn(H, H, generator=g) / H ** 0.5).half()
    bd = (torch.randn(H, generator=g) * 0.1).half()
    wo = (torch.randn(H, generator=g) * scale / H ** 0.5).half()
    bo = (torch.randn(1, generator=g) * 0.5).half()
    return wd, bd, wo, bo


def random_rows(H, ns):
    """the GPU tests' random cls rows: one generator per H, (n, cls fp32 [n][H]) for every n of ns in turn"""
    import torch
    g = torch.Generator().manual_seed(H + 1)
    for n in ns:
        yield n, torch.randn(n, H, generator=g)                             # LayerNorm output scale


def tight_reference(cls, wd, bd, wo, bo):
    """(fp64 score, tight): the bound for inputs whose z is exact in fp32 in every summation order (exact_probe's): the score's one
    rounding to fp32 and the fp64 tail (tanh, H products, H + H / 8 + 7 sums, exp, a division: 1e-12 relative to the logit's terms)"""
    h = _f64(cls)
    W_, b_, w_, c_ = (_f64(t) for t in (wd, bd, wo, bo))
    z = h @ W_.T + b_
    t = np.tanh(z)
    score = 1.0 / (1.0 + np.exp(-(t @ w_ + c_[0])))
    return score, U32 * score + 1e-12 * (np.abs(t) @ np.abs(w_) + abs(c_[0])) / 4 + 1e-15


def _butterfly(a, rnd):
    """a[..., 64]: a[l] += a[l ^ m] for m = 32 .. 1, every sum rounded by rnd; every lane then holds the same value"""
    lanes = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        a = rnd(a + a[..., lanes ^ m])
        yield a


def _dense(x, W, b, mutant=None, rnd32=None, seen=None):
    """z [n][H] of the documented order as fp64 values, every partial sum rounded by rnd32 (None: fp32) and shown to seen()"""
    n, H = x.shape
    f32 = (lambda a: a.astype(np.float32).astype(np.float64)) if rnd32 is None else rnd32
    with np.errstate(over="ignore", invalid="ignore"):
        f16 = lambda a: a.astype(np.float16).astype(np.float64)              # noqa: E731
        rnd = (lambda a: f16(f32(a))) if mutant in ("fp16_acc", "fp16_lanes") else f32   # fp16_lanes: the lane sums only, the butterfly in fp32
        if mutant == "pair_rows":                                            # x1 = x0: the odd row of every row pair reads the even row's cls
            x = x.copy()
            x[1::2] = x[0:2 * (n // 2):2]                                    # (row blocks hold 64 rows: local and global parity agree)
        rounds = H // 64
        live = np.ones(rounds, dtype=bool)
        if mutant == "drop_round":                                           # the k0 loop stops after its first pass / one step early
            live[KU if H > 64 * KU else rounds - 1:] = False
        xr, Wr = x.reshape(n, rounds, 64), np.ascontiguousarray(W.reshape(H, rounds, 64).transpose(1, 0, 2))
        z = np.empty((n, H))
        step = max(1, (1 << 21) // (64 * H))                                 # rows at a time: 2 M accumulators
        for r0 in range(0, n, step):
            acc = np.zeros((min(step, n - r0), H, 64))
            for j in range(rounds):                                          # lane l: k = l, l + 64, ... one fma each
                if not live[j]:
                    continue
                acc = rnd(acc + Wr[j][None] * xr[r0:r0 + step, None, j, :])
                if seen:
                    seen(acc)
            for acc in _butterfly(acc, f32 if mutant == "fp16_lanes" else rnd):
                if seen:
                    seen(acc)
            z[r0:r0 + step] = acc[:, :, 0] if mutant == "skip_bd" else f32(acc[:, :, 0] + b[None, :])   # + (float)b_d: one fp32 add
        if seen:
            seen(z)
    return z


def kernel_order(cls, wd, bd, wo, bo, mutant=None):
    """fp32 scores [n] of the documented order; mutant: None or one of MUTANTS"""
    assert mutant is None or mutant in MUTANTS, mutant
    x, W, b, w, c = (_f64(t) for t in (cls, wd, bd, wo, bo))
    n, H = x.shape
    assert H % 64 == 0 and W.shape == (H, H)
    z = _dense(x, W, b, mutant)
    if mutant == "swap_features":
        w = w.copy()
        i, j = H - FEATURES + SWAP[0], H - FEATURES + SWAP[1]
        w[i], w[j] = w[j], w[i]
    blocks = H // FEATURES
    with np.errstate(over="ignore", invalid="ignore"):
        t = np.tanh(z).reshape(n, blocks, FEATURES) * w.reshape(1, blocks, FEATURES)
        part = np.zeros((n, blocks))
        for f in range(FEATURES):                                            # p = 0.0; p += w_o[f] * tanh(z_f), f ascending
            part = part + t[:, :, f]
        lanes = np.zeros((n, 64))
        for b0 in range(0, blocks, 64):                                      # lane l: blocks l, l + 64, ...
            m = min(64, blocks - b0)
            lanes[:, :m] = lanes[:, :m] + part[:, b0:b0 + m]
        for lanes in _butterfly(lanes, lambda a: a):
            pass
        s = lanes[:, 0] + c[0]
        return (1.0 / (1.0 + np.exp(-s))).astype(np.float32)


def significant_bits(values, grid=GRID):
    """the largest number of significant bits among values that are whole multiples of grid (asserted)"""
    q = np.abs(np.asarray(values, dtype=np.float64)) / grid
    m = q.astype(np.int64)
    assert np.array_equal(m.astype(np.float64), q), "a value off the grid"
    m = m[m != 0]
    if m.size == 0:
        return 0
    low = m & -m
    return int((np.floor(np.log2(m.astype(np.float64))) - np.log2(low.astype(np.float64)) + 1).max())


def carrier_columns(H):
    """exact_probe's cancelling pairs (k, k'): the same lane in two k-rounds (H >= 128 only), partner lanes (k' = k ^ 32: they meet
    in the butterfly's first step), unrelated lanes (18 and 51 meet in its LAST step, after 31 other lanes joined each)"""
    pairs = [(9, 9 ^ 32), (18, 51 + (64 if H >= 128 else 0))]
    if H >= 128:
        pairs.append((5, 5 + 64 * (H // 64 - 1)))
    cols = [k for p in pairs for k in p]
    assert len(set(cols)) == len(cols) and max(cols) < H
    return pairs


def exact_probe(H, n, seed):
    """-> (cls fp32 [n][H], W_d fp16 [H][H], b_d fp16 [H], w_o fp16 [H], b_o fp16 [1]) as numpy arrays.
    cls in multiples of 2^-4 (|cls| <= 2), W_d in multiples of 2^-6 (|W_d| <= 1/8, about 128 non-zeros a row: z has unit scale), b_d in
    multiples of 2^-6: every product and every partial sum is a multiple of 2^-10 below 2^14, so exact in fp32 in any order.
    Carrier pairs (carrier_columns) share a dense W_d column of up to 7 bits and hold +C and -C (C in [64, 100), 11 bits) in cls:
    they cancel in z, and until they do the partial sums need up to 18 bits, which fp32 holds and fp16 does not."""
    assert H % 64 == 0 and n >= 1
    rng = np.random.default_rng([H, n, seed])
    keep = rng.uniform(size=(H, H)) < min(1.0, 128.0 / H)
    W = rng.integers(-8, 9, (H, H)) / 64.0 * keep
    x = rng.integers(-32, 33, (n, H)) / 16.0
    for k, k2 in carrier_columns(H):
        col = rng.integers(1, 65, H) * rng.choice([-1, 1], H) / 64.0
        W[:, k] = W[:, k2] = col
        C = (2 * rng.integers(512, 800, n) + 1) / 16.0                       # odd numerators: all 11 bits in use
        x[:, k], x[:, k2] = C, -C
    b = rng.integers(-16, 17, H) / 64.0
    w_o = (rng.standard_normal(H) * 3.0 / H ** 0.5).astype(np.float16)
    i, j = H - FEATURES + SWAP[0], H - FEATURES + SWAP[1]
    w_o[i], w_o[j] = np.float16(0.75), np.float16(-0.5)                      # what swap_features exchanges differs
    b_o = (rng.standard_normal(1) * 0.5).astype(np.float16)
    out = (x.astype(np.float32), W.astype(np.float16), b.astype(np.float16), w_o, b_o)
    assert np.array_equal(out[0], x) and np.array_equal(out[1].astype(np.float64), W) and np.array_equal(out[2].astype(np.float64), b)
    # exact in fp32: the sum of magnitudes, in units of the grid, stays below 2^24 (all rows)
    assert float((np.abs(x) @ np.abs(W).T + np.abs(b)).max()) / GRID < 2.0 ** 24
    # and fp16 would not do: on the way some partial sum of the kernel's order needs more than 11 bits (row 0 is shown; every row is built alike)
    bits = []
    z = _dense(x[:1], W, b, rnd32=lambda a: a, seen=lambda a: bits.append(significant_bits(a)))
    assert 11 < max(bits) <= 24, max(bits)
    assert np.array_equal(z, x[:1] @ W.T + b)                                # nothing rounded: the fp64 matmul gives the same z
    return out


def select_model(scores, boosts, top_k, min_score, keep_min):
    """-> (order, final, count) as rerank_kernel.hpp states them: final = (double)score (+ boost where boost > 0.0: false for NaN);
    a number comes before NaN, numbers descend, equal finals (+0.0 and -0.0 are equal) and NaN among themselves keep input order;
    count = min(top_k, #{final >= min_score}), lifted to keep_min when it is below and n >= keep_min"""
    final = [float(np.float32(s)) for s in scores]
    if boosts is not None:
        for i, b in enumerate(boosts):
            if float(b) > 0.0:
                final[i] = final[i] + float(b)
    n = len(final)
    numbers = [i for i in range(n) if final[i] == final[i]]
    order = sorted(numbers, key=lambda i: -final[i])                         # NaN-free: a total preorder, and the sort is stable
    order += [i for i in range(n) if final[i] != final[i]]
    count = min(top_k, sum(1 for f in final if f >= min_score))
    if count < keep_min and n >= keep_min:
        count = keep_min
    return order, final, count
