"""The bounds of tests/enc_reference.py have teeth (CPU, no GPU): numpy simulations of the encoder kernels' documented arithmetic
(fp32 where the headers say fp32, fp16 where they round) pass their bound on the inputs of tests/test_gpu_encoder_kernels.py, and
simulations with one plausible regression each fail it. Where the suite's earlier criterion (absolute 3e-3 for attention, 2e-3 of the
row scale for projections) would have accepted a regression, that is asserted too: it is the gap these bounds close."""
import numpy as np
import pytest

import enc_reference as R

F32, F16 = np.float32, np.float16


# ---- simulations ---------------------------------------------------------------------------------------------------------------

def sim_attention(q, k, v, scale, tile, p16, flush=False):
    """one (text, head): q [n][64], k / v [nk][64] fp16 -> fp16 [n][64]. Online soft-max over tiles of `tile` keys in fp32 (E1: 2,
    E12: 32, E5: all keys at once); p16: P rounded to fp16 before PV, the denominator from the fp32 values; flush: fp16 P below 2^-14
    becomes 0 (the regression)."""
    q32, k32, v32 = q.astype(F32), k.astype(F32), v.astype(F32)
    sl2 = F32(F32(scale) * F32(R.LOG2E))
    n, nk = q.shape[0], k.shape[0]
    m = np.full((n, 1), -np.inf, dtype=F32)
    l = np.zeros((n, 1), dtype=F32)
    o = np.zeros((n, 64), dtype=F32)
    for t0 in range(0, nk, tile):
        s = (q32 @ k32[t0:t0 + tile].T) * sl2
        mn = np.maximum(m, s.max(axis=1, keepdims=True))
        corr = np.exp2(m - mn).astype(F32)
        p = np.exp2(s - mn).astype(F32)
        pv = p
        if p16:
            pv = p.astype(F16)
            if flush:
                pv = np.where(np.abs(pv) < F16(2.0 ** -14), F16(0), pv)
            pv = pv.astype(F32)
        l = (l * corr + p.sum(axis=1, keepdims=True, dtype=F32)).astype(F32)
        o = (o * corr + pv @ v32[t0:t0 + tile]).astype(F32)
        m = mn
    return (o * (F32(1) / l)).astype(F16)


def sim_packed(qkv, texts, heads, scale, tile, p16, keys=None, flush=False):
    """all texts and heads; keys(i, f, n) -> the key indices text i attends to (default: its own)"""
    T = qkv.shape[0]
    x = qkv.reshape(T, 3, heads, 64)
    out = np.full((T, heads * 64), np.nan)
    for i, (f, n) in enumerate(texts):
        ks = np.arange(f, f + n) if keys is None else keys(i, f, n)
        for h in range(heads):
            out[f:f + n, h * 64:(h + 1) * 64] = sim_attention(x[f:f + n, 0, h], x[ks, 1, h], x[ks, 2, h], scale, tile, p16, flush)
    return out


def sim_linear(x, w, b, partial16=False, waves=16, gelu=False):
    """E3 / E4: waves split K, each accumulates its slice in fp32; the partial tiles are added to the bias in wave order in fp32 (the
    regression: the partial tiles rounded to fp16 and added in fp16); fp16 out"""
    K = x.shape[1]
    ks = K // waves
    parts = [x[:, i * ks:(i + 1) * ks].astype(F32) @ w[:, i * ks:(i + 1) * ks].astype(F32).T for i in range(waves)]
    if partial16:
        v = np.broadcast_to(b.astype(F16), parts[0].shape)
        for p in parts:
            v = (v + p.astype(F16)).astype(F16)
        return v
    v = np.broadcast_to(b.astype(F32), parts[0].shape)
    for p in parts:
        v = (v + p).astype(F32)
    if gelu:
        v = R.gelu64(v.astype(np.float64)).astype(F32)      # erff in fp32: a few ulps, inside the GELU term of the bound
    return v.astype(F16)


def sim_layernorm(x, g, b, eps, one_pass=False):
    """E2 / E4 prologue / E7: one wave per row, lane l holds elements c 512 + 8 l + e, sums lane-sequential then a butterfly; two
    passes (the regression: one pass, var = E[x^2] - mean^2)"""
    rows, hid = x.shape
    nch = hid // 512
    x32 = x.astype(F32).reshape(rows, nch, 64, 8)

    def wave_sum(vals):                      # [rows][nch][64][8] -> [rows] fp32
        lane = np.zeros((rows, 64), dtype=F32)
        for c in range(nch):
            for e in range(8):
                lane = (lane + vals[:, c, :, e]).astype(F32)
        for d in (32, 16, 8, 4, 2, 1):
            lane = (lane + lane[:, np.arange(64) ^ d]).astype(F32)
        return lane[:, 0]
    inv = F32(1.0 / hid)
    mean = (wave_sum(x32) * inv).astype(F32)[:, None, None, None]
    if one_pass:
        var = (wave_sum(x32 * x32) * inv - mean[:, 0, 0, 0] * mean[:, 0, 0, 0]).astype(F32)
    else:
        d = (x32 - mean).astype(F32)
        var = (wave_sum(d * d) * inv).astype(F32)
    rstd = (F32(1) / np.sqrt(var + F32(eps))).astype(F32)[:, None, None, None]
    y = ((x32 - mean) * rstd * g.astype(F32).reshape(nch, 64, 8) + b.astype(F32).reshape(nch, 64, 8)).astype(F16)
    return y.reshape(rows, hid)


def fails(got, ref, bnd):
    with pytest.raises(AssertionError):
        R.check(got, ref, bnd)


# ---- inputs (the GPU file's) --------------------------------------------------------------------------------------------------

LENS = [33, 1025, 1500]


def packed(lens):
    first = np.cumsum(lens) - np.asarray(lens)
    return [(int(f), int(n)) for f, n in zip(first, lens)]


def hot_probe(lens, heads, hot):
    """q = 0 (every weight exactly 1 / len); V zero but one hot key per (text, head) whose value row carries the text's channel
    (text % 64) and a head constant"""
    texts = packed(lens)
    T = sum(lens)
    qkv = np.zeros((T, 3, heads, 64), dtype=F16)
    for i, (f, n) in enumerate(texts):
        for h in range(heads):
            qkv[f + hot(i, n, h), 2, h, i % 64] = F16(1.0 + h / 16)
    return qkv.reshape(T, -1), texts


def sink_probe(lens, heads, rng=None):
    """key 0 of every text 12 nats above the others (q = 4 e_0, k_0 = 24 e_0, scale 1/8), v_0 = 0; the other values +1 in channel
    1 (rng None) or random: the output is carried by probabilities of e^-12 ~ 2^-17.3, fp16 subnormals"""
    texts = packed(lens)
    T = sum(lens)
    qkv = np.zeros((T, 3, heads, 64), dtype=F16)
    qkv[:, 0, :, 0] = 4
    for f, n in texts:
        qkv[f, 1, :, 0] = 24
        if rng is None:
            qkv[f + 1:f + n, 2, :, 1] = 1
        else:
            qkv[f + 1:f + n, 2] = (rng.standard_normal((n - 1, heads, 64)) * 1.5).astype(F16)
    return qkv.reshape(T, -1), texts


# ---- attention ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name, tile, p16, steps", [("E1", 2, False, R.e1_steps), ("E12", 32, True, R.e12_steps)])
def test_attention_bound_accepts_the_kernel_and_rejects_wrong_keys(name, tile, p16, steps):
    heads = 2
    qkv, texts = hot_probe(LENS, heads, lambda i, n, h: (n - 1 - 7 * h) if i % 2 else (17 + 9 * h) % n)
    ref, bnd = R.attention_packed(qkv, texts, heads, 0.125, p16=p16, steps=steps)
    R.check(sim_packed(qkv, texts, heads, 0.125, tile, p16), ref, bnd, name)
    hot = {}
    for i, (f, n) in enumerate(texts):
        hot[i] = f + ((n - 1) if i % 2 else 17)                  # head 0's hot key
    drop = lambda i, f, n: np.setdiff1d(np.arange(f, f + n), [hot[i]])
    twice = lambda i, f, n: np.concatenate([np.arange(f, f + n), [hot[i]]])
    neigh = lambda i, f, n: np.concatenate([np.arange(f, f + n), [hot[(i + 1) % len(texts)]]])
    for keys in (drop, twice, neigh):
        bad = sim_packed(qkv, texts, heads, 0.125, tile, p16, keys=keys)
        for f, n in texts:                                       # every text of 33, 1025 and 1500 tokens on its own
            fails(bad[f:f + n], ref[f:f + n], bnd[f:f + n])


def test_attention_bound_rejects_flushed_fp16_probabilities():
    heads = 2
    for lens in ([33], [1025], [1500], LENS):
        qkv, texts = sink_probe(lens, heads)
        ref, bnd = R.attention_packed(qkv, texts, heads, 0.125, p16=True, steps=R.e12_steps)
        R.check(sim_packed(qkv, texts, heads, 0.125, 32, True), ref, bnd, "E12 sink")
        fails(sim_packed(qkv, texts, heads, 0.125, 32, True, flush=True), ref, bnd)
    # E5 (<= 32 tokens, one tile): the same
    qkv, texts = sink_probe([32], heads)
    ref, bnd = R.attention_packed(qkv, texts, heads, 0.125, p16=True, steps=R.e5_steps)
    R.check(sim_packed(qkv, texts, heads, 0.125, 32, True), ref, bnd, "E5 sink")
    fails(sim_packed(qkv, texts, heads, 0.125, 32, True, flush=True), ref, bnd)


def test_flushed_probabilities_passed_the_old_criterion():
    """a sink with random values: flushing moves the output by less than the old absolute 3e-3, the new bound rejects it"""
    heads = 2
    qkv, texts = sink_probe([1500], heads, np.random.default_rng(1))
    ref, bnd = R.attention_packed(qkv, texts, heads, 0.125, p16=True, steps=R.e12_steps)
    good = sim_packed(qkv, texts, heads, 0.125, 32, True)
    bad = sim_packed(qkv, texts, heads, 0.125, 32, True, flush=True)
    R.check(good, ref, bnd)
    fails(bad, ref, bnd)
    assert 1e-4 < np.abs(bad - ref).max() <= 3e-3


def test_attention_bound_accepts_random_inputs():
    rng = np.random.default_rng(2)
    heads = 2
    lens = [1, 33, 64, 65, 300]
    texts = packed(lens)
    qkv = (rng.standard_normal((sum(lens), 3 * heads * 64)) * 1.5).astype(F16)
    for tile, p16, steps in ((2, False, R.e1_steps), (32, True, R.e12_steps)):
        ref, bnd = R.attention_packed(qkv, texts, heads, 0.125, p16=p16, steps=steps)
        R.check(sim_packed(qkv, texts, heads, 0.125, tile, p16), ref, bnd)


# ---- projections ----------------------------------------------------------------------------------------------------------------

def test_projection_bound_rejects_fp16_partial_tiles():
    rng = np.random.default_rng(3)
    T, N, K = 32, 1024, 4096
    x = rng.standard_normal((T, K)).astype(F16)
    w = (rng.standard_normal((N, K)) * K ** -0.5).astype(F16)
    b = (rng.standard_normal(N) * 0.1).astype(F16)
    ref, bnd = R.linear(x, w, b)
    R.check(sim_linear(x, w, b), ref, bnd, "E4")
    bad = sim_linear(x, w, b, partial16=True)
    fails(bad, ref, bnd)
    want32 = x.astype(F32) @ w.astype(F32).T + b.astype(F32)            # the old criterion (fp32 torch reference) accepts it
    assert np.abs(bad - want32).max() <= 2e-3 * max(1.0, np.abs(want32).max())


def test_projection_bound_on_cancelling_rows_and_outlier_columns():
    rng = np.random.default_rng(4)
    T, N, K = 17, 64, 1024
    x = rng.standard_normal((T, K))
    x[:, 5] *= 100                                                       # an outlier input column
    w = rng.standard_normal((N, K)) * K ** -0.5
    x[3] = np.concatenate([x[3, :K // 2], x[3, :K // 2]])                # a cancelling row: w's two halves opposite
    w[:, K // 2:] = -w[:, :K // 2]
    x, w = x.astype(F16), w.astype(F16)
    b = np.zeros(N, dtype=F16)
    for epi in (0, 1):
        ref, bnd = R.linear(x, w, b, epi=epi)
        R.check(sim_linear(x, w, b, gelu=bool(epi)), ref, bnd)
    assert np.abs(ref[3]).max() == 0.0                                   # cancelling row: exactly 0, whatever the order
    fails(sim_linear(x, w, b, partial16=True), *R.linear(x, w, b))


# ---- LayerNorm ------------------------------------------------------------------------------------------------------------------

def test_layernorm_bound_rejects_one_pass_variance():
    rng = np.random.default_rng(5)
    for hid in (512, 1024, 1536, 2048):
        x = (500 + rng.standard_normal((16, hid))).astype(F16)
        x[8:] = (-500 + rng.standard_normal((8, hid))).astype(F16)
        g = (rng.standard_normal(hid) * 0.3 + 1).astype(F16)
        b = (rng.standard_normal(hid) * 0.2).astype(F16)
        ref, bnd = R.layernorm(x, g, b, 1e-5)
        R.check(sim_layernorm(x, g, b, 1e-5), ref, bnd, f"LN {hid}")
        fails(sim_layernorm(x, g, b, 1e-5, one_pass=True), ref, bnd)


def test_layernorm_bound_on_outliers_constant_rows_and_tiny_variance():
    rng = np.random.default_rng(6)
    hid = 1024
    x = rng.standard_normal((6, hid))
    x[0, [7, 300]] = [3e4, -2.5e4]                                       # outlier features
    x[1] = 123.5                                                         # constant row -> beta exactly
    x[2] = 1 + rng.integers(-2, 3, hid) * 2.0 ** -10                     # variance ~ 1e-6, far below eps
    x[3] = -500 + x[3]
    x = x.astype(F16)
    g = (rng.standard_normal(hid) * 0.3 + 1).astype(F16)
    b = (rng.standard_normal(hid) * 0.2).astype(F16)
    ref, bnd = R.layernorm(x, g, b, 1e-5)
    got = sim_layernorm(x, g, b, 1e-5)
    R.check(got, ref, bnd)
    assert np.array_equal(got[1], b)
