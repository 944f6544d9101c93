"""TEST-ONLY: float64 references of the encoder kernels and per-element error bounds.

Every reference is computed in numpy float64 from the SAME fp16 values the kernel reads (qkv, activations, weights, gamma / beta),
so the only differences left are the kernel's own roundings. Every bound is the sum of terms, each tied to one operation the kernels'
headers (rag_dpo_amd/csrc/enc_kernels.hpp, enc_small.hpp) document; nothing here is fitted to a measured error.

    ROUND16   the final rounding to fp16: half an fp16 ulp of |ref| + (the other terms), subnormal spacing 2^-24 included.
    ACC32     fp32 accumulation of a long dot product (the MFMA chains of E3 / E4 / E5 / E12, E1's fma_mix chain, the partial tiles
              added in wave order): ACC32_REL * sum|terms|. The size is the MFMA-versus-fp64 error of a k-ordered fp32 chain at
              K <= 4096 (cdna_hip_programming.md §3, "FP32-input MFMA": 0.75 - 1.5e-7 at K <= 1024, 3.5e-7 at K = 4096), rounded up.
    SCORE     the attention scores: 64 exact fp16 products summed in fp32 (at most 64 roundings: 64 u sum|q k|), the scale
              multiply, the max subtraction (u each) and exp2 (2^-22 relative), plus one 2^-22 per running-max rescale that
              the online soft-max applies to everything before it. A relative error e_j of key j's weight moves the output by at most
              sum_j p_j e_j (|v_j| + |o|) / sum p.
    P16       E5 / E12 round the probabilities to fp16 before the PV product while the denominator sums the fp32 values: per key at
              most 2^-11 p_j (normal range) + 2^-25 (the subnormal spacing's half, p in units of the running maximum <= 1), i.e.
              sum_j (2^-11 p_j + 2^-25) |v_j| / sum p.  A kernel that flushed fp16 subnormals to zero would lose up to 2^-14 per key.
    LNSTAT    LayerNorm's fp32 statistics (E2, E4 prologue, E7: two passes, one wave per row: a lane adds its 8 * NCH values, a
              64-lane butterfly adds the lanes, so every value passes through at most 8 NCH + 6 additions): the mean is off by
              at most (8 NCH + 7) u mean|x|, the centred sum of squares by (8 NCH + 9) u sum d^2 (+ hidden * dmean^2: it is taken
              around the computed mean), rsqrt by 2^-22; each output element then by dmean rstd |g| + |d| rstd |g| (drstd + 3u) + u |b|.
"""
import numpy as np

U32 = 2.0 ** -24                 # unit roundoff of fp32
ACC32_REL = 4e-7                 # fp32 accumulation, relative to sum|terms| (see ACC32 above)
EXP2_REL = 2.0 ** -22            # v_exp_f32 / v_rcp_f32 / v_rsq_f32: about one fp32 ulp
LOG2E = 1.4426950408889634


def f16(a):
    return np.asarray(a, dtype=np.float16)


def ulp16(a):
    """spacing of fp16 numbers at |a| (2^-24 in the subnormal range)"""
    a = np.abs(np.asarray(a, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -14)))
    return 2.0 ** (e - 10)


def round16_bound(ref, other):
    """the final fp16 rounding of a value within `other` of `ref`"""
    return other + 0.5 * ulp16(np.abs(ref) + other)


# ---- attention (E1, E5, E12) -------------------------------------------------------------------------------------------------------

def split_qkv(qkv, heads):
    """qkv [T][3 heads 64] (fp16) -> q, k, v as float64 [heads][T][64]"""
    T = qkv.shape[0]
    x = np.asarray(qkv, dtype=np.float64).reshape(T, 3, heads, 64)
    return (x[:, i].transpose(1, 0, 2) for i in range(3))


def attention_text(q, k, v, scale, p16=False, steps=1):
    """one text, all heads at once: q, k, v float64 [heads][len][64] -> (ref, bound) [heads][len][64].
    p16: the kernel rounds P to fp16 before PV (E5, E12). steps: how many running-max rescales the kernel may apply to a row
    (E1: one per two keys, E12: one per 32-key tile, E5: none)."""
    s = q @ k.transpose(0, 2, 1) * scale                                    # nats
    a = np.abs(q) @ np.abs(k).transpose(0, 2, 1) * scale                    # sum |q k| scale
    m = s.max(axis=2, keepdims=True)
    p = np.exp(s - m)                                                       # final units: the largest weight is 1
    l = p.sum(axis=2, keepdims=True)
    o = p @ v / l
    av = np.abs(v)
    pav = p @ av / l                         # sum p |v| / sum p
    # SCORE: relative error of each weight (log2 units -> ln 2 per unit)
    s2, m2 = np.abs(s) * LOG2E, np.abs(m) * LOG2E
    ds2 = LOG2E * 64 * U32 * a + 4 * U32 * (s2 + m2)
    eps = np.log(2.0) * ds2 + EXP2_REL * (1 + steps)
    pe = p * eps
    score = 1.01 * (pe @ av + pe.sum(axis=2, keepdims=True) * np.abs(o)) / l
    other = score + ACC32_REL * (pav + np.abs(o)) + EXP2_REL * np.abs(o)
    if p16:
        other = other + (2.0 ** -11 * (p @ av) + 2.0 ** -25 * av.sum(axis=1)[:, None, :]) / l
    return o, round16_bound(o, other)


def attention_packed(qkv, texts, heads, scale, p16=False, steps=None):
    """packed layout: texts = [(first token, length)]; -> (ref, bound) float64 [T][heads 64], NaN on rows of no listed text.
    steps(length) -> rescale count (default: E1's, one per two keys)."""
    q, k, v = split_qkv(qkv, heads)
    T = qkv.shape[0]
    ref = np.full((T, heads * 64), np.nan)
    bnd = np.full((T, heads * 64), np.nan)
    for f, n in texts:
        st = (n + 1) // 2 if steps is None else steps(n)
        for h in range(heads):                                              # (one head at a time: [len][len] matrices)
            o, b = attention_text(q[h:h + 1, f:f + n], k[h:h + 1, f:f + n], v[h:h + 1, f:f + n], scale, p16, st)
            ref[f:f + n, h * 64:(h + 1) * 64] = o[0]
            bnd[f:f + n, h * 64:(h + 1) * 64] = b[0]
    return ref, bnd


def e1_steps(n):
    return (n + 1) // 2


def e12_steps(n):
    return (n + 31) // 32


def e5_steps(n):
    return 0


# ---- LayerNorm (E2, E4 prologue, E7) ------------------------------------------------------------------------------------------------

def layernorm(x16, gamma16, beta16, eps):
    """LayerNorm(x) * gamma + beta of fp16 rows, biased variance, eps as the kernel receives it (fp32) -> (ref, bound)"""
    x = np.asarray(x16, dtype=np.float64)
    g = np.asarray(gamma16, dtype=np.float64)
    b = np.asarray(beta16, dtype=np.float64)
    hid = x.shape[-1]
    nch = hid // 512
    eps = float(np.float32(eps))
    mu = x.mean(axis=-1, keepdims=True)
    d = x - mu
    var = (d * d).mean(axis=-1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    y = d * rstd * g + b
    # LNSTAT
    dmu = (8 * nch + 7) * U32 * np.abs(x).mean(axis=-1, keepdims=True)
    dvar = (8 * nch + 9) * U32 * (var + ((np.abs(d) + dmu) ** 2).mean(axis=-1, keepdims=True)) + dmu ** 2 + U32 * (var + eps)
    drstd = 0.5 * dvar / (var + eps) + EXP2_REL
    other = dmu * rstd * np.abs(g) + (np.abs(d) + dmu) * rstd * np.abs(g) * (drstd + 3 * U32) + U32 * (np.abs(y) + np.abs(b))
    return y, round16_bound(y, other)


def add_layernorm(a16, b16, gamma16, beta16, eps):
    """E2: LayerNorm(half(a + b)) (the fp16 add is exact input to the statistics)"""
    s = (np.asarray(a16, dtype=np.float16) + np.asarray(b16, dtype=np.float16)).astype(np.float16)
    return layernorm(s, gamma16, beta16, eps)


# ---- projections (E3, E4) -----------------------------------------------------------------------------------------------------------

def gelu64(v):
    from math import erf
    return 0.5 * v * (1.0 + np.vectorize(erf)(v / np.sqrt(2.0)))


def linear(x16, w16, b16, epi=0, res16=None):
    """x W^T + b: epi 0 plain, 1 erf GELU, 2 res + half(x W^T + b) (the module's fp16 add) -> (ref, bound).
    ACC32 over sum|x w| + |b|; GELU: its slope (<= 1.13) on that, erff's few fp32 ulps and 0.5 v (1 + erf) in fp32 (cancellation
    in the negative tail: |v| 2^-23); residual: the kernel's intermediate rounding may land one fp16 step away from the reference's."""
    x = np.asarray(x16, dtype=np.float64)
    w = np.asarray(w16, dtype=np.float64)
    b = np.asarray(b16, dtype=np.float64)
    v = x @ w.T + b
    acc = ACC32_REL * (np.abs(x) @ np.abs(w).T + np.abs(b))
    if epi == 0:
        return v, round16_bound(v, acc)
    if epi == 1:
        y = gelu64(v)
        other = 1.13 * acc + 2.0 ** -22 * (np.abs(v) + acc) + 6 * U32 * np.abs(y)
        return y, round16_bound(y, other)
    mid = v.astype(np.float16).astype(np.float64)
    y = mid + np.asarray(res16, dtype=np.float64)
    other = acc + ulp16(np.abs(v) + acc)
    return y, round16_bound(y, other)


# ---- the comparison -----------------------------------------------------------------------------------------------------------------

def check(got, ref, bound, what=""):
    """assert |got - ref| <= bound element-wise (where ref is not NaN); on failure name the worst element, its index, the values and
    the err / bound ratio. Returns the largest ratio."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    sel = ~np.isnan(ref)
    err = np.where(sel, np.abs(got - np.where(sel, ref, 0.0)), 0.0)
    err = np.where(sel & ~np.isfinite(got), np.inf, err)
    bnd = np.where(sel, bound, 1.0)
    r = np.where(err == 0, 0.0, err / np.maximum(bnd, 1e-300))
    worst = np.unravel_index(int(np.argmax(r)), r.shape)
    mx = float(r[worst])
    assert mx <= 1.0, (f"{what}: worst element {tuple(int(i) for i in worst)}: got {got[worst]!r}, ref {ref[worst]!r}, "
                       f"err {err[worst]:.3e}, bound {bound[worst]:.3e}, err/bound {mx:.3g}")
    return mx
