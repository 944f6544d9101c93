"""The encoder kernels (E1 rdx_enc_attention_f16, E2 rdx_enc_add_layernorm_f16, E3 rdx_enc_linear_small_f16, E4
rdx_enc_stage_f16, E5 rdx_enc_attention_small_f16, E7 rdx_enc_layernorm_rows_f16, E12 rdx_enc_attention_mfma_f16) against the float64
references and per-element bounds of tests/enc_reference.py (every term tied to an operation the kernels document; the CPU file
tests/test_enc_reference.py shows that they reject plausible regressions). Attention first by exact-answer probes (q = 0: every weight
is 1 / len, one hot value row per text and head), then peaked, sink and random inputs, then the metadata production builds
(_PackedEncoder's canonical shapes); LayerNorm on offset, outlier, constant and near-constant rows; projections on cancelling rows and
an outlier column at the token-block edges. Every tok_first / tok_len / query block passed describes real tokens inside the buffer."""
import numpy as np
import pytest

import enc_reference as R

pytestmark = pytest.mark.gpu

F16 = np.float16
SCALE = 0.125


@pytest.fixture(scope="module")
def L():
    from rag_dpo_amd import _lib
    return _lib.load()


def _dev(a):
    """a device copy; the caller keeps the tensor alive until the launch has been synchronised (a temporary's memory may be handed to
    the next allocation at once)"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _out(shape, dtype=None):
    import torch
    return torch.full(shape, float("nan"), dtype=dtype or torch.float16, device="cuda")


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.float().cpu().numpy().astype(np.float64)


def _err():
    from rag_dpo_amd import _lib
    return _lib.last_error()


# ---- attention launchers ---------------------------------------------------------------------------------------------------------

def packed(lens):
    lens = np.asarray(lens, dtype=np.int64)
    first = np.cumsum(lens) - lens
    return first, lens, [(int(f), int(n)) for f, n in zip(first, lens)]


def e1(L, qkv, tf, tl, heads, promise):
    T = qkv.shape[0]
    ctx = _out((T, heads * 64))
    q, tfd, tld = _dev(qkv), _dev(tf.astype(np.int32)), _dev(tl.astype(np.int32))
    rc = L.rdx_enc_attention_f16(0, q.data_ptr(), tfd.data_ptr(), tld.data_ptr(), T, heads, 64, SCALE, int(promise), ctx.data_ptr(), _stream())
    assert rc == 0, _err()
    return _host(ctx)


def e5(L, qkv, tf, heads):
    T = qkv.shape[0]
    assert T <= 32
    ctx = _out((T, heads * 64))
    q, t = _dev(qkv), _dev(tf.astype(np.int32))
    assert L.rdx_enc_attention_small_f16(0, q.data_ptr(), t.data_ptr(), T, heads, 64, SCALE, ctx.data_ptr(), _stream()) == 0, _err()
    return _host(ctx)


def e12(L, qkv, qb, heads):
    qb = np.ascontiguousarray(np.asarray(qb, dtype=np.int32))
    T = qkv.shape[0]
    assert (qb[:, 0] >= 0).all() and (qb[:, 0] + qb[:, 1] <= T).all() and (qb[:, 2] < qb[:, 1]).all()
    ctx = _out((T, heads * 64))
    q, b = _dev(qkv), _dev(qb)
    assert L.rdx_enc_attention_mfma_f16(0, q.data_ptr(), b.data_ptr(), int(qb.shape[0]), heads, 64, SCALE, ctx.data_ptr(), _stream()) == 0, _err()
    return _host(ctx)


def query_blocks(first, lens):
    from rag_dpo_amd.embedding_provider import _PackedEncoder
    return _PackedEncoder._query_blocks(np.asarray(first, dtype=np.int64), np.asarray(lens, dtype=np.int64)).numpy()


def run_all(L, qkv, lens, heads, kernels, promises=None):
    """the kernels named in `kernels` on one packed qkv -> {name: ctx}"""
    first, lens_a, _ = packed(lens)
    tf, tl = np.repeat(first, lens_a), np.repeat(lens_a, lens_a)
    out = {}
    if "E1" in kernels:
        for pr in promises or [int(lens_a.max())]:
            out[f"E1/{pr}"] = e1(L, qkv, tf, tl, heads, pr)
    if "E5" in kernels:
        out["E5"] = e5(L, qkv, tf, heads)
    if "E12" in kernels:
        out["E12"] = e12(L, qkv, query_blocks(first, lens_a), heads)
    return out


RATIOS = {}


def check_attention(got, qkv, texts, heads, what):
    """got {kernel: ctx}: each against the fp64 reference with its kernel's bound"""
    refs = {}
    for name, ctx in got.items():
        kind = name.split("/")[0]
        if kind not in refs:
            p16, steps = {"E1": (False, R.e1_steps), "E5": (True, R.e5_steps), "E12": (True, R.e12_steps)}[kind]
            refs[kind] = R.attention_packed(qkv, texts, heads, SCALE, p16=p16, steps=steps)
        ref, bnd = refs[kind]
        r = R.check(ctx, ref, bnd, f"{what} {name}")
        RATIOS[kind] = max(RATIOS.get(kind, 0.0), r)


# ---- a. exact-answer probes -------------------------------------------------------------------------------------------------------

def hot_positions(n):
    """tile edges and every residue mod 32 that fit a text of n tokens"""
    c = [0, 31, 32, 33, 63, 64, 65, n - 1, (n - 1) // 32 * 32 - 32, (n - 1) // 32 * 32, (n - 1) // 32 * 32 - 1] + list(range(32))
    return [p for p in dict.fromkeys(c) if 0 <= p < n]


def hot_probe(lens, heads, shift):
    """q = 0, V = 0 but row hot(text, head) = value 1 + h / 16 in channel (text % 64) -> qkv, expected ctx"""
    first, lens_a, texts = packed(lens)
    T = int(lens_a.sum())
    qkv = np.zeros((T, 3, heads, 64), dtype=F16)
    want = np.zeros((T, heads * 64))
    for i, (f, n) in enumerate(texts):
        pos = hot_positions(n)
        for h in range(heads):
            val = 1.0 + h / 16
            qkv[f + pos[(i + 7 * h + shift) % len(pos)], 2, h, i % 64] = val
            want[f:f + n, h * 64 + i % 64] = val / n
    return qkv.reshape(T, -1), want, texts


def check_probe(got, want, what):
    """v / len within one fp16 rounding, exactly 0 everywhere else"""
    zero = want == 0
    assert (got[zero] == 0).all(), (what, np.argwhere(~(got == 0) & zero)[:5])
    bnd = 0.5 * R.ulp16(want) + R.ACC32_REL * 2 * want
    R.check(got, want, np.where(zero, 0.0, bnd), what)


@pytest.mark.parametrize("heads", [16, 2])
def test_attention_exact_answer_probes(L, heads):
    rng = np.random.default_rng(heads)
    e5_packs = [[32], [1] * 32, [5, 1, 9, 3, 14], [16, 16], [17, 15], [31, 1], [1, 31], [7, 6, 1, 1, 1]]
    e1_packs = [list(rng.integers(1, 65, size=120)), [64] * 9 + [1, 63, 33, 32, 31, 2], [100, 150, 30, 200, 1, 64, 300]]
    e12_packs = [[1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 200, 1023, 1024, 1025, 1500, 3, 700] + list(rng.integers(1, 300, size=40))]
    for shift in range(3):
        for lens in e5_packs:
            qkv, want, _ = hot_probe(lens, heads, shift)
            for name, got in run_all(L, qkv, lens, heads, ("E5", "E1", "E12")).items():
                check_probe(got, want, f"{name} {lens}")
        for lens in e1_packs:
            qkv, want, _ = hot_probe(lens, heads, shift)
            for name, got in run_all(L, qkv, lens, heads, ("E1", "E12"), promises=[int(max(lens)), 0]).items():
                check_probe(got, want, f"{name} {lens[:6]}")
        for lens in e12_packs:
            qkv, want, _ = hot_probe(lens, heads, shift)
            check_probe(run_all(L, qkv, lens, heads, ("E12",))["E12"], want, "E12")
    lens = [5, 4096, 7]                                        # one text of 4096 tokens between two neighbours
    for shift in range(3):
        qkv, want, _ = hot_probe(lens, 2, shift)
        check_probe(run_all(L, qkv, lens, 2, ("E12",))["E12"], want, "E12 4096")


# ---- b. peaked and sink probes ----------------------------------------------------------------------------------------------------

def peaked(lens, heads, rng, where):
    """q_i = 8 k_target(i): the target's score leads every other key's by >= 20 log2 units (checked)"""
    first, lens_a, texts = packed(lens)
    T = int(lens_a.sum())
    x = rng.standard_normal((T, 3, heads, 64))
    x[:, 1] = np.sign(x[:, 1])                                   # |k|^2 = 64: s_target = 8 * 64 / 8 = 64 nats
    for f, n in texts:
        tgt = {"first": rng.integers(0, min(n, 32), n), "last": rng.integers(max(0, (n - 1) // 32 * 32 - 32), n, n),
               "partial": rng.integers((n - 1) // 32 * 32, n, n)}[where]
        x[f:f + n, 0] = 8 * x[f + tgt, 1]
    qkv = x.reshape(T, -1).astype(F16)
    q, k, _ = R.split_qkv(qkv, heads)
    for f, n in texts:
        for h in range(heads if n > 1 else 0):
            s = -np.partition(-(q[h, f:f + n] @ k[h, f:f + n].T) * SCALE, 1, axis=1)
            assert ((s[:, 0] - s[:, 1]) * R.LOG2E >= 20).all()
    return qkv, texts


def monotone(lens, heads, rng, rising):
    """scores that rise (or fall) from tile to tile: q = 0.5, k_j = c_j (all dims), c_j increasing (decreasing) in j"""
    first, lens_a, texts = packed(lens)
    T = int(lens_a.sum())
    x = np.zeros((T, 3, heads, 64))
    x[:, 0] = 0.5
    x[:, 2] = rng.standard_normal((T, heads, 64))
    for f, n in texts:
        c = np.linspace(-1.0, 1.0, n) if rising else np.linspace(1.0, -1.0, n)
        x[f:f + n, 1] = c[:, None, None]
    return x.reshape(T, -1).astype(F16), texts


def sink(lens, heads, rng=None):
    """key 0 of every text 12 nats above the rest (q = 4 e_0, k_0 = 24 e_0), v_0 = 0, the others +1 in channel 1 (or random): the output
    is carried entirely by weights of e^-12 ~ 2^-17.3, fp16 subnormals once E5 / E12 round P"""
    first, lens_a, texts = packed(lens)
    T = int(lens_a.sum())
    qkv = np.zeros((T, 3, heads, 64), dtype=F16)
    qkv[:, 0, :, 0] = 4
    for f, n in texts:
        qkv[f, 1, :, 0] = 24
        if rng is None:
            qkv[f + 1:f + n, 2, :, 1] = 1
        else:
            qkv[f + 1:f + n, 2] = (rng.standard_normal((n - 1, heads, 64)) * 1.5).astype(F16)
    return qkv.reshape(T, -1), texts


def test_attention_peaked_monotone_and_sink_probes(L):
    rng = np.random.default_rng(7)
    long_lens, short_lens, e5_lens = [33, 1025, 64, 1500, 97], [20, 64, 1, 33, 50, 2], [9, 23]
    for heads in (16, 2):
        for where in ("first", "last", "partial"):
            for lens, kern in ((long_lens, ("E12",)), (short_lens, ("E1", "E12")), (e5_lens, ("E5", "E1", "E12"))):
                qkv, texts = peaked(lens, heads, rng, where)
                check_attention(run_all(L, qkv, lens, heads, kern), qkv, texts, heads, f"peaked {where}")
        for rising in (True, False):
            for lens, kern in ((long_lens, ("E12",)), (short_lens, ("E1", "E12")), (e5_lens, ("E5", "E1", "E12"))):
                qkv, texts = monotone(lens, heads, rng, rising)
                check_attention(run_all(L, qkv, lens, heads, kern), qkv, texts, heads, f"monotone {rising}")
    # the sink: if the matrix cores (or the conversion) flushed fp16 subnormal P, the output here would be ~0 instead of ~9e-3
    for lens, kern in (([33, 1025, 1500], ("E12",)), ([64, 40], ("E1", "E12")), ([32], ("E5", "E1", "E12")), ([20, 12], ("E5", "E12"))):
        for vals in (None, rng):
            qkv, texts = sink(lens, 2, vals)
            got = run_all(L, qkv, lens, 2, kern)
            check_attention(got, qkv, texts, 2, f"sink {lens}")
            if vals is None:
                for name, ctx in got.items():
                    f, n = texts[-1]
                    want = (n - 1) * np.exp(-12.0) / (1 + (n - 1) * np.exp(-12.0))
                    assert abs(ctx[f, 1] - want) <= 0.01 * want, (name, ctx[f, 1], want)


# ---- c. random inputs -----------------------------------------------------------------------------------------------------------

def test_attention_random_inputs_all_kernels(L):
    rng = np.random.default_rng(8)
    cases = [(16, [1, 64, 7, 20, 33, 2, 19, 21, 5], ("E1", "E12")), (8, list(rng.integers(1, 30, size=200)), ("E1", "E12")),
             (2, [100, 150, 30, 200, 1, 64], ("E1", "E12")), (16, [20], ("E5", "E1", "E12")), (4, [5, 1, 9, 3], ("E5", "E1", "E12")),
             (16, [22] + [1] * 10, ("E5", "E1", "E12")), (2, [15, 16], ("E5", "E1", "E12")),
             (16, [1, 64, 7, 200, 33, 2, 65, 31, 32, 128, 129], ("E12",)), (2, [1500, 1, 1023, 1024, 1025], ("E12",)),
             (16, [2048], ("E12",)), (4, list(rng.integers(1, 90, size=150)), ("E12",))]
    for heads, lens, kern in cases:
        T = int(sum(lens))
        qkv = (rng.standard_normal((T, 3 * heads * 64)) * 1.5).astype(F16)
        mx = int(max(lens))
        promises = sorted({mx, -(-mx // 16) * 16, -(-mx // 32) * 32, -(-mx // 64) * 64, 0, 2})
        first, lens_a, texts = packed(lens)
        check_attention(run_all(L, qkv, lens, heads, kern, promises), qkv, texts, heads, f"random {heads} {lens[:5]}")


# ---- d. the metadata production builds ------------------------------------------------------------------------------------------

def test_attention_on_production_metadata(L):
    from rag_dpo_amd.embedding_provider import _PackedEncoder as PE
    rng = np.random.default_rng(9)
    heads = 16
    # small canonical shapes (<= 8 texts): real tokens padded with one-token dummy texts to a multiple of 8 (<= 32 tokens, E5) or 32 (E1)
    for lens in ([5], [20], [3, 1, 4], [13, 14, 1, 2], [30, 2], [9] * 7, [64, 3], [40, 17, 33, 2, 1, 60, 7, 8]):
        lens_a = np.asarray(lens, dtype=np.int64)
        first = np.cumsum(lens_a) - lens_a
        T = int(lens_a.sum())
        g = 8 if T <= PE.STAGE_TOKENS else PE.SMALL_TOKEN_GRANULE
        Tp = -(-T // g) * g
        tf, tl = PE._canonical_texts(first, lens_a, Tp)
        lb = PE._window_promise(int(lens_a.max()))
        texts = list(zip(first.tolist(), lens)) + [(t, 1) for t in range(T, Tp)]
        qkv = (rng.standard_normal((Tp, 3 * heads * 64)) * 1.5).astype(F16)
        got = {f"E1/{lb}": e1(L, qkv, tf, tl, heads, lb)}
        if Tp <= 32:
            got["E5"] = e5(L, qkv, tf, heads)
        check_attention(got, qkv, texts, heads, f"small canonical {lens}")
    # large canonical shapes: padded to a multiple of LARGE_TOKEN_GRANULE, the MFMA work units filled up to B + g with the last unit
    for B in (60, 130):
        lens_a = rng.integers(1, 65, size=B).astype(np.int64)
        first = np.cumsum(lens_a) - lens_a
        T = int(lens_a.sum())
        g = PE.LARGE_TOKEN_GRANULE
        Tp = -(-T // g) * g
        tf, tl = PE._canonical_texts(first, lens_a, Tp)
        qb = PE._canonical_query_blocks(first, lens_a, Tp, B + g).numpy()
        assert qb.shape[0] == B + g and (qb[-1] == qb[Tp - T + B - 1]).all()
        texts = list(zip(first.tolist(), lens_a.tolist())) + [(t, 1) for t in range(T, Tp)]
        qkv = (rng.standard_normal((Tp, 3 * heads * 64)) * 1.5).astype(F16)
        lb = PE._window_promise(int(lens_a.max()))
        check_attention({f"E1/{lb}": e1(L, qkv, tf, tl, heads, lb), "E12": e12(L, qkv, qb, heads)}, qkv, texts, heads, f"large canonical {B}")


# ---- e. LayerNorm ---------------------------------------------------------------------------------------------------------------

def ln_rows(hid, rng, rows=37):
    """offset +-500, outlier features up to +-3e4, constant rows, variance far below eps, ordinary rows"""
    x = rng.standard_normal((rows, hid)) * 2 + 0.5
    x[0:4] = 500 + rng.standard_normal((4, hid))
    x[4:8] = -500 + rng.standard_normal((4, hid))
    x[8, rng.integers(0, hid)] = 3e4
    x[9, rng.integers(0, hid, 3)] = [-3e4, 2e4, 1.5e4]
    x[10, :] = 0.0
    x[10, 5] = -2.9e4
    x[11] = 123.5                                                   # constant rows: the output is beta, exactly
    x[12] = -0.25
    x[13] = 500
    x[14] = 1 + rng.integers(-2, 3, hid) * 2.0 ** -10              # variance ~1e-6, far below eps
    x[15] = -7 + rng.integers(-1, 2, hid) * 2.0 ** -8
    const = [11, 12, 13]
    return x, const


def ln_params(hid, rng):
    return (rng.standard_normal(hid) * 0.3 + 1).astype(F16), (rng.standard_normal(hid) * 0.2).astype(F16)


def test_layernorm_kernels(L):
    import torch
    rng = np.random.default_rng(10)
    eps = 1e-5
    for hid in (512, 1024, 1536, 2048):
        x, const = ln_rows(hid, rng)
        s = x.astype(F16)
        g, b = ln_params(hid, rng)
        rows = s.shape[0]
        # E2: a + b rounded to fp16 first (b chosen so that a + b stays finite: the rows of s are split in two halves)
        a16 = (s.astype(np.float64) * 0.5).astype(F16)
        b16 = (s.astype(np.float64) - a16.astype(np.float64)).astype(F16)
        ref, bnd = R.add_layernorm(a16, b16, g, b, eps)
        out = _out((rows, hid))
        ad, bd, gd, btd, sd = _dev(a16), _dev(b16), _dev(g), _dev(b), _dev(s)
        assert L.rdx_enc_add_layernorm_f16(0, ad.data_ptr(), bd.data_ptr(), gd.data_ptr(), btd.data_ptr(), eps, rows, hid,
                                           out.data_ptr(), _stream()) == 0, _err()
        got = _host(out)
        RATIOS["E2"] = max(RATIOS.get("E2", 0), R.check(got, ref, bnd, f"E2 {hid}"))
        s_sum = (a16 + b16).astype(F16)
        for r in const:
            if (s_sum[r] == s_sum[r][0]).all():
                assert (got[r] == b.astype(np.float64)).all(), (hid, r)
        # E7: fp32 output of the fp16 LayerNorm
        o32 = _out((rows, hid), torch.float32)
        assert L.rdx_enc_layernorm_rows_f16(0, sd.data_ptr(), gd.data_ptr(), btd.data_ptr(), eps, rows, hid, o32.data_ptr(), _stream()) == 0, _err()
        got = _host(o32)
        ref, bnd = R.layernorm(s, g, b, eps)
        RATIOS["E7"] = max(RATIOS.get("E7", 0), R.check(got, ref, bnd, f"E7 {hid}"))
        assert (got.astype(F16).astype(np.float64) == got).all()
        for r in const:
            assert (got[r] == b.astype(np.float64)).all(), (hid, r)
        # E4's prologue (n_in 512, 1024): the stored LayerNorm output y
        if hid in (512, 1024):
            for T in (1, 16, 17, 32):
                sT = s[:T] if T > 16 else s[np.r_[0:4, 8:20][:T]]
                N = 64
                w = (rng.standard_normal((N, hid)) * hid ** -0.5).astype(F16)
                bias = (rng.standard_normal(N) * 0.1).astype(F16)
                y = _out((T, hid))
                out = _out((T, N))
                std, wd, biasd = _dev(sT), _dev(w), _dev(bias)
                assert L.rdx_enc_stage_f16(0, std.data_ptr(), None, gd.data_ptr(), btd.data_ptr(), eps, y.data_ptr(), wd.data_ptr(),
                                           biasd.data_ptr(), None, T, N, hid, 0, 0, out.data_ptr(), _stream()) == 0, _err()
                yg, og = _host(y), _host(out)
                ref, bnd = R.layernorm(sT, g, b, eps)
                RATIOS["E4-LN"] = max(RATIOS.get("E4-LN", 0), R.check(yg, ref, bnd, f"E4 prologue {hid} {T}"))
                ref, bnd = R.linear(yg.astype(F16), w, bias)            # the projection of the kernel's own LayerNorm output
                RATIOS["E4"] = max(RATIOS.get("E4", 0), R.check(og, ref, bnd, f"E4 after prologue {hid} {T}"))


# ---- f. projections -------------------------------------------------------------------------------------------------------------

def proj_inputs(T, K, N, rng, rows_src=None):
    """x with an outlier column (x 100) and cancelling rows (its halves equal, W's halves opposite on the first N / 2 features)"""
    n = rows_src or T
    x = rng.standard_normal((n, K))
    x[:, 3] *= 100
    w = rng.standard_normal((N, K)) * K ** -0.5
    x[::3, K // 2:] = x[::3, :K // 2]
    w[: N // 2, K // 2:] = -w[: N // 2, :K // 2]
    return x.astype(F16), w.astype(F16), (rng.standard_normal(N) * 0.1).astype(F16)


def test_projection_small_linear(L):
    rng = np.random.default_rng(11)
    for T, N, K in ((1, 1024, 4096), (255, 256, 1024), (256, 128, 4096), (15, 1024, 1024), (17, 512, 2048), (32, 4096, 1024), (7, 512, 512)):
        x, w, b = proj_inputs(T, K, N, rng)
        for act in (0, 1):
            out = _out((T, N))
            xd, wd, bd = _dev(x), _dev(w), _dev(b)
            assert L.rdx_enc_linear_small_f16(0, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), T, N, K, act, out.data_ptr(), _stream()) == 0, _err()
            ref, bnd = R.linear(x, w, b, epi=act)
            RATIOS["E3"] = max(RATIOS.get("E3", 0), R.check(_host(out), ref, bnd, f"E3 {T} {N} {K} {act}"))


def test_projection_stage(L):
    rng = np.random.default_rng(12)
    for T in (1, 15, 16, 17, 31, 32):
        for N, K in ((1024, 4096), (512, 1024), (256, 2048), (128, 512)):
            x, w, b = proj_inputs(T, K, N, rng, rows_src=40)
            res = (rng.standard_normal((40, N)) * 2).astype(F16)
            idx = rng.permutation(40)[:T].astype(np.int64)
            xd, wd, bd, rd, idd = _dev(x), _dev(w), _dev(b), _dev(res), _dev(idx)
            refs = [R.linear(x, w, b, epi=epi, res16=res) for epi in (0, 1, 2)]     # all 40 source rows, once per shape
            for fpb in (16, 8, 4):
                for epi in (0, 1, 2):
                    for gather in (False, True):
                        out = _out((T, N))
                        assert L.rdx_enc_stage_f16(0, xd.data_ptr(), idd.data_ptr() if gather else None, None, None, 0.0, None, wd.data_ptr(), bd.data_ptr(),
                                                   rd.data_ptr(), T, N, K, epi, fpb, out.data_ptr(), _stream()) == 0, _err()
                        rows = idx if gather else np.arange(T)
                        ref, bnd = refs[epi][0][rows], refs[epi][1][rows]
                        RATIOS["E4"] = max(RATIOS.get("E4", 0), R.check(_host(out), ref, bnd, f"E4 {T} {N} {K} fpb {fpb} epi {epi} gather {gather}"))
    # the LayerNorm prologue with the GELU epilogue on offset rows
    for T in (1, 16, 17, 32):
        for K in (512, 1024):
            s = ln_rows(K, rng, rows=max(T, 16))[0][:T].astype(F16)
            g, bt = ln_params(K, rng)
            N = 256
            w = (rng.standard_normal((N, K)) * K ** -0.5).astype(F16)
            b = (rng.standard_normal(N) * 0.1).astype(F16)
            y, out = _out((T, K)), _out((T, N))
            sd, gd, btd, wd, bd = _dev(s), _dev(g), _dev(bt), _dev(w), _dev(b)
            assert L.rdx_enc_stage_f16(0, sd.data_ptr(), None, gd.data_ptr(), btd.data_ptr(), 1e-5, y.data_ptr(), wd.data_ptr(), bd.data_ptr(),
                                       None, T, N, K, 1, 16, out.data_ptr(), _stream()) == 0, _err()
            yg = _host(y)
            ref, bnd = R.layernorm(s, g, bt, 1e-5)
            RATIOS["E4-LN"] = max(RATIOS.get("E4-LN", 0), R.check(yg, ref, bnd, f"E4 prologue {T} {K}"))
            ref, bnd = R.linear(yg.astype(F16), w, b, epi=1)
            RATIOS["E4"] = max(RATIOS.get("E4", 0), R.check(_host(out), ref, bnd, f"E4 LN + GELU {T} {K}"))


def test_report_ratios():
    """(runs last in this file: the largest err / bound per kernel seen by the tests above, for the record)"""
    print("\nlargest err/bound per kernel:", {k: round(v, 4) for k, v in sorted(RATIOS.items())})
    assert all(v <= 1.0 for v in RATIOS.values())
