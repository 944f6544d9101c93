"""E14 rdx_enc_gemm_f16 (csrc/enc_gemm.hpp) and rdx_enc_layernorm_f16 against the float64 references and per-element bounds
of tests/enc_reference.py (`linear`, `layernorm`: every term tied to a rounding the kernels document, nothing fitted; err / bound <= 1
passes), with the helpers of tests/test_gpu_encoder_kernels.py. Each epilogue on outlier / cancelling inputs at the ragged edges of both
tile shapes, a one-hot layout probe with an exact answer, bit-equality across calls, streams and graph replays, and the provider's
gemm="rdx" forward against the module forward."""
import numpy as np
import pytest

import enc_reference as R
import test_gpu_encoder_kernels as EK

pytestmark = pytest.mark.gpu

F16 = np.float16
PAD = 8                                   # rows of `out` behind T: pre-filled with NaN, must keep their bits
NAN16 = np.array([np.nan], dtype=F16).view(np.uint16)[0]
RATIOS = {}


@pytest.fixture(scope="module")
def L():
    from rag_dpo_amd import _lib
    return _lib.load()


def gemm(L, xd, wd, bd, T, N, K, epi, rd=None, out=None, stream=None):
    """-> the [T + PAD][N] output tensor (device); rows >= T were NaN before the launch"""
    out = EK._out((T + PAD, N)) if out is None else out
    rc = L.rdx_enc_gemm_f16(0, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), rd.data_ptr() if rd is not None else None, T, N, K, epi,
                            out.data_ptr(), EK._stream() if stream is None else stream)
    assert rc == 0, EK._err()
    return out


def bits(t):
    import torch
    torch.cuda.synchronize()
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def check_epilogues(L, T, N, K, rng, epis=(0, 1, 2)):
    x, w, b = EK.proj_inputs(T, K, N, rng)
    res = (rng.standard_normal((T, N)) * 2).astype(F16)
    xd, wd, bd, rd = EK._dev(x), EK._dev(w), EK._dev(b), EK._dev(res)
    for epi in epis:
        out = gemm(L, xd, wd, bd, T, N, K, epi, rd if epi == 2 else None)
        raw = bits(out)
        assert (raw[T:] == NAN16).all(), f"{T} {N} {K} epi {epi}: a row at or past T was written"
        got = EK._host(out)[:T]
        assert np.isfinite(got).all(), f"{T} {N} {K} epi {epi}: a row below T was not written"
        ref, bnd = R.linear(x, w, b, epi=epi, res16=res)
        r = R.check(got, ref, bnd, f"E14 {T} {N} {K} epi {epi}")
        print(f"E14 T {T} N {N} K {K} epi {epi}: err/bound {r:.4f}")
        RATIOS[f"E14/{epi}"] = max(RATIOS.get(f"E14/{epi}", 0.0), r)


# the issue's table: one, two and 64 k-steps; N not a multiple of either tile width; T on both sides of 64 and 256
SHAPES = [(1, 64, 64), (17, 64, 128), (63, 192, 512), (64, 256, 1024), (65, 320, 1024), (255, 1024, 1024), (256, 3072, 1024),
          (300, 4096, 1024), (513, 1024, 4096), (1000, 256, 64)]
# BM - 1, BM, BM + 1, 2 BM + 1 of the row tiles not in the table: 64 -> 129; 128 -> 127, 128, 129, 257
EDGES = [(127, 128, 128), (128, 192, 64), (129, 64, 128), (257, 128, 64)]


@pytest.mark.parametrize("T,N,K", SHAPES + EDGES)
def test_each_epilogue_against_the_fp64_model(L, T, N, K):
    check_epilogues(L, T, N, K, np.random.default_rng(T * 7 + N + K))


def large_tile(T, N):
    """the launcher's rule (enc_gemm.hpp enc_gemm_large): the 128 x 128 tile from 256 tiles on"""
    return -(-T // 128) * -(-N // 128) >= 256


# The same row edges ON the 128 x 128 tile, every epilogue: the launcher takes it from 256 tiles on, so few rows need many features.
# N = 11 072 = 86.5 tiles: the last column tile is half outside. K = 64 / 128 keep the row-edge cases small; the two K = 1024 and
# K = 4096 cases run the 16- and 64-step chain on this instantiation (8 LDS-DMA instructions per thread and stage, 64 KiB of LDS): every
# stage buffer is re-filled after it was read, which is what the loop's barrier orders.
LARGE = [(1, 32768, 64), (127, 32768, 64), (128, 32768, 64), (129, 16384, 128), (257, 11072, 64), (257, 11072, 1024), (129, 16384, 4096)]


@pytest.mark.parametrize("T,N,K", LARGE)
def test_row_edges_and_long_chains_of_the_large_tile(L, T, N, K):
    assert large_tile(T, N) and not any(large_tile(t, n) for t, n, _ in SHAPES + EDGES)
    check_epilogues(L, T, N, K, np.random.default_rng(T + N + K))


def test_layout_probe_is_exact(L):
    """x[t] = the one-hot row at column (7 t + 3) mod K, W asymmetric random: out[t][n] = half(w[n][k_t] + b[n]) bit for bit. A transposed
    fragment map, a wrong tile offset or a swizzle that differs between the staging and the read cannot pass. Both tile shapes."""
    rng = np.random.default_rng(21)
    for T, K, N in ((300, 512, 320), (300, 128, 11072)):
        kt = (7 * np.arange(T) + 3) % K
        x = np.zeros((T, K), dtype=F16)
        x[np.arange(T), kt] = 1
        w = rng.standard_normal((N, K)).astype(F16)
        b = (rng.standard_normal(N) * 0.1).astype(F16)
        want = (w.astype(np.float32)[:, kt].T + b.astype(np.float32)[None, :]).astype(F16)      # one fp32 add, one rounding
        xd, wd, bd = EK._dev(x), EK._dev(w), EK._dev(b)
        raw = bits(gemm(L, xd, wd, bd, T, N, K, 0))
        assert (raw[T:] == NAN16).all()
        bad = np.argwhere(raw[:T] != want.view(np.uint16))
        assert bad.size == 0, (T, K, N, len(bad), bad[:5])


def test_same_bits_on_every_call_stream_and_replay(L):
    import torch
    rng = np.random.default_rng(22)
    for T, N, K, epi in ((300, 320, 512, 2), (257, 11072, 1024, 1)):
        x, w, b = EK.proj_inputs(T, K, N, rng)
        res = (rng.standard_normal((T, N)) * 2).astype(F16)
        xd, wd, bd, rd = EK._dev(x), EK._dev(w), EK._dev(b), EK._dev(res)
        first = bits(gemm(L, xd, wd, bd, T, N, K, epi, rd))
        assert (bits(gemm(L, xd, wd, bd, T, N, K, epi, rd)) == first).all()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            o2 = gemm(L, xd, wd, bd, T, N, K, epi, rd, stream=side.cuda_stream)
        torch.cuda.current_stream().wait_stream(side)
        assert (bits(o2) == first).all()
        og = EK._out((T + PAD, N))
        side.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            gemm(L, xd, wd, bd, T, N, K, epi, rd, out=og, stream=torch.cuda.current_stream().cuda_stream)
        for _ in range(2):
            og.fill_(float("nan"))
            g.replay()
            assert (bits(og) == first).all()


@pytest.mark.parametrize("hid", [512, 1024, 2048])
def test_layernorm_kernel(L, hid):
    rng = np.random.default_rng(hid)
    big, const = EK.ln_rows(hid, rng, rows=257)
    g, b = EK.ln_params(hid, rng)
    gd, btd = EK._dev(g), EK._dev(b)
    ref_all, bnd_all = R.layernorm(big.astype(F16), g, b, 1e-5)
    for rows in (1, 17, 257):
        s = big.astype(F16)[:rows]
        sd = EK._dev(s)
        out = EK._out((rows + PAD, hid))
        assert L.rdx_enc_layernorm_f16(0, sd.data_ptr(), gd.data_ptr(), btd.data_ptr(), 1e-5, rows, hid, out.data_ptr(), EK._stream()) == 0, EK._err()
        assert (bits(out)[rows:] == NAN16).all()
        got = EK._host(out)[:rows]
        r = R.check(got, ref_all[:rows], bnd_all[:rows], f"LN {hid} {rows}")
        RATIOS["LN"] = max(RATIOS.get("LN", 0.0), r)
        for c in const:
            if c < rows:
                assert (got[c] == b.astype(np.float64)).all(), (hid, c)           # a constant row gives beta, exactly


def test_layernorm_refuses_hidden_768(L):
    from rag_dpo_amd import _lib
    s = EK._out((4, 768))
    assert L.rdx_enc_layernorm_f16(0, s.data_ptr(), s.data_ptr(), s.data_ptr(), 1e-5, 4, 768, s.data_ptr(), EK._stream()) == _lib.RDX_ERR_INVALID
    assert "hidden" in _lib.last_error()


# ---- the provider --------------------------------------------------------------------------------------------------------------

def test_provider_rdx_gemm_against_the_module_forward(monkeypatch):
    """gemm="rdx" from 33 tokens on: short questions (small canonical graphs), a batch with one 150-token text (the MFMA attention, eager)
    and a repeated large shape (captured on the second sighting, replayed on the third) against the module forward in fp16 and fp32,
    |1 - cos| <= 1e-5; no torch.nn.functional.linear / gelu runs during the forward."""
    import torch
    from rag_dpo_amd import synth
    from rag_dpo_amd.embedding_provider import EmbeddingProvider
    F = torch.nn.functional
    name = "random-init:mid"
    fast = EmbeddingProvider(model_name=name, device="cuda:0", dtype=torch.float16, batch_size=256, gemm="rdx").load()
    fast._packed.GEMM_MIN_TOKENS = 33
    assert fast._packed.fused and fast._packed.gemm == "rdx"
    mods = []
    for dt in (torch.float16, torch.float32):
        m = EmbeddingProvider(model_name=name, device="cuda:0", dtype=dt, batch_size=256)
        m.packed_forward = False
        mods.append(m.load())
    calls = {"linear": 0, "gelu": 0}
    real_linear, real_gelu = F.linear, F.gelu

    def counted(batch):
        def lin(*a, **k):
            calls["linear"] += 1
            return real_linear(*a, **k)

        def gel(*a, **k):
            calls["gelu"] += 1
            return real_gelu(*a, **k)
        with monkeypatch.context() as mp:
            mp.setattr(F, "linear", lin)
            mp.setattr(F, "gelu", gel)
            out = fast.embed_device(batch).clone()
        assert fast.last_encode_stats["tokens_real"] >= 33
        assert calls == {"linear": 0, "gelu": 0}, (calls, len(batch))
        return out

    def against_modules(got, batch, what):
        for m in mods:
            cos = F.cosine_similarity(got.double(), m.embed_device(batch).double(), dim=1)
            worst = float((1 - cos).abs().max())
            print(f"{what} vs module {m.dtype}: |1 - cos| {worst:.3e}")
            assert worst <= 1e-5, (what, m.dtype, worst)

    qs = synth.query_texts(6, seed=3)
    long_text = " ".join(f"w{i}" for i in range(148))                               # 150 tokens with <s> and </s>
    for what, batch in (("short questions", qs), ("one 150-token text", qs[:3] + [long_text] + qs[3:] + synth.query_texts(6, seed=4))):
        got = counted(batch)
        against_modules(got, batch, what)
        for _ in range(2):                                                          # (small canonical shapes: capture, replay)
            assert torch.equal(counted(batch), got), what
    # the padded scatter -> SDPA -> gather path (long texts with the MFMA attention switched off) takes the kernel for all four projections too
    fast._packed.long_attention = False
    mixed = qs[:3] + [long_text] + qs[3:] + synth.query_texts(6, seed=4)
    against_modules(counted(mixed), mixed, "one 150-token text, padded attention")
    fast._packed.long_attention = True
    big = synth.query_texts(90, seed=1)                                             # ~1.8 K tokens: the 2048-token canonical shape
    eager = counted(big)
    against_modules(eager, big, "large, eager")
    counted(big)                                                                    # second sighting: captured
    assert any(k[0] == "large" for k in fast._packed._graph)
    replayed = counted(big)                                                         # third: replayed
    against_modules(replayed, big, "large, replayed")
    cos = F.cosine_similarity(replayed.double(), eager.double(), dim=1)
    assert float((1 - cos).abs().max()) <= 1e-5
    for p in [fast] + mods:
        p.unload()


def test_report_ratios():
    """(runs last in this file: the largest err / bound per kernel seen by the tests above, for the record)"""
    print("\nlargest err/bound per kernel:", {k: round(v, 4) for k, v in sorted(RATIOS.items())})
    assert all(v <= 1.0 for v in RATIOS.values())
