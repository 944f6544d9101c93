"""The host side of rdx_enc_gemm_f16 / rdx_enc_layernorm_f16 (include/rdx.h) and of EmbeddingProvider(gemm=...): the symbols
are bound, every invalid argument is refused with RDX_ERR_INVALID and a message BEFORE the device is touched (so all of this runs on
a machine without a GPU), and the provider refuses what it cannot honour."""
import pytest

A = 0x10000          # a 16-byte aligned non-NULL "pointer": validation never dereferences it


@pytest.fixture(scope="module")
def L():
    from rag_dpo_amd import _lib
    return _lib.load(require_gpu=False)


def test_symbols_are_bound(L):
    from rag_dpo_amd import _lib
    assert "rdx_enc_gemm_f16" in _lib.SYMBOLS and "rdx_enc_layernorm_f16" in _lib.SYMBOLS
    assert hasattr(L, "rdx_enc_gemm_f16") and hasattr(L, "rdx_enc_layernorm_f16")


def gemm(L, x=A, w=A, bias=A, res=None, T=100, N=128, K=128, epi=0, out=A):
    return L.rdx_enc_gemm_f16(0, x, w, bias, res, T, N, K, epi, out, None)


@pytest.mark.parametrize("what,kw", [
    ("n_out % 64", dict(N=96)), ("n_out % 64", dict(N=0)), ("n_out % 64", dict(N=1000)),
    ("n_in % 64", dict(K=32)), ("n_in % 64", dict(K=0)), ("n_in % 64", dict(K=1056 - 8)),
    ("n_tokens < 0", dict(T=-1)),
    ("epilogue", dict(epi=-1)), ("epilogue", dict(epi=3)),
    ("residual", dict(epi=2, res=None)),
    ("too many tiles", dict(T=1 << 50)), ("too many tiles", dict(T=(1 << 24) * 128, N=64)), ("too many tiles", dict(T=1 << 30, N=4096)),
    ("null x", dict(x=None)), ("null w", dict(w=None)), ("null bias", dict(bias=None)), ("null out", dict(out=None)),
    ("misaligned x", dict(x=A + 2)), ("misaligned w", dict(w=A + 8)), ("misaligned bias", dict(bias=A + 4)),
    ("misaligned res", dict(epi=2, res=A + 2)), ("misaligned out", dict(out=A + 6)),
])
def test_gemm_refuses_invalid_arguments(L, what, kw):
    from rag_dpo_amd import _lib
    assert gemm(L, **kw) == _lib.RDX_ERR_INVALID, what
    assert "rdx_enc_gemm_f16" in _lib.last_error(), what


def test_gemm_of_no_tokens_succeeds_without_a_device(L):
    assert gemm(L, T=0) == 0
    assert gemm(L, T=0, epi=2, res=A) == 0


@pytest.mark.parametrize("what,kw", [
    ("hidden", dict(hidden=768)), ("hidden", dict(hidden=0)), ("hidden", dict(hidden=2560)), ("rows", dict(rows=-1)), ("rows", dict(rows=1 << 26)), ("rows", dict(rows=1 << 40)),
    ("null s", dict(s=None)), ("null gamma", dict(gamma=None)), ("null beta", dict(beta=None)), ("null out", dict(out=None)),
    ("misaligned s", dict(s=A + 2)), ("misaligned gamma", dict(gamma=A + 8)), ("misaligned out", dict(out=A + 4)),
])
def test_layernorm_refuses_invalid_arguments(L, what, kw):
    from rag_dpo_amd import _lib
    a = dict(s=A, gamma=A, beta=A, rows=5, hidden=1024, out=A)
    a.update(kw)
    assert L.rdx_enc_layernorm_f16(0, a["s"], a["gamma"], a["beta"], 1e-5, a["rows"], a["hidden"], a["out"], None) == _lib.RDX_ERR_INVALID, what
    assert "rdx_enc_layernorm_f16" in _lib.last_error() and (what != "rows" or "rows" in _lib.last_error()), what
    assert L.rdx_enc_layernorm_f16(0, A, A, A, 1e-5, 0, 1024, A, None) == 0


def test_provider_refuses_an_unknown_gemm():
    from rag_dpo_amd.embedding_provider import EmbeddingProvider
    with pytest.raises(ValueError):
        EmbeddingProvider(model_name="random-init:tiny", device="cpu", gemm="nope")
    for ok in ("blas", "rdx"):
        EmbeddingProvider(model_name="random-init:tiny", device="cpu", gemm=ok)       # construction alone never touches a device


def test_provider_refuses_rdx_gemm_where_the_fused_forward_does_not_run():
    import torch
    from rag_dpo_amd.embedding_provider import EmbeddingProvider
    p = EmbeddingProvider(model_name="random-init:tiny", device="cpu", dtype=torch.float32, gemm="rdx")
    with pytest.raises(ValueError):
        p.load()
    assert not p.is_loaded


def test_default_gemm_is_blas():
    from rag_dpo_amd.embedding_provider import EmbeddingProvider, _PackedEncoder
    import os
    assert EmbeddingProvider(model_name="random-init:tiny", device="cpu").gemm is None
    if "RDX_ENC_GEMM" not in os.environ:
        assert _PackedEncoder.gemm == "blas"
