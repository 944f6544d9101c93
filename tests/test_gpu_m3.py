"""GPU: the combined BGE-M3 score (rag_dpo_amd/m3.py) — rdx_m3_combine against the numpy model on bits, M3Reranker on
the GPU against its CPU twin on a scripted provider, embed_m3_device against the two separate calls, and the retriever."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_maxsim_kernel import exact_and_bound  # noqa: E402
from test_late_interaction import DIM, Boost, ranked  # noqa: E402
from test_m3 import ScriptedM3, build_sources, make_chunks  # noqa: E402

from rag_dpo_amd import m3 as M3  # noqa: E402

pytestmark = pytest.mark.gpu

UNITS = [(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)]
WEIGHTS = [(0.4, 0.2, 0.4), (1.0, 1.0, 1.0)] + UNITS + [(1.0, 0.3, 0.0), (0.0, 0.7, 0.1)]


def components(n, seed):
    """values whose products and sums round: cosine-like fp32, lexical-like f64 with low bits set, MaxSim-like fp32"""
    rng = np.random.default_rng(seed)
    d = rng.uniform(-1, 1, n).astype(np.float32)
    s = rng.uniform(0, 40, n) * (1 + rng.uniform(0, 1, n) * 2.0 ** -30)
    c = rng.uniform(-1, 1, n).astype(np.float32)
    s[::7] = 0.0
    return d, s, c


def device_combine(d, s, c, w):
    from rag_dpo_amd import engine as E
    up = lambda a: None if a is None else torch.from_numpy(a).cuda()   # noqa: E731
    final, value = E.m3_combine(up(d), up(s), up(c), w, want_value=True)
    return value.cpu().numpy(), final.cpu().numpy()


@pytest.mark.parametrize("n", [1, 64, 65, 1000])
def test_combine_equals_the_model_on_value_and_final(n):
    d, s, c = components(n, n)
    for w in WEIGHTS:
        parts = [x if wi else None for x, wi in zip((d, s, c), w)]
        want_v, want_f = M3.combine_model(*parts, w)
        got_v, got_f = device_combine(*parts, w)
        assert np.array_equal(got_v.view(np.uint64), want_v.view(np.uint64)), w     # out_value, not only out_final: a contraction shows here
        assert np.array_equal(got_f.view(np.uint32), want_f.view(np.uint32)), w
    # a unit triple reproduces the component, cast to fp32
    for w, x in zip(UNITS, (d, s, c)):
        parts = [p if wi else None for p, wi in zip((d, s, c), w)]
        _, f = device_combine(*parts, w)
        assert np.array_equal(f.view(np.uint32), x.astype(np.float32).view(np.uint32))


def test_combine_nan_null_components_and_refused_weights():
    from rag_dpo_amd import _lib as L
    d, s, c = components(65, 3)
    d[5], s[9], c[11] = np.nan, np.nan, np.nan
    s[20] = np.inf
    w = (0.4, 0.2, 0.4)
    got_v, got_f = device_combine(d, s, c, w)
    want_v, want_f = M3.combine_model(d, s, c, w)
    assert np.isnan(got_v[[5, 9, 11]]).all() and np.isnan(got_f[[5, 9, 11]]).all() and got_v[20] == np.inf
    ok = ~np.isnan(want_v)
    assert np.array_equal(got_v[ok].view(np.uint64), want_v[ok].view(np.uint64)) and np.array_equal(np.isnan(got_v), np.isnan(want_v))
    # a NaN in a component whose weight is 0 is never read
    got_v, _ = device_combine(None, s, c, (0.0, 0.5, 0.5))
    assert not np.isnan(got_v[5]) and np.isnan(got_v[9])
    lib = L.load()
    t = [torch.from_numpy(x).cuda() for x in (d, s, c)]
    out_f = torch.full((65,), 7.0, dtype=torch.float32, device="cuda")
    p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())   # noqa: E731
    f = lambda dd, ss, cc, n, w: lib.rdx_m3_combine(0, p(dd), p(ss), p(cc), n, *w, p(out_f), None, None)   # noqa: E731
    nan, inf = float("nan"), float("inf")
    for bad in ((nan, 0.2, 0.4), (0.4, nan, 0.4), (0.4, 0.2, nan), (-0.1, 0.2, 0.4), (inf, 0.2, 0.4), (0.0, 0.0, 0.0), (1e308, 1e308, 1e308)):
        assert f(*t, 65, bad) == L.RDX_ERR_INVALID, bad
    assert f(*t, 0, w) == L.RDX_ERR_INVALID and f(*t, (1 << 20) + 1, w) == L.RDX_ERR_INVALID
    assert f(None, t[1], t[2], 65, w) == L.RDX_ERR_INVALID                          # a weight without its component
    assert f(t[0], t[1], t[2], 65, (0.4, 0.0, 0.4)) == L.RDX_ERR_INVALID            # a component without its weight
    assert lib.rdx_m3_combine(0, p(t[0]), p(t[1]), p(t[2]), 65, *w, None, None, None) == L.RDX_ERR_INVALID
    torch.cuda.synchronize()
    assert out_f.cpu().tolist() == [7.0] * 65                                        # nothing was launched
    assert f(t[0], None, t[2], 65, (0.4, 0.0, 0.4)) == L.RDX_OK                      # out_value may be NULL


# ---- the reranker ---------------------------------------------------------------------------------------------------------------------
def twins(weights, stored=lambda i: True, n=40):
    chunks = make_chunks(n, long=True)
    prov = ScriptedM3()
    cpu = build_sources(prov, chunks, "cpu", stored)
    gpu = build_sources(prov, chunks, "cuda", stored)
    mk = lambda src, dev: M3.M3Reranker(prov, src[0] if weights[0] else None, src[1] if weights[1] else None,   # noqa: E731
                                        src[2] if weights[2] else None, weights=weights, device=dev)
    return chunks, prov, mk(cpu, "cpu"), mk(gpu, "cuda")


def check_question(prov, cpu, weights, query, chunks, boosts, got, want):
    """dense and sparse equal on bits (asserted by the caller on the models' components); final within (w_c / W) B + 2^-23 max(|got|,
    |want|), B = exact_and_bound's derived MaxSim bound of the pair; equal ranking wherever the model's neighbouring gaps exceed twice that"""
    if not chunks:
        assert got == [] and want == []
        return
    W = (weights[0] + weights[1]) + weights[2]
    qv = prov.vectors(query)
    bound = np.asarray([exact_and_bound(qv, prov.vectors(cpu.chunk_text(c)))[1] if weights[2] else 0.0 for c in chunks])
    final = {r.original_rank: r.rerank_score for r in want}
    tol = lambda rank, a, b: (weights[2] / W) * bound[rank] + 2.0 ** -23 * max(abs(a), abs(b))   # noqa: E731
    model_all = cpu._model.last["final"].astype(np.float64) + (np.asarray(boosts) if boosts is not None else 0.0)
    order = np.argsort(-model_all, kind="stable")
    gaps = np.abs(np.diff(model_all[order]))
    worst = 2 * ((weights[2] / W) * bound.max() + 2.0 ** -23 * np.abs(model_all).max())
    if len(gaps) == 0 or gaps.min() > worst:
        assert [r.chunk_id for r in got] == [r.chunk_id for r in want] and [r.original_rank for r in got] == [r.original_rank for r in want]
    else:                                                                            # only the separated prefix must agree
        first_tie = int(np.argmax(gaps <= worst))
        assert [r.chunk_id for r in got][:first_tie] == [r.chunk_id for r in want][:first_tie]
    for r in got:
        if r.original_rank in final:
            f = final[r.original_rank]
            assert abs(r.rerank_score - f) <= tol(r.original_rank, r.rerank_score, f), (r.chunk_id, r.rerank_score, f)


@pytest.mark.parametrize("boosted", [False, True])
@pytest.mark.parametrize("half_missing", [False, True])
def test_reranker_equals_its_cpu_twin(boosted, half_missing):
    w = M3.DEFAULT_WEIGHTS
    chunks, prov, cpu, gpu = twins(w, stored=(lambda i: i % 2 == 0) if half_missing else (lambda i: True))
    matcher, topics = (Boost(), ["cookies"]) if boosted else (None, None)
    boosts = [Boost().topic_boost(["cookies"], c.metadata["rgpd_topics"]) for c in chunks] if boosted else None
    q = "transfert hors union européenne"
    prov.calls.clear()
    got = gpu.rerank(q, chunks, top_k=10, topic_matcher=matcher, question_topics=topics)
    assert [c[0] for c in prov.calls if c[0] == "m3"] == ["m3"] and prov.calls[0] == ("m3", [q], True, True, True)   # ONE forward for the question
    g_last = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in gpu._model.last.items()}
    want = cpu.rerank(q, chunks, top_k=10, topic_matcher=matcher, question_topics=topics)
    c_last = cpu._model.last
    assert len(got) == 10 and gpu.last_rerank_stats["path"] == "m3" and cpu.last_rerank_stats["path"] == "m3-model"
    assert gpu.last_rerank_stats["device_calls"] == 1
    assert gpu.last_rerank_stats["encoded"] == cpu.last_rerank_stats["encoded"] == (20 if half_missing else 0)
    assert np.array_equal(g_last["dense"].view(np.uint32), c_last["dense"].view(np.uint32))          # the dense component: equal on bits
    assert np.array_equal(g_last["sparse"].view(np.uint64), c_last["sparse"].view(np.uint64))        # the sparse component: equal on bits
    assert (c_last["sparse"] > 0).any() and (g_last["sparse"][1::2] == 0).all() == half_missing       # missing from the lexical index: +0.0
    check_question(prov, cpu, w, q, chunks, boosts, got, want)
    # 3 questions x (0, 1, 40) candidates; rerank_batch equals the loop of rerank exactly
    queries = ["registre des traitements", "cookies et traceurs publicitaires", q]
    lists = [[], chunks[5:6], chunks]
    tq = [topics, None, topics]
    prov.calls.clear()
    got = gpu.rerank_batch(queries, lists, top_k=10, topic_matcher=matcher, question_topics=tq)
    assert [c[:2] for c in prov.calls if c[0] == "m3"] == [("m3", queries[1:])]                       # ONE forward for all distinct questions
    assert gpu.last_rerank_stats["device_calls"] == 1 and gpu.last_rerank_stats["questions"] == 2
    loop = [gpu.rerank(qq, cc, top_k=10, topic_matcher=matcher, question_topics=t) for qq, cc, t in zip(queries, lists, tq)]
    assert [ranked(g) for g in got] == [ranked(x) for x in loop] and [len(g) for g in got] == [0, 1, 10]
    for i in (1, 2):
        want = cpu.rerank(queries[i], lists[i], top_k=10, topic_matcher=matcher, question_topics=tq[i])
        b = None if (boosts is None or tq[i] is None) else [boosts[chunks.index(c)] for c in lists[i]]
        check_question(prov, cpu, w, queries[i], lists[i], b, got[i], want)


def test_reranker_without_a_store_and_the_fallback():
    w = (1.0, 0.3, 0.0)
    chunks, prov, cpu, gpu = twins(w)
    assert gpu.store is None and gpu._on_gpu
    q = "durée de conservation"
    got, want = gpu.rerank(q, chunks, top_k=8), cpu.rerank(q, chunks, top_k=8)
    assert prov.calls[-2] == ("m3", [q], True, True, False)                                           # only the components with a weight
    assert ranked(got) == ranked(want)                                                                # no MaxSim: every bit is the model's
    # a candidate the collection does not hold: the scoring raises, the reference's fallback answers
    from test_late_interaction import chunk
    stranger = chunk(999, "inconnu au bataillon")
    out = gpu.rerank(q, chunks[:5] + [stranger], top_k=4)
    assert gpu.last_rerank_stats["path"] == "fallback"
    assert ranked(out) == [(c.chunk_id, c.similarity_score, i) for i, c in enumerate(chunks[:4])]
    both = gpu.rerank_batch([q, q], [chunks[:3] + [stranger], chunks[:6]], top_k=3)
    assert ranked(both[0]) == [(c.chunk_id, c.similarity_score, i) for i, c in enumerate(chunks[:3])]


def test_retrieve_reranked_batch_equals_the_loop():
    from rag_dpo_amd.retriever import DenseRetriever
    chunks, prov, cpu, gpu = twins(M3.DEFAULT_WEIGHTS, stored=lambda i: i < 25, n=60)
    col = gpu.collection

    class Dense:
        def embed(self, texts):
            return [prov.dense(t).tolist() for t in texts]

    ret = DenseRetriever(col, Dense())
    queries = ["durée de conservation", "cookies et traceurs", "registre"]
    topics = [["cookies"], None, ["cookies"]]
    got = ret.retrieve_reranked_batch(queries, gpu, n_candidates=40, top_k=10, topic_matcher=Boost(), question_topics=topics)
    assert gpu.last_rerank_stats["device_calls"] == 1 and gpu.last_rerank_stats["encoded"] > 0 and gpu.last_rerank_stats["path"] == "m3"
    want = [ret.retrieve_reranked(q, gpu, n_candidates=40, top_k=10, topic_matcher=Boost(), question_topics=t) for q, t in zip(queries, topics)]
    assert got == want and sum(len(x.chunks) for x in got[0]) == 10


# ---- one forward, three outputs -------------------------------------------------------------------------------------------------------
def test_embed_m3_device_against_the_separate_calls():
    from rag_dpo_amd.embedding_provider import EmbeddingProvider
    g = torch.Generator().manual_seed(7)
    rng = np.random.default_rng(3)
    words = [f"w{i}" for i in range(300)]
    texts = [" ".join(rng.choice(words, size=int(n))) for n in (5, 1, 17, 60, 2, 150)] + [""]

    def make(name, hidden, fused=None):
        col = (torch.randn((DIM, hidden), generator=g) * 0.125, torch.randn((DIM,), generator=g) * 0.1)
        sp = (torch.randn((1, hidden), generator=g) * 0.5, torch.zeros((1,)))
        p = EmbeddingProvider(model_name=name, device="cuda", dtype=torch.float16, batch_size=4, colbert_head=col, sparse_head=sp)
        p.fused_kernels = fused
        return p.load()

    # the tiny model in fp16 (tests/test_embedding_provider.py's 3e-3) and the mid model on librdx's fused kernels (its 2e-3)
    for name, hidden, tol in (("random-init:tiny", 64, 3e-3), ("random-init:mid", 512, 2e-3)):
        p = make(name, hidden)
        for batch in (texts, texts[:3], ["w1 w2 w3"]):
            cls = p.embed_device(batch).clone()
            out = p.embed_m3_device(batch)
            assert sorted(out) == ["dense", "lex", "tokens"]
            v, off = p.embed_tokens_device(batch)
            assert torch.equal(out["tokens"][0], v) and out["tokens"][1].tolist() == off.tolist()                 # bit-equal to the separate call
            ids, ws, loff = p.embed_lexical_device(batch)
            assert torch.equal(out["lex"][0], ids) and torch.equal(out["lex"][1].view(torch.int16), ws.view(torch.int16)) and out["lex"][2].tolist() == loff.tolist()
            d = out["dense"]
            assert d.is_cuda and d.dtype == torch.float32 and d.shape == cls.shape
            unit = lambda x: x / x.norm(dim=1, keepdim=True)   # noqa: E731
            assert float((unit(d) - unit(cls)).abs().max()) < tol, (name, float((unit(d) - unit(cls)).abs().max()))
            assert torch.equal(p.embed_device(batch), cls)                                                        # embed_device is unchanged afterwards
        assert sorted(p.embed_m3_device(texts[:2], dense=False, colbert=False)) == ["lex"]
    bare = EmbeddingProvider(model_name="random-init:tiny", device="cuda", dtype=torch.float16, batch_size=4).load()
    with pytest.raises(RuntimeError, match="colbert_linear.pt"):
        bare.embed_m3_device(["bonjour"])
    with pytest.raises(RuntimeError, match="sparse_linear.pt"):
        bare.embed_m3_device(["bonjour"], colbert=False)
    assert sorted(bare.embed_m3_device(["bonjour"], sparse=False, colbert=False)) == ["dense"]
