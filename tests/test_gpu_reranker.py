"""GPU: the reranker's librdx kernels (rdx_rerank_head_f16, rdx_rerank_select) against fp64 references with derived error bounds,
exact-answer probes and the golden fixture of the reference's own rerank; the reranker end to end against transformers' fp32 module
forward of the same weights; DenseRetriever.retrieve_reranked against its parts."""
import copy
import os
import sys
import zlib

import numpy as np
import pytest
import torch

from rag_dpo_amd import reranker as RR

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import reranker_world as W  # noqa: E402
from test_reranker import GOLDEN, check_against_gold, run_case  # noqa: E402

pytestmark = pytest.mark.gpu
U32 = 2.0 ** -24


def lib():
    from rag_dpo_amd import _lib
    return _lib, _lib.load()


def head(cls, wd, bd, wo, bo, stream=None):
    L, lib_ = lib()
    n, H = cls.shape
    ws = torch.empty(((H // L.RERANK_FEATURES) * n,), dtype=torch.float64, device="cuda")
    out = torch.empty((n,), dtype=torch.float32, device="cuda")
    st = (stream or torch.cuda.current_stream()).cuda_stream
    rc = lib_.rdx_rerank_head_f16(0, cls.data_ptr(), n, H, wd.data_ptr(), bd.data_ptr(), wo.data_ptr(), bo.data_ptr(), ws.data_ptr(),
                                  out.data_ptr(), st)
    assert rc == 0, L.last_error()
    return out


def select(scores, boosts, top_k, min_score, keep_min=3):
    L, lib_ = lib()
    n = len(scores)
    s = torch.as_tensor(np.asarray(scores, dtype=np.float32)).cuda()
    b = torch.as_tensor(np.asarray(boosts, dtype=np.float64)).cuda() if boosts is not None else None
    order = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    final = torch.empty((n,), dtype=torch.float64, device="cuda")
    count = torch.empty((1,), dtype=torch.int32, device="cuda")
    rc = lib_.rdx_rerank_select(0, s.data_ptr(), b.data_ptr() if b is not None else None, n, top_k, float(min_score), keep_min,
                                order.data_ptr(), final.data_ptr(), count.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.last_error()
    return order.cpu().tolist(), final.cpu().tolist(), int(count.item())


def head_reference(cls, wd, bd, wo, bo):
    """fp64 of the fp16 weights: (score, the derived bound on |kernel score - score|)"""
    h = cls.double().cpu().numpy()
    W_, b_, w_, c_ = (t.double().cpu().numpy() for t in (wd, bd, wo, bo))
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


def make_head(H, seed, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    wd = (torch.randn(H, H, generator=g) / H ** 0.5).half().cuda()
    bd = (torch.randn(H, generator=g) * 0.1).half().cuda()
    wo = (torch.randn(H, generator=g) * scale / H ** 0.5).half().cuda()
    bo = (torch.randn(1, generator=g) * 0.5).half().cuda()
    return wd, bd, wo, bo


@pytest.mark.parametrize("H", [512, 768, 1024])
def test_head_against_fp64_with_derived_bound(H):
    w = make_head(H, H)
    g = torch.Generator().manual_seed(H + 1)
    for n in (1, 3, 40, 100, 1024):
        cls = torch.randn(n, H, generator=g).cuda()                         # LayerNorm output scale
        got = head(cls, *w).double().cpu().numpy()
        want, bound = head_reference(cls, *w)
        err = np.abs(got - want)
        assert (err <= 1.0001 * bound).all(), (H, n, float((err / bound).max()))
        assert np.ptp(want) > 0.3 if n >= 40 else True
        again = head(cls, *w)                                               # no atomics: bit-identical on every call
        assert torch.equal(again, head(cls, *w)) and np.array_equal(again.double().cpu().numpy(), got)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = head(cls, *w, stream=side)
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(other, again)


def test_head_exact_probes():
    H = 1024
    wd, bd, wo, bo = make_head(H, 5)
    zero = torch.zeros_like(wd)
    cls = torch.randn(100, H).cuda()
    s = head(cls, zero, bd, wo, bo).cpu().numpy()
    assert (s == s[0]).all()                                                # W_d = 0: every pair scores sigmoid(w_o . tanh(b_d) + b_o)
    t = np.tanh(bd.double().cpu().numpy())
    want = 1.0 / (1.0 + np.exp(-(t @ wo.double().cpu().numpy() + bo.double().item())))
    assert abs(float(s[0]) - want) <= 2 * U32 * want
    order, final, count = select(s, None, 10, 0.08)
    assert order == list(range(100)) and count == 10 and final == [float(s[0])] * 100   # all tied: input order
    dup = cls[[7, 3, 7, 7, 3]].contiguous()                                 # duplicate rows: bit-equal scores
    d = head(dup, wd, bd, wo, bo).cpu().numpy()
    assert d[0] == d[2] == d[3] and d[1] == d[4]
    full = head(cls, wd, bd, wo, bo).cpu().numpy()
    assert d[0] == full[7] and d[1] == full[3]                              # a row's score does not depend on its neighbours


def test_select_reproduces_golden_fixture():
    for case, gold in zip(W.cases(), GOLDEN["cases"]):
        if case["raises"] or not case["idx"]:
            continue
        boosts = [float(b[2]) for b in gold["boosts"]] if gold["boosts"] else None
        order, final, count = select(case["scores"], boosts, case["top_k"], case["min_score"])
        want = [] if "raises" in gold else gold["result"]
        assert count == len(want), case["name"]
        assert order[:count] == [r["original_rank"] for r in want], case["name"]
        assert [repr(final[i]) for i in order[:count]] == [r["rerank_score"] for r in want], case["name"]
        assert sorted(order) == list(range(len(case["idx"])))


def test_select_fuzz_against_python_restatement():
    rng = np.random.default_rng(11)
    for it in range(60):
        n = int(rng.choice([1, 2, 3, 4, 17, 40, 100, 513, 1000, 1024]))
        levels = rng.uniform(0, 1, int(rng.integers(1, 6))).astype(np.float32)     # few distinct values: heavy ties
        scores = levels[rng.integers(0, len(levels), n)] if it % 3 else rng.uniform(0, 1, n).astype(np.float32)
        boosts = None
        if it % 2:
            boosts = np.where(rng.uniform(size=n) < 0.4, rng.choice([0.15, 0.05, -0.1, 0.0, 0.15 * 0.5], n), 0.0)
        top_k = int(rng.choice([0, 1, 2, 3, 8, 10, n, n + 5]))
        min_score = float(rng.choice([0.08, 0.0, 0.5, float(levels[0]), 2.0]))
        want = RR.select_host(scores, boosts, top_k, min_score)
        got = select(scores, boosts, top_k, min_score)
        assert got[0] == want[0] and got[2] == want[2], (it, n, top_k, min_score)
        assert np.array_equal(np.asarray(got[1]).view(np.int64), np.asarray(want[1]).view(np.int64)), it


def test_invalid_arguments_on_device():
    L, lib_ = lib()
    x = torch.zeros(4096, dtype=torch.float64, device="cuda")
    p = x.data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    for n, H in ((0, 1024), (1025, 1024), (4, 1000), (4, 4160), (4, 0)):
        assert lib_.rdx_rerank_head_f16(0, p, n, H, p, p, p, p, p, p, st) == L.RDX_ERR_INVALID and L.last_error()
    for n, top_k in ((0, 3), (1025, 3), (4, -1)):
        assert lib_.rdx_rerank_select(0, p, None, n, top_k, 0.08, 3, p, p, p, st) == L.RDX_ERR_INVALID and L.last_error()
    assert "top_k" in L.last_error()


# ---- end to end --------------------------------------------------------------------------------------------------------------

def pairs_of_lengths(lengths, seed):
    rng = np.random.default_rng(seed)
    vocab = [a + b for a in "abcdefghijklmnopqrstuvwxyz" for b in "abcdefghijklmnopqrstuvwxyz"]   # 3 characters a word: 512 tokens fit the 2048-character cut
    q = " ".join(rng.choice(vocab, 12))
    return [(q, " ".join(rng.choice(vocab, max(1, L - 16)))) for L in lengths]


def module_cls32(ref, tokenize, pairs):
    enc = tokenize([p[0] for p in pairs], [p[1] for p in pairs])
    with torch.no_grad():
        out = []
        for a in range(0, len(pairs), 8):
            ids, att = enc["input_ids"][a:a + 8].cuda(), enc["attention_mask"][a:a + 8].cuda()
            w = int(att.sum(1).max())
            out.append(ref.roberta(input_ids=ids[:, :w], attention_mask=att[:, :w]).last_hidden_state[:, 0].double())
    return torch.cat(out)


def spread_head_along_pairs(m, ref, cls32):
    """point out_proj along the direction the pairs' tanh(z) rows differ most, scaled to a logit spread of ~2 (a random-init head
    barely separates them); the same fp16 values in the kernel's weights (views of the module's) and in the fp32 reference"""
    c = ref.classifier
    t = torch.tanh(cls32 @ c.dense.weight.double().T + c.dense.bias.double())
    tc = t - t.mean(0)
    v = torch.linalg.svd(tc, full_matrices=False).Vh[0]
    k = 2.0 / float((tc @ v).std().detach())
    w = (v * k).half()
    with torch.no_grad():
        m.model.classifier.out_proj.weight.copy_(w[None, :].to(m.model.dtype))
        m.model.classifier.out_proj.bias.fill_(float(-(t @ w.double()).mean()))
        c.out_proj.weight.copy_(m.model.classifier.out_proj.weight.float())
        c.out_proj.bias.copy_(m.model.classifier.out_proj.bias.float())
    assert m.w_o.data_ptr() == m.model.classifier.out_proj.weight.data_ptr() or m.model.dtype != torch.float16
    if m.model.dtype != torch.float16:
        m.w_o.copy_(m.model.classifier.out_proj.weight.reshape(-1).half())
        m.b_o.copy_(m.model.classifier.out_proj.bias.half())


def check_end_to_end(spec, lengths, want_path, seed=0):
    r = RR.CrossEncoderReranker(f"random-init:{spec}", device="cuda", dtype=torch.float16, min_score=0.0)
    r._load_model()
    m = r._model
    assert m.path == want_path
    ref = copy.deepcopy(m.model).float()
    pairs = pairs_of_lengths(lengths, seed)
    cls32 = module_cls32(ref, m.tokenize, pairs)
    spread_head_along_pairs(m, ref, cls32)
    from rag_dpo_amd.retriever import RetrievedChunk
    chunks = [RetrievedChunk(f"c{i}", d, f"doc{i % 7}", "GUIDE", i, "high", 0.5, {}) for i, (_, d) in enumerate(pairs)]
    out = r.rerank(pairs[0][0], chunks, top_k=len(pairs))
    st = r.last_rerank_stats
    assert st["path"] == want_path and st["pairs"] == len(pairs) and st["tokens"] == sum(max(L, 17) for L in lengths)   # (12 query pieces + 1 text piece + 4 specials at least)
    assert st["ms_forward"] > 0 and st["ms_head_select"] > 0
    got = np.empty(len(pairs))
    for o in out:
        got[o.original_rank] = o.rerank_score
    assert len(out) == len(pairs)
    with torch.no_grad():
        cls16 = m._cls_rows(pairs, 32).double()
        cos = torch.nn.functional.cosine_similarity(cls16, cls32, dim=1)
        assert float((1 - cos).max()) <= 1e-4, float((1 - cos).max())          # the fp16 backbone against the fp32 module forward
        c = m.model.classifier
        hw = (c.dense.weight.half(), c.dense.bias.half(), c.out_proj.weight.half().reshape(-1), c.out_proj.bias.half())
        want, _ = head_reference(cls32, *hw)                     # the fp32 module backbone, its head in fp64
        _, head_bound = head_reference(cls16, *hw)               # the kernel's own rounding on the rows it was given
        # tolerance: the two backbones' difference pushed through the head (tanh 1-Lipschitz, sigmoid 1/4-Lipschitz) + the head's rounding
        dz = ((cls16 - cls32) @ hw[0].double().T).abs()
        tol = (0.25 * (dz @ hw[2].double().abs())).cpu().numpy() + head_bound + 1e-9
    err = np.abs(got - want)
    assert (err <= tol).all(), (spec, float((err / tol).max()), float(err.max()))
    T = float(tol.max())
    assert T <= 0.1 and np.ptp(want) > 0.3, (T, np.ptp(want))
    idx = np.argsort(-want, kind="stable")
    for a, b in zip(idx[:-1], idx[1:]):
        if want[a] - want[b] > 2 * T:
            assert got[a] > got[b]
    return T


def test_end_to_end_mid_fused_both_attention_paths():
    rng = np.random.default_rng(3)
    T1 = check_end_to_end("mid", [int(x) for x in rng.integers(10, 513, 40)], "fused", seed=1)        # > 64 tokens: MFMA attention
    T2 = check_end_to_end("mid", [int(x) for x in rng.integers(10, 65, 12)], "fused", seed=2)         # all <= 64: VALU attention
    print(f"mid: score tolerance {T1:.2e} (mixed lengths), {T2:.2e} (short)")


def test_end_to_end_xlm_roberta_large_fused():
    rng = np.random.default_rng(4)
    T = check_end_to_end("xlm-roberta-large", [int(x) for x in rng.integers(10, 513, 40)], "fused", seed=3)
    print(f"xlm-roberta-large: score tolerance {T:.2e}")


def test_end_to_end_xlm_roberta_base_module_backbone_with_head_kernels():
    rng = np.random.default_rng(5)
    T = check_end_to_end("xlm-roberta-base", [int(x) for x in rng.integers(10, 513, 24)], "module+kernels", seed=4)
    print(f"xlm-roberta-base: score tolerance {T:.2e}")


def test_fake_model_on_gpu_equals_cpu_result():
    for case, gold in zip(W.cases(), GOLDEN["cases"]):
        check_against_gold(case, gold, *run_case(case, gold, device="cuda"))


def test_retrieve_reranked_equals_its_parts():
    from rag_dpo_amd.collection import Collection
    from rag_dpo_amd.retriever import DenseRetriever, documents_from_ranked_chunks

    rng = np.random.default_rng(9)
    n, d = 300, 64
    emb = rng.standard_normal((n, d)).astype(np.float32)
    col = Collection("rerank_test", metadata={"hnsw:space": "cosine"})
    col.add(ids=[f"chunk_{i}" for i in range(n)], embeddings=emb, documents=[f"texte {i} conservation" for i in range(n)],
            metadatas=[{"document_path": f"doc_{i % 23}", "chunk_nature": ["GUIDE", "DOCTRINE"][(i % 23) % 2], "chunk_index": i // 23,
                        "rgpd_topics": "cookies" if i % 5 == 0 else ""} for i in range(n)])

    class Provider:
        def embed(self, texts):
            return [list(np.random.default_rng(zlib.crc32(t.encode())).standard_normal(d)) for t in texts]

    class Model:
        def predict(self, pairs, batch_size=32, show_progress_bar=True):
            return np.asarray([(zlib.crc32(p[1].encode()) % 1000) / 1000.0 for p in pairs], dtype=np.float32)

    class Boost:
        def topic_boost(self, topics, tags):
            return 0.15 if tags == "cookies" else 0.0

    ret = DenseRetriever(col, Provider())
    gpu = RR.CrossEncoderReranker(device="cuda")
    cpu = RR.CrossEncoderReranker(device="cpu")
    gpu._model = cpu._model = Model()
    got = ret.retrieve_reranked("durée de conservation", gpu, n_candidates=40, top_k=10, topic_matcher=Boost(), question_topics=["cookies"])
    cands = ret.retrieve_candidates("durée de conservation", n_candidates=40)
    want = documents_from_ranked_chunks(cpu.rerank("durée de conservation", cands, top_k=10, topic_matcher=Boost(), question_topics=["cookies"]))
    assert len(cands) == 40 and got == want and sum(len(x.chunks) for x in got) == 10
