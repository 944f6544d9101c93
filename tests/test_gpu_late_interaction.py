"""GPU end to end: LateInteractionReranker on a GPU store (rdx_maxsim_f16, rdx_rerank_select_batch) against the CPU reranker, which scores
through the numpy model, on the same stored vectors; the provider's token vectors on the GPU against the CPU provider's; the retriever."""
import os
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_maxsim_kernel import exact_and_bound  # noqa: E402
from test_late_interaction import DIM, Boost, ScriptedProvider, chunk, ranked  # noqa: E402

from rag_dpo_amd import late_interaction as LI  # noqa: E402

pytestmark = pytest.mark.gpu


def world(n=40, stored=lambda i: True):
    chunks = [chunk(i, " ".join(f"mot{(i * 7 + j) % 53}" for j in range(20 + (i * 11) % 50)), heading="Titre" if i % 3 == 0 else "",
                    tags="cookies" if i % 4 == 0 else "") for i in range(n)]
    prov = ScriptedProvider()
    cpu = LI.LateInteractionReranker(prov, LI.MultiVectorStore(DIM, "cpu"))
    gpu = LI.LateInteractionReranker(prov, LI.MultiVectorStore(DIM, "cuda"))
    held = [c for i, c in enumerate(chunks) if stored(i)]
    cpu.index_chunks(held)
    gpu.index_chunks(held)
    assert len(gpu.store) == len(held) and gpu.store.get(held[-1].chunk_id).tobytes() == cpu.store.get(held[-1].chunk_id).tobytes()
    return chunks, prov, cpu, gpu


def check_question(prov, cpu, query, chunks, boosts, got, want):
    """the model's finals are separated by more than twice the largest pair bound -> same order, same count, scores within the bound"""
    if not chunks:
        assert got == [] and want == []
        return
    qv = prov.vectors(query)
    pairs = [exact_and_bound(qv, prov.vectors(cpu.chunk_text(c))) for c in chunks]
    final = np.asarray([e for e, _ in pairs]) + (np.asarray(boosts) if boosts is not None else 0.0)
    worst = max(b for _, b in pairs)
    gaps = np.diff(np.sort(final))
    assert len(final) < 2 or gaps.min() > 2 * worst, (gaps.min(), worst)                 # asserted on the model's numbers first
    assert [r.chunk_id for r in got] == [r.chunk_id for r in want] and [r.original_rank for r in got] == [r.original_rank for r in want]
    for r in got:
        e, b = pairs[r.original_rank]
        f = final[r.original_rank]
        assert abs(r.rerank_score - f) <= b + 2.0 ** -53 * abs(f), (r.chunk_id, r.rerank_score, f, b)   # (the boost is one fp64 add)


@pytest.mark.parametrize("boosted", [False, True])
@pytest.mark.parametrize("half_missing", [False, True])
def test_ranking_equals_the_cpu_reranker(boosted, half_missing):
    chunks, prov, cpu, gpu = world(stored=(lambda i: i % 2 == 0) if half_missing else (lambda i: True))
    matcher, topics = (Boost(), ["cookies"]) if boosted else (None, None)
    boosts = [Boost().topic_boost(["cookies"], c.metadata["rgpd_topics"]) for c in chunks] if boosted else None
    before = gpu.store.stats()
    # 1 question x 40 candidates
    q = "transfert hors union européenne"        # (the model's closest finals of each question here lie 3e-5 or more apart, the bound is 4e-7)
    got = gpu.rerank(q, chunks, top_k=10, topic_matcher=matcher, question_topics=topics)
    want = cpu.rerank(q, chunks, top_k=10, topic_matcher=matcher, question_topics=topics)
    assert len(got) == 10 and gpu.last_rerank_stats["path"] == "maxsim" and gpu.last_rerank_stats["device_calls"] == 1
    assert gpu.last_rerank_stats["encoded"] == cpu.last_rerank_stats["encoded"] == (20 if half_missing else 0)
    assert gpu._model.calls == (2 if half_missing else 1)
    check_question(prov, cpu, q, chunks, boosts, got, want)
    # 3 questions x (0, 1, 40) candidates: one encode of the questions, at most two kernel calls, one selection launch
    queries = ["registre des traitements", "cookies et traceurs publicitaires", q]
    lists = [[], chunks[5:6], chunks]
    tq = [topics, None, topics]
    prov.calls.clear()
    got = gpu.rerank_batch(queries, lists, top_k=10, topic_matcher=matcher, question_topics=tq)
    assert prov.calls[0] == queries[1:] and len(prov.calls) == (2 if half_missing else 1)
    assert gpu.last_rerank_stats["device_calls"] == 1 and gpu.last_rerank_stats["questions"] == 2 and gpu._model.calls <= 2
    want = cpu.rerank_batch(queries, lists, top_k=10, topic_matcher=matcher, question_topics=tq)
    for i in range(3):
        b = None if (boosts is None or tq[i] is None) else [boosts[chunks.index(c)] for c in lists[i]]
        check_question(prov, cpu, queries[i], lists[i], b, got[i], want[i])
    assert [len(g) for g in got] == [0, 1, 10]
    # rerank_batch equals the loop of rerank exactly: a pair's bits do not depend on the call it is in
    loop = [gpu.rerank(qq, cc, top_k=10, topic_matcher=matcher, question_topics=t) for qq, cc, t in zip(queries, lists, tq)]
    assert [ranked(g) for g in got] == [ranked(x) for x in loop]
    assert gpu.store.stats() == before                                                   # nothing encoded on the fly was stored


def test_store_on_the_gpu_compacts_saves_and_loads(tmp_path):
    rng = np.random.default_rng(1)
    unit = lambda n: (lambda v: (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float16))(rng.standard_normal((n, DIM)))   # noqa: E731
    st = LI.MultiVectorStore(DIM, "cuda")
    mats = {f"c{i}": unit(n) for i, n in enumerate((40, 3, 65, 1))}
    st.add(list(mats), [torch.from_numpy(m).cuda() for m in mats.values()])
    mats["c0"] = unit(2)
    st.add(["c0"], [mats["c0"]])                                                         # dead 40 < live 71: no compaction yet
    assert st.stats()["dead_tokens"] == 40
    st.delete(["c2"])                                                                     # dead 105 > live 6: compacts by itself
    del mats["c2"]
    assert st.stats()["dead_tokens"] == 0 and st.stats()["live_tokens"] == 6 and st.slots_of(["c0", "c1", "c2", "c3"]).tolist() == [0, 1, -1, 3]
    for k, m in mats.items():
        assert st.get(k).tobytes() == m.tobytes()
    arena, start, length = st.tables()
    assert arena.is_cuda and start.is_cuda and length.tolist() == [2, 3, 0, 1]
    st.save(str(tmp_path / "mv"))
    back = LI.MultiVectorStore.load(str(tmp_path / "mv"), "cuda")
    assert back.slots_of(["c0", "c1", "c2", "c3"]).tolist() == [0, 1, -1, 3]
    for k, m in mats.items():
        assert back.get(k).tobytes() == m.tobytes()
    # a deleted slot scores NaN, the live ones as the model says
    q = unit(4)
    from rag_dpo_amd import engine
    s = engine.maxsim(torch.from_numpy(q).cuda(), torch.tensor([0, 4], dtype=torch.int32).pin_memory(), *back.tables(),
                      torch.zeros(4, dtype=torch.int32).cuda(), torch.arange(4).cuda()).cpu().numpy()
    assert np.isnan(s[2]) and np.isfinite(s[[0, 1, 3]]).all()
    for slot, k in ((0, "c0"), (1, "c1"), (3, "c3")):
        e, b = exact_and_bound(q, mats[k])
        assert abs(float(s[slot]) - e) <= b


def test_embed_tokens_device_against_the_cpu_provider():
    from rag_dpo_amd.embedding_provider import EmbeddingProvider
    g = torch.Generator().manual_seed(7)
    rng = np.random.default_rng(3)
    words = [f"w{i}" for i in range(300)]
    texts = [" ".join(rng.choice(words, size=int(n))) for n in (5, 1, 17, 60, 2, 150)] + [""]

    def make(name, device, dtype, head, fused=None):
        p = EmbeddingProvider(model_name=name, device=device, dtype=dtype, batch_size=4, colbert_head=head)
        p.fused_kernels = fused
        return p.load()

    # the tiny model: fp16 on the GPU (torch operations: 16-wide heads) against fp32 on the CPU, tests/test_embedding_provider.py's 3e-3
    head = (torch.randn((DIM, 64), generator=g) * 0.125, torch.randn((DIM,), generator=g) * 0.1)
    want = make("random-init:tiny", "cpu", torch.float32, head).embed_tokens(texts)
    v, off = make("random-init:tiny", "cuda", torch.float16, head).embed_tokens_device(texts)
    assert v.is_cuda and v.dtype == torch.float16 and off.tolist() == np.cumsum([0] + [len(w) for w in want]).tolist()
    got = v.cpu().numpy().astype(np.float32)
    assert np.abs(got - np.concatenate(want).astype(np.float32)).max() < 3e-3
    assert np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1).max() < 2e-3
    # the mid model: librdx's encoder kernels (VALU and MFMA attention, every row behind the last attention) against the torch
    # operations on the same GPU, that file's 2e-3 for the fused forward
    head = (torch.randn((DIM, 512), generator=g) * 0.05, torch.randn((DIM,), generator=g) * 0.1)
    fast, plain = make("random-init:mid", "cuda", torch.float16, head), make("random-init:mid", "cuda", torch.float16, head, fused=False)
    assert fast._packed.fused and not plain._packed.fused
    for batch in (texts, texts[:3], ["w1 w2 w3"]):                                       # long texts (MFMA attention), short ones, one question
        a, oa = fast.embed_tokens_device(batch)
        b, ob = plain.embed_tokens_device(batch)
        assert oa.tolist() == ob.tolist() and float((a.float() - b.float()).abs().max()) <= 2e-3
    cls = fast.embed_device(["w1 w2 w3"]).clone()                                        # cls() and its graphs are untouched by tokens()
    fast.embed_tokens_device(["w1 w2 w3"])
    assert torch.equal(fast.embed_device(["w1 w2 w3"]), cls)


def test_retrieve_reranked_batch_equals_the_loop():
    from rag_dpo_amd.retriever import DenseRetriever
    rng = np.random.default_rng(9)
    n, d = 120, 16
    emb = rng.standard_normal((n, d)).astype(np.float32)
    emb /= np.linalg.norm(emb, axis=1, keepdims=True)
    metas = [{"document_path": f"doc_{i % 11}", "chunk_nature": ["GUIDE", "DOCTRINE"][i % 2], "chunk_index": i // 11, "heading": "T" if i % 3 else "",
              "rgpd_topics": "cookies" if i % 5 == 0 else ""} for i in range(n)]

    class HostCollection:
        def query(self, query_embeddings, n_results, where=None, include=None):
            out = {"ids": [], "documents": [], "metadatas": [], "distances": []}
            for q in query_embeddings:
                q = np.asarray(q, dtype=np.float32)
                dist = 1.0 - emb @ (q / np.linalg.norm(q))
                rows = [i for i in np.argsort(dist, kind="stable") if where is None or metas[i]["chunk_nature"] == where["chunk_nature"]][:n_results]
                out["ids"].append([f"chunk_{i}" for i in rows])
                out["documents"].append([f"texte {i} conservation mot{i % 7} mot{i % 13}" for i in rows])
                out["metadatas"].append([metas[i] for i in rows])
                out["distances"].append([float(dist[i]) for i in rows])
            return out

    class Dense:
        def embed(self, texts):
            return [list(np.random.default_rng(zlib.crc32(t.encode())).standard_normal(d)) for t in texts]

    ret = DenseRetriever(HostCollection(), Dense())
    rr = LI.LateInteractionReranker(ScriptedProvider(), LI.MultiVectorStore(DIM, "cuda"))
    queries = ["durée de conservation", "cookies et traceurs", "registre"]
    wheres = [None, {"chunk_nature": "GUIDE"}, {"chunk_nature": "ABSENT"}]
    topics = [["cookies"], None, ["cookies"]]
    rr.index_chunks(ret.retrieve_candidates(queries[0], n_candidates=40)[:25])
    got = ret.retrieve_reranked_batch(queries, rr, n_candidates=40, top_k=10, where_filter=wheres, topic_matcher=Boost(), question_topics=topics)
    assert rr.last_rerank_stats["device_calls"] == 1 and rr.last_rerank_stats["encoded"] > 0
    want = [ret.retrieve_reranked(q, rr, n_candidates=40, top_k=10, where_filter=w, topic_matcher=Boost(), question_topics=t)
            for q, w, t in zip(queries, wheres, topics)]
    assert got == want and got[2] == [] and sum(len(x.chunks) for x in got[0]) == 10
