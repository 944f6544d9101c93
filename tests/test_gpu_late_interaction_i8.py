"""GPU end to end: the int8 token-vector store on the GPU (rdx_maxsim_quantize_i8, rdx_maxsim_i8) against its CPU twin,
which quantises and scores through the numpy model, on a scripted provider: codes, scales, scores and finals equal bit for bit."""
import os
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_late_interaction import DIM, Boost, ScriptedProvider, chunk, ranked  # noqa: E402
from test_late_interaction_i8 import expected_i8  # noqa: E402

from rag_dpo_amd import late_interaction as LI  # noqa: E402

pytestmark = pytest.mark.gpu


def world(n=40, stored=lambda i: True):
    chunks = [chunk(i, " ".join(f"mot{(i * 7 + j) % 53}" for j in range(20 + (i * 11) % 50)), heading="Titre" if i % 3 == 0 else "",
                    tags="cookies" if i % 4 == 0 else "") for i in range(n)]
    prov = ScriptedProvider()
    cpu = LI.LateInteractionReranker(prov, LI.MultiVectorStore(DIM, "cpu", dtype="int8"))
    gpu = LI.LateInteractionReranker(prov, LI.MultiVectorStore(DIM, "cuda", dtype="int8"))
    held = [c for i, c in enumerate(chunks) if stored(i)]
    cpu.index_chunks(held)
    gpu.index_chunks(held)
    return chunks, prov, cpu, gpu, held


def same_codes(a, b, ids):
    for cid in ids:
        (ca, sa), (cb, sb) = a.get_codes(cid), b.get_codes(cid)
        assert ca.tobytes() == cb.tobytes() and sa.tobytes() == sb.tobytes(), cid
    return True


@pytest.mark.parametrize("boosted", [False, True])
@pytest.mark.parametrize("half_missing", [False, True])
def test_gpu_int8_store_equals_its_cpu_twin_on_bits(boosted, half_missing):
    chunks, prov, cpu, gpu, held = world(stored=(lambda i: i % 2 == 0) if half_missing else (lambda i: True))
    assert len(gpu.store) == len(held) and gpu.store.stats() == cpu.store.stats() and gpu.store.stats()["dtype"] == "int8"
    assert same_codes(gpu.store, cpu.store, [c.chunk_id for c in held])
    (codes, scales), start, length = gpu.store.tables()
    assert codes.is_cuda and codes.dtype == torch.int8 and scales.is_cuda and scales.dtype == torch.float32 and start.is_cuda
    matcher, topics = (Boost(), ["cookies"]) if boosted else (None, None)
    before = gpu.store.stats()
    q = "transfert hors union européenne"
    got = gpu.rerank(q, chunks, top_k=40, topic_matcher=matcher, question_topics=topics)
    want = cpu.rerank(q, chunks, top_k=40, topic_matcher=matcher, question_topics=topics)
    assert len(got) == 40 and ranked(got) == ranked(want)                                 # every score and every final, on bits (Python floats compare exactly)
    assert gpu.last_rerank_stats["path"] == "maxsim-i8" and cpu.last_rerank_stats["path"] == "maxsim-i8-model" and gpu.last_rerank_stats["device_calls"] == 1
    assert gpu.last_rerank_stats["encoded"] == cpu.last_rerank_stats["encoded"] == (20 if half_missing else 0)
    assert gpu._model.calls == (2 if half_missing else 1)
    # the model, pair by pair, from the provider's vectors: stored or scored from the scratch arena, a chunk scores the same
    boosts = [Boost().topic_boost(["cookies"], c.metadata["rgpd_topics"]) for c in chunks] if boosted else None
    assert ranked(got) == expected_i8(gpu, prov, q, chunks, 40, boosts)
    # 3 questions x (0, 1, 40) candidates: one encode of the questions, at most two kernel calls, one selection launch
    queries = ["registre des traitements", "cookies et traceurs publicitaires", q]
    lists = [[], chunks[5:6], chunks]
    tq = [topics, None, topics]
    prov.calls.clear()
    got = gpu.rerank_batch(queries, lists, top_k=10, topic_matcher=matcher, question_topics=tq)
    assert prov.calls[0] == queries[1:] and len(prov.calls) == (2 if half_missing else 1)
    assert gpu.last_rerank_stats["device_calls"] == 1 and gpu.last_rerank_stats["questions"] == 2 and gpu._model.calls <= 2
    want = cpu.rerank_batch(queries, lists, top_k=10, topic_matcher=matcher, question_topics=tq)
    assert [ranked(g) for g in got] == [ranked(w) for w in want] and [len(g) for g in got] == [0, 1, 10]
    assert gpu.store.stats() == before                                                    # nothing encoded on the fly was stored


def test_gpu_store_writes_files_and_to_int8(tmp_path):
    rng = np.random.default_rng(1)
    unit = lambda n: (lambda v: (v / np.linalg.norm(v, axis=1, keepdims=True) * np.exp(rng.uniform(-3, 3, size=(n, 1)))).astype(np.float16))(rng.standard_normal((n, DIM)))   # noqa: E731
    holds = lambda st, mats: all(st.get_codes(k)[0].tobytes() == LI.quantize_rows_model(m)[0].tobytes() and   # noqa: E731
                                 st.get_codes(k)[1].tobytes() == LI.quantize_rows_model(m)[1].tobytes() for k, m in mats.items())
    st, f16 = LI.MultiVectorStore(DIM, "cuda", dtype="int8"), LI.MultiVectorStore(DIM, "cuda")
    mats = {f"c{i}": unit(n) for i, n in enumerate((40, 3, 65, 1))}
    for s in (st, f16):
        s.add(list(mats), [torch.from_numpy(m).cuda() for m in mats.values()])
    mats["c0"] = unit(2)
    for s in (st, f16):
        s.add(["c0"], [mats["c0"]])                                                      # dead 40 < live 71: no compaction yet
    assert st.stats()["dead_tokens"] == 40 and holds(st, mats)
    bad = unit(5)
    bad[3, 4] = np.inf
    before = (st.stats(), st.tables()[0][0].cpu().numpy().tobytes(), st.tables()[0][1].cpu().numpy().tobytes())
    with pytest.raises(ValueError, match="non-finite"):
        st.add(["c1", "c7"], [torch.from_numpy(unit(2)).cuda(), torch.from_numpy(bad).cuda()])
    assert (st.stats(), st.tables()[0][0].cpu().numpy().tobytes(), st.tables()[0][1].cpu().numpy().tobytes()) == before and "c7" not in st
    for s in (st, f16):
        s.delete(["c2"])                                                                  # dead 105 > live 6: compacts by itself
    del mats["c2"]
    assert st.stats()["dead_tokens"] == 0 and st.stats()["live_tokens"] == 6 and st.slots_of(["c0", "c1", "c2", "c3"]).tolist() == [0, 1, -1, 3]
    assert holds(st, mats) and st.stats()["bytes"] < f16.stats()["bytes"]
    for k, m in mats.items():
        c, s = LI.quantize_rows_model(m)
        assert st.get(k).dtype == np.float32 and st.get(k).tobytes() == (c.astype(np.float32) * s[:, None]).tobytes()
    # to_int8() of the fp16 store: the same ids, slots, codes and scales as the store that was given the matrices
    conv = f16.to_int8()
    assert conv.on_gpu and conv.dtype == "int8" and holds(conv, mats) and conv.slots_of(["c0", "c1", "c2", "c3"]).tolist() == [0, 1, -1, 3]
    a, b = conv.tables(), st.tables()
    assert torch.equal(a[0][0], b[0][0]) and torch.equal(a[0][1].view(torch.int32), b[0][1].view(torch.int32)) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    # files: written from the GPU, read on both sides
    st.save(str(tmp_path / "mv8"))
    assert sorted(os.listdir(tmp_path / "mv8")) == ["codes.npy", "scales.npy", "slots.npy", "store.json"]
    for dev in ("cuda", "cpu"):
        back = LI.MultiVectorStore.load(str(tmp_path / "mv8"), dev)
        assert back.dtype == "int8" and back.on_gpu == (dev == "cuda") and back.slots_of(["c0", "c1", "c2", "c3"]).tolist() == [0, 1, -1, 3] and holds(back, mats)
    # a deleted slot scores NaN, the live ones as the model says, on bits
    from rag_dpo_amd import engine
    q = unit(4)
    cq, sq = engine.maxsim_quantize(torch.from_numpy(q).cuda())
    (codes, scales), start, length = LI.MultiVectorStore.load(str(tmp_path / "mv8"), "cuda").tables()
    s = engine.maxsim_i8(cq, sq, torch.tensor([0, 4], dtype=torch.int32).pin_memory(), codes, scales, start, length,
                         torch.zeros(4, dtype=torch.int32).cuda(), torch.arange(4).cuda()).cpu().numpy()
    assert np.isnan(s[2])
    for slot, k in ((0, "c0"), (1, "c1"), (3, "c3")):
        assert s[slot].tobytes() == LI.maxsim_i8_model(*LI.quantize_rows_model(q), *LI.quantize_rows_model(mats[k])).tobytes()
    assert codes.is_cuda and scales.is_cuda


def test_m3_reranker_with_an_int8_store_is_the_model_on_every_bit():
    from test_m3 import ScriptedM3, build_sources, make_chunks
    from rag_dpo_amd import m3 as M3
    chunks = make_chunks(40, long=True)
    prov = ScriptedM3()
    stored = lambda i: i % 2 == 0   # noqa: E731
    c_src, g_src = build_sources(prov, chunks, "cpu", stored), build_sources(prov, chunks, "cuda", stored)
    cpu = M3.M3Reranker(prov, c_src[0], c_src[1], c_src[2].to_int8(), device="cpu")
    gpu = M3.M3Reranker(prov, g_src[0], g_src[1], g_src[2].to_int8(), device="cuda")
    q = "transfert hors union européenne"
    got = gpu.rerank(q, chunks, top_k=40, topic_matcher=Boost(), question_topics=["cookies"])
    g_last = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in gpu._model.last.items()}
    want = cpu.rerank(q, chunks, top_k=40, topic_matcher=Boost(), question_topics=["cookies"])
    c_last = cpu._model.last
    assert gpu.last_rerank_stats["path"] == "m3" and gpu._model._maxsim.path == "maxsim-i8" and cpu._model._maxsim.path == "maxsim-i8-model"
    assert gpu.last_rerank_stats["encoded"] == cpu.last_rerank_stats["encoded"] == 20
    assert np.array_equal(g_last["dense"].view(np.uint32), c_last["dense"].view(np.uint32))
    assert np.array_equal(g_last["sparse"].view(np.uint64), c_last["sparse"].view(np.uint64))
    assert np.array_equal(g_last["colbert"].view(np.uint32), c_last["colbert"].view(np.uint32))      # with the fp16 store this component is within a bound only
    assert np.array_equal(g_last["value"].view(np.uint64), c_last["value"].view(np.uint64))
    assert np.array_equal(g_last["final"].view(np.uint32), c_last["final"].view(np.uint32))
    assert len(got) == 40 and ranked(got) == ranked(want)
    # the colbert component is the int8 model's, from the provider's vectors
    cq, sq = LI.quantize_rows_model(prov.vectors(q))
    for i in (0, 1, 17, 39):
        s = LI.maxsim_i8_model(cq, sq, *LI.quantize_rows_model(prov.vectors(gpu.chunk_text(chunks[i]))))
        assert g_last["colbert"][i].tobytes() == s.tobytes()


def test_retrieve_reranked_batch_runs_with_an_int8_store():
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
    rr = LI.LateInteractionReranker(ScriptedProvider(), LI.MultiVectorStore(DIM, "cuda", dtype="int8"))
    queries = ["durée de conservation", "cookies et traceurs", "registre"]
    wheres = [None, {"chunk_nature": "GUIDE"}, {"chunk_nature": "ABSENT"}]
    topics = [["cookies"], None, ["cookies"]]
    rr.index_chunks(ret.retrieve_candidates(queries[0], n_candidates=40)[:25])
    got = ret.retrieve_reranked_batch(queries, rr, n_candidates=40, top_k=10, where_filter=wheres, topic_matcher=Boost(), question_topics=topics)
    assert rr.last_rerank_stats["device_calls"] == 1 and rr.last_rerank_stats["encoded"] > 0 and rr.last_rerank_stats["path"] == "maxsim-i8"
    want = [ret.retrieve_reranked(q, rr, n_candidates=40, top_k=10, where_filter=w, topic_matcher=Boost(), question_topics=t)
            for q, w, t in zip(queries, wheres, topics)]
    assert got == want and got[2] == [] and sum(len(x.chunks) for x in got[0]) == 10
