"""CPU: late-interaction rerank (rag_dpo_amd/late_interaction.py) — the numpy model, MultiVectorStore, the provider's
token vectors and LateInteractionReranker on a CPU store (which scores through the model)."""
import os
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import enc_reference as ER  # noqa: E402

from rag_dpo_amd import late_interaction as LI  # noqa: E402
from rag_dpo_amd.reranker import select_host  # noqa: E402
from rag_dpo_amd.retriever import RetrievedChunk  # noqa: E402

DIM = 32


def unit16(rng, n, dim=DIM):
    v = rng.standard_normal((n, dim))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float16)


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def triple_loop(q, d):
    total = 0.0
    for i in range(q.shape[0]):
        best = -np.inf
        for j in range(d.shape[0]):
            s = 0.0
            for k in range(q.shape[1]):
                s += float(q[i, k]) * float(d[j, k])
            best = max(best, s)
        total += best
    return np.float32(total / q.shape[0])


def test_model_equals_the_triple_loop():
    rng = np.random.default_rng(0)
    for nq, nd, dim in ((1, 1, 32), (3, 5, 32), (7, 2, 64)):
        # (small integers over 8: every product and sum is exact in fp64, so the two summation orders cannot differ)
        q = (rng.integers(-8, 9, size=(nq, dim)) / 8.0).astype(np.float16)
        d = (rng.integers(-8, 9, size=(nd, dim)) / 8.0).astype(np.float16)
        got = LI.maxsim_model(q, d)
        assert got.dtype == np.float32 and got.tobytes() == triple_loop(q, d).tobytes()


def test_all_negative_similarities_give_a_negative_score():
    q = np.zeros((3, DIM), dtype=np.float16)
    d = np.zeros((4, DIM), dtype=np.float16)
    q[:, 0] = 1.0
    d[:, 0] = [-0.5, -0.25, -1.0, -0.75]
    assert LI.maxsim_model(q, d) == np.float32(-0.25)            # the largest of the negatives, not the 0 of a padded row


def test_pairs_model_marks_what_is_out_of_range():
    rng = np.random.default_rng(1)
    qv, dv = unit16(rng, 5), unit16(rng, 9)
    q_off = np.array([0, 2, 5], dtype=np.int32)
    start, length = np.array([0, 4, 7, 8], dtype=np.int64), np.array([4, 3, 2, 0], dtype=np.int32)
    got = LI.maxsim_pairs(qv, q_off, dv, start, length, np.array([0, 1, 2, -1, 0, 1, 0], dtype=np.int32), np.array([0, 1, 0, 0, 4, 2, 3], dtype=np.int64))
    assert got[0] == LI.maxsim_model(qv[0:2], dv[0:4]) and got[1] == LI.maxsim_model(qv[2:5], dv[4:7]) and got[5] == LI.maxsim_model(qv[2:5], dv[7:9])
    assert np.isnan(got[[2, 3, 4, 6]]).all()


# ---- the store ------------------------------------------------------------------------------------------------------------------------
def test_store_add_replace_delete_compact():
    rng = np.random.default_rng(2)
    st = LI.MultiVectorStore(DIM, "cpu")
    mats = {f"c{i}": unit16(rng, n) for i, n in enumerate((3, 1, 7, 2))}
    st.add(list(mats), list(mats.values()))
    assert len(st) == 4 and "c2" in st and "zz" not in st
    assert st.slots_of(["c0", "zz", "c3", "c1"]).tolist() == [0, -1, 3, 1]
    assert st.stats()["live_tokens"] == 13 and st.stats()["dead_tokens"] == 0 and st.stats()["slots"] == 4
    assert st.stats()["bytes"] >= 13 * DIM * 2
    for k, m in mats.items():
        assert st.get(k).tobytes() == m.tobytes()
    # replace keeps the slot, the old rows are dead
    mats["c1"] = unit16(rng, 2)
    st.add(["c1"], (mats["c1"], np.array([0, 2])))                # the (vecs, off) form
    assert st.slots_of(["c1"]).tolist() == [1] and st.stats()["dead_tokens"] == 1 and st.stats()["live_tokens"] == 14
    assert st.get("c1").tobytes() == mats["c1"].tobytes()
    # delete frees the slot for a later add; absent ids are ignored
    st.delete(["c0", "nope"])
    assert len(st) == 3 and "c0" not in st and st.slots_of(["c0"]).tolist() == [-1] and st.stats()["dead_tokens"] == 4
    st.compact()
    assert st.stats()["dead_tokens"] == 0 and st.stats()["live_tokens"] == 11
    arena, start, length = st.tables()
    assert arena.shape == (11, DIM) and length.tolist() == [0, 2, 7, 2] and start[1:].tolist() == [0, 2, 9]
    for k in ("c1", "c2", "c3"):
        assert st.get(k).tobytes() == mats[k].tobytes()
    mats["c9"] = unit16(rng, 4)
    st.add(["c9"], [mats["c9"]])
    assert st.slots_of(["c9"]).tolist() == [0]                    # the freed slot
    with pytest.raises(ValueError):
        st.add(["bad"], [np.zeros((0, DIM), dtype=np.float16)])    # a text always has at least one vector
    with pytest.raises(ValueError):
        st.add(["bad"], [np.zeros((2, DIM + 32), dtype=np.float16)])
    with pytest.raises(ValueError):
        LI.MultiVectorStore(48)


def test_compaction_triggers_by_itself():
    rng = np.random.default_rng(3)
    st = LI.MultiVectorStore(DIM)
    st.add(["a", "b"], [unit16(rng, 10), unit16(rng, 4)])
    new = unit16(rng, 3)
    st.add(["a"], [new])                                          # dead 10 > live 7: compacts
    s = st.stats()
    assert s["dead_tokens"] == 0 and s["live_tokens"] == 7 and st.tables()[0].shape[0] == 7
    assert st.get("a").tobytes() == new.tobytes() and st.slots_of(["a", "b"]).tolist() == [0, 1]
    st.delete(["b"])                                              # dead 4 > live 3
    assert st.stats()["dead_tokens"] == 0 and st.tables()[0].shape[0] == 3


def test_save_load_keeps_slots_and_bits(tmp_path):
    rng = np.random.default_rng(4)
    st = LI.MultiVectorStore(DIM)
    mats = {f"c{i}": unit16(rng, n) for i, n in enumerate((5, 2, 9, 1, 3))}
    st.add(list(mats), list(mats.values()))
    st.delete(["c1"])
    st.add(["c3"], [unit16(rng, 2)])
    mats["c3"] = st.get("c3")
    del mats["c1"]
    st.save(str(tmp_path / "mv"))
    assert sorted(os.listdir(tmp_path / "mv")) == ["slots.npy", "store.json", "vecs.npy"]
    back = LI.MultiVectorStore.load(str(tmp_path / "mv"), "cpu")
    assert len(back) == 4 and back.dim == DIM and back.stats() ["dead_tokens"] == 0
    assert back.slots_of(list(mats) + ["c1"]).tolist() == st.slots_of(list(mats) + ["c1"]).tolist() == [0, 2, 3, 4, -1]
    for k, m in mats.items():
        assert back.get(k).tobytes() == m.tobytes()
    back.add(["new"], [unit16(rng, 1)])
    assert back.slots_of(["new"]).tolist() == [1]                 # the free slot survived the round trip


# ---- the provider ---------------------------------------------------------------------------------------------------------------------
def tiny_provider(head="random", packed=True, batch_size=512):
    from rag_dpo_amd.embedding_provider import EmbeddingProvider
    kw = {}
    if head == "random":
        g = torch.Generator().manual_seed(7)
        kw["colbert_head"] = (torch.randn((DIM, 64), generator=g) * 0.125, torch.randn((DIM,), generator=g) * 0.1)
    elif head is not None:
        kw["colbert_head"] = head
    p = EmbeddingProvider(model_name="random-init:tiny", device="cpu", dtype=torch.float32, batch_size=batch_size, **kw)
    p.packed_forward = packed
    return p.load()


def test_embed_tokens_against_the_module_forward(tmp_path):
    rng = np.random.default_rng(9)
    words = [f"w{i}" for i in range(300)]
    texts = [" ".join(rng.choice(words, size=int(n))) for n in (5, 1, 17, 60, 2)] + ["", " ".join(rng.choice(words, size=200))]
    p = tiny_provider()
    w, b = p._colbert
    tok = p._tokenizer
    want = []
    with torch.no_grad():
        for t in texts:                                           # one text at a time: no padding involved
            enc = tok([t])
            h = p._model(**enc).last_hidden_state[0, 1:].to(torch.float32)
            v = torch.nn.functional.linear(h, w, b)
            want.append((v / v.norm(dim=1, keepdim=True).clamp_min(1e-12)).numpy().astype(np.float64))
    for prov in (p, tiny_provider(batch_size=3), tiny_provider(packed=False, batch_size=4)):
        assert (prov._packed is None) == (prov is not p and prov.batch_size == 4)
        got = prov.embed_tokens(texts)
        assert len(got) == len(texts)
        for t, g, r in zip(texts, got, want):
            assert g.dtype == np.float16 and g.shape == (len(t.split()) + 1, DIM)       # len - 1 rows: every token but <s>, </s> kept
            # tests/test_embedding_provider.py's tolerance for the packed forward (2e-5), then the one rounding to fp16
            assert (np.abs(g.astype(np.float64) - r) <= ER.round16_bound(r, 2e-5)).all(), float(np.abs(g - r).max())
        v, off = prov.embed_tokens_device(texts)
        assert v.dtype == torch.float16 and off.dtype == np.int64 and off.tolist() == np.cumsum([0] + [len(t.split()) + 1 for t in texts]).tolist()
        assert np.concatenate(got).tobytes() == v.numpy().tobytes()
    assert got[5].shape == (1, DIM)                               # "" is <s></s>: one vector, never an empty list
    # input order is kept, and a text's vectors do not depend on its neighbours beyond the forward's tolerance
    rev = p.embed_tokens(texts[::-1])[::-1]
    for a, c in zip(p.embed_tokens(texts), rev):
        assert a.shape == c.shape and np.abs(a.astype(np.float32) - c.astype(np.float32)).max() <= 2 * 2.0 ** -11
    v0, off0 = p.embed_tokens_device([])
    assert v0.shape == (0, DIM) and off0.tolist() == [0]
    # the head from a file
    torch.save({"weight": w, "bias": b}, str(tmp_path / "colbert_linear.pt"))
    filed = tiny_provider(head=str(tmp_path / "colbert_linear.pt"))
    assert filed.embed_tokens(texts[:2])[0].tobytes() == p.embed_tokens(texts[:2])[0].tobytes()
    with pytest.raises(ValueError, match="colbert_head"):
        tiny_provider(head=(torch.zeros((DIM, 48)), torch.zeros(DIM)))


def test_a_missing_head_raises_and_leaves_the_rest_alone():
    p = tiny_provider(head=None)
    for fn in (p.embed_tokens, p.embed_tokens_device):
        with pytest.raises(RuntimeError, match="colbert_linear.pt"):
            fn(["bonjour"])
    assert p.embed_device(["bonjour"]).shape == (1, 64)


# ---- the reranker ---------------------------------------------------------------------------------------------------------------------
class ScriptedProvider:
    """token vectors from the text alone: len(words) + 1 unit rows seeded by the text"""

    def __init__(self, dim=DIM):
        self.dim, self.calls = dim, []

    def vectors(self, text):
        return unit16(np.random.default_rng(zlib.crc32(text.encode())), len(text.split()) + 1, self.dim)

    def embed_tokens_device(self, texts):
        self.calls.append(list(texts))
        mats = [self.vectors(t) for t in texts]
        off = np.zeros(len(texts) + 1, dtype=np.int64)
        np.cumsum([len(m) for m in mats], out=off[1:])
        return torch.from_numpy(np.concatenate(mats) if mats else np.zeros((0, self.dim), dtype=np.float16)), off


def chunk(i, text, heading="", tags=""):
    return RetrievedChunk(chunk_id=f"chunk_{i}", text=text, document_path=f"doc_{i % 4}", chunk_nature="GUIDE", chunk_index=i, confidence="high",
                          distance=0.1 * i, metadata={"heading": heading, "rgpd_topics": tags})


class Boost:
    def topic_boost(self, topics, tags):
        return 0.15 if tags == topics[0] else 0.0


def make_world(n=12):
    chunks = [chunk(i, " ".join(f"mot{(i * 7 + j) % 23}" for j in range(3 + i % 5)), heading="Titre" if i % 3 == 0 else "",
                    tags="cookies" if i % 4 == 0 else "") for i in range(n)]
    prov = ScriptedProvider()
    store = LI.MultiVectorStore(DIM)
    rr = LI.LateInteractionReranker(prov, store)
    return chunks, prov, store, rr


def expected(rr, prov, query, chunks, top_k, boosts=None, min_score=float("-inf")):
    qv = prov.vectors(query)
    scores = [LI.maxsim_model(qv, prov.vectors(rr.chunk_text(c))) for c in chunks]
    order, final, count = select_host(scores, boosts, top_k, min_score)
    return [(chunks[i].chunk_id, final[i], i) for i in order[:count]]


def ranked(out):
    return [(r.chunk_id, r.rerank_score, r.original_rank) for r in out]


def test_cpu_reranker_equals_the_model_plus_select_host():
    chunks, prov, store, rr = make_world()
    assert rr.chunk_text(chunks[0]) == "Titre\n" + chunks[0].text and rr.chunk_text(chunks[1]) == chunks[1].text
    long = chunk(99, "x" * 5000)
    assert len(rr.chunk_text(long)) == rr.max_length * 4
    assert rr.index_chunks(chunks) == len(chunks) == len(store)
    assert store.get("chunk_3").tobytes() == prov.vectors(rr.chunk_text(chunks[3])).tobytes()
    prov.calls.clear()
    q = "durée de conservation des cookies"
    out = rr.rerank(q, chunks, top_k=5)
    assert ranked(out) == expected(rr, prov, q, chunks, 5) and len(out) == 5
    assert prov.calls == [[q]] and rr.last_rerank_stats["encoded"] == 0 and rr.last_rerank_stats["path"] == "maxsim-model"
    assert all(-1.0 <= r.rerank_score <= 1.0 for r in out)
    # boosts, and a min_score that cuts (the keep-3 rule still holds)
    boosts = [Boost().topic_boost(["cookies"], c.metadata["rgpd_topics"]) for c in chunks]
    assert ranked(rr.rerank(q, chunks, top_k=8, topic_matcher=Boost(), question_topics=["cookies"])) == expected(rr, prov, q, chunks, 8, boosts)
    cut = LI.LateInteractionReranker(prov, store, min_score=0.99)
    assert ranked(cut.rerank(q, chunks, top_k=8)) == expected(rr, prov, q, chunks, 8, None, 0.99) and len(cut.rerank(q, chunks, top_k=8)) == 3
    assert rr.min_score == float("-inf") and rr.is_loaded
    with pytest.raises(ValueError, match="store lives on"):
        LI.LateInteractionReranker(prov, store, device="cuda")


def test_missing_candidates_are_encoded_and_not_stored():
    chunks, prov, store, rr = make_world()
    rr.index_chunks(chunks[::2])
    before = store.stats()
    prov.calls.clear()
    q = "registre des traitements"
    out = rr.rerank(q, chunks + [chunks[1]], top_k=20)            # chunk_1 is missing and listed twice: encoded once
    assert ranked(out) == expected(rr, prov, q, chunks + [chunks[1]], 20)
    assert rr.last_rerank_stats["encoded"] == 6 and len(prov.calls) == 2 and len(prov.calls[1]) == 6
    assert store.stats() == before and "chunk_1" not in store
    assert rr._model.calls == 2                                   # stored candidates from the arena, the others from the scratch arena


def test_rerank_batch_equals_the_loop_and_takes_an_empty_list():
    chunks, prov, store, rr = make_world(20)
    rr.index_chunks(chunks[:15])
    queries = ["durée de conservation", "cookies et traceurs", "registre", "durée de conservation"]
    lists = [chunks[:8], [], chunks[10:20], chunks[3:4]]
    topics = [["cookies"], None, ["cookies"], None]
    got = rr.rerank_batch(queries, lists, top_k=4, topic_matcher=Boost(), question_topics=topics)
    assert rr.last_rerank_stats["encoded"] == 5
    want = [rr.rerank(q, c, top_k=4, topic_matcher=Boost(), question_topics=t) for q, c, t in zip(queries, lists, topics)]
    assert [ranked(g) for g in got] == [ranked(w) for w in want]
    assert got[1] == [] and len(got[0]) == 4 and len(got[3]) == 1 and rr.rerank("x", []) == []


def test_fallback_when_the_scoring_fails():
    chunks, prov, store, rr = make_world()

    class Broken:
        def embed_tokens_device(self, texts):
            raise RuntimeError("no head")

    bad = LI.LateInteractionReranker(Broken(), store)
    out = bad.rerank("q", chunks, top_k=4)
    assert ranked(out) == [(c.chunk_id, c.similarity_score, i) for i, c in enumerate(chunks[:4])]
    assert bad.last_rerank_stats["path"] == "fallback"
    assert [ranked(x) for x in bad.rerank_batch(["q", "r"], [chunks[:2], chunks], top_k=3)] == \
        [[(c.chunk_id, c.similarity_score, i) for i, c in enumerate(cs[:3])] for cs in (chunks[:2], chunks)]


def test_dense_retriever_takes_the_new_reranker():
    from rag_dpo_amd.retriever import DenseRetriever, RetrievedDocument
    rng = np.random.default_rng(9)
    n, d = 60, 16
    emb = rng.standard_normal((n, d)).astype(np.float32)
    emb /= np.linalg.norm(emb, axis=1, keepdims=True)
    metas = [{"document_path": f"doc_{i % 7}", "chunk_nature": "GUIDE", "chunk_index": i // 7, "heading": "T" if i % 2 else ""} for i in range(n)]

    class HostCollection:
        def query(self, query_embeddings, n_results, where=None, include=None):
            out = {"ids": [], "documents": [], "metadatas": [], "distances": []}
            for q in query_embeddings:
                q = np.asarray(q, dtype=np.float32)
                dist = 1.0 - emb @ (q / np.linalg.norm(q))
                rows = list(np.argsort(dist, kind="stable")[:n_results])
                out["ids"].append([f"chunk_{i}" for i in rows])
                out["documents"].append([f"texte {i} conservation mot{i % 5}" for i in rows])
                out["metadatas"].append([metas[i] for i in rows])
                out["distances"].append([float(dist[i]) for i in rows])
            return out

    class Dense:
        def embed(self, texts):
            return [list(np.random.default_rng(zlib.crc32(t.encode())).standard_normal(d)) for t in texts]

    prov = ScriptedProvider()
    rr = LI.LateInteractionReranker(prov, LI.MultiVectorStore(DIM))
    ret = DenseRetriever(HostCollection(), Dense())
    cands = ret.retrieve_candidates("durée de conservation", n_candidates=20)
    rr.index_chunks(cands[:10])
    docs = ret.retrieve_reranked("durée de conservation", rr, n_candidates=20, top_k=6)
    assert all(isinstance(x, RetrievedDocument) for x in docs) and sum(len(x.chunks) for x in docs) == 6
    want = expected(rr, prov, "durée de conservation", cands, 6)
    assert sorted((c.chunk_id, c.hybrid_score) for x in docs for c in x.chunks) == sorted((cid, s) for cid, s, _ in want)
    both = ret.retrieve_reranked_batch(["durée de conservation", "cookies"], rr, n_candidates=20, top_k=6)
    assert both[0] == docs and both[1] == ret.retrieve_reranked("cookies", rr, n_candidates=20, top_k=6)
