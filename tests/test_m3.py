"""CPU: the combined BGE-M3 score (rag_dpo_amd/m3.py) — the numpy model against an independent restatement, the weight
rules, M3Reranker on CPU sources (a CPU store, lexical.model_factory, the oracle engine), Collection.score_pairs, embed_m3_device on
the CPU provider, and the posting lookup (csrc/lex_find.hpp) as a stand-alone program under the sanitizers."""
import os
import subprocess
import sys
import zlib
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle_engine import factory as oracle_factory  # noqa: E402
from test_late_interaction import DIM, Boost, chunk, ranked, unit16  # noqa: E402
from test_sanitizers import ENV, ROOT, SAN  # noqa: E402

from rag_dpo_amd import late_interaction as LI  # noqa: E402
from rag_dpo_amd import lexical as LX  # noqa: E402
from rag_dpo_amd import m3 as M3  # noqa: E402
from rag_dpo_amd.collection import Collection  # noqa: E402
from rag_dpo_amd.reranker import select_host  # noqa: E402

DDIM, VOCAB = 16, 997
LEXICON = ["cookies", "registre", "conservation", "durée", "transfert", "union", "traitements", "traceurs", "européenne", "hors"]


# ---- what the reranker tests share (test_gpu_m3.py too) ----------------------------------------------------------------------------
class ScriptedM3:
    """all three outputs from the text alone: a dense vector, token vectors (test_late_interaction's rule) and terms (one per word: id
    and weight from the word's crc32, through terms_model)"""
    lexical_vocab, lexical_special_ids = VOCAB, LX.XLMR_SPECIAL_IDS

    def __init__(self):
        self.calls = []

    def dense(self, text):
        return np.random.default_rng(zlib.crc32(("d" + text).encode())).standard_normal(DDIM).astype(np.float32) * 3.0

    def vectors(self, text):
        return unit16(np.random.default_rng(zlib.crc32(text.encode())), len(text.split()) + 1, DIM)

    def terms(self, text):
        crc = [zlib.crc32(w.encode()) for w in text.split()]
        return LX.terms_model([4 + c % (VOCAB - 4) for c in crc], [((c >> 8) % 63 + 1) / 16.0 for c in crc], VOCAB)

    def _tokens(self, texts):
        mats = [self.vectors(t) for t in texts]
        off = np.zeros(len(texts) + 1, dtype=np.int64)
        np.cumsum([len(m) for m in mats], out=off[1:])
        return torch.from_numpy(np.concatenate(mats) if mats else np.zeros((0, DIM), dtype=np.float16)), off

    def _lex(self, texts):
        t = [self.terms(x) for x in texts]
        off = np.zeros(len(texts) + 1, dtype=np.int64)
        np.cumsum([len(a) for a, _ in t], out=off[1:])
        cat = lambda i, dt: torch.from_numpy(np.concatenate([x[i] for x in t]).astype(dt) if t else np.zeros(0, dt))   # noqa: E731
        return cat(0, np.int32), cat(1, np.float16), off

    def embed_tokens_device(self, texts):
        self.calls.append(("tokens", list(texts)))
        return self._tokens(texts)

    def embed_lexical_device(self, texts):
        self.calls.append(("lex", list(texts)))
        return self._lex(texts)

    def embed_m3_device(self, texts, dense=True, sparse=True, colbert=True):
        self.calls.append(("m3", list(texts), dense, sparse, colbert))
        out = {}
        if dense:
            out["dense"] = torch.from_numpy(np.stack([self.dense(t) for t in texts]))
        if sparse:
            out["lex"] = self._lex(texts)
        if colbert:
            out["tokens"] = self._tokens(texts)
        return out


def text_of(c):
    """the reranker's text rule (LateInteractionReranker.chunk_text)"""
    h = c.metadata.get("heading", "")
    return (f"{h}\n{c.text}" if h else c.text)[:512 * 4]


def make_chunks(n, long=False):
    words = lambda i: [f"mot{(i * 7 + j) % 53}" for j in range((20 + (i * 11) % 50) if long else (3 + i % 5))]   # noqa: E731
    return [chunk(i, " ".join(words(i) + [LEXICON[(i + j) % len(LEXICON)] for j in range(1 + i % 3)]), heading="Titre" if i % 3 == 0 else "",
                  tags="cookies" if i % 4 == 0 else "") for i in range(n)]


def build_sources(prov, chunks, device, stored=lambda i: True):
    """-> (collection of every chunk's dense row, lexical index and token store of the chunks `stored` names) on "cpu" (the oracle engine,
    lexical.model_factory, a CPU store) or "cuda" (the product's engines)"""
    cpu = device == "cpu"
    col = Collection("m3_chunks", metadata={"hnsw:space": "cosine"}, **({"engine_factory": oracle_factory} if cpu else {}))
    col.add(ids=[c.chunk_id for c in chunks], embeddings=[prov.dense(text_of(c)).tolist() for c in chunks], documents=[c.text for c in chunks],
            metadatas=[{"document_path": c.document_path, "chunk_nature": "GUIDE", "chunk_index": c.chunk_index, "heading": c.metadata["heading"],
                        "rgpd_topics": c.metadata["rgpd_topics"], "confidence": "high"} for c in chunks])
    held = [c for i, c in enumerate(chunks) if stored(i)]
    ix = LX.LexicalChunkIndex(prov, engine_factory=LX.model_factory if cpu else None)
    ix.build_from_weights([c.chunk_id for c in held], [c.text for c in held], [{"document_path": c.document_path} for c in held],
                          [prov.terms(text_of(c)) for c in held])
    store = LI.MultiVectorStore(DIM, device)
    store.add([c.chunk_id for c in held], [prov.vectors(text_of(c)) for c in held])
    return col, ix, store


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def once(x: Fraction) -> float:
    return float(x)                     # Fraction -> float rounds once, to nearest even


def restated_value(dense, sparse, colbert, w):
    """the issue's definition with Python floats, every operation an exact Fraction rounded once"""
    total = once(Fraction(once(Fraction(w[0]) + Fraction(w[1]))) + Fraction(w[2]))
    acc = None
    for x, wi in zip((dense, sparse, colbert), w):
        if wi == 0:
            continue
        term = once(Fraction(wi) * Fraction(float(x)))
        acc = term if acc is None else once(Fraction(acc) + Fraction(term))
    return once(Fraction(acc) / Fraction(total))


def restated_sparse(q_terms, d_terms):
    d = {int(t): float(w) for t, w in zip(*d_terms)}
    s = 0.0
    for t, w in sorted((int(t), float(w)) for t, w in zip(*q_terms)):
        if t in d:
            s = once(Fraction(s) + Fraction(w) * Fraction(d[t]))     # the product is exact: only the sum rounds
    return s


def test_combine_model_equals_the_restatement():
    rng = np.random.default_rng(0)
    n = 300
    d = rng.uniform(-1, 1, n).astype(np.float32)
    s = rng.uniform(0, 40, n) * (1 + rng.uniform(0, 1, n) * 2.0 ** -30)
    c = rng.uniform(-1, 1, n).astype(np.float32)
    for w in ((0.4, 0.2, 0.4), (1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0.3, 0), (0, 0.7, 0.1), (3, 0, 1e-3)):
        parts = [x if wi else None for x, wi in zip((d, s, c), w)]
        value, final = M3.combine_model(*parts, w)
        assert value.dtype == np.float64 and final.dtype == np.float32
        want = np.array([restated_value(d[i], s[i], c[i], w) for i in range(n)])
        assert np.array_equal(value.view(np.uint64), want.view(np.uint64)), w
        assert np.array_equal(final.view(np.uint32), want.astype(np.float32).view(np.uint32))
    # unit weights reproduce the single component, cast to fp32
    for w, x in (((1, 0, 0), d), ((0, 1, 0), s), ((0, 0, 1), c)):
        parts = [p if wi else None for p, wi in zip((d, s, c), w)]
        assert np.array_equal(M3.combine_model(*parts, w)[1].view(np.uint32), x.astype(np.float32).view(np.uint32))
    # a NaN component gives NaN; one whose weight is 0 is never read
    d2 = d.copy()
    d2[3] = np.nan
    assert np.isnan(M3.combine_model(d2, s, c, (0.4, 0.2, 0.4))[0][3]) and not np.isnan(M3.combine_model(None, s, c, (0, 0.5, 0.5))[0][3])


def test_weight_rules_and_refusals():
    assert M3.check_weights(M3.DEFAULT_WEIGHTS) == (0.4, 0.2, 0.4) and M3.check_weights([1, 0, 0]) == (1.0, 0.0, 0.0)
    nan, inf = float("nan"), float("inf")
    for bad in ((nan, 0.2, 0.4), (0.4, 0.2, nan), (-0.1, 0.2, 0.4), (inf, 0, 0), (0, 0, 0), (1e308, 1e308, 1e308), (1, 1), (1, 1, 1, 1), "abc", None,
                (True, 1, 1)):
        with pytest.raises(ValueError):
            M3.check_weights(bad)
    x = np.zeros(2, np.float32)
    with pytest.raises(ValueError, match="dense"):
        M3.combine_model(None, x.astype(np.float64), x, (0.4, 0.2, 0.4))
    with pytest.raises(ValueError, match="sparse"):
        M3.combine_model(x, x.astype(np.float64), x, (0.4, 0.0, 0.4))


def test_sparse_pairs_model_equals_score_model_and_the_restatement():
    prov = ScriptedM3()
    chunks = make_chunks(12)
    _, ix, _ = build_sources(prov, chunks, "cpu")
    qs = ["durée de conservation des cookies", "registre des traitements", "", "transfert hors union européenne mot3"]
    ids, ws, off = prov._lex(qs)
    pq = np.repeat(np.arange(4), 12).astype(np.int32)
    rows = np.tile(ix.rows_of([c.chunk_id for c in chunks]), 4)
    got = M3.sparse_pairs_model(ix.arrays, off, ids.numpy(), ws.numpy(), pq, rows)
    k = 0
    for q in qs:
        for c in chunks:
            assert got[k] == LX.score_model(*prov.terms(q), *prov.terms(text_of(c))) == restated_sparse(prov.terms(q), prov.terms(text_of(c)))
            k += 1
    assert (got > 0).any() and (got[24:36] == 0).all()
    # the search's own scores, where it lists the row
    sc, ro, cn = ix.engine.search(off, ids.numpy(), ws.numpy(), 12)
    for b in range(4):
        assert sorted(ro[b, :cn[b]].tolist()) == np.flatnonzero(got[12 * b:12 * b + 12] > 0).tolist()
        assert np.array_equal(sc[b, :cn[b]].view(np.uint64), got[12 * b + ro[b, :cn[b]]].view(np.uint64))
    # out of range, and a bad question
    bad = M3.sparse_pairs_model(ix.arrays, np.array([0, 2, 4]), np.array([5, 5, 7, VOCAB]), np.array([1, 1, 1, 1], np.float16), [0, 1, -1, 2, 0], [0, 0, 0, 0, 12])
    assert np.isnan(bad).all()


# ---- Collection.score_pairs -----------------------------------------------------------------------------------------------------------
def test_score_pairs_equals_query_on_the_oracle_engine():
    rng = np.random.default_rng(5)
    n, dim = 70, 260
    col = Collection("c", metadata={"hnsw:space": "cosine"}, engine_factory=oracle_factory)
    col.add(ids=[f"id{i}" for i in range(n)], embeddings=(rng.standard_normal((n, dim)) * 2).astype(np.float32).tolist())
    col.delete(ids=["id7"])
    q = (rng.standard_normal((3, dim)) * np.array([[1.0], [1e3], [1e-3]])).astype(np.float32)
    res = col.query(query_embeddings=q.tolist(), n_results=n - 1, include=["distances"])
    pq = np.repeat(np.arange(3), n - 1).astype(np.int32)
    ids = [i for lst in res["ids"] for i in lst]
    got = col.score_pairs(q, pq, ids)
    assert got.dtype == np.float32 and got.shape == (3 * (n - 1),)
    dist = np.asarray([d for lst in res["distances"] for d in lst], dtype=np.float32)
    assert np.array_equal((np.float32(1.0) - got).astype(np.float32).view(np.uint32), dist.view(np.uint32))      # query()'s distances, bit for bit
    s, r, _ = col._engine.search(q, n)                                                                           # and the engine's scores themselves
    table = {(b, int(rr)): ss for b in range(3) for ss, rr in zip(s[b], r[b])}
    rows = col.rows_of(ids)
    assert all(got[k].tobytes() == np.float32(table[(int(pq[k]), rows[k])]).tobytes() for k in range(len(ids)))
    # unknown and deleted ids, a pair_query entry out of range
    odd = col.score_pairs(q, [0, 0, 1, 3, -1, 2], ["id3", "nope", "id7", "id3", "id3", "id69"])
    assert np.isnan(odd[[1, 2, 3, 4]]).all() and odd[0] == got[ids.index("id3")] and np.isfinite(odd[5])
    assert col.score_pairs(q, [], []).shape == (0,)
    with pytest.raises(ValueError):
        col.score_pairs(q, [0, 1], ["id3"])
    with pytest.raises(ValueError):
        col.score_pairs(q[:, :8], [0], ["id3"])
    with pytest.raises(NotImplementedError):
        col.score_pairs_device(q, [0], ["id3"])                      # the oracle engine has no device call
    with pytest.raises(TypeError):
        col.score_pairs(q, [0], ["id3"], where={"a": 1})             # it does not take `where`
    for space in ("ip", "l2"):
        other = Collection("o", metadata={"hnsw:space": space}, engine_factory=oracle_factory)
        other.add(ids=["a"], embeddings=[[1.0] * 8])
        with pytest.raises(NotImplementedError, match=space):
            other.score_pairs([[1.0] * 8], [0], ["a"])
    empty = Collection("e", metadata={"hnsw:space": "cosine"}, engine_factory=oracle_factory)
    assert np.isnan(empty.score_pairs([[1.0] * 8], [0], ["a"])).all()


# ---- the reranker ---------------------------------------------------------------------------------------------------------------------
def expected(prov, col, query, chunks, top_k, w=M3.DEFAULT_WEIGHTS, boosts=None, min_score=float("-inf"), in_lex=lambda c: True):
    """the definition, pair by pair, from the parts"""
    finals = []
    if w[0]:                                                      # the engine's own exact score of (query, row)
        s, r, _ = col._engine.search(prov.dense(query)[None, :], col.count())
        score_of = dict(zip(r[0].tolist(), s[0]))
    for c in chunks:
        dense = score_of[col.rows_of([c.chunk_id])[0]] if w[0] else None
        d_terms = prov.terms(text_of(c)) if in_lex(c) else (np.zeros(0, np.int32), np.zeros(0, np.float16))
        finals.append(M3.score_model(dense, prov.terms(query), d_terms, prov.vectors(query), prov.vectors(text_of(c)), w)[1])
    order, final, count = select_host(finals, boosts, top_k, min_score)
    return [(chunks[i].chunk_id, final[i], i) for i in order[:count]]


def test_cpu_reranker_equals_the_model():
    prov = ScriptedM3()
    chunks = make_chunks(12)
    col, ix, store = build_sources(prov, chunks, "cpu")
    rr = M3.M3Reranker(prov, col, ix, store)
    assert rr.weights == (0.4, 0.2, 0.4) and rr.min_score == float("-inf") and rr.is_loaded and rr.chunk_text(chunks[0]) == text_of(chunks[0])
    q = "durée de conservation des cookies"
    out = rr.rerank(q, chunks, top_k=5)
    assert prov.calls == [("m3", [q], True, True, True)]                                   # ONE call for the question, nothing else encoded
    assert ranked(out) == expected(prov, col, q, chunks, 5) and len(out) == 5
    assert rr.last_rerank_stats["path"] == "m3-model" and rr.last_rerank_stats["encoded"] == 0
    assert (rr._model.last["sparse"] > 0).any()
    boosts = [Boost().topic_boost(["cookies"], c.metadata["rgpd_topics"]) for c in chunks]
    assert ranked(rr.rerank(q, chunks, top_k=8, topic_matcher=Boost(), question_topics=["cookies"])) == expected(prov, col, q, chunks, 8, boosts=boosts)
    cut = M3.M3Reranker(prov, col, ix, store, min_score=1e9)                               # (the sparse part is not bounded by 1)
    assert ranked(cut.rerank(q, chunks, top_k=8)) == expected(prov, col, q, chunks, 8, min_score=1e9) and len(cut.rerank(q, chunks, top_k=8)) == 3   # the keep-3 rule
    # other weights; the batch equals the loop and encodes the distinct questions once
    for w in ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0.3, 0)):
        r2 = M3.M3Reranker(prov, col, ix, store, weights=w)
        assert ranked(r2.rerank(q, chunks, top_k=6)) == expected(prov, col, q, chunks, 6, w=w), w
    prov.calls.clear()
    queries, lists = [q, "registre des traitements", q], [chunks[:8], [], chunks[3:]]
    got = rr.rerank_batch(queries, lists, top_k=4)
    assert [ranked(g) for g in got] == [ranked(rr.rerank(a, b, top_k=4)) for a, b in zip(queries, lists)] and got[1] == []


def test_missing_candidates_fallback_and_none_sources():
    prov = ScriptedM3()
    chunks = make_chunks(12)
    col, ix, store = build_sources(prov, chunks, "cpu", stored=lambda i: i % 2 == 0)
    rr = M3.M3Reranker(prov, col, ix, store)
    q = "registre des traitements cookies"
    out = rr.rerank(q, chunks, top_k=12)
    # missing from the store: encoded on the fly (one more call) and not stored; missing from the lexical index: sparse +0.0
    assert rr.last_rerank_stats["encoded"] == 6 and [c[0] for c in prov.calls] == ["m3", "tokens"] and len(store) == 6
    assert ranked(out) == expected(prov, col, q, chunks, 12, in_lex=lambda c: int(c.chunk_id.split("_")[1]) % 2 == 0)
    assert (rr._model.last["sparse"][1::2] == 0).all() and (rr._model.last["sparse"][::2] > 0).any()
    # missing from the collection: the scoring raises, the reference's fallback answers
    stranger = chunk(999, "inconnu au bataillon")
    out = rr.rerank(q, chunks[:5] + [stranger], top_k=4)
    assert rr.last_rerank_stats["path"] == "fallback" and ranked(out) == [(c.chunk_id, c.similarity_score, i) for i, c in enumerate(chunks[:4])]
    with pytest.raises(ValueError, match="does not hold"):
        rr._model.predict(rr._pairs(q, [stranger]))
    # a source whose weight is 0 may be None; only the components with a weight are asked for
    prov.calls.clear()
    no_store = M3.M3Reranker(prov, col, ix, None, weights=(1, 0.3, 0))
    assert ranked(no_store.rerank(q, chunks, top_k=5)) == expected(prov, col, q, chunks, 5, w=(1, 0.3, 0), in_lex=lambda c: int(c.chunk_id.split("_")[1]) % 2 == 0)
    assert prov.calls == [("m3", [q], True, True, False)] and no_store.last_rerank_stats["encoded"] == 0
    only_colbert = M3.M3Reranker(prov, None, None, store, weights=(0, 0, 2))
    li = LI.LateInteractionReranker(prov, store)
    assert ranked(only_colbert.rerank(q, chunks[::2], top_k=4)) == ranked(li.rerank(q, chunks[::2], top_k=4))   # W divides out: x * 2 / 2
    for args, name in (((None, ix, store), "collection"), ((col, None, store), "lexical_index"), ((col, ix, None), "store")):
        with pytest.raises(ValueError, match=name):
            M3.M3Reranker(prov, *args)
    with pytest.raises(ValueError, match="store lives on"):
        M3.M3Reranker(prov, col, ix, store, device="cuda")
    with pytest.raises(ValueError):
        M3.M3Reranker(prov, col, ix, store, weights=(0, 0, 0))


def test_dense_retriever_takes_the_reranker():
    from rag_dpo_amd.retriever import DenseRetriever
    prov = ScriptedM3()
    chunks = make_chunks(30)
    col, ix, store = build_sources(prov, chunks, "cpu", stored=lambda i: i < 20)

    class Dense:
        def embed(self, texts):
            return [prov.dense(t).tolist() for t in texts]

    rr = M3.M3Reranker(prov, col, ix, store)
    ret = DenseRetriever(col, Dense())
    docs = ret.retrieve_reranked("durée de conservation", rr, n_candidates=20, top_k=6)
    assert sum(len(x.chunks) for x in docs) == 6 and rr.last_rerank_stats["path"] == "m3-model"
    both = ret.retrieve_reranked_batch(["durée de conservation", "cookies"], rr, n_candidates=20, top_k=6)
    assert both[0] == docs and both[1] == ret.retrieve_reranked("cookies", rr, n_candidates=20, top_k=6)


# ---- one forward, three outputs -------------------------------------------------------------------------------------------------------
def test_embed_m3_device_on_the_cpu_provider():
    from rag_dpo_amd.embedding_provider import EmbeddingProvider
    g = torch.Generator().manual_seed(7)
    heads = dict(colbert_head=(torch.randn((DIM, 64), generator=g) * 0.125, torch.randn((DIM,), generator=g) * 0.1),
                 sparse_head=(torch.randn((1, 64), generator=g) * 0.5, torch.zeros((1,))))
    rng = np.random.default_rng(9)
    words = [f"w{i}" for i in range(300)]
    texts = [" ".join(rng.choice(words, size=int(n))) for n in (5, 1, 17, 60, 2)] + ["", " ".join(rng.choice(words, size=200))]
    for packed, batch_size in ((True, 512), (True, 3), (False, 4)):
        p = EmbeddingProvider(model_name="random-init:tiny", device="cpu", dtype=torch.float32, batch_size=batch_size, **heads)
        p.packed_forward = packed
        p.load()
        calls = []
        inner = p._token_states
        p._token_states = lambda *a, **k: (calls.append(1), inner(*a, **k))[1]
        out = p.embed_m3_device(texts)
        assert len(calls) == 1 and sorted(out) == ["dense", "lex", "tokens"]                 # one _token_states call for the three outputs
        v, off = p.embed_tokens_device(texts)
        assert out["tokens"][0].numpy().tobytes() == v.numpy().tobytes() and out["tokens"][1].tolist() == off.tolist()
        ids, ws, loff = p.embed_lexical_device(texts)
        assert torch.equal(out["lex"][0], ids) and out["lex"][1].numpy().tobytes() == ws.numpy().tobytes() and out["lex"][2].tolist() == loff.tolist()
        want = p.embed_device(texts)
        assert out["dense"].dtype == torch.float32 and out["dense"].shape == want.shape == (len(texts), 64)
        assert torch.allclose(out["dense"], want, atol=2e-5, rtol=1e-5), float((out["dense"] - want).abs().max())   # tests/test_embedding_provider.py's fp32 tolerance
        assert sorted(p.embed_m3_device(texts[:2], sparse=False)) == ["dense", "tokens"]
        assert sorted(p.embed_m3_device(texts[:2], dense=False, colbert=False)) == ["lex"]
        empty = p.embed_m3_device([])
        assert empty["dense"].shape == (0, 64) and empty["tokens"][0].shape == (0, DIM) and empty["lex"][2].tolist() == [0]
    bare = EmbeddingProvider(model_name="random-init:tiny", device="cpu", dtype=torch.float32).load()
    with pytest.raises(RuntimeError, match="colbert_linear.pt"):
        bare.embed_m3_device(["bonjour"])
    with pytest.raises(RuntimeError, match="sparse_linear.pt"):
        bare.embed_m3_device(["bonjour"], colbert=False)
    assert sorted(bare.embed_m3_device(["bonjour"], sparse=False, colbert=False)) == ["dense"]


# ---- the posting lookup on the host ---------------------------------------------------------------------------------------------------
def test_lex_find_rehearsed_on_the_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "lex_find_host")
    subprocess.check_call(["g++", "-std=c++17", *SAN, "-Wall", "-Wextra", os.path.join(ROOT, "tests", "c_abi", "lex_find_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=ENV)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    for word in ("runtime error", "AddressSanitizer"):
        assert word not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok" and [line.split(":")[0] for line in lines[:-1]] == [f"length {n}" for n in (*range(10), 64, 4097)]
