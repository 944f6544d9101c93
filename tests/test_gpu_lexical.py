"""GPU: BGE-M3 lexical weights end to end — EmbeddingProvider.embed_lexical_device on cuda (k_lex_reduce behind the torch head) against the
model applied to the same token ids and the same fp32 head outputs; LexicalChunkIndex on librdx against the same index on the model
engine, array for array and search for search; DenseRetriever with device fusion against the per-question loop. All on bits."""
import numpy as np
import pytest
import torch

import lexical_world as LW
from lexical_world import W
from rag_dpo_amd import lexical as LX
from rag_dpo_amd.retriever import DenseRetriever

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def prov():
    return LW.provider(device="cuda", dtype=torch.float16, batch_size=16)


class Recorded:
    """records what every rdx_lex_reduce call of the provider is given: the token ids, the fp32 head outputs, the offsets"""

    def __enter__(self):
        from rag_dpo_amd import engine
        self.calls, self.engine, self.real = [], engine, engine.lex_reduce

        def spy(tok, w, off, vocab, skip, *out):
            self.calls.append((tok.cpu().numpy(), w.cpu().numpy(), off.numpy().copy(), vocab, tuple(skip)))
            return self.real(tok, w, off, vocab, skip, *out)
        engine.lex_reduce = spy
        return self

    def __exit__(self, *exc):
        self.engine.lex_reduce = self.real

    def model(self):
        """the model's terms of every recorded text, call after call -> (ids, weights fp16, off)"""
        parts = [LX.terms_of_texts_model(*c) for c in self.calls]
        off = np.concatenate([[0]] + [p[2][1:] + sum(int(q[2][-1]) for q in parts[:i]) for i, p in enumerate(parts)]).astype(np.int64)
        return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), off


def test_embed_lexical_device_against_the_model(prov):
    rng = np.random.default_rng(3)
    words = [f"w{i}" for i in range(300)]
    texts = [" ".join(rng.choice(words, size=int(n))) for n in (5, 1, 17, 60, 2, 150, 300)] * 6 + ["", "w1 w1 w1"]     # 44 texts: crosses batch_size
    with Recorded() as rec:
        ids, ws, got_off = prov.embed_lexical_device(texts)
        as_dicts = prov.embed_lexical(texts[:20])
    assert len(rec.calls) == 2 and rec.calls[0][1].dtype == np.float32 and rec.calls[0][3:] == (1000, (0, 1, 2, 3))
    tok, w, off = rec.calls[0][:3]
    assert len(off) == 45 and len(tok) == off[-1] == len(w) and (w > 0).any() and (w == 0).any()
    assert tok[off[1:] - 1].tolist() == [2] * 44                                                     # the same token ids: every text ends with </s>
    want_ids, want_w, want_off = LX.terms_of_texts_model(*rec.calls[0])
    assert ids.is_cuda and ids.dtype == torch.int32 and ws.is_cuda and ws.dtype == torch.float16 and got_off.dtype == np.int64
    assert got_off.tolist() == want_off.tolist() and want_off[-1] > 100
    assert ids.cpu().numpy().tolist() == want_ids.tolist()
    assert ws.cpu().numpy().view(np.uint16).tolist() == want_w.view(np.uint16).tolist()
    assert got_off[-2] - got_off[-3] == 0 and got_off[-1] - got_off[-2] <= 1                         # "" has no terms, "w1 w1 w1" at most one
    d_ids, d_w, d_off = LX.terms_of_texts_model(*rec.calls[1])
    assert as_dicts == [dict(zip(d_ids[d_off[i]:d_off[i + 1]].tolist(), d_w[d_off[i]:d_off[i + 1]].astype(np.float64).tolist())) for i in range(20)]
    assert prov.embed_lexical_device([])[2].tolist() == [0]


@pytest.fixture(scope="module")
def world(prov):
    col = LW.collection(None)                                                                        # librdx on cuda:0
    hip = LX.LexicalChunkIndex(prov)
    with Recorded() as rec:
        hip.build_from_collection(col, batch_size=70)
    return col, hip, rec


def test_index_and_searches_against_the_model_engine(world, prov):
    col, hip, rec = world
    assert isinstance(hip.engine, LX.HipLexical) and len(hip.chunk_ids) >= LW.N_CHUNKS - 10 and len(rec.calls) == 5
    # the index array for array: the model's terms of the recorded token ids and fp32 weights, rows without terms dropped, one CSR
    ids, ws, t_off = rec.model()
    counts = np.diff(t_off)
    assert (counts > 0).sum() == len(hip.chunk_ids)
    rows = np.repeat(np.cumsum(counts > 0) - 1, counts)
    want = LX.csr_by_term(torch.from_numpy(ids), torch.from_numpy(rows), torch.from_numpy(ws), len(hip.chunk_ids), prov.lexical_vocab)
    a = hip.arrays
    for name, x in zip(("post_off", "post_row", "post_w"), want):
        assert getattr(a, name).dtype == x.dtype and np.array_equal(getattr(a, name), x), name
    # the same index on the model engine answers every search with the same bits
    model = LX.LexicalChunkIndex(prov, engine_factory=LX.model_factory)
    model._install_csr(hip.chunk_ids, hip.chunk_texts, hip.chunk_metadatas, a.post_off, a.post_row, a.post_w)
    assert np.array_equal(model.arrays.row_group, a.row_group) and model.arrays.n_groups == a.n_groups > 10
    docs = sorted({(m or {}).get("document_path", "") for m in hip.chunk_metadatas} - {""})
    f1, f2 = set(docs[:15]), set(docs[10:40]) | {"absent.html"}

    class Replay:
        """the queries' terms as the GPU provider gave them to the first index, for the second one"""

        def __init__(self):
            self.seen = {}

        def embed_lexical_device(self, texts):
            key = tuple(texts)
            if key not in self.seen:
                self.seen[key] = prov.embed_lexical_device(texts)
            return self.seen[key]
    hip.provider = model.provider = Replay()
    for kw in ({}, {"doc_filter": f1}, {"doc_filters": [f1, None, f2, {"absent.html"}, f2]}, {"doc_filter": {"absent.html"}}):
        for k in (5, 30, 1000):
            g = hip.search_batch_arrays(LW.QUESTIONS, top_k=k, **kw)
            m = model.search_batch_arrays(LW.QUESTIONS, top_k=k, **kw)
            assert g[0] == m[0]
            LW.same_bits(g[1:], m[1:])
    got = hip.search_batch(LW.QUESTIONS, top_k=30, doc_filters=[f1, None, f2, None, f2])
    flat = lambda rss: [[(r.doc_key, r.score, sorted(r.metadata.items())) for r in rs] for rs in rss]   # noqa: E731
    assert flat(got) == flat(model.search_batch(LW.QUESTIONS, top_k=30, doc_filters=[f1, None, f2, None, f2]))
    assert got[2] == [] and len(got[1]) == 30
    hip.provider = prov


class DeviceHashEmbedder(W.HashEmbedder):
    """EmbeddingProvider's contract on the hash embedder: embed_device = the raw rows on the GPU, embed = those rows through
    rdx_l2_normalize, as lists (both retrieval paths then see the same normalised bits)"""

    def embed_device(self, texts):
        import zlib
        out = []
        for t in texts:
            h = zlib.crc32(t.encode("utf-8"))
            out.append(3.0 * (self.c[h % W.N] + 0.8 * np.random.default_rng(h).standard_normal(W.DIM).astype(np.float32)))
        return torch.from_numpy(np.asarray(out, dtype=np.float32)).to("cuda:0")

    def embed(self, texts):
        import ctypes
        from rag_dpo_amd import _lib as L
        raw = self.embed_device(texts)
        out = torch.empty_like(raw)
        L.check(L.load().rdx_l2_normalize(0, ctypes.c_void_p(raw.data_ptr()), raw.shape[0], raw.shape[1], ctypes.c_void_p(out.data_ptr()),
                                          L.RDX_DEVICE, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return out.cpu().numpy().tolist()


def test_dense_retriever_with_device_fusion(world):
    col, hip, _ = world
    qs = [s for s in LW.QUESTIONS if s]
    hip.provider = LW.PerText(hip.provider)          # the batch asks for all sub-queries at once, the loop question by question
    r = DenseRetriever(col, DeviceHashEmbedder(), query_expander=W.expander, chunk_bm25_index=hip, fusion="device")
    got = r.retrieve_candidates_batch(qs, n_candidates=40)
    loop = [r.retrieve_candidates(s, n_candidates=40) for s in qs]
    assert [[LW.chunk_values(c) for c in g] for g in got] == [[LW.chunk_values(c) for c in g] for g in loop]
    assert all(len(g) == 40 for g in got) and any(c.bm25_score > 0 for c in got[0])
