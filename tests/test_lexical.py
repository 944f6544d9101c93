"""CPU: BGE-M3 lexical weights (rag_dpo_amd/lexical.py) — the numpy model on hand-worked cases, its fp16 rounding edges and
its summation order; LexicalChunkIndex on the model engine; EmbeddingProvider's sparse head. Every comparison is on bits. The kernels:
tests/test_gpu_lex_reduce.py, test_gpu_lex_search.py, test_gpu_lexical.py."""
import numpy as np
import pytest
import torch

import lexical_world as LW
from lexical_world import W
from oracle_engine import factory as dense_cpu
from rag_dpo_amd import lexical as LX
from rag_dpo_amd.retriever import DenseRetriever


def bits(w):
    return np.asarray(w, np.float16).view(np.uint16).tolist()


def test_the_model_on_a_hand_worked_example():
    # text A: id 5's maximum is its first occurrence, id 7's a middle one, id 9's the last; ids 0 and 2 are special; id 11 has weight
    # 0, id 12 a negative one
    a_tok = [5, 7, 5, 9, 0, 7, 9, 5, 2, 7, 11, 9, 12]
    a_w = [0.5, 0.25, 0.25, 0.125, 3.0, 1.0, 0.25, 0.125, 4.0, 0.5, 0.0, 2.0, -1.0]
    b_tok = [9, 5, 20, 1, 3]
    b_w = [0.5, 4.0, 1.0, 9.0, 9.0]
    a = LX.terms_model(a_tok, a_w, 100)
    b = LX.terms_model(b_tok, b_w, 100)
    assert a[0].dtype == np.int32 and a[1].dtype == np.float16
    assert a[0].tolist() == [5, 7, 9] and bits(a[1]) == bits([0.5, 1.0, 2.0])
    assert b[0].tolist() == [5, 9, 20] and bits(b[1]) == bits([4.0, 0.5, 1.0])
    assert LX.score_model(*a, *b) == 0.5 * 4.0 + 2.0 * 0.5 == 3.0 == LX.score_model(*b, *a)
    assert LX.score_model(*a, *a) == 0.25 + 1.0 + 4.0
    assert LX.score_model(*a, np.zeros(0, np.int32), np.zeros(0, np.float16)) == 0.0
    # both texts in one call; a text without terms; other special ids
    ids, ws, off = LX.terms_of_texts_model(np.array(a_tok + b_tok + [0, 2]), np.array(a_w + b_w + [1.0, 1.0], np.float32), [0, 13, 18, 20, 20], 100)
    assert off.tolist() == [0, 3, 6, 6, 6] and ids.tolist() == [5, 7, 9, 5, 9, 20] and bits(ws) == bits([0.5, 1.0, 2.0, 4.0, 0.5, 1.0])
    assert LX.terms_model(b_tok, b_w, 100, skip=(9, 20))[0].tolist() == [1, 3, 5]
    with pytest.raises(ValueError, match="text 1: a token id outside"):
        LX.terms_of_texts_model(np.array([4, 100]), np.ones(2, np.float32), [0, 1, 2], 100)
    with pytest.raises(ValueError, match="outside"):
        LX.terms_model([-1], [1.0], 100)

    class Tok:
        cls_token_id, eos_token_id, pad_token_id, unk_token_id = 101, 102, 0, None
    assert LX.special_ids(Tok) == (0, 101, 102) and LX.special_ids(object()) == (0, 1, 2, 3)


def test_fp16_rounding_at_its_edges():
    for i, (w, kept) in enumerate(LW.ROUNDING_EDGES):
        ids, ws = LX.terms_model([40 + i], [w], 100)
        if kept is None:
            assert ids.tolist() == [], (i, w)
        else:
            assert ids.tolist() == [40 + i] and ws.view(np.uint16).tolist() == [kept], (i, w)
    assert np.float16(2.0 ** -24).view(np.uint16) == 1 and np.float16(65504).view(np.uint16) == 0x7BFF
    # the maximum is taken over the ROUNDED weights of the kept tokens: an infinity does not win, it is dropped
    ids, ws = LX.terms_model([8, 8, 8], np.array([70000.0, 1 + 2.0 ** -11, 0.5], np.float32), 100)
    assert ids.tolist() == [8] and ws.view(np.uint16).tolist() == [0x3C00]


def order_probe(big_first: bool):
    """three terms whose products are 2^30, 2^-23, 2^-23 (fp16 32768 * 32768 and 2^-12 * 2^-11) -> (q_w, d_w) over ids 10, 20, 30"""
    big, sq, sd = (32768.0, 32768.0), 2.0 ** -12, 2.0 ** -11
    q = [big[0], sq, sq] if big_first else [sq, sq, big[0]]
    d = [big[1], sd, sd] if big_first else [sd, sd, big[1]]
    return np.array(q, np.float16), np.array(d, np.float16)


def test_the_summation_order_shows():
    assert (2.0 ** 30 + 2.0 ** -23) + 2.0 ** -23 == 2.0 ** 30 and (2.0 ** -23 + 2.0 ** -23) + 2.0 ** 30 != 2.0 ** 30
    ids = np.array([10, 20, 30], np.int32)
    off = np.array([0, 3], np.int64)
    for big_first, want in ((True, 2.0 ** 30), (False, 2.0 ** 30 + 2.0 ** -22)):
        q_w, d_w = order_probe(big_first)
        assert LX.score_model(ids, q_w, ids, d_w) == want
        arrays = LW.arrays_from_triples(2, 40, [10, 20, 30], [1, 1, 1], d_w)
        sc, ro, cn = LX.ModelLexical(arrays).search(off, ids, q_w, 2)
        assert cn.tolist() == [1] and ro.tolist() == [[1, -1]] and sc.tolist() == [[want, 0.0]]
        mutant = LX.ModelLexical(arrays, order=-1).search(off, ids, q_w, 2)[0]          # the terms added in descending id
        assert mutant[0, 0] != want and mutant[0, 0] == (2.0 ** 30 + 2.0 ** -22 if big_first else 2.0 ** 30)


def test_model_engine_filters_ties_and_format():
    groups = np.array([0, 1, 0, 2, 1], np.int32)
    # term 3 in every row with one weight: a plateau; term 5 lifts row 3
    arrays = LW.arrays_from_triples(5, 8, [3] * 5 + [5], [0, 1, 2, 3, 4, 3], [1.0] * 5 + [2.0], groups, 3)
    eng = LX.ModelLexical(arrays)
    off, ids, w = LW.pack([([3, 5], [0.5, 0.25]), ([], []), ([3], [2.0]), ([6], [1.0])])
    sets = np.array([[0b010], [0b101], [0]], np.uint32)
    sc, ro, cn = eng.search(off, ids, w, 3, sets, np.array([-1, -1, 0, -1], np.int32))
    assert cn.tolist() == [3, 0, 2, 0]
    assert ro.tolist() == [[3, 0, 1], [-1, -1, -1], [1, 4, -1], [-1, -1, -1]]
    assert sc.tolist() == [[1.0, 0.5, 0.5], [0.0] * 3, [2.0, 2.0, 0.0], [0.0] * 3]
    sc, ro, cn = eng.search(off, ids, w, 5, sets, np.array([1, 2, 2, 0], np.int32))
    assert cn.tolist() == [3, 0, 0, 0] and ro[0].tolist() == [3, 0, 2, -1, -1]


@pytest.fixture(scope="module")
def world():
    prov = LW.provider()
    col = LW.collection(dense_cpu)
    ix = LX.LexicalChunkIndex(prov, engine_factory=LX.model_factory)
    ix.build_from_collection(col, batch_size=70)
    return prov, col, ix


def results(rs):
    return [(r.doc_key, np.float64(r.score).tobytes(), sorted(r.metadata.items())) for r in rs]


def test_index_on_the_model_engine(world, tmp_path):
    prov, col, ix = world
    assert ix.is_built and LW.N_CHUNKS - 10 <= len(ix.chunk_ids) <= LW.N_CHUNKS - 2                        # blank texts are skipped
    assert not {"chunk_00007", "chunk_00120"} & set(ix.chunk_ids) and all(t.strip() for t in ix.chunk_texts)
    a = ix.arrays
    assert a.n_terms == prov.lexical_vocab == 1000 and a.post_off[-1] == len(a.post_row) == len(a.post_w) > 0
    # the index is the model applied to every chunk: postings of row r = the terms of its text
    terms = prov.embed_lexical(ix.chunk_texts)
    assert all(t for t in terms)
    row_terms = [dict() for _ in ix.chunk_ids]
    for t in range(a.n_terms):
        seg = slice(int(a.post_off[t]), int(a.post_off[t + 1]))
        assert (np.diff(a.post_row[seg]) > 0).all()
        for r, w in zip(a.post_row[seg].tolist(), a.post_w[seg].view(np.float16).astype(np.float64).tolist()):
            row_terms[r][t] = w
    assert row_terms == terms
    # one query's scores are the pair scores of the definition
    q = prov.embed_lexical([LW.QUESTIONS[0]])[0]
    assert q
    q_ids, q_w = np.array(list(q), np.int32), np.array(list(q.values()), np.float16)
    hits = ix.search(LW.QUESTIONS[0], top_k=len(ix.chunk_ids))
    want = sorted(((LX.score_model(q_ids, q_w, np.array(list(t), np.int32), np.array(list(t.values()), np.float16)), -r)
                   for r, t in enumerate(terms)), reverse=True)
    want = [(s, -r) for s, r in want if s > 0]
    assert [(h.score, ix.chunk_ids.index(h.doc_key)) for h in hits] == want and len(hits) > 10
    # search == search_batch == search_batch_arrays
    batch = ix.search_batch(LW.QUESTIONS, top_k=30)
    assert [results(b) for b in batch] == [results(ix.search(s, top_k=30)) for s in LW.QUESTIONS]
    assert batch[2] == [] and all(len(b) for i, b in enumerate(batch) if i != 2)                     # a query without terms finds nothing
    live, sc, ro, cn = ix.search_batch_arrays(LW.QUESTIONS, top_k=30)
    assert live == [0, 1, 3, 4] and sc.dtype == np.float64 and ro.dtype == np.int64 and cn.dtype == np.int32
    for j, i in enumerate(live):
        assert [(ix.chunk_ids[r], s) for r, s in zip(ro[j, :cn[j]].tolist(), sc[j, :cn[j]].tolist())] == [(h.doc_key, h.score) for h in batch[i]]
        assert (ro[j, cn[j]:] == -1).all() and (sc[j, cn[j]:] == 0).all()
    # doc_filter and doc_filters
    docs = sorted({h.metadata.get("document_path", "") for h in batch[0]} - {""})
    f1, f2 = set(docs[:3]), set(docs[3:5]) | {"absent.html"}
    filtered = ix.search(LW.QUESTIONS[0], top_k=30, doc_filter=f1)
    assert filtered and results(filtered) == results([h for h in ix.search(LW.QUESTIONS[0], top_k=len(ix.chunk_ids)) if h.metadata.get("document_path", "") in f1][:30])
    assert ix.search(LW.QUESTIONS[0], top_k=30, doc_filter={"absent.html"}) == [] and ix.search(LW.QUESTIONS[0], top_k=30, doc_filter=set()) == []
    per = ix.search_batch(LW.QUESTIONS, top_k=30, doc_filters=[f1, None, f1, {"absent.html"}, f2])
    assert [results(p) for p in per] == [results(ix.search(s, top_k=30, doc_filter=f)) for s, f in zip(LW.QUESTIONS, [f1, None, f1, {"absent.html"}, f2])]
    assert per[3] == [] and per[4]
    with pytest.raises(ValueError, match="not both"):
        ix.search_batch(LW.QUESTIONS, doc_filter=f1, doc_filters=[None] * 5)
    # all queries of a call go through ONE encode
    calls = []
    real = prov.embed_lexical_device
    prov.embed_lexical_device = lambda texts: (calls.append(len(texts)), real(texts))[1]
    try:
        ix.search_batch(LW.QUESTIONS, top_k=5)
    finally:
        del prov.embed_lexical_device
    assert calls == [5]
    # save / load: equal arrays, equal results
    ix.save(str(tmp_path / "lex"))
    back = LX.LexicalChunkIndex.load(str(tmp_path / "lex"), prov, engine_factory=LX.model_factory)
    for name in ("post_off", "post_row", "post_w", "row_group"):
        x, y = getattr(ix.arrays, name), getattr(back.arrays, name)
        assert x.dtype == y.dtype and np.array_equal(x, y), name
    assert (back.arrays.n_rows, back.arrays.n_terms, back.arrays.n_groups) == (a.n_rows, a.n_terms, a.n_groups)
    assert (back.chunk_ids, back.chunk_texts, back.chunk_metadatas) == (ix.chunk_ids, ix.chunk_texts, ix.chunk_metadatas)
    assert [results(b) for b in back.search_batch(LW.QUESTIONS, top_k=30, doc_filters=[f1, None, None, None, f2])] == \
        [results(b) for b in ix.search_batch(LW.QUESTIONS, top_k=30, doc_filters=[f1, None, None, None, f2])]
    # build_from_weights: the same index from the weights computed elsewhere
    other = LX.LexicalChunkIndex(prov, engine_factory=LX.model_factory)
    other.build_from_weights(ix.chunk_ids + ["blank"], ix.chunk_texts + ["-"], ix.chunk_metadatas + [None], terms + [{0: 1.0, 7: 0.0}])
    assert other.chunk_ids == ix.chunk_ids and all(np.array_equal(getattr(ix.arrays, n), getattr(other.arrays, n)) for n in ("post_off", "post_row", "post_w"))
    empty = LX.LexicalChunkIndex(prov, engine_factory=LX.model_factory)
    with pytest.raises(RuntimeError, match="not built"):
        empty.search("x")
    empty.build_from_weights([], [], [], [])
    assert empty.is_built and empty.search(LW.QUESTIONS[0]) == []


def test_dense_retriever_takes_the_index(world):
    prov, col, ix = world
    ix = LX.LexicalChunkIndex.__new__(LX.LexicalChunkIndex)
    ix.__dict__.update(world[2].__dict__)
    ix.provider = LW.PerText(prov)                    # the batch asks for all sub-queries at once, the loop question by question
    r = DenseRetriever(col, W.HashEmbedder(), query_expander=W.expander, chunk_bm25_index=ix, fusion="host")
    qs = [s for s in LW.QUESTIONS if s]
    got = r.retrieve_candidates_batch(qs, n_candidates=40)
    loop = [r.retrieve_candidates(s, n_candidates=40) for s in qs]
    assert [[LW.chunk_values(c) for c in g] for g in got] == [[LW.chunk_values(c) for c in g] for g in loop]
    assert all(len(g) == 40 for g in got) and any(c.bm25_score > 0 for c in got[0])
    plain = DenseRetriever(col, W.HashEmbedder(), query_expander=W.expander, fusion="host").retrieve_candidates(qs[0], n_candidates=40)
    assert [c.chunk_id for c in plain] != [c.chunk_id for c in got[0]]                                # the sparse ranking took part


def test_the_provider():
    from rag_dpo_amd.embedding_provider import EmbeddingProvider
    none = EmbeddingProvider(model_name="random-init:tiny", device="cpu", dtype=torch.float32).load()
    with pytest.raises(RuntimeError, match="no lexical-weight head"):
        none.embed_lexical(["a b"])
    with pytest.raises(RuntimeError, match="no lexical-weight head"):
        none.embed_lexical_device(["a b"])
    assert none._token_states(["a b"])[0].shape == (3, 64)                                            # everything else is unchanged
    for bad in ((torch.zeros((2, 64)), torch.zeros((2,))), (torch.zeros((1, 32)), torch.zeros((1,))), (torch.zeros((64,)), torch.zeros((1,))),
                (torch.zeros((1, 64)), torch.zeros((2,)))):
        with pytest.raises(ValueError, match="sparse_head"):
            EmbeddingProvider(model_name="random-init:tiny", device="cpu", dtype=torch.float32, sparse_head=bad).load()
    p = LW.provider(batch_size=3)
    texts = ["alpha beta gamma alpha", "", "beta", "delta " * 40 + "alpha", "epsilon zeta eta theta iota kappa lambda", "alpha alpha alpha", "mu nu"]
    h, off = p._token_states(texts)
    h2, off2, tok = p._token_states(texts, with_ids=True)
    assert torch.equal(h, h2) and off.tolist() == off2.tolist() and tok.dtype == np.int32 and len(tok) == off[-1] == h.shape[0]
    assert tok[off[1:] - 1].tolist() == [2] * len(texts)                                              # every text ends with </s>
    assert tok[off[0]:off[1]].tolist()[0] == tok[off[0]:off[1]].tolist()[3] and off[2] - off[1] == 1
    w = torch.relu(torch.nn.functional.linear(h, *p._sparse)).reshape(-1).numpy()
    assert (w > 0).any() and (w == 0).any()
    ids, ws, out_off = LX.terms_of_texts_model(tok, w, off, 1000)
    got_ids, got_w, got_off = p.embed_lexical_device(texts)
    assert got_ids.dtype == torch.int32 and got_w.dtype == torch.float16 and isinstance(got_off, np.ndarray) and got_off.dtype == np.int64
    assert got_off.tolist() == out_off.tolist() and got_ids.tolist() == ids.tolist() and got_w.numpy().view(np.uint16).tolist() == ws.view(np.uint16).tolist()
    assert got_off[2] == got_off[1]                                                                   # "" has only </s>: no terms
    d = p.embed_lexical(texts)
    assert [list(x) for x in d] == [ids[out_off[i]:out_off[i + 1]].tolist() for i in range(len(texts))]
    assert all(isinstance(v, float) and v > 0 for x in d for v in x.values()) and not (set(ids.tolist()) & {0, 1, 2, 3})
    assert p.embed_lexical([]) == [] and p.embed_lexical_device([])[2].tolist() == [0]
