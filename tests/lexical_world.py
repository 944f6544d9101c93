"""TEST-ONLY: what the lexical-weight tests share (test_lexical.py on the CPU, test_gpu_lex_*.py and test_gpu_lexical.py on the GPU):
the fp16 rounding edges of the term rule, small synthetic indexes built straight from (term, row, weight) triples, a provider with
an explicit sparse head, and a few hundred of bm25_world's chunks as a collection. The oracle is rag_dpo_amd/lexical.py's model."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import bm25_world as W  # noqa: E402
from rag_dpo_amd import lexical as LX  # noqa: E402
from rag_dpo_amd import synth  # noqa: E402
from rag_dpo_amd.collection import Collection  # noqa: E402

# (fp32 weight, the fp16 bits it is kept with, or None when the token is dropped): every rounding edge of the rule
ROUNDING_EDGES = [
    (np.float32(2.0 ** -25), None),                                  # a tie between 0 and 2^-24: to even, 0
    (np.nextafter(np.float32(2.0 ** -25), np.float32(1)), 0x0001),   # just above: 2^-24, the smallest fp16
    (np.float32(1 + 2.0 ** -11), 0x3C00),                            # a tie between 1 and 1 + 2^-10: to even, 1.0
    (np.float32(1 + 3 * 2.0 ** -11), 0x3C02),                        # a tie between 1 + 2^-10 and 1 + 2^-9: to even, up
    (np.float32(65519.9), 0x7BFF),                                   # below the tie at 65520: 65504, the largest fp16
    (np.float32(65520.0), None),                                     # the tie goes to infinity
    (np.float32(np.inf), None),
    (np.float32(np.nan), None),
    (np.float32(-0.0), None),
    (np.float32(0.0), None),
    (np.float32(-1.5), None),
]


def f16(x) -> np.uint16:
    return np.asarray(x, dtype=np.float16).view(np.uint16)[()]


def arrays_from_triples(n_rows, vocab, terms, rows, weights, row_group=None, n_groups=0) -> LX.LexArrays:
    """LexArrays from (term, row, fp16 weight) triples, at most one per (term, row), any order"""
    terms, rows = np.asarray(terms, np.int64), np.asarray(rows, np.int64)
    w = np.asarray(weights, np.float16)
    order = np.argsort(terms * n_rows + rows, kind="stable")
    post_off = np.zeros(vocab + 1, np.int64)
    np.cumsum(np.bincount(terms, minlength=vocab), out=post_off[1:])
    return LX.LexArrays(n_rows, vocab, post_off, rows[order].astype(np.int32), w[order].view(np.uint16).copy(), row_group, n_groups)


def dense_corpus(n_rows, vocab, seed, groups=0) -> LX.LexArrays:
    """every row holds term 0 (so every row scores) and each other term with probability 1/2; weights are random fp16 in [2^-4, 4)"""
    rng = np.random.default_rng(seed)
    has = rng.random((vocab, n_rows)) < 0.5
    has[0] = True
    terms, rows = np.nonzero(has)
    w = (rng.integers(1, 64, terms.size) / 16.0).astype(np.float16)
    g = rng.integers(0, groups, n_rows).astype(np.int32) if groups else None
    return arrays_from_triples(n_rows, vocab, terms, rows, w, g, groups)


def query(vocab, n_terms, seed):
    """-> (ids int32 ascending, weights fp16)"""
    rng = np.random.default_rng(seed)
    ids = np.sort(rng.choice(vocab, size=n_terms, replace=False)).astype(np.int32)
    return ids, (rng.integers(1, 64, n_terms) / 16.0).astype(np.float16)


def pack(queries):
    """[(ids, weights)] -> (off int64, ids int32, weights fp16)"""
    off = np.zeros(len(queries) + 1, np.int64)
    np.cumsum([len(q[0]) for q in queries], out=off[1:])
    cat = lambda i, dt: np.concatenate([np.asarray(q[i], dt) for q in queries]) if queries else np.zeros(0, dt)   # noqa: E731
    return off, cat(0, np.int32), cat(1, np.float16)


def same_bits(got, want):
    """search results compared on bits: scores as uint64, rows, counts"""
    (gs, gr, gc), (ws, wr, wc) = got, want
    assert gc.tolist() == wc.tolist()
    assert np.array_equal(gr, wr)
    assert np.array_equal(np.ascontiguousarray(gs).view(np.uint64), np.ascontiguousarray(ws).view(np.uint64))


def head(hidden: int, seed: int = 5):
    """an explicit sparse head: about half of the tokens get a positive weight"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn((1, hidden), generator=g) * 0.5, torch.zeros((1,))


def provider(name="random-init:tiny", device="cpu", dtype=torch.float32, batch_size=16, hidden=64, **kw):
    from rag_dpo_amd.embedding_provider import EmbeddingProvider
    return EmbeddingProvider(model_name=name, device=device, dtype=dtype, batch_size=batch_size, sparse_head=head(hidden), **kw).load()


class PerText:
    """a provider's embed_lexical_device with every distinct text encoded ALONE, once: a text's terms then do not depend on the batch
    it is asked in (a GPU forward's low bits may depend on the batch's shape), which is what a comparison of the batched retrieval
    with the loop over questions needs"""

    def __init__(self, prov):
        self.prov, self.seen = prov, {}

    def embed_lexical_device(self, texts):
        for t in texts:
            if t not in self.seen:
                ids, ws, _ = self.prov.embed_lexical_device([t])
                self.seen[t] = (ids, ws)
        off = np.zeros(len(texts) + 1, np.int64)
        np.cumsum([len(self.seen[t][0]) for t in texts], out=off[1:])
        return torch.cat([self.seen[t][0] for t in texts]), torch.cat([self.seen[t][1] for t in texts]), off


N_CHUNKS = 300


def collection(engine_factory, n=N_CHUNKS):
    """the first n chunks of bm25_world, a few of them blank"""
    texts = W.chunk_texts()[:n]
    for i in (7, 120):
        texts[i] = "   "
    col = Collection("rag_dpo_chunks", metadata={"hnsw:space": "cosine"}, engine_factory=engine_factory)
    col.add(ids=[f"chunk_{i:05d}" for i in range(n)], documents=texts, embeddings=synth.make_corpus(n, W.DIM).tolist(), metadatas=W.metadatas()[:n])
    return col


QUESTIONS = [W.Q0, "registre des traitements du sous-traitant article 28", "", "notification d'une violation en 72 heures", "biométrie badge salariés"]


def chunk_values(c):
    import json
    return (c.chunk_id, c.text, c.document_path, np.float32(c.distance).tobytes(), np.float64(c.bm25_score).tobytes(),
            np.float64(c.semantic_score).tobytes(), np.float64(c.hybrid_score).tobytes(), json.dumps(c.metadata, sort_keys=True))
