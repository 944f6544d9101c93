"""Synthetic BM25 indexes straight from integer token streams (no text): the arrays of include/rdx.h rdx_bm25_create with the
same statistics rag_dpo_amd/bm25.py computes from tokens (idf_of, and the denominators in rank_bm25's operation order).
Shared by tests/test_gpu_bm25.py and tools/bm25_bench.py."""
import numpy as np

from rag_dpo_amd import bm25


def zipf_p(vocab, a=1.05):
    p = 1.0 / np.arange(1, vocab + 1, dtype=np.float64) ** a
    return p / p.sum()


def arrays_from_tokens(n_rows, vocab, rows, terms, row_group=None, n_groups=0):
    """rows[i], terms[i]: the i-th token (any order; duplicates = tf)"""
    rows = np.asarray(rows, np.int64)
    terms = np.asarray(terms, np.int64)
    doc_len = np.bincount(rows, minlength=n_rows).astype(np.int64)
    key, tf = np.unique(terms * n_rows + rows, return_counts=True)
    post_off = np.zeros(vocab + 1, np.int64)
    np.cumsum(np.bincount(key // n_rows, minlength=vocab), out=post_off[1:])
    avgdl = int(doc_len.sum()) / n_rows
    idf, _ = bm25.idf_of(n_rows, np.diff(post_off))
    denom = bm25.K1 * (1 - bm25.B + bm25.B * doc_len / avgdl)
    return bm25.Bm25Arrays(n_rows, idf, denom, post_off, (key % n_rows).astype(np.int32), tf.astype(np.uint16), row_group, n_groups)


def tokens(n_rows, vocab, mean_len, seed, every_row_term=None):
    rng = np.random.default_rng(seed)
    lens = np.maximum(rng.poisson(mean_len, n_rows), 1)
    rows = np.repeat(np.arange(n_rows, dtype=np.int64), lens)
    terms = rng.choice(vocab, size=rows.size, p=zipf_p(vocab)).astype(np.int64)
    if every_row_term is not None:
        rows = np.concatenate([rows, np.arange(n_rows)])
        terms = np.concatenate([terms, np.full(n_rows, every_row_term)])
    return rows, terms


def make(n_rows, vocab, mean_len, seed, every_row_term=None, groups=0):
    rows, terms = tokens(n_rows, vocab, mean_len, seed, every_row_term)
    g = np.random.default_rng(seed + 1).integers(0, groups, n_rows).astype(np.int32) if groups else None
    return arrays_from_tokens(n_rows, vocab, rows, terms, g, groups)


def make_by_term(n_rows, vocab, mean_len, seed):
    """large corpora without materialising the token stream: term t is in each row with probability 1 - (1 - p_t)^mean_len
    (rows drawn with geometric gaps), with tf = 1 + Poisson(mean_len * p_t); doc_len = the sum of the row's tf"""
    rng = np.random.default_rng(seed)
    p = zipf_p(vocab)
    q = -np.expm1(mean_len * np.log1p(-p))
    rows_l, tf_l, off = [], [], np.zeros(vocab + 1, np.int64)
    for t in range(vocab):
        m = int(n_rows * q[t] * 1.2 + 64)
        if q[t] > 0.5:
            r = np.nonzero(rng.random(n_rows) < q[t])[0]
        else:
            r = np.cumsum(rng.geometric(q[t], m)) - 1
            r = r[r < n_rows]
        rows_l.append(r.astype(np.int32))
        tf_l.append(np.minimum(1 + rng.poisson(mean_len * p[t], r.size), bm25.MAX_TF).astype(np.uint16))
        off[t + 1] = off[t] + r.size
    post_row = np.concatenate(rows_l)
    del rows_l
    post_tf = np.concatenate(tf_l)
    del tf_l
    doc_len = np.maximum(np.bincount(post_row, weights=post_tf, minlength=n_rows).astype(np.int64), 1)
    avgdl = int(doc_len.sum()) / n_rows
    idf, _ = bm25.idf_of(n_rows, np.diff(off))
    denom = bm25.K1 * (1 - bm25.B + bm25.B * doc_len / avgdl)
    return bm25.Bm25Arrays(n_rows, idf, denom, off, post_row, post_tf)


def query(vocab, n_terms, seed):
    """a mix of common and rare terms (Zipf draws), duplicates possible"""
    rng = np.random.default_rng(seed)
    return rng.choice(vocab, size=n_terms, p=zipf_p(vocab, 0.6)).astype(np.int32)
