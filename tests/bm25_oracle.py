"""TEST-ONLY: a CPU restatement of rank_bm25 0.2.2's BM25Okapi (the scorer behind the reference's bm25_index.py) and a CPU
engine with the interface of rag_dpo_amd.bm25.HipBm25, for the engine-factory hook of SummaryBM25Index / ChunkBM25Index.
The product never imports this file.

rank_bm25 0.2.2 (k1 = 1.5, b = 0.75, epsilon = 0.25):
    doc_len = tokens per document, avgdl = sum(doc_len) / N (Python true division), nd[w] = documents containing w, in the
    order words are first met; idf[w] = log(N - nd + 0.5) - log(nd + 0.5), idf_sum accumulated in that order with plain
    float additions; average_idf = idf_sum / |V|; every negative idf is replaced by epsilon * average_idf.
    get_scores(query): score = zeros(N); for q in query: q_freq = [doc.get(q) or 0 for doc]; score += (idf.get(q) or 0) *
    (q_freq * (k1 + 1) / (q_freq + k1 * (1 - b + b * doc_len / avgdl))), numpy float64, doc_len an int64 array.
"""
import math

import numpy as np


class BM25Okapi:
    def __init__(self, corpus, k1=1.5, b=0.75, epsilon=0.25):
        self.k1, self.b, self.epsilon = k1, b, epsilon
        self.corpus_size = 0
        self.doc_len, self.doc_freqs, self.idf = [], [], {}
        nd, total = {}, 0
        for doc in corpus:
            self.doc_len.append(len(doc))
            total += len(doc)
            freqs = {}
            for w in doc:
                freqs[w] = freqs.get(w, 0) + 1
            self.doc_freqs.append(freqs)
            for w in freqs:
                nd[w] = nd.get(w, 0) + 1
            self.corpus_size += 1
        self.avgdl = total / self.corpus_size
        idf_sum, negative = 0, []
        for w, f in nd.items():
            v = math.log(self.corpus_size - f + 0.5) - math.log(f + 0.5)
            self.idf[w] = v
            idf_sum += v
            if v < 0:
                negative.append(w)
        self.average_idf = idf_sum / len(self.idf)
        for w in negative:
            self.idf[w] = self.epsilon * self.average_idf

    def get_scores(self, query):
        score = np.zeros(self.corpus_size)
        doc_len = np.array(self.doc_len)
        for q in query:
            q_freq = np.array([(d.get(q) or 0) for d in self.doc_freqs])
            score += (self.idf.get(q) or 0) * (q_freq * (self.k1 + 1) /
                                               (q_freq + self.k1 * (1 - self.b + self.b * doc_len / self.avgdl)))
        return score


def topk(scores, k, allow_rows=None):
    """the reference's cut: score > 0 (and allowed), score descending, ties by ascending row (stable sort), first k"""
    idx = np.nonzero(scores > 0)[0]
    if allow_rows is not None:
        idx = idx[allow_rows[idx]]
    order = idx[np.argsort(-scores[idx], kind="stable")][:k]
    return order, scores[order]


class CpuBm25:
    """the engine interface of rag_dpo_amd.bm25.HipBm25 on the CPU: the postings added in query order, as numpy would"""

    def __init__(self, arrays, device=0):
        self.a = arrays
        self.device = device

    def scores(self, ids):
        a = self.a
        score = np.zeros(a.n_rows)
        for t in ids:
            b, e = int(a.post_off[t]), int(a.post_off[t + 1])
            rows = a.post_row[b:e].astype(np.int64)
            tf = a.post_tf[b:e].astype(np.float64)
            score[rows] = score[rows] + a.idf[t] * ((tf * 2.5) / (tf + a.denom[rows]))
        return score

    def search(self, term_offsets, term_ids, k, allow_bits=None):
        a = self.a
        if not 1 <= k <= 4096:
            raise ValueError("k out of range")
        nq = len(term_offsets) - 1
        sc, ro, cn = np.zeros((nq, k)), np.full((nq, k), -1, np.int64), np.zeros(nq, np.int32)
        allow = None
        if allow_bits is not None:
            gbits = np.unpackbits(np.asarray(allow_bits, np.uint32).view(np.uint8), bitorder="little").astype(bool)
            allow = gbits[a.row_group]
        for q in range(nq):
            ids = term_ids[term_offsets[q]:term_offsets[q + 1]]
            rows, s = topk(self.scores(ids), k, allow)
            cn[q] = len(rows)
            ro[q, :len(rows)] = rows
            sc[q, :len(rows)] = s
        return sc, ro, cn

    def close(self):
        pass


def factory(arrays, device=0):
    return CpuBm25(arrays, device)
