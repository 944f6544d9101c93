"""TEST-ONLY: the diversity-aware search's definition (rag_dpo_amd/mmr.py) as a literal double loop over the ORACLE's exact
scores — written without looking at rag_dpo_amd.mmr, which it pins — and the planted worlds the MMR tests share."""
import numpy as np

from oracle import oracle as O


def literal_mmr(cand_scores, cand_rows, corpus_hat, k, lam, n_rows=None):
    """one query: cand_scores / cand_rows = the candidate list (an entry whose row is negative, or >= n_rows, is padding);
    corpus_hat = the stored rows of the whole index. -> [(position, row, score f32, value f64)] in pick order.
    Pick 0 is the first live position; afterwards, for every unpicked position i, m_i = the largest O.scores(row_i, row_j) over the
    picked j, v_i = lam * s_i - (1 - lam) * m_i in doubles, and the largest v wins, the smaller position on ties."""
    n_rows = corpus_hat.shape[0] if n_rows is None else n_rows
    lam = float(lam)                                             # Python floats are IEEE doubles: one rounding per operation, nothing fused
    rest = 1.0 - lam
    live = [i for i, r in enumerate(cand_rows) if 0 <= r < n_rows]
    live_hat = corpus_hat[[int(cand_rows[x]) for x in live]]
    column = {}                                                  # j -> {i: p(i, j)} for every live i, from the oracle, when j is picked

    picked, out = [], []
    while len(picked) < k and len(picked) < len(live):
        if picked:
            j = picked[-1]
            column[j] = dict(zip(live, O.scores(live_hat, corpus_hat[int(cand_rows[j])]).tolist()))   # (an fp32 is a double exactly)
        best = None
        for i in live:
            if i in column:                                      # picked already
                continue
            a = lam * float(np.float32(cand_scores[i]))
            if not picked:
                best = (i, a)
                break
            m = None
            for j in picked:
                p = column[j][i]
                if m is None or p > m:
                    m = p
            b = rest * m
            v = a - b
            if best is None or v > best[1]:
                best = (i, v)
        picked.append(best[0])
        out.append((best[0], int(cand_rows[best[0]]), np.float32(cand_scores[best[0]]), np.float64(best[1])))
    return out


def as_arrays(picks, k):
    """literal_mmr's picks as the padded arrays of the kernel: pos i32 / row i64 / score f32 / value f64 [k], count"""
    pos = np.full(k, -1, dtype=np.int32)
    row = np.full(k, -1, dtype=np.int64)
    sc = np.full(k, -np.inf, dtype=np.float32)
    va = np.full(k, -np.inf, dtype=np.float64)
    for t, (p, r, s, v) in enumerate(picks):
        pos[t], row[t], sc[t], va[t] = p, r, s, v
    return pos, row, sc, va, len(picks)


def expected(corpus_hat, q_raw, k, fetch_k, lam, allow=None):
    """per query, from the oracle's ranking of the allowed rows: [(row, distance f32, value f64)] in pick order"""
    s, r, c = O.cosine_topk(corpus_hat, q_raw, min(fetch_k, corpus_hat.shape[0]), allow)
    out = []
    for b in range(s.shape[0]):
        picks = literal_mmr(s[b, : c[b]], r[b, : c[b]], corpus_hat, k, lam)
        out.append([(row, np.float32(1.0) - sc, v) for _, row, sc, v in picks])
    return out


def same(res, col, want):
    """a query_mmr result against expected(): ids, their order, the distances' and the values' bits"""
    assert len(res["ids"]) == len(want)
    for b, wq in enumerate(want):
        assert col.rows_of(res["ids"][b]) == [row for row, _, _ in wq], f"query {b}: rows"
        assert np.asarray(res["distances"][b], dtype=np.float32).tobytes() == np.asarray([d for _, d, _ in wq], dtype=np.float32).tobytes(), f"query {b}"
        assert np.asarray(res["mmr_scores"][b], dtype=np.float64).tobytes() == np.asarray([v for _, _, v in wq], dtype=np.float64).tobytes(), f"query {b}"


def planted_world(n_clusters=40, paragraphs=3, copies=4, dim=64, seed=0, extra=0):
    """n_clusters topics; a topic is a centre and `paragraphs` passages around it (centre + 0.6 N(0,1)), every passage stored `copies`
    times as near-duplicates (passage + 0.01 N(0,1)); rows scattered over the collection, then `extra` unrelated rows.
    -> (emb f32 [n][dim], cluster i64 [n] (-1 for the extra rows), centres f32 [n_clusters][dim]).
    The centres share a common direction (cosine ~0.55 between two of them), so a query at a centre ranks its own topic's rows first
    (the copies of its nearest passage ahead of all) and the other topics' rows next. A plain top-10 is the copies of one or two
    passages of ONE topic; MMR has used up the topic's distinct passages after `paragraphs` picks and goes on to other topics."""
    rng = np.random.default_rng(seed)
    common = rng.standard_normal(dim).astype(np.float32)
    centres = (common[None, :] + 0.9 * rng.standard_normal((n_clusters, dim))).astype(np.float32)
    passages = centres[:, None, :] + 0.6 * rng.standard_normal((n_clusters, paragraphs, dim))
    n = n_clusters * paragraphs * copies
    which = rng.permutation(np.repeat(np.arange(n_clusters * paragraphs), copies))
    emb = (passages.reshape(-1, dim)[which] + 0.01 * rng.standard_normal((n, dim))).astype(np.float32)
    cluster = which // paragraphs
    if extra:
        emb = np.concatenate([emb, rng.standard_normal((extra, dim)).astype(np.float32)])
        cluster = np.concatenate([cluster, np.full(extra, -1)])
    return emb, cluster.astype(np.int64), centres
