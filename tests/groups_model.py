"""TEST-ONLY: the grouped search's definition (rag_dpo_amd/groups.py) as a literal double loop, and the expected answer
of a collection computed from the ORACLE's exact scores — never from a second call into the code under test."""
import numpy as np

from oracle import oracle as O
from rag_dpo_amd.where import kind_of


def group_key(v):
    """what makes two metadata values one group: equal and of the same kind (1 and True differ); None = the row has no group"""
    return None if v is None else (kind_of(v), v)


def literal_groups(ranked_scores, ranked_rows, key_of_row, G, m):
    """walk the ranking; -> [(key, [(score, row), ...])]: the first G distinct keys met, each with its first m rows"""
    groups = []
    for s, r in zip(ranked_scores, ranked_rows):
        if r < 0:
            continue
        key = key_of_row[r]
        if key is None:
            continue
        for k2, members in groups:
            if k2 == key:
                if len(members) < m:
                    members.append((s, int(r)))
                break
        else:
            if len(groups) < G:
                groups.append((key, [(s, int(r))]))
    return groups


def oracle_ranking(corpus_hat, q_raw, allow=None):
    """the whole ranking of the allowed rows per query: (scores f32 [nq][n], rows i64 [nq][n], counts i32 [nq])"""
    return O.cosine_topk(corpus_hat, q_raw, corpus_hat.shape[0], allow)


def expected(corpus_hat, q_raw, values, G, m, allow=None):
    """per query [(value, [row, ...], [score bits, ...], [distance, ...])] from the oracle's ranking; values[r] = the key's value or None"""
    keys = [group_key(v) for v in values]
    s, r, c = oracle_ranking(corpus_hat, q_raw, allow)
    out = []
    for b in range(s.shape[0]):
        gs = literal_groups(s[b, : c[b]], r[b, : c[b]], keys, G, m)
        out.append([(key[1], [row for _, row in mem], [int(np.float32(sc).view(np.uint32)) for sc, _ in mem],
                     [float(np.float32(1.0) - np.float32(sc)) for sc, _ in mem]) for key, mem in gs])
    return out


def as_expected(res, col):
    """a query_groups result in expected()'s shape: rows from ids, score bits unknown (None), distances as returned"""
    out = []
    for b in range(len(res["ids"])):
        out.append([(res["groups"][b][g], col.rows_of(res["ids"][b][g]), None, res["distances"][b][g]) for g in range(len(res["ids"][b]))])
    return out


def same(got, want):
    """groups, their order, rows, their order and the distances' bits"""
    assert len(got) == len(want)
    for b, (gq, wq) in enumerate(zip(got, want)):
        assert [(type(v), v) for v, _, _, _ in gq] == [(type(v), v) for v, _, _, _ in wq], f"query {b}: groups"
        for (v, gr, _, gd), (_, wr, _, wd) in zip(gq, wq):
            assert gr == wr, f"query {b} group {v!r}: rows {gr} != {wr}"
            assert np.asarray(gd, dtype=np.float32).tobytes() == np.asarray(wd, dtype=np.float32).tobytes(), f"query {b} group {v!r}: distances"
