"""The model of rdx_fuse_rankings and the list sets its tests run: `DenseRetriever._fuse` ITSELF, driven with objects built from packed
lists. Nothing here restates the fusion: a question's lists become the RetrievedChunk / BM25Result objects _fuse takes, _fuse runs, and
what it returns is read back as (key, distance, semantic, bm25, hybrid, first list, first rank).

A question is a list of `n_lists` entries in _fuse's visiting order (dense q0, BM25 q0, dense q1, BM25 q1, ...): None = absent, else
(kind, weight, keys, values). _fuse fixes two things the kernel leaves open, so every list set here keeps to them: the dense list of
sub-query i has weight 2.0 (i = 0) or 1.0, and a BM25 list cannot be present when its sub-query's dense list is absent."""
import numpy as np

from rag_dpo_amd.bm25 import BM25Result
from rag_dpo_amd.fusion import BM25, DENSE, PackedLists
from rag_dpo_amd.retriever import DenseRetriever, RetrievedChunk

N_ROWS, N_GROUPS = 4096, 40                 # more than 32 groups: the allow bitset has a second word


def row_group_table():
    return (np.arange(N_ROWS, dtype=np.int64) * 7 % N_GROUPS).astype(np.int32)


ROW_GROUP = row_group_table()
NOTHING = "no such document"


def _path(key: int) -> str:
    return f"g{int(ROW_GROUP[key])}" if 0 <= key < N_ROWS else "outside the table"


def dense_weight(l: int) -> float:
    return 2.0 if l == 0 else 1.0


def run_model(lists, allowed_groups=None, min_semantic=10, bm25_keep_max=True, top_n=100):
    """-> (winners, distinct keys): winners = _fuse(...)[:top_n] as tuples (key, fp32 distance, semantic, bm25, hybrid, list, rank).
    allowed_groups: None = no filter, else the groups that pass ([] = a filter nothing passes)"""
    assert len(lists) % 2 == 0
    per_query, bm25 = [], []
    for i in range(len(lists) // 2):
        d, b = lists[2 * i], lists[2 * i + 1]
        if d is None:
            assert b is None, "_fuse skips the BM25 ranking of a skipped sub-query"
            per_query.append(None)
            bm25.append(None)
            continue
        kind, weight, keys, vals = d
        assert kind == DENSE and weight == dense_weight(2 * i)
        per_query.append([RetrievedChunk(chunk_id=str(k), text="", document_path=_path(k), chunk_nature="", chunk_index=0, confidence="",
                                         distance=float(np.float32(v)), metadata={"pos": (2 * i, r)}) for r, (k, v) in enumerate(zip(keys, vals))])
        if b is None:
            bm25.append(None)
        else:
            kind, weight, keys, vals = b
            assert kind == BM25
            bm25.append(([BM25Result(doc_key=str(k), score=float(v), metadata={"pos": (2 * i + 1, r)}) for r, (k, v) in enumerate(zip(keys, vals))],
                         weight))
    doc_filter = None
    if allowed_groups is not None:
        doc_filter = {f"g{g}" for g in allowed_groups} or {NOTHING}      # (an EMPTY doc_filter would switch the filter off)
    fused = DenseRetriever(None, None)._fuse(per_query, bm25=bm25, doc_filter=doc_filter, min_semantic=min_semantic,
                                             bm25_keep_max=bm25_keep_max)
    out = [(int(c.chunk_id), np.float32(c.distance), c.semantic_score, c.bm25_score, c.hybrid_score) + tuple(c.metadata["pos"])
           for c in fused[:top_n]]
    for c, o in zip(fused, out):
        assert float(o[1]) == c.distance                                # the distance is an fp32 value throughout
    return out, len(fused)


def pack(questions, n_lists, stride, filters=None):
    """questions: list of list sets; filters: per question None or the allowed groups"""
    p = PackedLists(len(questions), n_lists, stride)
    for q, lists in enumerate(questions):
        assert len(lists) <= n_lists
        for l, ent in enumerate(lists):
            if ent is not None:
                p.set_list(q, l, *ent)
        if filters is not None and filters[q] is not None:
            p.set_filter(q, filters[q], N_GROUPS)
    return p


def bits(x, dtype):
    return np.asarray(x, dtype=dtype).view({4: np.uint32, 8: np.uint64}[np.dtype(dtype).itemsize]).tolist()


def same_as_model(winners, model, distinct, top_n):
    """the kernel's winners (rag_dpo_amd.fusion.Winner) against run_model's, bit for bit"""
    assert len(winners) == min(top_n, distinct) == len(model), (len(winners), distinct, len(model))
    assert [w.key for w in winners] == [m[0] for m in model]                                   # order
    assert bits([w.distance for w in winners], np.float32) == bits([m[1] for m in model], np.float32)
    for j, name in ((2, "semantic_score"), (3, "bm25_score"), (4, "hybrid_score")):
        assert bits([getattr(w, name) for w in winners], np.float64) == bits([m[j] for m in model], np.float64), name
    assert [(w.first_list, w.first_rank) for w in winners] == [(m[5], m[6]) for m in model]


# ---- list sets ----------------------------------------------------------------------------------------------------------------------
def dense(l, keys, dists):
    return (DENSE, dense_weight(l), list(keys), [float(np.float32(d)) for d in dists])


def sparse(weight, keys, scores):
    return (BM25, float(weight), list(keys), [float(s) for s in scores])


def random_question(rng, n_pairs, stride, pool=None, absent=0.15, fill=None):
    """n_pairs sub-queries; keys from a pool small enough that lists overlap and a key may repeat inside a list"""
    pool = pool or max(8, n_pairs * stride // 2)
    lists = []
    for i in range(n_pairs):
        if i > 0 and rng.random() < absent:
            lists += [None, None]
            continue
        n = stride if fill else int(rng.integers(0, stride + 1))
        keys = rng.integers(0, min(pool, N_ROWS), n)
        d = np.sort(rng.random(n).astype(np.float32) * np.float32(1.6))
        if n > 2 and rng.random() < 0.5:
            d[1] = d[0]                                                       # equal distances
        lists.append(dense(2 * i, keys, d))
        if rng.random() < absent:
            lists.append(None)
            continue
        m = stride if fill else int(rng.integers(0, stride + 1))
        bkeys = rng.integers(0, min(pool, N_ROWS), m)
        gone = rng.random(m) < 0.05
        bkeys = np.where(gone, -2 - bkeys, bkeys)                             # chunks the collection no longer holds
        lists.append(sparse(3.0 if i == 0 else 0.75, bkeys, np.sort(rng.random(m) * 20 + 1e-3)[::-1]))
    return lists


def random_filter(rng):
    """None, or some of the groups (sometimes none of them)"""
    r = rng.random()
    if r < 0.3:
        return None
    return sorted(rng.choice(N_GROUPS, int(rng.integers(0, N_GROUPS // 2)), replace=False).tolist())


def keys_of_group(g, n, start=0):
    out = [k for k in range(start, N_ROWS) if ROW_GROUP[k] == g][:n]
    assert len(out) == n
    return out


def named_cases():
    """name -> dict(lists, allowed, min_semantic, keep_max, top_n): the smallest list sets at which each rule of the contract can go wrong"""
    C = {}

    def case(name, lists, allowed=None, ms=10, keep=True, top_n=100):
        C[name] = dict(lists=lists, allowed=allowed, min_semantic=ms, keep_max=keep, top_n=top_n)

    d5, k5 = [0.1, 0.2, 0.3, 0.4, 0.5], [10, 11, 12, 13, 14]
    # list presence
    case("one list: hybrid = semantic", [dense(0, k5, d5[::-1]), None])
    case("second list empty: RRF applies", [dense(0, k5, d5), sparse(3.0, [], [])])
    case("absent pair between present ones", [dense(0, k5, d5), sparse(3.0, [12, 99], [4.0, 2.0]), None, None,
                                               dense(4, [14, 50, 10], [0.05, 0.2, 0.6]), sparse(0.75, [50, 10], [9.0, 1.0])])
    case("absent BM25 beside a present dense", [dense(0, k5, d5), None, dense(2, [11, 60], [0.15, 0.3]), sparse(0.75, [60], [2.5])])
    case("no list present", [None, None, None, None])
    # overlap
    case("full overlap", [dense(0, k5, d5), sparse(3.0, k5[::-1], [5, 4, 3, 2, 1]), dense(2, k5[2:] + k5[:2], [0.09, 0.21, 0.33, 0.41, 0.55]),
                          sparse(0.75, k5, [1, 2, 3, 4, 5])])
    case("no overlap", [dense(0, [1, 2, 3], d5[:3]), sparse(3.0, [4, 5, 6], [3, 2, 1]), dense(2, [7, 8, 9], d5[:3]), sparse(0.75, [20, 21], [2, 1])])
    # RRF ties: the same rank and weight in two lists
    case("RRF tie: first appearance decides", [dense(0, [1], [0.3]), None, dense(2, [2, 3], [0.5, 0.6]), None, dense(4, [4, 5], [0.1, 0.2]), None])
    case("RRF tie across a BM25 list", [dense(0, [1, 2], [0.3, 0.4]), sparse(2.0, [3, 4], [2.0, 1.0])])
    # first-appearance rules
    case("BM25 first, then dense above 1.0", [dense(0, [1], [0.3]), sparse(3.0, [7], [4.0]), dense(2, [7], [1.2]), None])
    case("BM25 first, then dense below 1.0", [dense(0, [1], [0.3]), sparse(3.0, [7], [4.0]), dense(2, [7], [0.25]), None])
    case("a key repeated inside a dense list", [dense(0, [5, 6, 5, 5], [0.4, 0.5, 0.2, 0.9]), sparse(3.0, [6], [1.0])])
    case("a key repeated inside a BM25 list", [dense(0, [5], [0.4]), sparse(3.0, [6, 5, 6], [3.0, 2.0, 1.0])])
    case("a key repeated, one list", [dense(0, [5, 6, 5], [0.4, 0.5, 0.2]), None])
    case("dense distances fall and rise", [dense(0, [5, 6], [0.4, 0.5]), None, dense(2, [6, 5], [0.45, 0.7]), None, dense(4, [5, 6], [0.1, 0.6]), None])
    # the filtered dense list: group 3 allowed
    g3, other = keys_of_group(3, 12), [k for k in range(200, 260) if ROW_GROUP[k] != 3][:12]
    dd = [0.05 * (i + 1) for i in range(12)]
    b = sparse(3.0, [g3[0], other[0], 900], [3.0, 2.0, 1.0])
    case("filter keeps 0", [dense(0, other[:6], dd[:6]), b], allowed=[3], ms=4)
    case("filter keeps nothing at all", [dense(0, other[:6], dd[:6]), b], allowed=[], ms=4)
    case("filter keeps min_semantic - 1", [dense(0, [other[0], g3[0], other[1], g3[1], g3[2], other[2], other[3]], dd[:7]), b], allowed=[3], ms=4)
    case("filter keeps exactly min_semantic", [dense(0, [other[0], g3[0], other[1], g3[1], g3[2], other[2], g3[3]], dd[:7]), b], allowed=[3], ms=4)
    case("filter keeps more than min_semantic", [dense(0, g3[:6] + other[:2], dd[:8]), b], allowed=[3], ms=4)
    case("fewer than min_semantic entries in total", [dense(0, [other[0], g3[0], other[1]], dd[:3]), b], allowed=[3], ms=4)
    case("filter in the second word of the bitset", [dense(0, keys_of_group(35, 3) + other[:4], dd[:7]), b], allowed=[35], ms=2)
    case("a dense key outside the table is never allowed", [dense(0, [N_ROWS + 5, g3[0], -7, g3[1]], dd[:4]), None], allowed=list(range(N_GROUPS)), ms=1)
    case("min_semantic 0", [dense(0, other[:4], dd[:4]), b], allowed=[3], ms=0)
    case("the top-up repeats a key", [dense(0, [other[0], other[0], g3[0], other[1]], dd[:4]), b], allowed=[3], ms=3)
    case("BM25 lists are not filtered", [dense(0, g3[:3], dd[:3]), sparse(3.0, other[:3], [3.0, 2.0, 1.0])], allowed=[3], ms=1)
    # bm25_keep_max: a lower score arrives later
    lower = [dense(0, [1], [0.3]), sparse(3.0, [7, 8], [4.0, 3.0]), dense(2, [2], [0.4]), sparse(0.75, [8, 7], [5.0, 1.5])]
    case("keep_max on, lower score later", lower, keep=True)
    case("keep_max off, lower score later", lower, keep=False)
    # top_n
    case("top_n above the distinct keys", [dense(0, k5, d5), sparse(3.0, [12, 77], [2.0, 1.0])], top_n=50)
    case("top_n below the distinct keys", [dense(0, k5, d5), sparse(3.0, [12, 77], [2.0, 1.0])], top_n=3)
    case("top_n 1", [dense(0, k5, d5), sparse(3.0, [12, 77], [2.0, 1.0])], top_n=1)
    return C


def sized_cases(rng):
    """name -> (lists, stride): entry counts at the wave's edges, a non-power-of-two total, and the documented maximum"""
    S = {}
    S["1 entry"] = ([dense(0, [3], [0.25]), None], 1)
    for n in (63, 64, 65):
        keys = rng.integers(0, 90, n)
        S[f"{n} entries"] = ([dense(0, keys, np.sort(rng.random(n).astype(np.float32))), sparse(3.0, rng.integers(0, 90, n), np.sort(rng.random(n))[::-1] + 0.1)], n)
    S["non-power-of-two total"] = (random_question(rng, 3, 37, fill=True, absent=0.0), 37)
    S["the maximum: 8 lists x 128, all distinct"] = ([dense(2 * i, range(256 * i, 256 * i + 128), np.sort(rng.random(128).astype(np.float32)))
                                                     if l == 0 else sparse(3.0 if i == 0 else 0.75, range(256 * i + 128, 256 * i + 256), np.sort(rng.random(128))[::-1] + 0.1)
                                                     for i in range(4) for l in range(2)], 128)
    S["the maximum: 2 lists x 512, overlapping"] = (random_question(rng, 1, 512, pool=700, fill=True, absent=0.0), 512)
    S["the maximum: 16 lists x 64"] = (random_question(rng, 8, 64, pool=300, fill=True, absent=0.0), 64)
    return S
