"""The BM25 kernels' model, its mutants and the named cases, shared by tests/test_bm25_model.py (CPU) and
tests/test_gpu_bm25_edges.py (GPU). The truth is bm25_oracle.CpuBm25 with bm25_oracle.topk; every comparison is bit equality.

  plan                 the launches rdx_bm25_search makes for (n_rows, k, nq): [(q0, queries of the launch)] (csrc/rdx_bm25.hip)
  mutant_search        what a WRONG kernel would return, in CpuBm25.search's format. Scorers: 1 terms summed in sorted order,
                       2 duplicates merged ((m * w) * x added once), 3 tf * (2.5 / (tf + denom)), 4 acc = fma(w, x, acc) (exact
                       rational arithmetic, rounded once), 5 the second 256-term chunk added before the first. Selectors: 6 score >= 0
                       passes, 7 ties by descending row, 8 ties by position inside the tile (then tile) instead of the global row,
                       9 the tiles from BM25_MERGE_THREADS on never merged, 10 the allow bitset's word index ignored (bit g & 31 of
                       word 0)
  from_docs            an index from integer token lists with rank_bm25's own idf: over the terms that occur, summed in
                       first-occurrence order (bm25_synth.arrays_from_tokens sums over the whole vocabulary in id order, which is
                       the same thing only while no idf is negative)
  CASES                name -> builder of a Case: the index, its runs (queries, k, allow bits, the mutants the run must tell from
                       the truth), the token lists for the BM25Okapi anchor where the case has them, and the facts the CPU test
                       asserts about the branch the case is built for

A case whose idf is overridden, or that is written as arrays, says so in `exempt`: BM25Okapi has no say there."""
from collections import Counter
from dataclasses import dataclass, field
from fractions import Fraction
from functools import lru_cache
from typing import Optional

import numpy as np

import bm25_oracle as O
import bm25_synth as S
from rag_dpo_amd import bm25

# csrc/bm25_kernel.hpp and csrc/rdx_bm25.hip; tests/test_bm25_model.py reads them out of the sources
TILE = 4096
THREADS = 256
TERM_CHUNK = 256
MAX_TERMS = 4096
MAX_K = 4096
MERGE_THREADS = 512
MERGE_CAP = 8192
WORKSPACE = 256 << 20          # bytes of tile partials per launch
GRID_Y = 65535                 # queries per launch at the most


def n_tiles(n_rows):
    return (n_rows + TILE - 1) // TILE


def chunk_of(n_rows, k, nq):
    return max(1, min(nq, WORKSPACE // (n_tiles(n_rows) * (12 * k + 4)), GRID_Y))


def plan(n_rows, k, nq):
    c = chunk_of(n_rows, k, nq) if nq else 1
    return [(q0, min(c, nq - q0)) for q0 in range(0, nq, c)]


def offsets(qs):
    off = np.zeros(len(qs) + 1, np.int64)
    np.cumsum([len(q) for q in qs], out=off[1:])
    ids = np.concatenate([np.asarray(q, np.int32) for q in qs]) if off[-1] else np.zeros(0, np.int32)
    return off, ids


def bits_of(groups, words):
    b = np.zeros(words, np.uint32)
    for g in groups:
        b[g >> 5] |= np.uint32(1 << (g & 31))
    return b


# ---- the truth and the mutants --------------------------------------------------------------------------------------------------------
def truth(a, qs, k, allow_bits=None):
    return O.CpuBm25(a).search(*offsets(qs), k, allow_bits)


def _fma(w, x, acc):
    fw = Fraction(float(w))
    return np.array([float(fw * Fraction(xi) + Fraction(si)) for xi, si in zip(x.tolist(), acc.tolist())])


def mutant_scores(a, ids, m):
    ids = [int(t) for t in ids]
    mult = Counter(ids)
    if m == 1:
        ids = sorted(ids)
    elif m == 2:
        ids = list(dict.fromkeys(ids))
    elif m == 5:
        ids = ids[TERM_CHUNK:2 * TERM_CHUNK] + ids[:TERM_CHUNK] + ids[2 * TERM_CHUNK:]
    score = np.zeros(a.n_rows)
    for t in ids:
        b, e = int(a.post_off[t]), int(a.post_off[t + 1])
        rows = a.post_row[b:e].astype(np.int64)
        tf = a.post_tf[b:e].astype(np.float64)
        w = a.idf[t]
        x = tf * (2.5 / (tf + a.denom[rows])) if m == 3 else (tf * 2.5) / (tf + a.denom[rows])
        if m == 2:
            score[rows] = score[rows] + (mult[t] * w) * x
        elif m == 4:
            score[rows] = _fma(w, x, score[rows])
        else:
            score[rows] = score[rows] + w * x
    return score


def mutant_topk(scores, k, allow_rows, m):
    idx = np.nonzero(scores >= 0 if m == 6 else scores > 0)[0]
    if allow_rows is not None:
        idx = idx[allow_rows[idx]]
    if m == 9:
        idx = idx[idx < MERGE_THREADS * TILE]
    s = scores[idx]
    if m == 7:
        order = idx[np.lexsort((-idx, -s))]
    elif m == 8:
        order = idx[np.lexsort((idx // TILE, idx % TILE, -s))]
    else:
        order = idx[np.argsort(-s, kind="stable")]
    order = order[:k]
    return order, scores[order]


def mutant_search(a, qs, k, allow_bits, m):
    nq = len(qs)
    sc, ro, cn = np.zeros((nq, k)), np.full((nq, k), -1, np.int64), np.zeros(nq, np.int32)
    allow = None
    if allow_bits is not None:
        gbits = np.unpackbits(np.asarray(allow_bits, np.uint32).view(np.uint8), bitorder="little").astype(bool)
        allow = gbits[a.row_group & 31] if m == 10 else gbits[a.row_group]
    cpu = O.CpuBm25(a)
    for q, ids in enumerate(qs):
        scores = mutant_scores(a, ids, m) if m in (1, 2, 3, 4, 5) else cpu.scores(ids)
        rows, s = mutant_topk(scores, k, allow, m)
        cn[q] = len(rows)
        ro[q, :len(rows)] = rows
        sc[q, :len(rows)] = s
    return sc, ro, cn


def differs(x, y):
    """(scores, rows, counts) of two searches differ somewhere, scores compared as bit patterns"""
    return bool((x[2] != y[2]).any() or (x[1] != y[1]).any() or (x[0].view(np.int64) != y[0].view(np.int64)).any())


def result_of(res, q):
    """one query's (count, rows, score bits), hashable"""
    return int(res[2][q]), res[1][q].tobytes(), res[0][q].tobytes()


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Run:
    name: str
    qs: list
    k: int
    allow: Optional[np.ndarray] = None
    mutants: tuple = ()


@dataclass
class Case:
    a: bm25.Bm25Arrays
    runs: list
    docs: Optional[list] = None        # the token lists the index was built from: the BM25Okapi anchor applies (<= 5000 rows)
    exempt: str = ""                   # why it does not
    facts: dict = field(default_factory=dict)

    _truth: dict = field(default_factory=dict, repr=False)

    def truth(self, run):
        """computed once per run, shared, never written to"""
        if run.name not in self._truth:
            t = truth(self.a, run.qs, run.k, run.allow)
            for x in t:
                x.setflags(write=False)
            self._truth[run.name] = t
        return self._truth[run.name]


def from_docs(docs, vocab, row_group=None, n_groups=0):
    n = len(docs)
    rows = np.repeat(np.arange(n, dtype=np.int64), [len(d) for d in docs])
    terms = np.concatenate([np.asarray(d, np.int64) for d in docs])
    a = S.arrays_from_tokens(n, vocab, rows, terms, row_group, n_groups)
    seen = np.array(list(dict.fromkeys(terms.tolist())), np.int64)
    idf = a.idf.copy()
    idf[seen], _ = bm25.idf_of(n, np.diff(a.post_off)[seen])
    a.idf = idf
    return a


def docs_of(n_rows, rows, terms):
    """token lists from a token stream whose rows ascend (bm25_synth.tokens without every_row_term)"""
    cut = np.searchsorted(rows, np.arange(1, n_rows))
    return [d.tolist() for d in np.split(terms, cut)]


def arrays_of(n_rows, postings, idf, denom=None, row_group=None, n_groups=0):
    """an index written directly: postings[t] = (rows ascending, tf scalar or array)"""
    off = np.zeros(len(postings) + 1, np.int64)
    np.cumsum([len(r) for r, _ in postings], out=off[1:])
    pr = np.concatenate([np.asarray(r, np.int32) for r, _ in postings]) if off[-1] else np.zeros(0, np.int32)
    pt = np.concatenate([np.broadcast_to(np.asarray(tf, np.uint16), (len(r),)) for r, tf in postings]) if off[-1] else np.zeros(0, np.uint16)
    den = np.full(n_rows, 1.5) if denom is None else np.asarray(denom, np.float64)
    return bm25.Bm25Arrays(n_rows, np.asarray(idf, np.float64), den, off, pr, np.ascontiguousarray(pt), row_group, n_groups)


def with_terms(a, postings):
    """`a` with terms appended behind its vocabulary (rank_bm25's idf over the new document frequencies; the denominators stay:
    the model is CpuBm25 over whatever arrays the index is made of)"""
    rows = [np.asarray(r, np.int32) for r, _ in postings]
    off = np.concatenate([a.post_off, a.post_off[-1] + np.cumsum([len(r) for r in rows])])
    pr = np.concatenate([a.post_row] + rows)
    pt = np.concatenate([a.post_tf] + [np.broadcast_to(np.asarray(tf, np.uint16), (len(r),)) for r, (_, tf) in zip(rows, postings)])
    idf, _ = bm25.idf_of(a.n_rows, np.diff(off))
    return bm25.Bm25Arrays(a.n_rows, idf, a.denom, off, pr, np.ascontiguousarray(pt), a.row_group, a.n_groups)


# ---- launch plan
CHUNK_ROWS, CHUNK_K = 64 * TILE - 5, MAX_K


@lru_cache(maxsize=None)
def case_workspace_chunks():
    """64 tiles at k = 4096: 85 queries per launch; 2 * 85 + 3 queries are three launches. Empty queries and queries of more than
    256 terms sit in the second and third launch; a term in most rows (every tile cut to k, the merge cut with tau) in the third"""
    a = S.make_by_term(CHUNK_ROWS, 2000, 6, seed=41)
    c = chunk_of(CHUNK_ROWS, CHUNK_K, 10 ** 6)
    nq = 2 * c + 3
    rng = np.random.default_rng(42)
    qs = [rng.integers(200, 2000, int(rng.choice([1, 1, 2, 3, 5]))).astype(np.int32) for _ in range(nq)]
    qs[c + 5] = np.zeros(0, np.int32)
    qs[c + 9] = rng.integers(200, 2000, 300).astype(np.int32)
    qs[2 * c + 1] = np.zeros(0, np.int32)
    qs[2 * c + 2] = rng.integers(100, 2000, 700).astype(np.int32)
    qs[2 * c] = np.array([0, 1500, 0], np.int32)
    return Case(a, [Run("batch", qs, CHUNK_K)], exempt="262 139 rows by term",
                facts={"chunk": c, "alone": (3, c + 9, 2 * c + 2), "empty": (c + 5, 2 * c + 1), "long": (c + 9, 2 * c + 2)})


GRID_NQ = GRID_Y + 6


@lru_cache(maxsize=None)
def case_grid_cap():
    """one tile, k = 1: the workspace allows millions of queries per launch, the grid's y extent 65 535; 65 541 queries of 0 to 3
    terms are two launches, the second of 6 queries"""
    rows, terms = S.tokens(50, 40, 8, seed=43)
    docs = docs_of(50, rows, terms)
    a = from_docs(docs, 40)
    rng = np.random.default_rng(44)
    lens = rng.integers(0, 4, GRID_NQ)
    flat = rng.integers(0, 40, int(lens.sum())).astype(np.int32)
    qs = np.split(flat, np.cumsum(lens)[:-1])
    return Case(a, [Run("batch", qs, 1)], docs=docs, facts={"chunk": GRID_Y})


MERGE_ROWS = MERGE_THREADS * TILE + 1
PLANT_511, PLANT_512 = 511 * TILE + 1234, MERGE_ROWS - 1


@lru_cache(maxsize=None)
def case_merge_rounds():
    """512 * 4096 + 1 rows = 513 tiles, tile 512 of one row: the fewest with which k_bm25_merge's tile loop takes a second round.
    Term 2000 is planted (tf 9) in a row of tile 0, one of tile 511 and the single row of tile 512; with it in the query those
    rows head the answer"""
    base = S.make_by_term(MERGE_ROWS, 2000, 6, seed=45)
    a = with_terms(base, [([77, PLANT_511, PLANT_512], 9)])
    common, rare = [0, 2000], [1990, 2000, 1995]
    return Case(a, [Run("k4096", [common, rare, [0]], MAX_K, mutants=(8, 9)), Run("k50", [common, rare], 50, mutants=(8, 9))],
                exempt="2.1 M rows by term", facts={"plant": (77, PLANT_511, PLANT_512)})


# ---- sign and zero
def _half_docs():
    """300 rows; term 0 in exactly 150 of them (idf exactly 0.0); terms 1 to 19 in 8 to 46 rows (positive idf)"""
    rng = np.random.default_rng(46)
    docs = [[] for _ in range(300)]
    for r in rng.choice(300, 150, replace=False):
        docs[r] += [0] * int(rng.integers(1, 4))
    for t in range(1, 20):
        for r in rng.choice(300, 8 + 2 * t, replace=False):
            docs[r] += [t] * int(rng.integers(1, 3))
    for r in range(300):
        docs[r] += [20 + r % 7]                  # no empty row
        rng.shuffle(docs[r])
    return docs


@lru_cache(maxsize=None)
def case_idf_zero():
    docs = _half_docs()
    a = from_docs(docs, 27)
    return Case(a, [Run("alone", [[0], [0, 0, 0]], 300, mutants=(6,)),
                    Run("mixed", [[0, 3, 0, 5], [7, 0], [0, 12, 12, 0, 4]], 300, mutants=(6,))], docs=docs)


def _floor_docs(n, rare_rows):
    """terms 0 to 9 in about 90 % of the rows (negative idf, floored to epsilon * a negative average), terms 10, 11, 12 rare"""
    rng = np.random.default_rng(47 + n)
    docs = [[t for t in range(10) if rng.random() < 0.9] * int(rng.integers(1, 3)) for _ in range(n)]
    for t, rows in zip((10, 11, 12), rare_rows):
        for r in rows:
            docs[r] += [t] * (1 + r % 3)
    for d in docs:
        if not d:
            d.append(0)
    return docs


@lru_cache(maxsize=None)
def case_negative_floor():
    rng = np.random.default_rng(48)
    docs = _floor_docs(300, [rng.choice(300, m, replace=False) for m in (70, 85, 95)])
    a = from_docs(docs, 13)
    return Case(a, [Run("mixed", [[10, 0, 11, 1, 2], [0, 10], [12, 5, 5, 11]], 300, mutants=(1, 6)),
                    Run("negative only", [[0, 1, 2], [5], [9, 9, 3]], 7)], docs=docs)


@lru_cache(maxsize=None)
def case_negative_tile():
    """three tiles; the rare (positive) terms only in tiles 0 and 2: tile 1 has postings of the query and no passing row"""
    n = 3 * TILE - 7
    rng = np.random.default_rng(49)
    pool = np.concatenate([np.arange(TILE), np.arange(2 * TILE, n)])
    docs = _floor_docs(n, [rng.choice(pool, m, replace=False) for m in (900, 1100, 1300)])
    a = from_docs(docs, 13)
    return Case(a, [Run("mixed", [[10, 0, 11, 1, 2], [3, 12]], MAX_K, mutants=(6,))], exempt="12 281 rows (natural idf)")


CANCEL_ROW, KEPT_ROW = 4100, 4200


@lru_cache(maxsize=None)
def case_cancellation():
    """written as arrays, idf overridden: terms 0 (+1) and 1 (-1) have equal postings and tf, so their rows score +0.0 exactly and
    must be absent; term 2 (+0.5) brings row KEPT_ROW back above zero, in one query only from position 300 (the second term chunk);
    term 3 has postings elsewhere (the filler of that query), term 4 (-2) is negative"""
    n = 2 * TILE + 3
    both = np.array([5, 4095, 4096, CANCEL_ROW, KEPT_ROW, 2 * TILE + 2])
    tf = np.array([1, 7, 65535, 3, 2, 1], np.uint16)
    post = [(both, tf), (both, tf), ([KEPT_ROW, 6000], 4), (np.arange(100, 200), 1), ([5, 300, KEPT_ROW], 2)]
    den = 0.4 + np.random.default_rng(50).random(n) * 3
    a = arrays_of(n, post, [1.0, -1.0, 0.5, 0.25, -2.0], den)
    late = [0, 1] + [3] * 298 + [2]
    return Case(a, [Run("cancel", [[0, 1], [1, 0], [0, 1, 0, 1]], 64, mutants=(6,)),
                    Run("late", [late, [0, 1, 2], [2, 0, 1]], 200, mutants=(6,)),
                    Run("negative only", [[1], [4, 1], [1, 4, 4]], 16)],
                exempt="idf overridden (+1, -1, +0.5, +0.25, -2)", facts={"late": late})


# ---- arithmetic
Q10 = [3, 17, 3, 0, 25, 9, 3, 17, 30, 1]


def _dense_queries(seed):
    rng = np.random.default_rng(seed)
    q300 = rng.integers(0, 40, 300).astype(np.int32)
    q300[TERM_CHUNK] = q300[TERM_CHUNK - 1] = 11           # an equal pair across the term-chunk boundary
    q300[:3] = (39, 38, 39)                                # and an order a sort would change, in both chunks
    q300[-3:] = (2, 1, 0)
    return q300, rng.integers(0, 40, MAX_TERMS).astype(np.int32)


@lru_cache(maxsize=None)
def case_dense_vocab(n):
    """vocab 40, mean length 30: every row holds most of a query's terms, so every addition's rounding shows. k = 4096 >= the
    passing rows at n = TILE - 1 (every row's bits compared); n = 4097 adds the second tile (one row is cut)"""
    rows, terms = S.tokens(n, 40, 30, seed=51)
    docs = docs_of(n, rows, terms)
    a = from_docs(docs, 40)
    q300, q4096 = _dense_queries(52)
    runs = [Run("ten terms", [Q10, [5, 5], [8, 2, 8]], MAX_K, mutants=(1, 2, 3, 4)),
            Run("pair at 255 | 256", [q300], MAX_K, mutants=(1, 2, 3, 5))]
    if n > TILE:
        runs.append(Run("4096 terms", [q4096], MAX_K, mutants=(1, 2, 3, 5)))
    return Case(a, runs, docs=docs)


@lru_cache(maxsize=None)
def case_tf_extremes():
    """tf 65535 and tf 1 of one term; rows of length 1 and a row of 200 000 tokens: denom from 0.38 to 1.3e2"""
    rng = np.random.default_rng(53)
    docs = [rng.integers(10, 300, int(rng.integers(5, 60))).tolist() for _ in range(200)]
    for t in (3, 4, 5, 6):
        for r in rng.choice(200, 40, replace=False):
            docs[r] += [t] * int(rng.integers(1, 4))
    docs[0] = [3] * 65535 + [4]
    docs[1] = [3]
    docs[2] = [t for t in (3, 4, 5, 6) for _ in range(50000)]
    docs[3] = [4] * 65535 + [3] * 2 + [5]
    docs[4] = [5]
    a = from_docs(docs, 300)
    return Case(a, [Run("extremes", [[3, 4, 3, 5], [5, 3], [4, 4, 6, 3]], 200, mutants=(1, 2, 3, 4))], docs=docs)


# ---- ties across tiles
@lru_cache(maxsize=None)
def case_plateau():
    """five tiles, one term with tf 1 in every row, equal denominators: one plateau over everything; the answer is rows 0 to k - 1"""
    n = 5 * TILE
    a = arrays_of(n, [(np.arange(n), 1)], [1.0])
    return Case(a, [Run(f"k{k}", [[0]], k, mutants=(7, 8) if k > 1 else (7,)) for k in (1, MAX_K - 1, MAX_K)],
                exempt="written as arrays, idf 1.0")


PLATEAU_FROM = 2000


@lru_cache(maxsize=None)
def case_plateau_mid_tile():
    """the plateau starts in the middle of tile 0; three rows of the last tile score higher (two of them equal)"""
    n = 5 * TILE - 9
    top = [4 * TILE + 17, 4 * TILE + 3000, 4 * TILE + 500]          # in result order: tf 5, 5, 2
    a = arrays_of(n, [(np.arange(PLATEAU_FROM, n), 1), (sorted(top), [5, 2, 5])], [1.0, 1.0])
    runs = [Run(f"k{k}", [[0, 1], [0]], k, mutants=(7, 8)) for k in (2, 4, MAX_K - 1, MAX_K)]
    return Case(a, [Run("k1", [[0, 1], [0]], 1, mutants=(8,))] + runs, exempt="written as arrays, idf 1.0", facts={"top": top})


# ---- groups
GROUP_COUNTS = (1, 31, 32, 33, 64, 65)


@lru_cache(maxsize=None)
def case_groups(g):
    """TILE + 50 rows, group = row % g; the allow bitset is two words longer than needed, those words and the bits past g set"""
    n = TILE + 50
    rows, terms = S.tokens(n, 60, 12, seed=54)
    docs = docs_of(n, rows, terms)
    a = from_docs(docs, 60, (np.arange(n) % g).astype(np.int32), g)
    words = (g + 31) // 32

    def bits(groups):
        b = np.concatenate([bits_of(groups, words), np.full(2, 0xFFFFFFFF, np.uint32)])
        if g % 32:
            b[words - 1] |= np.uint32((0xFFFFFFFF << (g % 32)) & 0xFFFFFFFF)
        return b

    qs = [[1, 7, 1], [30], [4, 59, 12, 4]]
    runs = [Run("last", qs, 100, bits([g - 1]), mutants=(10,) if g > 32 else ()), Run("all", qs, 100, bits(range(g))),
            Run("none", qs, 100, bits([])), Run("no filter", qs, 100)]
    for only in (31, 32):
        if only < g:
            runs.append(Run(f"only {only}", qs, 100, bits([only]), mutants=(10,) if only == 32 else ()))
    return Case(a, runs, docs=docs, facts={"words": words})


# ---- index shapes
@lru_cache(maxsize=None)
def case_one_row():
    """rank_bm25 at N = 1: every idf is log(0.5) - log(1.5) < 0, floored to a negative: nothing passes"""
    docs = [[0, 1, 0]]
    return Case(from_docs(docs, 2), [Run("natural", [[0], [1, 0], []], 1), Run("k7", [[0]], 7)], docs=docs)


@lru_cache(maxsize=None)
def case_one_row_positive():
    a = arrays_of(1, [([0], 3), ([0], 1)], [1.0, 0.5], [0.7])
    return Case(a, [Run("k1", [[0], [1, 0], []], 1), Run("k4096", [[0, 1, 1]], MAX_K)], exempt="idf overridden (+1, +0.5)")


@lru_cache(maxsize=None)
def case_no_terms():
    a = arrays_of(3, [], np.zeros(0))
    return Case(a, [Run("empty queries", [[], [], []], 2)], exempt="no vocabulary")


@lru_cache(maxsize=None)
def case_shapes():
    """2 tiles + 10 rows. Term 1's postings are exactly rows 4095 and 4096; term 2 fills exactly tile 1; term 6, the last one with
    postings, ends at nnz (the directory's last entry); term 7, the vocabulary's last, has no postings; term 5 has none either"""
    n = 2 * TILE + 10
    rng = np.random.default_rng(55)
    docs = [[0] * int(rng.integers(1, 4)) if rng.random() < 0.3 else [3] for _ in range(n)]
    docs[TILE - 1] += [1, 1]
    docs[TILE] += [1]
    for r in range(TILE, 2 * TILE):
        docs[r] += [2] * (1 + r % 2)
    for r in (7, 4000, 2 * TILE + 9):
        docs[r] += [6]
    docs[9] += [4]
    a = from_docs(docs, 8)
    return Case(a, [Run("shapes", [[1], [2], [6], [7], [5, 6, 7], [7, 5], [2, 1, 6, 0, 4]], MAX_K),
                    Run("k3", [[1], [2], [6], [2, 1]], 3)], exempt="8 202 rows (natural idf)")


CASES = {"workspace-chunks": (case_workspace_chunks,), "grid-cap": (case_grid_cap,), "merge-rounds": (case_merge_rounds,),
         "idf-zero": (case_idf_zero,), "negative-floor": (case_negative_floor,), "negative-tile": (case_negative_tile,),
         "cancellation": (case_cancellation,), "dense-4097": (case_dense_vocab, TILE + 1), "dense-4095": (case_dense_vocab, TILE - 1),
         "tf-extremes": (case_tf_extremes,), "plateau": (case_plateau,), "plateau-mid-tile": (case_plateau_mid_tile,),
         "one-row": (case_one_row,), "one-row-positive": (case_one_row_positive,), "no-terms": (case_no_terms,),
         "shapes": (case_shapes,)}
CASES.update({f"groups-{g}": (case_groups, g) for g in GROUP_COUNTS})


def case(name):
    f, *args = CASES[name]
    return f(*args)
