"""Score landscapes for the top-k selection kernels — a helper, not a test.

The selectors (K5b select_dense_query, the endings of k_refine, the merges, rank_and_write) promise ONE order: score descending,
ties by ascending row id, scores compared as floats (+0.0 == -0.0; include/rdx.h, oracle/rdx_oracle.c `before`). On random
Gaussian corpora every top-k score is positive and distinct and their branchy parts are reached by accident. Here the corpora
are built from a few sparse directions so that the EXACT scores take designed values:

  column E0  a tiny component (1e-25) whose product with the query's is +-1e-50 in fp64: (float) of it is a SIGNED ZERO
  column E1  the bulk of a row (carries no score: the queries hold 0 there)
  column E2  the score: a row (sqrt(1 - s^2) E1 + s E2) scores s against the query E2
  column E3  queries only: spreads the queries of a batch (another norm, hence other score bits, the same order)
  columns 4+ optional Gaussian filler (the queries hold 0 there): makes "other" rows distinct

Distinct levels come from distinct rows, a plateau is bit-identical scores from identical rows, negative levels come from
negated scores. Every builder returns (corpus, queries, facts); `facts` is computed from the oracle's own scores
(oracle.scores on oracle.normalize_rows) and `facts.at(k, allow)` gives, per query, what a test asserts BEFORE it touches the
GPU: how many scores lie strictly above the k-th, the plateau at the k-th, the counts of +0.0 and -0.0, and whether the order
of the radix keys (f2key, -0.0 strictly below +0.0) would give another answer than the documented order.

The edges the landscapes are built around (tests/test_selection_landscapes.py compares them with the kernels' sources):"""
import numpy as np

EQ_CAP = 1024           # k_rows.hpp: ties at the k-th ranked from a side list up to here, by an in-order walk beyond
RN = 32                 # k_rows.hpp: K5b keeps score rows of up to RN * 1024 in registers
SELECT_MAX_K = 4096     # rows_core.hpp: largest k of a search
REFINE_PMAX = 1024      # refine_kernel.hpp: the ranking arrays of k_refine
MERGE_MAX = 4096        # merge_kernel.hpp: most candidates per query one k_merge launch ranks
REG_ROWS = RN * 1024    # 32 768: the register form of K5b up to here, the global form beyond

TINY = 1e-25
E0, E1, E2, E3, FILL0 = 0, 1, 2, 3, 4


def f2key(s):
    """numpy restatement of rdx_common.hpp f2key (monotone float -> uint32): what the radix selects order by"""
    u = np.ascontiguousarray(s, dtype=np.float32).view(np.uint32)
    return np.where(u >> 31, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def order_documented(scores, rows):
    """score desc (as floats: the zeros tie), row asc"""
    return rows[np.lexsort((rows, -scores.astype(np.float64)))]


def order_by_keys(scores, rows):
    """radix key desc (-0.0 below +0.0), row asc: what a selector that trusts f2key for ties computes"""
    return rows[np.lexsort((rows, -f2key(scores).astype(np.int64)))]


class Facts:
    """the oracle's scores of every (query, row) of a landscape and what they say about a top-k"""

    def __init__(self, oracle, corpus, queries):
        ch = oracle.normalize_rows(corpus)
        qh = oracle.normalize_rows(queries)
        self.scores = np.stack([oracle.scores(ch, qh[b]) for b in range(qh.shape[0])])
        self.n = corpus.shape[0]

    def at(self, k, allow=None):
        out = []
        rows_all = np.arange(self.n, dtype=np.int64)
        keep = rows_all if allow is None else rows_all[np.asarray(allow, dtype=bool)]
        for b in range(self.scores.shape[0]):
            s = self.scores[b, keep]
            kk = min(k, keep.shape[0])
            zero = s == 0
            f = {"valid": int(keep.shape[0]), "kk": kk, "pos_zero": int((zero & ~np.signbit(s)).sum()),
                 "neg_zero": int((zero & np.signbit(s)).sum())}
            doc = order_documented(s, keep)[:kk]
            f["rows"] = doc
            if kk:
                kth = self.scores[b, doc[kk - 1]]
                f["kth"] = float(kth)
                f["n_gt"] = int((s > kth).sum())
                f["plateau"] = int((s == kth).sum())
                f["need_eq"] = kk - f["n_gt"]
                f["key_order_differs"] = not np.array_equal(doc, order_by_keys(s, keep)[:kk])
                f["negative_in_list"] = int((self.scores[b, doc] < 0).sum())
            out.append(f)
        return out


def make_rows(level, zsign, d, fill=None):
    """row i = zsign[i] * TINY * E0 + sqrt(1 - level[i]^2) * E1 + level[i] * E2 (+ fill[i] in the columns from FILL0 on)"""
    level = np.asarray(level, dtype=np.float64)
    x = np.zeros((level.shape[0], d), dtype=np.float32)
    x[:, E0] = np.asarray(zsign, dtype=np.float64) * TINY
    x[:, E1] = np.sqrt(1.0 - level * level)
    x[:, E2] = level
    if fill is not None:
        x[:, FILL0:] = fill
    return x


def make_queries(nq, d, flip=True):
    """query j = +-TINY * E0 + E2 + 0.25 j * E3: every second one (flip) turns the sign of every zero score"""
    q = np.zeros((nq, d), dtype=np.float32)
    q[:, E0] = TINY
    if flip:
        q[1::2, E0] = -TINY
    q[:, E2] = 1.0
    q[:, E3] = 0.25 * (np.arange(nq) % 7)
    return q


def signed_zeros(oracle, n=3000, tiles=1, nq=1, n_zero=None, d=64):
    """q = TINY E0 + E2; rows = +-TINY E0 + E1, the sign from default_rng(0); four rows also get +0.5 E2 (score 0.4472136).
    n = 3000: 4 x 0.4472136, 1563 x +0.0 and 1433 x -0.0 for the first query; the documented top-10 is [143 653 1474 1969 0 1 2 3 4 5],
    the order of the radix keys gives [143 653 1474 1969 0 1 2 9 10 11].
    n_zero: only that many rows (spread over the corpus) stay zeros, the others take distinct negative scores with filler.
    tiles: the corpus repeated (rows past 32 768: the global form of K5b); every score then occurs `tiles` times."""
    rng = np.random.default_rng(0)
    sign = np.where(rng.integers(0, 2, size=n) == 1, 1.0, -1.0)
    x = make_rows(np.zeros(n), sign, d)
    x[[143, 653, 1474, 1969], E2] = 0.5
    if n_zero is not None:
        r2 = np.random.default_rng(1)
        others = np.setdiff1d(np.arange(n), [143, 653, 1474, 1969])
        neg = np.sort(r2.permutation(others)[: others.shape[0] - n_zero])
        x[neg, E2] = -(0.3 + 0.5 * r2.random(neg.shape[0]))
        x[neg, FILL0:] = 0.05 * r2.standard_normal((neg.shape[0], d - FILL0))
    corpus = np.tile(x, (tiles, 1))
    queries = make_queries(nq, d)
    return corpus, queries, Facts(oracle, corpus, queries)


def mfma_zeros(oracle, n=40_000, plateau=1500, nq=8, d=64):
    """the signed-zero edge behind the MFMA scan: 4 positives (0.4472136), a zero plateau of mixed sign at random rows, and every
    other row spread over [-0.76, -0.56] — a threshold sampled from the corpus lands in that spread or at the zeros, never floods
    the candidate segments. The documented order and the order of the radix keys differ from place 5 on."""
    rng = np.random.default_rng(7)
    level = -(0.56 + 0.2 * rng.random(n))
    zsign = np.zeros(n)
    perm = rng.permutation(n)
    zrows, prow = perm[:plateau], perm[plateau:plateau + 4]
    level[zrows] = 0.0
    zsign[zrows] = np.where(rng.integers(0, 2, size=plateau) == 1, 1.0, -1.0)
    level[prow] = 0.4472136
    corpus = make_rows(level, zsign, d)
    queries = make_queries(nq, d)
    return corpus, queries, Facts(oracle, corpus, queries)


def plateau_at_kth(oracle, n, size, level, n_above=7, nq=1, d=64):
    """`size` identical rows (score `level`) at HIGH row ids, every second row of the corpus' tail, interleaved with and behind
    lower-scoring rows; n_above rows with distinct higher scores spread over the low rows. k = n_above + need_eq puts the k-th
    place at depth need_eq of the plateau."""
    rng = np.random.default_rng(size * 7 + n)
    lv = level - 0.05 - 0.5 * rng.random(n)
    assert 2 * size <= n // 2
    lv[n - 2 * size + 1:: 2] = level
    above = (np.arange(1, n_above + 1) * (n // (4 * (n_above + 1)))) + 3
    lv[above] = level + 0.04 * np.arange(1, n_above + 1)
    corpus = make_rows(lv, np.zeros(n), d)
    queries = make_queries(nq, d, flip=False)
    return corpus, queries, Facts(oracle, corpus, queries)


def tie_groups(oracle, n, nq=3, d=64, group=3):
    """many small tie groups: n rows drawn (with repetition) from n / group distinct Gaussian rows; Gaussian queries"""
    rng = np.random.default_rng(n + d)
    pool = rng.standard_normal((max(1, n // group), d)).astype(np.float32)
    corpus = pool[rng.integers(0, pool.shape[0], size=n)]
    queries = rng.standard_normal((nq, d)).astype(np.float32)
    return corpus, queries, Facts(oracle, corpus, queries)


def negatives(oracle, n, nq=2, d=64, crossing=False):
    """every row on the far side of the query: scores in [-0.9, -0.1], drawn from n / 2 distinct levels (ties among the negatives).
    crossing: rows 40..48 become three -0.0, three positives and three +0.0 (the -0.0 rows at the lowest ids), so a list of
    k > 9 runs from positive through both zeros into the negatives."""
    rng = np.random.default_rng(n + 17)
    pool = -(0.1 + 0.8 * rng.random(max(1, n // 2)))
    level = pool[rng.integers(0, pool.shape[0], size=n)]
    zsign = np.zeros(n)
    if crossing:
        level[40:43] = 0.0
        zsign[40:43] = -1.0
        level[43:46] = [0.2, 0.3, 0.2]
        level[46:49] = 0.0
        zsign[46:49] = 1.0
    corpus = make_rows(level, zsign, d)
    queries = make_queries(nq, d, flip=False)
    return corpus, queries, Facts(oracle, corpus, queries)


def shard_parts(oracle, corpus, queries, n_parts, k, allow=None):
    """per-shard answers of a landscape, rows dealt round-robin (shard p holds rows p, p + n_parts, ...), with GLOBAL row ids:
    (score [P][B][k], row [P][B][k], count [P][B]) — what a merge is given"""
    ch = oracle.normalize_rows(corpus)
    B = queries.shape[0]
    ps = np.empty((n_parts, B, k), dtype=np.float32)
    pr = np.empty((n_parts, B, k), dtype=np.int64)
    pc = np.empty((n_parts, B), dtype=np.int32)
    for p in range(n_parts):
        ids = np.arange(p, corpus.shape[0], n_parts, dtype=np.int64)
        s, r, c = oracle.cosine_topk(ch[ids], queries, k, None if allow is None else allow[ids])
        ps[p], pc[p] = s, c
        pr[p] = np.where(r >= 0, ids[np.clip(r, 0, None)], -1)
    return ps, pr, pc


# ---- every landscape the suite uses, by name: (builder, [(k, mask name or None), ...]) ------------------------------------------
# tests/test_selection_landscapes.py pins the reference order on each of them; tests/test_gpu_selection_order.py runs them on the GPU.

def masks(n):
    """the row bitmaps the tests use, by name"""
    rng = np.random.default_rng(n)
    low = np.ones(n, dtype=bool)
    low[[0, 1, 4, 9, 10]] = False                    # hides some of the low-row zeros of signed_zeros
    few = np.zeros(n, dtype=bool)
    few[rng.permutation(n)[:100]] = True             # leaves 100 rows: k above that walks over masked (-inf) entries
    return {None: None, "low": low, "few": few, "none": np.zeros(n, dtype=bool)}


PLATEAU_SIZES = [1, 2, 1023, 1024, 1025, 3000]
PLATEAU_ROWS = [REG_ROWS, REG_ROWS + 1, 20_011]      # the last register row count, the first global one, one off the 1024 grid
K_RANGE = [1, 257, 1000, 4095, 4096]


def need_eqs(size):
    return sorted({1, max(1, size // 2), size})


def catalogue():
    """name -> (builder(oracle) -> (corpus, queries, facts), [(k, mask name), ...]); k = None: chosen by the test from facts"""
    cat = {}
    cat["zeros_3000"] = (lambda o: signed_zeros(o, 3000, nq=6), [(10, None), (10, "low"), (5, None), (3000, None), (1500, "low")])
    cat["zeros_3000_few"] = (lambda o: signed_zeros(o, 3000, nq=6, n_zero=600), [(10, None), (10, "low"), (5, None), (604, None), (300, "low")])
    cat["zeros_tiled"] = (lambda o: signed_zeros(o, 3000, tiles=12, nq=6), [(58, None), (58, "low"), (49, None), (4096, None)])
    cat["zeros_tiled_few"] = (lambda o: signed_zeros(o, 3000, tiles=12, nq=6, n_zero=60), [(58, None), (58, "low"), (49, None), (768, None)])
    for plateau in (40, 1500):
        for d in (64, 128):
            cat[f"mfma_zeros_{plateau}_d{d}"] = (lambda o, p=plateau, d=d: mfma_zeros(o, 40_000, p, nq=8, d=d), [(10, None), (5, None), (44, None)])
    for n in PLATEAU_ROWS:
        for size in PLATEAU_SIZES:
            for level in (0.35, -0.35):
                cat[f"plateau_{n}_{size}_{'neg' if level < 0 else 'pos'}"] = (
                    lambda o, n=n, size=size, level=level: plateau_at_kth(o, n, size, level), [(7 + e, None) for e in need_eqs(size)])
    for n in (5000, 40_000):
        cat[f"ties_{n}"] = (lambda o, n=n: tie_groups(o, n), [(k, None) for k in K_RANGE] + [(257, "few"), (10, "none")])
    cat["ties_3000"] = (lambda o: tie_groups(o, 3000), [(4096, None)])
    cat["ties_5000_d256"] = (lambda o: tie_groups(o, 5000, d=256), [(257, None)])
    for n in (5000, 40_000):
        cat[f"negatives_{n}"] = (lambda o, n=n: negatives(o, n), [(10, None), (200, None)])
        cat[f"crossing_{n}"] = (lambda o, n=n: negatives(o, n, crossing=True), [(4, None), (8, None), (12, None), (200, None)])
    return cat
