"""Numpy model of the int8 coarse pass as the kernels document it (DESIGN.md §5 "int8 coarse pass" and "two-round re-score"), shared
by tests/test_i8_model.py (CPU) and tests/test_gpu_i8_bound.py / tests/test_gpu_i8_refine.py (GPU). Built on the per-block quantiser
of test_i8_bound_model.py (quant_rows / quant_query) and on e_q / sub_down / kth_largest of test_i8_refine_model.py; the vectorised
quantisers here are checked against those in tests/test_i8_model.py.

  quant_blocks / quant_queries   k_quant8_corpus / k_quant8_query: any n (the last block's scale and eps_b cover its nr real rows, rows
                                 past n and columns past dim are zeros), all-zero blocks (s_b = 0, inv = 0), zero queries (t_q = 1);
                                 the error terms are rounded UP to float32 only when the conversion fell short (f32_up)
  Copy8                          what prepare_i8 keeps between searches: the watermark (an append re-quantises from the last partial
                                 block on, an update or a compaction rebuilds everything), and eps_max as the running maximum over every
                                 block quantisation since the last full rebuild (which resets it)
  predict                        per query S1, X1, t3 = sub_down(X1, E_q), |{coarse >= t3}| for a pilot and an optional allow mask, the
                                 queries that qualify, and the counts the MUTANTS of the bound would give on those queries

The rows the model starts from are the ones the C oracle normalises (the bits the library's master holds). The compact bf16 master
recomputes (float)((double)x / den) from the widened bf16 values, the oracle's own operation: the oracle's rows of the widened values ARE
MasterRow's, no separate model of it is needed (tests/test_gpu_i8_bound.py::test_compact_bf16_master asserts the score bits)."""
from dataclasses import dataclass
from typing import Optional

import numpy as np

import test_i8_refine_model as RM
from rag_dpo_amd import synth
from test_i8_bound_model import F32

REFINE_PMAX = 1024           # refine_kernel.hpp: a band with more rows than this is re-scored in place (not what is measured here)
REFINE_LIST = 7168           # rdx_limits.hpp: a query with more hits than this goes to the fallback passes
K = 10


def f32_up(x):
    """k_rows.hpp f32_up: the float32 >= x (x >= 0, float64)"""
    x = np.asarray(x, np.float64)
    f = x.astype(F32)
    return np.where(f.astype(np.float64) < x, np.nextafter(f, F32(np.inf)), f).astype(F32)


def quant_blocks(y):
    """y: [n, d] float32, n any -> (s [nb], c8 [32 nb, d] as float32 integers, eps [nb]) as k_quant8_corpus computes them"""
    n, d = y.shape
    nb = (n + 31) // 32
    yb = np.zeros((nb * 32, d), F32)
    yb[:n] = y
    yb = yb.reshape(nb, 32, d)
    mx = np.abs(yb).max(axis=(1, 2)).astype(F32)                         # (the padding rows are zeros: the max over the nr real rows)
    s = (mx / F32(127)).astype(F32)
    with np.errstate(divide="ignore"):
        inv = np.where(mx > 0, F32(1) / s, F32(0)).astype(F32)
    c8 = np.clip(np.rint((yb * inv[:, None, None]).astype(F32)), -127, 127).astype(F32)
    err = yb.astype(np.float64) - s.astype(np.float64)[:, None, None] * c8
    eps = f32_up(np.sqrt((err * err).sum(axis=2).max(axis=1)) * (1 + 1e-12))
    return s, c8.reshape(nb * 32, d), eps


def quant_queries(qh):
    """qh: [nq, d] normalised queries -> (t, q8 as float32 integers, e, n) as k_quant8_query computes them"""
    mx = np.abs(qh).max(axis=1).astype(F32)
    t = np.where(mx > 0, mx / F32(127), F32(1)).astype(F32)
    inv = np.where(mx > 0, F32(1) / t, F32(0)).astype(F32)
    q8 = np.clip(np.rint((qh * inv[:, None]).astype(F32)), -127, 127).astype(F32)
    a = t.astype(np.float64)[:, None] * q8
    e = f32_up(np.sqrt(((qh.astype(np.float64) - a) ** 2).sum(axis=1)) * (1 + 1e-12))
    nn = f32_up(np.sqrt((a * a).sum(axis=1)) * (1 + 1e-12))
    return t, q8, e, nn


def e_q(e, nn, eps_max):
    return np.array([RM.e_q(a, b, eps_max) for a, b in zip(e, nn)], F32)


def coarse_scores(c8, s, t, q8, n):
    """[nq, n] float32: (float)D * s_b * t_q, the products in that order (k_scan<I8>'s epilogue)"""
    D = c8[:n] @ q8.T                                    # integers, |D| <= 127^2 * 1024 < 2^24 with every partial sum: exact in float32
    assert np.abs(D).max() < 2 ** 24
    cs = (D * np.repeat(s, 32)[:n, None]).astype(F32)
    return np.ascontiguousarray((cs * t[None, :]).astype(F32).T)


@dataclass
class State:
    """the int8 copy at one search"""
    s: np.ndarray
    c8: np.ndarray
    eps_max: F32
    eps_before: F32                      # eps_max as it was before the quantisation this search ran (mutant 5)
    eps_full: F32                        # the running maximum over FULL blocks only (mutant 4)
    stale: Optional[tuple] = None        # (s, c8, eps_max) had the append left the last partial block alone (mutant 6)


class Copy8:
    """prepare_i8's state across searches and writes. The tests reserve the final row count before the first search: an append
    does not reallocate the copy (a reallocation would be a full rebuild)."""

    def __init__(self):
        self.valid = 0
        self.s = self.c8 = None
        self.eps_max = self.eps_full = F32(0)

    def appended(self, row0):
        self.valid = min(self.valid, row0 // 32 * 32)

    def rewritten(self):                                  # update, compact
        self.valid = 0

    def prepare(self, y):
        n, d = y.shape
        before, stale = self.eps_max, None
        if self.valid < n:
            if self.valid == 0:
                self.s, self.c8 = np.zeros(0, F32), np.zeros((0, d), F32)
                self.eps_max = self.eps_full = F32(0)
            b0 = self.valid // 32
            s, c8, eps = quant_blocks(y[32 * b0:])
            if len(self.c8) == 32 * (b0 + 1):                               # an append onto a partial block (the copy ends inside it)
                s1, c81, eps1 = quant_blocks(y[32 * (b0 + 1):]) if n > 32 * (b0 + 1) else (np.zeros(0, F32), np.zeros((0, d), F32), np.zeros(0, F32))
                stale = (np.concatenate([self.s, s1]), np.concatenate([self.c8, c81]), max([self.eps_max] + list(eps1)))
            full = eps[:len(eps) - (1 if n % 32 else 0)]
            self.s = np.concatenate([self.s[:b0], s])
            self.c8 = np.concatenate([self.c8[:32 * b0], c8])
            self.eps_max = max(self.eps_max, eps.max())
            self.eps_full = max([self.eps_full] + list(full))
            self.valid = n
        return State(self.s, self.c8, F32(self.eps_max), F32(before), F32(self.eps_full), stale)


def coarse_model(oracle, corpus, q):
    """a fresh index of `corpus` searched with `q`: (rows, queries as the C oracle normalises them, coarse [nq, n], E_q [nq])"""
    y, qh = oracle.normalize_rows(corpus), oracle.normalize_rows(q)
    st = Copy8().prepare(y)
    t, q8, e, nn = quant_queries(qh)
    return y, qh, coarse_scores(st.c8, st.s, t, q8, len(y)), e_q(e, nn, st.eps_max)


def _count(cs, t3):
    return int((cs >= t3).sum())


def _rounds(oracle, cs, rows, y, qv, Eq, k, pilot):
    """(|S1|, X1, |{coarse >= t3}|) over the allowed rows `rows`, cs = their coarse scores"""
    top = np.argsort(-cs.astype(np.float64), kind="stable")
    S1 = np.flatnonzero(cs >= cs[top[pilot * k - 1]])
    X1 = RM.kth_largest(oracle.scores(y[rows[S1]], qv), k)
    return len(S1), X1, _count(cs, RM.sub_down(X1, Eq))


MUTANTS = (1, 2, 3, 4, 5, 6, "7-", "7+")


@dataclass
class Prediction:
    """use: the qualifying queries; counts[i]: the model's |{coarse >= t3}| of use[i]; mutant[j][i]: what mutant j of the bound
    would count there (6 only after an append onto a partial block)"""
    use: list
    counts: np.ndarray
    mutant: dict
    drawn: int
    Eq: np.ndarray
    coarse: np.ndarray

    @property
    def want(self):
        return int(self.counts.sum())

    @property
    def mutants(self):
        return {j: int(c.sum()) for j, c in self.mutant.items()}

    def take(self, m):
        """the first m qualifying queries only"""
        assert len(self.use) >= m, (len(self.use), m)
        return Prediction(self.use[:m], self.counts[:m], {j: c[:m] for j, c in self.mutant.items()}, self.drawn, self.Eq, self.coarse)

    def check_cap(self):
        """the cap of the GPU tests: more than 128 qualifying queries (or the int8 pass is not taken), at least half of those drawn"""
        assert len(self.use) >= 129 and 2 * len(self.use) >= self.drawn, (len(self.use), self.drawn)

    def line(self, name):
        m = " ".join(f"{j}:{c}" for j, c in self.mutants.items())
        return f"{name}: {len(self.use)} of {self.drawn} queries qualify, rescored {self.want}; mutants {m}"

    def differ(self, *which):
        """every named mutant (7 stands for 7- and 7+) counts differently from the model"""
        for w in which:
            keys = [j for j in self.mutant if str(j).startswith(str(w))]
            assert keys, (w, list(self.mutant))
            for j in keys:
                assert self.mutants[j] != self.want, (j, self.mutants[j], self.want)


def predict(oracle, st, y, qh, es, k=K, pilot=1, allow=None):
    """st: the copy's State at this search; y, qh: normalised rows and queries; es: the oracle's scores [nq, k] under `allow`.
    A query qualifies if X1 is the oracle's k-th score, at least |S1| rows reach t3 and fewer than REFINE_PMAX do."""
    n = len(y)
    rows = np.arange(n) if allow is None else np.flatnonzero(allow)
    t, q8, e, nn = quant_queries(qh)
    coarse = coarse_scores(st.c8, st.s, t, q8, n)
    Eq = e_q(e, nn, st.eps_max)
    E_alt = {3: e_q(e, np.zeros_like(nn), st.eps_max), 4: e_q(e, nn, st.eps_full), 5: e_q(e, nn, st.eps_before)}
    s_alt = {"7-": np.concatenate([st.s[:1], st.s[:-1]]), "7+": np.concatenate([st.s[1:], st.s[-1:]])}
    c_alt = {j: coarse_scores(st.c8, s, t, q8, n) for j, s in s_alt.items()}
    E6 = None
    if st.stale is not None:
        c_alt[6] = coarse_scores(st.stale[1], st.stale[0], t, q8, n)
        E6 = e_q(e, nn, st.stale[2])
    nq = len(qh)
    use, counts = [], []
    mut = {j: [] for j in MUTANTS if j != 6 or st.stale is not None}
    for i in range(nq):
        if len(rows) < pilot * k:
            continue
        cs = coarse[i][rows]
        n1, X1, cnt = _rounds(oracle, cs, rows, y, qh[i], Eq[i], k, pilot)
        if not (X1 == es[i, k - 1] and n1 <= cnt < REFINE_PMAX):
            continue
        use.append(i)
        counts.append(cnt)
        mut[1].append(_count(cs, RM.sub_down(X1, F32(2) * Eq[i])))
        mut[2].append(_count(cs, RM.sub_down(X1, Eq[(i + 1) % nq])))
        for j, E in E_alt.items():
            mut[j].append(_count(cs, RM.sub_down(X1, E[i])))
        for j, c in c_alt.items():
            mut[j].append(_rounds(oracle, c[i][rows], rows, y, qh[i], (E6 if j == 6 else Eq)[i], k, pilot)[2])
    return Prediction(use, np.array(counts, np.int64), {j: np.array(c, np.int64) for j, c in mut.items()}, nq, Eq, coarse)


# ---- the corpora of the GPU cases ------------------------------------------------------------------------------------------------
def outlier_row(rng, d, size):
    """a row whose normalised form has one element of about `size`: its block's scale, hence its eps_b, grows with it"""
    v = rng.standard_normal(d).astype(F32)
    v *= np.sqrt(max(1 - size * size, 0.0)) / np.linalg.norm(v)
    v[int(rng.integers(d))] = size
    return v


def build(n, d, nq, seed, owners=None, pin=None):
    """(corpus [n, d], queries [nq, d], own: query -> first row of its block). synth rows without duplicates; each of the first
    `owners` queries (default: all) owns one 32-row block of adversarial rows aligned with it (make_blocks of
    test_i8_refine_model.py) at a 32-aligned row the seed chooses — or the row `pin` names for it."""
    rng = np.random.default_rng(seed)
    corpus = synth.make_corpus(n, d, duplicates=False)
    q = synth.make_queries(nq, d, corpus)
    qn = RM.normalize(q)
    pin = dict(pin or {})
    free = [int(r) for r in rng.permutation(n // 32) * 32 if r not in pin.values()]
    own = {i: pin.get(i, free[i]) for i in range(nq if owners is None else owners)}
    for i, r in own.items():
        corpus[r:r + 32] = RM.make_blocks("adversarial", qn[i], rng, 1, d)[0]
    return corpus, q, own


def free_block(own, n, rng):
    """the first row of a full 32-row block no query owns"""
    taken = set(own.values())
    return next(int(r) for r in rng.permutation(n // 32) * 32 if r not in taken)


def typical_max(corpus):
    return float(np.abs(RM.normalize(corpus)).max())


# ---- scenarios: what a GPU test replays on an index and what the model says of every search ------------------------------------------
@dataclass
class Search:
    name: str
    ops: list                            # [(method of HipIndex, args)] to apply before this search
    y: np.ndarray                        # the normalised rows the index holds at this search
    q: np.ndarray                        # the queries drawn (raw); the GPU test sends q[pred.use]
    allow: Optional[np.ndarray]
    pred: Prediction
    es: np.ndarray
    er: np.ndarray
    ec: np.ndarray
    differ: tuple
    extra_q: Optional[np.ndarray] = None   # queries sent behind the qualifying ones (the zero queries)


class Scenario:
    """a script of writes and searches on one index (created with coarse_i8 = 1, spec_tau = 0, refine_pilot = pilot and
    reserve(reserve)), with the model's prediction of every search"""

    def __init__(self, oracle, d, reserve, pilot=1, bf16=False, **options):
        self.oracle, self.d, self.reserve, self.pilot, self.bf16, self.options = oracle, d, reserve, pilot, bf16, options
        self.y = np.zeros((0, d), F32)
        self.copy = Copy8()
        self.ops, self.searches = [], []

    def _norm(self, rows):
        if self.bf16:
            import torch
            rows = torch.from_numpy(np.ascontiguousarray(rows, F32)).to(torch.bfloat16).to(torch.float32).numpy()
        return self.oracle.normalize_rows(rows)

    def add(self, rows):
        self.ops.append(("add_bf16" if self.bf16 else "add", (np.ascontiguousarray(rows, F32),)))
        self.copy.appended(len(self.y))
        self.y = np.concatenate([self.y, self._norm(rows)])

    def update(self, ids, rows):
        self.ops.append(("update", (np.asarray(ids), np.ascontiguousarray(rows, F32))))
        self.copy.rewritten()
        self.y = self.y.copy()
        self.y[np.asarray(ids)] = self._norm(rows)

    def compact(self, keep):
        self.ops.append(("compact", (np.asarray(keep),)))
        self.copy.rewritten()
        self.y = self.y[np.asarray(keep)].copy()

    def search(self, name, q, differ, allow=None, take=None, extra_q=None, cap=True):
        assert len(self.y) <= self.reserve
        st = self.copy.prepare(self.y)
        es, er, ec = self.oracle.cosine_topk(self.y, q, K, allow)
        pred = predict(self.oracle, st, self.y, self.oracle.normalize_rows(q), es, K, self.pilot, allow)
        if cap:
            pred.check_cap()
        if take is not None:
            pred = pred.take(take)
        self.searches.append(Search(name, self.ops, self.y, q, allow, pred, es, er, ec, tuple(differ), extra_q))
        self.ops = []
        return pred


# ---- the cases (issue table: shape, and the mutants that must count differently) -------------------------------------------------------
NQ = 240                                                # queries drawn per case (160 ... 300)
WIDTHS = (100, 128, 200, 256, 324, 512, 580, 1000, 1024)   # k_scan<I8> k-steps 1, 1, 2, 2, 3, 4, 5, 8, 8
RAGGED = (1, 31, 33, 255)


def case_width(oracle, d):
    """n = 256 * 36 + 77: several tiles per stream, a ragged last tile and a ragged last block"""
    n = 256 * 36 + 77
    corpus, q, own = build(n, d, NQ, seed=d)
    sc = Scenario(oracle, d, n)
    sc.own = own
    sc.add(corpus)
    sc.search(f"width {d}", q, (1, 2, 3, 7))
    return sc


def case_ragged(oracle, d, r):
    """n = 256 * 36 + r; the last block (r % 32 rows) holds the rows of query 0's adversarial block that fit before a row with one
    outlier element (1.5 to 3 times the corpus' largest): that block alone carries eps_max"""
    n = 256 * 36 + r
    nr = n % 32
    corpus, q, own = build(n + 32, d, NQ, seed=1000 * d + r, pin={0: n - nr})
    corpus = corpus[:n]
    eps = quant_blocks(oracle.normalize_rows(corpus[:n - nr]))[2].max()
    for f in (1.5, 2.0, 2.5, 3.0):                       # the mildest of these that puts the block's eps_b a quarter above every other
        corpus[n - 1] = outlier_row(np.random.default_rng(r), d, f * typical_max(corpus[:n - nr]))
        if quant_blocks(oracle.normalize_rows(corpus[n - nr:]))[2][0] >= 1.25 * eps:
            break
    sc = Scenario(oracle, d, n)
    sc.own = own
    sc.add(corpus)
    sc.search(f"ragged d {d} n % 256 = {r}", q, (4,))
    return sc


def case_qtile(oracle, nq):
    """d = 512, exactly nq qualifying queries sent: 129 and 256 (one 256-query tile, padded), 257 (two tiles, the second one query),
    1030 (five tiles; the first 300 queries drawn own a block: one block each would be more rows than the corpus has)"""
    d, n = 512, 256 * 40 + 77
    drawn = {129: 200, 256: 300, 257: 300, 1030: 1760}[nq]
    corpus, q, own = build(n, d, drawn, seed=nq, owners=min(drawn, 300))
    sc = Scenario(oracle, d, n)
    sc.own = own
    sc.add(corpus)
    sc.search(f"query tiles nq {nq}", q, (1, 2), take=nq)
    return sc


def case_where(oracle):
    """40 % of the rows allowed; query 0's own block entirely disallowed"""
    d, n = 512, 256 * 60 + 77
    corpus, q, own = build(n, d, NQ, seed=7)
    allow = np.random.default_rng(4).random(n) < 0.4
    allow[own[0]:own[0] + 32] = False
    sc = Scenario(oracle, d, n)
    sc.own = own
    sc.add(corpus)
    sc.search("where 40 %", q, (1,), allow=allow)
    return sc


def case_append(oracle):
    """search at n0 = 256 * 30 + 13, append to n = 256 * 36 + 77, search again: query 0's block lies across n0 (13 rows before
    it, 19 appended), so the re-quantised block changes scale and gains rows that matter"""
    d, n0, n = 512, 256 * 30 + 13, 256 * 36 + 77
    corpus, q, own = build(n, d, NQ, seed=11, pin={0: n0 // 32 * 32})
    sc = Scenario(oracle, d, n)
    sc.own = own
    sc.add(corpus[:n0])
    sc.search("append: before", q, (1,))
    sc.add(corpus[n0:])
    sc.search("append: after", q, (6,))
    return sc


def case_update(oracle):
    """(i) one row of a plain block becomes an outlier row: eps_max rises; (ii) it is updated back: the full rebuild's reset
    lowers eps_max again. Either time the eps_max of before the write would count differently."""
    d, n = 512, 256 * 36 + 77
    corpus, q, own = build(n, d, NQ, seed=13)
    rng = np.random.default_rng(13)
    r = free_block(own, n, rng) + 5
    sc = Scenario(oracle, d, n)
    sc.own = own
    sc.add(corpus)
    sc.search("update: fresh", q, (1,))
    sc.update([r], outlier_row(rng, d, 2.0 * typical_max(corpus))[None, :])
    sc.search("update: outlier in", q, (5,))
    sc.update([r], corpus[r][None, :])
    sc.search("update: outlier out", q, (5,))
    return sc


def case_compact(oracle):
    """a plain block holds an outlier row; every 7th row and that row are deleted by bitmap, then compacted away: the kept rows
    re-block (every scale changes) and the rebuild's eps_max is the smaller one"""
    d, n = 512, 256 * 40 + 77
    corpus, q, own = build(n, d, NQ, seed=17)
    rng = np.random.default_rng(17)
    r = free_block(own, n, rng) + 9
    corpus[r] = outlier_row(rng, d, 2.0 * typical_max(corpus))
    dead = np.zeros(n, bool)
    dead[np.arange(3, n, 7)] = True
    dead[r] = True
    sc = Scenario(oracle, d, n)
    sc.own = own
    sc.add(corpus)
    sc.search("compact: deleted by bitmap", q, (1,), allow=~dead)
    sc.compact(np.flatnonzero(~dead))
    sc.search("compact: compacted", q, (5, 7))
    return sc


def case_bf16(oracle, d):
    """the compact bf16 master: the model starts from the widened bf16 values as the C oracle normalises them"""
    n = 256 * 36 + 77
    corpus, q, own = build(n, d, NQ, seed=19 + d)
    sc = Scenario(oracle, d, n, bf16=True, compact_master=1)
    sc.own = own
    sc.add(corpus)
    sc.search(f"compact bf16 master d {d}", q, (1, 3))
    return sc


def case_zeros(oracle):
    """one all-zero 32-row block (s_b = 0, inv = 0), zero rows inside plain blocks, and two zero queries (t_q = 1, E_q = 1e-6)
    behind the qualifying ones in a second search"""
    d, n = 512, 256 * 36 + 77
    corpus, q, own = build(n, d, NQ, seed=23)
    rng = np.random.default_rng(23)
    r = free_block(own, n, rng)
    corpus[r:r + 32] = 0
    for _ in range(3):
        corpus[free_block(own, n, rng) + int(rng.integers(32))] = 0
    sc = Scenario(oracle, d, n)
    sc.own = own
    sc.add(corpus)
    sc.search("zeros: blocks and rows", q, ())
    sc.search("zeros: two zero queries", q, (), extra_q=np.zeros((2, d), F32))
    return sc


CASES = {f"width-{d}": (case_width, d) for d in WIDTHS}
CASES.update({f"ragged-{d}-{r}": (case_ragged, d, r) for d in (256, 1024) for r in RAGGED})
CASES.update({f"qtile-{nq}": (case_qtile, nq) for nq in (129, 256, 257, 1030)})
CASES.update({"where": (case_where,), "append": (case_append,), "update": (case_update,), "compact": (case_compact,),
              "bf16-1024": (case_bf16, 1024), "bf16-256": (case_bf16, 256), "zeros": (case_zeros,)})
