"""Numpy model of the int8 scan's classes of block error (DESIGN.md §5 "classes of eps_b"; k_rows.hpp k_eps_edges, k_eps_classify,
k_tau8; scan_kernel.hpp class_base), on top of tests/i8_model.py. Shared by tests/test_i8_class_model.py (CPU) and
tests/test_gpu_i8_classes.py (GPU).

  edges7 / classify     the EPS_CLASSES - 1 stored edges of a full quantisation — edge[c] the ceil((1 - 2^-(c+1)) nb)-th smallest eps_b,
                        an exact order statistic — and a block's class byte: the smallest c with eps_b <= edge[c], or 7
  ClassCopy             prepare_i8's state across writes: i8_model.Copy8 plus the eps_b table, the edges (taken at a full
                        quantisation only) and the class bytes (an append classifies what it quantised against the edges that stand)
  thresholds            k_tau8 with C classes: E_{q,c}, thr_c = fl_down((T - E_{q,c}) / t_q), tau_c, and
                        taus8 = max_c (tau_c + E_{q,c}) - E_q in fp64 rounded up; class C - 1 is the bound with the live eps_max,
                        statement for statement what k_tau8 computed before the classes
  emitted_mask          k_scan<I8>'s check: row r of block b is a hit iff (float)D * s_b >= thr[min(cls[b], C - 1)]

Every float32 rounding is the kernel's: the model's counts are meant to match the library's to the row."""
import numpy as np

import i8_model as M
from test_i8_bound_model import F32

EPS_CLASSES = 8


def edges7(eps):
    """the stored edges of a full quantisation over the eps_b table `eps` (nb >= 1 blocks)"""
    s = np.sort(np.asarray(eps, F32))
    nb = len(s)
    return np.array([s[nb - (nb >> (c + 1)) - 1] for c in range(EPS_CLASSES - 1)], F32)


def classify(eps, e7):
    """class bytes: the smallest c with eps_b <= edge[c], else EPS_CLASSES - 1"""
    eps = np.asarray(eps, F32)
    cls = np.full(len(eps), EPS_CLASSES - 1, np.int64)
    for c in range(EPS_CLASSES - 2, -1, -1):
        cls[eps <= e7[c]] = c
    return cls


class ClassCopy:
    """the int8 copy with its classes at one search after another (reserve the final row count first: see i8_model.Copy8)"""

    def __init__(self):
        self.copy = M.Copy8()
        self.eps = np.zeros(0, F32)
        self.cls = np.zeros(0, np.int64)
        self.e7 = None

    def appended(self, row0):
        self.copy.appended(row0)

    def rewritten(self):
        self.copy.rewritten()

    def prepare(self, y):
        need, full, b0 = self.copy.valid < len(y), self.copy.valid == 0, self.copy.valid // 32
        st = self.copy.prepare(y)
        if need:
            eps_new = M.quant_blocks(y[32 * b0:])[2]
            self.eps = np.concatenate([self.eps[:0 if full else b0], eps_new])
            if full:
                self.e7 = edges7(self.eps)
            self.cls = np.concatenate([self.cls[:0 if full else b0], classify(eps_new, self.e7)])
        assert len(self.eps) == len(st.s) == len(self.cls)
        return st


def _thr_down(T, Ef, t):
    """fl_down((T - Ef) / t): k_tau8's threshold in t_q units, rounded down (a lower threshold only emits more)"""
    want = T.astype(np.float64) - Ef.astype(np.float64)
    th = (want / t.astype(np.float64)).astype(F32)
    over = th.astype(np.float64) * t.astype(np.float64) > want
    return np.where(over, np.nextafter(th, F32(-np.inf)), th).astype(F32)


def _tau(th, t):
    return M.f32_up(th.astype(np.float64) * t.astype(np.float64) + 1e-6)


def class_edges(e7, eps_max, C):
    """the C edges a search with C classes charges: the first C - 1 stored ones, then the live eps_max"""
    return np.concatenate([np.asarray(e7, F32)[:C - 1], [F32(eps_max)]]).astype(F32)


def thresholds(T, t, e, nn, edges):
    """T [nq] float32 finite (the fp16 bootstrap's threshold, score units); t, e, nn: quant_queries' t_q, e_q, n_q; edges: class_edges.
    -> (thr [C, nq], tau [C, nq], E [C, nq], taus8 [nq]) all float32; E[C - 1] is E_q"""
    T, t = np.asarray(T, F32), np.asarray(t, F32)
    C = len(edges)
    E = np.stack([M.f32_up(e.astype(np.float64) * (1.0 + 1e-6) + nn.astype(np.float64) * np.float64(edges[c]) + 1e-6) for c in range(C)])
    thr = np.stack([_thr_down(T, E[c], t) for c in range(C)])
    tau = np.stack([_tau(thr[c], t) for c in range(C)])
    top = tau[C - 1].astype(np.float64) + E[C - 1].astype(np.float64)
    taus8 = tau[C - 1].copy()
    if C > 1:
        worst = (tau[:C - 1].astype(np.float64) + E[:C - 1].astype(np.float64)).max(axis=0)
        lower = worst > top
        taus8 = np.where(lower, M.f32_up(worst - E[C - 1].astype(np.float64)), taus8).astype(F32)
    return thr, tau, E, taus8


def acc_units(c8, s, q8, n):
    """[nq, n] float32: (float)D * s_b, what k_scan<I8> compares with thr (t_q units)"""
    D = c8[:n] @ q8.T
    assert np.abs(D).max() < 2 ** 24
    return np.ascontiguousarray((D * np.repeat(s, 32)[:n, None]).astype(F32).T)


def emitted_mask(acc, cls, thr, allow=None):
    """[nq, n] bool: the scan's hits with C = len(thr) classes; cls: the class byte of every 32-row block"""
    C = thr.shape[0]
    n = acc.shape[1]
    row_cls = np.minimum(np.repeat(np.asarray(cls), 32)[:n], C - 1)
    hit = acc >= thr[row_cls, :].T
    if allow is not None:
        hit &= np.asarray(allow, bool)[None, :]
    return hit


# ---- the corpora of the GPU cases (tests/test_gpu_i8_classes.py) -----------------------------------------------------------------------
# What makes `emitted` predictable to the row is a threshold T the model knows exactly. Every query is a 16-hot vector of +-0.25 (unit
# norm, exact in fp16 and in int8) and the corpus holds it as a row of its own, its ANCHOR: the search runs with k = 1 on a corpus small
# enough that the threshold sample is the whole corpus, so the sampled maximum is the anchor's fp16 coarse score, 16 exact products that
# sum to exactly 1, and T = fl32(1 - 2E) (search_plan.hpp: the proven threshold, slack 2E). X1, the best exact score, is 1 as well.
# Half the other blocks hold a SPIKE row (one large element: s_b and eps_b grow with it, graded over a factor 2, so every class is
# populated), half are flat. The first `owners` queries own PLANTED rows in spiky blocks, near copies whose score lies around
# T - E_q ... 1 - E_q: with one class a planted row is a hit when coarse + E_q reaches T, with 8 classes when coarse + E_{q,c} does, so
# some are dropped — that is `emitted` falling. k_refine re-scores the hits with coarse >= X1 - E_q whatever the classes (its band is not
# touched); `rescored` is the same under both settings exactly when no DROPPED row lies in that band, which at T = 1 - 2E, only 2E
# below X1, has to be arranged: design() redraws planted rows until none does, in every search of the case. (On a large corpus T lies
# far below X1 - E_q and no arrangement is needed.)
from dataclasses import dataclass, field
from typing import Optional

import coarse_model as CO
import test_i8_refine_model as RM

HOT = 16


def hot_queries(rng, nq, d):
    seen, out = set(), np.zeros((nq, d), F32)
    for i in range(nq):
        while True:
            cols = tuple(sorted(rng.choice(d, HOT, replace=False).tolist()))
            if cols not in seen:
                break
        seen.add(cols)
        out[i, list(cols)] = rng.choice([-0.25, 0.25], HOT)
    return out


def spike_row(rng, d, z):
    v = rng.standard_normal(d)
    j = int(rng.integers(d))
    v[j] = 0
    v *= np.sqrt(1 - z * z) / np.linalg.norm(v)
    v[j] = z
    return v.astype(F32)


def planted_row(rng, q, a):
    """a near copy of q with exact score a: q's 16 elements weighted a +- 0.05 each, a on average (so that they do not all round
    alike), unit norm with noise on the other columns"""
    on = q != 0
    w = 0.05 * (2 * rng.random(HOT) - 1)
    w += a - w.mean()
    v = np.zeros(len(q))
    v[on] = q[on] * w
    u = rng.standard_normal(len(q))
    u[on] = 0
    v += u * np.sqrt(max(1 - (v * v).sum(), 0.0)) / np.linalg.norm(u)
    return v.astype(F32)


@dataclass
class Step:
    """one search of a case: the writes before it, the rows the index then holds (raw, and `src`: the base corpus row each came from,
    -1 for none), the bitmap, and, once evaluated, the oracle's answer and the model's counts"""
    name: str
    ops: list
    raw: np.ndarray
    src: np.ndarray
    allow: Optional[np.ndarray] = None
    write: str = "add"                         # how the rows got there since the last search: add (append), rewrite (update, compact)
    row0: int = 0                              # add: the row count before the append
    want: dict = field(default_factory=dict)   # C -> (emitted, rescored)
    es: np.ndarray = None
    er: np.ndarray = None
    ec: np.ndarray = None
    cls_used: tuple = ()
    eps_max: float = 0.0


class Case:
    def __init__(self, oracle, d, n, nq, seed, owners=96, per=6, bf16=False, z_top=None, top_block=None, zero_blocks=0, **options):
        """n rows, the last block ragged when n % 32; z_top: one more spike, z_top times the largest of the graded ones, in block
        top_block (default: the last); zero_blocks: that many flat blocks of all-zero rows (s_b = 0, eps_b = 0)"""
        self.oracle, self.d, self.n, self.nq, self.bf16, self.options = oracle, d, n, nq, bf16, options
        self.rng = rng = np.random.default_rng(seed)
        self.q = hot_queries(rng, nq, d)
        self.two_e = CO.two_e(d)
        self.T = F32(F32(1.0) - self.two_e)
        base = rng.standard_normal((n, d)).astype(F32)
        base[:nq] = self.q                                                  # the anchors, in blocks of their own
        na, nb, nfull = (nq + 31) // 32, (n + 31) // 32, n // 32
        flat_max = float(np.abs(RM.normalize(base[32 * na:32 * na + 2048])).max())
        self.z_lo = min(0.47, max(0.3, 1.35 * flat_max))                    # (spikes up to 2.06 z_lo < 1)
        spiky = [b for b in range(na, nb) if (b - na) % 2 == 1]
        grade = rng.permutation(len(spiky)) / len(spiky)
        self.z = {b: self.z_lo * 2.0 ** g for b, g in zip(spiky, grade)}
        if z_top is not None:
            self.z[nb - 1 if top_block is None else top_block] = 2.0 * self.z_lo * z_top
        for b, z in self.z.items():
            base[32 * b] = spike_row(rng, d, z)
        for b in [b for b in range(na, nfull) if b not in self.z][1:1 + zero_blocks]:
            base[32 * b:32 * b + 32] = 0
        slots = [(b, r) for b in spiky if b < nfull for r in range(1, 32)]
        take = rng.permutation(len(slots))[:owners * per]
        self.planted = {}                                                   # base row -> owner
        for j, t in enumerate(take):
            b, r = slots[t]
            self.planted[32 * b + r] = j % owners
        self.base = base
        self.eq_guess = None

    def norm(self, rows):
        if self.bf16:
            rows = CO.to_bf16(rows)
        return self.oracle.normalize_rows(rows)

    def draw(self, rows, Eq):
        lo, hi = 1.0 - float(self.two_e) - Eq - 0.004, 1.0 - Eq + 0.002
        for r in rows:
            self.base[r] = planted_row(self.rng, self.q[self.planted[r]], lo + (hi - lo) * self.rng.random())

    def evaluate(self, steps, full):
        """the model over the case's searches. full: every query and the oracle (what the GPU test asserts); otherwise only the planted
        rows against their owners. Returns (forbidden base rows, dropped rows per step)."""
        cc, forbidden, dropped = ClassCopy(), set(), []
        qh = self.oracle.normalize_rows(self.q)
        t, q8, e, nn = M.quant_queries(qh)
        for s in steps:
            y = self.norm(s.raw)
            if s.write == "add":
                cc.appended(s.row0)
            else:
                cc.rewritten()
            st = cc.prepare(y)
            n = len(y)
            Tq = np.full(self.nq, self.T, F32)
            thr = {C: thresholds(Tq, t, e, nn, class_edges(cc.e7, st.eps_max, C)) for C in (1, 8)}
            Eq = thr[1][2][0]
            t3 = np.array([RM.sub_down(F32(1.0), x) for x in Eq], F32)
            s.eps_max, s.cls_used = float(st.eps_max), tuple(sorted(set(cc.cls[:(n + 31) // 32].tolist())))
            rows = np.flatnonzero(np.isin(s.src, list(self.planted)))
            own = np.array([self.planted[int(b)] for b in s.src[rows]])
            rs = np.repeat(st.s, 32)[rows]
            acc = ((st.c8[rows] * q8[own]).sum(axis=1) * rs).astype(F32)     # (float)D * s_b of a planted row against its owner
            coarse = (acc * t[own]).astype(F32)
            rc = np.minimum(cc.cls[rows // 32], 7)
            ok = np.ones(len(rows), bool) if s.allow is None else s.allow[rows]
            hit1, hit8 = (acc >= thr[1][0][0, own]) & ok, (acc >= thr[8][0][rc, own]) & ok
            assert not (hit8 & ~hit1).any()
            gone = hit1 & ~hit8
            forbidden |= set(int(b) for b in s.src[rows[gone & (coarse >= t3[own])]])
            dropped.append(int(gone.sum()))
            if not full:
                continue
            a_all = acc_units(st.c8, st.s, q8, n)
            c_all = (a_all * t[:, None]).astype(F32)
            for C in (1, 8):
                hit = emitted_mask(a_all, cc.cls, thr[C][0], s.allow)
                s.want[C] = (int(hit.sum()), int((hit & (c_all >= t3[:, None])).sum()))
            s.es, s.er, s.ec = self.oracle.cosine_topk(y, self.q, 1, s.allow)
            # the premises of T and X1: the anchor is every query's best row, exactly 1, and nothing else comes near in fp16
            assert (s.es[:, 0] == F32(1.0)).all() and (s.ec == 1).all()
            x = qh.astype(np.float64) @ y.astype(np.float64).T
            assert np.sort(x, axis=1)[:, -2].max() < 0.995
        self.eq_guess = float(np.median(Eq))
        return forbidden, dropped

    def design(self, script, least=4, rounds=40):
        """script(case) -> the case's steps from self.base. Draw the planted rows, then redraw those that would make `rescored` differ
        between the settings in some search, until none is left; every search must drop at least `least` rows."""
        self.evaluate(script(self), False)                                  # (planted slots still hold noise: E_q only)
        self.draw(list(self.planted), self.eq_guess)
        for _ in range(rounds):
            bad, dropped = self.evaluate(script(self), False)
            if not bad:
                break
            self.draw(sorted(bad), self.eq_guess)
        steps = script(self)
        bad, dropped = self.evaluate(steps, True)
        assert not bad and min(dropped) >= least, (sorted(bad)[:8], dropped)
        for s in steps:
            assert s.want[8][0] < s.want[1][0] and s.want[8][1] == s.want[1][1], (s.name, s.want)
        return steps


def script_plain(allow_frac=None, allow_seed=0):
    def script(c):
        allow = None
        if allow_frac is not None:
            allow = np.random.default_rng(allow_seed).random(c.n) < allow_frac
            allow[:c.nq] = True                                              # the anchors stay: T and X1 rest on them
            allow[32 * ((c.nq + 31) // 32) + 32:32 * ((c.nq + 31) // 32) + 64] = False   # one whole spiky block out
        return [Step("fresh", [("add", (c.base.copy(),))], c.base.copy(), np.arange(c.n), allow)]
    return script


def script_append(n0):
    """search at n0 rows (inside a block), append the rest, search again"""
    def script(c):
        src = np.arange(c.n)
        return [Step("before the append", [("add", (c.base[:n0].copy(),))], c.base[:n0].copy(), src[:n0]),
                Step("after the append", [("add", (c.base[n0:].copy(),))], c.base.copy(), src, row0=n0)]
    return script


def script_update(row, z_up):
    """one row of a flat block becomes the corpus' largest spike (eps_max rises), then is updated back (the rebuild lowers it)"""
    def script(c):
        src, up = np.arange(c.n), c.base.copy()
        spike = spike_row(np.random.default_rng(row), c.d, 2.0 * c.z_lo * z_up)
        up[row] = spike
        src_up = src.copy()
        src_up[row] = -1
        return [Step("fresh", [("add", (c.base.copy(),))], c.base.copy(), src),
                Step("spike in", [("update", (np.array([row]), spike[None, :].copy()))], up, src_up, write="rewrite"),
                Step("spike out", [("update", (np.array([row]), c.base[row][None, :].copy()))], c.base.copy(), src, write="rewrite")]
    return script


def script_compact(every):
    """delete every `every`-th row behind the anchors by bitmap, search, compact them away (the kept rows re-block), search"""
    def script(c):
        src = np.arange(c.n)
        dead = np.zeros(c.n, bool)
        dead[np.arange(c.nq + 3, c.n, every)] = True
        keep = np.flatnonzero(~dead)
        return [Step("deleted by bitmap", [("add", (c.base.copy(),))], c.base.copy(), src, ~dead),
                Step("compacted", [("compact", (keep,))], c.base[keep].copy(), src[keep], write="rewrite")]
    return script
