"""Chroma's "ip" and "l2" spaces on the cosine engine: the plan, the numpy model and the engine wrapper.

The contract (include/rdx.h "Inner-product and squared-L2 spaces"): rows are kept exactly as given; the distance is
`1 - sum q_j x_j` (ip) or `sum (q_j - x_j)^2` (l2, squared), computed in fp64 from the raw fp32 values in ONE order (`ordered_sum`)
and rounded to fp32 once; results are ordered by (fp32 distance, row id) and depend on the raw values only.

The reduction. The cosine engine stores rows verbatim (`add_stored`) and normalises only the query, and its bounds need |row| <= 1,
not = 1: it returns the exact top-k of <p^, y> for any stored y with |y| <= 1. A collection in a new space stores LIFTED rows
    ip:  y = 2^e x               query p = q                engine dim = dim
    l2:  y = 2^e (x, a, 0, 0, 0) query p = (q, 1, 0, 0, 0)  engine dim = dim + 4,   a = (float)(-|x|^2 / 2)
with one power of two per collection (max |y| in (1/2, 1]; scaling by it is exact and checked). Then <p, y> = 2^e g with the gain
g = q.x (ip) or q.x - |x|^2 / 2 (l2), and the distance falls strictly as g grows. A search fetches k' > k candidates from the engine,
computes their exact distances, and PROVES that no other row can belong to the answer: a row that was not returned scores at most
the lowest returned score e_last, so its gain is at most (e_last + G) |p| 2^-e and its fp32 distance at least `lower_bound32`; the
query is proven when that bound is strictly above the k-th distance among the candidates (or fewer than k' rows were allowed at
all). What is not proven takes one larger fetch, then a brute-force pass over all allowed rows: results never depend on the path.

This file holds the model in numpy — the path of engines without device pointers and the reference of the GPU tests, the way
where.py is for where_device.py — and `SpaceEngine`, which gives `Collection` the engine interface it already uses. On a librdx
engine the candidates are re-scored, ordered and proven on the GPU (csrc/space_kernel.hpp); both paths give the same bits and take
the same decisions.
"""
from __future__ import annotations

import math
from contextlib import closing as _closing
from typing import Optional

import numpy as np

from . import where as W

SPACES = ("ip", "l2")
KIND = {"ip": 0, "l2": 1}          # include/rdx.h RDX_SPACE_IP / RDX_SPACE_L2

# The guard G, in units of the engine's score (DESIGN.md §17 derives it from k_normalize's arithmetic):
#   2^-24  every element of p^ = (float)((double)p_j / den) is rounded to fp32 once: sum |p_j y_j| / |p| * 2^-24 <= |y| 2^-24
#   2^-24  the score itself is rounded to fp32 once, and is at most |p^| |y| <= 1 + 2^-23 in magnitude
#   2^-24  (l2) a = (float)(-|x|^2 / 2) is rounded: 2^e |a| <= 1 is one coordinate of y, and |p| >= 1
#   the rest (den's fp64 roundings: |p|'s uncertainty; the fp64 sums; sub-normal p^ elements; this file's own fp64 steps): < 2^-40
GUARD_IP = 2.0 ** -23 + 2.0 ** -40
GUARD_L2 = 3.0 * 2.0 ** -24 + 2.0 ** -39
GUARD = {"ip": GUARD_IP, "l2": GUARD_L2}
PN2_MIN, PN2_MAX = 1.0e-18, 1.0e30   # |p|^2 the derivation covers (k_normalize clamps den below 1e-12); others: brute force
MAX_FETCH = 4096                     # the engine's largest k = rdx_space_rescore's limit
FIRST_FETCH_MAX = 256                # above 256 the engine takes its exact scan: the first fetch stays at or below it while k allows
PAGE_ROWS = 16384                    # rows paged out of the engine at a time (brute force, rescale)
_FLT_MAX = float(np.finfo(np.float32).max)
_LANE = np.arange(64)
_UP30, _DN30, _T40 = 1.0 + 2.0 ** -30, 1.0 - 2.0 ** -30, 2.0 ** -40


# ---- the model --------------------------------------------------------------------------------------------------------------
def ordered_sum(terms) -> np.ndarray:
    """sum over the last axis in the contract's order: 64 partial sums (partial l takes j = l, l + 64, ... from +0.0), then the
    xor butterfly s[l] += s[l ^ m] for m = 32, 16, 8, 4, 2, 1"""
    t = np.asarray(terms, dtype=np.float64)
    acc = np.zeros(t.shape[:-1] + (64,), dtype=np.float64)
    for j0 in range(0, t.shape[-1], 64):
        blk = t[..., j0: j0 + 64]
        acc[..., : blk.shape[-1]] += blk
    for m in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[..., _LANE ^ m]
    return acc[..., 0]


def sq_norms(x) -> np.ndarray:
    x64 = np.asarray(x, dtype=np.float32).astype(np.float64)
    return ordered_sum(x64 * x64)


def distances(space: str, q, x) -> np.ndarray:
    """fp32 distances of the contract between q [dim] (or [n][dim], row by row) and the rows x [n][dim]"""
    q64 = np.asarray(q, dtype=np.float32).astype(np.float64)
    x64 = np.asarray(x, dtype=np.float32).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        if space == "ip":
            return (1.0 - ordered_sum(q64 * x64)).astype(np.float32)   # (the product of two floats is exact in fp64)
        diff = q64 - x64
        return ordered_sum(diff * diff).astype(np.float32)


def lifted_dim(space: str, dim: int) -> int:
    return dim + 4 if space == "l2" else dim


def measure(space: str, x):
    """-> (lifted_sq fp64 [n]: the lifted rows' squared norms before scaling, bad bool [n]: the row cannot be lifted)"""
    n2 = sq_norms(x)
    with np.errstate(over="ignore", invalid="ignore"):
        if space == "ip":
            return n2, ~(n2 < 1.0e300)
        a = (n2 * -0.5).astype(np.float32)
        a64 = a.astype(np.float64)
        sq = n2 + a64 * a64
        return sq, ~(sq < 1.0e300) | ~(np.abs(a) <= np.float32(_FLT_MAX))


def scale_exp_for(lifted_sq_max: float) -> int:
    """the largest e with 4^e * lifted_sq_max <= 1: max |y| lands in (1/2, 1]"""
    if not lifted_sq_max > 0.0:
        return 0
    m, x = math.frexp(lifted_sq_max)          # = m 2^x, m in [1/2, 1)
    return (1 - x) // 2 if m == 0.5 else (-x) // 2


def lift_rows(space: str, x, scale_exp: int):
    """-> (engine rows fp32 [n][engine dim], bad bool [n]: some element does not scale back to its own bits)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    e = np.int32(scale_exp)
    src = x
    if space == "l2":
        with np.errstate(over="ignore"):
            a = (sq_norms(x) * -0.5).astype(np.float32)
        src = np.concatenate([x, a[:, None]], axis=1)
    with np.errstate(over="ignore", under="ignore"):
        y = np.ldexp(src, e)
        back = np.ldexp(y, -e)
    bad = (back.view(np.uint32) != np.ascontiguousarray(src).view(np.uint32)).any(axis=1)
    if space == "l2":
        y = np.concatenate([y, np.zeros((x.shape[0], 3), dtype=np.float32)], axis=1)
    return np.ascontiguousarray(y, dtype=np.float32), bad


def lift_queries(space: str, q) -> np.ndarray:
    q = np.ascontiguousarray(q, dtype=np.float32)
    if space == "ip":
        return q
    tail = np.zeros((q.shape[0], 4), dtype=np.float32)
    tail[:, 0] = 1.0
    return np.ascontiguousarray(np.concatenate([q, tail], axis=1))


def unlift_rows(space: str, y, scale_exp: int) -> np.ndarray:
    y = np.asarray(y, dtype=np.float32)
    if space == "l2":
        y = y[:, :-4]
    return np.ascontiguousarray(np.ldexp(y, np.int32(-scale_exp)), dtype=np.float32)


def lower_bound32(space: str, e_last, n2q, scale_exp: int) -> np.ndarray:
    """fp32 lower bound on the distance of every row the engine did not return (its score is at most e_last); NaN = the query's
    norm is outside the range the guard covers. csrc/space_kernel.hpp space_lower_bound32 is the same arithmetic."""
    n2q = np.asarray(n2q, dtype=np.float64)
    e = int(scale_exp)
    with np.errstate(all="ignore"):
        pn2 = n2q + 1.0 if space == "l2" else n2q
        ok = (pn2 >= PN2_MIN) & (pn2 <= PN2_MAX)
        P = np.sqrt(pn2)
        U = np.asarray(e_last, dtype=np.float32).astype(np.float64) + GUARD[space]
        Pb = np.where(U >= 0.0, P * _UP30, P * _DN30)
        B = np.ldexp(U * Pb, -e)
        if space == "l2":
            Bup = B + np.abs(B) * _T40
            lb = n2q * (1.0 - _T40) - 2.0 * Bup
        else:
            Bup = B + np.ldexp(P * _UP30 * _T40, -e)
            Bup = Bup + np.abs(Bup) * _T40
            lb = 1.0 - Bup
        lb = lb - np.abs(lb) * _T40
        out = lb.astype(np.float32)
    return np.where(ok, out, np.float32(np.nan)).astype(np.float32)


def direct_queries(space: str, q) -> np.ndarray:
    """bool [nq]: queries that go straight to brute force (zero queries, norms outside the guard's range)"""
    pn2 = sq_norms(q) + (1.0 if space == "l2" else 0.0)
    return ~((pn2 >= PN2_MIN) & (pn2 <= PN2_MAX))


def brute_force(space: str, q, x, k: int, allow: Optional[np.ndarray] = None):
    """the contract restated over raw rows x [n][dim]: (dist f32 [nq][k], rows i64 [nq][k], counts i32 [nq])"""
    q = np.ascontiguousarray(q, dtype=np.float32)
    x = np.ascontiguousarray(x, dtype=np.float32)
    nq = q.shape[0]
    rows = np.arange(x.shape[0]) if allow is None else np.flatnonzero(np.asarray(allow, dtype=bool))
    od = np.full((nq, k), np.inf, dtype=np.float32)
    orow = np.full((nq, k), -1, dtype=np.int64)
    oc = np.zeros(nq, dtype=np.int32)
    for b in range(nq):
        d = distances(space, q[b], x[rows]) if rows.size else np.zeros(0, np.float32)
        order = np.argsort(d, kind="stable")[:k]          # rows ascend: a stable sort ties by ascending row id
        od[b, : order.size], orow[b, : order.size], oc[b] = d[order], rows[order], order.size
    return od, orow, oc


def unpack_bits(bits, n: int) -> np.ndarray:
    return np.unpackbits(np.ascontiguousarray(bits, dtype=np.uint32).view(np.uint8), bitorder="little")[:n].astype(bool)


# ---- the engine wrapper -----------------------------------------------------------------------------------------------------
class SpaceMask:
    """a row bitmap for SpaceEngine.search(mask=): the words (numpy uint32, or a torch int32 tensor on the engine's device) and,
    made on demand, the inner engine's resident mask — made again after a rescale has replaced the inner engine"""

    def __init__(self, engine: "SpaceEngine", bits):
        self._engine, self.bits = engine, bits
        self._inner, self._gen, self._dev_bits, self._host = None, -1, None, None

    def inner(self):
        eng = self._engine
        if self._inner is None or self._gen != eng._generation:
            self.close()
            self._inner, self._gen = eng.inner.make_mask(self.bits), eng._generation
        return self._inner

    def host_bool(self, n: int) -> np.ndarray:
        if self._host is None:
            b = self.bits
            self._host = unpack_bits(b.cpu().numpy().view(np.uint32) if hasattr(b, "cpu") else b, n)
        return self._host

    def device_bits(self, dev):
        if self._dev_bits is None:
            import torch
            b = self.bits
            self._dev_bits = b if hasattr(b, "cpu") else torch.from_numpy(np.ascontiguousarray(b, dtype=np.uint32).view(np.int32)).to(dev)
        return self._dev_bits

    def close(self):
        if self._inner is not None and hasattr(self._inner, "close"):
            self._inner.close()
        self._inner = None


class SpaceEngine:
    """`inner` (a cosine engine of the LIFTED dimension: HipIndex, or any engine with add_stored / update_stored / get / search)
    behind the engine interface Collection uses, in the space "ip" or "l2". search() returns DISTANCES (ascending), not scores.
    last_stats: the last search's candidates fetched, queries proven by the first / the second fetch and answered by brute force,
    and the rescales since the engine was made. pad: None, or the number of extra candidates of the first fetch (tests)."""

    returns_distances = True

    def __init__(self, space: str, inner, scale_exp: Optional[int] = None, factory=None):
        if space not in SPACES:
            raise ValueError(f"SpaceEngine serves the spaces {SPACES}, got {space!r}")
        if hasattr(inner, "devices"):
            raise ValueError(f"the {space!r} space runs on one device in this version (no devices= / RDX_DEVICES)")
        self.space, self.kind, self.inner = space, KIND[space], inner
        self.dim = int(inner.dim) - (4 if space == "l2" else 0)
        if self.dim < 4 or self.dim % 4:
            raise ValueError(f"the {space!r} space needs a dimension that is a positive multiple of 4, at most {4096 - (4 if space == 'l2' else 0)}")
        self._factory = factory or (lambda: type(inner)(int(inner.dim), getattr(inner, "device", 0)))
        self._hint = None if scale_exp is None else int(scale_exp)
        self.scale_exp: Optional[int] = None      # set by the first write
        self._generation = 0
        self._options = {}
        self.rescales = 0
        self.pad: Optional[int] = None
        self.last_stats = {"fetched": 0, "proven_first": 0, "proven_second": 0, "brute": 0, "rescales": 0}
        self._on_device = hasattr(inner, "search_device") and hasattr(inner, "get_device")

    device = property(lambda self: getattr(self.inner, "device", 0))
    has_device_docs = property(lambda self: getattr(self.inner, "has_device_docs", False))
    has_device_meta = property(lambda self: getattr(self.inner, "has_device_meta", False))

    def __len__(self) -> int:
        return len(self.inner)

    def close(self):
        if hasattr(self.inner, "close"):
            self.inner.close()

    def set_option(self, name: str, value: int):
        if name == "compact_master":
            raise ValueError(f"compact_master is not available in the {self.space!r} space in this version")
        self.inner.set_option(name, value)
        self._options[name] = value

    def add_bf16(self, rows):
        raise ValueError(f"bf16 ingest is not available in the {self.space!r} space in this version")

    # ---- writes -------------------------------------------------------------------------------------------------------------
    def _lift_batch(self, x, first_label: int = 0):
        """validate a batch and lift it, rescaling the stored rows first when it does not fit the scale in use. Nothing is changed
        unless the whole batch can be stored. -> engine rows (numpy, or a torch tensor when x is one on the device)"""
        on_dev = hasattr(x, "is_cuda") and x.is_cuda
        if on_dev:
            from . import engine as E
            if x.dim() != 2 or x.shape[1] != self.dim:
                raise ValueError(f"expected [n][{self.dim}] embeddings, got shape {tuple(x.shape)}")
            import torch
            x = x.contiguous()
            if not bool(torch.isfinite(x).all()):
                raise ValueError("embeddings contain NaN or Inf")
            sq_t, bad_t = E.space_measure(self.kind, x)
            sq, bad = sq_t.cpu().numpy(), bad_t.cpu().numpy().astype(bool)
        else:
            x = np.ascontiguousarray(x, dtype=np.float32)
            if x.ndim != 2 or x.shape[1] != self.dim:
                raise ValueError(f"expected [n][{self.dim}] embeddings, got shape {x.shape}")
            if not np.isfinite(x).all():
                raise ValueError("embeddings contain NaN or Inf")
            sq, bad = measure(self.space, x)
        if bad.any():
            raise ValueError(f"row {first_label + int(np.flatnonzero(bad)[0])} of the batch cannot be stored in the {self.space!r} space: "
                             "its lifted form is not finite in fp32")
        need = scale_exp_for(float(sq.max()) if sq.size else 0.0)
        cur = self.scale_exp if self.scale_exp is not None else (need if self._hint is None else min(need, self._hint))
        e = min(cur, need)
        if on_dev:
            y, lost_t = E.space_lift(self.kind, x, e)
            lost = lost_t.cpu().numpy().astype(bool)
        else:
            y, lost = lift_rows(self.space, x, e)
        if lost.any():
            raise ValueError(f"row {first_label + int(np.flatnonzero(lost)[0])} of the batch cannot be stored in the {self.space!r} space: "
                             f"scaling it by 2^{e} is not exactly invertible in fp32")
        if self.scale_exp is not None and e < self.scale_exp and len(self.inner):
            self._rescale(e)
        self.scale_exp = e
        return y

    def _rescale(self, e_new: int):
        """a smaller scale: page the stored rows out, scale them exactly and add_stored them into a fresh engine"""
        n, shift = len(self.inner), np.int32(e_new - self.scale_exp)
        fresh = self._factory()
        try:
            for name, value in self._options.items():
                fresh.set_option(name, value)
            for a in range(0, n, PAGE_ROWS):
                y = self.inner.get(np.arange(a, min(n, a + PAGE_ROWS), dtype=np.int64))
                with np.errstate(under="ignore"):
                    z = np.ldexp(y, shift)
                    lost = (np.ldexp(z, -shift).view(np.uint32) != y.view(np.uint32)).any(axis=1)
                if lost.any():
                    raise ValueError(f"stored row {a + int(np.flatnonzero(lost)[0])} cannot be rescaled by 2^{int(shift)} exactly: the batch "
                                     f"is too large in norm for this {self.space!r} collection")
                fresh.add_stored(np.ascontiguousarray(z, dtype=np.float32))
        except BaseException:
            if hasattr(fresh, "close"):
                fresh.close()
            raise
        old, self.inner = self.inner, fresh
        if hasattr(old, "close"):
            old.close()
        self._generation += 1
        self.rescales += 1

    def add(self, rows):
        y = self._lift_batch(rows)       # (may replace self.inner: a rescale)
        self.inner.add_stored(y)

    add_stored = add      # a reload re-lifts the raw rows: the lift is a function of the raw values and the scale alone

    def update(self, row_ids, rows):
        ids = np.ascontiguousarray(row_ids, dtype=np.int64)
        if ids.size and (ids.min() < 0 or ids.max() >= len(self.inner)):
            raise ValueError(f"row id out of range [0, {len(self.inner)})")
        uniq, times = np.unique(ids, return_counts=True)
        if (times > 1).any():       # the engine's refusal (include/rdx.h), ahead of a lift that may rescale the stored rows
            raise ValueError(f"row id {int(uniq[times > 1][0])} is given more than once")
        y = self._lift_batch(np.ascontiguousarray(rows, dtype=np.float32))
        if y.shape[0] != ids.shape[0]:
            raise ValueError("update: rows must be [len(row_ids)][dim]")
        self.inner.update_stored(ids, y)

    def get(self, row_ids) -> np.ndarray:
        return unlift_rows(self.space, self.inner.get(row_ids), self.scale_exp or 0)

    def compact(self, keep_rows):
        self.inner.compact(keep_rows)
        self._generation += 1       # masks describe the rows before the compaction

    def make_mask(self, allow_bits) -> SpaceMask:
        return SpaceMask(self, allow_bits)

    # ---- search -------------------------------------------------------------------------------------------------------------
    def _fetch_sizes(self, k: int, n: int):
        """(k used, first fetch, second fetch); a fetch of 0 is skipped"""
        ke = min(k, n)
        cap = min(n, MAX_FETCH)
        if ke >= cap:
            return ke, (cap if cap == n else 0), 0      # everything fits one fetch, or k is beyond the engine's largest k
        if self.pad is not None:
            k1 = ke + max(1, int(self.pad))
        else:
            k1 = ke + max(16, ke)
            if ke < FIRST_FETCH_MAX:
                k1 = min(k1, FIRST_FETCH_MAX)
        k1 = min(k1, cap)
        k2 = min(max(4 * k1, 1024), cap)
        return ke, k1, (k2 if k2 > k1 else 0)

    def _ladder(self, nq: int, k: int, direct: np.ndarray, fetch, brute):
        """fetch(query indices, k', k used) -> proven bool; brute(query indices, k used). Both write their queries' results."""
        n = len(self.inner)
        ke, k1, k2 = self._fetch_sizes(k, n)
        st = {"fetched": 0, "proven_first": 0, "proven_second": 0, "brute": 0, "rescales": self.rescales}
        todo = np.flatnonzero(~direct)
        rest = np.flatnonzero(direct)
        for kp, key in ((k1, "proven_first"), (k2, "proven_second")):
            if kp == 0 or todo.size == 0:
                continue
            proven = np.asarray(fetch(todo, kp, ke), dtype=bool)
            if kp >= n:
                proven[:] = True            # every row was a candidate
            st["fetched"] += int(todo.size) * kp
            st[key] += int(proven.sum())
            todo = todo[~proven]
        rest = np.sort(np.concatenate([rest, todo]))
        if rest.size:
            brute(rest, ke)
            st["brute"] = int(rest.size)
        self.last_stats = st

    def _check_queries(self, q) -> np.ndarray:
        q = np.ascontiguousarray(q, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"expected [nq][{self.dim}] query embeddings, got shape {q.shape}")
        if not np.isfinite(q).all():
            raise ValueError("embeddings contain NaN or Inf")
        return q

    def search(self, queries, k: int, allow_bits=None, mask: Optional[SpaceMask] = None):
        """host in / host out: (distance f32 [nq][k] ascending, row i64 [nq][k], count i32 [nq]); padding (+inf, -1)"""
        q = self._check_queries(queries)
        if mask is not None and allow_bits is not None:
            raise ValueError("pass allow_bits or mask, not both")
        nq, n, k = q.shape[0], len(self.inner), int(k)
        od = np.full((nq, k), np.inf, dtype=np.float32)
        orow = np.full((nq, k), -1, dtype=np.int64)
        oc = np.zeros(nq, dtype=np.int32)
        if n == 0 or k == 0:
            return od, orow, oc
        if mask is None and allow_bits is not None:
            with _closing(SpaceMask(self, np.ascontiguousarray(allow_bits, dtype=np.uint32))) as tmp:
                return self.search(q, k, mask=tmp)
        direct = direct_queries(self.space, q)
        if self._on_device:
            import torch
            dev = torch.device("cuda", self.device)
            td, tr, tc = self._search_torch(torch.from_numpy(q).to(dev), k, mask, direct)
            return td.cpu().numpy(), tr.cpu().numpy(), tc.cpu().numpy()
        allow = mask.host_bool(n) if mask is not None else None
        inner_args = {}
        if mask is not None:
            inner_args = {"mask": mask.inner()} if hasattr(self.inner, "make_mask") else {"allow_bits": W.pack_bits(allow)}
        e, n2q = self.scale_exp or 0, sq_norms(q)

        def fetch(idx, kp, ke):
            sc, ro, cn = self.inner.search(lift_queries(self.space, q[idx]), kp, **inner_args)
            x = unlift_rows(self.space, self.inner.get(np.maximum(ro, 0).reshape(-1)), e).reshape(idx.size, kp, self.dim)
            lb = lower_bound32(self.space, sc[:, kp - 1], n2q[idx], e)
            proven = np.zeros(idx.size, dtype=bool)
            for j, b in enumerate(idx):
                c = int(cn[j])
                d = distances(self.space, q[b], x[j, :c])
                order = np.lexsort((ro[j, :c], d))[:ke]
                m = order.size
                od[b, :m], orow[b, :m], oc[b] = d[order], ro[j, :c][order], m
                od[b, m:], orow[b, m:] = np.inf, -1
                proven[j] = c < kp or bool(lb[j] > d[order[ke - 1]])
            return proven

        def brute(idx, ke):
            rows = np.arange(n) if allow is None else np.flatnonzero(allow)
            d = np.empty((idx.size, rows.size), dtype=np.float32)
            for a in range(0, rows.size, PAGE_ROWS):
                x = unlift_rows(self.space, self.inner.get(rows[a: a + PAGE_ROWS]), e)
                for j, b in enumerate(idx):
                    d[j, a: a + x.shape[0]] = distances(self.space, q[b], x)
            for j, b in enumerate(idx):
                order = np.argsort(d[j], kind="stable")[:ke]
                m = order.size
                od[b, :m], orow[b, :m], oc[b] = d[j, order], rows[order], m
                od[b, m:], orow[b, m:] = np.inf, -1

        self._ladder(nq, k, direct, fetch, brute)
        return od, orow, oc

    def search_device(self, queries, k: int, out_dist, out_row, out_count, allow_bits=None, mask: Optional[SpaceMask] = None):
        """torch CUDA tensors in / out: the same floats and the same decisions as search(). The embeddings and the results stay on
        the device; what crosses PCIe per fetch is small: the queries' out-of-range flags and the proof flags (one device-to-host
        copy each, which waits for the stream), and inside the gather (rdx_index_get with device pointers) a device synchronise
        and a copy of the nq * k' candidate row ids to the host, where the library range-checks them."""
        if not self._on_device:
            raise NotImplementedError("this collection's engine has no device-pointer search")
        import torch
        if mask is not None and allow_bits is not None:
            raise ValueError("pass allow_bits or mask, not both")
        if queries.dim() != 2 or queries.shape[1] != self.dim or queries.dtype != torch.float32:
            raise ValueError(f"expected a [nq][{self.dim}] fp32 tensor of query embeddings")
        q = queries.contiguous()
        if mask is None and allow_bits is not None:
            with _closing(SpaceMask(self, allow_bits)) as tmp:
                return self.search_device(q, k, out_dist, out_row, out_count, mask=tmp)
        from . import engine as E
        with torch.cuda.device(q.device):   # |q|^2 in the contract's order: the bits search() decides on (sq_norms)
            n2q_t, bad_t = E.space_measure(KIND["ip"], q)
        n2q = n2q_t.cpu().numpy()
        if bad_t.cpu().numpy().any():
            raise ValueError("embeddings contain NaN or Inf")
        pn2 = n2q + (1.0 if self.space == "l2" else 0.0)
        direct = ~((pn2 >= PN2_MIN) & (pn2 <= PN2_MAX))
        td, tr, tc = self._search_torch(q, int(k), mask, direct)
        out_dist.copy_(td)
        out_row.copy_(tr)
        out_count.copy_(tc)

    def _search_torch(self, q, k: int, mask: Optional[SpaceMask], direct: np.ndarray):
        import torch
        from . import engine as E
        dev, n, nq, e = q.device, len(self.inner), q.shape[0], self.scale_exp or 0
        od = torch.full((nq, k), float("inf"), dtype=torch.float32, device=dev)
        orow = torch.full((nq, k), -1, dtype=torch.int64, device=dev)
        oc = torch.zeros(nq, dtype=torch.int32, device=dev)
        bits = mask.device_bits(dev) if mask is not None else None
        inner_mask = mask.inner() if mask is not None else None
        dim_e = int(self.inner.dim)

        def fetch(idx, kp, ke):
            it = torch.from_numpy(idx).to(dev)
            qs = q if idx.size == nq else q.index_select(0, it).contiguous()
            p = qs if self.space == "ip" else E.space_lift(self.kind, qs, 0, is_query=True)[0]
            m = qs.shape[0]
            sc = torch.empty((m, kp), dtype=torch.float32, device=dev)
            ro = torch.empty((m, kp), dtype=torch.int64, device=dev)
            cn = torch.empty(m, dtype=torch.int32, device=dev)
            self.inner.search_device(p, kp, sc, ro, cn, mask=inner_mask)
            vec = torch.empty((m * kp, dim_e), dtype=torch.float32, device=dev)
            self.inner.get_device(ro.clamp(min=0).reshape(-1).contiguous(), vec)
            d, r, c, pv = E.space_rescore(self.kind, qs, vec, ro, sc, cn, ke, e, GUARD[self.space])
            od[it, :ke], orow[it, :ke], oc[it] = d, r, c
            return pv.cpu().numpy().astype(bool)

        def brute(idx, ke):
            # only allowed rows are ranked, as in the model: a disallowed row's +inf must never tie with an allowed row whose own
            # distance overflows fp32
            rows_t = None
            if bits is not None:
                lanes = torch.arange(32, dtype=torch.int32, device=dev)
                rows_t = ((bits.view(torch.int32)[:, None] >> lanes) & 1).reshape(-1)[:n].nonzero().reshape(-1)
            m = min(ke, n if rows_t is None else int(rows_t.numel()))
            for a in range(0, idx.size, 64):
                it = torch.from_numpy(idx[a: a + 64]).to(dev)
                qs = q.index_select(0, it).contiguous()
                dist = torch.empty((qs.shape[0], n), dtype=torch.float32, device=dev)
                for r0 in range(0, n, PAGE_ROWS):
                    ids = torch.arange(r0, min(n, r0 + PAGE_ROWS), dtype=torch.int64, device=dev)
                    vec = torch.empty((ids.numel(), dim_e), dtype=torch.float32, device=dev)
                    self.inner.get_device(ids, vec)
                    E.space_distances(self.kind, qs, vec, e, bits, r0, dist, r0)
                if rows_t is not None:
                    dist = dist.index_select(1, rows_t)
                sd, si = torch.sort(dist, dim=1, stable=True)      # a stable sort ties by ascending row id
                od[it, :m], orow[it, :m] = sd[:, :m], (si[:, :m] if rows_t is None else rows_t[si[:, :m]])
                od[it, m:], orow[it, m:], oc[it] = float("inf"), -1, m

        with torch.cuda.device(dev):
            self._ladder(nq, k, direct, fetch, brute)
        return od, orow, oc
