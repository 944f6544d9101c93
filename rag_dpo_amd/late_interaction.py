"""Late-interaction rerank (ColBERT-style MaxSim) over BGE-M3's per-token vectors — DESIGN.md §29.

The definition, stated once (`maxsim_model` below is it, in numpy):

  Token vectors of a text (`EmbeddingProvider.embed_tokens`): the encoder's last hidden states of every token except the first
  (`<s>`; `</s>` is included) through the ColBERT head `W [dim][hidden]`, `b [dim]`; each row divided by max(|row|, 1e-12) in fp32;
  rounded once to fp16. A text always has at least one (`</s>`).

  Score of a pair, over the fp16 vectors as stored: s_ij = q_i . d_j, m_i = max_j s_ij, score = the fp64 sum of the m_i in token
  order, divided by n_q, rounded once to fp32. The model computes s_ij in fp64; the kernel (`rdx_maxsim_f16`, include/rdx.h) computes
  s_ij with fp32 MFMA accumulation in a fixed k order and everything behind the max exactly as the model does. Nothing else differs.

  Rerank: final = score (+ boost when boost > 0), stable descending order, min_score, top_k and the keep-3 rule: exactly
  `rdx_rerank_select` / `select_host` (rag_dpo_amd/reranker.py), reused unchanged.

`MultiVectorStore` keeps the chunks' token vectors (computed once, at ingest) in one arena with a slot table, on the GPU as torch
tensors; `LateInteractionReranker` has `CrossEncoderReranker`'s interface and costs a question the forward it already pays for its
dense embedding plus one kernel call.

The int8 store (`quantize_model` and `maxsim_i8_model` below are its definition, in numpy):

  Quantising one token vector x (fp16 [dim]): a = max_k |x_k| (exact in fp16); scale = (float)((double)a / 127.0);
  c_k = clamp(rint((double)x_k / (double)scale), -127, 127), rint rounding ties to even. A row of zeros, or one holding NaN or Inf,
  has all codes 0 and scale +0.0.

  Score of a pair over (cq, sq), (cd, sd): acc_ij = sum_k cq_ik cd_jk in int32 (exact; |acc| <= 127^2 * 1024 < 2^24, so (float)acc
  is exact); v_ij = (float)acc_ij * sd_j, one fp32 multiply; m_i = max_j v_ij; score = the fp64 sum of (double)sq_i * (double)m_i in
  token order from +0.0, divided by n_q, rounded once to fp32. sq_i >= 0 is constant in j, so it is applied after the maximum. No -0.0
  can arise in v: sd_j = 0 only for an all-zero row, whose acc is 0, and otherwise sd_j >= 2^-24 / 127 > 0 with acc_ij an integer, so
  the maximum is order-free. The kernels (`rdx_maxsim_quantize_i8`, `rdx_maxsim_i8`) give these bits exactly; `quant_bound` bounds
  the distance to the fp64 MaxSim of the fp16 vectors."""
from __future__ import annotations

import json
import logging
import os
from typing import List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from .reranker import MAX_GPU_CANDIDATES, CrossEncoderReranker, RankedChunk, _ranked

logger = logging.getLogger(__name__)

# include/rdx.h RDX_MAXSIM_MAX_*: a question's and a slot's token vectors
MAX_Q_TOKENS, MAX_SLOT_TOKENS, MAX_DIM = 256, 8192, 1024


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def maxsim_model(q, d) -> np.float32:
    """score of one pair: q fp16 [n_q][dim], d fp16 [n_d][dim] (n_q, n_d >= 1) -> fp32"""
    q64 = np.asarray(q, dtype=np.float16).astype(np.float64)
    d64 = np.asarray(d, dtype=np.float16).astype(np.float64)
    m = (q64 @ d64.T).max(axis=1)
    acc = 0.0
    for x in m:                      # token order
        acc += float(x)
    return np.float32(acc / len(m))


def maxsim_pairs_model(q_vecs, q_off, d_vecs, slot_start, slot_len, pair_q, pair_slot) -> np.ndarray:
    """rdx_maxsim_f16's arguments as numpy arrays -> fp32 [n_pairs]; NaN for a pair whose question or slot is out of range"""
    out = np.full((len(pair_q),), np.nan, dtype=np.float32)
    nq, ns, rows = len(q_off) - 1, len(slot_start), len(d_vecs)
    for p, (qi, si) in enumerate(zip(pair_q, pair_slot)):
        if not (0 <= qi < nq and 0 <= si < ns):
            continue
        a, n = int(slot_start[si]), int(slot_len[si])
        if not (1 <= n <= MAX_SLOT_TOKENS and 0 <= a and a + n <= rows):
            continue
        out[p] = maxsim_model(q_vecs[q_off[qi]:q_off[qi + 1]], d_vecs[a:a + n])
    return out


def quantize_rows_model(x):
    """quantize_model over the rows of x fp16 [rows][dim] -> (codes int8 [rows][dim], scales fp32 [rows])"""
    x = np.asarray(x, dtype=np.float16)
    x64 = x.astype(np.float64)
    with np.errstate(invalid="ignore"):
        a = np.abs(x64).max(axis=1) if x.shape[1] else np.zeros(len(x))      # exact: a maximum of fp16 values
    zero = ~np.isfinite(x64).all(axis=1) | (a == 0.0)
    a = np.where(zero, 0.0, a)
    scales = (a / 127.0).astype(np.float32)                                   # (float)((double)a / 127.0); +0.0 for a zero row
    den = np.where(zero, 1.0, scales.astype(np.float64))
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.clip(np.rint(np.where(zero[:, None], 0.0, x64) / den[:, None]), -127.0, 127.0)   # np.rint: ties to even; -0.0 is stored as 0
    return c.astype(np.int8), scales


def quantize_model(x):
    """one token vector: x fp16 [dim] -> (codes int8 [dim], scale fp32)"""
    c, s = quantize_rows_model(np.asarray(x, dtype=np.float16).reshape(1, -1))
    return c[0], s[0]


def _i8_parts(cq, sq, cd, sd):
    """-> (acc float64 [n_q][n_d]: the exact integer dot products, v fp32 [n_q][n_d] = (float)acc * sd, sq fp32)"""
    sq, sd = np.asarray(sq, dtype=np.float32), np.asarray(sd, dtype=np.float32)
    acc = np.asarray(cq, dtype=np.int8).astype(np.float64) @ np.asarray(cd, dtype=np.int8).astype(np.float64).T   # integers below 2^24: exact
    v = acc.astype(np.float32) * sd[None, :]                                  # (float)acc exact; one fp32 multiply
    return acc, v, sq


def maxsim_i8_model(cq, sq, cd, sd) -> np.float32:
    """score of one pair over quantised token vectors: cq int8 [n_q][dim], sq fp32 [n_q], cd int8 [n_d][dim], sd fp32 [n_d] -> fp32.
    No -0.0 arises in v for codes and scales that quantize_model made (sd_j = 0 only with acc_ij = 0), so the maximum is order-free."""
    _, v, sq = _i8_parts(cq, sq, cd, sd)
    m = v.max(axis=1)
    acc = 0.0
    for s, x in zip(sq, m):          # token order; a product of two floats is exact in fp64
        acc += float(s) * float(x)
    return np.float32(acc / len(m))


def maxsim_i8_pairs_model(q_codes, q_scales, q_off, d_codes, d_scales, slot_start, slot_len, pair_q, pair_slot) -> np.ndarray:
    """rdx_maxsim_i8's arguments as numpy arrays -> fp32 [n_pairs]; NaN for a pair whose question or slot is out of range"""
    out = np.full((len(pair_q),), np.nan, dtype=np.float32)
    nq, ns, rows = len(q_off) - 1, len(slot_start), len(d_codes)
    for p, (qi, si) in enumerate(zip(pair_q, pair_slot)):
        if not (0 <= qi < nq and 0 <= si < ns):
            continue
        a, n = int(slot_start[si]), int(slot_len[si])
        if not (1 <= n <= MAX_SLOT_TOKENS and 0 <= a and a + n <= rows):
            continue
        b, e = int(q_off[qi]), int(q_off[qi + 1])
        out[p] = maxsim_i8_model(q_codes[b:e], q_scales[b:e], d_codes[a:a + n], d_scales[a:a + n])
    return out


def quant_bound(cq, sq, cd, sd) -> float:
    """the bound on |maxsim_i8_model(cq, sq, cd, sd) - the fp64 MaxSim of the fp16 vectors the codes and scales were made from|,
    computed from the pair's codes and scales in fp64 (DESIGN.md §32 has the proof). With x = s c + e, |e_k| <= s / 2:
        |q_i . d_j - sq_i sd_j acc_ij| <= T_ij = sq_i sd_j ((|cq_i|_1 + |cd_j|_1) / 2 + dim / 4)
    (times 1 + 2^-30 for the rounding of the fp64 quotient that rint saw); v_ij carries one fp32 rounding, R_ij = 2^-24 sq_i sd_j
    |acc_ij|; the maximum over j is 1-Lipschitz in the sup norm, so token i is off by at most max_j (T_ij + R_ij); the score by their
    mean B, plus the final fp32 rounding and the fp64 sum: (S + B) (2^-24 + n_q 2^-52) with S = mean_i sq_i |m_i|."""
    acc, v, sq = _i8_parts(cq, sq, cd, sd)
    sq64, sd64 = sq.astype(np.float64), np.asarray(sd, dtype=np.float32).astype(np.float64)
    dim = np.asarray(cq).shape[1]
    n1q = np.abs(np.asarray(cq, dtype=np.int8).astype(np.float64)).sum(axis=1)
    n1d = np.abs(np.asarray(cd, dtype=np.int8).astype(np.float64)).sum(axis=1)
    ss = sq64[:, None] * sd64[None, :]
    t = ss * ((n1q[:, None] + n1d[None, :]) / 2.0 + dim / 4.0) * (1.0 + 2.0 ** -30)
    r = 2.0 ** -24 * ss * np.abs(acc)
    b = float((t + r).max(axis=1).mean())
    s = float((sq64 * np.abs(v.max(axis=1).astype(np.float64))).mean())
    return b + (s + b) * (2.0 ** -24 + len(sq64) * 2.0 ** -52)


def quantize_rows(vecs):
    """(codes int8, scales fp32) of fp16 rows: numpy in -> the model; a torch CUDA tensor in -> rdx_maxsim_quantize_i8 on the current
    stream, device tensors out. Never one for the other."""
    if isinstance(vecs, np.ndarray):
        return quantize_rows_model(vecs)
    from . import engine
    return engine.maxsim_quantize(vecs)


def maxsim_pairs(q_vecs, q_off, d_vecs, slot_start, slot_len, pair_q, pair_slot):
    """fp32 scores of the listed pairs: numpy in (a CPU store) -> the model, numpy out; torch CUDA tensors in -> rdx_maxsim_f16 on the
    current stream, a device tensor out (q_off: int32, pinned). Never one for the other: a missing kernel is an error. An int8 store's
    vectors are pairs (codes, scales), of the question and of the arena alike (MultiVectorStore.tables): -> maxsim_i8_pairs_model /
    rdx_maxsim_i8."""
    if isinstance(d_vecs, tuple):
        if not isinstance(q_vecs, tuple):
            raise TypeError("maxsim_pairs: an int8 arena (codes, scales) takes the question as (codes, scales) too")
        if isinstance(d_vecs[0], np.ndarray):
            return maxsim_i8_pairs_model(*q_vecs, q_off, *d_vecs, slot_start, slot_len, pair_q, pair_slot)
        from . import engine
        return engine.maxsim_i8(*q_vecs, q_off, *d_vecs, slot_start, slot_len, pair_q, pair_slot)
    if isinstance(d_vecs, np.ndarray):
        return maxsim_pairs_model(q_vecs, q_off, d_vecs, slot_start, slot_len, pair_q, pair_slot)
    from . import engine
    return engine.maxsim(q_vecs, q_off, d_vecs, slot_start, slot_len, pair_q, pair_slot)


# ---- the store ------------------------------------------------------------------------------------------------------------------------
def _as_vecs_off(matrices, dim: int):
    """matrices: a list of [T_i][dim] arrays / tensors, or (vecs [sum T_i][dim], off [n + 1]) -> (vecs, off int64 numpy)"""
    if isinstance(matrices, tuple) and len(matrices) == 2 and not (hasattr(matrices[1], "ndim") and matrices[1].ndim == 2):
        vecs, off = matrices
        off = np.asarray(off.cpu().numpy() if isinstance(off, torch.Tensor) else off, dtype=np.int64)
    else:
        mats = list(matrices)
        off = np.zeros(len(mats) + 1, dtype=np.int64)
        np.cumsum([int(m.shape[0]) for m in mats], out=off[1:])
        if mats and isinstance(mats[0], torch.Tensor):
            vecs = torch.cat([m.reshape(-1, dim) for m in mats]) if mats else torch.empty((0, dim), dtype=torch.float16)
        else:
            vecs = np.concatenate([np.asarray(m).reshape(-1, dim) for m in mats]) if mats else np.empty((0, dim), dtype=np.float16)
    if vecs.ndim != 2 or vecs.shape[1] != dim or len(off) < 1 or off[0] != 0 or off[-1] != vecs.shape[0] or (np.diff(off) < 0).any():
        raise ValueError(f"token vectors must be [rows][{dim}] with offsets from 0 to rows")
    return vecs, off


class MultiVectorStore:
    """The chunks' token vectors, keyed by chunk id: one fp16 arena [rows][dim] and a slot table (first row, rows) per chunk, grown
    by doubling. On a GPU (`device="cuda"`, "cuda:1") both are torch tensors there and pairs are scored by rdx_maxsim_f16; a CPU store
    keeps numpy arrays and scores through the model. A replaced or deleted chunk's rows are dead until compact(), which runs by itself
    when the dead rows outnumber the live ones. A chunk keeps its slot number through replace, compact, save and load; a deleted
    chunk's number is given to a later add.

    `dtype="int8"` keeps per-token symmetric int8 codes and one fp32 scale per token instead: a code arena int8
    [rows][dim] and a scale array fp32 [rows] that are grown, compacted, replaced and deleted together, dim + 4 bytes per token where
    fp16 takes 2 dim. `add` takes the same fp16 input and quantises it (rdx_maxsim_quantize_i8 on a GPU, quantize_model on the CPU);
    pairs are scored by rdx_maxsim_i8 / maxsim_i8_model."""

    FORMAT = 1          # the fp16 store's files; an int8 store writes FORMAT_I8
    FORMAT_I8 = 2

    def __init__(self, dim: int, device: str = "cpu", dtype: str = "float16"):
        if dtype not in ("float16", "int8"):
            raise ValueError(f"MultiVectorStore: dtype must be 'float16' or 'int8', not {dtype!r}")
        self.dtype = dtype
        self.is_i8 = dtype == "int8"
        if dim < 32 or dim > MAX_DIM or dim % 32:
            raise ValueError(f"MultiVectorStore: dim must be a multiple of 32 in [32, {MAX_DIM}], not {dim}")
        self.dim = int(dim)
        self.device = str(device)
        self.on_gpu = self.device.startswith("cuda")
        if self.on_gpu:
            from . import _lib
            _lib.load()                                  # raises RdxUnavailable: a GPU store has no torch substitute for the kernel
        self._arena = self._empty(0)
        self._scales = self._empty_scales(0) if self.is_i8 else None   # fp32 [rows]: row r's scale lives and moves with arena row r
        self._rows = 0                                   # arena rows in use (live + dead)
        self._dead = 0
        self._start = np.zeros(0, dtype=np.int64)        # host copy of the slot table, [slots]; a free slot has length 0
        self._len = np.zeros(0, dtype=np.int32)
        self._ids: List[Optional[str]] = []              # slot -> chunk id (None: free)
        self._slot: dict = {}                            # chunk id -> slot
        self._free: List[int] = []
        self._tables = None                              # the device copy of the slot table, rebuilt when it is asked for after a change

    # -- storage ------------------------------------------------------------------------------------------------------------------
    def _empty(self, rows: int):
        if self.on_gpu:
            return torch.empty((rows, self.dim), dtype=torch.int8 if self.is_i8 else torch.float16, device=self.device)
        return np.empty((rows, self.dim), dtype=np.int8 if self.is_i8 else np.float16)

    def _empty_scales(self, rows: int):
        if self.on_gpu:
            return torch.empty((rows,), dtype=torch.float32, device=self.device)
        return np.empty((rows,), dtype=np.float32)

    def _reserve(self, rows: int):
        cap = self._arena.shape[0]
        if rows <= cap:
            return
        new = self._empty(max(rows, 2 * cap, 1024))
        new[:self._rows] = self._arena[:self._rows]
        self._arena = new
        if self.is_i8:
            new = self._empty_scales(self._arena.shape[0])
            new[:self._rows] = self._scales[:self._rows]
            self._scales = new

    def _to_arena_type(self, vecs):
        if self.on_gpu:
            t = vecs if isinstance(vecs, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(vecs))
            return t.to(device=self.device, dtype=torch.float16)
        a = vecs.detach().cpu().numpy() if isinstance(vecs, torch.Tensor) else np.asarray(vecs)
        return a.astype(np.float16, copy=False)

    def _quantize(self, vecs):
        """fp16 rows in the arena's type (_to_arena_type) -> (codes, scales) in the arena's type; no rows: empty arrays, no call"""
        if vecs.shape[0] == 0:
            return self._empty(0), self._empty_scales(0)
        return quantize_rows(vecs.contiguous() if self.on_gpu else np.ascontiguousarray(vecs))

    def _put(self, base: int, vecs) -> None:
        """writes fp16 rows (any input type) at arena rows [base, base + len): as they are, or quantised, codes and scales together"""
        v = self._to_arena_type(vecs)
        if not self.is_i8:
            self._arena[base:base + v.shape[0]] = v
            return
        codes, scales = self._quantize(v)
        self._arena[base:base + v.shape[0]] = codes
        self._scales[base:base + v.shape[0]] = scales

    # -- writes -------------------------------------------------------------------------------------------------------------------
    def add(self, ids: Sequence[str], matrices) -> None:
        """ids[i] gets the token vectors matrices[i] ([T_i][dim], 1 <= T_i <= 8192), or rows [off[i], off[i + 1]) of (vecs, off). An
        id already present is replaced (it keeps its slot; the old rows count as dead); an id listed twice keeps the later matrix.
        An int8 store quantises the rows, and raises ValueError, leaving the store untouched, when they hold a non-finite value."""
        ids = list(ids)
        vecs, off = _as_vecs_off(matrices, self.dim)
        lens = np.diff(off)
        if len(off) != len(ids) + 1:
            raise ValueError(f"MultiVectorStore.add: {len(ids)} ids for {len(off) - 1} matrices")
        if len(ids) and (lens.min() < 1 or lens.max() > MAX_SLOT_TOKENS):
            raise ValueError(f"MultiVectorStore.add: a chunk has 1 to {MAX_SLOT_TOKENS} token vectors")
        if not ids:
            return
        if self.is_i8:                                   # refused before anything is written: a non-finite row has no scale
            v = self._to_arena_type(vecs)
            if not bool(torch.isfinite(v).all() if self.on_gpu else np.isfinite(v).all()):
                raise ValueError("MultiVectorStore.add: the token vectors hold a non-finite value")
            vecs = v
        base = self._rows
        self._reserve(base + int(off[-1]))
        self._put(base, vecs)
        self._rows = base + int(off[-1])
        self._start = np.concatenate([self._start, np.zeros(len(ids), dtype=np.int64)])     # room for every id being new; cut back below
        self._len = np.concatenate([self._len, np.zeros(len(ids), dtype=np.int32)])
        for i, cid in enumerate(ids):
            s = self._slot.get(cid)
            if s is None:
                if self._free:
                    s = self._free.pop()
                else:
                    s = len(self._ids)
                    self._ids.append(None)
                self._ids[s], self._slot[cid] = cid, s
            else:
                self._dead += int(self._len[s])
            self._start[s], self._len[s] = base + off[i], lens[i]
        self._start, self._len = self._start[:len(self._ids)].copy(), self._len[:len(self._ids)].copy()
        self._tables = None
        self._maybe_compact()

    def delete(self, ids: Sequence[str]) -> None:
        """forgets the listed chunks (absent ids are ignored); their rows count as dead"""
        for cid in ids:
            s = self._slot.pop(cid, None)
            if s is None:
                continue
            self._dead += int(self._len[s])
            self._ids[s], self._len[s], self._start[s] = None, 0, 0
            self._free.append(s)
        self._tables = None
        self._maybe_compact()

    def _maybe_compact(self):
        if self._dead > self._rows - self._dead:
            self.compact()

    def compact(self) -> None:
        """drops the dead rows: the live rows move to the front in slot order by ONE index_select; slot numbers stay"""
        live = np.flatnonzero(self._len > 0)
        lens = self._len[live].astype(np.int64)
        new_start = np.cumsum(lens) - lens
        total = int(lens.sum())
        src = np.repeat(self._start[live] - new_start, lens) + np.arange(total, dtype=np.int64)
        if self.on_gpu:
            at = torch.from_numpy(src).to(self.device)
            self._arena = self._arena.index_select(0, at)
            if self.is_i8:
                self._scales = self._scales.index_select(0, at)
        else:
            self._arena = self._arena[src]
            if self.is_i8:
                self._scales = self._scales[src]
        self._start[live] = new_start
        self._rows, self._dead, self._tables = total, 0, None

    # -- reads --------------------------------------------------------------------------------------------------------------------
    def __len__(self) -> int:
        return len(self._slot)

    def __contains__(self, cid) -> bool:
        return cid in self._slot

    def slots_of(self, ids: Sequence[str]) -> np.ndarray:
        """int64 [len(ids)]: each id's slot, -1 for an id the store does not hold"""
        return np.fromiter((self._slot.get(c, -1) for c in ids), dtype=np.int64, count=len(ids))

    def get(self, cid: str) -> np.ndarray:
        """the stored fp16 matrix of a chunk, on the host; of an int8 store the dequantised rows, fp32 codes * scale"""
        if self.is_i8:
            codes, scales = self.get_codes(cid)
            return codes.astype(np.float32) * scales[:, None]
        s = self._slot[cid]
        m = self._arena[int(self._start[s]):int(self._start[s]) + int(self._len[s])]
        return m.cpu().numpy() if self.on_gpu else m.copy()

    def get_codes(self, cid: str):
        """(codes int8 [T][dim], scales fp32 [T]) of a chunk of an int8 store, on the host"""
        if not self.is_i8:
            raise TypeError("MultiVectorStore.get_codes: the store keeps fp16 vectors (dtype='float16')")
        s = self._slot[cid]
        a, b = int(self._start[s]), int(self._start[s]) + int(self._len[s])
        c, sc = self._arena[a:b], self._scales[a:b]
        return (c.cpu().numpy(), sc.cpu().numpy()) if self.on_gpu else (c.copy(), sc.copy())

    def stats(self) -> dict:
        table = self._start.nbytes + self._len.nbytes
        if self.is_i8:
            return {"slots": len(self._slot), "live_tokens": self._rows - self._dead, "dead_tokens": self._dead,
                    "bytes": int(self._arena.shape[0]) * (self.dim + 4) + table, "dtype": "int8"}
        return {"slots": len(self._slot), "live_tokens": self._rows - self._dead, "dead_tokens": self._dead,
                "bytes": int(self._arena.shape[0]) * self.dim * 2 + table}

    def tables(self):
        """(arena rows in use [rows][dim], slot_start int64 [slots], slot_len int32 [slots]) as maxsim_pairs takes them: torch
        tensors on the store's GPU, numpy on the CPU. An int8 store's arena is the pair (codes [rows][dim], scales [rows])."""
        arena = (self._arena[:self._rows], self._scales[:self._rows]) if self.is_i8 else self._arena[:self._rows]
        if not self.on_gpu:
            return arena, self._start, self._len
        if self._tables is None:
            self._tables = (torch.from_numpy(self._start.copy()).to(self.device), torch.from_numpy(self._len.copy()).to(self.device))
        return (arena,) + self._tables

    def to_int8(self) -> "MultiVectorStore":
        """a new int8 store on the same device with the same ids and slot numbers, built by ONE quantise call over the live rows
        (this store is compacted first); its codes and scales are those of an int8 store that was given the same matrices"""
        if self.is_i8:
            raise TypeError("MultiVectorStore.to_int8: the store is int8 already")
        self.compact()
        st = MultiVectorStore(self.dim, self.device, dtype="int8")
        st._reserve(self._rows)
        st._put(0, self._arena[:self._rows])
        st._rows = self._rows
        st._start, st._len = self._start.copy(), self._len.copy()
        st._ids, st._slot, st._free = list(self._ids), dict(self._slot), list(self._free)
        return st

    # -- files --------------------------------------------------------------------------------------------------------------------
    def save(self, path: str) -> None:
        """compacts, then writes <path>/vecs.npy (fp16 rows), slots.npy (int64 [slots][2]: first row, rows) and store.json (dim, ids by
        slot); an int8 store writes codes.npy (int8 rows) and scales.npy (fp32) in place of vecs.npy, and store.json says "format": 2, "dtype": "int8" """
        self.compact()
        os.makedirs(path, exist_ok=True)
        host = lambda a: a.cpu().numpy() if self.on_gpu else a   # noqa: E731
        rows = self._arena[:self._rows]
        if self.is_i8:
            np.save(os.path.join(path, "codes.npy"), host(rows))
            np.save(os.path.join(path, "scales.npy"), host(self._scales[:self._rows]))
        else:
            np.save(os.path.join(path, "vecs.npy"), host(rows))
        np.save(os.path.join(path, "slots.npy"), np.stack([self._start, self._len.astype(np.int64)], axis=1).reshape(-1, 2))
        with open(os.path.join(path, "store.json"), "w") as f:
            if self.is_i8:
                json.dump({"format": self.FORMAT_I8, "dtype": "int8", "dim": self.dim, "ids": self._ids}, f)
            else:
                json.dump({"format": self.FORMAT, "dim": self.dim, "ids": self._ids}, f)

    @classmethod
    def load(cls, path: str, device: str = "cpu") -> "MultiVectorStore":
        with open(os.path.join(path, "store.json")) as f:
            meta = json.load(f)
        i8 = meta.get("format") == cls.FORMAT_I8 and meta.get("dtype") == "int8"
        if meta.get("format") != cls.FORMAT and not i8:
            raise ValueError(f"MultiVectorStore.load: unknown format {meta.get('format')!r}")
        st = cls(int(meta["dim"]), device, dtype="int8" if i8 else "float16")
        vecs = np.load(os.path.join(path, "codes.npy" if i8 else "vecs.npy"))
        slots = np.load(os.path.join(path, "slots.npy")).reshape(-1, 2)
        if vecs.dtype != (np.int8 if i8 else np.float16) or vecs.ndim != 2 or vecs.shape[1] != st.dim or len(slots) != len(meta["ids"]):
            raise ValueError("MultiVectorStore.load: the files do not belong together")
        st._reserve(len(vecs))
        if i8:
            scales = np.load(os.path.join(path, "scales.npy"))
            if scales.dtype != np.float32 or scales.shape != (len(vecs),):
                raise ValueError("MultiVectorStore.load: the files do not belong together")
            st._arena[:len(vecs)] = torch.from_numpy(vecs).to(st.device) if st.on_gpu else vecs
            st._scales[:len(vecs)] = torch.from_numpy(scales).to(st.device) if st.on_gpu else scales
        else:
            st._arena[:len(vecs)] = st._to_arena_type(vecs)
        st._rows = len(vecs)
        st._start, st._len = slots[:, 0].astype(np.int64), slots[:, 1].astype(np.int32)
        st._ids = list(meta["ids"])
        st._slot = {c: s for s, c in enumerate(st._ids) if c is not None}
        st._free = [s for s, c in enumerate(st._ids) if c is None][::-1]
        return st


# ---- the reranker ---------------------------------------------------------------------------------------------------------------------
class _Candidate(NamedTuple):
    chunk_id: str
    text: str


class _MaxSimModel:
    """What CrossEncoderReranker calls its model, scoring by late interaction: predict() -> float32 numpy (the CPU path), predict_device_batch() -> an
    fp32 device tensor. A pair is (question, _Candidate). All questions of a call are encoded in ONE
    embed_tokens_device call, all candidates the store does not hold in one more; the pairs are scored in at most two calls of
    maxsim_pairs (stored candidates from the store's arena, the others from a scratch arena that is dropped afterwards). With an int8
    store the questions' vectors are quantised once per call and the scratch arena by the same rule."""

    def __init__(self, provider, store: MultiVectorStore):
        self.provider, self.store = provider, store
        self.encoded = 0
        self.calls = 0                   # maxsim_pairs calls of the last scoring

    @property
    def path(self) -> str:
        if self.store.is_i8:
            return "maxsim-i8" if self.store.on_gpu else "maxsim-i8-model"
        return "maxsim" if self.store.on_gpu else "maxsim-model"

    def _vectors(self, texts, cap: int):
        """one embed_tokens_device call -> (vecs in the store's arena type, off int64 numpy), every text cut to its first `cap` vectors"""
        return self._cut(*self.provider.embed_tokens_device(list(texts)), cap)

    def _cut(self, v, off, cap: int):
        """embed_tokens_device's pair -> (vecs in the store's arena type, off int64 numpy), every text cut to its first `cap` vectors"""
        v, off = (torch.from_numpy(v) if isinstance(v, np.ndarray) else v), np.asarray(off, dtype=np.int64)
        if v.shape[1] != self.store.dim:
            raise ValueError(f"the provider's token vectors are {v.shape[1]} wide, the store's {self.store.dim}")
        lens = np.diff(off)
        if len(lens) and lens.max() > cap:
            keep = np.minimum(lens, cap)
            new_off = np.zeros_like(off)
            np.cumsum(keep, out=new_off[1:])
            src = np.repeat(off[:-1] - new_off[:-1], keep) + np.arange(int(new_off[-1]), dtype=np.int64)
            v, off = v.index_select(0, torch.from_numpy(src).to(v.device)), new_off
        return self.store._to_arena_type(v), off

    def _score(self, pairs, q_tokens=None) -> "torch.Tensor | np.ndarray":
        """q_tokens: embed_tokens_device's pair for the distinct questions in order of first appearance, for a caller that has
        encoded them already (rag_dpo_amd/m3.py); None: encoded here"""
        st, n = self.store, len(pairs)
        self.calls = 0
        questions: dict = {}
        pair_q = np.fromiter((questions.setdefault(q, len(questions)) for q, _ in pairs), dtype=np.int32, count=n)
        q_vecs, q_off = self._vectors(list(questions), MAX_Q_TOKENS) if q_tokens is None else self._cut(*q_tokens, MAX_Q_TOKENS)
        if st.is_i8:
            q_vecs = st._quantize(q_vecs)                # once per call: (codes, scales), used against the store and the scratch arena
        slots = st.slots_of([c.chunk_id for _, c in pairs])
        held, missing = np.flatnonzero(slots >= 0), np.flatnonzero(slots < 0)
        if st.on_gpu:
            dev = torch.device(st.device)
            q_off_t = torch.from_numpy(q_off.astype(np.int32)).pin_memory()   # (read by the library and by the kernel: pinned, alive until the caller's copy has drained the stream)
            self._keep = q_off_t
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
            scores = torch.empty((n,), dtype=torch.float32, device=dev)
        else:
            q_off_t, up, scores = q_off, (lambda a: a), np.empty((n,), dtype=np.float32)
        if len(held):
            arena, s0, sl = st.tables()
            scores[up(held)] = maxsim_pairs(q_vecs, q_off_t, arena, s0, sl, up(pair_q[held]), up(slots[held]))
            self.calls += 1
        if len(missing):
            texts: dict = {}
            scratch = np.fromiter((texts.setdefault(pairs[p][1].chunk_id, len(texts)) for p in missing), dtype=np.int64, count=len(missing))
            by_id = {c.chunk_id: c.text for _, c in (pairs[p] for p in missing)}
            d_vecs, d_off = self._vectors([by_id[cid] for cid in texts], MAX_SLOT_TOKENS)
            self.encoded += len(texts)
            if st.is_i8:
                d_vecs = st._quantize(d_vecs)            # by the store's rule: a chunk scores the same whether it was stored or not
            scores[up(missing)] = maxsim_pairs(q_vecs, q_off_t, d_vecs, up(d_off[:-1].copy()), up(np.diff(d_off).astype(np.int32)),
                                               up(pair_q[missing]), up(scratch))
            self.calls += 1
        return scores

    def predict(self, pairs, batch_size: int = 32, show_progress_bar: bool = False) -> np.ndarray:
        if not pairs:
            return np.zeros((0,), dtype=np.float32)
        s = self._score(pairs)
        return s.cpu().numpy() if isinstance(s, torch.Tensor) else s

    def predict_device_batch(self, pairs, batch_size: int = 32) -> torch.Tensor:
        from . import _lib as L
        if not self.store.on_gpu:
            raise RuntimeError("predict_device_batch needs the store on a GPU")
        if not 1 <= len(pairs) <= L.MAXSIM_MAX_PAIRS:
            raise ValueError(f"rdx_maxsim_f16 / rdx_maxsim_i8 score 1 to {L.MAXSIM_MAX_PAIRS} pairs per call, got {len(pairs)}")
        return self._score(pairs)


class LateInteractionReranker(CrossEncoderReranker):
    """CrossEncoderReranker's interface (rerank, rerank_batch, RankedChunk; DenseRetriever.retrieve_reranked(_batch) take it unchanged)
    with MaxSim scores: the question's token vectors against the candidates' stored ones. `provider`: an EmbeddingProvider with a
    ColBERT head; `store`: the MultiVectorStore that index_chunks() fills; `device`: where boosts and selection run (default: the
    store's). min_score=None means no cut (-inf): MaxSim scores live in [-1, 1], not in a sigmoid's range. A candidate the store does
    not hold is encoded on the fly (all of a call's in one forward), scored from a scratch arena, not stored, and counted in
    last_rerank_stats["encoded"]. A question of more than 256 token vectors is scored by its first 256. On a GPU both rerank and
    rerank_batch end in one selection launch and ONE copy to the host; on any failure of the scoring the result is the reference's
    fallback (the first top_k candidates, similarity_score as score)."""

    def __init__(self, provider, store: MultiVectorStore, device: Optional[str] = None, min_score: Optional[float] = None, max_length: int = 512):
        device = store.device if device is None else str(device)
        if device.startswith("cuda") != store.on_gpu:
            raise ValueError(f"LateInteractionReranker: the store lives on {store.device}, the reranker was asked to run on {device}")
        super().__init__(model_name="late-interaction", device=device, max_length=max_length,
                         min_score=float("-inf") if min_score is None else float(min_score))
        self.provider, self.store = provider, store
        self._model = _MaxSimModel(provider, store)
        self._on_gpu = store.on_gpu                      # which of rerank's two paths runs (M3Reranker may have no store)
        self._is_loaded = True
        self._nested = False

    def chunk_text(self, chunk) -> str:
        """the reranker's text rule: heading + "\\n" + text, cut at max_length * 4 characters"""
        return super()._pairs("", [chunk])[0][1]

    def _pairs(self, query: str, chunks) -> list:
        return [(query, _Candidate(c.chunk_id, self.chunk_text(c))) for c in chunks]

    def index_chunks(self, chunks, batch_size: int = 256) -> int:
        """encodes the chunks' texts (chunk_text) and stores their token vectors under chunk_id -> chunks stored"""
        chunks = list(chunks)
        for a in range(0, len(chunks), batch_size):
            part = chunks[a:a + batch_size]
            vecs, off = self._model._vectors([self.chunk_text(c) for c in part], MAX_SLOT_TOKENS)
            self.store.add([c.chunk_id for c in part], (vecs, off))
        return len(chunks)

    def _fallback(self, chunks, top_k: int) -> List[RankedChunk]:
        return [_ranked(c, c.similarity_score, i) for i, c in enumerate(chunks[:top_k])]

    def _finish(self, stats):
        if not self._nested and stats is not None:
            stats["encoded"] = self._model.encoded

    def rerank(self, query: str, chunks: List, top_k: int = 8, topic_matcher=None, question_topics: Optional[List[str]] = None) -> List[RankedChunk]:
        if not chunks:
            return []
        if not self._nested:
            self._model.encoded = 0
        if not self._on_gpu:
            out = super().rerank(query, chunks, top_k=top_k, topic_matcher=topic_matcher, question_topics=question_topics)
            self._finish(self.last_rerank_stats)
            return out
        # the batch's path for one question: one selection launch, one copy to the host
        chunks = list(chunks)
        total = {"questions": 0, "pairs": 0, "tokens": None, "ms_forward": None, "ms_head_select": None, "path": None, "kept": 0, "device_calls": 0}
        self.last_rerank_stats = total
        ranked = None
        if len(chunks) <= MAX_GPU_CANDIDATES:
            ranked = self._rerank_group([0], [query], [chunks], [question_topics], top_k, topic_matcher, total)
        else:
            logger.error(f"reranking failed: the GPU reranker takes at most {MAX_GPU_CANDIDATES} candidates per question, got {len(chunks)}")
        self._finish(total)
        if ranked is None:                                           # reranker.py:153-160
            total["path"] = "fallback"
            return self._fallback(chunks, top_k)
        return ranked[0]

    def rerank_batch(self, queries, chunks_lists, top_k: int = 8, topic_matcher=None, question_topics=None) -> List[List[RankedChunk]]:
        self._model.encoded = 0
        self._nested = True
        try:
            out = super().rerank_batch(queries, chunks_lists, top_k=top_k, topic_matcher=topic_matcher, question_topics=question_topics)
        finally:
            self._nested = False
        self._finish(self.last_rerank_stats)
        return out
