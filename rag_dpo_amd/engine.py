"""HipIndex — one corpus shard in one MI355X's HBM, driven through the C-ABI (include/rdx.h).

numpy arrays cross as host pointers (RDX_HOST, synchronous); torch CUDA tensors cross as device
pointers (RDX_DEVICE) on the current torch stream. No arithmetic happens in this file.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _lib as L


def _np_ptr(a: np.ndarray):
    return ctypes.c_void_p(a.ctypes.data)


def _ptr(t):
    """a torch tensor's data pointer as the C-ABI takes it; None stays None (an optional argument)"""
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _want_tensors(what: str, device_index, *pairs):
    """ValueError(what) unless every (tensor, dtype) is a contiguous CUDA tensor of that dtype on the first one's device — on
    cuda:device_index where one is given"""
    dev = pairs[0][0].device
    for t, dt in pairs:
        if not t.is_cuda or t.device != dev or t.dtype != dt or not t.is_contiguous() \
                or (device_index is not None and t.device.index != device_index):
            raise ValueError(what)


class _Handle:
    """one opaque librdx handle and the rdx_*_destroy that frees it: close() may be called any number of times, and __del__
    swallows errors (at interpreter exit the library may be gone before the object)"""
    _destroy = ""   # the subclass names its destroy function
    _lib = None
    _h = None

    def _new_handle(self):
        """loads the library; -> what an rdx_*_create takes as its `out`"""
        self._lib = L.load(require_gpu=True)
        self._h = ctypes.c_void_p()
        return ctypes.byref(self._h)

    def close(self):
        if self._h is not None and self._h.value:
            getattr(self._lib, self._destroy)(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ResidentMask(_Handle):
    """a `where` bitmap resident in HBM (rdx_mask): made once per distinct filter, passed with every search"""
    _destroy = "rdx_mask_destroy"

    def __init__(self, lib, handle):
        self._lib, self._h = lib, handle


def _filter_host(fn, lead, words: int, base_bits) -> np.ndarray:
    """DocStore.filter / MetaStore.filter: fn(*lead, base_bits, out_bits, space, stream) is rdx_docs_filter / rdx_meta_filter"""
    out = np.zeros(words, dtype=np.uint32)
    base = None
    if base_bits is not None:
        base = np.ascontiguousarray(base_bits, dtype=np.uint32)
        if base.shape[0] != words:
            raise ValueError("base_bits must hold ceil(rows/32) words")
    L.check(fn(*lead, _np_ptr(base) if base is not None else None, _np_ptr(out), L.RDX_HOST, None))
    return out


def _filter_device(fn, lead, device: int, words: int, out_bits, base_bits):
    """DocStore.filter_device / MetaStore.filter_device: the same call with device pointers, on the current torch stream"""
    import torch
    for t in (out_bits, base_bits):
        if t is not None and (not t.is_cuda or t.device.index != device or t.dtype != torch.int32
                              or t.numel() != words or not t.is_contiguous()):
            raise ValueError(f"expected a contiguous int32 tensor of {words} words on cuda:{device}")
    stream = HipIndex._raw_stream(out_bits.device)
    L.check(fn(*lead, _ptr(base_bits), _ptr(out_bits), L.RDX_DEVICE, ctypes.c_void_p(stream)))


class HipIndex(_Handle):
    _destroy = "rdx_index_destroy"
    has_device_docs = True   # Collection keeps a DocStore on this device for where_document
    has_device_meta = True   # ... and a MetaStore for `where` (single-device collections)

    def __init__(self, dim: int, device: int = 0):
        out = self._new_handle()
        L.check(self._lib.rdx_index_create(int(device), int(dim), out))
        self.dim = int(dim)
        self.device = int(device)

    def __len__(self) -> int:
        n = ctypes.c_int64(0)
        L.check(self._lib.rdx_index_count(self._h, ctypes.byref(n)))
        return int(n.value)

    def reserve(self, rows: int):
        L.check(self._lib.rdx_index_reserve(self._h, int(rows)))

    def set_option(self, name: str, value: int):
        L.check(self._lib.rdx_index_set_option(self._h, name.encode(), int(value)))

    def xcd_shares(self, new=None):
        """the main scan's per-XCD tile shares (include/rdx.h rdx_index_xcd_shares): returns the current 8 values; `new` replaces them"""
        out = (ctypes.c_double * 8)()
        inp = (ctypes.c_double * 8)(*[float(x) for x in new]) if new is not None else None
        L.check(self._lib.rdx_index_xcd_shares(self._h, out, inp))
        return list(out)

    # ---- helpers ----------------------------------------------------------------------------
    def _rows_arg(self, x, dtype=np.float32):
        """-> (pointer, n, space, keepalive)"""
        import torch
        if isinstance(x, torch.Tensor):
            want = torch.float32 if dtype == np.float32 else torch.bfloat16
            if x.dtype != want or x.dim() != 2 or x.shape[1] != self.dim:
                raise ValueError(f"expected a [n][{self.dim}] {want} tensor, got {tuple(x.shape)} {x.dtype}")
            if x.is_cuda:
                if x.device.index != self.device:
                    raise ValueError("tensor lives on another device than the index")
                x = x.contiguous()
                torch.cuda.current_stream(x.device).synchronize()  # ingest runs on the index's own stream
                return _ptr(x), x.shape[0], L.RDX_DEVICE, x
            x = x.numpy() if dtype == np.float32 else x.view(torch.uint16).numpy()
        a = np.ascontiguousarray(x, dtype=dtype if dtype == np.float32 else np.uint16)
        if a.ndim != 2 or a.shape[1] != self.dim:
            raise ValueError(f"expected [n][{self.dim}] embeddings, got shape {a.shape}")
        return _np_ptr(a), a.shape[0], L.RDX_HOST, a

    # ---- ingest -----------------------------------------------------------------------------
    def add(self, rows):
        p, n, space, keep = self._rows_arg(rows)
        L.check(self._lib.rdx_index_add(self._h, p, n, space))

    def add_stored(self, rows):
        """rows previously returned by get() (already normalised): stored verbatim (snapshot reload)"""
        p, n, space, keep = self._rows_arg(rows)
        L.check(self._lib.rdx_index_add_stored(self._h, p, n, space))

    def add_bf16(self, rows):
        p, n, space, keep = self._rows_arg(rows, dtype=np.uint16)
        L.check(self._lib.rdx_index_add_bf16(self._h, p, n, space))

    def update(self, row_ids, rows):
        ids = np.ascontiguousarray(row_ids, dtype=np.int64)
        a = np.ascontiguousarray(rows, dtype=np.float32)
        if a.ndim != 2 or a.shape != (ids.shape[0], self.dim):
            raise ValueError("update: rows must be [len(row_ids)][dim]")
        L.check(self._lib.rdx_index_update(self._h, _np_ptr(ids), _np_ptr(a), ids.shape[0], L.RDX_HOST))

    def update_stored(self, row_ids, rows):
        """update() for rows that are stored values (spaces.py's lifted rows): written verbatim"""
        ids = np.ascontiguousarray(row_ids, dtype=np.int64)
        a = np.ascontiguousarray(rows, dtype=np.float32)
        if a.ndim != 2 or a.shape != (ids.shape[0], self.dim):
            raise ValueError("update_stored: rows must be [len(row_ids)][dim]")
        L.check(self._lib.rdx_index_update_stored(self._h, _np_ptr(ids), _np_ptr(a), ids.shape[0], L.RDX_HOST))

    def get_device(self, row_ids, out):
        """get() with torch CUDA tensors: row_ids int64 [n], out fp32 [n][dim] on this index's device; complete on return (the call
        waits for the device first: include/rdx.h, calls without a stream argument)"""
        import torch
        n = row_ids.numel()
        if not (row_ids.is_cuda and out.is_cuda and row_ids.device.index == self.device and out.device.index == self.device
                and row_ids.dtype == torch.int64 and out.dtype == torch.float32 and row_ids.is_contiguous() and out.is_contiguous()
                and out.numel() == n * self.dim):
            raise ValueError(f"get_device: expected int64 [n] and fp32 [n][{self.dim}] contiguous tensors on cuda:{self.device}")
        L.check(self._lib.rdx_index_get(self._h, _ptr(row_ids), n, _ptr(out), L.RDX_DEVICE))

    def get(self, row_ids) -> np.ndarray:
        ids = np.ascontiguousarray(row_ids, dtype=np.int64)
        out = np.empty((ids.shape[0], self.dim), dtype=np.float32)
        L.check(self._lib.rdx_index_get(self._h, _np_ptr(ids), ids.shape[0], _np_ptr(out), L.RDX_HOST))
        return out

    def set_row_ids(self, first_row: int, ids):
        """returned row id of local row first_row + i = ids[i] (strictly increasing over the shard)"""
        a = np.ascontiguousarray(ids, dtype=np.int64)
        L.check(self._lib.rdx_index_set_row_ids(self._h, int(first_row), _np_ptr(a), a.shape[0], L.RDX_HOST))

    def compact(self, keep_rows):
        keep = np.ascontiguousarray(keep_rows, dtype=np.int64)
        L.check(self._lib.rdx_index_compact(self._h, _np_ptr(keep), keep.shape[0]))

    # ---- search -----------------------------------------------------------------------------
    def make_mask(self, allow_bits) -> ResidentMask:
        """allow_bits: ceil(count/32) uint32 words, a numpy array or a torch tensor (int32 / uint32) on this index's device
        (e.g. DocStore.filter's output: the bitmap then never leaves the device)"""
        words = (len(self) + 31) // 32
        h = ctypes.c_void_p()
        import sys
        torch = sys.modules.get("torch")
        if torch is not None and isinstance(allow_bits, torch.Tensor) and allow_bits.is_cuda:
            if allow_bits.device.index != self.device:
                raise ValueError("allow_bits lives on another device than the index")
            if allow_bits.element_size() != 4 or allow_bits.numel() != words or not allow_bits.is_contiguous():
                raise ValueError("allow_bits must hold ceil(count/32) contiguous 32-bit words")
            L.check(self._lib.rdx_mask_create(self._h, _ptr(allow_bits), L.RDX_DEVICE, ctypes.byref(h)))
            return ResidentMask(self._lib, h)
        allow_bits = np.ascontiguousarray(allow_bits, dtype=np.uint32)
        if allow_bits.shape[0] != words:
            raise ValueError("allow_bits must hold ceil(count/32) words")
        L.check(self._lib.rdx_mask_create(self._h, _np_ptr(allow_bits), L.RDX_HOST, ctypes.byref(h)))
        return ResidentMask(self._lib, h)

    def search(self, queries, k: int, allow_bits: Optional[np.ndarray] = None, mask: Optional[ResidentMask] = None
               ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Host in / host out. Returns (score f32[nq,k], row i64[nq,k], count i32[nq]).
        allow_bits: host bitmap uploaded for this call; mask: a resident one (make_mask) — not both."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"expected [nq][{self.dim}] query embeddings, got shape {q.shape}")
        nq = q.shape[0]
        sc = np.empty((nq, k), dtype=np.float32)
        ro = np.empty((nq, k), dtype=np.int64)
        cn = np.zeros((nq,), dtype=np.int32)
        bits = allow_bits
        if allow_bits is not None and mask is None:     # (beside a mask it is refused unread)
            allow_bits = np.ascontiguousarray(allow_bits, dtype=np.uint32)
            if allow_bits.shape[0] != (len(self) + 31) // 32:
                raise ValueError("allow_bits must hold ceil(count/32) words")
            bits = _np_ptr(allow_bits)
        self._search(_np_ptr(q), nq, k, bits, mask, (_np_ptr(sc), _np_ptr(ro), _np_ptr(cn)), L.RDX_HOST, None)
        return sc, ro, cn

    def _search(self, q, nq: int, k: int, bits, mask: Optional[ResidentMask], outs, where: int, stream):
        """search's and search_device's one call into the library: rdx_search_masked with a resident mask, else rdx_search with `bits`
        (the call's own bitmap, or None). q, bits and outs = (score, row, count) are pointers on the side `where` names (RDX_HOST /
        RDX_DEVICE)."""
        if mask is not None:
            if bits is not None:
                raise ValueError("pass allow_bits or mask, not both")
            L.check(self._lib.rdx_search_masked(self._h, q, nq, int(k), mask._h, *outs, where, stream))
        else:
            L.check(self._lib.rdx_search(self._h, q, nq, int(k), bits, *outs, where, stream))

    @staticmethod
    def _raw_stream(device) -> int:
        """handle of torch's current stream on `device` (the private one-call form when this torch has it: 0.3 instead of 4 us)"""
        import torch
        try:
            return torch._C._cuda_getCurrentRawStream(device.index if device.index is not None else torch.cuda.current_device())
        except AttributeError:   # pragma: no cover
            return torch.cuda.current_stream(device).cuda_stream

    def search_device(self, queries, k: int, out_score, out_row, out_count, allow_bits=None, mask: Optional[ResidentMask] = None):
        """torch CUDA tensors in/out, enqueued on the current torch stream (no host copies).
        allow_bits: a device bitmap for this call; mask: a resident one (make_mask) — not both."""
        nq = self._device_call_shapes(queries, k, out_score, out_row, out_count)
        self._search(_ptr(queries), nq, k, _ptr(allow_bits), mask, (_ptr(out_score), _ptr(out_row), _ptr(out_count)), L.RDX_DEVICE,
                     ctypes.c_void_p(self._raw_stream(queries.device)))

    def _search_filtered(self, q, nq: int, k: int, masks: Sequence[ResidentMask], query_filter, outs, where: int, stream):
        """search_filtered's and search_filtered_device's one call into the library (rdx_search_filtered): the masks' handles and
        the queries' indices are host arrays whichever side `where` names for q and outs"""
        qf = np.ascontiguousarray(query_filter, dtype=np.int32)
        if qf.shape != (nq,):
            raise ValueError(f"query_filter must hold one int32 per query ({nq}), got shape {qf.shape}")
        handles = (ctypes.c_void_p * max(len(masks), 1))(*[m._h for m in masks])
        L.check(self._lib.rdx_search_filtered(self._h, q, nq, int(k), handles if len(masks) else None, len(masks), _np_ptr(qf), *outs,
                                              where, stream))

    def search_filtered(self, queries, k: int, masks: Sequence[ResidentMask], query_filter
                        ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """search() with a filter per query: query q is held to masks[query_filter[q]] (make_mask), to none when query_filter[q] is -1.
        Host in / host out; per query the results search(mask=...) gives for it alone (include/rdx.h rdx_search_filtered)."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"expected [nq][{self.dim}] query embeddings, got shape {q.shape}")
        nq = q.shape[0]
        sc = np.empty((nq, k), dtype=np.float32)
        ro = np.empty((nq, k), dtype=np.int64)
        cn = np.zeros((nq,), dtype=np.int32)
        self._search_filtered(_np_ptr(q), nq, k, masks, query_filter, (_np_ptr(sc), _np_ptr(ro), _np_ptr(cn)), L.RDX_HOST, None)
        return sc, ro, cn

    def search_filtered_device(self, queries, k: int, out_score, out_row, out_count, masks: Sequence[ResidentMask], query_filter):
        """search_device() with a filter per query (see search_filtered): torch CUDA tensors in/out, enqueued on the current torch
        stream; masks and query_filter (int32 numpy) stay on the host"""
        nq = self._device_call_shapes(queries, k, out_score, out_row, out_count)
        self._search_filtered(_ptr(queries), nq, k, masks, query_filter, (_ptr(out_score), _ptr(out_row), _ptr(out_count)), L.RDX_DEVICE,
                              ctypes.c_void_p(self._raw_stream(queries.device)))

    @staticmethod
    def _device_call_shapes(queries, k: int, out_score, out_row, out_count) -> int:
        """search_device's and search_device_async's conditions on their tensors -> nq"""
        import torch
        nq = queries.shape[0]
        assert queries.is_cuda and queries.dtype == torch.float32 and queries.is_contiguous()
        assert out_score.shape == (nq, k) and out_score.dtype == torch.float32 and out_score.is_contiguous()
        assert out_row.shape == (nq, k) and out_row.dtype == torch.int64 and out_row.is_contiguous()
        assert out_count.shape == (nq,) and out_count.dtype == torch.int32
        return nq

    def search_device_async(self, queries, k: int, out_score, out_row, out_count, out_flags=None, mask: Optional[ResidentMask] = None):
        """enqueue the search on the current torch stream and return at once; search_wait() completes it (include/rdx.h).
        `queries` may be reused by stream-ordered work enqueued afterwards; the outputs (and out_flags: int32[4] on the device,
        [0] = 1 while the results are incomplete) must stay valid until search_wait() has returned."""
        import torch
        nq = self._device_call_shapes(queries, k, out_score, out_row, out_count)
        assert out_flags is None or (out_flags.numel() >= L.PACKED_FLAGS and out_flags.dtype == torch.int32)
        L.check(self._lib.rdx_search_async(self._h, _ptr(queries), nq, int(k), mask._h if mask is not None else None, _ptr(out_score),
                                           _ptr(out_row), _ptr(out_count), _ptr(out_flags), ctypes.c_void_p(self._raw_stream(queries.device))))

    def search_wait(self) -> bool:
        """-> True when fallback passes rewrote results after the asynchronous search's kernels (consumers must be re-run)"""
        redone = ctypes.c_int(0)
        L.check(self._lib.rdx_search_wait(self._h, ctypes.byref(redone)))
        return bool(redone.value)

    def last_stats_struct(self):
        """the raw rdx_search_stats of the last search (a ctypes struct: field access without building a dict)"""
        s = L.SearchStats()
        L.check(self._lib.rdx_search_last_stats(self._h, ctypes.byref(s)))
        return s

    def last_stats(self) -> dict:
        d = self.last_stats_struct().as_dict()
        bits = ctypes.c_int32(0)
        L.check(self._lib.rdx_search_last_coarse_bits(self._h, ctypes.byref(bits)))
        d["coarse_bits"] = int(bits.value)   # 16 / 8: which MFMA pass ran the main scan; 0: the exact scan alone
        return d


class DocStore(_Handle):
    """The rows' document text resident in one device's HBM (include/rdx.h rdx_docs_*): where_document's substring scan.
    Rows follow the collection's row order; the caller keeps it in step (append / replace / compact)."""

    _destroy = "rdx_docs_destroy"

    def __init__(self, device: int = 0):
        out = self._new_handle()
        L.check(self._lib.rdx_docs_create(int(device), out))
        self.device = int(device)

    def append(self, docs):
        from .where_document import pack_docs
        b, off = pack_docs(docs)
        L.check(self._lib.rdx_docs_append(self._h, _np_ptr(b), _np_ptr(off), len(docs)))

    def replace(self, rows, docs):
        from .where_document import pack_docs
        ids = np.ascontiguousarray(rows, dtype=np.int64)
        b, off = pack_docs(docs)
        if ids.shape[0] != len(docs):
            raise ValueError("replace: one document per row")
        L.check(self._lib.rdx_docs_replace(self._h, _np_ptr(ids), _np_ptr(b), _np_ptr(off), ids.shape[0]))

    def compact(self, keep_rows):
        keep = np.ascontiguousarray(keep_rows, dtype=np.int64)
        L.check(self._lib.rdx_docs_compact(self._h, _np_ptr(keep), keep.shape[0]))

    def stats(self) -> dict:
        r, lv, ar = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        L.check(self._lib.rdx_docs_stats(self._h, ctypes.byref(r), ctypes.byref(lv), ctypes.byref(ar)))
        return {"rows": r.value, "live_bytes": lv.value, "arena_bytes": ar.value}

    def __len__(self) -> int:
        return self.stats()["rows"]

    def set_query(self, leaves, program=()):
        """leaves: non-empty byte strings; program: postfix ops (include/rdx.h RDX_DOCS_OP_*), may be empty for contains()"""
        from .where_document import pack_patterns
        b, off = pack_patterns(leaves)
        prog = np.ascontiguousarray(program, dtype=np.int32)
        self._n_leaves = 0
        L.check(self._lib.rdx_docs_set_query(self._h, _np_ptr(b), _np_ptr(off), len(leaves),
                                             _np_ptr(prog) if prog.shape[0] else None, prog.shape[0]))
        self._n_leaves = len(leaves)

    _n_leaves = 0

    def contains(self) -> np.ndarray:
        """-> uint32 [P][ceil(rows/32)]: the leaf bitmaps of the query set last (host); P = its number of leaves"""
        if not self._n_leaves:
            raise RuntimeError("DocStore.contains: no query set")
        out = np.zeros((self._n_leaves, (len(self) + 31) // 32), dtype=np.uint32)
        L.check(self._lib.rdx_docs_contains(self._h, _np_ptr(out), L.RDX_HOST, None))
        return out

    def filter(self, base_bits: Optional[np.ndarray] = None) -> np.ndarray:
        """-> uint32 [ceil(rows/32)]: program(leaves) AND base_bits (host in, host out)"""
        return _filter_host(self._lib.rdx_docs_filter, (self._h,), (len(self) + 31) // 32, base_bits)

    def filter_device(self, out_bits, base_bits=None):
        """torch int32 tensors on the store's device, enqueued on the current torch stream: nothing crosses PCIe"""
        _filter_device(self._lib.rdx_docs_filter, (self._h,), self.device, (len(self) + 31) // 32, out_bits, base_bits)


class MetaStore(_Handle):
    """Some of a collection's metadata columns resident in one device's HBM (include/rdx.h rdx_meta_*): the `where` predicate
    scan. A column lives in a slot chosen by the caller; rows follow the collection's row order and the caller keeps them in
    step (set_rows / drop_column / truncate). Nothing is allocated on the device before the first set_rows."""
    _destroy = "rdx_meta_destroy"

    def __init__(self, device: int = 0):
        out = self._new_handle()
        L.check(self._lib.rdx_meta_create(int(device), out))
        self.device = int(device)

    def set_rows(self, col: int, first_row: int, kind, num, code):
        """rows [first_row, first_row + n) of slot `col` from where.Column's three arrays (kind int8 / uint8, num f64, code i32)"""
        kind = np.ascontiguousarray(kind).view(np.uint8)
        num = np.ascontiguousarray(num, dtype=np.float64)
        code = np.ascontiguousarray(code, dtype=np.int32)
        if not (kind.shape[0] == num.shape[0] == code.shape[0]):
            raise ValueError("set_rows: kind, num and code must have one entry per row")
        L.check(self._lib.rdx_meta_set_rows(self._h, int(col), int(first_row), _np_ptr(kind), _np_ptr(num), _np_ptr(code), kind.shape[0]))

    def drop_column(self, col: int):
        L.check(self._lib.rdx_meta_drop_column(self._h, int(col)))

    def truncate(self, rows: int):
        L.check(self._lib.rdx_meta_truncate(self._h, int(rows)))

    def stats(self) -> dict:
        c, b = ctypes.c_int64(), ctypes.c_int64()
        L.check(self._lib.rdx_meta_stats(self._h, ctypes.byref(c), ctypes.byref(b)))
        return {"columns": c.value, "bytes": b.value}

    def set_query(self, leaves, program):
        """leaves: a where_device.LEAF array (col = slot); program: postfix ops (include/rdx.h RDX_META_OP_*)"""
        from .where_device import LEAF
        lv = np.ascontiguousarray(leaves, dtype=LEAF)
        prog = np.ascontiguousarray(program, dtype=np.int32)
        L.check(self._lib.rdx_meta_set_query(self._h, _np_ptr(lv) if lv.shape[0] else None, lv.shape[0],
                                             _np_ptr(prog) if prog.shape[0] else None, prog.shape[0]))

    def filter(self, rows: int, base_bits: Optional[np.ndarray] = None) -> np.ndarray:
        """-> uint32 [ceil(rows/32)]: program(leaves) AND base_bits (host in, host out)"""
        return _filter_host(self._lib.rdx_meta_filter, (self._h, int(rows)), (int(rows) + 31) // 32, base_bits)

    def filter_device(self, rows: int, out_bits, base_bits=None):
        """torch int32 tensors on the store's device, enqueued on the current torch stream: nothing crosses PCIe"""
        _filter_device(self._lib.rdx_meta_filter, (self._h, int(rows)), self.device, (int(rows) + 31) // 32, out_bits, base_bits)


# ---- the "ip" / "l2" spaces (include/rdx.h rdx_space_*; rag_dpo_amd/spaces.py drives them) ------------------------------------
def _space_ptrs(*tensors):
    dev = tensors[0].device
    for t in tensors:
        if t is not None and (not t.is_cuda or t.device != dev or not t.is_contiguous()):
            raise ValueError("the rdx_space_* calls take contiguous torch tensors on one CUDA device")
    return dev, [_ptr(t) for t in tensors]


def space_measure(kind: int, rows):
    """rows fp32 [n][dim] on the device -> (lifted_sq fp64 [n], bad int32 [n]) there, enqueued on the current torch stream"""
    import torch
    lib = L.load(require_gpu=True)
    n, dim = rows.shape
    sq = torch.empty(n, dtype=torch.float64, device=rows.device)
    bad = torch.empty(n, dtype=torch.int32, device=rows.device)
    dev, (pr, ps, pb) = _space_ptrs(rows, sq, bad)
    L.check(lib.rdx_space_measure(dev.index, int(kind), pr, n, dim, ps, pb, ctypes.c_void_p(HipIndex._raw_stream(dev))))
    return sq, bad


def space_lift(kind: int, rows, scale_exp: int, is_query: bool = False):
    """rows fp32 [n][dim] on the device -> (engine rows fp32 [n][engine dim], bad int32 [n])"""
    import torch
    lib = L.load(require_gpu=True)
    n, dim = rows.shape
    out = torch.empty((n, dim + 4 if kind == L.SPACE_L2 else dim), dtype=torch.float32, device=rows.device)
    bad = torch.empty(n, dtype=torch.int32, device=rows.device)
    dev, (pr, po, pb) = _space_ptrs(rows, out, bad)
    L.check(lib.rdx_space_lift(dev.index, int(kind), int(bool(is_query)), pr, n, dim, int(scale_exp), po, pb,
                               ctypes.c_void_p(HipIndex._raw_stream(dev))))
    return out, bad


def space_rescore(kind: int, queries, cand_vecs, cand_rows, cand_scores, cand_counts, k: int, scale_exp: int, guard: float):
    """-> (dist f32 [nq][k], rows i64 [nq][k], counts i32 [nq], proven i32 [nq]) of the candidates [nq][kp]"""
    import torch
    lib = L.load(require_gpu=True)
    nq, dim = queries.shape
    kp = cand_rows.shape[1]
    dev = queries.device
    work = torch.empty((nq, kp), dtype=torch.float32, device=dev)
    od = torch.empty((nq, k), dtype=torch.float32, device=dev)
    orow = torch.empty((nq, k), dtype=torch.int64, device=dev)
    oc = torch.empty(nq, dtype=torch.int32, device=dev)
    pv = torch.empty(nq, dtype=torch.int32, device=dev)
    _, p = _space_ptrs(queries, cand_vecs, cand_rows, cand_scores, cand_counts, work, od, orow, oc, pv)
    L.check(lib.rdx_space_rescore(dev.index, int(kind), p[0], nq, dim, p[1], p[2], p[3], p[4], int(kp), int(k), int(scale_exp),
                                  float(guard), p[5], p[6], p[7], p[8], p[9], ctypes.c_void_p(HipIndex._raw_stream(dev))))
    return od, orow, oc, pv


def space_distances(kind: int, queries, vecs, scale_exp: int, allow_bits, first_row: int, out, col0: int):
    """out[b][col0 + r] = distance(query b, engine row r of the page `vecs`), +inf where bit first_row + r of allow_bits is clear"""
    lib = L.load(require_gpu=True)
    nq, dim = queries.shape
    n = vecs.shape[0]
    if out.dim() != 2 or out.shape[0] != nq or col0 < 0 or col0 + n > out.shape[1]:
        raise ValueError("space_distances: the page does not fit the output")
    dev, p = _space_ptrs(queries, vecs, allow_bits, out)
    L.check(lib.rdx_space_distances(dev.index, int(kind), p[0], nq, dim, p[1], n, int(scale_exp), p[2], int(first_row),
                                    ctypes.c_void_p(out.data_ptr() + 4 * col0), out.shape[1], ctypes.c_void_p(HipIndex._raw_stream(dev))))


# ---- late-interaction scoring (include/rdx.h rdx_maxsim_f16, rdx_maxsim_quantize_i8, rdx_maxsim_i8; rag_dpo_amd/late_interaction.py drives it)
def maxsim(q_vecs, q_off, d_vecs, slot_start, slot_len, pair_q, pair_slot, scores=None, n_pairs: Optional[int] = None):
    """score(q, d) = (1 / n_q) sum_i max_j q_i . d_j for the listed pairs -> fp32 [n_pairs] on the device (written into `scores` when
    given). q_vecs fp16 [sum n_q][dim], d_vecs fp16 [rows][dim], slot_start i64 / slot_len i32 [slots], pair_q i32 / pair_slot i64
    [pairs]: contiguous torch tensors on one CUDA device; q_off int32 [nq + 1]: a PINNED host tensor, left unchanged until the stream
    has passed the call. Enqueued on the current torch stream, nothing synchronised."""
    import torch
    lib = L.load(require_gpu=True)
    _want_tensors("maxsim takes contiguous torch tensors of the documented types on one CUDA device", None, (q_vecs, torch.float16),
                  (d_vecs, torch.float16), (slot_start, torch.int64), (slot_len, torch.int32), (pair_q, torch.int32), (pair_slot, torch.int64))
    if q_vecs.dim() != 2 or d_vecs.dim() != 2 or q_vecs.shape[1] != d_vecs.shape[1] or slot_start.shape != slot_len.shape or pair_q.shape != pair_slot.shape:
        raise ValueError("maxsim: q_vecs / d_vecs must be [rows][dim] of one dim, the slot tables and the pair lists of one length each")
    if q_off.is_cuda or q_off.dtype != torch.int32 or not q_off.is_contiguous() or q_off.numel() < 2:
        raise ValueError("maxsim: q_off must be a contiguous int32 host tensor [nq + 1]")
    dev = q_vecs.device
    n = int(pair_q.numel()) if n_pairs is None else int(n_pairs)
    if scores is None:
        scores = torch.empty((n,), dtype=torch.float32, device=dev)
    _want_tensors("maxsim: scores must be a contiguous fp32 tensor on the vectors' device", dev.index, (scores, torch.float32))
    if n > pair_q.numel() or n > scores.numel() or int(q_off[-1]) > q_vecs.shape[0]:
        raise ValueError("maxsim: n_pairs exceeds the pair lists or the scores, or q_off reaches past q_vecs")
    p = _ptr
    L.check(lib.rdx_maxsim_f16(dev.index or 0, p(q_vecs), p(q_off), int(q_off.numel()) - 1, p(d_vecs), int(d_vecs.shape[0]), p(slot_start),
                               p(slot_len), int(slot_start.numel()), p(pair_q), p(pair_slot), n, int(q_vecs.shape[1]), p(scores),
                               ctypes.c_void_p(HipIndex._raw_stream(dev))))
    return scores


def maxsim_quantize(vecs, codes=None, scales=None):
    """per-token symmetric int8 (late_interaction.quantize_model): vecs fp16 [rows][dim], rows >= 1, a contiguous torch tensor on a
    CUDA device -> (codes int8 [rows][dim], scales fp32 [rows]) there (written into `codes` / `scales` when given). Enqueued on the
    current torch stream, nothing synchronised."""
    import torch
    lib = L.load(require_gpu=True)
    _want_tensors("maxsim_quantize takes a contiguous fp16 torch tensor [rows][dim] on a CUDA device", None, (vecs, torch.float16))
    if vecs.dim() != 2 or vecs.shape[0] < 1:
        raise ValueError("maxsim_quantize: vecs must be [rows][dim] with at least one row")
    dev, rows, dim = vecs.device, int(vecs.shape[0]), int(vecs.shape[1])
    codes = torch.empty((rows, dim), dtype=torch.int8, device=dev) if codes is None else codes
    scales = torch.empty((rows,), dtype=torch.float32, device=dev) if scales is None else scales
    _want_tensors("maxsim_quantize: codes / scales must be contiguous int8 / fp32 tensors on the vectors' device", dev.index,
                  (codes, torch.int8), (scales, torch.float32))
    if codes.numel() < rows * dim or scales.numel() < rows:
        raise ValueError("maxsim_quantize: codes or scales are too small for the rows")
    p = _ptr
    L.check(lib.rdx_maxsim_quantize_i8(dev.index or 0, p(vecs), rows, dim, p(codes), p(scales), ctypes.c_void_p(HipIndex._raw_stream(dev))))
    return codes, scales


def maxsim_i8(q_codes, q_scales, q_off, d_codes, d_scales, slot_start, slot_len, pair_q, pair_slot, scores=None, n_pairs: Optional[int] = None):
    """maxsim over quantised token vectors (late_interaction.maxsim_i8_model): q_codes int8 [sum n_q][dim] / q_scales fp32 [sum n_q],
    d_codes int8 [rows][dim] / d_scales fp32 [rows], the rest as maxsim takes it -> fp32 [n_pairs] on the device. Enqueued on the
    current torch stream, nothing synchronised."""
    import torch
    lib = L.load(require_gpu=True)
    _want_tensors("maxsim_i8 takes contiguous torch tensors of the documented types on one CUDA device", None, (q_codes, torch.int8),
                  (q_scales, torch.float32), (d_codes, torch.int8), (d_scales, torch.float32), (slot_start, torch.int64), (slot_len, torch.int32),
                  (pair_q, torch.int32), (pair_slot, torch.int64))
    if q_codes.dim() != 2 or d_codes.dim() != 2 or q_codes.shape[1] != d_codes.shape[1] or q_scales.shape != q_codes.shape[:1] or \
            d_scales.shape != d_codes.shape[:1] or slot_start.shape != slot_len.shape or pair_q.shape != pair_slot.shape:
        raise ValueError("maxsim_i8: codes must be [rows][dim] of one dim with one scale per row, the slot tables and the pair lists of one length each")
    if q_off.is_cuda or q_off.dtype != torch.int32 or not q_off.is_contiguous() or q_off.numel() < 2:
        raise ValueError("maxsim_i8: q_off must be a contiguous int32 host tensor [nq + 1]")
    dev = q_codes.device
    n = int(pair_q.numel()) if n_pairs is None else int(n_pairs)
    if scores is None:
        scores = torch.empty((n,), dtype=torch.float32, device=dev)
    _want_tensors("maxsim_i8: scores must be a contiguous fp32 tensor on the vectors' device", dev.index, (scores, torch.float32))
    if n > pair_q.numel() or n > scores.numel() or int(q_off[-1]) > q_codes.shape[0]:
        raise ValueError("maxsim_i8: n_pairs exceeds the pair lists or the scores, or q_off reaches past q_codes")
    p = _ptr
    L.check(lib.rdx_maxsim_i8(dev.index or 0, p(q_codes), p(q_scales), p(q_off), int(q_off.numel()) - 1, p(d_codes), p(d_scales),
                              int(d_codes.shape[0]), p(slot_start), p(slot_len), int(slot_start.numel()), p(pair_q), p(pair_slot), n,
                              int(q_codes.shape[1]), p(scores), ctypes.c_void_p(HipIndex._raw_stream(dev))))
    return scores


# ---- BGE-M3 lexical weights (include/rdx.h rdx_lex_reduce; rag_dpo_amd/lexical.py states the rule) ------------------------------
def lex_reduce(tok, w, off, vocab: int, skip_ids, out_tok=None, out_w=None, out_n=None):
    """the terms of every text: tok int32 [T], w fp32 [T] contiguous torch tensors on one CUDA device, off int64 [n + 1] a PINNED host
    tensor (left unchanged until the stream has passed the call) -> (out_tok int32 [T], out_w fp16 [T], out_n int32 [n]) on the device:
    text i's terms are out_*[off[i] : off[i] + out_n[i]], out_n[i] = -1 for a text with an id outside [0, vocab). Enqueued on the
    current torch stream, nothing synchronised. Outputs that are given are written in place (nothing of them is touched elsewhere)."""
    import torch
    lib = L.load(require_gpu=True)
    _want_tensors("lex_reduce takes contiguous torch tensors (tok int32, w fp32) on one CUDA device", None, (tok, torch.int32), (w, torch.float32))
    if tok.dim() != 1 or tok.shape != w.shape:
        raise ValueError("lex_reduce: tok and w must be [T] of one length")
    if off.is_cuda or off.dtype != torch.int64 or not off.is_contiguous() or off.dim() != 1 or off.numel() < 1:
        raise ValueError("lex_reduce: off must be a contiguous int64 host tensor [n + 1]")
    dev, n, T = tok.device, int(off.numel()) - 1, int(tok.numel())
    out_tok = torch.empty((T,), dtype=torch.int32, device=dev) if out_tok is None else out_tok
    out_w = torch.empty((T,), dtype=torch.float16, device=dev) if out_w is None else out_w
    out_n = torch.empty((n,), dtype=torch.int32, device=dev) if out_n is None else out_n
    _want_tensors("lex_reduce: the outputs must be contiguous (int32, fp16, int32) tensors on the tokens' device", dev.index,
                  (out_tok, torch.int32), (out_w, torch.float16), (out_n, torch.int32))
    if out_tok.numel() < T or out_w.numel() < T or out_n.numel() < n:
        raise ValueError("lex_reduce: an output is shorter than its input")
    skip = np.ascontiguousarray(list(skip_ids), dtype=np.int32)
    L.check(lib.rdx_lex_reduce(dev.index or 0, _ptr(tok), _ptr(w), T, _ptr(off), n, int(vocab), _np_ptr(skip), int(skip.shape[0]),
                               _ptr(out_tok), _ptr(out_w), _ptr(out_n), ctypes.c_void_p(HipIndex._raw_stream(dev))))
    return out_tok, out_w, out_n


# ---- grouped search (include/rdx.h rdx_group_select / rdx_index_group_fill; rag_dpo_amd/groups.py drives them) -----------------
def group_select(scores, rows, counts, row_group, group_off, n_groups: int, group_size: int):
    """ranked lists (scores f32 / rows i64 [nq][k], counts i32 [nq]) and the tables row_group i32 [n_rows], group_off i64 [groups + 1],
    all on one device -> dict of tensors there: score f32 / row i64 [nq][G][m], count / code / complete i32 [nq][G], found / short
    i32 [nq], bad i32 [1] (1 = a listed row or code lies outside the tables: the caller treats the call as failed). Enqueued on the
    current torch stream."""
    import torch
    lib = L.load(require_gpu=True)
    nq, k = rows.shape
    G, m = int(n_groups), int(group_size)
    dev = rows.device
    out = {"score": torch.empty((nq, G, m), dtype=torch.float32, device=dev), "row": torch.empty((nq, G, m), dtype=torch.int64, device=dev),
           "count": torch.empty((nq, G), dtype=torch.int32, device=dev), "code": torch.empty((nq, G), dtype=torch.int32, device=dev),
           "complete": torch.empty((nq, G), dtype=torch.int32, device=dev), "found": torch.empty(nq, dtype=torch.int32, device=dev),
           "short": torch.empty(nq, dtype=torch.int32, device=dev), "bad": torch.zeros(1, dtype=torch.int32, device=dev)}
    _want_tensors("group_select takes contiguous torch tensors of the documented types on one CUDA device", None, (scores, torch.float32),
                  (rows, torch.int64), (counts, torch.int32), (row_group, torch.int32), (group_off, torch.int64))
    if scores.shape != rows.shape or counts.shape != (nq,) or group_off.numel() < 1:
        raise ValueError("group_select: scores / rows must be [nq][k], counts [nq], group_off [groups + 1]")
    p = _ptr
    L.check(lib.rdx_group_select(dev.index or 0, p(scores), p(rows), p(counts), nq, int(k), p(row_group), row_group.numel(), p(group_off),
                                 group_off.numel() - 1, G, m, p(out["score"]), p(out["row"]), p(out["count"]), p(out["code"]),
                                 p(out["complete"]), p(out["found"]), p(out["short"]), p(out["bad"]),
                                 ctypes.c_void_p(HipIndex._raw_stream(dev))))
    return out


def group_fill(index: "HipIndex", queries, job_query, job_begin, job_end, group_rows, group_size: int, mask: Optional[ResidentMask] = None):
    """jobs (numpy: job_query i32, job_begin / job_end i64 into group_rows, spans of at most L.GROUP_FILL_SPAN) -> (score f32 [jobs][m],
    row i64 [jobs][m], count i32 [jobs]) on the device: each job's best m allowed rows by (exact score descending, row ascending).
    queries fp32 [nq][dim] and group_rows i64 are torch tensors on the index's device; complete on return."""
    import torch
    jq = np.ascontiguousarray(job_query, dtype=np.int32)
    jb = np.ascontiguousarray(job_begin, dtype=np.int64)
    je = np.ascontiguousarray(job_end, dtype=np.int64)
    n_jobs, m = jq.shape[0], int(group_size)
    if jb.shape != (n_jobs,) or je.shape != (n_jobs,):
        raise ValueError("group_fill: job_query, job_begin and job_end must have one entry per job")
    what = f"group_fill: queries must be a contiguous fp32 [nq][{index.dim}] tensor on cuda:{index.device}"
    _want_tensors(what, index.device, (queries, torch.float32))
    if queries.dim() != 2 or queries.shape[1] != index.dim:
        raise ValueError(what)
    _want_tensors("group_fill: group_rows must be a contiguous int64 tensor on the index's device", index.device, (group_rows, torch.int64))
    dev = queries.device
    sc = torch.empty((n_jobs, max(m, 1)), dtype=torch.float32, device=dev)
    ro = torch.empty((n_jobs, max(m, 1)), dtype=torch.int64, device=dev)
    cn = torch.empty(n_jobs, dtype=torch.int32, device=dev)
    p = _ptr
    L.check(index._lib.rdx_index_group_fill(index._h, p(queries), queries.shape[0], mask._h if mask is not None else None, _np_ptr(jq),
                                            _np_ptr(jb), _np_ptr(je), n_jobs, p(group_rows), group_rows.numel(), m, p(sc), p(ro), p(cn),
                                            ctypes.c_void_p(HipIndex._raw_stream(dev))))
    return sc, ro, cn


# ---- diversity-aware selection (include/rdx.h rdx_index_mmr; rag_dpo_amd/mmr.py states the definition) --------------------------
def mmr_select(index: "HipIndex", cand_score, cand_row, cand_count, n_results: int, lambda_mult: float):
    """candidate lists (cand_score f32 / cand_row i64 [nq][fetch_k], cand_count i32 [nq], torch tensors on the index's device; rows are the
    index's own) -> dict of tensors there, in pick order: pos i32 / row i64 / score f32 / value f64 [nq][k] (padding -1 / -1 / -inf / -inf),
    count i32 [nq], bad i32 [1] (1 = a listed row lies outside the index: it was skipped, the caller treats the call as failed).
    One launch enqueued on the current torch stream."""
    import torch
    nq, F = cand_row.shape
    k = int(n_results)
    dev = cand_row.device
    _want_tensors(f"mmr_select takes contiguous torch tensors of the documented types on cuda:{index.device}", index.device,
                  (cand_score, torch.float32), (cand_row, torch.int64), (cand_count, torch.int32))
    if cand_score.shape != cand_row.shape or cand_count.shape != (nq,):
        raise ValueError("mmr_select: cand_score / cand_row must be [nq][fetch_k], cand_count [nq]")
    kk = max(k, 1)
    out = {"pos": torch.empty((nq, kk), dtype=torch.int32, device=dev), "row": torch.empty((nq, kk), dtype=torch.int64, device=dev),
           "score": torch.empty((nq, kk), dtype=torch.float32, device=dev), "value": torch.empty((nq, kk), dtype=torch.float64, device=dev),
           "count": torch.empty(nq, dtype=torch.int32, device=dev), "bad": torch.zeros(1, dtype=torch.int32, device=dev)}
    p = _ptr
    L.check(index._lib.rdx_index_mmr(index._h, p(cand_score), p(cand_row), p(cand_count), nq, int(F), k, float(lambda_mult), p(out["pos"]),
                                     p(out["row"]), p(out["score"]), p(out["value"]), p(out["count"]), p(out["bad"]),
                                     ctypes.c_void_p(HipIndex._raw_stream(dev))))
    return out


# ---- the combined BGE-M3 score (include/rdx.h rdx_index_score_pairs / rdx_lex_score_pairs / rdx_m3_combine; rag_dpo_amd/m3.py) -------
def score_pairs(index: "HipIndex", queries, pair_q, pair_row, out=None):
    """the exact search score of each named pair: queries fp32 [nq][dim] (raw), pair_q int32 [n], pair_row int64 [n] (the index's own
    rows) as contiguous torch tensors on the index's device -> fp32 [n] there; NaN for a pair out of range. One launch enqueued on the
    current torch stream, nothing synchronised."""
    import torch
    what = f"score_pairs: queries must be a contiguous fp32 [nq][{index.dim}] tensor on cuda:{index.device}"
    _want_tensors(what, index.device, (queries, torch.float32))
    if queries.dim() != 2 or queries.shape[1] != index.dim:
        raise ValueError(what)
    _want_tensors("score_pairs: pair_q int32 and pair_row int64 must be contiguous tensors on the index's device", index.device,
                  (pair_q, torch.int32), (pair_row, torch.int64))
    if pair_q.dim() != 1 or pair_q.shape != pair_row.shape:
        raise ValueError("score_pairs: pair_q and pair_row must be [n] of one length")
    n = int(pair_q.numel())
    out = torch.empty((n,), dtype=torch.float32, device=queries.device) if out is None else out
    _want_tensors("score_pairs: out must be a contiguous fp32 tensor on the index's device", index.device, (out, torch.float32))
    if out.numel() < n:
        raise ValueError("score_pairs: out is shorter than the pair lists")
    p = _ptr
    L.check(index._lib.rdx_index_score_pairs(index._h, p(queries), int(queries.shape[0]), p(pair_q), p(pair_row), n, p(out),
                                             ctypes.c_void_p(HipIndex._raw_stream(queries.device))))
    return out


def lex_score_pairs(lex, term_off, term_ids, term_w, pair_q, pair_row, out=None):
    """the lexical score of each named pair over a HipLexical: term_ids int32 / term_w fp16 (or its uint16 bits' int16 view) and pair_q
    int32 / pair_row int64 [n] as contiguous torch tensors on the index's device, term_off int64 [nq + 1] a PINNED host tensor (left
    unchanged until the stream has passed the call) -> f64 [n] on the device; NaN for a pair out of range or of a bad question. One
    launch enqueued on the current torch stream, nothing synchronised."""
    import torch
    if term_off.is_cuda or term_off.dtype != torch.int64 or not term_off.is_contiguous() or term_off.dim() != 1 or term_off.numel() < 2:
        raise ValueError("lex_score_pairs: term_off must be a contiguous int64 host tensor [nq + 1]")
    _want_tensors("lex_score_pairs: pair_q int32 and pair_row int64 must be contiguous tensors on the index's device", lex.device,
                  (pair_q, torch.int32), (pair_row, torch.int64))
    if term_w.dtype not in (torch.float16, torch.int16, torch.uint16):
        raise ValueError("lex_score_pairs: term_w must hold fp16 values or their 16-bit patterns")
    _want_tensors("lex_score_pairs: term_ids int32 and term_w must be contiguous tensors on the index's device", lex.device,
                  (term_ids, torch.int32), (term_w, term_w.dtype))
    if pair_q.dim() != 1 or pair_q.shape != pair_row.shape or term_ids.dim() != 1 or term_ids.shape != term_w.shape:
        raise ValueError("lex_score_pairs: pair_q / pair_row and term_ids / term_w must be lists of one length each")
    if int(term_off[-1]) > term_ids.numel():
        raise ValueError("lex_score_pairs: term_off reaches past term_ids")
    n, dev = int(pair_q.numel()), pair_q.device
    out = torch.empty((n,), dtype=torch.float64, device=dev) if out is None else out
    _want_tensors("lex_score_pairs: out must be a contiguous f64 tensor on the index's device", lex.device, (out, torch.float64))
    if out.numel() < n:
        raise ValueError("lex_score_pairs: out is shorter than the pair lists")
    p = _ptr
    L.check(lex._lib.rdx_lex_score_pairs(lex._h, p(term_off), p(term_ids), p(term_w), int(term_off.numel()) - 1, p(pair_q), p(pair_row), n,
                                         p(out), ctypes.c_void_p(HipIndex._raw_stream(dev))))
    return out


def m3_combine(dense, sparse, colbert, weights, want_value: bool = False):
    """value = ((w_d dense + w_s sparse) + w_c colbert) / W per element (rag_dpo_amd/m3.py combine_model): dense fp32 / sparse f64 /
    colbert fp32 [n] contiguous torch tensors on one CUDA device, each None exactly when its weight is 0 -> final fp32 [n] there, or
    (final, value f64 [n]) with want_value. One launch enqueued on the current torch stream, nothing synchronised."""
    import torch
    lib = L.load(require_gpu=True)
    given = [(t, dt) for t, dt in ((dense, torch.float32), (sparse, torch.float64), (colbert, torch.float32)) if t is not None]
    if not given:
        raise ValueError("m3_combine: no component given")
    _want_tensors("m3_combine takes contiguous torch tensors (dense fp32, sparse f64, colbert fp32) on one CUDA device", None, *given)
    n, dev = int(given[0][0].numel()), given[0][0].device
    if any(t.dim() != 1 or t.numel() != n for t, _ in given):
        raise ValueError("m3_combine: the components must be [n] of one length")
    final = torch.empty((n,), dtype=torch.float32, device=dev)
    value = torch.empty((n,), dtype=torch.float64, device=dev) if want_value else None
    w = [float(x) for x in weights]
    p = _ptr
    L.check(lib.rdx_m3_combine(dev.index or 0, p(dense), p(sparse), p(colbert), n, w[0], w[1], w[2], p(final), p(value),
                               ctypes.c_void_p(HipIndex._raw_stream(dev))))
    return (final, value) if want_value else final


# ---- threshold search (include/rdx.h rdx_index_range; rag_dpo_amd/range_search.py states the definition) ------------------------
def range_search(index: "HipIndex", queries, thresholds, max_results: int, mask: Optional[ResidentMask] = None):
    """queries fp32 [nq][dim] and thresholds fp32 [nq] (score thresholds t, range_search.score_threshold) as contiguous torch tensors on
    the index's device -> (scores f32 [nq][m], rows i64 [nq][m], counts i32 [nq], totals i64 [nq]) there and paths = [queries answered
    by the MFMA path, by the exact scan] (a host list): per query the allowed rows with score >= t, counted exactly, the best m =
    max_results of them in a search's order, padding -inf / -1. Enqueued on the current torch stream, complete on return."""
    import torch
    m = int(max_results)
    dev = queries.device
    _want_tensors(f"range_search takes contiguous fp32 torch tensors on cuda:{index.device}", index.device, (queries, torch.float32),
                  (thresholds, torch.float32))
    if queries.dim() != 2 or queries.shape[1] != index.dim:
        raise ValueError(f"range_search: queries must be [nq][{index.dim}]")
    nq = int(queries.shape[0])
    if thresholds.shape != (nq,):
        raise ValueError("range_search: thresholds must be [nq]")
    mm = max(m, 1)
    sc = torch.empty((nq, mm), dtype=torch.float32, device=dev)
    ro = torch.empty((nq, mm), dtype=torch.int64, device=dev)
    cn = torch.empty(nq, dtype=torch.int32, device=dev)
    tt = torch.empty(nq, dtype=torch.int64, device=dev)
    paths = (ctypes.c_int32 * 2)(0, 0)
    p = _ptr
    L.check(index._lib.rdx_index_range(index._h, p(queries), nq, p(thresholds), m, mask._h if mask is not None else None, p(sc), p(ro),
                                       p(cn), p(tt), paths, ctypes.c_void_p(HipIndex._raw_stream(dev))))
    return sc, ro, cn, tt, [int(paths[0]), int(paths[1])]


# ---- near-duplicate clustering (include/rdx.h rdx_index_near_dup; rag_dpo_amd/dedup.py states the definition) ---------------------
def near_dup(index: "HipIndex", t, mask: Optional[ResidentMask] = None, list_cap: int = 1024, max_dense: int = 4096):
    """-> (labels i64 [rows], totals i64 [rows]) on the index's device and stats = [allowed rows examined, rows linked from their
    lists, rows linked by the dense pass, batches] (a host list): the connected components of "allowed row j scores >= t against the
    stored row i", labelled by their smallest row (-1: not allowed), and per row the number of rows in range (0: not allowed).
    Enqueued on the current torch stream, complete on return. ValueError: a NaN t, list_cap outside [1, RANGE_MAX_RESULTS], more
    than max_dense rows with more than list_cap rows in range (the distance is too loose for duplicate detection)."""
    import torch
    dev = torch.device("cuda", index.device)
    n = len(index)
    lab = torch.empty(n, dtype=torch.int64, device=dev)
    tot = torch.empty(n, dtype=torch.int64, device=dev)
    stats = (ctypes.c_int64 * 4)(0, 0, 0, 0)
    p = lambda x: _ptr(x) if n else None   # noqa: E731  (no rows: null pointers)
    with torch.cuda.device(dev):
        L.check(index._lib.rdx_index_near_dup(index._h, ctypes.c_float(float(t)), mask._h if mask is not None else None, int(list_cap),
                                              int(max_dense), p(lab), p(tot), stats, ctypes.c_void_p(HipIndex._raw_stream(dev))))
    return lab, tot, [int(x) for x in stats]


# ---- k-means of the stored rows (include/rdx.h rdx_index_kmeans; rag_dpo_amd/kmeans.py states the definition) -------------------
def kmeans(index: "HipIndex", init, max_iter: int, mask: Optional[ResidentMask] = None):
    """init fp32 [K][dim], a contiguous torch tensor on the index's device -> (labels i64 [rows], scores f32 [rows], centroids f32
    [K][dim], counts i64 [K]) there and n_iter, converged on the host: spherical k-means of the allowed rows from the centroids
    K1(init), at most max_iter updates. Enqueued on the current torch stream, complete on return. ValueError: K outside
    [1, KMEANS_MAX_CLUSTERS], max_iter outside [0, KMEANS_MAX_ITER], an empty index, a NaN or Inf in init."""
    import torch
    _want_tensors(f"kmeans: init must be a contiguous fp32 [K][{index.dim}] tensor on cuda:{index.device}", index.device, (init, torch.float32))
    if init.dim() != 2 or init.shape[1] != index.dim:
        raise ValueError(f"kmeans: init must be [K][{index.dim}]")
    dev = init.device
    n, K = len(index), int(init.shape[0])
    lab = torch.empty(n, dtype=torch.int64, device=dev)
    sc = torch.empty(n, dtype=torch.float32, device=dev)
    cen = torch.empty((max(K, 1), index.dim), dtype=torch.float32, device=dev)
    cnt = torch.empty(max(K, 1), dtype=torch.int64, device=dev)
    info = (ctypes.c_int32 * 2)(0, 0)
    p = _ptr
    with torch.cuda.device(dev):
        L.check(index._lib.rdx_index_kmeans(index._h, p(init), K, int(max_iter), mask._h if mask is not None else None, p(lab), p(sc), p(cen),
                                            p(cnt), info, ctypes.c_void_p(HipIndex._raw_stream(dev))))
    return lab, sc, cen, cnt, int(info[0]), bool(info[1])


# ---- value counts (include/rdx.h rdx_index_facet_count / rdx_index_range_facets; rag_dpo_amd/facets.py states the definitions) ----
def facet_count(index: "HipIndex", row_group=None, n_groups: int = 0, mask: Optional[ResidentMask] = None):
    """row_group i32 [rows] (a contiguous torch tensor on the index's device: -1 or a code < n_groups; None with n_groups = 0: no table)
    -> (counts i64 [n_groups] on the device, missing, total): the allowed rows per code, those without a code, and their number.
    Enqueued on the current torch stream, complete on return. ValueError: a code outside the table's range."""
    import torch
    dev = torch.device("cuda", index.device)
    G = int(n_groups)
    if row_group is not None:
        _want_tensors(f"facet_count: row_group must be a contiguous int32 [rows] tensor on cuda:{index.device}", index.device, (row_group, torch.int32))
        if row_group.shape != (len(index),):
            raise ValueError("facet_count: row_group must hold one code per row of the index")
    elif G:
        raise ValueError("facet_count: n_groups > 0 needs row_group")
    counts = torch.empty(G, dtype=torch.int64, device=dev)
    missing, total = ctypes.c_int64(0), ctypes.c_int64(0)
    with torch.cuda.device(dev):
        L.check(index._lib.rdx_index_facet_count(index._h, mask._h if mask is not None else None, _ptr(row_group) if G else None, G,
                                                 _ptr(counts) if G else None, ctypes.byref(missing), ctypes.byref(total),
                                                 ctypes.c_void_p(HipIndex._raw_stream(dev))))
    return counts, int(missing.value), int(total.value)


def range_facets(index: "HipIndex", queries, thresholds, row_group, n_groups: int, limit: int, mask: Optional[ResidentMask] = None):
    """queries fp32 [nq][dim], thresholds fp32 [nq] (score thresholds, as range_search takes them) and row_group i32 [rows] as contiguous
    torch tensors on the index's device -> (codes i32 [nq][limit], counts i64 [nq][limit], n_values i32 [nq], missing i64 [nq], totals i64
    [nq]) there and paths (a host list, range_search's): per query the rows in range counted by code, the best `limit` codes by (count
    descending, code ascending), padding -1 / 0. Enqueued on the current torch stream, complete on return."""
    import torch
    dev = queries.device
    _want_tensors(f"range_facets takes contiguous fp32 torch tensors on cuda:{index.device}", index.device, (queries, torch.float32),
                  (thresholds, torch.float32))
    _want_tensors(f"range_facets: row_group must be a contiguous int32 [rows] tensor on cuda:{index.device}", index.device, (row_group, torch.int32))
    if queries.dim() != 2 or queries.shape[1] != index.dim:
        raise ValueError(f"range_facets: queries must be [nq][{index.dim}]")
    nq = int(queries.shape[0])
    if thresholds.shape != (nq,):
        raise ValueError("range_facets: thresholds must be [nq]")
    if row_group.shape != (len(index),):
        raise ValueError("range_facets: row_group must hold one code per row of the index")
    m = int(limit)
    mm = max(m, 1)
    code = torch.empty((nq, mm), dtype=torch.int32, device=dev)
    cnt = torch.empty((nq, mm), dtype=torch.int64, device=dev)
    found = torch.empty(nq, dtype=torch.int32, device=dev)
    mis = torch.empty(nq, dtype=torch.int64, device=dev)
    tot = torch.empty(nq, dtype=torch.int64, device=dev)
    paths = (ctypes.c_int32 * 2)(0, 0)
    p = _ptr
    L.check(index._lib.rdx_index_range_facets(index._h, p(queries), nq, p(thresholds), mask._h if mask is not None else None, p(row_group),
                                              int(n_groups), m, p(code), p(cnt), p(found), p(mis), p(tot), paths,
                                              ctypes.c_void_p(HipIndex._raw_stream(dev))))
    return code, cnt, found, mis, tot, [int(paths[0]), int(paths[1])]


def l2_normalize(x: np.ndarray, device: int = 0) -> np.ndarray:
    lib = L.load(require_gpu=True)
    a = np.ascontiguousarray(x, dtype=np.float32)
    if a.ndim != 2:
        raise ValueError("l2_normalize wants [n][dim]")
    out = np.empty_like(a)
    L.check(lib.rdx_l2_normalize(device, _np_ptr(a), a.shape[0], a.shape[1], _np_ptr(out), L.RDX_HOST, None))
    return out


def merge_topk_device(part_score, part_row, part_count, k: int, out_score, out_row, out_count):
    """rdx_merge_topk on torch CUDA tensors ([P][nq][k], [P][nq][k], [P][nq] on ONE device), enqueued on that device's current
    torch stream; any P * k (the library folds the parts pairwise beyond what one merge launch ranks)"""
    lib = L.load(require_gpu=True)
    P, nq = part_count.shape
    dev = part_score.device
    assert part_score.is_contiguous() and part_row.is_contiguous() and part_count.is_contiguous()
    stream = HipIndex._raw_stream(dev)
    p = _ptr
    L.check(lib.rdx_merge_topk(dev.index or 0, p(part_score), p(part_row), p(part_count), int(P), int(nq), int(k),
                               p(out_score), p(out_row), p(out_count), L.RDX_DEVICE, ctypes.c_void_p(stream)))


def merge_topk(part_score: np.ndarray, part_row: np.ndarray, part_count: np.ndarray, k: int, device: int = 0):
    lib = L.load(require_gpu=True)
    ps = np.ascontiguousarray(part_score, dtype=np.float32)
    pr = np.ascontiguousarray(part_row, dtype=np.int64)
    pc = np.ascontiguousarray(part_count, dtype=np.int32)
    P, nq = pc.shape
    sc = np.empty((nq, k), dtype=np.float32)
    ro = np.empty((nq, k), dtype=np.int64)
    cn = np.empty((nq,), dtype=np.int32)
    L.check(lib.rdx_merge_topk(device, _np_ptr(ps), _np_ptr(pr), _np_ptr(pc), P, nq, int(k),
                               _np_ptr(sc), _np_ptr(ro), _np_ptr(cn), L.RDX_HOST, None))
    return sc, ro, cn
