"""Chroma's `where_document` filter: validation, compilation to the librdx document-store program, and a host evaluator.

Grammar (chromadb 1.x `validate_where_document`): exactly one operator per dict;
    {"$contains": str} / {"$not_contains": str}     a non-empty str operand
    {"$and": [expr, expr, ...]} / {"$or": [...]}      a list of at least two expressions, nested to any depth
`$regex` / `$not_regex` are valid in Chroma 1.x and refused here (not implemented). `{}` (and None) means no filter.
Size limits, the same on every engine: at most 1024 distinct patterns, 4096 compiled operations and 16 stack entries (an $and /
$or nesting of about 15 levels); a larger tree raises ValueError.

Match rule: case-sensitive, byte-exact substring of the UTF-8 text (`errors="surrogatepass"`, so every str has bytes) — exactly
Python's `needle in document`, UTF-8 being self-synchronising. A row without a document, or with "", contains nothing;
`$not_contains` is the complement of `$contains` over the live rows, so such rows match it. That is how Chroma's
`NOT IN (subquery)` behaves as far as we know; chromadb is not a dependency, so it is a decision, not verified parity.

`compile_tree` turns a tree into (leaf patterns, postfix program) for include/rdx.h rdx_docs_set_query; `evaluate_host` is the
path of engines without a device document store.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from ._lib import MAX_OPS, MAX_STACK, OP_AND, OP_NOT, OP_OR   # the program format, shared with where_device.py

MAX_LEAVES = 1024

_LEAF_OPS = ("$contains", "$not_contains")
_BOOL_OPS = ("$and", "$or")


def encode(s: str) -> bytes:
    return s.encode("utf-8", errors="surrogatepass")


def is_empty(where_document) -> bool:
    return where_document is None or (isinstance(where_document, dict) and len(where_document) == 0)


def validate(where_document) -> None:
    """grammar and size limits (raises ValueError); every engine applies both"""
    _grammar(where_document)
    _compile(where_document)


def _grammar(where_document) -> None:
    if not isinstance(where_document, dict):
        raise ValueError(f"Expected where_document to be a dict, got {where_document!r}")
    if len(where_document) != 1:
        raise ValueError(f"Expected where_document to have exactly one operator, got {where_document!r}")
    (op, val), = where_document.items()
    if op in ("$regex", "$not_regex"):
        raise ValueError(f"where_document operator {op} is not implemented (only $contains, $not_contains, $and, $or)")
    if op in _LEAF_OPS:
        if not isinstance(val, str) or not val:
            raise ValueError(f"Expected where_document operand of {op} to be a non-empty str, got {val!r}")
        return
    if op in _BOOL_OPS:
        if not isinstance(val, list) or len(val) < 2:
            raise ValueError(f"Expected where_document value for {op} to be a list with at least two expressions, got {val!r}")
        for sub in val:
            _grammar(sub)
        return
    raise ValueError(f"Expected where_document operator to be one of $contains, $not_contains, $and, $or, got {op!r}")


def compile_tree(where_document) -> Tuple[List[bytes], List[int]]:
    """-> (leaf patterns as UTF-8 bytes, identical ones shared; postfix program). An n-ary $and / $or becomes a left chain of
    binary ops, so the stack holds at most depth + 1 entries."""
    _grammar(where_document)
    return _compile(where_document)


def _compile(where_document) -> Tuple[List[bytes], List[int]]:
    leaves: List[bytes] = []
    index = {}
    prog: List[int] = []
    depth = [0, 0]   # current, max

    def push(n):
        depth[0] += n
        depth[1] = max(depth[1], depth[0])

    def walk(t):
        (op, val), = t.items()
        if op in _LEAF_OPS:
            b = encode(val)
            if b not in index:
                index[b] = len(leaves)
                leaves.append(b)
            prog.append(index[b])
            push(1)
            if op == "$not_contains":
                prog.append(OP_NOT)
            return
        code = OP_AND if op == "$and" else OP_OR
        walk(val[0])
        for sub in val[1:]:
            walk(sub)
            prog.append(code)
            push(-1)

    walk(where_document)
    if depth[1] > MAX_STACK or len(prog) > MAX_OPS or len(leaves) > MAX_LEAVES:
        raise ValueError(f"where_document is too large: {len(leaves)} patterns, {len(prog)} operations, nesting {depth[1]} "
                         f"(at most {MAX_LEAVES}, {MAX_OPS}, {MAX_STACK})")
    return leaves, prog


def pack_patterns(leaves: Sequence[bytes]) -> Tuple[np.ndarray, np.ndarray]:
    """-> (uint8 bytes, int64 offsets[P + 1]) as rdx_docs_set_query takes them"""
    off = np.zeros(len(leaves) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(b) for b in leaves])
    return np.frombuffer(b"".join(leaves), dtype=np.uint8).copy(), off


def pack_docs(docs: Sequence) -> Tuple[np.ndarray, np.ndarray]:
    """documents (str, raw bytes, or None = no text) -> (uint8 bytes, int64 offsets[n + 1]) as rdx_docs_append / _replace
    take them"""
    enc = [d if isinstance(d, bytes) else (encode(d) if d else b"") for d in docs]
    off = np.zeros(len(enc) + 1, dtype=np.int64)
    if enc:
        off[1:] = np.cumsum([len(b) for b in enc])
    return np.frombuffer(b"".join(enc), dtype=np.uint8).copy(), off


def evaluate_host(where_document, docs: Sequence[Optional[str]]) -> np.ndarray:
    """-> bool[len(docs)]: the rows whose document satisfies the tree (same rule as the device store)"""
    validate(where_document)
    n = len(docs)
    memo = {}

    def contains(s: str) -> np.ndarray:
        if s not in memo:
            memo[s] = np.fromiter((d is not None and s in d for d in docs), dtype=bool, count=n)
        return memo[s]

    def ev(t) -> np.ndarray:
        (op, val), = t.items()
        if op == "$contains":
            return contains(val)
        if op == "$not_contains":
            return ~contains(val)
        parts = [ev(sub) for sub in val]
        out = parts[0].copy()
        for p in parts[1:]:
            out = (out & p) if op == "$and" else (out | p)
        return out

    return ev(where_document)
