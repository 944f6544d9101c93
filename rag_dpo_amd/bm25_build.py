"""Building a BM25 index from text on the GPU: the byte-level statement of `tokenize_french`, and the builder that drives
include/rdx.h rdx_bm25_build_* (csrc/bm25_build_kernel.hpp). The index is bit for bit the one `Bm25Model(corpus_tokens)` builds.

The tokenizer as a rule over UTF-8 bytes. `tokenize_french` is text.lower(), a regex over a fixed character class, and two filters.
Exactly 98 code points have a lowercase form that touches the class — the word characters W:
    0-9 a-z, à â ä ç é è ê ë î ï ô ù û ü ÿ æ œ        their own lowercase (53)
    A-Z                                               byte + 0x20
    À Â Ä Æ Ç È É Ê Ë Î Ï Ô Ù Û Ü  (C3 80..9C)        second byte + 0x20
    Œ (C5 92) -> œ (C5 93);  Ÿ (C5 B8) -> ÿ (C3 BF);  the Kelvin sign U+212A (E2 84 AA) -> k
    İ U+0130 (C4 B0) -> i, followed by U+0307, which is outside the class: the word character i with a forced break after it
Lowering is per character for every code point, and every other character is a separator whatever its case. A token is a maximal
run of W characters and joining hyphens; a hyphen joins when the characters before and after it are both W (the break after İ
counts as a non-W). A token is kept when it has more than one CHARACTER and its normalised bytes are not a stop word.

`tokenize_utf8` states this in plain Python (no `re`, no `lower()`, only the byte tables) the way the kernel does it: a position
starts a token by looking one character behind (two across a hyphen), and a token is walked one character at a time from its
start. tests/test_bm25_build_model.py holds it against `tokenize_french` over every code point; the device tests compare the
kernel against it.
"""
from __future__ import annotations

import ctypes
import time
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib as L
from .bm25 import MAX_TF, STOPWORDS, Bm25Model

# second bytes b of the two-byte word characters C3 b, as bits of (b - 0xA0): à â ä æ ç è é ê ë î ï ô ù û ü ÿ. The capitals are
# the same bits at (b - 0x80), except bit 31: C3 9F is ß, which is its own lowercase and not in the class
C3_LOWER = sum(1 << (b - 0xA0) for b in (0xA0, 0xA2, 0xA4, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xAB, 0xAE, 0xAF, 0xB4, 0xB9, 0xBB, 0xBC, 0xBF))
C3_UPPER = C3_LOWER & 0x7FFFFFFF

STOPWORD_BYTES = frozenset(w.encode("utf-8") for w in STOPWORDS)
_LEADS = frozenset(b"0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ\xc3\xc4\xc5\xe2")   # first bytes of W characters


def word_char(d: bytes, p: int) -> Optional[Tuple[int, bytes, bool]]:
    """the word character that starts at d[p] -> (bytes it takes, its normalised bytes, forced break after it), or None.
    A continuation byte (80..BF) never starts one, so any byte position may be asked. Reads past the end see a NUL."""
    n = len(d)
    b0 = d[p] if p < n else 0
    if b0 < 0x80:
        if 0x30 <= b0 <= 0x39 or 0x61 <= b0 <= 0x7A:
            return 1, d[p:p + 1], False
        if 0x41 <= b0 <= 0x5A:
            return 1, bytes((b0 + 0x20,)), False
        return None
    b1 = d[p + 1] if p + 1 < n else 0
    if b0 == 0xC3:
        if 0xA0 <= b1 <= 0xBF and C3_LOWER >> (b1 - 0xA0) & 1:
            return 2, d[p:p + 2], False
        if 0x80 <= b1 <= 0x9F and C3_UPPER >> (b1 - 0x80) & 1:
            return 2, bytes((0xC3, b1 + 0x20)), False
        return None
    if b0 == 0xC5:
        if b1 == 0x92 or b1 == 0x93:
            return 2, b"\xc5\x93", False
        if b1 == 0xB8:
            return 2, b"\xc3\xbf", False
        return None
    if b0 == 0xC4:
        return (2, b"i", True) if b1 == 0xB0 else None
    if b0 == 0xE2 and b1 == 0x84 and p + 2 < n and d[p + 2] == 0xAA:
        return 3, b"k", False
    return None


def word_ends_at(d: bytes, q: int) -> bool:
    """does a word character WITHOUT a forced break end just before d[q]? (the kernel's look-behind; never reads before d[0])"""
    if q >= 1:
        b = d[q - 1]
        if b < 0x80:
            return 0x30 <= b <= 0x39 or 0x61 <= b <= 0x7A or 0x41 <= b <= 0x5A
        if q >= 2 and d[q - 2] in (0xC3, 0xC5):
            return word_char(d, q - 2) is not None
        if q >= 3 and d[q - 3] == 0xE2:
            return word_char(d, q - 3) is not None
    return False


def starts_token(d: bytes, p: int) -> bool:
    """a word character starts at d[p], none ends just before it, and no joining hyphen stands between it and one"""
    return (word_char(d, p) is not None and not word_ends_at(d, p)
            and not (p >= 1 and d[p - 1] == 0x2D and word_ends_at(d, p - 1)))


def walk_token(d: bytes, p: int) -> Tuple[bytes, int, int]:
    """from a token start -> (normalised bytes, characters, position after the token)"""
    out, chars = [], 0
    while True:
        take, norm, brk = word_char(d, p)
        out.append(norm)
        chars += 1
        p += take
        if brk:
            break
        if word_char(d, p) is not None:
            continue
        if p < len(d) and d[p] == 0x2D and word_char(d, p + 1) is not None:
            out.append(b"-")
            chars += 1
            p += 1
            continue
        break
    return b"".join(out), chars, p


def tokenize_utf8(data: bytes) -> List[bytes]:
    """== [t.encode() for t in tokenize_french(data.decode())], by the byte rule of this module's docstring"""
    out = []
    for p, b0 in enumerate(data):
        if b0 in _LEADS and starts_token(data, p):
            tok, chars, _ = walk_token(data, p)
            if chars > 1 and tok not in STOPWORD_BYTES:
                out.append(tok)
    return out


def stopword_keys() -> List[int]:
    """the stop words of more than one character as the kernel tests them: the normalised bytes packed little-endian into
    64 bits (none is longer than 8 bytes), ascending. csrc/bm25_build_kernel.hpp BM25_STOPWORDS must be this list."""
    words = [w for w in STOPWORD_BYTES if len(w.decode("utf-8")) > 1]
    assert all(len(w) <= 8 for w in words)
    return sorted(int.from_bytes(w, "little") for w in words)


# ------------------------------------------------------------------------------------------------
# the builder
# ------------------------------------------------------------------------------------------------
MAX_ROWS = 2 ** 31 - 1      # csrc/bm25_build_kernel.hpp: rows, bytes of one row and terms of one build
MAX_ROW_BYTES = 2 ** 32 - 1
HASH_MASK_ALL = 2 ** 64 - 1


class DeviceBm25Builder:
    """Builds a Bm25Model from texts on one GPU. torch (on the index's device) is plumbing: uploads, one sort, scans and
    run lengths over integer keys. Tokenising and the term table are HIP (k_bm25_tok, k_bm25_vocab); the statistics that reach
    a score are computed on the host by Bm25Model.from_postings with the expressions of Bm25Model.__init__.

    table_slots: size of the first term table (a power of two; a slot is 16 bytes). A build whose vocabulary fills more than half
    of it starts over with a table 4x larger — the text stays on the device — and raises RuntimeError beyond max_slots.
    hash_mask is ANDed onto a token's hash before its slot is chosen: all ones in production, a few bits in tests that force
    every token into a few probe chains. `timings` holds the seconds of the last build's stages."""

    def __init__(self, device: int = 0, table_slots: int = 1 << 20, max_slots: int = 1 << 30, hash_mask: int = HASH_MASK_ALL,
                 batch_rows: int = 1 << 18, batch_bytes: int = 1 << 28):
        for name, v in (("table_slots", table_slots), ("max_slots", max_slots)):
            if v < 2 or v & (v - 1):
                raise ValueError(f"{name} must be a power of two >= 2 (got {v})")
        if batch_rows < 1 or batch_bytes < 1:
            raise ValueError("batch_rows and batch_bytes must be positive")
        self._lib = L.load(require_gpu=True)
        self.device = int(device)
        self.table_slots, self.max_slots, self.hash_mask = int(table_slots), int(max_slots), int(hash_mask)
        self.batch_rows, self.batch_bytes = int(batch_rows), int(batch_bytes)
        self.timings: Dict[str, float] = {}
        self.retries = 0

    def _batches(self, texts: Sequence[Optional[str]]):
        """-> [(first row, concatenated bytes with one NUL after each row, row_off int64 [rows + 1])]; raises UnicodeEncodeError"""
        out, rows, size, first = [], [], 0, 0
        for i, t in enumerate(texts):
            b = t.encode("utf-8") if t else b""
            if len(b) > MAX_ROW_BYTES:
                raise ValueError(f"text {i} has {len(b)} bytes: a row of a device-built BM25 index holds less than 4 GiB")
            if rows and (len(rows) >= self.batch_rows or size + len(b) + 1 > self.batch_bytes):
                out.append((first, rows))
                first, rows, size = i, [], 0
            rows.append(b)
            size += len(b) + 1
        if rows:
            out.append((first, rows))
        packed = []
        for first, rows in out:
            off = np.zeros(len(rows) + 1, np.int64)
            np.cumsum(np.fromiter(map(len, rows), np.int64, len(rows)) + 1, out=off[1:])
            packed.append((first, b"\0".join(rows) + b"\0", off))
        return packed

    def _tokenize(self, torch, dev, slots, uploaded, n_rows):
        """one pass of k_bm25_tok over every batch with a table of `slots` -> (handle, keys, doc_len, (terms, tokens, full))"""
        h = ctypes.c_void_p()
        L.check(self._lib.rdx_bm25_build_create(self.device, slots, ctypes.c_uint64(self.hash_mask), ctypes.byref(h)))
        try:
            stream = ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(self.device))
            keys, lens = [], []
            for first, text, off in uploaded:
                n = off.shape[0] - 1
                cap = int((np.diff(off) // 3).sum())      # a row of len bytes (+ its NUL) keeps at most (len + 1) / 3 tokens
                k = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
                dl = torch.empty(n, dtype=torch.int32, device=dev)
                L.check(self._lib.rdx_bm25_build_tokenize(h, ctypes.c_void_p(text.data_ptr()), int(text.numel()),
                                                          ctypes.c_void_p(off.ctypes.data), n, first, ctypes.c_void_p(k.data_ptr()),
                                                          cap, ctypes.c_void_p(dl.data_ptr()), stream))
                keys.append(k[:cap][k[:cap] >= 0])      # the kept tokens' keys; the rest of each row's stretch holds -1
                lens.append(dl)
            terms, tokens, full = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32()
            L.check(self._lib.rdx_bm25_build_stats(h, ctypes.byref(terms), ctypes.byref(tokens), ctypes.byref(full)))
        except BaseException:
            self._lib.rdx_bm25_build_destroy(h)
            raise
        return h, torch.cat(keys), torch.cat(lens), (terms.value, tokens.value, bool(full.value))

    def build(self, texts: Sequence[Optional[str]]) -> Tuple[np.ndarray, Bm25Model]:
        """-> (kept, model): `kept` are the indexes (ascending, int64) of the texts that have a token — None, empty and blank
        texts and texts of stop words alone are dropped, as the host build drops them — and model's row r is texts[kept[r]]."""
        import torch
        if len(texts) > MAX_ROWS:
            raise ValueError(f"{len(texts)} texts: a device-built BM25 index holds fewer than 2^31 rows")
        T = self.timings = {}
        t0 = time.perf_counter()
        dev = torch.device("cuda", self.device)
        if not len(texts):
            return np.zeros(0, np.int64), Bm25Model.from_postings(0, np.zeros(0, np.int64), [], np.zeros(1, np.int64),
                                                                  np.zeros(0, np.int32), np.zeros(0, np.uint16))

        def mark(name, t):
            torch.cuda.synchronize(dev)
            T[name] = T.get(name, 0.0) + time.perf_counter() - t
            return time.perf_counter()

        with torch.cuda.device(dev):
            # every batch stays alive until the build ends: a term's slot holds the address of one of its occurrences
            uploaded = [(first, torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev), off)
                        for first, data, off in self._batches(texts)]
            t = mark("upload", t0)
            slots, self.retries = self.table_slots, 0
            while True:
                h, keys, doc_len, (n_terms, n_tokens, full) = self._tokenize(torch, dev, slots, uploaded, len(texts))
                if not full:
                    break
                self._lib.rdx_bm25_build_destroy(h)
                del keys, doc_len
                if slots * 4 > self.max_slots:
                    raise RuntimeError(f"the BM25 term table of {slots} slots is more than half full and max_slots = {self.max_slots} "
                                       "allows no larger one: raise max_slots")
                slots *= 4
                self.retries += 1
            try:
                t = mark("tokenise", t)
                assert keys.numel() == n_tokens, (keys.numel(), n_tokens)
                kept = doc_len > 0
                new_row = torch.cumsum(kept, 0) - 1
                n_rows = int(new_row[-1]) + 1
                # term id = rank of the slot's first occurrence (row, byte) = Bm25Model's vocabulary order; which lane claimed a slot
                # and which occurrence represents it vanish here
                first_pos = torch.empty(slots, dtype=torch.int64, device=dev)
                stream = ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(self.device))
                L.check(self._lib.rdx_bm25_build_first_pos(h, ctypes.c_void_p(first_pos.data_ptr()), slots, stream))
                occupied = torch.nonzero(first_pos >= 0).squeeze(1)
                assert occupied.numel() == n_terms, (occupied.numel(), n_terms)
                by_first = occupied[torch.argsort(first_pos[occupied])]
                term_of_slot = torch.empty(slots, dtype=torch.int64, device=dev)
                term_of_slot[by_first] = torch.arange(n_terms, dtype=torch.int64, device=dev)
                key = (term_of_slot[keys >> 32] << 32) | new_row[keys & 0xFFFFFFFF]
                del keys
                key, tf = torch.unique_consecutive(torch.sort(key).values, return_counts=True)
                if tf.numel() and int(tf.max()) > MAX_TF:
                    raise ValueError(f"a token occurs {int(tf.max())} times in one text: the index stores tf in 16 bits (<= {MAX_TF})")
                post_off = torch.zeros(n_terms + 1, dtype=torch.int64, device=dev)
                post_off[1:] = torch.cumsum(torch.bincount(key >> 32, minlength=n_terms), 0)
                post_row = (key & 0xFFFFFFFF).to(torch.int32)
                # the vocabulary: lengths, offsets, then the normalised bytes of each term's representative occurrence
                by_first32 = by_first.to(torch.int32)
                term_off = torch.zeros(n_terms + 1, dtype=torch.int64, device=dev)
                L.check(self._lib.rdx_bm25_build_vocab(h, ctypes.c_void_p(by_first32.data_ptr()), n_terms,
                                                       ctypes.c_void_p(term_off[1:].data_ptr()), None, 0, stream))
                term_off[1:] = torch.cumsum(term_off[1:], 0)
                arena_bytes = int(term_off[-1])
                arena = torch.empty(max(arena_bytes, 1), dtype=torch.uint8, device=dev)
                L.check(self._lib.rdx_bm25_build_vocab(h, ctypes.c_void_p(by_first32.data_ptr()), n_terms,
                                                       ctypes.c_void_p(term_off.data_ptr()), ctypes.c_void_p(arena.data_ptr()),
                                                       arena_bytes, stream))
                t = mark("sort_rle", t)
                h_off, h_arena = term_off.cpu().numpy(), arena.cpu().numpy().tobytes()
                h_post_off, h_post_row = post_off.cpu().numpy(), post_row.cpu().numpy()
                h_post_tf = tf.to(torch.int32).cpu().numpy().astype(np.uint16)
                h_kept = torch.nonzero(kept).squeeze(1).cpu().numpy()
                h_doc_len = doc_len[kept].to(torch.int64).cpu().numpy()
            finally:
                self._lib.rdx_bm25_build_destroy(h)
            t = mark("download", t)
        vocab = [h_arena[a:b].decode("utf-8") for a, b in zip(h_off[:-1].tolist(), h_off[1:].tolist())]
        model = Bm25Model.from_postings(n_rows, h_doc_len, vocab, h_post_off, h_post_row, h_post_tf)
        T["host_stats"] = time.perf_counter() - t
        T["total"] = time.perf_counter() - t0
        return h_kept, model
