"""CPU: the byte-level statement of tokenize_french (rag_dpo_amd/bm25_build.py tokenize_utf8, the model of k_bm25_tok) against
tokenize_french itself over every code point, Bm25Model.from_postings against Bm25Model, the constants csrc/bm25_build_kernel.hpp
shares with the model, and the `build` keyword of the indexes without a GPU. Every assertion is exact equality."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import bm25_world as W  # noqa: E402
from rag_dpo_amd import bm25, bm25_build as BB  # noqa: E402
from rag_dpo_amd.bm25 import Bm25Model, tokenize_french  # noqa: E402

HEADER = os.path.join(os.path.dirname(HERE), "rag_dpo_amd", "csrc", "bm25_build_kernel.hpp")
LOWER_W = "0123456789abcdefghijklmnopqrstuvwxyzàâäçéèêëîïôùûüÿæœ"
UPPER_W = "ABCDEFGHIJKLMNOPQRSTUVWXYZÀÂÄÆÇÈÉÊËÎÏÔÙÛÜŒŸKİ"


def code_points():
    return (cp for cp in range(0x110000) if not 0xD800 <= cp <= 0xDFFF)


def same(text):
    want = [t.encode("utf-8") for t in tokenize_french(text)]
    got = BB.tokenize_utf8(text.encode("utf-8"))
    assert got == want, (text, got, want)


def test_exactly_98_code_points_lower_into_the_class():
    cls = set(LOWER_W)
    found = {chr(cp) for cp in code_points() if cls & set(chr(cp).lower())}
    assert len(LOWER_W) == 53 and len(UPPER_W) == 45
    assert found == set(LOWER_W) | set(UPPER_W) and len(found) == 98
    for c in sorted(found):                       # what the model says of each: its normalised bytes, and İ's break alone
        take, norm, brk = BB.word_char(c.encode("utf-8"), 0)
        assert take == len(c.encode("utf-8")) and brk == (c == "İ")
        assert norm == (b"i" if brk else c.lower().encode("utf-8"))
    for cp in code_points():                      # and of no other code point
        if chr(cp) not in found:
            assert BB.word_char(chr(cp).encode("utf-8"), 0) is None, hex(cp)


@pytest.mark.parametrize("context", ["ab{}cd", "{}{}", "a-{}-b"])
def test_every_code_point(context):
    encode, model = str.encode, BB.tokenize_utf8
    for cp in code_points():
        text = context.replace("{}", chr(cp))
        if model(encode(text)) != [encode(t) for t in tokenize_french(text)]:
            same(text)


def test_world_tokenizer_texts():
    for t in W.TOKENIZER_TEXTS:
        same(t)
    for t in W.chunk_texts()[:300]:
        same(t)


def test_random_strings():
    alphabet = list(LOWER_W + UPPER_W) + ["-", "-", " ", " ", "é", " ", "\U0001F600", "\0", "'", "ß", "̇"]
    alphabet += [" " + w + " " for w in sorted(bm25.STOPWORDS)] + sorted(bm25.STOPWORDS)
    rng = np.random.default_rng(20)
    for _ in range(4000):
        same("".join(rng.choice(alphabet, size=int(rng.integers(0, 24)))))
    for t in ("a--b", "-ab-", "ab-cd-ef", "İstanbul", "a-İ-b", "peut-être", "é", "K", "Kb", "a-b", "ab-", "-", ""):
        same(t)
    assert BB.tokenize_utf8("a--b -ab- ab-cd-ef İstanbul".encode()) == [b"ab", b"ab-cd-ef", b"stanbul"]


def test_header_constants_are_the_models():
    src = open(HEADER).read()
    assert int(re.search(r"BM25_C3_LOWER = (0x[0-9A-Fa-f]+)u", src).group(1), 16) == BB.C3_LOWER
    assert int(re.search(r"BM25_C3_UPPER = (0x[0-9A-Fa-f]+)u", src).group(1), 16) == BB.C3_UPPER
    table = re.search(r"BM25_STOPWORDS\[BM25_N_STOPWORDS\] = \{(.*?)\};", src, re.S).group(1)
    keys = [int(x, 16) for x in re.findall(r"0x([0-9a-f]+)ull", table)]
    assert keys == BB.stopword_keys() and keys == sorted(set(keys))
    assert int(re.search(r"BM25_N_STOPWORDS = (\d+);", src).group(1)) == len(keys)
    assert int(re.search(r"BM25_BUILD_MAX_ROWS = (\d+);", src).group(1)) == BB.MAX_ROWS
    assert int(re.search(r"BM25_BUILD_MAX_ROW_BYTES = (\d+);", src).group(1)) == BB.MAX_ROW_BYTES
    assert int(re.search(r"BM25_TOK_CHUNK = (\d+);", src).group(1)) == int(re.search(r"BM25_TOK_THREADS = (\d+);", src).group(1))


def test_from_postings_reproduces_the_model():
    tokens = [t for t in map(tokenize_french, W.chunk_texts()) if t]
    m = Bm25Model(tokens)
    f = Bm25Model.from_postings(m.n_rows, m.doc_len.copy(), list(m.term_id), m.post_off.copy(), m.post_row.copy(), m.post_tf.copy())
    assert list(f.term_id.items()) == list(m.term_id.items()) and (f.n_rows, f.n_terms) == (m.n_rows, m.n_terms)
    assert f.idf.tobytes() == m.idf.tobytes() and f.denom.tobytes() == m.denom.tobytes()
    assert repr(f.average_idf) == repr(m.average_idf) and repr(f.avgdl) == repr(m.avgdl)
    assert (m.idf == bm25.EPSILON * m.average_idf).any()                # the epsilon floor is in play in this corpus
    for name, a in vars(f.arrays()).items():
        b = getattr(m.arrays(), name)
        assert (a is None and b is None) or np.array_equal(a, b), name
    e = Bm25Model.from_postings(0, np.zeros(0, np.int64), [], np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.uint16))
    z = Bm25Model([])
    assert (e.n_rows, e.n_terms, e.avgdl, e.average_idf) == (z.n_rows, z.n_terms, z.avgdl, z.average_idf) and e.denom.shape == (0,)
    with pytest.raises(ValueError):
        Bm25Model.from_postings(m.n_rows, m.doc_len[:-1], list(m.term_id), m.post_off, m.post_row, m.post_tf)


def test_build_keyword():
    import torch
    for cls in (bm25.ChunkBM25Index, bm25.SummaryBM25Index):
        assert cls().build_mode == "host"
        with pytest.raises(ValueError, match="build"):
            cls(build="x")
        if not torch.cuda.is_available():
            with pytest.raises(RuntimeError):
                cls(build="device")
            assert cls(build="auto").build_mode == "host"
