"""GPU: a BM25 index built from text on the device (rag_dpo_amd/bm25_build.py DeviceBm25Builder over k_bm25_tok / k_bm25_vocab,
csrc/bm25_build_kernel.hpp) is the index the host builds: the same vocabulary in the same order, the same postings, and the same
float64 statistics bit for bit. Every assertion is exact equality. The chunk constant the edge cases aim at is read out of the
header."""
import os
import re
from collections import Counter

import numpy as np
import pytest

import bm25_replay as R
from bm25_replay import W
from rag_dpo_amd import bm25
from rag_dpo_amd.bm25 import Bm25Model, ChunkBM25Index, SummaryBM25Index, tokenize_french
from rag_dpo_amd.bm25_build import DeviceBm25Builder, tokenize_utf8

pytestmark = pytest.mark.gpu
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rag_dpo_amd", "csrc", "bm25_build_kernel.hpp")
CHUNK = int(re.search(r"constexpr int BM25_TOK_CHUNK = (\d+);", open(HEADER).read()).group(1))
# str.split() separates on these, the tokeniser does not (the CPU sweep of tests/test_bm25_build_model.py covers them)
SPLIT_ONLY = {0x1C, 0x1D, 0x1E, 0x1F, 0x85, 0x1680, 0x2028, 0x2029, 0x205F, 0x3000}


def host_build(texts):
    """-> (kept indexes, Bm25Model) the way ChunkBM25Index.build_from_collection builds them on the host"""
    kept, tokens = [], []
    for i, t in enumerate(texts):
        if not t or not t.strip():
            continue
        tok = tokenize_french(t)
        if tok:
            kept.append(i)
            tokens.append(tok)
    return kept, Bm25Model(tokens)


def assert_equal(dev, host):
    assert list(dev.term_id.items()) == list(host.term_id.items())
    assert (dev.n_rows, dev.n_terms) == (host.n_rows, host.n_terms)
    for name in ("post_off", "post_row", "post_tf", "idf", "denom", "doc_len"):
        a, b = getattr(dev, name), getattr(host, name)
        assert a.dtype == b.dtype and np.array_equal(a, b), name
    assert dev.idf.tobytes() == host.idf.tobytes() and dev.denom.tobytes() == host.denom.tobytes()
    assert repr(dev.average_idf) == repr(host.average_idf) and repr(dev.avgdl) == repr(host.avgdl)


def same_as_host(texts, **builder):
    b = DeviceBm25Builder(0, **builder)
    kept, dev = b.build(texts)
    want_kept, host = host_build(texts)
    assert kept.tolist() == want_kept
    assert_equal(dev, host)
    return b, dev


def row_tokens(model):
    """per row the multiset of its tokens {term bytes: tf}, rebuilt from the postings"""
    terms = [t.encode("utf-8") for t in model.term_id]
    term = np.repeat(np.arange(model.n_terms), np.diff(model.post_off))
    out = [Counter() for _ in range(model.n_rows)]
    for t, r, tf in zip(term.tolist(), model.post_row.tolist(), model.post_tf.tolist()):
        out[r][terms[t]] = tf
    return out


@pytest.fixture(scope="module")
def world():
    return W.chunk_texts()


def device_chunk_index():
    ix = ChunkBM25Index(build="device")
    ix.build_from_collection(W.build_collection(R.dense_cpu), batch_size=700)
    return ix


def test_world_equals_host_and_replays_the_fixture(world, tmp_path):
    same_as_host(world)
    chunk = device_chunk_index()
    assert chunk.corpus_tokens == [] and isinstance(chunk.engine, bm25.HipBm25)
    R.replay_chunk_search(chunk)
    host = R.chunk_index(None)
    assert_equal(chunk.model, host.model)
    assert (chunk.chunk_ids, chunk.chunk_texts, chunk.chunk_metadatas, chunk._group_of) == \
           (host.chunk_ids, host.chunk_texts, host.chunk_metadatas, host._group_of)
    summ = SummaryBM25Index(summaries_path=W.write_summaries(str(tmp_path)), build="device")
    summ.build()
    R.replay_summary(summ)
    R.replay_retriever(None, summ, chunk)


@pytest.mark.parametrize("quarter", range(4))
def test_every_code_point_through_the_kernel(quarter):
    cps = [cp for cp in range(0x110000) if not 0xD800 <= cp <= 0xDFFF and cp not in SPLIT_ONLY]
    cps = cps[quarter * len(cps) // 4:(quarter + 1) * len(cps) // 4]
    texts = [" ".join("ab" + chr(cp) + "cd" for cp in cps[lo:lo + 4096]) for lo in range(0, len(cps), 4096)]
    _, dev = same_as_host(texts)                          # the vocabulary and everything else
    got = row_tokens(dev)
    for r, t in enumerate(texts):
        assert got[r] == Counter(tokenize_utf8(t.encode("utf-8"))), r


def test_chunk_and_row_edges():
    texts = []
    for start in range(2 * CHUNK + 3):                    # a token start at every offset around two chunk boundaries
        pad = " " * start
        texts += [pad + "éab fin", pad + "abé", pad + "Kz x", pad + "Œuvre-É", pad + "ab-cd"]
    long = "a" * 70000                                    # longer than any 16-bit field, walked across hundreds of chunks
    texts += ["x " + long + " premier", long, "", "a", "é", "ab", "zé", "fin ab-", "cd début", "ligne finissant par abc",
              "a--b", "-ab-", "İstanbul", "ab-İ-cd", "aİ", None, " " * (CHUNK - 1) + "É", " " * (CHUNK - 1) + "-ab-cd-"]
    _, dev = same_as_host(texts, batch_rows=1000)
    got = row_tokens(dev)
    kept = [t for t in texts if t and tokenize_french(t)]
    for r, t in enumerate(kept):
        assert got[r] == Counter(tokenize_utf8(t.encode("utf-8"))), t[-20:]
    vocab = dev.term_id
    assert long in vocab and np.diff(dev.post_off)[vocab[long]] == 2            # one term, two rows
    assert "stanbul" in vocab and "istanbul" not in vocab and "ab-cd" in vocab and "abcd" not in vocab
    rows = {t: i for i, t in enumerate(kept)}
    assert got[rows["fin ab-"]] == Counter([b"fin", b"ab"]) and got[rows["cd début"]] == Counter([b"cd", "début".encode()])
    assert "a--b" not in rows and got[rows["-ab-"]] == Counter([b"ab"]) and got[rows["ab-İ-cd"]] == Counter([b"ab-i", b"cd"])


def test_order_of_the_idf_sum():
    rng = np.random.default_rng(5)
    words = [f"mot{i}" for i in range(1200)]
    texts = [("commun " if i % 3 else "") + " ".join(rng.choice(words, size=int(rng.integers(3, 30)))) for i in range(900)]
    _, host = host_build(texts)
    assert host.n_terms >= 1000 and np.diff(host.post_off).max() > host.n_rows / 2
    assert (host.idf == bm25.EPSILON * host.average_idf).any()                   # the epsilon floor is in play
    nd = np.diff(host.post_off)
    _, reversed_average = bm25.idf_of(host.n_rows, nd[::-1])
    assert repr(reversed_average) != repr(host.average_idf)                      # the sum's order shows in the bits
    same_as_host(texts)


def test_forced_collisions(world):
    same_as_host(world, hash_mask=0x3, table_slots=1 << 12)                      # every term probes from one of four slots


def test_full_table_retries_or_raises(world):
    texts = world[:40]
    assert host_build(texts)[1].n_terms > 32
    b, _ = same_as_host(texts, table_slots=64)
    assert b.retries >= 1
    with pytest.raises(RuntimeError, match="max_slots"):
        DeviceBm25Builder(0, table_slots=64, max_slots=64).build(texts)


def test_tf_limit():
    same_as_host(["mot " * 65535 + "autre", "autre mot"])
    with pytest.raises(ValueError) as e:
        DeviceBm25Builder(0).build(["mot " * 65536 + "autre", "autre mot"])
    with pytest.raises(ValueError) as h:
        host_build(["mot " * 65536 + "autre", "autre mot"])
    assert str(e.value) == str(h.value)


def test_contention_and_determinism():
    texts = ["alpha beta gamma"] * 20000
    _, one = same_as_host(texts)
    _, small = same_as_host(texts, batch_rows=7)
    _, again = same_as_host(texts)
    for m in (small, again):
        assert_equal(m, one)


class FakeCollection:
    def __init__(self, docs):
        self.docs = docs

    def count(self):
        return len(self.docs)

    def get(self, limit, offset, include):
        d = self.docs[offset:offset + limit]
        return {"ids": [f"id{offset + i}" for i in range(len(d))], "documents": d,
                "metadatas": [{"document_path": f"doc{(offset + i) % 3}"} for i in range(len(d))]}


def test_dropped_rows_line_up():
    docs = []
    for i, hole in enumerate([None, "", "   ", "le la", "é"] * 3):
        docs += [f"texte numéro {i} du registre", hole, f"autre texte {i} sous-traitant"]
    col = FakeCollection(docs)
    dev, host = ChunkBM25Index(build="device"), ChunkBM25Index()
    dev.build_from_collection(col, batch_size=4)
    host.build_from_collection(col, batch_size=4)
    assert (dev.chunk_ids, dev.chunk_texts, dev.chunk_metadatas, dev._group_of) == \
           (host.chunk_ids, host.chunk_texts, host.chunk_metadatas, host._group_of)
    assert_equal(dev.model, host.model)
    q = "registre sous-traitant numéro 3"
    assert [(r.doc_key, repr(r.score)) for r in dev.search(q, 10)] == [(r.doc_key, repr(r.score)) for r in host.search(q, 10)]
    with pytest.raises(UnicodeEncodeError):
        DeviceBm25Builder(0).build(["bon texte", "mauvais \ud800 texte"])
    empty = ChunkBM25Index(build="device")
    empty.build_from_collection(FakeCollection(["le la", None]))
    assert empty.is_built and empty.engine is None and empty.search("registre") == []
