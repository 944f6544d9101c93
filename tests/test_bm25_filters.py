"""CPU: a document filter per query in ChunkBM25Index.search_batch / search_batch_arrays (`doc_filters`), on the CPU engine
(bm25_oracle.factory): the batch equals the per-query searches with `doc_filter`, as rows, counts and float64 score BITS; equal sets
reach the engine once; an engine that has search_filtered is asked once for the whole batch, one that has not gives the same answer."""
import numpy as np
import pytest

import bm25_oracle as O
import bm25_replay as R

A ={"cnil/doc_003.html", "cnil/doc_010.html", "cnil/doc_077.html", "absent/doc.html"}
B = {"cnil/doc_042.html", ""}
QUERIES = ["sécurité des données de santé", "durée de conservation des données de vidéosurveillance", "transfert union européenne",
           "sécurité des données de santé", "registre des traitements sous-traitant article 28", "consentement consentement cookies",
           "le la les de", "données", "sécurité des données de santé", "zzzinconnu conservation qqqabsent"]
# None, real sets, set(), unknown paths only, two equal sets (as distinct objects), and a filtered query without a known token
FILTERS = [set(A), None, set(B), None, set(), {"absent/doc.html", "nowhere"}, set(A), set(B), set(A), frozenset(A)]
TOP_K = 25


class Recorder:
    """an engine that has search_filtered: records its calls and answers through CpuBm25, query by query"""

    def __init__(self, arrays, device=0):
        self.cpu = O.CpuBm25(arrays, device)
        self.calls = []

    def search(self, off, ids, k, allow_bits=None):
        self.calls.append(("search", len(off) - 1, None, None))
        return self.cpu.search(off, ids, k, allow_bits)

    def search_filtered(self, off, ids, k, filter_sets, query_filter):
        self.calls.append(("search_filtered", len(off) - 1, np.array(filter_sets), np.array(query_filter)))
        nq = len(off) - 1
        sc, ro, cn = np.zeros((nq, k)), np.full((nq, k), -1, np.int64), np.zeros(nq, np.int32)
        for q in range(nq):
            f = int(query_filter[q])
            one = self.cpu.search(np.array([0, off[q + 1] - off[q]]), ids[off[q]:off[q + 1]], k, None if f < 0 else filter_sets[f])
            sc[q], ro[q], cn[q] = one[0][0], one[1][0], one[2][0]
        return sc, ro, cn

    def close(self):
        pass


@pytest.fixture(scope="module")
def plain():
    return R.chunk_index(O.factory)


@pytest.fixture(scope="module")
def recording():
    return R.chunk_index(Recorder)


def loop_arrays(ix, queries, filters, top_k):
    """search_batch_arrays of every query alone, with its own doc_filter -> {query index: (rows, score bits, count)}"""
    out = {}
    for i, (q, f) in enumerate(zip(queries, filters)):
        live, sc, ro, cn = ix.search_batch_arrays([q], top_k, doc_filter=f)
        if live:
            out[i] = (ro[0].tolist(), sc[0].view(np.int64).tolist(), int(cn[0]))
    return out


def batch_arrays(ix, queries, filters, top_k):
    live, sc, ro, cn = ix.search_batch_arrays(queries, top_k, doc_filters=filters)
    assert sc.shape == ro.shape == (len(live), sc.shape[1]) and cn.shape == (len(live),)
    return {i: (ro[j].tolist(), sc[j].view(np.int64).tolist(), int(cn[j])) for j, i in enumerate(live)}


def hits(results):
    return [[(r.doc_key, np.float64(r.score).tobytes(), sorted(r.metadata.items())) for r in rs] for rs in results]


def test_the_inputs_mix_every_kind_of_filter(plain):
    known = [f for f in FILTERS if f is not None and any(p in plain._group_of for p in f)]
    assert any(f is None for f in FILTERS) and set() in FILTERS and len(known) == 6
    assert any(f and not any(p in plain._group_of for p in f) for f in FILTERS if f is not None)      # unknown paths only
    assert len({frozenset(f) for f in known}) == 2 < len(known)                                          # equal sets, twice over
    want = loop_arrays(plain, QUERIES, FILTERS, TOP_K)
    assert 4 not in want and 5 not in want and 6 not in want and {0, 1, 2, 3, 7, 8, 9} <= set(want)    # set(), unknown, no token
    assert want[0] == want[8] and want[0] != want[3]                                                     # the filter shows


def test_search_batch_equals_the_per_query_searches(plain):
    got = plain.search_batch(QUERIES, TOP_K, doc_filters=FILTERS)
    want = [plain.search(q, TOP_K, doc_filter=f) for q, f in zip(QUERIES, FILTERS)]
    assert hits(got) == hits(want)
    assert [len(g) for g in got][4:7] == [0, 0, 0] and all(len(g) > 0 for g in got[:4])


@pytest.mark.parametrize("top_k", [TOP_K, 1, 4000])
def test_search_batch_arrays_equals_the_per_query_searches(plain, top_k):
    assert batch_arrays(plain, QUERIES, FILTERS, top_k) == loop_arrays(plain, QUERIES, FILTERS, top_k)


def test_no_filter_at_all_and_nothing_to_find(plain):
    nones = [None] * len(QUERIES)
    assert batch_arrays(plain, QUERIES, nones, TOP_K) == loop_arrays(plain, QUERIES, nones, TOP_K)
    live, sc, ro, cn = plain.search_batch_arrays(QUERIES[:3], TOP_K, doc_filters=[set(), {"nowhere"}, set()])
    assert list(live) == [] and len(cn) == 0
    assert plain.search_batch([], TOP_K, doc_filters=[]) == []
    assert hits(plain.search_batch(QUERIES, 0, doc_filters=FILTERS)) == [[] for _ in QUERIES]


def test_both_keywords_or_a_wrong_length_are_refused(plain):
    for call in (plain.search_batch, plain.search_batch_arrays):
        with pytest.raises(ValueError, match="not both"):
            call(QUERIES, TOP_K, doc_filter=set(A), doc_filters=FILTERS)
        with pytest.raises(ValueError, match="doc_filters has 9 entries for 10 queries"):
            call(QUERIES, TOP_K, doc_filters=FILTERS[:-1])
        with pytest.raises(ValueError, match="doc_filters has 0 entries"):
            call(QUERIES, TOP_K, doc_filters=[])


def test_an_engine_with_search_filtered_is_called_once_with_one_row_per_distinct_set(recording, plain):
    eng = recording.engine
    eng.calls.clear()
    got = batch_arrays(recording, QUERIES, FILTERS, TOP_K)
    assert [c[0] for c in eng.calls] == ["search_filtered"]
    _, nq, sets, qf = eng.calls[0]
    # the queries sent: the ones with a known token whose filter names an indexed document (or that have no filter)
    assert nq == 7 and qf.tolist() == [0, -1, 1, -1, 1, 0, 0]
    assert sets.shape == (2, (len(recording._group_of) + 31) // 32) and sets.dtype == np.uint32       # A (four times over) and B
    for row, f in zip(sets, (A, B)):
        assert (row == recording._allow_bits(f)).all()
    assert got == loop_arrays(plain, QUERIES, FILTERS, TOP_K)
    # several distinct filters, still one call; without any set the engine's plain search serves
    eng.calls.clear()
    paths = [p for p in recording._group_of if p][:6]
    batch_arrays(recording, QUERIES[:6], [{p} for p in paths], TOP_K)
    assert [c[0] for c in eng.calls] == ["search_filtered"] and eng.calls[0][2].shape[0] == 6
    eng.calls.clear()
    batch_arrays(recording, QUERIES, [None] * len(QUERIES), TOP_K)
    assert [c[0] for c in eng.calls] == ["search"]


def test_an_engine_without_search_filtered_gives_the_same_answer(plain, recording):
    assert not hasattr(plain.engine, "search_filtered")
    assert batch_arrays(plain, QUERIES, FILTERS, TOP_K) == batch_arrays(recording, QUERIES, FILTERS, TOP_K)
    assert hits(plain.search_batch(QUERIES, TOP_K, doc_filters=FILTERS)) == hits(recording.search_batch(QUERIES, TOP_K, doc_filters=FILTERS))


def test_the_existing_keyword_is_unchanged(plain):
    for f in (None, set(A), set(), {"nowhere"}):
        got = plain.search_batch(QUERIES, TOP_K, doc_filter=f)
        assert hits(got) == hits([plain.search(q, TOP_K, doc_filter=f) for q in QUERIES])
        assert hits(got) == hits(plain.search_batch(QUERIES, TOP_K, doc_filters=[f] * len(QUERIES)))


def test_set_filters_equals_set_filter():
    from rag_dpo_amd import fusion as F
    rng = np.random.default_rng(5)
    allowed = {q: sorted(rng.choice(70, int(rng.integers(0, 20)), replace=False).tolist()) for q in (0, 2, 3, 6)}
    allowed[3] = [31, 32, 63, 64, 69, 0]
    one, many = F.PackedLists(7, 2, 4), F.PackedLists(7, 2, 4)
    for q, gs in allowed.items():
        one.set_filter(q, gs, 70)
    many.set_filters(allowed, 70)
    assert many.group_words == one.group_words == 3 and (many.allow == one.allow).all() and (many.filter_on == one.filter_on).all()
    for q in range(7):
        assert many.allowed_groups_of(q) == (sorted(allowed[q]) if q in allowed else None)
    many.set_filters({}, 1000)
    assert many.group_words == 3
