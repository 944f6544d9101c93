"""The spill list of k_refine (option refine_spill, DESIGN.md §5 "spill list"): a query with more hits than the LDS list holds is
answered by k_refine_spill from a list in HBM instead of the fallback passes, by the same code. Every case searches the SAME index
twice — refine_spill = 0 with the automatic LDS list (the path before the spill list existed), then refine_spill = 1 with
refine_list = 32 (every query with more than 32 hits spills) — and asserts: ids, score bits and counts equal the C oracle's in both
runs, `emitted` and `rescored` are equal between the runs (which rows are re-scored does not depend on where the list lives), no
query took a fallback pass in either, and the second run did spill (the library's developer line RDX_DEBUG_HITS on stderr: the
longest hit list of the search and the number of queries k_refine queued for k_refine_spill).

The int8 leg (coarse_i8 = 1; dim 128 and 1024; 129 and 257 queries) and the fp16 leg (3 and 64 queries) share the list code.
Corpora have 9 000 - 15 000 rows; the oracle's answers are computed once per (corpus, queries, k, bitmap) and shared."""
import re

import numpy as np
import pytest

from rag_dpo_amd import synth

pytestmark = pytest.mark.gpu

ROWS = 9_000
I8_AUTO_SAMPLE_MUL = 2      # rdx_index.hip: the sample of an automatically chosen int8 search, in units of the fp16 pass's
_refs = {}


@pytest.fixture(scope="module")
def eng():
    from rag_dpo_amd import engine
    return engine


@pytest.fixture(autouse=True)
def _debug_hits(monkeypatch):
    monkeypatch.setenv("RDX_DEBUG_HITS", "1")


@pytest.fixture(scope="module")
def data():
    out = {}
    for d in (128, 1024):
        corpus = synth.make_corpus(ROWS, d)
        out[d] = (corpus, synth.make_queries(257, d, corpus))
    return out


def _ref(oracle, tag, corpus, q, k, allow=None):
    key = (tag, q.shape[0], k, None if allow is None else int(allow.sum()))
    if key not in _refs:
        _refs[key] = oracle.cosine_topk(oracle.normalize_rows(corpus), q, k, allow)
    return _refs[key]


def _hits_line(capfd):
    """(longest hit list, queries spilled) summed / maximised over the searches since the last read (a fallback pass prints too)"""
    found = re.findall(r"hits max (\d+) spilled (\d+)", capfd.readouterr().err)
    assert found, "the library did not print its RDX_DEBUG_HITS line"
    return max(int(a) for a, _ in found), sum(int(b) for _, b in found)


def _index(eng, corpus, i8, **opts):
    ix = eng.HipIndex(corpus.shape[1])
    ix.set_option("coarse_i8", 1 if i8 else 0)
    if not i8:
        ix.set_option("force_fast", 1)       # 3 queries on 9 000 rows would take the exact full scan alone
    for name, v in opts.items():
        ix.set_option(name, v)
    ix.add(corpus)
    return ix


def _search(oracle, capfd, ix, ref, q, k, allow, n, i8):
    capfd.readouterr()
    gs, gr, gc = ix.search(q, k, oracle.pack_mask(allow, n))
    st = ix.last_stats()
    hits_max, spilled = _hits_line(capfd)
    es, er, ec = ref
    np.testing.assert_array_equal(gc, ec)
    np.testing.assert_array_equal(gr, er)
    np.testing.assert_array_equal(gs, es)
    assert st["coarse_bits"] == (8 if i8 else 16) and st["path"] == 0, st
    return st, hits_max, spilled


def _both(oracle, capfd, ix, ref, q, k, i8, n, allow=None, list_b=32, base_overflows=False):
    """the two runs on one index; -> (stats of the spilling run, its longest list, its spilled queries).
    base_overflows: the first run's automatic LDS list is known to be too short for some query (it takes the fallback passes, which
    count their own hits): only the spilling run must answer by itself"""
    ix.set_option("refine_spill", 0)
    ix.set_option("refine_list", 0)
    a, max_a, sp_a = _search(oracle, capfd, ix, ref, q, k, allow, n, i8)
    ix.set_option("refine_spill", 1)
    ix.set_option("refine_list", list_b)
    b, max_b, sp_b = _search(oracle, capfd, ix, ref, q, k, allow, n, i8)
    print(f"nq {q.shape[0]} k {k}: emitted {a['emitted']} / {b['emitted']} rescored {a['rescored']} / {b['rescored']} "
          f"longest list {max_b} spilled {sp_b}")
    assert b["retried_queries"] == 0 and b["exact_queries"] == 0, b
    if base_overflows:
        assert a["retried_queries"] >= 1, a
    else:
        assert a["retried_queries"] == 0 and a["exact_queries"] == 0, a
        assert a["emitted"] == b["emitted"] and a["rescored"] == b["rescored"], (a, b)
    assert sp_a == 0 and max_a == max_b, (sp_a, max_a, max_b)
    assert sp_b >= 1 and max_b > list_b, (sp_b, max_b)
    return b, max_b, sp_b


@pytest.mark.parametrize("nq", [129, 257])
@pytest.mark.parametrize("d", [128, 1024])
def test_i8_widths_and_tiles(eng, oracle, capfd, data, d, nq):
    corpus, q = data[d]
    ix = _index(eng, corpus, True)
    _both(oracle, capfd, ix, _ref(oracle, d, corpus, q[:nq], 10), q[:nq], 10, True, ROWS)
    ix.close()


@pytest.mark.parametrize("k", [1, 100])
def test_i8_other_k(eng, oracle, capfd, data, k):
    corpus, q = data[1024]
    ix = _index(eng, corpus, True)
    _both(oracle, capfd, ix, _ref(oracle, 1024, corpus, q[:129], k), q[:129], k, True, ROWS)
    ix.close()


@pytest.mark.parametrize("spec", [0, 1])
@pytest.mark.parametrize("pilot", [0, 1, 4])
def test_i8_pilot_and_threshold(eng, oracle, capfd, data, pilot, spec):
    corpus, q = data[1024]
    ix = _index(eng, corpus, True, refine_pilot=pilot, spec_tau=spec)
    _both(oracle, capfd, ix, _ref(oracle, 1024, corpus, q[:129], 10), q[:129], 10, True, ROWS)
    ix.close()


def test_i8_where_bitmap(eng, oracle, capfd, data):
    corpus, q = data[1024]
    allow = np.random.default_rng(4).random(ROWS) < 0.6
    ix = _index(eng, corpus, True)
    _both(oracle, capfd, ix, _ref(oracle, 1024, corpus, q[:129], 10, allow), q[:129], 10, True, ROWS, allow)
    ix.close()


def test_i8_compact_bf16_master(eng, oracle, capfd, data):
    import torch
    corpus, q = data[1024]
    cb = torch.from_numpy(corpus).to(torch.bfloat16)
    wide = cb.to(torch.float32).numpy()
    ix = eng.HipIndex(1024)
    ix.set_option("compact_master", 1)
    ix.set_option("coarse_i8", 1)
    ix.add_bf16(cb)
    _both(oracle, capfd, ix, _ref(oracle, "bf16", wide, q[:129], 10), q[:129], 10, True, ROWS)
    ix.close()


@pytest.mark.parametrize("nq", [3, 64])
def test_f16_leg(eng, oracle, capfd, data, nq, k=100):
    """an fp16 search of a corpus this small samples all of it and emits little more than k hits: k = 100 is what fills more than
    32 slots (k = 10 on the fp16 leg: the crowded corpus below)"""
    corpus, q = data[1024]
    ix = _index(eng, corpus, False)
    _both(oracle, capfd, ix, _ref(oracle, 1024, corpus, q[:nq], k), q[:nq], k, False, ROWS)
    ix.close()


def test_boundary_between_the_two_lists(eng, oracle, capfd, data):
    """one query with m hits (counted by a first run): refine_list = m keeps it in LDS, refine_list = m - 1 spills it"""
    corpus, q = data[1024]
    q1, k = q[5:6], 100
    ref = _ref(oracle, "one", corpus, q1, k)
    ix = _index(eng, corpus, False)
    first, m, spilled = _search(oracle, capfd, ix, ref, q1, k, None, ROWS, False)
    assert m == first["emitted"] and m > 33 and spilled == 0, (m, first)
    ix.set_option("refine_spill", 1)
    for cap, want in ((m, 0), (m - 1, 1)):
        ix.set_option("refine_list", cap)
        st, m2, spilled = _search(oracle, capfd, ix, ref, q1, k, None, ROWS, False)
        assert (m2, spilled) == (m, want), (cap, m2, spilled)
        assert st["emitted"] == first["emitted"] and st["rescored"] == first["rescored"], (st, first)
        assert st["retried_queries"] == 0 and st["exact_queries"] == 0, st
    ix.close()


@pytest.fixture(scope="module")
def crowded():
    """1 500 near copies of one direction (the band below X1 holds more rows than the ranking arrays, REFINE_PMAX = 1 024: the
    compaction in the list) and 1 200 IDENTICAL rows (they tie at the k-th score: the selection by row key)"""
    d = 1024
    rng = np.random.default_rng(31)
    corpus = synth.make_corpus(15_000, d)
    centres = rng.standard_normal((2, d)).astype(np.float32)
    corpus[2000:3500] = centres[0] + 0.002 * rng.standard_normal((1500, d)).astype(np.float32)
    corpus[6000:7200] = centres[1]
    q = synth.make_queries(129, d, corpus)
    q[:2] = centres + 0.01 * rng.standard_normal((2, d)).astype(np.float32)
    return corpus, q


@pytest.mark.parametrize("i8,nq", [(True, 129), (False, 64), (False, 3)])
def test_near_duplicates_and_ties_in_the_spill_list(eng, oracle, capfd, crowded, i8, nq):
    """(fp16 leg: the automatic LDS list of so small an fp16 search is 1 024 entries, so without the spill list the two crowds'
    queries take the fallback passes; with it they do not)"""
    corpus, q = crowded
    q = q[:nq]
    ix = _index(eng, corpus, i8, spec_tau=0)
    st, longest, _ = _both(oracle, capfd, ix, _ref(oracle, "crowded", corpus, q, 10), q, 10, i8, corpus.shape[0], base_overflows=not i8)
    assert longest >= 1500 and st["rescored"] >= 1500 + 1200, (longest, st)      # both queries' crowds were re-scored from the list
    ix.close()


def test_zero_query(eng, oracle, capfd, data):
    """a zero query scores 0 on every row: 9 000 hits. Without the spill list (refine_spill = 0, and the default for a forced int8
    search) it overflows the LDS list and takes both fallback passes, as before; with it, it is answered from the spill list"""
    corpus, q = data[128]
    qz = q[:129].copy()
    qz[7] = 0.0
    ref = _ref(oracle, "zero", corpus, qz, 10)
    ix = _index(eng, corpus, True)
    for spill in (None, 0):
        if spill is not None:
            ix.set_option("refine_spill", spill)
        st, longest, spilled = _search(oracle, capfd, ix, ref, qz, 10, None, ROWS, True)
        assert longest == ROWS and spilled == 0, (longest, spilled)
        assert st["retried_queries"] == 1 and st["exact_queries"] == 1, st
    ix.set_option("refine_spill", 1)
    st, longest, spilled = _search(oracle, capfd, ix, ref, qz, 10, None, ROWS, True)
    assert longest == ROWS and spilled == 1, (longest, spilled)
    assert st["retried_queries"] == 0 and st["exact_queries"] == 0, st
    ix.close()


def test_spill_cap_exceeded_takes_the_fallback(eng, oracle, capfd, data):
    """developer option spill_cap = 32 with refine_list = 32: a query with more than 32 hits fits neither list and is answered by
    the fallback passes, exactly, and counted in retried_queries"""
    corpus, q = data[128]
    ref = _ref(oracle, 128, corpus, q[:129], 10)
    ix = _index(eng, corpus, True, refine_spill=1, refine_list=32, spill_cap=32)
    st, longest, spilled = _search(oracle, capfd, ix, ref, q[:129], 10, None, ROWS, True)
    assert longest > 32 and spilled == 0, (longest, spilled)
    assert 1 <= st["retried_queries"] <= 129, st
    ix.close()


def test_plan_sample_rows(eng):
    """The default plan thins the int8 sample only where int8 is chosen automatically: 2^20 rows x 257 queries sample every
    (64 / I8_AUTO_SAMPLE_MUL)-th 32-row block (sample_div = 64: 128 eight-block entries per multiple), option i8_sample_mul = 8 is the
    earlier plan's every 8th block; a forced int8 search of 15 000 rows samples what it did before: div = 1, floor(469 blocks / 8)
    = 58 entries of 256 rows"""
    n, d = 1 << 20, 128
    rng = np.random.default_rng(5)
    corpus = rng.standard_normal((n, d), dtype=np.float32)
    q = rng.standard_normal((257, d), dtype=np.float32)
    for mul, want in ((None, n // (64 // I8_AUTO_SAMPLE_MUL)), (8, n // 8)):   # (an index each: a search adapts the next one's sample)
        ix = eng.HipIndex(d)
        if mul is not None:
            ix.set_option("i8_sample_mul", mul)
        ix.add(corpus)
        ix.search(q, 10)
        st = ix.last_stats()
        assert st["coarse_bits"] == 8 and st["sample_rows"] == want, (mul, want, st)
        ix.close()
    ix = eng.HipIndex(d)
    ix.set_option("coarse_i8", 1)
    ix.add(corpus[:15_000])
    ix.search(q, 10)
    st = ix.last_stats()
    assert st["coarse_bits"] == 8 and st["sample_rows"] == 58 * 256, st
    ix.close()
