"""Returned row ids on the routes of k_refine and k_select_dense that translate a local row into the id the caller sees (RowIds::of,
k_rows.hpp). The corpus is built so that the searches meet them — a spill list, a re-score band with more than REFINE_PMAX rows
(the crowded band), more than 1 024 ties at the k-th score (k_refine's row-key select, and past EQ_CAP k_select_dense's tie walk) —
and every index answers either through a row-id map (3 i + 7) or through option row_base = 1000. What a leg ASSERTS of its route is
what the library reports: the spill count of its RDX_DEBUG_HITS line, retried / exact queries, coarse_bits, path, and on the int8
leg that both crowds were re-scored (rescored >= 1 500 + 1 200, more than the ranking arrays hold); which branch inside k_refine
ranked the rows is not reported and not asserted. Then every leg compares with the C oracle: counts, score bits, and
ids[oracle row] (-1 stays -1).

The corpus is the `crowded` fixture of test_gpu_refine_spill.py at 4 096 rows: 1 500 near copies of one direction and 1 200
identical rows of another, a query aimed at each crowd and ordinary queries behind them; k = 10. Two widths: 128, and 1 152 (above
1 024: k_refine's re-score takes exact_score, and the exact path k_exact_scores instead of k_exact_scores_reg).

The int8 leg at 1 152 columns: the search plan runs the int8 pass up to dim_pad = 1 024 only (search_plan.hpp i8_shape: at most 8
k-steps of 128 columns, so that the int8 dot product stays exact in fp32), whatever the number of rows. Asked for int8 at that
width the library answers on the fp16 pass, and that is what the leg asserts there (coarse_bits == 16 on the MFMA path) next to the
same comparison with the oracle: at that width the leg pins 129 queries on the fp16 pass and nothing of the int8 path. At 128 columns
it asserts coarse_bits == 8."""
import re

import numpy as np
import pytest

from rag_dpo_amd import synth

pytestmark = pytest.mark.gpu

ROWS, K, NQ, BASE = 4096, 10, 129, 1000
DIMS = (128, 1152)
I8_MAX_DIM = 1024           # search_plan.hpp: i8_shape
_cache = {}


@pytest.fixture(autouse=True)
def _debug_hits(monkeypatch):
    monkeypatch.setenv("RDX_DEBUG_HITS", "1")


def _data(oracle, d):
    """(corpus, queries, the oracle's answer for all NQ queries), once per width"""
    if d not in _cache:
        rng = np.random.default_rng(31)
        corpus = synth.make_corpus(ROWS, d)
        centres = rng.standard_normal((2, d)).astype(np.float32)
        corpus[500:2000] = centres[0] + 0.002 * rng.standard_normal((1500, d)).astype(np.float32)
        corpus[2500:3700] = centres[1]
        q = synth.make_queries(NQ, d, corpus)
        q[:2] = centres + 0.01 * rng.standard_normal((2, d)).astype(np.float32)
        ref = oracle.cosine_topk(oracle.normalize_rows(corpus), q, K)
        for a in (corpus, q) + ref:
            a.setflags(write=False)
        _cache[d] = corpus, q, ref
    return _cache[d]


def _index(corpus, mapped):
    """-> (index, ids): local row r is returned as ids[r]"""
    from rag_dpo_amd import engine
    ix = engine.HipIndex(corpus.shape[1])
    if mapped:
        ix.add(corpus)
        ids = 3 * np.arange(ROWS, dtype=np.int64) + 7
        ix.set_row_ids(0, ids)
    else:
        ix.set_option("row_base", BASE)
        ix.add(corpus)
        ids = BASE + np.arange(ROWS, dtype=np.int64)
    return ix, ids


def _search(capfd, ix, ids, q, ref):
    """one search compared with the first len(q) queries of the reference; -> (stats, queries the RDX_DEBUG_HITS lines count as spilled,
    or None when the search printed no such line)"""
    capfd.readouterr()
    gs, gr, gc = ix.search(q, K)
    st = ix.last_stats()
    found = re.findall(r"hits max (\d+) spilled (\d+)", capfd.readouterr().err)
    spilled = sum(int(b) for _, b in found) if found else None
    es, er, ec = (a[:q.shape[0]] for a in ref)
    np.testing.assert_array_equal(gc, ec)
    np.testing.assert_array_equal(gs.view(np.uint32), es.view(np.uint32))
    np.testing.assert_array_equal(gr, np.where(er >= 0, ids[np.maximum(er, 0)], -1))
    return st, spilled


@pytest.mark.parametrize("mapped", [True, False], ids=["id_map", "row_base"])
@pytest.mark.parametrize("d", DIMS)
def test_f16_spill_list_then_fallback(oracle, capfd, d, mapped):
    """the two crowds and an ordinary query on the fp16 pass: from the spill list, then (no spill list, the automatic LDS list of
    1 024 entries) through the fallback passes, whose exact scan ends in k_select_dense"""
    corpus, q, ref = _data(oracle, d)
    ix, ids = _index(corpus, mapped)
    for name, v in (("force_fast", 1), ("spec_tau", 0), ("refine_spill", 1), ("refine_list", 32)):
        ix.set_option(name, v)
    st, spilled = _search(capfd, ix, ids, q[:3], ref)
    assert spilled is not None, "the library did not print its RDX_DEBUG_HITS line"
    assert st["path"] == 0 and st["coarse_bits"] == 16 and spilled >= 1, (st, spilled)
    assert st["retried_queries"] == 0 and st["exact_queries"] == 0, st
    ix.set_option("refine_spill", 0)
    ix.set_option("refine_list", 0)
    st, spilled = _search(capfd, ix, ids, q[:3], ref)
    assert spilled is not None, "the library did not print its RDX_DEBUG_HITS line"
    assert st["path"] == 0 and spilled == 0, (st, spilled)
    assert st["retried_queries"] >= 1 or st["exact_queries"] >= 1, st
    ix.close()


@pytest.mark.parametrize("pilot", [0, 4])
@pytest.mark.parametrize("mapped", [True, False], ids=["id_map", "row_base"])
@pytest.mark.parametrize("d", DIMS)
def test_i8(oracle, capfd, d, mapped, pilot):
    """129 queries with the int8 pass asked for: the crowds are re-scored in place in the LDS list (the crowded band), in one band
    and behind a pilot round"""
    corpus, q, ref = _data(oracle, d)
    ix, ids = _index(corpus, mapped)
    ix.set_option("coarse_i8", 1)
    ix.set_option("refine_pilot", pilot)
    st, _ = _search(capfd, ix, ids, q, ref)
    assert st["path"] == 0 and st["coarse_bits"] == (8 if d <= I8_MAX_DIM else 16), st
    if d <= I8_MAX_DIM:   # every row of both crowds lies inside its query's band: identical rows, and copies 1e-6 apart in cosine
        assert st["rescored"] >= 1500 + 1200, st
    ix.close()


@pytest.mark.parametrize("mapped", [True, False], ids=["id_map", "row_base"])
@pytest.mark.parametrize("d", DIMS)
def test_exact(oracle, capfd, d, mapped):
    corpus, q, ref = _data(oracle, d)
    ix, ids = _index(corpus, mapped)
    ix.set_option("force_exact", 1)
    st, _ = _search(capfd, ix, ids, q[:3], ref)
    assert st["path"] == 1, st
    ix.close()
