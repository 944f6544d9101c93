"""The two-round exact re-score of int8 searches (option refine_pilot, DESIGN.md §5 "two-round re-score") against the CPU oracle
and against its numpy model (tests/test_i8_refine_model.py): ids, score bits and counts do not depend on the pilot — with the
single band (0), the smallest pilot (1) and the default, with the speculative and the proven threshold, through a `where` bitmap,
after append / update / compact, on the compact bf16 master and on a corpus built to fail the verification — and `rescored` is the
model's |S1 u S2| exactly, which a band of 2 E_q, or E_q taken from another query, would move."""
import numpy as np
import pytest

import test_i8_refine_model as RM
from i8_model import coarse_model as _model
from rag_dpo_amd import synth
from test_i8_bound_model import F32

pytestmark = pytest.mark.gpu

PILOTS = [0, 1, None]          # None: the library's default


@pytest.fixture(scope="module")
def eng():
    from rag_dpo_amd import engine
    return engine


@pytest.fixture(scope="module")
def data():
    corpus = synth.make_corpus(60_000, 1024)
    return corpus, synth.make_queries(1100, 1024, corpus)


def _index(eng, corpus, pilot, **opts):
    ix = eng.HipIndex(corpus.shape[1])
    ix.set_option("coarse_i8", 1)
    if pilot is not None:
        ix.set_option("refine_pilot", pilot)
    for k, v in opts.items():
        ix.set_option(k, v)
    ix.add(corpus)
    return ix


def _check(oracle, ix, corpus, q, k, allow=None, fallback_ok=False):
    es, er, ec = oracle.cosine_topk(oracle.normalize_rows(corpus), q, k, allow)
    gs, gr, gc = ix.search(q, k, oracle.pack_mask(allow, corpus.shape[0]))
    st = ix.last_stats()
    np.testing.assert_array_equal(gc, ec)
    np.testing.assert_array_equal(gr, er)
    np.testing.assert_array_equal(gs, es)
    assert st["coarse_bits"] == 8 and st["path"] == 0, st
    if not fallback_ok:
        assert st["exact_queries"] == 0 and st["retried_queries"] == 0, st
    return st


@pytest.mark.parametrize("spec", [0, 1])
@pytest.mark.parametrize("pilot", PILOTS)
@pytest.mark.parametrize("nq", [257, 1100])
def test_parity_pilot_and_threshold(eng, oracle, data, nq, pilot, spec):
    corpus, q = data
    ix = _index(eng, corpus, pilot, spec_tau=spec)
    st = _check(oracle, ix, corpus, q[:nq], 10)
    print(f"nq {nq} pilot {pilot} spec_tau {spec}: emitted/query {st['emitted'] / nq:.1f} rescored/query {st['rescored'] / nq:.1f}")
    ix.close()


def test_pilot_never_rescores_more_than_the_single_band(eng, oracle, data):
    """S1 of the smallest pilot lies inside the single band and t3 >= c_k - 2 E_q: on the same hits, never more rows"""
    corpus, q = data
    got = {}
    for pilot in (0, 1):
        ix = _index(eng, corpus, pilot, spec_tau=0)
        got[pilot] = _check(oracle, ix, corpus, q[:600], 10)
        ix.close()
    assert got[0]["emitted"] == got[1]["emitted"], got           # the pilot does not change what the scan emits
    assert got[1]["rescored"] <= got[0]["rescored"], got


@pytest.mark.parametrize("pilot", PILOTS)
def test_where_bitmap(eng, oracle, data, pilot):
    corpus, q = data
    ix = _index(eng, corpus, pilot)
    allow = np.random.default_rng(4).random(corpus.shape[0]) < 0.4
    _check(oracle, ix, corpus, q[:520], 10, allow)
    ix.close()


@pytest.mark.parametrize("k", [1, 100])
def test_other_k(eng, oracle, data, k):
    """k = 100: the default pilot of 400 hits is most of a query's hits, S1 can be every hit (fewer hits than k1)"""
    corpus, q = data
    for pilot in (1, None, 64):
        ix = _index(eng, corpus, pilot)
        _check(oracle, ix, corpus, q[:300], k)
        ix.close()


@pytest.mark.parametrize("pilot", [1, None])
def test_update_append_compact(eng, oracle, data, pilot):
    corpus, q = data
    ref = corpus[:50_017].copy()
    ix = _index(eng, ref, pilot)
    _check(oracle, ix, ref, q[:300], 10)
    ix.add(corpus[50_017:])
    ref = corpus.copy()
    _check(oracle, ix, ref, q[:300], 10)
    rng = np.random.default_rng(9)
    rows = np.array([5, 31, 32, 40_000, 59_999])
    new = q[:5] + 0.01 * rng.standard_normal((5, 1024)).astype(np.float32)
    ix.update(rows, new)
    ref[rows] = new
    _check(oracle, ix, ref, q[:300], 10)
    dead = np.zeros(ref.shape[0], bool)
    dead[np.arange(100, ref.shape[0], 7)] = True
    dead[rows] = True
    _check(oracle, ix, ref, q[:300], 10, ~dead)
    keep = np.flatnonzero(~dead)
    ix.compact(keep)
    _check(oracle, ix, ref[keep], q[:300], 10)
    ix.close()


@pytest.mark.parametrize("pilot", [1, None])
def test_compact_bf16_master(eng, oracle, data, pilot):
    import torch
    corpus, q = data
    cb = torch.from_numpy(corpus).to(torch.bfloat16)
    wide = cb.to(torch.float32).numpy()
    ix = eng.HipIndex(1024)
    ix.set_option("compact_master", 1)
    ix.set_option("coarse_i8", 1)
    if pilot is not None:
        ix.set_option("refine_pilot", pilot)
    ix.add_bf16(cb)
    _check(oracle, ix, wide, q[:300], 10)
    ix.close()


def test_near_duplicates_overflow_the_ranking_arrays(eng, oracle):
    """1 500 near copies of each of 8 directions: the band below X1 holds more rows than the ranking arrays (REFINE_PMAX), S2 is
    re-scored in place and S1 joins it from the arrays; 1 200 IDENTICAL rows tie at every coarse rank (the single-band fallback)"""
    d, k = 1024, 10
    rng = np.random.default_rng(31)
    corpus = synth.make_corpus(40_000, d)
    centres = rng.standard_normal((9, d)).astype(np.float32)
    for c in range(8):
        corpus[2000 * c:2000 * c + 1500] = centres[c] + 0.002 * rng.standard_normal((1500, d)).astype(np.float32)
    corpus[30_000:31_200] = centres[8]
    q = synth.make_queries(300, d, corpus)
    q[:9] = centres + 0.01 * rng.standard_normal((9, d)).astype(np.float32)
    for pilot in (1, None):
        ix = _index(eng, corpus, pilot)
        st = _check(oracle, ix, corpus, q, k, fallback_ok=True)
        print(f"pilot {pilot}: emitted {st['emitted']} rescored {st['rescored']} exact {st['exact_queries']} retried {st['retried_queries']}")
        ix.close()


def test_failed_verification_falls_back(eng, oracle):
    """the corpus of tests/test_gpu_scan_i8.py::test_failed_verification_falls_back: the queries fail X - E_q >= tau after the two
    rounds as they did after one, take the fallback passes and get the oracle's answers"""
    n, d, k = 2_200_000, 128, 10
    rng = np.random.default_rng(77)
    corpus = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((160, d)).astype(np.float32)
    for j in range(8):
        for g in range(4):
            corpus[32 * j + 4 * g: 32 * j + 4 * g + 3] = q[:3] + 0.05 * rng.standard_normal((3, d)).astype(np.float32)
    ix = _index(eng, corpus, None, spread_boot=0, sample_div=256)
    st = _check(oracle, ix, corpus, q, k, fallback_ok=True)
    assert st["tau_rank"] < k and st["retried_queries"] >= 3, st
    ix.close()


@pytest.mark.parametrize("pilot", [1, 4])
def test_rescored_is_the_models_count(eng, oracle, pilot):
    """Where the model says X1 = X (the pilot holds the exact top-k) and at least k1 rows reach t3 = X - E_q, the verified search
    emitted every row with coarse >= t3 (X - E_q >= tau), so S1 u S2 = {coarse >= t3} whatever the threshold was: `rescored` is that
    count summed over the queries, to the row. The queries are chosen by the model alone, before the search."""
    k = 10
    corpus = synth.make_corpus(40_000, 1024, duplicates=False)
    q_all = synth.make_queries(400, 1024, corpus)
    y, qh, coarse, Eq = _model(oracle, corpus, q_all)
    es, er, ec = oracle.cosine_topk(y, q_all, k)
    use, want, wide, other = [], 0, 0, 0
    for i in range(q_all.shape[0]):
        k1 = pilot * k
        top = np.argsort(-coarse[i].astype(np.float64), kind="stable")
        S1 = np.flatnonzero(coarse[i] >= coarse[i][top[k1 - 1]])
        X1 = RM.kth_largest(oracle.scores(y[S1], qh[i]), k)
        t3 = RM.sub_down(X1, Eq[i])
        cnt = int((coarse[i] >= t3).sum())
        if X1 == es[i, k - 1] and cnt >= len(S1):
            use.append(i)
            want += cnt
            wide += int((coarse[i] >= RM.sub_down(X1, F32(2) * Eq[i])).sum())
            other += int((coarse[i] >= RM.sub_down(X1, Eq[(i + 1) % len(Eq)])).sum())
    assert len(use) >= 257, len(use)                     # enough for the int8 path (more than 128 queries)
    assert wide > want + len(use) and other != want, (want, wide, other)   # the mutants would be seen
    ix = _index(eng, corpus, pilot, spec_tau=0)
    gs, gr, gc = ix.search(q_all[use], k)
    st = ix.last_stats()
    np.testing.assert_array_equal(gr, er[use])
    np.testing.assert_array_equal(gs, es[use])
    print(f"pilot {pilot}: {len(use)} queries, rescored {st['rescored']} model {want} (2E_q: {wide}, neighbour's E_q: {other}), emitted {st['emitted']}")
    assert st["coarse_bits"] == 8 and st["path"] == 0 and st["exact_queries"] == 0 and st["retried_queries"] == 0, st
    assert st["rescored"] == want, (st, want, wide, other)
    ix.close()
