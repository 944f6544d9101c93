"""The int8 main scan (option coarse_i8, DESIGN.md §5 "int8 coarse pass") against the CPU oracle: it only widens the band the
exact fp64 re-score sees, so ids and score bits must equal the oracle's — through a `where` bitmap, after update / compact, on a
compact bf16 master, with the fused and the stand-alone emit check, with the speculative and the proven threshold — and a
threshold built to fail its verification must be answered exactly by the fallback passes."""
import numpy as np
import pytest

from rag_dpo_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from rag_dpo_amd import engine
    return engine


def _index(eng, corpus, **opts):
    ix = eng.HipIndex(corpus.shape[1])
    ix.set_option("coarse_i8", 1)
    ix.add(corpus)
    for k, v in opts.items():
        ix.set_option(k, v)
    return ix


def _check(oracle, ix, corpus, q, k, allow=None, bits=8, fallback_ok=False):
    """oracle-equal answers from the coarse pass named by `bits` — and, unless the case is built to fail, answered by that pass
    itself: the fallback passes (fp16 second pass, exact scan) are oracle-exact on their own and would hide a broken int8 pass"""
    es, er, ec = oracle.cosine_topk(oracle.normalize_rows(corpus), q, k, allow)
    gs, gr, gc = ix.search(q, k, oracle.pack_mask(allow, corpus.shape[0]))
    st = ix.last_stats()
    np.testing.assert_array_equal(gc, ec)
    np.testing.assert_array_equal(gr, er)
    np.testing.assert_array_equal(gs, es)
    assert st["coarse_bits"] == bits and st["path"] == 0, st
    if not fallback_ok:
        assert st["exact_queries"] == 0 and st["retried_queries"] == 0, st
    return st


@pytest.fixture(scope="module")
def data():
    corpus = synth.make_corpus(60_000, 1024)
    return corpus, synth.make_queries(1100, 1024, corpus)


@pytest.mark.parametrize("nq", [257, 512, 1024, 1100])
def test_batch_sizes(eng, oracle, data, nq):
    corpus, q = data
    ix = _index(eng, corpus)
    _check(oracle, ix, corpus, q[:nq], 10)
    ix.close()


@pytest.mark.parametrize("fuse", [0, 1])
@pytest.mark.parametrize("spec", [0, 1])
def test_options(eng, oracle, data, fuse, spec):
    corpus, q = data
    ix = _index(eng, corpus, fuse_epilogue=fuse, spec_tau=spec)
    _check(oracle, ix, corpus, q[:300], 10)
    ix.close()


def test_where_bitmap(eng, oracle, data):
    corpus, q = data
    ix = _index(eng, corpus)
    allow = np.random.default_rng(4).random(corpus.shape[0]) < 0.4
    _check(oracle, ix, corpus, q[:520], 10, allow)
    ix.close()


def test_default_keeps_fp16_below_the_row_gate(eng, oracle, data):
    corpus, q = data
    ix = eng.HipIndex(1024)
    ix.add(corpus)
    _check(oracle, ix, corpus, q[:600], 10, bits=16)          # auto: fewer than 2^20 rows
    ix.set_option("coarse_i8", 1)
    _check(oracle, ix, corpus, q[:600], 10, bits=8)
    _check(oracle, ix, corpus, q[:100], 10, bits=16)          # one query tile of <= 128: fp16 whatever the option
    ix.close()


def test_update_append_compact(eng, oracle, data):
    """the int8 copy follows every write: it is built lazily, an append re-quantises the last partial block and the new ones, an
    update or a compaction the whole copy"""
    corpus, q = data
    ref = corpus[:50_017].copy()
    ix = _index(eng, ref)
    _check(oracle, ix, ref, q[:300], 10)
    ix.add(corpus[50_017:])
    ref = corpus.copy()
    _check(oracle, ix, ref, q[:300], 10)
    rng = np.random.default_rng(9)
    rows = np.array([5, 31, 32, 40_000, 59_999])
    new = q[:5] + 0.01 * rng.standard_normal((5, 1024)).astype(np.float32)   # near copies of queries: they must be found
    ix.update(rows, new)
    ref[rows] = new
    _check(oracle, ix, ref, q[:300], 10)
    dead = np.zeros(ref.shape[0], bool)                    # a delete is a tombstone in the row bitmap until the compaction
    dead[np.arange(100, ref.shape[0], 7)] = True
    dead[rows] = True                                      # (including the rows the queries' near copies went to)
    _check(oracle, ix, ref, q[:300], 10, ~dead)
    keep = np.flatnonzero(~dead)
    ix.compact(keep)
    _check(oracle, ix, ref[keep], q[:300], 10)
    ix.close()


def test_compact_bf16_master(eng, oracle, data):
    import torch
    corpus, q = data
    cb = torch.from_numpy(corpus).to(torch.bfloat16)
    wide = cb.to(torch.float32).numpy()
    ix = eng.HipIndex(1024)
    ix.set_option("compact_master", 1)
    ix.set_option("coarse_i8", 1)
    ix.add_bf16(cb)
    _check(oracle, ix, wide, q[:300], 10)
    ix.close()


def test_failed_verification_falls_back(eng, oracle):
    """a corpus built to fool the speculative threshold (tests/test_gpu_parity.py::test_speculative_threshold_is_verified): the
    queries fail the int8 verification X - E_q >= T, take the fallback passes and still get the oracle's answers. (The int8 pass
    samples 8x more densely than sample_div asks: 2.2 M rows at sample_div 256 keep the sample thin enough to speculate.)"""
    n, d, k = 2_200_000, 128, 10
    rng = np.random.default_rng(77)
    corpus = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((160, d)).astype(np.float32)
    for j in range(8):                                     # tile 0 (in every whole-tile sample): each of the 32 bootstrap sets of its
        for g in range(4):                                 # 8 waves x 4 lane groups holds one near copy of each of the first 3 queries
            corpus[32 * j + 4 * g: 32 * j + 4 * g + 3] = q[:3] + 0.05 * rng.standard_normal((3, d)).astype(np.float32)
    ix = _index(eng, corpus, spread_boot=0, sample_div=256)   # (the speculative rank is then 9: T = the 9th best near copy > the 10th)
    st = _check(oracle, ix, corpus, q, k, fallback_ok=True)
    assert st["tau_rank"] < k and st["retried_queries"] >= 3, st
    ix.close()


def test_lane_map_counts_exact():
    """The int8 lane map with exact integer data (cdna_hip_programming.md §3): every row has 16 entries +-1 at distinct dimensions,
    so its normalised elements are +-0.25 exactly and every block's scale quantises them to +-127 (error below 1e-9); query j is the
    unit vector e_j (q8 = 127 e_j). The int8 dot product is then 127^2 times the row's entry at dimension j, the coarse scores sit on
    the levels +-0.25 and 0, and whatever the threshold sample, the emitted and the re-scored rows of query j are exactly the rows with
    +1 at dimension j. A corpus fragment and a query image that disagree on where a dimension sits move those counts."""
    from rag_dpo_amd import engine as eng
    rng = np.random.default_rng(21)
    n, d, k = 60_000, 1024, 10
    corpus = np.zeros((n, d), np.float32)
    for r in range(n):
        corpus[r, rng.choice(d, 16, replace=False)] = rng.choice([-1.0, 1.0], 16)
    q = np.eye(d, dtype=np.float32)                       # all 1024 dimensions: every lane, chunk, swizzle slot and k-step
    plus = (corpus > 0).sum(axis=0)
    assert plus.min() > k and plus.max() < 1024          # k tied rows exist for every query, the band fits the ranking arrays
    ix = eng.HipIndex(d)
    ix.set_option("coarse_i8", 1)
    ix.add(corpus)
    s, r, c = ix.search(q, k)
    st = ix.last_stats()
    assert st["coarse_bits"] == 8 and st["exact_queries"] == 0 and st["retried_queries"] == 0, st
    assert st["emitted"] == plus.sum() and st["rescored"] == plus.sum(), (st, plus.sum())
    for j in range(d):                                    # ties at 0.25: the k lowest row ids with +1 at dimension j
        np.testing.assert_array_equal(r[j], np.flatnonzero(corpus[:, j] > 0)[:k])
    assert (s == np.float32(0.25)).all() and (c == k).all()
    ix.close()
