"""The int8 coarse pass against its model (tests/i8_model.py) on the GPU: across the widths (every k-step count of k_scan<I8>'s
4-slot ring, padded columns), ragged last blocks and tiles, the query-tile shapes, a `where` bitmap, append / update / compact, the
compact bf16 master and zeros. Every index runs with coarse_i8 = 1, spec_tau = 0 and the final row count reserved; only queries that
qualify by the model alone are sent, and every search must
  * return the C oracle's ids, counts and score bits,
  * answer by the int8 pass alone (coarse_bits 8, path 0, no query retried, none left to the exact scan),
  * re-score exactly the rows the model counts: st["rescored"] == sum over the queries of |{coarse >= X1 - E_q}|.
The last is what pins s_b, eps_b, e_q, n_q and eps_max: tests/test_i8_model.py shows, case by case, that an E_q twice as wide, a
neighbour's E_q, a missing n_q eps_max term, an eps_max that ignores the ragged block or is stale after a write, a partial block left
alone by an append and a scale taken from the neighbouring block would each count differently. `emitted` is not asserted (the fp16
bootstrap's threshold is not modelled).

Zero queries: a zero query scores 0 on every row, so every row is a hit — more than the refine list holds (REFINE_LIST < n) — and
by design the query is handed to the second pass, which serves two queries on a corpus this small with the exact scan. That search
therefore asserts retried_queries == exact_queries == 2 (the zero queries and nobody else) in place of 0; `rescored` is still the
model's count, since neither an overflowing query nor the exact scan re-scores a band."""
import functools

import numpy as np
import pytest

import i8_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from rag_dpo_amd import engine
    return engine


def _replay(eng, oracle, sc, **options):
    """run the scenario's writes and searches on an index; every search is checked against the oracle and the model"""
    import torch
    ix = eng.HipIndex(sc.d)
    for name, v in {"coarse_i8": 1, "spec_tau": 0, "refine_pilot": sc.pilot, **sc.options, **options}.items():
        ix.set_option(name, v)
    ix.reserve(sc.reserve)
    try:
        for s in sc.searches:
            for op, args in s.ops:
                if op == "add_bf16":
                    args = (torch.from_numpy(args[0]).to(torch.bfloat16),)
                getattr(ix, op)(*args)
            n = len(ix)
            assert n == len(s.y)
            use, zeros = s.pred.use, 0 if s.extra_q is None else len(s.extra_q)
            q, es, er, ec = s.q[use], s.es[use], s.er[use], s.ec[use]
            if zeros:
                assert n > M.REFINE_LIST
                zs, zr, zc = oracle.cosine_topk(s.y, s.extra_q, M.K, s.allow)
                q, es, er, ec = np.concatenate([q, s.extra_q]), np.concatenate([es, zs]), np.concatenate([er, zr]), np.concatenate([ec, zc])
            gs, gr, gc = ix.search(q, M.K, oracle.pack_mask(s.allow, n))
            st = ix.last_stats()
            print(s.pred.line(s.name), "| GPU rescored", st["rescored"], "emitted", st["emitted"], "exact", st["exact_queries"], "retried",
                  st["retried_queries"])
            np.testing.assert_array_equal(gc, ec)
            np.testing.assert_array_equal(gr, er)
            np.testing.assert_array_equal(gs.view(np.uint32), es.view(np.uint32))
            assert st["coarse_bits"] == 8 and st["path"] == 0, st
            assert st["exact_queries"] == zeros and st["retried_queries"] == zeros, st
            assert st["rescored"] == s.pred.want, (st, s.pred.want, s.pred.mutants)
    finally:
        ix.close()


@functools.lru_cache(maxsize=2)
def _width(oracle, d):
    return M.case_width(oracle, d)


@pytest.mark.parametrize("d,fuse", [(d, 1) for d in M.WIDTHS] + [(d, 0) for d in (100, 324, 1024)])
def test_widths(eng, oracle, d, fuse):
    """1, 1, 2, 2, 3, 4, 5, 8, 8 k-steps of 128 dimensions: fewer steps than ring slots, an odd count, padded columns; the
    separate epilogue (fuse_epilogue = 0) as well at dims 100, 324 and 1024"""
    _replay(eng, oracle, _width(oracle, d), fuse_epilogue=fuse)


@pytest.mark.parametrize("r", M.RAGGED)
@pytest.mark.parametrize("d", [256, 1024])
def test_ragged_ends(eng, oracle, d, r):
    _replay(eng, oracle, M.case_ragged(oracle, d, r))


@pytest.mark.parametrize("nq", [129, 256, 257])
def test_query_tiles(eng, oracle, nq):
    _replay(eng, oracle, M.case_qtile(oracle, nq))


def test_query_tiles_1030(eng, oracle):
    _replay(eng, oracle, M.case_qtile(oracle, 1030))


def test_where_bitmap(eng, oracle):
    _replay(eng, oracle, M.case_where(oracle))


def test_append(eng, oracle):
    _replay(eng, oracle, M.case_append(oracle))


def test_update_both_ways(eng, oracle):
    _replay(eng, oracle, M.case_update(oracle))


def test_compact(eng, oracle):
    _replay(eng, oracle, M.case_compact(oracle))


@pytest.mark.parametrize("d", [1024, 256])
def test_compact_bf16_master(eng, oracle, d):
    _replay(eng, oracle, M.case_bf16(oracle, d))


def test_zeros(eng, oracle):
    _replay(eng, oracle, M.case_zeros(oracle))
