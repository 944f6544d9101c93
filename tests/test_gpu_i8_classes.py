"""The int8 scan's classes of block error (option i8_eps_classes, DESIGN.md §5 "classes of eps_b") on the GPU against their model
(tests/i8_class_model.py). Every index runs with coarse_i8 = 1 (forced int8: one class unless the option says otherwise), spec_tau = 0,
refine_pilot = 1 and the final row count reserved, and every search runs twice on the same index, with i8_eps_classes = 1 and = 8. Both
times it must
  * return the C oracle's ids, counts and score bits,
  * answer by the int8 pass alone (coarse_bits 8, path 0, no query retried, none left to the exact scan),
  * emit exactly the rows the model counts — with one class that is the model of the scan as it was before the classes
    (tests/test_i8_class_model.py holds its thresholds to i8_model's E_q, bit for bit) — and re-score exactly the rows the model counts;
and with 8 classes `emitted` must be strictly smaller while `rescored` is the same.

The corpora (9 000 - 15 000 rows; i8_class_model.Case) make the threshold known exactly: k = 1, every query's best row is an exact copy
of it whose fp16 coarse score is exactly 1, and the whole corpus is the threshold sample, so T = fl32(1 - 2E). Half the blocks hold one
spiky row (a large s_b and eps_b, graded over a factor 2: all 8 classes are populated), half are flat; near copies of the queries are
planted around T - E_q, where the classes decide. The cases: dims 128 (one k-step), 896 (7 k-steps) — both run the variant with the
stand-alone emit check, which the build carries with all 8 classes like the fused one — and 1024 (8 k-steps, fused; and with
fuse_epilogue = 0); 129 / 257 / 1 030 queries; a `where` bitmap on either variant; a ragged last block that alone carries eps_max; an
append onto a partial block; an appended block above the top edge (its class's edge is the running eps_max); an update that raises
eps_max and one that lowers it again; a compaction; the compact bf16 master; all-zero blocks. Last, a speculative threshold built to
fail its verification: with 8 classes too the queries take the fallback passes and the answers are the oracle's."""
import numpy as np
import pytest

import i8_class_model as CM

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from rag_dpo_amd import engine
    return engine


def _replay(eng, oracle, case, script, **options):
    import torch
    steps = case.design(script)
    ix = eng.HipIndex(case.d)
    for name, v in {"coarse_i8": 1, "spec_tau": 0, "refine_pilot": 1, **case.options, **options}.items():
        ix.set_option(name, v)
    ix.reserve(case.n)
    try:
        for s in steps:
            for op, args in s.ops:
                if op == "add" and case.bf16:
                    op, args = "add_bf16", (torch.from_numpy(args[0]).to(torch.bfloat16),)
                getattr(ix, op)(*args)
            n = len(ix)
            assert n == len(s.raw)
            got = {}
            for C in (1, 8):
                ix.set_option("i8_eps_classes", C)
                gs, gr, gc = ix.search(case.q, 1, oracle.pack_mask(s.allow, n))
                st = got[C] = ix.last_stats()
                print(f"{s.name}: {C} class(es): emitted {st['emitted']} (model {s.want[C][0]}) rescored {st['rescored']} (model {s.want[C][1]}) "
                      f"exact {st['exact_queries']} retried {st['retried_queries']}; classes in use {s.cls_used}, eps_max {s.eps_max:.5f}")
                np.testing.assert_array_equal(gc, s.ec)
                np.testing.assert_array_equal(gr, s.er)
                np.testing.assert_array_equal(gs.view(np.uint32), s.es.view(np.uint32))
                assert st["coarse_bits"] == 8 and st["path"] == 0, st
                assert st["exact_queries"] == 0 and st["retried_queries"] == 0, st
                assert st["emitted"] == s.want[C][0], (C, st, s.want)
                assert st["rescored"] == s.want[C][1], (C, st, s.want)
            assert got[8]["emitted"] < got[1]["emitted"] and got[8]["rescored"] == got[1]["rescored"], got
            assert len(s.cls_used) == 8, s.cls_used                       # every class holds a block
    finally:
        ix.close()
    return steps


@pytest.mark.parametrize("d,fuse", [(128, 1), (896, 1), (1024, 1), (1024, 0)])
def test_dims(eng, oracle, d, fuse):
    _replay(eng, oracle, CM.Case(oracle, d, 9000 + 13 + d % 64, 257, seed=d), CM.script_plain(), fuse_epilogue=fuse)


@pytest.mark.parametrize("nq", [129, 1030])
def test_query_tiles(eng, oracle, nq):
    """one padded tile of 256, and five tiles (the last of 6 queries); 257 runs in every other case"""
    _replay(eng, oracle, CM.Case(oracle, 256, 11000 + 7, nq, seed=nq), CM.script_plain())


@pytest.mark.parametrize("d", [256, 896])
def test_where_bitmap(eng, oracle, d):
    """40 % of the rows allowed (the anchors all, one spiky block not at all): the fused and the stand-alone check with a bitmap"""
    _replay(eng, oracle, CM.Case(oracle, d, 9000 + 13, 257, seed=5 + d), CM.script_plain(0.4, 4))


def test_ragged_last_block_alone_carries_eps_max(eng, oracle):
    case = CM.Case(oracle, 256, 9000 + 13, 257, seed=6, z_top=1.03)
    steps = _replay(eng, oracle, case, CM.script_plain())
    eps = CM.M.quant_blocks(case.norm(steps[0].raw))[2]
    assert len(steps[0].raw) % 32 == 21 and eps[-1] > eps[:-1].max() and np.float32(steps[0].eps_max) == eps[-1]


def test_append_onto_a_partial_block(eng, oracle):
    _replay(eng, oracle, CM.Case(oracle, 256, 12000 + 13, 257, seed=7), CM.script_append(9000 + 13))


def test_appended_block_above_the_top_edge(eng, oracle):
    n0 = 9000 + 13
    case = CM.Case(oracle, 256, 12000 + 13, 257, seed=8, z_top=1.03, top_block=(n0 + 31) // 32 + 20)
    steps = _replay(eng, oracle, case, CM.script_append(n0))
    assert steps[1].eps_max > steps[0].eps_max                            # the appended spike raised the running eps_max


def test_update_raises_then_lowers_eps_max(eng, oracle):
    case = CM.Case(oracle, 256, 9000 + 13, 257, seed=9)
    steps = _replay(eng, oracle, case, CM.script_update(32 * ((257 + 31) // 32) + 64 + 5, 1.03))
    assert steps[1].eps_max > steps[0].eps_max == steps[2].eps_max


def test_compact(eng, oracle):
    _replay(eng, oracle, CM.Case(oracle, 256, 9000 + 13, 257, seed=10), CM.script_compact(7))


def test_compact_bf16_master(eng, oracle):
    _replay(eng, oracle, CM.Case(oracle, 256, 9000 + 13, 257, seed=11, bf16=True, compact_master=1), CM.script_plain())


def test_zero_blocks(eng, oracle):
    _replay(eng, oracle, CM.Case(oracle, 256, 9000 + 13, 257, seed=12, zero_blocks=2), CM.script_plain())


def test_failed_verification_falls_back_with_classes(eng, oracle):
    """the corpus of tests/test_gpu_scan_i8.py::test_failed_verification_falls_back, built to fool the speculative threshold: with 8
    classes the queries fail the verification X - E_q >= taus8 just the same, take the fallback passes and get the oracle's answers"""
    n, d, k = 2_200_000, 128, 10
    rng = np.random.default_rng(77)
    corpus = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((160, d)).astype(np.float32)
    for j in range(8):
        for g in range(4):
            corpus[32 * j + 4 * g: 32 * j + 4 * g + 3] = q[:3] + 0.05 * rng.standard_normal((3, d)).astype(np.float32)
    ix = eng.HipIndex(d)
    for name, v in {"coarse_i8": 1, "i8_eps_classes": 8, "spread_boot": 0, "sample_div": 256}.items():
        ix.set_option(name, v)
    ix.add(corpus)
    try:
        es, er, ec = oracle.cosine_topk(oracle.normalize_rows(corpus), q, k)
        gs, gr, gc = ix.search(q, k)
        st = ix.last_stats()
        np.testing.assert_array_equal(gc, ec)
        np.testing.assert_array_equal(gr, er)
        np.testing.assert_array_equal(gs, es)
        assert st["coarse_bits"] == 8 and st["path"] == 0, st
        assert st["tau_rank"] < k and st["retried_queries"] >= 3, st
    finally:
        ix.close()
