"""CPU: the reranker head's model (tests/rerank_head_model.py) against the two bounds the GPU tests hold the kernel to, and proof that
the exact probes bite: the documented order stays inside `tight` on exact_probe and inside the derived bound on random inputs, while
every named mutant of it leaves `tight` by a factor of at least 100. One test records why the probes exist: on the random inputs
of test_gpu_reranker's comparison an fp16 accumulator stays INSIDE the derived bound.

Ratios max(err / tight) on exact_probe(H, 6, 0), measured with this file (`pytest -s -k report`):

    H     faithful  fp16_acc  fp16_lanes  drop_round  swap_features  pair_rows  skip_bd
    64    0.54      1.7e5     0.54        4.5e6       9.7e6          7.9e6      6.8e6
    512   0.70      1.8e6     1.2e6       2.8e8       2.7e7          1.5e7      2.1e6
    768   0.75      1.8e6     1.5e6       2.0e8       4.1e7          2.3e8      1.8e6
    1024  0.61      1.5e6     3.8e5       1.7e7       3.0e7          1.8e7      2.8e6
    1088  0.72      1.6e6     1.0e6       3.9e9       6.5e6          7.0e9      2.7e6
    2048  0.44      6.2e5     2.9e5       5.8e7       1.1e7          1.1e7      3.0e6
    4096  0.50      2.7e6     1.3e6       5.9e8       9.1e6          1.6e7      2.0e6

(fp16_lanes rounds the lane sums only: at H = 64 a lane holds one product and the mutant changes nothing on the probe; fp16_acc rounds
the butterfly's sums too and bites from H = 64 up.)
"""
import functools
import os
import sys

import numpy as np
import pytest

from rag_dpo_amd import reranker as RR

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import rerank_head_model as M  # noqa: E402

HIDDEN = (64, 512, 768, 1024, 1088, 2048, 4096)                              # the GPU tests' list
PROBE_ROWS = 6                                                               # three row pairs: pair_rows has something to change
FLOOR = 100.0                                                                # mutants leave `tight` by at least this factor


def ratio(got, want, bound):
    """max(err / bound); a NaN score counts as an infinite error"""
    return float(np.nan_to_num(np.abs(np.asarray(got, dtype=np.float64) - want) / bound, nan=np.inf).max())


@functools.lru_cache(maxsize=None)
def probe_ratios(H):
    p = M.exact_probe(H, PROBE_ROWS, 0)
    want, tight = M.tight_reference(*p)
    return {m: ratio(M.kernel_order(*p, mutant=m), want, tight) for m in (None,) + M.MUTANTS}


@pytest.mark.parametrize("H", HIDDEN)
def test_documented_order_is_inside_tight_on_the_exact_probes(H):
    assert probe_ratios(H)[None] <= 1.0, probe_ratios(H)
    for n in (1, 2):                                                         # the GPU test's other row counts (65 is 6 rows many times over)
        p = M.exact_probe(H, n, 1)
        want, tight = M.tight_reference(*p)
        assert ratio(M.kernel_order(*p), want, tight) <= 1.0, (H, n)


@pytest.mark.parametrize("H", HIDDEN)
def test_every_mutant_leaves_tight_by_a_factor_of_100(H):
    r = probe_ratios(H)
    for m in M.MUTANTS:                                                      # each of them changes something at every H (6 rows, H >= 64) ...
        if (m, H) == ("fp16_lanes", 64):
            # ... but this one: a lane holds ONE product there, the plain products have at most 10 bits and the carriers' two roundings
            # cancel. fp16_acc, which also rounds the butterfly, is the mutant that bites at H = 64
            assert r[m] == r[None]
            continue
        assert r[m] >= FLOOR, (H, m, r[m])


@pytest.mark.parametrize("H", HIDDEN)
def test_documented_order_is_inside_the_derived_bound_on_random_inputs(H):
    w = M.random_head(H, H)
    for n, cls in M.random_rows(H, (1, 3) if H > 1024 else (1, 3, 40)):
        want, bound = M.reference(cls, *w)
        r = ratio(M.kernel_order(cls, *w), want, bound)
        assert r <= 1.0, (H, n, r)
        tight = M.tight_reference(cls, *w)[1]
        assert (tight <= bound).all()                                        # tight is the derived bound without its z term


def test_an_fp16_accumulator_hides_inside_the_derived_bound_on_random_inputs():
    """The finding behind the exact probes: at H = 1024, n = 40, the inputs of test_head_against_fp64_with_derived_bound, lane
    accumulators rounded to fp16 after every k-step (fp16_lanes) stay inside the worst-case bound: measured 0.758 of it, the documented
    order 0.0002. With the butterfly's sums rounded as well (fp16_acc) the worst row is at 1.35: caught, by a third. At H = 2048 both
    hide (0.62 and 0.85). If the derived bound is ever tightened below that, this test says so and wants an update."""
    H = 1024
    w = M.random_head(H, H)
    cls = dict(M.random_rows(H, (1, 3, 40)))[40]
    want, bound = M.reference(cls, *w)
    faithful = ratio(M.kernel_order(cls, *w), want, bound)
    mutant = ratio(M.kernel_order(cls, *w, mutant="fp16_lanes"), want, bound)
    both = ratio(M.kernel_order(cls, *w, mutant="fp16_acc"), want, bound)
    print(f"H = 1024, n = 40, random inputs: max(err / derived bound) documented order {faithful:.4f}, fp16_lanes {mutant:.4f}, fp16_acc {both:.4f}")
    assert faithful < 0.05 and 0.1 < mutant < 1.0, (faithful, mutant)
    assert both < 10.0                                                       # (no margin to speak of either: tight rejects it by 1.5e6)


def test_exact_probe_is_what_it_says():
    for H in (64, 128, 1088):
        pairs = M.carrier_columns(H)
        assert (9, 41) in pairs and any(k % 64 == k2 % 64 and k != k2 for k, k2 in pairs) == (H >= 128)
        assert any((k ^ k2) % 64 not in (0, 32) for k, k2 in pairs)
        cls, wd, bd, wo, bo = M.exact_probe(H, 3, 2)
        assert cls.dtype == np.float32 and all(t.dtype == np.float16 for t in (wd, bd, wo, bo))
        for k, k2 in pairs:
            assert np.array_equal(wd[:, k], wd[:, k2]) and np.array_equal(cls[:, k], -cls[:, k2]) and (np.abs(cls[:, k]) >= 64).all()
        assert np.array_equal(cls * 16, np.round(cls * 16)) and np.array_equal(wd.astype(np.float64) * 64, np.round(wd.astype(np.float64) * 64))
        z = cls.astype(np.float64) @ wd.astype(np.float64).T + bd.astype(np.float64)
        assert (np.abs(z) < 3).mean() > 0.97                                 # tanh does not hide an error in z
    assert M.significant_bits([3 * M.GRID, 1.0 + M.GRID, 4.0]) == 11 and M.significant_bits([0.0]) == 0


def test_report_ratios():
    print("\nmax(err / tight) on exact_probe(H, 6, 0)")
    print("H     " + "  ".join(f"{str(m or 'faithful'):>13}" for m in (None,) + M.MUTANTS))
    for H in HIDDEN:
        r = probe_ratios(H)
        print(f"{H:<6}" + "  ".join(f"{r[m]:13.3g}" for m in (None,) + M.MUTANTS))


# ---- selection -----------------------------------------------------------------------------------------------------------------------

def test_select_model_equals_select_host_without_nan():
    rng = np.random.default_rng(21)
    for it in range(200):
        n = int(rng.choice([1, 2, 3, 4, 17, 64, 65, 300]))
        levels = np.asarray([0.0, -0.0, 0.1, 0.3, 0.7, 0.7, 0.95], dtype=np.float32)
        scores = levels[rng.integers(0, len(levels), n)] if it % 3 else rng.uniform(0, 1, n).astype(np.float32)
        boosts = rng.choice([0.15, 0.05, -0.1, 0.0, 0.6], n) if it % 2 else None
        top_k = int(rng.choice([0, 1, 3, n, n + 5]))
        keep_min = int(rng.choice([0, 1, 3, n, n + 1]))
        min_score = float(rng.choice([0.08, 0.0, 0.3, 0.7, 2.0]))
        want = RR.select_host(scores, boosts, top_k, min_score, keep_min)
        got = M.select_model(scores, boosts, top_k, min_score, keep_min)
        assert got[0] == want[0] and got[2] == want[2], (it, n, top_k, keep_min)
        assert np.array_equal(np.asarray(got[1]).view(np.int64), np.asarray(want[1]).view(np.int64)), it


def test_select_model_puts_nan_last_in_input_order():
    nan = float("nan")
    order, final, count = M.select_model([0.5, nan, 0.9, nan, 0.5, 0.1], [0.0, 0.5, nan, 0.2, -1.0, 0.45], 4, 0.5, 3)
    assert order == [2, 5, 0, 4, 1, 3]                                       # 0.9 (a NaN boost adds nothing), 0.55, the 0.5 tie, NaN, NaN
    assert final[2] == float(np.float32(0.9)) and final[5] == float(np.float32(0.1)) + 0.45 and final[1] != final[1] and final[3] != final[3]
    assert count == 4
    assert M.select_model([nan, nan], None, 5, 0.0, 3)[0::2] == ([0, 1], 0)  # nothing passes, and n < keep_min
    assert M.select_model([nan, nan, nan], None, 0, 0.0, 3)[2] == 3          # keep_min lifts the count even over NaN finals
