"""plan_forward(): which path the packed encoder takes for a batch, as a table (no GPU: the function is pure), and the one-buffer
serialisation of a small canonical shape's index arrays. A wrong condition here would not fail a GPU test: it would run another kernel
that is also correct, only slower."""
from types import SimpleNamespace

import numpy as np
import pytest

from rag_dpo_amd.packed_encoder import ForwardPlan, _PackedEncoder, canonical, pack_blob, plan_forward, unpack_blob

CAPS = dict(fused=True, small_linear=True, small_stage=True, gemm_shapes=True)
KNOBS = dict(graphs="auto", large_graphs=True, long_attention=True, gemm="blas", GEMM_MIN_TOKENS=1 << 40, MFMA_MIN_TOKENS=1 << 40,
             SMALL_TEXTS=8, SMALL_TOKENS=32, STAGE_TOKENS=32, SMALL_TOKEN_GRANULE=32, LARGE_TOKEN_GRANULE=1024, FUSED_MAX_TOKENS=64)
RDX = dict(gemm="rdx", GEMM_MIN_TOKENS=33)
LENS_13 = np.array([700] * 20 + [152] + [136] * 43)       # row 13's texts: 64 of them, 20 000 tokens (11 blocks of 64 queries each, then 3 each)
BLOCKS_13 = 20 * 11 + 44 * 3

# (row of the issue's table, overrides, (B, T, max_len, blocks), expected plan)
TABLE = [
    (1, {}, (1, 20, 20, 1), ForwardPlan("packed", "stage", "small", ("small", 24, 32), 24, 32, 0)),
    (2, {}, (1, 32, 32, 1), ForwardPlan("packed", "stage", "small", ("small", 32, 32), 32, 32, 0)),
    (3, {}, (4, 30, 10, 4), ForwardPlan("packed", "stage", "small", ("small", 32, 16), 32, 16, 0)),
    (4, {}, (2, 33, 17, 2), ForwardPlan("packed", "blas", "valu", ("small", 64, 32), 64, 32, 0)),
    (5, {}, (8, 192, 24, 8), ForwardPlan("packed", "blas", "valu", ("small", 192, 32), 192, 32, 0)),
    (6, dict(small_stage=False), (1, 20, 20, 1), ForwardPlan("packed", "small", "valu", ("small", 32, 32), 32, 32, 0)),
    (7, dict(graphs=False), (1, 20, 20, 1), ForwardPlan("packed", "stage", "small", None, 20, 20, 0)),
    (8, {}, (9, 200, 30, 9), ForwardPlan("packed", "blas", "valu", None, 200, 30, 0)),
    (9, dict(graphs=True), (9, 200, 30, 9), ForwardPlan("packed", "blas", "valu", (9, 200, 30, 0), 200, 30, 0)),
    (10, {}, (1024, 20649, 40, 1024), ForwardPlan("packed", "blas", "valu", ("large", 1024, 21504, 64), 21504, 64, 0)),
    (11, dict(MFMA_MIN_TOKENS=1024), (1024, 20649, 40, 1024), ForwardPlan("packed", "blas", "mfma", ("large", 1024, 21504, 64), 21504, 64, 2048)),
    (12, dict(large_graphs=False), (1024, 20649, 40, 1024), ForwardPlan("packed", "blas", "valu", None, 20649, 40, 0)),
    (13, {}, (64, 20000, 700, BLOCKS_13), ForwardPlan("packed", "blas", "mfma", None, 20000, 700, BLOCKS_13)),
    (14, dict(long_attention=False), (64, 20000, 700, BLOCKS_13), ForwardPlan("padded", "blas", "sdpa", None, 20000, 700, 0)),
    (15, RDX, (2, 33, 17, 2), ForwardPlan("packed", "rdx", "valu", ("small", 64, 32), 64, 32, 0)),
    (16, RDX, (1, 20, 20, 1), ForwardPlan("packed", "stage", "small", ("small", 24, 32), 24, 32, 0)),
    (17, dict(RDX, long_attention=False), (64, 20000, 700, BLOCKS_13), ForwardPlan("padded", "rdx", "sdpa", None, 20000, 700, 0)),
    # 18: gemm="rdx" with the default GEMM_MIN_TOKENS is the BLAS path everywhere
    (18, dict(gemm="rdx"), (2, 33, 17, 2), ForwardPlan("packed", "blas", "valu", ("small", 64, 32), 64, 32, 0)),
    (18, dict(gemm="rdx"), (1024, 20649, 40, 1024), ForwardPlan("packed", "blas", "valu", ("large", 1024, 21504, 64), 21504, 64, 0)),
    (18, dict(gemm="rdx"), (64, 20000, 700, BLOCKS_13), ForwardPlan("packed", "blas", "mfma", None, 20000, 700, BLOCKS_13)),
    (18, dict(gemm="rdx", long_attention=False), (64, 20000, 700, BLOCKS_13), ForwardPlan("padded", "blas", "sdpa", None, 20000, 700, 0)),
    # 19: without the fused kernels (their capabilities are then all false) every shape is padded, SDPA, BLAS, eager
    (19, dict(fused=False), (1, 20, 20, 1), ForwardPlan("padded", "blas", "sdpa", None, 20, 20, 0)),
    (19, dict(RDX, fused=False, small_linear=False, small_stage=False, gemm_shapes=False, graphs=True), (1024, 20649, 40, 1024),
     ForwardPlan("padded", "blas", "sdpa", None, 20649, 40, 0)),
    # the exact-shape key of graphs=True counts the work units of a batch on the MFMA kernel
    (9, dict(graphs=True), (64, 20000, 700, BLOCKS_13), ForwardPlan("packed", "blas", "mfma", (64, 20000, 700, BLOCKS_13), 20000, 700, BLOCKS_13)),
    # rdx projections follow the PADDED count of a canonical shape (33 real tokens run as 64) and the real count otherwise
    (15, dict(RDX, GEMM_MIN_TOKENS=64), (2, 33, 17, 2), ForwardPlan("packed", "rdx", "valu", ("small", 64, 32), 64, 32, 0)),
    (15, dict(RDX, GEMM_MIN_TOKENS=64, graphs=False), (2, 33, 17, 2), ForwardPlan("packed", "blas", "valu", None, 33, 17, 0)),
]


@pytest.mark.parametrize("row,over,shape,want", TABLE, ids=[f"row{t[0]}-{i}" for i, t in enumerate(TABLE)])
def test_plan_table(row, over, shape, want):
    caps = SimpleNamespace(**{n: over.get(n, v) for n, v in CAPS.items()})
    knobs = SimpleNamespace(**{n: over.get(n, v) for n, v in KNOBS.items()})
    assert set(over) <= set(CAPS) | set(KNOBS)
    assert plan_forward(caps, knobs, *shape) == want


def test_row_13_counts_the_work_units_of_query_blocks():
    first = np.cumsum(LENS_13) - LENS_13
    assert int(LENS_13.sum()) == 20000 and _PackedEncoder._query_blocks(first, LENS_13).shape == (BLOCKS_13, 4)


def test_the_class_defaults_are_the_knobs_of_the_table():
    """an encoder is its own knobs: the names plan_forward() reads exist on the class (values may follow RDX_ENC_* developer knobs)"""
    for n in KNOBS:
        assert hasattr(_PackedEncoder, n), n
    for n in ("SMALL_TEXTS", "SMALL_TOKENS", "STAGE_TOKENS", "SMALL_TOKEN_GRANULE", "LARGE_TOKEN_GRANULE", "FUSED_MAX_TOKENS", "graphs"):
        assert getattr(_PackedEncoder, n) == KNOBS[n], n


@pytest.mark.parametrize("lens,Tp", [([20], 24), ([24] * 8, 192)], ids=["row1", "row5"])
def test_blob_round_trip(lens, Tp):
    lens = np.asarray(lens, dtype=np.int64)
    B, T, n_first, pad = len(lens), int(lens.sum()), _PackedEncoder.SMALL_TEXTS, 1
    first = np.cumsum(lens) - lens
    col = np.arange(T, dtype=np.int64) - np.repeat(first, lens)
    ids = np.random.default_rng(0).integers(4, 1000, T)
    arrays = canonical(ids, col, first, lens, Tp, n_first, pad)
    tok, pos, fst, tf, tl = arrays
    assert (tok[:T] == ids).all() and (tok[T:] == pad).all() and (pos[:T] == col + pad + 1).all() and (pos[T:] == pad + 1).all()
    assert (fst[:B] == first).all() and not fst[B:].any() and len(fst) == n_first
    assert (tf[T:] == np.arange(T, Tp)).all() and (tl[T:] == 1).all() and (tl[:T] == np.repeat(lens, lens)).all()
    blob = pack_blob(arrays)
    assert blob.dtype == np.uint8 and blob.shape == (24 * Tp + 8 * n_first,)
    back = unpack_blob(blob, Tp, n_first)
    assert len(back) == 5
    for a, b in zip(arrays, back):
        assert a.dtype == b.dtype and np.array_equal(a, b)
