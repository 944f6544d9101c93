"""GPU: rdx_maxsim_quantize_i8 (csrc/maxsim_i8_kernel.hpp k_maxsim_quant) against quantize_model (rag_dpo_amd/late_interaction.py,
DESIGN.md §32) — codes and scale bits, no tolerance: every operation of the rule is exact or one IEEE fp64 / fp32 operation."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_late_interaction_i8 import tie_row  # noqa: E402

from rag_dpo_amd import late_interaction as LI  # noqa: E402

pytestmark = pytest.mark.gpu

ROWS = (1, 3, 4, 5, 1000)          # one wave of a workgroup, three, a full workgroup, one more, many workgroups
GUARD = 64


def lib():
    from rag_dpo_amd import _lib
    return _lib, _lib.load()


def rows_of(dim, n=1000):
    """unit rows, rows of every magnitude fp16 has, the tie probe, zero rows and non-finite rows, in the first few rows too"""
    rng = np.random.default_rng(dim)
    v = rng.standard_normal((n, dim))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    v[n // 2:] *= np.exp(rng.uniform(-14, 10, size=(n - n // 2, 1)))
    x = np.clip(v, -65504, 65504).astype(np.float16)
    x[1] = tie_row(dim)
    x[2] = 0
    x[2, dim - 1] = -0.0
    if n > 11:
        x[4, dim // 2] = np.inf
        x[7, 0] = np.nan
        x[8, dim - 1] = -np.inf
        x[9] = tie_row(dim)[::-1]
        x[10] = 65504.0
        x[11] = 0
        x[11, 5] = 6e-8                                            # the smallest fp16 subnormal alone
    return x


def quantize(x, rows=None, stream=None):
    """-> (codes int8 [rows][dim], scales fp32 [rows], the guard bytes behind each) through the C ABI"""
    L, so = lib()
    rows = len(x) if rows is None else rows
    dim = x.shape[1]
    t = torch.from_numpy(x).cuda()
    codes = torch.full((rows * dim + GUARD,), 0x5A, dtype=torch.int8, device="cuda")
    scales = torch.full((rows + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    st = stream if stream is not None else torch.cuda.current_stream()
    rc = so.rdx_maxsim_quantize_i8(0, t.data_ptr(), rows, dim, codes.data_ptr(), scales.data_ptr(), st.cuda_stream)
    assert rc == 0, L.last_error()
    st.synchronize()
    c, s = codes.cpu().numpy(), scales.cpu().numpy()
    return c[:rows * dim].reshape(rows, dim), s[:rows], c[rows * dim:], s[rows:]


@pytest.mark.parametrize("dim", [32, 64, 96, 1024])               # two lanes of a wave, ..., both pieces of every lane
def test_codes_and_scale_bits_equal_the_model(dim):
    x = rows_of(dim)
    wc, ws = LI.quantize_rows_model(x)
    assert ws[1] == np.float32(2.0 ** -10) and wc[1, :6].tolist() == [127, 0, 2, 2, 0, -4]            # the tie probe says what it claims, on the model
    assert not wc[[2, 4, 7, 8]].any() and not ws[[2, 4, 7, 8]].any() and ws[11] > 0
    for rows in ROWS:
        c, s, gc, gs = quantize(x, rows)
        assert c.tobytes() == wc[:rows].tobytes(), (dim, rows, np.argwhere(c != wc[:rows])[:4].tolist())
        assert s.tobytes() == ws[:rows].tobytes(), (dim, rows)                                        # +0.0 for the zero and the non-finite rows, on bits
        assert (gc == 0x5A).all() and np.isnan(gs).all()                                              # nothing behind the outputs is written


def test_engine_wrapper_and_streams():
    from rag_dpo_amd import engine
    x = rows_of(96, 300)
    wc, ws = LI.quantize_rows_model(x)
    t = torch.from_numpy(x).cuda()
    c, s = engine.maxsim_quantize(t)
    assert c.dtype == torch.int8 and s.dtype == torch.float32 and c.cpu().numpy().tobytes() == wc.tobytes() and s.cpu().numpy().tobytes() == ws.tobytes()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c2, s2 = engine.maxsim_quantize(t[5:])                                                        # rows do not depend on their position
    side.synchronize()
    assert c2.cpu().numpy().tobytes() == wc[5:].tobytes() and s2.cpu().numpy().tobytes() == ws[5:].tobytes()
    with pytest.raises(ValueError):
        engine.maxsim_quantize(t[:0])
    with pytest.raises(ValueError):
        engine.maxsim_quantize(t.float())


def test_refusals():
    L, so = lib()
    x = torch.from_numpy(rows_of(64, 8)).cuda()
    codes = torch.full((8 * 64 + 16,), 0x5A, dtype=torch.int8, device="cuda")
    scales = torch.full((9,), float("nan"), dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def rc(vecs=x.data_ptr(), rows=8, dim=64, c=codes.data_ptr(), s=scales.data_ptr(), device=0):
        return so.rdx_maxsim_quantize_i8(device, vecs, rows, dim, c, s, st)

    for kw, word in ((dict(dim=0), "dim"), (dict(dim=16), "dim"), (dict(dim=48), "dim"), (dict(dim=1056), "dim"), (dict(rows=0), "rows"),
                     (dict(rows=-1), "rows"), (dict(rows=1 << 31), "rows"), (dict(vecs=None), "null"), (dict(c=None), "null"), (dict(s=None), "null"),
                     (dict(vecs=x.data_ptr() + 2), "misaligned"), (dict(c=codes.data_ptr() + 8), "misaligned"), (dict(s=scales.data_ptr() + 2), "misaligned"),
                     (dict(device=-1), "device")):
        assert rc(**kw) == L.RDX_ERR_INVALID and word in L.last_error(), (kw, L.last_error())
    torch.cuda.synchronize()
    assert (codes.cpu().numpy() == 0x5A).all() and np.isnan(scales.cpu().numpy()).all()               # nothing was launched
    assert rc() == 0, L.last_error()
    torch.cuda.synchronize()
    assert (codes.cpu().numpy()[8 * 64:] == 0x5A).all() and np.isnan(scales.cpu().numpy()[8:]).all()
