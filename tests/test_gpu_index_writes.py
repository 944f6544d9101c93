"""The dense index's write path, row by row (csrc/k_rows.hpp k_normalize<false>, k_reshadow, k_gather_rows, k_gather_raw, k_iota64;
csrc/rdx_index.hip ingest, grow, rdx_index_update*, rdx_index_get, rdx_index_compact, rdx_l2_normalize).

The model is tests/oracle_engine.py::OracleEngine, whose rows are oracle.normalize_rows (fp64, lane order); bf16 input enters the model
as its widened values. Everything is compared bit for bit — rows, ids, score bits, counts — and no tolerance appears anywhere.

check_state runs after every write: the count, get() of EVERY row, and the self-query sweep. The sweep's queries are the model's own
stored rows (k = 3), answered on the exact path, on the fp16 MFMA path (from 256 rows) and on the int8 MFMA path (more than 128
queries, dim_pad a multiple of 128 up to 1024); which of them run is decided by those shape rules, never by what the library chose.
Its precondition is asserted on the ORACLE's answer: every query's first id is its own row and its second score is strictly smaller.
A row whose scan copy (fp16, or int8 built from the master) is stale or misplaced then misses its own query, so every scan-copy row
is observed, not only the ones that happen to land in some query's top-k. Data: synth.make_corpus(n, dim, duplicates=False); updates
write fresh rows of the same distribution from another seed (largest off-diagonal cosine: 0.99982 at 600 x 4, 0.976 at 600 x 8,
0.9972 at 33 000 x 8, at most 0.28 from dim 252 up).

Refused writes: the call raises, the state is bit for bit what it was, and a following valid write lands where it should. Before
rdx_index_update* judged a call's rows ahead of writing them, test_refused_update_nan failed (the good rows of the call were written);
before it refused a repeated id, test_refused_update_repeated_id failed (no error)."""
import ctypes

import numpy as np
import pytest

from rag_dpo_amd import synth

from oracle_engine import OracleEngine

pytestmark = pytest.mark.gpu

K = 3
SWEEP_MAX = 640
DIMS = [4, 8, 60, 64, 68, 252, 256, 260, 1020, 1024, 1028, 4096]   # one live lane; float4 groups ragged at 64 / 256 lanes' worth; the
PIECES = [1, 3, 4, 5, 243, 1, 343]                                  # register / loop boundary of k_normalize (dim/4 <= 256); MAX_DIM
FORMS = ["f32", "bf16", "bf16_compact"]                             # how rows arrive and which master keeps them


# ---- data -----------------------------------------------------------------------------------------------------------------------
def fresh_rows(n, dim, seed):
    """rows of synth.make_corpus's distribution from another seed"""
    return np.random.default_rng([seed, 0]).standard_normal((n, dim), dtype=np.float32)


def to_bf16(x):
    """fp32 -> bf16 patterns, round to nearest even (finite values)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def widen(u16):
    return (np.ascontiguousarray(u16, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same_bits(got, want, what):
    np.testing.assert_array_equal(bits(got), bits(want), err_msg=what)


# ---- the index under test and its calls that engine.HipIndex does not wrap ----------------------------------------------------------
def new_index(dim, form="f32", **options):
    from rag_dpo_amd import engine
    ix = engine.HipIndex(dim)
    if form == "bf16_compact":
        ix.set_option("compact_master", 1)
    for name, value in options.items():
        ix.set_option(name, value)
    return ix


def update_device(ix, ids, rows, stored=False):
    """rdx_index_update / _update_stored with RDX_DEVICE ids and rows (HipIndex.update is host only)"""
    import torch
    from rag_dpo_amd import _lib as L
    dev = f"cuda:{ix.device}"
    d_ids = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int64)).to(dev)
    d_rows = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float32)).to(dev)
    torch.cuda.synchronize()
    fn = ix._lib.rdx_index_update_stored if stored else ix._lib.rdx_index_update
    L.check(fn(ix._h, ctypes.c_void_p(d_ids.data_ptr()), ctypes.c_void_p(d_rows.data_ptr()), d_ids.numel(), L.RDX_DEVICE))


def get_device(ix, ids):
    """rdx_index_get with RDX_DEVICE ids and output"""
    import torch
    dev = f"cuda:{ix.device}"
    d_ids = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int64)).to(dev)
    out = torch.empty((d_ids.numel(), ix.dim), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ix.get_device(d_ids, out)
    return out.cpu().numpy()


def normalize_device(x, side_stream=False):
    """rdx_l2_normalize with RDX_DEVICE pointers, on the default stream or on a stream of its own"""
    import torch
    from rag_dpo_amd import _lib as L
    lib = L.load(require_gpu=True)
    d_in = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to("cuda:0")
    d_out = torch.empty_like(d_in)
    torch.cuda.synchronize()                       # the input is in place whichever stream the call runs on
    st = torch.cuda.Stream(device="cuda:0") if side_stream else None
    L.check(lib.rdx_l2_normalize(0, ctypes.c_void_p(d_in.data_ptr()), d_in.shape[0], d_in.shape[1], ctypes.c_void_p(d_out.data_ptr()),
                                 L.RDX_DEVICE, ctypes.c_void_p(st.cuda_stream) if st is not None else None))
    return d_out.cpu().numpy()                     # (the call returns with its stream drained: include/rdx.h)


def normalize_host(x):
    from rag_dpo_amd import engine
    return engine.l2_normalize(x)


# ---- the writes, applied to the index and to the model alike -------------------------------------------------------------------------
class Pair:
    """one index and its model; `form` decides how rows arrive"""

    def __init__(self, dim, form="f32", **options):
        self.dim, self.form = dim, form
        self.ix = new_index(dim, form, **options)
        self.model = OracleEngine(dim)

    def add(self, raw):
        if self.form == "f32":
            self.ix.add(raw)
            self.model.add(raw)
        else:
            u = to_bf16(raw)
            self.ix.add_bf16(u)
            self.model.add(widen(u))

    def update(self, ids, raw, how="host"):
        if how == "host":
            self.ix.update(ids, raw)
        else:
            update_device(self.ix, ids, raw)
        self.model.update(ids, raw)

    def update_stored(self, ids, rows, how="host"):
        if how == "host":
            self.ix.update_stored(ids, rows)
        else:
            update_device(self.ix, ids, rows, stored=True)
        self.model.rows[np.asarray(ids, dtype=np.int64)] = np.ascontiguousarray(rows, dtype=np.float32)

    def compact(self, keep):
        self.ix.compact(keep)
        self.model.compact(keep)

    def close(self):
        self.ix.close()


# ---- the state check ----------------------------------------------------------------------------------------------------------------
def sweep_modes(n_rows, n_queries, dim):
    """which paths the sweep runs on, by shape alone"""
    dim_pad = (dim + 63) // 64 * 64
    modes = ["exact"]
    if n_rows >= 256:
        modes.append("fast16")
        if n_queries > 128 and dim_pad % 128 == 0 and dim_pad <= 1024:
            modes.append("fast8")
    return modes


def search_in_mode(ix, mode, q):
    opts = {"exact": {"force_exact": 1}, "fast16": {"force_fast": 1}, "fast8": {"force_fast": 1, "coarse_i8": 1}}[mode]
    for name, v in opts.items():
        ix.set_option(name, v)
    try:
        got = ix.search(q, K)
        st = ix.last_stats()
    finally:
        for name in opts:
            ix.set_option(name, 2 if name == "coarse_i8" else 0)      # (the defaults)
    if mode == "exact":
        assert st["path"] == 1, (mode, st["path"])
    else:
        assert st["path"] == 0 and st["coarse_bits"] == (16 if mode == "fast16" else 8), (mode, st["path"], st["coarse_bits"])
    return got


def sweep_rows(n, named=None):
    if named is not None:
        return np.asarray(named, dtype=np.int64)
    assert n <= SWEEP_MAX, "a case with more rows names the rows its sweep queries"
    return np.arange(n, dtype=np.int64)


def sweep(oracle, ix, model, qrows, returned_ids=None, modes=None):
    """the self-query sweep; -> {mode: (scores, ids, counts)} as the index answered"""
    n = len(model)
    q = model.rows[qrows]
    es, er, ec = oracle.cosine_topk(model.rows, q, K)
    # the precondition, on the oracle's answer: a row that is not found by its own query is then the index's fault
    assert (er[:, 0] == qrows).all(), "precondition: a query's best row is not its own"
    if n > 1:
        assert (es[:, 1] < es[:, 0]).all(), "precondition: a query's second score is not strictly below its first"
    want = er if returned_ids is None else np.where(er >= 0, np.asarray(returned_ids)[np.maximum(er, 0)], -1)
    out = {}
    for mode in (modes or sweep_modes(n, len(qrows), model.dim)):
        gs, gr, gc = search_in_mode(ix, mode, q)
        np.testing.assert_array_equal(gc, ec, err_msg=f"{mode}: counts")
        np.testing.assert_array_equal(gr, want, err_msg=f"{mode}: ids")
        assert_same_bits(gs, es, f"{mode}: score bits")
        out[mode] = (gs, gr, gc)
    return out


def check_state(oracle, ix, model, named=None, returned_ids=None, device_get=False):
    n = len(model)
    assert len(ix) == n
    if n == 0:
        return {}
    every = np.arange(n, dtype=np.int64)
    rows = ix.get(every)
    assert_same_bits(rows, model.rows, "get(all rows)")
    if device_get:
        assert_same_bits(get_device(ix, every), model.rows, "get_device(all rows)")
    out = sweep(oracle, ix, model, sweep_rows(n, named), returned_ids)
    out["rows"] = rows
    return out


# ---- dims and row tails --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dim", DIMS)
def test_ingest_dims_and_row_tails(oracle, dim, form):
    """600 rows in pieces of 1, 3, 4, 5, 243, 1, 343 (4 rows to a block of k_normalize): capacity 256 -> 512 at exactly 257 rows, then
    512 -> 768; the state after the row tails, after each capacity step and at the end"""
    corpus = synth.make_corpus(sum(PIECES), dim, duplicates=False)
    p = Pair(dim, form)
    at = 0
    for piece in PIECES:
        p.add(corpus[at:at + piece])
        at += piece
        if at in (13, 257, 600):
            check_state(oracle, p.ix, p.model)
    assert at == 600
    p.close()


@pytest.mark.parametrize("dim", DIMS)
def test_l2_normalize_dims_and_row_tails(oracle, dim):
    x = synth.make_corpus(257, dim, duplicates=False)
    for n in (1, 3, 4, 5, 257):
        want = oracle.normalize_rows(x[:n])
        assert_same_bits(normalize_host(x[:n]), want, f"host, n = {n}")
        assert_same_bits(normalize_device(x[:n]), want, f"device, n = {n}")
    assert_same_bits(normalize_device(x, side_stream=True), oracle.normalize_rows(x), "device, a stream of its own")


# ---- special rows --------------------------------------------------------------------------------------------------------------------
def special_rows(dim, bf16):
    r = np.zeros((8, dim), dtype=np.float32)      # row 0: all zero (divisor 1e-12: stays zero)
    r[1] = 1e-20                                  # norm below 1e-12: divided by 1e-12, not by the norm
    r[2] = 1e15                                   # squares far beyond fp32's range: the sum is fp64
    r[3, dim - 1] = -2.5                          # one element, in the last float4 group
    r[4, 0] = 7.0                                 # ... in the first
    r[5, dim - 4] = 3.0                           # the last group's first element and the first group's last
    r[5, 3] = -4.0
    r[6] = synth.make_corpus(1, dim, duplicates=False)[0]
    if bf16:                                      # bf16 subnormals: patterns 0x0001 .. 0x007F, both signs (fp32 subnormals once widened)
        u = to_bf16(r)
        u[7] = (np.arange(dim) % 0x7F + 1).astype(np.uint16) | ((np.arange(dim) % 2) << 15).astype(np.uint16)
        return u
    r[7] = np.float32(1e-39) * (1 + np.arange(dim) % 5)   # fp32 subnormals
    return r


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dim", [8, 1028])
def test_special_rows(oracle, dim, form):
    raw = special_rows(dim, form != "f32")
    vals = raw if form == "f32" else widen(raw)
    want = oracle.normalize_rows(vals)
    assert (want[0] == 0).all() and np.isfinite(want).all() and (np.abs(want[7]) > 0).all()   # (what the model itself says of them)
    ix = new_index(dim, form)
    ix.add(raw) if form == "f32" else ix.add_bf16(raw)
    assert len(ix) == 8
    assert_same_bits(ix.get(np.arange(8)), want, "get")
    assert_same_bits(ix.get(np.arange(8)[::-1].copy()), want[::-1], "get, descending ids")
    if form != "bf16_compact":                     # (rdx_l2_normalize takes fp32: the widened values)
        assert_same_bits(normalize_host(vals), want, "l2_normalize, host")
        assert_same_bits(normalize_device(vals), want, "l2_normalize, device")
    ix.close()


# ---- stored rows ---------------------------------------------------------------------------------------------------------------------
def test_add_stored_round_trip(oracle):
    """add_stored(get(...)) into a second index: the same bits and the same answers as the first"""
    dim, n = 260, 300
    a = Pair(dim)
    a.add(synth.make_corpus(n, dim, duplicates=False))
    first = check_state(oracle, a.ix, a.model)
    b = new_index(dim)
    for lo, hi in ((0, 1), (1, 257), (257, n)):     # (a capacity step on the way)
        b.add_stored(first["rows"][lo:hi])
    second = check_state(oracle, b, a.model, device_get=True)
    for mode in ("exact", "fast16"):
        for x, y in zip(first[mode], second[mode]):
            np.testing.assert_array_equal(x.view(np.int32) if x.dtype == np.float32 else x, y.view(np.int32) if y.dtype == np.float32 else y)
    a.close()
    b.close()


@pytest.mark.parametrize("how", ["host", "device"])
def test_stored_rows_not_unit_length(oracle, how):
    """add_stored / update_stored keep rows that are not unit length verbatim (scaled by 0.5 and 3), and the exact scores are the
    oracle's on those rows. Only the exact path is asked: the MFMA paths' coarse bound is derived for rows of at most unit length.
    The sweep's precondition still holds (a row of length 0.5 scores 0.5 with itself, a row of length 3 at most 3 x 0.09 with it)."""
    dim, n = 1028, 300
    unit = oracle.normalize_rows(synth.make_corpus(n, dim, duplicates=False))
    scale = np.where(np.arange(n) % 2 == 0, np.float32(0.5), np.float32(3.0))[:, None]
    p = Pair(dim)
    stored = (unit * scale).astype(np.float32)
    p.ix.add_stored(stored)
    p.model.add_stored(stored)
    every = np.arange(n)
    assert_same_bits(p.ix.get(every), stored, "add_stored: verbatim")
    sweep(oracle, p.ix, p.model, every, modes=["exact"])
    ids = np.array([n - 1, 256, 255, 32, 31, 0, 77], dtype=np.int64)
    new = (oracle.normalize_rows(fresh_rows(ids.size, dim, 7)) * scale[:ids.size][::-1]).astype(np.float32)
    p.update_stored(ids, new, how)
    assert_same_bits(p.ix.get(ids), new, "update_stored: verbatim")
    assert_same_bits(p.ix.get(every), p.model.rows, "update_stored: the other rows")
    sweep(oracle, p.ix, p.model, every, modes=["exact"])
    p.close()


# ---- update --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["host", "device"])
@pytest.mark.parametrize("dim", [68, 1028])
def test_update_rows(oracle, dim, how):
    """ids at the edges of a scan block (31, 32), of a tile and a capacity step (255, 256) and of the index (0, n - 1), not ascending;
    update, then update_stored on the same ids"""
    n = 600
    p = Pair(dim)
    p.add(synth.make_corpus(n, dim, duplicates=False))
    check_state(oracle, p.ix, p.model)              # (the int8 copy is built here: the update has to bring it along)
    ids = np.array([n - 1, 256, 255, 32, 0, 31, 300, 299, 511, 512], dtype=np.int64)
    p.update(ids, fresh_rows(ids.size, dim, 11), how)
    check_state(oracle, p.ix, p.model, device_get=True)
    p.update_stored(ids, oracle.normalize_rows(fresh_rows(ids.size, dim, 12)), how)
    check_state(oracle, p.ix, p.model, device_get=True)
    p.close()


# ---- the 32 768-row staging chunk of host calls ------------------------------------------------------------------------------------------
CHUNK_ROWS = 32768 + 5
CHUNK_SWEEP = np.concatenate([np.arange(300), np.arange(32760, 32773), np.arange(CHUNK_ROWS - 300, CHUNK_ROWS)])
CHUNK_SWEEP = np.unique(CHUNK_SWEEP)                # rows 32 760 .. 32 772 around the chunk's edge (the index ends at 32 772), first and last 300


@pytest.mark.parametrize("form", ["f32", "bf16"])
def test_staging_chunk_add_get(oracle, form):
    """one host add of 32 768 + 5 rows (two staging chunks), one host get of all of them"""
    p = Pair(8, form)
    p.add(synth.make_corpus(CHUNK_ROWS, 8, duplicates=False))
    check_state(oracle, p.ix, p.model, named=CHUNK_SWEEP)
    p.close()


def test_staging_chunk_update(oracle):
    """one host update of 32 768 + 5 distinct ids in shuffled order: the second chunk's ids are d_ids + 32 768"""
    p = Pair(8)
    p.add(synth.make_corpus(CHUNK_ROWS, 8, duplicates=False))
    ids = np.random.default_rng(5).permutation(CHUNK_ROWS).astype(np.int64)
    p.update(ids, fresh_rows(CHUNK_ROWS, 8, 21))
    check_state(oracle, p.ix, p.model, named=CHUNK_SWEEP)
    p.close()


# ---- compact -------------------------------------------------------------------------------------------------------------------------
COMPACT_ROWS, BASE = 780, 1000
KEEP = {"all": np.arange(COMPACT_ROWS), "every_third": np.arange(0, COMPACT_ROWS, 3), "row_0": np.array([0]),
        "last_row": np.array([COMPACT_ROWS - 1]), "none": np.array([], dtype=np.int64)}


def _named(n):
    return None if n <= SWEEP_MAX else np.concatenate([np.arange(320), np.arange(n - 320, n)])


@pytest.mark.parametrize("form", ["f32", "bf16_compact"])
@pytest.mark.parametrize("keep", list(KEEP))
def test_compact_then_write(oracle, keep, form):
    """compaction to a keep list, with a row-id map set before it (gone afterwards: local row + row_base); then an add of 10 rows at
    the compacted capacity and an update. An index with a compact master takes no update (rdx_index_update* are fp32 calls)."""
    dim = 252
    p = Pair(dim, form, row_base=BASE)
    p.add(synth.make_corpus(COMPACT_ROWS, dim, duplicates=False))
    ids = 3 * np.arange(COMPACT_ROWS, dtype=np.int64) + 7
    p.ix.set_row_ids(0, ids)
    check_state(oracle, p.ix, p.model, named=_named(COMPACT_ROWS), returned_ids=ids)
    p.compact(KEEP[keep].astype(np.int64))
    n = KEEP[keep].size
    local = lambda m: BASE + np.arange(m, dtype=np.int64)
    check_state(oracle, p.ix, p.model, named=_named(n), returned_ids=local(n))
    if n == 0:
        q = fresh_rows(5, dim, 3)
        for mode in ({"force_exact": 1}, {"force_fast": 1}, {}):
            for name, v in mode.items():
                p.ix.set_option(name, v)
            gs, gr, gc = p.ix.search(q, K)
            for name in mode:
                p.ix.set_option(name, 0)
            assert (gc == 0).all() and (gr == -1).all() and np.isneginf(gs).all(), mode
    p.add(fresh_rows(10, dim, 31))
    check_state(oracle, p.ix, p.model, named=_named(n + 10), returned_ids=local(n + 10))
    upd = np.unique(np.array([n + 9, n, n // 2, 0], dtype=np.int64))[::-1].copy()
    if form == "f32":
        p.update(upd, fresh_rows(upd.size, dim, 32))
        check_state(oracle, p.ix, p.model, named=_named(n + 10), returned_ids=local(n + 10))
    else:
        from rag_dpo_amd._lib import RdxError
        with pytest.raises(RdxError, match="compact"):
            p.ix.update(upd, fresh_rows(upd.size, dim, 32))
        check_state(oracle, p.ix, p.model, named=_named(n + 10), returned_ids=local(n + 10))
    p.close()


# ---- refused writes change nothing ---------------------------------------------------------------------------------------------------
REF_DIM, REF_ROWS = 68, 300        # all three sweep modes run: 300 rows, 300 queries, dim_pad 128


def _refused_pair(form="f32"):
    p = Pair(REF_DIM, form)
    p.add(synth.make_corpus(REF_ROWS, REF_DIM, duplicates=False))
    return p


def assert_unchanged(oracle, p, before):
    """the state check against the unchanged model, and bit for bit what the snapshot held"""
    now = check_state(oracle, p.ix, p.model, device_get=True)
    assert set(now) == set(before) and {"exact", "fast16", "fast8", "rows"} <= set(now)
    assert_same_bits(now["rows"], before["rows"], "rows against the snapshot")
    for mode in now:
        if mode != "rows":
            for x, y in zip(now[mode], before[mode]):
                np.testing.assert_array_equal(x.view(np.int32) if x.dtype == np.float32 else x, y.view(np.int32) if y.dtype == np.float32 else y,
                                              err_msg=f"{mode} against the snapshot")


POISON = {"nan": (np.float32(np.nan), 0x7FC0), "+inf": (np.float32(np.inf), 0x7F80), "-inf": (np.float32(-np.inf), 0xFF80)}


@pytest.mark.parametrize("poison", list(POISON))
@pytest.mark.parametrize("call", ["add", "add_stored", "add_bf16"])
def test_refused_append(oracle, call, poison):
    """a NaN / +Inf / -Inf in a middle row of 100: nothing is added. The rejected batch repeats rows the index holds, so a row of it
    that a scan could still see would tie with a query's own row and show up as its second hit. The add of 7 rows that follows leaves
    rows 7 .. 99 of the rejected batch beyond count(), inside the last 32-row block and after it."""
    p = _refused_pair("bf16" if call == "add_bf16" else "f32")
    before = check_state(oracle, p.ix, p.model, device_get=True)
    batch = before["rows"][:100].copy()
    if call == "add_bf16":
        batch = to_bf16(batch)
        batch[50, REF_DIM // 2] = POISON[poison][1]
    else:
        batch[50, REF_DIM // 2] = POISON[poison][0]
    with pytest.raises(ValueError, match="NaN or Inf"):
        getattr(p.ix, call)(batch)
    assert_unchanged(oracle, p, before)
    p.add(fresh_rows(7, REF_DIM, 41))
    check_state(oracle, p.ix, p.model, device_get=True)
    p.close()


@pytest.mark.parametrize("how", ["host", "device"])
@pytest.mark.parametrize("stored", [False, True], ids=["update", "update_stored"])
def test_refused_update_nan(oracle, stored, how):
    """3 rows whose second holds a NaN: neither the first nor the third is written"""
    p = _refused_pair()
    before = check_state(oracle, p.ix, p.model, device_get=True)
    ids = np.array([255, 31, 256], dtype=np.int64)
    rows = oracle.normalize_rows(fresh_rows(3, REF_DIM, 51))
    bad = rows.copy()
    bad[1, REF_DIM - 1] = np.nan
    with pytest.raises(ValueError, match="NaN or Inf"):
        if how == "host":
            (p.ix.update_stored if stored else p.ix.update)(ids, bad)
        else:
            update_device(p.ix, ids, bad, stored=stored)
    assert_unchanged(oracle, p, before)
    (p.update_stored if stored else p.update)(ids, rows, how)
    check_state(oracle, p.ix, p.model, device_get=True)
    p.close()


def test_refused_ids_out_of_range(oracle):
    """update / get with an id equal to count(), and with -1"""
    p = _refused_pair()
    before = check_state(oracle, p.ix, p.model, device_get=True)
    rows = fresh_rows(3, REF_DIM, 52)
    for wrong in (REF_ROWS, -1):
        ids = np.array([5, wrong, 9], dtype=np.int64)
        for call in (lambda: p.ix.update(ids, rows), lambda: p.ix.update_stored(ids, rows), lambda: update_device(p.ix, ids, rows),
                     lambda: p.ix.get(ids), lambda: get_device(p.ix, ids)):
            with pytest.raises(ValueError, match="out of range"):
                call()
    assert_unchanged(oracle, p, before)
    p.update(np.array([9, 5], dtype=np.int64), rows[:2])
    check_state(oracle, p.ix, p.model)
    p.close()


@pytest.mark.parametrize("how", ["host", "device"])
def test_refused_update_repeated_id(oracle, how):
    """a row id given twice in one call: two waves would write one row at once"""
    p = _refused_pair()
    before = check_state(oracle, p.ix, p.model, device_get=True)
    ids = np.array([5, 9, 5], dtype=np.int64)
    rows = fresh_rows(3, REF_DIM, 53)
    for stored in (False, True):
        with pytest.raises(ValueError, match="row id 5 is given more than once"):
            if how == "host":
                (p.ix.update_stored if stored else p.ix.update)(ids, rows)
            else:
                update_device(p.ix, ids, rows, stored=stored)
        assert_unchanged(oracle, p, before)
    p.update(np.array([9, 5], dtype=np.int64), rows[:2], how)
    check_state(oracle, p.ix, p.model)
    p.close()
