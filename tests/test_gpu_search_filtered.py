"""rdx_search_filtered through HipIndex: one search, a row filter per query.

Every result is compared with assert_array_equal — scores, rows, counts and the (-inf, -1) padding — against the CPU oracle called once
per distinct bitmap, and against search_device(mask=...) per distinct mask on the same index under the same options. The mask set used
throughout: even rows, odd rows, all ones, all zeros, fewer than k rows, rows of the last (ragged) 32-row block only, and -1 (no
filter); query q names filter (q % 7) - 1, so the neighbours of every 16-query MFMA block alternate between all of them.

Paths: the exact path (k_exact_scores_reg<U> at dims 64 / 200, k_exact_scores at 1 280; two groups of four queries, the second with
one), the small path (k_boot + k_scan_small), the streaming k_scan (one 64-query tile, the 128-query tile, the half-tile bootstrap,
several tiles; the plan's fused choice on and off, block and tile sample), the ragged k-step at dim 200, the fallback passes with
cand_cap = 8 (second-chance batch and exact scan of the list), the int8 option, chunking at 4 096 queries, the degenerate calls and
the refusals. The leak probe plants, per query, the query itself in a row its mask forbids and a near copy in a row it allows."""
import ctypes

import numpy as np
import pytest

from rag_dpo_amd import synth

pytestmark = pytest.mark.gpu

DEFAULTS = {"force_exact": 0, "force_fast": 0, "small_scan": 1, "split_boot": 1, "fuse_epilogue": 1, "spread_boot": 1, "cand_cap": 0,
            "retry": 1, "coarse_i8": 2}
N_STREAM, D_STREAM, B_STREAM = 30_011, 64, 600


@pytest.fixture(scope="module")
def eng():
    from rag_dpo_amd import engine
    return engine


def mask_set(n, k):
    """the six bitmaps of the module's docstring, as bool[n]"""
    rows = np.arange(n)
    few = np.zeros(n, dtype=bool)
    few[(np.arange(min(k - 1, 7)) * 997 + 41) % n] = True
    return [rows % 2 == 0, rows % 2 == 1, np.ones(n, dtype=bool), np.zeros(n, dtype=bool), few, rows >= (n - 1) // 32 * 32]


def assignment(nq):
    return ((np.arange(nq) % 7) - 1).astype(np.int32)


def oracle_per_query(oracle, corpus, q, k, allows, qf):
    """the model: the oracle called per distinct bitmap with the queries that name it"""
    ch = oracle.normalize_rows(corpus)
    sc = np.empty((len(q), k), dtype=np.float32)
    ro = np.empty((len(q), k), dtype=np.int64)
    cn = np.empty((len(q),), dtype=np.int32)
    for f in np.unique(qf):
        sel = np.flatnonzero(qf == f)
        sc[sel], ro[sel], cn[sel] = oracle.cosine_topk(ch, q[sel], k, None if f < 0 else allows[f])
    return sc, ro, cn


class Index:
    """an index, the resident masks of `allows` and the device-side calls of the tests"""

    def __init__(self, eng, oracle, corpus, allows, **opts):
        self.ix = eng.HipIndex(corpus.shape[1])
        self.ix.add(corpus)
        self.n = corpus.shape[0]
        self.masks = [self.ix.make_mask(oracle.pack_mask(a, self.n)) for a in allows]
        self.set(**opts)

    def set(self, **opts):
        for name, v in {**DEFAULTS, **opts}.items():
            self.ix.set_option(name, v)

    def _outs(self, nq, k):
        import torch
        return (torch.full((nq, k), 7.0, dtype=torch.float32, device="cuda"), torch.full((nq, k), 7, dtype=torch.int64, device="cuda"),
                torch.full((nq,), 7, dtype=torch.int32, device="cuda"))

    def filtered(self, q, k, qf, masks=None):
        import torch
        s, r, c = self._outs(len(q), k)
        self.ix.search_filtered_device(torch.from_numpy(q).cuda(), k, s, r, c, self.masks if masks is None else masks, qf)
        torch.cuda.synchronize()
        return s.cpu().numpy(), r.cpu().numpy(), c.cpu().numpy()

    def masked_loop(self, q, k, qf):
        """search_device(mask=...) per distinct mask: the route one filtered search replaces"""
        import torch
        sc = np.empty((len(q), k), dtype=np.float32)
        ro = np.empty((len(q), k), dtype=np.int64)
        cn = np.empty((len(q),), dtype=np.int32)
        for f in np.unique(qf):
            sel = np.flatnonzero(qf == f)
            s, r, c = self._outs(len(sel), k)
            self.ix.search_device(torch.from_numpy(q[sel]).cuda(), k, s, r, c, mask=None if f < 0 else self.masks[f])
            torch.cuda.synchronize()
            sc[sel], ro[sel], cn[sel] = s.cpu().numpy(), r.cpu().numpy(), c.cpu().numpy()
        return sc, ro, cn

    def close(self):
        for m in self.masks:
            m.close()
        self.ix.close()


def check(got, want, what=""):
    for g, w, name in zip(got, want, ("scores", "rows", "counts")):
        np.testing.assert_array_equal(g, w, err_msg=f"{what}: {name}")


def check_both(I, q, k, qf, ref, what, path=None):
    got = I.filtered(q, k, qf)
    st = I.ix.last_stats()
    check(got, ref, what + " against the oracle")
    check(got, I.masked_loop(q, k, qf), what + " against search_device(mask) per mask")
    if path is not None:
        assert st["path"] == path, (what, st)
    return st


# ---- exact path --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [64, 200, 1280])
def test_exact_path(eng, oracle, dim):
    corpus = synth.make_corpus(1317, dim)
    q = synth.make_queries(5, dim, corpus)
    for k in (1, 10):
        allows = mask_set(1317, k)
        qf = np.array([0, 1, 4, 5, -1], dtype=np.int32) if k == 10 else np.array([1, 3, 5, -1, 0], dtype=np.int32)
        I = Index(eng, oracle, corpus, allows, force_exact=1)
        ref = oracle_per_query(oracle, corpus, q, k, allows, qf)
        st = check_both(I, q, k, qf, ref, f"exact dim {dim} k {k}", path=1)
        assert st["coarse_bits"] == 0
        # host in / host out: the same call through rdx_search_filtered with RDX_HOST
        check(I.ix.search_filtered(q, k, I.masks, qf), ref, "host arrays")
        I.close()


# ---- small path: k_boot + k_scan_small -------------------------------------------------------------------------------------------------
def test_small_path(eng, oracle):
    corpus = synth.make_corpus(9000, 64)
    q = synth.make_queries(40, 64, corpus)
    allows, qf = mask_set(9000, 10), assignment(40)
    I = Index(eng, oracle, corpus, allows, force_fast=1)
    st = check_both(I, q, 10, qf, oracle_per_query(oracle, corpus, q, 10, allows, qf), "small path", path=0)
    assert st["coarse_bits"] == 16
    I.close()


# ---- streaming path: k_scan<SETMAX> + k_scan<EMIT> ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stream_case(eng, oracle):
    corpus = synth.make_corpus(N_STREAM, D_STREAM)
    q = synth.make_queries(B_STREAM, D_STREAM, corpus)
    allows, qf = mask_set(N_STREAM, 10), assignment(B_STREAM)
    I = Index(eng, oracle, corpus, allows)
    ref = oracle_per_query(oracle, corpus, q, 10, allows, qf)   # per query: a smaller batch is its first rows
    yield I, q, qf, ref
    I.close()


@pytest.mark.parametrize("b", [33, 130, 200, 257, 600])
@pytest.mark.parametrize("fuse,spread", [(1, 1), (0, 1), (1, 0), (0, 0)])
def test_streaming_path(stream_case, b, fuse, spread):
    I, q, qf, ref = stream_case
    I.set(force_fast=1, small_scan=0, split_boot=0, fuse_epilogue=fuse, spread_boot=spread)
    got = I.filtered(q[:b], 10, qf[:b])
    st = I.ix.last_stats()
    check(got, tuple(x[:b] for x in ref), f"streaming b {b} fuse {fuse} spread {spread} against the oracle")
    assert st["path"] == 0 and st["coarse_bits"] == 16, st
    if fuse == 1 and spread == 1:
        check(got, I.masked_loop(q[:b], 10, qf[:b]), f"streaming b {b} against search_device(mask) per mask")


def test_streaming_ragged_kstep(eng, oracle):
    corpus = synth.make_corpus(N_STREAM, 200)
    q = synth.make_queries(130, 200, corpus)
    allows, qf = mask_set(N_STREAM, 10), assignment(130)
    I = Index(eng, oracle, corpus, allows, force_fast=1, small_scan=0, split_boot=0)
    check_both(I, q, 10, qf, oracle_per_query(oracle, corpus, q, 10, allows, qf), "dim 200", path=0)
    I.close()


# ---- leak probe --------------------------------------------------------------------------------------------------------------------
def test_leak_probe(eng, oracle):
    """Per query: the query itself in a row its mask forbids, a slightly rotated copy in a row it allows. Unfiltered, the forbidden row
    is every query's top-1 (checked on the CPU first: without that a leak would not show); filtered, the top-1 must be the allowed plant,
    on every path."""
    n, d, b = N_STREAM, D_STREAM, 257
    rng = np.random.default_rng(26)
    corpus = synth.make_corpus(n, d).copy()
    q = rng.standard_normal((b, d)).astype(np.float32)
    last0 = (n - 1) // 32 * 32
    allows = [np.arange(n) % 2 == 0, np.arange(n) % 2 == 1, np.arange(n) >= last0]
    qf = (np.arange(b) % 2).astype(np.int32)
    qf[np.arange(5, b, 16)] = 2                  # 16 queries allowed only the ragged last block (27 rows)
    forbid, allowed = np.empty(b, dtype=np.int64), np.empty(b, dtype=np.int64)
    n_last = 0
    for i in range(b):
        base = 64 + 100 * i                      # even; distinct rows per query, all below the last block
        if qf[i] == 0:
            forbid[i], allowed[i] = base + 1, base + 2
        elif qf[i] == 1:
            forbid[i], allowed[i] = base + 2, base + 1
        else:
            forbid[i], allowed[i] = base + 1, last0 + n_last
            n_last += 1
        corpus[forbid[i]] = q[i]
        corpus[allowed[i]] = q[i] + 0.05 * rng.standard_normal(d).astype(np.float32)
    assert n_last <= n - last0 and base + 2 < last0
    ch = oracle.normalize_rows(corpus)
    np.testing.assert_array_equal(oracle.cosine_topk(ch, q, 1)[1][:, 0], forbid)       # a leak would show
    ref = oracle_per_query(oracle, corpus, q, 10, allows, qf)
    np.testing.assert_array_equal(ref[1][:, 0], allowed)
    I = Index(eng, oracle, corpus, allows)
    stream = dict(force_fast=1, small_scan=0, split_boot=0)
    for what, nq, opts in (("exact", 37, dict(force_exact=1)), ("small", 40, dict(force_fast=1)), ("stream 33", 33, stream), ("stream 130", 130, stream),
                           ("stream 200", 200, stream), ("stream 257", b, stream), ("stream 257 unfused", b, dict(stream, fuse_epilogue=0)),
                           ("stream 257 tile sample", b, dict(stream, spread_boot=0))):
        I.set(**opts)
        got = I.filtered(q[:nq], 10, qf[:nq])
        np.testing.assert_array_equal(got[1][:, 0], allowed[:nq], err_msg=what)
        check(got, tuple(x[:nq] for x in ref), what)
    I.close()


# ---- fallback passes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,b,scan", [(9000, 40, "small"), (N_STREAM, 200, "stream")])
@pytest.mark.parametrize("retry", [1, 0])
def test_fallbacks(eng, oracle, n, b, scan, retry):
    """cand_cap = 8: rows [64 q, 64 q + 64) are near copies of query q, all within the scan's error band of one another and in one
    256-row tile, so every query whose mask allows more than eight of them overflows its segment: the second-chance batch (retry = 1,
    the overflowed queries' filter indices gathered with their vectors) or the exact scan of the list (retry = 0) answers them."""
    rng = np.random.default_rng(n + retry)
    corpus = synth.make_corpus(n, 64).copy()
    q = rng.standard_normal((b, 64)).astype(np.float32)
    for i in range(b):
        corpus[64 * i:64 * i + 64] = q[i] + 1e-3 * rng.standard_normal((64, 64)).astype(np.float32)
    allows, qf = mask_set(n, 10), assignment(b)
    opts = dict(force_fast=1, cand_cap=8, retry=retry)
    if scan == "stream":
        opts.update(small_scan=0, split_boot=0)
    I = Index(eng, oracle, corpus, allows, **opts)
    st = check_both(I, q, 10, qf, oracle_per_query(oracle, corpus, q, 10, allows, qf), f"fallback {scan} retry {retry}", path=0)
    overflowing = int(np.isin(qf, (-1, 0, 1, 2)).sum())      # no filter, even, odd, all ones: 32 or 64 near copies allowed
    assert (st["retried_queries"] if retry else st["exact_queries"]) >= overflowing, st
    I.close()


# ---- the int8 option ------------------------------------------------------------------------------------------------------------------
def test_int8_option_is_not_taken(eng, oracle):
    n, d, b = 20_000, 256, 300
    corpus = synth.make_corpus(n, d)
    q = synth.make_queries(b, d, corpus)
    allows, qf = mask_set(n, 10), assignment(b)
    I = Index(eng, oracle, corpus, allows, force_fast=1, coarse_i8=1)
    import torch
    qd = torch.from_numpy(q).cuda()
    plain = I._outs(b, 10)
    I.ix.search_device(qd, 10, *plain)
    torch.cuda.synchronize()
    before = I.ix.last_stats()["coarse_bits"]
    st = check_both(I, q, 10, qf, oracle_per_query(oracle, corpus, q, 10, allows, qf), "coarse_i8 = 1", path=0)
    assert st["coarse_bits"] == 16, st
    I.ix.search_device(qd, 10, *plain)
    torch.cuda.synchronize()
    assert I.ix.last_stats()["coarse_bits"] == before == 8
    I.close()


# ---- chunking -------------------------------------------------------------------------------------------------------------------------
def test_chunks_of_4096(eng, oracle):
    n, b = 2000, 4100
    corpus = synth.make_corpus(n, 64)
    q = np.random.default_rng(41).standard_normal((b, 64)).astype(np.float32)
    allows = mask_set(n, 10)
    qf = assignment(b)
    qf[4090:4096], qf[4096:] = 0, 1           # the index changes across the chunk boundary
    I = Index(eng, oracle, corpus, allows)
    check(I.filtered(q, 10, qf), oracle_per_query(oracle, corpus, q, 10, allows, qf), "4 100 queries")
    I.close()


# ---- degenerate calls --------------------------------------------------------------------------------------------------------------
def test_degenerate_calls_are_the_existing_search(eng, oracle):
    """one distinct mask, and no mask at all: search_device's results, planned as search_device plans (with coarse_i8 = 1 the int8 pass
    runs, which a search with a filter per query never takes), with search_device's statistics"""
    n, d, b = 20_000, 256, 300
    corpus = synth.make_corpus(n, d)
    q = synth.make_queries(b, d, corpus)
    allows = mask_set(n, 10)
    I = Index(eng, oracle, corpus, allows, force_fast=1, coarse_i8=1)
    keys = ("path", "coarse_bits", "emitted", "rescored", "exact_queries", "retried_queries", "sample_rows")
    for qf, masks in ((np.zeros(b, dtype=np.int32), None), (np.full(b, 1, dtype=np.int32), None), (np.full(b, -1, dtype=np.int32), None),
                      (np.full(b, -1, dtype=np.int32), [])):
        got = I.filtered(q, 10, qf, masks)
        st = I.ix.last_stats()
        want = I.masked_loop(q, 10, qf)
        st_want = I.ix.last_stats()
        check(got, want, f"one filter {qf[0]}")
        assert st["coarse_bits"] == 8 and {x: st[x] for x in keys} == {x: st_want[x] for x in keys}, (st, st_want)
    I.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(eng, oracle):
    import torch
    from rag_dpo_amd import _lib as L
    n, b, k = 1317, 5, 3
    corpus = synth.make_corpus(n, 64)
    q = synth.make_queries(b, 64, corpus)
    I = Index(eng, oracle, corpus, mask_set(n, k)[:2])
    lib, h = I.ix._lib, I.ix._h
    qd = torch.from_numpy(q).cuda()
    outs = I._outs(b, k)
    handles = (ctypes.c_void_p * 2)(*[m._h for m in I.masks])
    null_in = (ctypes.c_void_p * 2)(I.masks[0]._h, None)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731

    def call(filters, n_filters, qf):
        a = None if qf is None else np.ascontiguousarray(qf, dtype=np.int32)
        rc = lib.rdx_search_filtered(h, ptr(qd), b, k, filters, n_filters, None if a is None else ctypes.c_void_p(a.ctypes.data),
                                     ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), L.RDX_DEVICE, None)
        return rc, lib.rdx_last_error().decode()

    ok = [0, 1, -1, 0, 1]
    for filters, n_filters, qf, words in (
            (handles, 2, [0, 1, 2, 0, 1], ("query 2", "filter 2", "[-1, 2)")),
            (handles, 2, [0, -2, 1, 0, 1], ("query 1", "filter -2", "[-1, 2)")),
            (None, 0, [0, -1, -1, -1, -1], ("query 0", "filter 0", "[-1, 0)")),
            (None, 2, ok, ("filters is NULL", "n_filters = 2")),
            (null_in, 2, ok, ("filters[1]", "NULL handle")),
            (handles, 2, None, ("query_filter is NULL", "nq = 5")),
            (handles, -1, ok, ("n_filters", "[0, 65535]", "-1")),
            (handles, 65536, ok, ("n_filters", "[0, 65535]", "65536"))):
        rc, msg = call(filters, n_filters, qf)
        assert rc == L.RDX_ERR_INVALID and all(w in msg for w in words), (rc, msg, words)
    # a mask of another row count: RDX_ERR_STATE, as rdx_search_masked refuses it — also when the call would be the existing search
    I.ix.add(corpus[:1])
    for qf in (ok, [1, 1, 1, 1, 1]):
        rc, msg = call(handles, 2, qf)
        assert rc == L.RDX_ERR_STATE and "rdx_search_filtered" in msg and "does not outlive a write" in msg, (rc, msg)
    torch.cuda.synchronize()
    assert (outs[0] == 7.0).all() and (outs[1] == 7).all() and (outs[2] == 7).all()
    I.close()
