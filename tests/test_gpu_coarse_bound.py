"""The fp16 coarse scan against its model (tests/coarse_model.py) at the error bound E, through every scan variant the launch plan
(rdx_index.hip plan_search) can choose. Each query of a batch gets an instance of its own — a ladder of probe rows around its refine
band edge t2 = c_k - 2E (dyadic: the kernel's coarse scores are the model's to the bit; aligned: the anchor sits 0.78 E above or
below its exact score), a split pair (coarse(B) - coarse(A) > E, exact(A) > exact(B)) or a subnormal ladder — on its own columns
or sign pattern; the rest of the corpus lies on other columns (coarse score exactly 0).

Asserted: ids and score bits equal the C oracle; path 0 with no query left to the exact scan and, at the proven threshold, none
retried; `rescored` (rows k_refine found in its band) equals the model's count exactly — a kernel coarse score off by more than the
probes' distance to t2 (2.5e-6 in the band, 6e-6 outside) changes it; `emitted` too where the threshold is known (k = 1: the sampled maximum is the query's own anchor).

Which kernels a parametrisation takes (plan_search; `_plan` restates the part that decides it):
  B <= 64, split_boot / small_scan: k_boot / k_scan<SETMAX,64> + k_scan_small (d <= 1024: at most 16 k-steps) / k_scan<EMIT,64>
  B = 65 .. 128: k_scan<*,128>; B = 129 .. 256: bootstrap k_scan<SETMAX,128> x 2 tiles (half_boot) or <SETMAX,256>, main <EMIT,256>
  B > 1024: several 256-query tiles; force_bn: 64 / 128 / 256 queries per workgroup; d = 4096: no k_scan_small (64 k-steps)
  fuse_epilogue 0/1: the emit check after the tile or fused into the next tile's first k-step (k_scan<EMIT> only)
  cand_cap = 1: every segment with two hits overflows -> the second MFMA pass (depth 1) re-runs the query
`_plan` reads the device's CU count as the library does and assumes sample_div = 1 at depth 0; every test checks that its anchors
lie in the blocks the plan samples.

Not covered: the speculative threshold. Every index here runs with spec_tau = 0; spec_tau = 1 would change nothing, because at
k = 1 speculative_rank returns k, and with the whole corpus sampled (sample_div = 1) it returns k for any k. Exercising it needs a
sample much thinner than the corpus (hundreds of thousands of rows), which these tests do not build.
"""
import zlib

import numpy as np
import pytest

import coarse_model as M

pytestmark = pytest.mark.gpu

W = 40                 # columns per instance block
N_FILL_COLS = 4


@pytest.fixture(scope="module")
def eng():
    from rag_dpo_amd import engine
    return engine


def _n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count    # what rdx_index_create reads (rdx_index.hip h->n_cu)


def _plan(rows, dim, nq, k, opts, n_cu):
    """plan_search restated for sample_div = 1 at depth 0 (no dense sample): (use_boot, use_small, sampled) — which bootstrap and
    main-scan kernels the search takes and the set of 32-row blocks its threshold sample covers. The tests place every anchor
    inside that set (and fail loudly if they could not), which is what pins the threshold and `emitted`."""
    g = lambda n, d: opts.get(n, d)
    bn = 64 if nq <= 64 else (128 if nq <= 128 else (128 if 256 < nq <= 384 else 256))
    fb = g("force_bn", 0)
    if fb and (nq + fb - 1) // fb <= 32:
        bn = fb
    nqt = (nq + bn - 1) // bn
    grid = max(8, n_cu // 8 * 8)
    wpx = grid // 8
    G = wpx // nqt
    n_streams = 8 * G
    n_tiles = (rows + 255) // 256
    n_blocks32 = (rows + 31) // 32
    ksteps = M.dim_pad(dim) // 64
    ns_b = 8 * (wpx // 2) if (g("half_boot", 1) and bn == 256 and nqt == 1) else n_streams
    want_rows = max(64 * k, 8192)
    div = 1                                            # min(sample_div = 1, ...)
    n_sched = n_tiles
    if n_sched > ns_b and n_sched % ns_b != 0:         # whole rounds of the streams
        full = n_sched // ns_b * ns_b
        div2 = (n_tiles + full - 1) // full
        if (n_tiles + div2 - 1) // div2 * 256 >= want_rows:
            div = div2
            n_sched = (n_tiles + div - 1) // div
    n_virtual = ((n_blocks32 - 1) // div + 1) // 8
    spread = bool(g("spread_boot", 1)) and n_virtual >= 1
    if spread:
        n_sched = n_virtual
    units = min(n_blocks32, n_sched * 8)
    if units > n_cu:
        units = units // n_cu * n_cu
    use_boot = bool(g("split_boot", 1)) and bn == 64 and nqt == 1 and units <= 4 * n_cu
    use_small = (bool(g("small_scan", 1)) and bn == 64 and nqt == 1 and ksteps <= 16 and n_streams == grid and
                 grid <= n_blocks32 <= 32 * n_cu)
    if use_boot:                                       # k_boot: unit u scans block u * n_blocks32 / units
        sampled = {u * n_blocks32 // units for u in range(units)}
    elif spread:                                       # wave w of entry j: block (8 j + w) * div
        sampled = {(8 * j + w) * div for j in range(n_virtual) for w in range(8)}
    else:                                              # every div-th 256-row tile
        sampled = {8 * t + w for t in range(0, n_tiles, div) for w in range(8)}
    return use_boot, use_small, {b for b in sampled if b < n_blocks32}


def _template(kind, dim, cols, rng, bf16=False):
    """(query, anchors, probes) raw rows of one instance on `cols`"""
    if kind == "ladder":
        q = M.dyadic_query(dim, cols)
        t2 = M.ladder_prediction(q, q[None], 1, dim)["t2"]
        pr, _ = M.ladder_probes(q, t2, dim, cols, rng, bf16=bf16)
        return q, q[None].copy(), pr
    if kind in ("aligned+", "aligned-"):
        q, r = M.aligned(dim, cols, +1 if kind == "aligned+" else -1)
        p = M.ladder_prediction(q, r[None], 1, dim)
        lo = M.band_edge(np.float32(p["c_k_lo"]), dim)
        pr, _ = M.ladder_probes(q, p["t2"], dim, cols, rng, rtz_sensitive=0, edge_lo=lo, bf16=bf16)
        return q, r[None], pr
    if kind == "split":
        # a copy of A goes with the anchors (inside the bootstrap sample); A and B themselves go to block / tile edges. The
        # sampled maximum is then coarse(A) or coarse(B), and either way the threshold emits exactly {copy, A, B}
        q, a, b = M.split_pair(dim, cols)
        return q, a[None].copy(), np.stack([a, b])
    if kind.startswith("sub-"):
        q, anc, pr, _ = M.subnormal_ladder(dim, cols, kind[4:])
        return q, anc[None], pr
    raise ValueError(kind)


_TEMPLATES = {}


def _instances(dim, B, kinds, bf16=False, blocks=None):
    """per query: its raw query, anchor rows (sampled: placed first) and probe rows; block b = i mod nb of W columns, sign pattern
    i // nb on the block's columns 0..5 and 15..20 (the heaviest of every construction): instances that share a block differ there."""
    fill = list(range(dim - N_FILL_COLS, dim))
    nb = blocks or (dim - N_FILL_COLS) // W
    assert B <= 64 * nb
    out = []
    for i in range(B):
        kind = kinds[i % len(kinds)]
        b = i % nb
        key = (kind, dim, bf16)
        if key not in _TEMPLATES:
            seed = zlib.crc32(repr(key).encode())          # from the key: a test run alone builds the same rows as in the full run
            _TEMPLATES[key] = _template(kind, dim, list(range(W)), np.random.default_rng(seed), bf16)
        q, anc, pr = (x.copy() for x in _TEMPLATES[key])
        t = i // nb
        sign = np.ones(dim, np.float32)
        for j in range(6):
            if (t >> j) & 1:
                sign[[j, 15 + j]] = -1.0
        def mv(x):
            x = np.atleast_2d(x) * sign[None, :]
            y = np.zeros_like(x)
            y[:, b * W:(b + 1) * W] = x[:, :W]
            return y
        out.append((kind, mv(q)[0], mv(anc), mv(pr)))
    return out, fill


def _corpus(insts, fill, dim, n_rows, rng, bf16=False, cluster=False, k=1, opts_list=({},)):
    """anchors of every query in blocks the bootstrap samples under every option set of `opts_list` (`_plan`), probes at tile /
    block edges, in the ragged last tile and at random, N(0,1) filler on the filler columns elsewhere. Returns corpus raw rows
    and, per query, its rows' indices."""
    n_anchor = sum(len(a) for _, _, a, _ in insts)
    n_probe = sum(len(p) for _, _, _, p in insts)
    n = max(n_rows, n_anchor + 3 * n_probe + 600)
    if n % 256 == 0:
        n += 77
    corpus = np.zeros((n, dim), np.float32)
    corpus[:, fill] = rng.standard_normal((n, len(fill))).astype(np.float32)
    if cluster:
        arows = np.arange(n_anchor)
    else:
        sampled = set.intersection(*(_plan(n, dim, len(insts), k, o, _n_cu())[2] for o in opts_list))
        arows = np.array([r for b in sorted(sampled) for r in range(32 * b, min(32 * b + 32, n))][:n_anchor])
        assert len(arows) == n_anchor, "not enough sampled rows for the anchors"
    taken = set(arows.tolist())
    edges = [p for m in range(1, n // 32) for p in (32 * m - 1, 32 * m) if p not in taken]
    edges = list(dict.fromkeys(edges[::3] + [r for r in range(n - 1, n - 1 - (n % 256), -7) if r not in taken]))
    rest = np.setdiff1d(np.setdiff1d(np.arange(n), arows), edges)
    rng.shuffle(rest)
    slots = list(edges[: n_probe // 2]) + list(rest[: n_probe])
    slots = slots[:n_probe]
    rng.shuffle(slots)
    owner, at, sp = [], 0, 0
    for kind, q, anc, pr in insts:
        if cluster:                              # the instance's rows back to back at the front: several hits per segment
            idx = list(range(at, at + len(anc)))
            pidx = list(range(at + len(anc), at + len(anc) + len(pr)))
            at += len(anc) + len(pr)
        else:
            idx = [int(r) for r in arows[at:at + len(anc)]]
            at += len(anc)
            pidx = slots[sp:sp + len(pr)]
            sp += len(pr)
        corpus[idx] = anc
        corpus[pidx] = pr
        owner.append(np.array(idx + list(pidx), dtype=np.int64))
    if bf16:
        corpus = M.to_bf16(corpus)
    return corpus, owner


def _predict(insts, owner, corpus, dim, k, plan, allow=None, want_emit=True):
    """model `rescored` and `emitted` summed over the queries (emitted: None unless k = 1, where the proven threshold is pinned),
    after two checks of the construction itself: every anchor lies in a sampled block, and every row of the corpus that is not
    the query's own scores certainly below its threshold"""
    use_boot, use_small, sampled = plan
    resc, emit = 0, (0 if k == 1 and want_emit else None)
    ch_all = M.normalize(corpus)
    q_all = M.normalize(np.stack([q for _, q, _, _ in insts]))
    for (kind, _, anc, _), qh, own in zip(insts, q_all, owner):
        assert emit is None or all(int(r) // 32 in sampled for r in own[:len(anc)]), "an anchor outside the bootstrap sample"
        rows = ch_all[own]
        al = None if allow is None else allow[own]
        if kind == "split":
            # own = [copy of A, A, B]: c_k = coarse(B); the sampled maximum m is coarse(A) (copy) or coarse(B), T = m - slack
            p = M.ladder_prediction(qh, rows, 1, dim, allow=al, normalized=True)
            cs = p["coarse"]
            ts = [(M.threshold(np.float32(cs.hi[i]), dim, use_boot, use_small),
                   M.threshold(np.float32(cs.lo[i]), dim, use_boot, use_small)) for i in (0, 2)]
            counts = {M.count_at_least(cs, hi, lo) for hi, lo in ts}
            assert len(counts) == 1
            if emit is not None:
                emit += counts.pop()
            lo_t = float(min(lo for _, lo in ts))
        else:
            p = M.ladder_prediction(qh, rows, k, dim, use_boot, use_small, allow=al, normalized=True)
            if emit is not None:
                assert p.get("emitted") is not None
                emit += p["emitted"]
            lo_t = float(M.threshold(np.float32(p["c_k_lo"]), dim, True, False))
        resc += p["rescored"]
        supp = np.nonzero(qh)[0]
        sc = np.float32(2.0 ** M.scale_log2(dim))
        q16 = (qh[supp] * sc).astype(np.float16).astype(np.float64)
        c16 = (ch_all[:, supp] * sc).astype(np.float16).astype(np.float64)
        bound = c16 @ q16 + np.abs(c16) @ np.abs(q16) * len(supp) * 2.0 ** -23
        bound[own] = -np.inf
        worst = bound.max() * 4.0 ** -M.scale_log2(dim)
        assert worst < lo_t - 1e-4, (kind, worst, lo_t)
    return resc, emit


def _run(eng, oracle, ix, corpus, insts, owner, dim, k, opts, allow=None, expect_retry=0):
    qs = np.stack([q for _, q, _, _ in insts])
    plan = _plan(corpus.shape[0], dim, len(insts), k, opts, _n_cu())
    resc, emit = _predict(insts, owner, corpus, dim, k, plan, allow, want_emit=expect_retry == 0)
    ch = oracle.normalize_rows(corpus)
    es, er, ec = oracle.cosine_topk(ch, qs, k, allow)
    gs, gr, gc = ix.search(qs, k, oracle.pack_mask(allow, corpus.shape[0]))
    st = ix.last_stats()
    np.testing.assert_array_equal(gc, ec)
    np.testing.assert_array_equal(gr, er)
    np.testing.assert_array_equal(gs, es)
    for (kind, q, anc, pr), own, r in zip(insts, owner, gr):
        if kind == "split":                          # A (the exact best; its copy ties and ranks first) whatever the coarse order says
            assert r[0] in (own[0], own[1]), (own, r)
    assert st["path"] == 0, st
    assert st["exact_queries"] == 0, st
    if expect_retry == 0:
        assert st["retried_queries"] == 0, st
    else:
        assert st["retried_queries"] == expect_retry, st
    assert st["rescored"] == resc, (st, resc)
    if emit is not None and expect_retry == 0 and k == 1:
        assert st["emitted"] == emit, (st, emit)
    return st


def _index(eng, corpus, opts, bf16=False):
    ix = eng.HipIndex(corpus.shape[1])
    if bf16:
        ix.set_option("compact_master", 1)
        ix.add_bf16(M.bf16_bits(corpus))
    else:
        ix.add(corpus)
    ix.set_option("force_fast", 1)
    ix.set_option("sample_div", 1)
    ix.set_option("spec_tau", 0)
    for n, v in opts.items():
        ix.set_option(n, v)
    return ix


KINDS = ["ladder", "aligned+", "split", "aligned-"]

SMALL = [dict(split_boot=a, small_scan=b, fuse_epilogue=f) for a in (0, 1) for b in (0, 1) for f in (0, 1)]


@pytest.mark.parametrize("dim", [64, 100, 576, 1024, 1536])
@pytest.mark.parametrize("opts", SMALL, ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_small_launch_variants(eng, oracle, dim, opts):
    """B = 64 (one LDS-resident 64-query tile): k_boot or the tile bootstrap, k_scan_small or k_scan<EMIT,64>, at 1, 2, 9, 16 and
    24 k-steps. 9: wave 0 of the split-K kernels owns two k-steps (0 and 8), waves 1..7 one each. 24: k_boot's second round holds
    one k-step per wave, and k_scan_small (<= 16 k-steps) is not planned, so the threshold carries the extra slack."""
    rng = np.random.default_rng(dim)
    insts, fill = _instances(dim, 64 if dim >= 100 else 48, KINDS)
    corpus, owner = _corpus(insts, fill, dim, 9000, rng, opts_list=[opts])
    ix = _index(eng, corpus, opts)
    _run(eng, oracle, ix, corpus, insts, owner, dim, 1, opts)
    ix.close()


@pytest.mark.parametrize("B,opts", [
    (1, {}), (65, {}), (65, {"fuse_epilogue": 0}), (200, {}), (200, {"half_boot": 0}), (200, {"spread_boot": 0}),
    (300, {}), (1100, {}),
    (100, {"force_bn": 64}), (100, {"force_bn": 128}), (100, {"force_bn": 256}), (100, {"force_bn": 256, "fuse_epilogue": 0}),
])
def test_batch_sizes_and_tiles(eng, oracle, B, opts):
    """query tiles of 64 / 128 / 256 queries, several tiles per launch (B > 1024), the bootstrap as half tiles or whole ones, the
    sample as blocks or tiles, the emit check fused or not; adversarial queries at every tile position"""
    dim = 1024
    rng = np.random.default_rng(B)
    insts, fill = _instances(dim, B, KINDS)
    corpus, owner = _corpus(insts, fill, dim, 12_000, rng, opts_list=[opts])
    ix = _index(eng, corpus, opts)
    _run(eng, oracle, ix, corpus, insts, owner, dim, 1, opts)
    ix.close()


@pytest.mark.parametrize("B", [1, 64, 130])
def test_dim_4096(eng, oracle, B):
    """d = 4096: 64 k-steps (no k_scan_small, query tile not resident), E = 2.0e-3"""
    dim = 4096
    rng = np.random.default_rng(4096 + B)
    insts, fill = _instances(dim, B, KINDS)
    corpus, owner = _corpus(insts, fill, dim, 9000, rng)
    ix = _index(eng, corpus, {})
    _run(eng, oracle, ix, corpus, insts, owner, dim, 1, {})
    ix.close()


@pytest.mark.parametrize("dim", [64, 1024, 4096])
@pytest.mark.parametrize("small", [0, 1])
def test_subnormal_products(eng, oracle, dim, small):
    """probe rows whose band membership rests on fp16 SUBNORMAL products, the subnormal operand on the corpus side (scan copy
    written by K1) and on the query side (the query copy): a conversion or MFMA that flushed them would drop them from the band"""
    rng = np.random.default_rng(dim + 7)
    for side in ("row", "query"):
        insts, fill = _instances(dim, 1, ["sub-" + side])
        opts = {"small_scan": small}
        corpus, owner = _corpus(insts, fill, dim, 9000, rng, opts_list=[opts])
        ix = _index(eng, corpus, opts)
        _run(eng, oracle, ix, corpus, insts, owner, dim, 1, opts)
        ix.close()


@pytest.mark.parametrize("where", ["first", "last", "edge64", "tail"])
@pytest.mark.parametrize("dim", [100, 1024, 4096])
def test_probe_columns(eng, oracle, where, dim):
    """ladder columns in the first and the last k-step, across columns 63 / 64 and ending at column dim - 1 (dim = 100: the last
    k-step is 36 columns wide, the rest of it padding)"""
    rng = np.random.default_rng(dim)
    tmpl = _template("ladder", dim, list(range(14)), np.random.default_rng(3))
    start = {"first": 0, "last": dim - 14, "edge64": 57, "tail": dim - 14}[where]
    if where == "last":
        start = max(M.dim_pad(dim) - 64, dim - 28)
    cols = np.arange(start, start + 14)
    fill = [c for c in range(dim // 2 - 2 * N_FILL_COLS, dim) if c not in cols][:N_FILL_COLS]
    insts = []
    for t in range(16):
        sign = np.where((t >> np.arange(14)) & 1, -1.0, 1.0).astype(np.float32)
        def mv(x):
            x = np.atleast_2d(x)
            y = np.zeros_like(x)
            y[:, cols] = x[:, :14] * sign
            return y
        insts.append(("ladder", mv(tmpl[0])[0], mv(tmpl[1]), mv(tmpl[2])))
    corpus, owner = _corpus(insts, fill, dim, 9000, rng, opts_list=[{}, {"small_scan": 0, "split_boot": 0}])
    for opts in ({}, {"small_scan": 0, "split_boot": 0}):
        ix = _index(eng, corpus, opts)
        _run(eng, oracle, ix, corpus, insts, owner, dim, 1, opts)
        ix.close()


def test_band_wider_than_refine_arrays(eng, oracle):
    """k = 40, forty copies of the query and 1 100 copies of in-band probes: the band holds more than REFINE_PMAX rows and is
    re-scored in place; `rescored` still counts every band row"""
    dim = 1024
    q = M.dyadic_query(dim, list(range(14)))
    t2 = M.ladder_prediction(q, q[None], 1, dim)["t2"]
    pr, above = M.ladder_probes(q, t2, dim, list(range(14)), np.random.default_rng(5))
    anc = np.repeat(q[None], 40, axis=0)
    probes = np.vstack([np.repeat(pr[above], 275, axis=0), pr[~above]])
    insts = [("ladder", q, anc, probes)]
    rng = np.random.default_rng(40)
    corpus, owner = _corpus(insts, list(range(dim - 4, dim)), dim, 12_000, rng, k=40)
    p = M.ladder_prediction(q, corpus[owner[0]], 40, dim)
    assert p["rescored"] > M.REFINE_PMAX
    ix = _index(eng, corpus, {})
    _run(eng, oracle, ix, corpus, insts, owner, dim, 40, {})
    ix.close()


def test_where_bitmap(eng, oracle):
    """a row bitmap that hides a third of every query's probes and half the filler"""
    dim = 1024
    rng = np.random.default_rng(77)
    insts, fill = _instances(dim, 64, ["ladder", "aligned+", "aligned-"])
    corpus, owner = _corpus(insts, fill, dim, 9000, rng, opts_list=[{}, {"small_scan": 0}])
    allow = rng.random(corpus.shape[0]) < 0.5
    for own in owner:
        allow[own] = True
        allow[own[1::3]] = False
    for opts in ({}, {"small_scan": 0}):
        ix = _index(eng, corpus, opts)
        _run(eng, oracle, ix, corpus, insts, owner, dim, 1, opts, allow=allow)
        ix.close()


def test_update_and_compact_refresh_the_scan_copy(eng, oracle):
    """update() writes a copy of every query's first in-band probe over its last out-of-band probe (one more row in the band and
    above the threshold per query), then compact() drops every query's second in-band probe (one fewer) and a slice of the filler:
    a scan copy that kept the old rows, or the old row order, would leave `rescored` / `emitted` where they were"""
    dim = 1024
    rng = np.random.default_rng(91)
    insts, fill = _instances(dim, 32, ["ladder", "aligned+"])
    corpus, owner = _corpus(insts, fill, dim, 9000, rng)
    plan = _plan(corpus.shape[0], dim, len(insts), 1, {}, _n_cu())
    ix = _index(eng, corpus, {})
    _run(eng, oracle, ix, corpus, insts, owner, dim, 1, {})
    before = _predict(insts, owner, corpus, dim, 1, plan)
    ids = np.array([own[-1] for own in owner])
    new = np.stack([corpus[own[len(anc)]] for (_, _, anc, _), own in zip(insts, owner)])
    ix.update(ids, new)
    corpus[ids] = new
    after = _predict(insts, owner, corpus, dim, 1, plan)
    assert after == (before[0] + len(insts), before[1] + len(insts))      # an update the scan copy ignored would be seen
    _run(eng, oracle, ix, corpus, insts, owner, dim, 1, {})
    drop = set(int(own[len(a) + 1]) for (_, _, a, _), own in zip(insts, owner))
    drop |= set(range(5000, 5400)) - set(int(r) for own in owner for r in own)
    keep = np.array([r for r in range(corpus.shape[0]) if r not in drop], dtype=np.int64)
    ix.compact(keep)
    remap = -np.ones(corpus.shape[0], np.int64)
    remap[keep] = np.arange(keep.size)
    owner = [remap[own][remap[own] >= 0] for own in owner]
    corpus = corpus[keep]
    plan = _plan(corpus.shape[0], dim, len(insts), 1, {}, _n_cu())
    assert _predict(insts, owner, corpus, dim, 1, plan) == (after[0] - len(insts), after[1] - len(insts))
    _run(eng, oracle, ix, corpus, insts, owner, dim, 1, {})
    ix.close()


def test_compact_bf16_master(eng, oracle):
    """compact_master: raw bf16 rows (powers of two: the aligned worst case; the ladder's probes drawn among bf16 values), the scan
    copy from (float)((double)x / den)"""
    dim = 1024
    rng = np.random.default_rng(16)
    nb = (dim - N_FILL_COLS) // W
    insts, fill = _instances(dim, 2 * (nb - 8), ["aligned+", "aligned-"], bf16=True, blocks=nb - 8)
    q = M.dyadic_query(dim, list(range(14)))
    t2 = M.ladder_prediction(q, q[None], 1, dim)["t2"]
    pr, _ = M.ladder_probes(q, t2, dim, list(range(14)), np.random.default_rng(2), bf16=True)
    lad = []
    for t in range(8):
        b = nb - 1 - t
        def mv(x):
            x = np.atleast_2d(x)
            y = np.zeros_like(x)
            y[:, b * W:b * W + 14] = x[:, :14]
            return y
        lad.append(("ladder", mv(q)[0], mv(q), mv(pr)))
    insts = insts + lad
    corpus, owner = _corpus(insts, fill, dim, 9000, rng, bf16=True, opts_list=[{}, {"small_scan": 0, "split_boot": 0}])
    for opts in ({}, {"small_scan": 0, "split_boot": 0}):
        ix = _index(eng, corpus, opts, bf16=True)
        _run(eng, oracle, ix, corpus, insts, owner, dim, 1, opts)
        ix.close()


@pytest.mark.parametrize("B", [8, 200])
def test_second_mfma_pass(eng, oracle, B):
    """cand_cap = 1: a query with two hits in one segment overflows and is re-run by the second MFMA pass (depth 1: 8x denser
    sample, 4096-slot segments); its band is counted once, in that pass"""
    dim = 1024
    rng = np.random.default_rng(5 + B)
    insts, fill = _instances(dim, B, ["ladder", "aligned+", "aligned-"])
    corpus, owner = _corpus(insts, fill, dim, 9000, rng, cluster=True)
    ix = _index(eng, corpus, {"cand_cap": 1})
    _run(eng, oracle, ix, corpus, insts, owner, dim, 1, {"cand_cap": 1}, expect_retry=B)
    ix.close()
