"""GPU: k-means called directly (rag_dpo_amd.engine.kmeans -> rdx_index_kmeans -> K1, k_km_assign, k_km_hist / k_km_scan / k_km_place,
k_km_seg_table, k_km_segment_sums, k_km_finish) on a HipIndex, byte for byte against the definition (rag_dpo_amd/kmeans.py kmeans_model)
over the oracle's exact scores: labels, score bits, centroid bits, counts, n_iter, converged.

The rows are stored verbatim (add_stored), so a world's stored values are the test's own. Every claim about a world — which labels the
first assignment gives, how many members a cluster has, that two scores tie or lie one ulp apart, that an order probe tells the
definition's order from another — is asserted on the CPU from the oracle and the model before anything runs.

Worlds. (1) Rows r around direction r % K (labels interleaved: the stable order crosses every tile and block border) at dims 64 / 260 /
1024 (and 2048 / 4096: the any-dim form of the assignment), rows 1 .. 8 229, K 1 .. 4 096, as planned and with blocks of three tiles
(option km_tiles). (2) Clusters of exactly 0, 1, 255, 256, 257, 512 and 513 members. (3) A resident mask and a mask of zeros. (4) A row
that ties two centroids bit for bit and a pair of scores one ulp apart. (5) x and -x: a zero sum, a zero centroid. (6) Order probes for
the per-cluster sum (elements that span more than 2^53) and for the score's lane order."""
import numpy as np
import pytest

from rag_dpo_amd import kmeans as KM

pytestmark = pytest.mark.gpu

F32 = np.float32


def pack(allow):
    bits = np.packbits(allow, bitorder="little")
    return np.concatenate([bits, np.zeros(-len(bits) % 4, np.uint8)]).view(np.uint32)


def model(oracle, x, init, max_iter, allow=None, **kw):
    return KM.kmeans_model(x, init, max_iter, allow, scores_of=lambda q: oracle.scores(x, q), **kw)


class Index:
    """a HipIndex that holds x verbatim, and a resident mask where the case has one"""

    def __init__(self, x, allow=None):
        from rag_dpo_amd import engine as E
        self.E = E
        self.ix = E.HipIndex(x.shape[1])
        self.mask = None
        try:
            self.ix.add_stored(np.ascontiguousarray(x, dtype=np.float32))
            if allow is not None:
                self.mask = self.ix.make_mask(pack(allow))
        except BaseException:
            self.close()
            raise

    def run(self, init, max_iter, **options):
        import torch
        for name, v in options.items():
            self.ix.set_option(name, v)
        try:
            t = torch.from_numpy(np.ascontiguousarray(init, dtype=np.float32)).to(f"cuda:{self.ix.device}")
            lab, sc, cen, cnt, n_iter, conv = self.E.kmeans(self.ix, t, max_iter, self.mask)
        finally:
            for name in options:
                self.ix.set_option(name, 0)
        return lab.cpu().numpy(), sc.cpu().numpy(), cen.cpu().numpy(), cnt.cpu().numpy(), n_iter, conv

    def close(self):
        if self.mask is not None:
            self.mask.close()
        self.ix.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def same(got, want, what):
    """the definition's bytes: labels, score bits, centroid bits, counts, n_iter, converged"""
    lab, sc, cen, cnt, n_iter, conv = got
    wl, ws, wc, wn, w_iter, w_conv = want
    assert lab.dtype == np.int64 and sc.dtype == np.float32 and cen.dtype == np.float32 and cnt.dtype == np.int64
    assert lab.shape == wl.shape and sc.shape == ws.shape and cen.shape == wc.shape and cnt.shape == wn.shape, what
    assert (n_iter, conv) == (w_iter, w_conv), (what, n_iter, conv, w_iter, w_conv)
    assert lab.tobytes() == wl.tobytes(), (what, "labels", np.flatnonzero(lab != wl)[:8].tolist())
    assert sc.view(np.uint32).tobytes() == ws.view(np.uint32).tobytes(), (what, "scores", np.flatnonzero(sc.view(np.uint32) != ws.view(np.uint32))[:8].tolist())
    bad = np.argwhere(cen.view(np.uint32) != wc.view(np.uint32))
    assert bad.size == 0, (what, "centroids", bad[:8].tolist())
    assert cnt.tolist() == wn.tolist(), (what, "counts")


# ---- 1. interleaved labels -------------------------------------------------------------------------------------------------------
def interleaved(oracle, dim, rows, K, seed=0):
    """row r = direction r % K + 2 % noise, normalised; init = the directions, 30 % off"""
    rng = np.random.default_rng(1000003 * dim + 1009 * rows + K + seed)
    dirs = oracle.normalize_rows(rng.standard_normal((K, dim)).astype(F32))
    x = oracle.normalize_rows((dirs[np.arange(rows) % K] + 0.02 * rng.standard_normal((rows, dim)) / np.sqrt(dim)).astype(F32))
    init = (dirs + 0.3 * rng.standard_normal((K, dim)) / np.sqrt(dim)).astype(F32)
    return x, dirs, init


@pytest.mark.parametrize("dim,rows,K,max_iter", [
    (64, 1, 1, 3), (64, 63, 2, 5), (260, 63, 5, 5), (64, 257, 5, 5), (1024, 257, 65, 3), (260, 4097, 65, 3), (64, 4097, 4096, 1),
    (1024, 4097, 2, 5), (64, 8229, 65, 3), (260, 8229, 5, 5), (1024, 8229, 5, 3), (2048, 257, 5, 3), (4096, 63, 2, 3)])
def test_interleaved_labels(dim, rows, K, max_iter, oracle):
    x, dirs, init = interleaved(oracle, dim, rows, K)
    first = model(oracle, x, dirs, 0)
    assert first[0].tolist() == (np.arange(rows) % K).tolist()                       # the stable order meets every label in every tile
    assert first[3].tolist() == np.bincount(np.arange(rows) % K, minlength=K).tolist() and first[4:] == (0, False)
    want = model(oracle, x, init, max_iter)
    with Index(x) as ix:
        same(ix.run(dirs, 0), first, (dim, rows, K, "assign"))
        same(ix.run(init, max_iter), want, (dim, rows, K, max_iter))
        if rows > 3 * 256:
            same(ix.run(init, max_iter, km_tiles=3), want, (dim, rows, K, max_iter, "three tiles per block"))
        if max_iter != 1:
            same(ix.run(init, 1), model(oracle, x, init, 1), (dim, rows, K, 1))


# ---- 2. clusters of exactly 0, 1, 255, 256, 257, 512 and 513 members -----------------------------------------------------------
SIZES = [0, 1, 255, 256, 257, 512, 513]


@pytest.mark.parametrize("dim", [64, 260])
def test_clusters_at_the_segment_borders(dim, oracle):
    rng = np.random.default_rng(dim)
    K = len(SIZES)
    owner = rng.permutation(np.repeat(np.arange(K), SIZES))
    rows = len(owner)
    x = np.zeros((rows, dim), dtype=F32)
    x[np.arange(rows), 2 * owner] = 1.0                                              # cluster c lives around axis 2 c ...
    x[:, 20:40] = 0.2 * rng.standard_normal((rows, 20)).astype(F32)                  # ... with a spread on axes of their own
    x = oracle.normalize_rows(x)
    init = np.zeros((K, dim), dtype=F32)
    init[np.arange(K), 2 * np.arange(K)] = 1.0                                       # cluster 0's axis holds no row: it stays empty
    want = model(oracle, x, init, 4)
    assert want[3].tolist() == SIZES and want[0].tolist() == owner.tolist() and want[5]
    assert want[2][0].tolist() == init[0].tolist()                                   # the empty cluster kept its centroid
    with Index(x) as ix:
        same(ix.run(init, 4), want, (dim, "sizes"))
        same(ix.run(init, 1), model(oracle, x, init, 1), (dim, "sizes", 1))


# ---- 3. masks --------------------------------------------------------------------------------------------------------------------
def test_a_resident_mask_and_a_mask_of_zeros(oracle):
    dim, rows, K = 64, 4097, 5
    x, dirs, init = interleaved(oracle, dim, rows, K)
    allow = np.arange(rows) % 3 != 1
    allow[256:512] = False                                                           # a whole tile without a row
    want = model(oracle, x, init, 5, allow)
    assert (want[0][~allow] == -1).all() and np.isneginf(want[1][~allow]).all() and want[3].sum() == allow.sum()
    with Index(x, allow) as ix:
        same(ix.run(init, 5), want, "mask")
        same(ix.run(init, 0), model(oracle, x, init, 0, allow), "mask, assign")
    none = np.zeros(rows, dtype=bool)
    want = model(oracle, x, init, 5, none)
    assert (want[0] == -1).all() and want[3].tolist() == [0] * K and want[4:] == (1, True)
    assert want[2].tobytes() == KM.k1(init).tobytes()                                # nothing moved
    with Index(x, none) as ix:
        same(ix.run(init, 5), want, "mask of zeros")


# ---- 4. ties and neighbours -------------------------------------------------------------------------------------------------------
def test_a_tie_goes_to_the_smaller_index_and_one_ulp_decides(oracle):
    dim = 64
    a = F32(0.70710677)
    up = np.nextafter(a, F32(1.0))
    x = np.zeros((6, dim), dtype=F32)
    x[0, [0, 1]] = a                                                                 # ties centroids 0 and 1 bit for bit
    x[1, [0, 1]] = a, up                                                             # one ulp for centroid 1
    x[2, [0, 1]] = up, a                                                             # one ulp for centroid 0
    x[3, [1, 2]] = a                                                                 # ties centroids 1 and 2
    x[4, 5] = 1.0                                                                    # scores +0.0 against all of them
    x[5, [0, 1, 2]] = F32(0.57735026)                                                # ties all three
    init = np.eye(3, dim, dtype=F32)
    init = np.concatenate([init, init[1:2]])                                         # centroid 3 = centroid 1: the later one stays empty
    q = KM.k1(init)
    s = np.stack([oracle.scores(x, q[c]) for c in range(4)])
    assert s[0, 0] == s[1, 0] and s[1, 1].view(np.uint32) == s[0, 1].view(np.uint32) + 1 and s[0, 2].view(np.uint32) == s[1, 2].view(np.uint32) + 1
    assert s[1, 3] == s[2, 3] and (s[:, 4] == 0).all() and s[0, 5] == s[1, 5] == s[2, 5] and (s[1] == s[3]).all()
    want = model(oracle, x, init, 0)
    assert want[0].tolist() == [0, 1, 0, 1, 0, 0] and want[3].tolist() == [4, 2, 0, 0]
    with Index(x) as ix:
        same(ix.run(init, 0), want, "ties")
        same(ix.run(init, 3), model(oracle, x, init, 3), "ties, iterated")


# ---- 5. a zero sum ---------------------------------------------------------------------------------------------------------------
def test_x_and_minus_x_give_a_zero_centroid(oracle):
    dim = 64
    rng = np.random.default_rng(9)
    v = oracle.normalize_rows(rng.standard_normal((3, dim)).astype(F32))
    x = np.concatenate([v, -v])
    init = np.ones((1, dim), dtype=F32)
    want = model(oracle, x, init, 3)
    assert not want[2].any() and not want[1].any() and want[3].tolist() == [6] and want[4:] == (1, True)
    with Index(x) as ix:
        same(ix.run(init, 3), want, "zero sum")


# ---- 6. order probes --------------------------------------------------------------------------------------------------------------
T = F32(0.4 * 2.0 ** -52)                                                            # 1 + T = 1 in fp64, 1 + 2 T = 1 + 2^-52


def sum_probe_rows(rows=700, dim=64):
    """one cluster of every row; column 0: 1, -1, 2^-60 at members 0, 256, 257; column 1: 1, T, T, -1 at members 0, 128, 129, 300; column 2:
    ones, which carry the centroid's norm"""
    x = np.zeros((rows, dim), dtype=F32)
    x[[0, 256, 257], 0] = 1.0, -1.0, 2.0 ** -60
    x[[0, 128, 129, 300], 1] = 1.0, T, T, -1.0
    x[:, 2] = 1.0
    return x


def test_the_sum_s_order_shows(oracle):
    x = sum_probe_rows()
    rows, dim = x.shape
    init = np.zeros((1, dim), dtype=F32)
    init[0, 2] = 1.0
    labels = np.zeros(rows, dtype=np.int64)
    c0 = KM.k1(init)
    definition = KM.update(x, labels, c0)
    assert definition[0, 0] == 0 and definition[0, 1] == 0 and definition[0, 2] == 1   # 1 + (-1 + 2^-60) and (1 + T + T) + (-1) in fp64
    others = {"sequential": KM.update(x, labels, c0, segment=1 << 30), "segments of 128": KM.update(x, labels, c0, segment=128),
              "segments of 512": KM.update(x, labels, c0, segment=512),
              "numpy's sum": KM.k1(x.astype(np.float64).sum(axis=0).astype(F32)[None, :])}
    for name, c in others.items():                                                   # the probes are not vacuous
        assert c.view(np.uint32).tobytes() != definition.view(np.uint32).tobytes(), name
    want = model(oracle, x, init, 1)
    assert want[2].tobytes() == definition.tobytes() and want[3].tolist() == [rows]
    with Index(x) as ix:
        same(ix.run(init, 1), want, "sum probes")
        same(ix.run(init, 1, km_tiles=2), want, "sum probes, two tiles per block")


def lane_sum_variant(prod, lanes):
    """the lane-order sum with another number of lanes (1 = plain sequential)"""
    p = np.asarray(prod, dtype=np.float64).reshape(-1, 4)
    acc = np.zeros(lanes, dtype=np.float64)
    for g in range(p.shape[0]):
        for e in range(4):
            acc[g % lanes] += p[g, e]
    while lanes > 1:
        lanes //= 2
        acc = acc[:lanes] + acc[lanes: 2 * lanes]
    return acc[0]


def test_the_score_s_lane_order_shows(oracle):
    dim = 1024
    x = np.zeros((3, dim), dtype=F32)
    x[0, [0, 4, 5, 256]] = 1.0, T, T, -1.0                                           # groups 0, 1, 1, 64: lanes 0, 1, 1, 0
    x[1, [0, 128, 129, 256]] = 1.0, T, T, -1.0                                       # groups 0, 32, 32, 64: lanes 0, 32, 32, 0 of 64
    x[2, :] = 1.0
    init = np.stack([np.ones(dim, dtype=F32), -np.ones(dim, dtype=F32)])
    q = KM.k1(init)
    assert (q[0] == F32(1 / 32)).all()                                               # a power of two: every product is exact, the order alone decides
    s = oracle.scores(x, q[0])
    assert s[:2].tolist() == [F32(2 * np.float64(T) / 32)] * 2 and s[2] == 32
    for lanes, row in ((1, 0), (32, 1)):                                             # another order gives other bits: the probes are not vacuous
        other = F32(lane_sum_variant(q[0].astype(np.float64) * x[row].astype(np.float64), lanes))
        assert other == 0 and other != s[row], lanes
    assert F32(lane_sum_variant(q[0].astype(np.float64) * x[0].astype(np.float64), 64)) == s[0]
    want = model(oracle, x, init, 0)
    assert want[0].tolist() == [0, 0, 0] and want[1].tolist() == s.tolist()
    with Index(x) as ix:
        same(ix.run(init, 0), want, "lane order")


# ---- refusals at the C-ABI --------------------------------------------------------------------------------------------------------
def test_argument_checks():
    import torch
    from rag_dpo_amd import engine as E
    ix, other = E.HipIndex(64), E.HipIndex(64)
    mask = None
    try:
        init = torch.eye(3, 64, device="cuda")
        with pytest.raises(ValueError, match="empty"):
            E.kmeans(ix, init, 1)
        ix.add(np.eye(8, 64, dtype=np.float32))
        other.add(np.eye(9, 64, dtype=np.float32))
        mask = other.make_mask(pack(np.ones(9, dtype=bool)))
        for bad in (dict(init=torch.zeros((0, 64), device="cuda")), dict(init=torch.zeros((4097, 64), device="cuda")), dict(max_iter=-1),
                    dict(max_iter=1001), dict(mask=mask), dict(init=torch.eye(3, 60, device="cuda")), dict(init=np.eye(3, 64, dtype=np.float32))):
            with pytest.raises((ValueError, AttributeError)):
                E.kmeans(ix, **{"init": init, "max_iter": 1, **bad})
        for poison in (float("nan"), float("inf")):
            bad_init = init.clone()
            bad_init[1, 5] = poison
            with pytest.raises(ValueError, match="NaN or Inf"):
                E.kmeans(ix, bad_init, 1)
        with pytest.raises(ValueError):
            ix.set_option("km_tiles", 4097)
        got = E.kmeans(ix, init, 2)
        assert got[0].cpu().tolist() == [0, 1, 2, 0, 0, 0, 0, 0] and got[3].cpu().tolist() == [6, 1, 1] and got[4:] == (1, True)
        ix.set_option("row_base", 5)                                                 # a shard's index returns mapped ids
        with pytest.raises(E.L.RdxError, match="mapped row ids"):
            E.kmeans(ix, init, 1)
    finally:
        if mask is not None:
            mask.close()
        other.close()
        ix.close()
