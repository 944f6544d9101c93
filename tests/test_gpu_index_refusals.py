"""GPU: the refusals that the index's derived searches share (rdx_index.hip check_mask / check_own_rows, called from rdx_derived.hip too), word for word and code for
code, and that a refused call leaves the index usable.

An index of dim 64 with 256 rows, a resident mask made for it, then one more row: the mask is stale. rdx_search_masked and
rdx_index_group_fill refuse it with RDX_ERR_STATE (engine: RdxError "librdx error 4: ..."), rdx_index_range and rdx_index_near_dup with
RDX_ERR_INVALID (ValueError), as include/rdx.h documents; every message names its own entry point and ends in the same clause.
A shard — a row-id map, or option row_base — is refused by rdx_index_group_fill, rdx_index_mmr, rdx_index_range and rdx_index_near_dup
with RDX_ERR_STATE, each with its own tail. Where a call is given a stale mask on a shard, the mask's refusal comes first.
Every call here is refused on the host before anything is launched; after each one a plain search returns the oracle's rows."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DIM, ROWS, K, BASE = 64, 256, 5, 1000
STALE = (" the mask was made for 256 rows on device 0, the index now holds 257 (a mask does not outlive a write to the index)")
SHARD = " the index returns mapped row ids (a shard): "
TAILS = {"rdx_index_group_fill": "group_rows must be the index's own rows", "rdx_index_mmr": "cand_row must be the index's own rows",
         "rdx_index_range": "not available", "rdx_index_near_dup": "not available"}

_cache = {}


def _data(oracle):
    """(257 rows, queries, the oracle's answer over the first 256 rows and over all 257), once"""
    if not _cache:
        rng = np.random.default_rng(64256)
        corpus = rng.standard_normal((ROWS + 1, DIM)).astype(np.float32)
        q = (corpus[[3, 100, 255, 256]] + 0.3 * rng.standard_normal((4, DIM))).astype(np.float32)
        ref256 = oracle.cosine_topk(oracle.normalize_rows(corpus[:ROWS]), q, K)
        ref257 = oracle.cosine_topk(oracle.normalize_rows(corpus), q, K)
        for a in (corpus, q) + ref256 + ref257:
            a.setflags(write=False)
        _cache["d"] = corpus, q, ref256, ref257
    return _cache["d"]


def _usable(ix, q, ref, ids):
    """a plain search answers as the oracle does (local row r is returned as ids[r])"""
    gs, gr, gc = ix.search(q, K)
    es, er, ec = ref
    np.testing.assert_array_equal(gc, ec)
    np.testing.assert_array_equal(gs.view(np.uint32), es.view(np.uint32))
    np.testing.assert_array_equal(gr, ids[er])


def _calls(ix, q, mask):
    """{entry point: a call of it with arguments that pass every check before the mask's and the shard's} (mask: None where the entry
    point takes none or the case gives none)"""
    import torch
    from rag_dpo_amd import engine
    dev = torch.device("cuda", ix.device)
    tq = torch.from_numpy(np.array(q)).to(dev)
    group_rows = torch.arange(8, dtype=torch.int64, device=dev)
    cand = (torch.zeros((1, 4), dtype=torch.float32, device=dev), torch.arange(4, dtype=torch.int64, device=dev).reshape(1, 4),
            torch.full((1,), 4, dtype=torch.int32, device=dev))
    thr = torch.full((tq.shape[0],), 0.5, dtype=torch.float32, device=dev)
    return {
        "rdx_search_masked": lambda: ix.search(q, K, mask=mask),
        "rdx_index_group_fill": lambda: engine.group_fill(ix, tq, [0, 1], [0, 4], [4, 8], group_rows, 2, mask=mask),
        "rdx_index_mmr": lambda: engine.mmr_select(ix, *cand, 2, 0.5),
        "rdx_index_range": lambda: engine.range_search(ix, tq, thr, 8, mask=mask),
        "rdx_index_near_dup": lambda: engine.near_dup(ix, 0.9, mask=mask),
    }


def _refused(call, state: bool, message: str):
    """the call raises RDX_ERR_STATE's exception (state) or RDX_ERR_INVALID's, with exactly this message"""
    from rag_dpo_amd import _lib
    if state:
        with pytest.raises(_lib.RdxError) as e:
            call()
        assert str(e.value) == "librdx error 4: " + message
    else:
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == message


def _stale(corpus):
    """-> (an index of 257 rows, a mask made when it held 256)"""
    from rag_dpo_amd import engine
    ix = engine.HipIndex(DIM)
    ix.add(corpus[:ROWS])
    mask = ix.make_mask(np.full(ROWS // 32, 0xFFFFFFFF, dtype=np.uint32))
    ix.add(corpus[ROWS:])
    return ix, mask


def test_stale_mask(oracle):
    corpus, q, _, ref257 = _data(oracle)
    ix, mask = _stale(corpus)
    own = np.arange(ROWS + 1, dtype=np.int64)
    calls = _calls(ix, q, mask)
    for who, state in (("rdx_search_masked", True), ("rdx_index_group_fill", True), ("rdx_index_range", False), ("rdx_index_near_dup", False)):
        _refused(calls[who], state, who + ":" + STALE)
        _usable(ix, q, ref257, own)
    mask.close()
    ix.close()


@pytest.mark.parametrize("mapped", [True, False], ids=["id_map", "row_base"])
def test_shard(oracle, mapped):
    from rag_dpo_amd import engine
    corpus, q, ref256, _ = _data(oracle)
    ix = engine.HipIndex(DIM)
    ix.add(corpus[:ROWS])
    if mapped:
        ids = 3 * np.arange(ROWS, dtype=np.int64) + 7
        ix.set_row_ids(0, ids)
    else:
        ids = BASE + np.arange(ROWS, dtype=np.int64)
        ix.set_option("row_base", BASE)
    calls = _calls(ix, q, None)
    for who, tail in TAILS.items():
        _refused(calls[who], True, who + ":" + SHARD + tail)
        _usable(ix, q, ref256, ids)
    ix.close()


def test_stale_mask_on_a_shard_the_mask_is_refused_first(oracle):
    corpus, q, _, ref257 = _data(oracle)
    ix, mask = _stale(corpus)
    ix.set_option("row_base", BASE)
    ids = BASE + np.arange(ROWS + 1, dtype=np.int64)
    calls = _calls(ix, q, mask)
    for who, state in (("rdx_index_group_fill", True), ("rdx_index_range", False), ("rdx_index_near_dup", False)):
        _refused(calls[who], state, who + ":" + STALE)
        _usable(ix, q, ref257, ids)
    _refused(calls["rdx_index_mmr"], True, "rdx_index_mmr:" + SHARD + TAILS["rdx_index_mmr"])   # (takes no mask)
    _usable(ix, q, ref257, ids)
    mask.close()
    ix.close()
