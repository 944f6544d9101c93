"""The index's row storage through a reallocation and a compaction (rdx_index.hpp RowStore): both master forms and the row-id map
are carried from the old arrays to the new ones. After every step the count, the returned ids and the score bits are the CPU
oracle's, on the path the library picks, on the exact full scan and on the MFMA path.

  300 rows, an id map 3 i + 7 over them        capacity 512
  300 more                                     512 -> 768: the map's old entries are kept, the new ones are local row + row_base
  compact to every third row                   256; the rows are renumbered, the map is gone: local row + row_base
"""
import numpy as np
import pytest

from rag_dpo_amd import synth

pytestmark = pytest.mark.gpu

D, NQ, K, BASE = 64, 3, 5, 1000
MODES = ({}, {"force_exact": 1}, {"force_fast": 1})


@pytest.fixture(scope="module")
def data():
    corpus = synth.make_corpus(600, D, duplicates=False)
    return corpus, synth.make_queries(NQ, D, corpus)


def _check(oracle, ix, rows, q, ids):
    """rows: the raw rows the index holds; ids: what local row r is returned as"""
    es, er, ec = oracle.cosine_topk(oracle.normalize_rows(rows), q, K)
    want = np.where(er >= 0, ids[np.maximum(er, 0)], -1)
    for mode in MODES:
        for name, v in mode.items():
            ix.set_option(name, v)
        gs, gr, gc = ix.search(q, K)
        if mode:
            assert ix.last_stats()["path"] == (1 if "force_exact" in mode else 0), mode
        for name in mode:
            ix.set_option(name, 0)
        assert len(ix) == len(rows)
        np.testing.assert_array_equal(gc, ec, err_msg=str(mode))
        np.testing.assert_array_equal(gr, want, err_msg=str(mode))
        np.testing.assert_array_equal(gs, es, err_msg=str(mode))


@pytest.mark.parametrize("compact_master", [0, 1])
def test_rows_and_id_map_through_growth_and_compaction(oracle, data, compact_master):
    import torch
    from rag_dpo_amd import engine
    corpus, q = data
    ix = engine.HipIndex(D)
    ix.set_option("compact_master", compact_master)
    ix.set_option("row_base", BASE)
    if compact_master:                                       # bf16 rows: the oracle on the widened values (test_gpu_parity's bf16 cases)
        cb = torch.from_numpy(corpus).to(torch.bfloat16)
        held = cb.to(torch.float32).numpy()
        add = lambda a, b: ix.add_bf16(cb[a:b])
    else:
        held = corpus
        add = lambda a, b: ix.add(corpus[a:b])
    add(0, 300)
    ids = 3 * np.arange(300, dtype=np.int64) + 7
    ix.set_row_ids(0, ids)
    _check(oracle, ix, held[:300], q, ids)
    add(300, 600)
    ids = np.concatenate([ids, BASE + np.arange(300, 600, dtype=np.int64)])
    _check(oracle, ix, held, q, ids)
    keep = np.arange(0, 600, 3)
    ix.compact(keep)
    _check(oracle, ix, held[keep], q, BASE + np.arange(keep.size, dtype=np.int64))
    if not compact_master:
        np.testing.assert_array_equal(ix.get(np.arange(keep.size)), oracle.normalize_rows(held[keep]))
    ix.close()
