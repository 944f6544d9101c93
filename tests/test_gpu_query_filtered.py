"""GPU end to end: Collection.query_filtered_device (one rdx_search_filtered) against the loop of query_device with each
query's own filters — `where`, `where_document`, after a delete (tombstones: "no filter" becomes the alive mask) and after an add (the
masks are rebuilt) — and DenseRetriever.retrieve_candidates_batch with several where_filters under fusion="device" against
fusion="host"."""
import numpy as np
import pytest

import bm25_replay as R
from bm25_replay import W
from rag_dpo_amd import synth
from rag_dpo_amd.collection import Collection
from rag_dpo_amd.retriever import DenseRetriever
from test_gpu_fusion import DeviceHashEmbedder, chunk_values

pytestmark = pytest.mark.gpu

N, DIM, NQ, K = 20_000, 64, 70, 10


def user_where(tags):
    """the reference's per-user filter (src/rag/pipeline.py:35-71)"""
    return {"$or": [{"source": {"$ne": "ENTREPRISE"}}] + [{"tag": t} for t in tags]}


@pytest.fixture(scope="module")
def case():
    corpus = synth.make_corpus(N + 500, DIM)
    col = Collection("filtered", metadata={"hnsw:space": "cosine"})
    col.add(ids=[f"c{i}" for i in range(N)], embeddings=corpus[:N], documents=[f"chunk {i} topic{i % 7} {'pensions' if i % 4 == 0 else 'contracts'}" for i in range(N)],
            metadatas=[{"source": "ENTREPRISE" if i % 3 == 0 else "PUBLIC", "tag": f"t{i % 5}", "n": i} for i in range(N)])
    return col, corpus, synth.make_queries(NQ, DIM, corpus[:N])


def wheres_of(nq):
    pool = [user_where(["t1"]), user_where(["t2", "t4"]), None, {"source": "ENTREPRISE"}, {"n": {"$lt": 4}}, {"tag": "none"}, {}]
    return [pool[i % len(pool)] for i in range(nq)]


def check(col, q, wheres, wds):
    import torch
    qd = torch.from_numpy(q).cuda()
    filtered = getattr(col._engine, "search_filtered_device")
    calls = []

    def spy(*a, **kw):
        calls.append(len(a[5]))
        return filtered(*a, **kw)
    col._engine.search_filtered_device = spy
    try:
        got = col.query_filtered_device(qd, wheres, n_results=K, where_documents=wds)
    finally:
        del col._engine.search_filtered_device
    assert len(calls) == 1                                      # ONE search of the engine
    for i in range(len(q)):
        want = col.query_device(qd[i:i + 1], n_results=K, where=wheres[i], where_document=None if wds is None else wds[i])
        for g, w, name in zip(got, want, ("distances", "rows", "counts")):
            np.testing.assert_array_equal(g[i:i + 1].cpu().numpy(), w.cpu().numpy(), err_msg=f"query {i}: {name}")
    host = col.query_filtered(q, wheres, n_results=K, where_documents=wds, include=["distances"])
    rows, cnt = got[1].cpu().numpy(), got[2].cpu().numpy()
    assert host["ids"] == col.ids_of(rows) and [len(x) for x in host["ids"]] == cnt.tolist()
    return calls[0], cnt


def test_query_filtered_device_against_the_loop(case):
    col, corpus, q = case
    wheres = wheres_of(NQ)
    n_masks, cnt = check(col, q, wheres, None)
    assert n_masks == 5 and cnt[4] == 4 and cnt[5] == 0 and cnt[0] == K
    wds = ([None, {"$contains": "pensions"}, {"$contains": "topic3"}, {}, {"$not_contains": "contracts"}] * NQ)[:NQ]
    check(col, q, wheres, wds)
    # tombstones: every query is filtered now, "no filter" by the alive mask
    top = col.query(query_embeddings=q[2:3], n_results=3)["ids"][0]
    col.delete(ids=top + [f"c{i}" for i in range(100, 160)])
    n_masks, _ = check(col, q, wheres, None)
    assert n_masks == 7
    assert not set(top) & set(col.query_filtered(q[2:3], [None], n_results=K)["ids"][0])
    # an add drops the masks: they are made again for the new row count
    col.add(ids=[f"c{i}" for i in range(N, N + 500)], embeddings=corpus[N:], documents=[f"chunk {i} pensions" for i in range(N, N + 500)],
            metadatas=[{"source": "PUBLIC", "tag": "t1", "n": i} for i in range(N, N + 500)])
    check(col, q, wheres, wds)


def test_batch_with_several_where_filters_fused_on_the_device(tmp_path):
    col = W.build_collection(None)
    chunk, summ = R.chunk_index(None), R.summary_index(None, str(tmp_path))
    queries = [W.Q0, "registre des traitements du sous-traitant article 28", "notification d'une violation en 72 heures",
               "biométrie badge salariés", "durée de conservation des données"]
    wheres = [None, {"chunk_nature": {"$in": ["GUIDE", "DOCTRINE"]}}, {"chunk_nature": "GUIDE"}, {"chunk_nature": {"$ne": "GUIDE"}},
              {"chunk_nature": {"$in": ["GUIDE", "DOCTRINE"]}}]
    made = []
    real = col.query_filtered_device

    def spy(*a, **kw):
        made.append(len(a[1]))
        return real(*a, **kw)
    col.query_filtered_device = spy
    dev = DenseRetriever(col, DeviceHashEmbedder(), query_expander=W.expander, summary_bm25_index=summ, chunk_bm25_index=chunk, fusion="device")
    got = dev.retrieve_candidates_batch(queries, n_candidates=40, where_filter=wheres)
    del col.query_filtered_device
    assert len(made) == 1 and made[0] >= len(queries)          # one dense search for every sub-query of the batch
    host = DenseRetriever(col, DeviceHashEmbedder(), query_expander=W.expander, summary_bm25_index=summ, chunk_bm25_index=chunk, fusion="host")
    want = host.retrieve_candidates_batch(queries, 40, wheres)
    assert [[chunk_values(c) for c in g] for g in got] == [[chunk_values(c) for c in g] for g in want]
    assert all(len(g) > 0 for g in got)
