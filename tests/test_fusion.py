"""CPU: the Python side of the GPU rank fusion (rag_dpo_amd/fusion.py): packing and unpacking, Collection.rows_of and the write counter
the row tables are keyed on, and DenseRetriever.retrieve_candidates_batch on the host path — against the per-question loop and against
the two fixtures captured from the reference (tests/golden/bm25_golden.json, retriever_golden.json). The kernel itself:
tests/test_gpu_fusion.py."""
import json
import os
import sys

import numpy as np
import pytest

import bm25_oracle as O
import bm25_replay as R
import fusion_model as M
from bm25_replay import W
from oracle_engine import factory as dense_cpu
from rag_dpo_amd import fusion as F
from rag_dpo_amd.collection import Collection
from rag_dpo_amd.retriever import DenseRetriever

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def chunk():
    return R.chunk_index(O.factory)


@pytest.fixture(scope="module")
def summ(tmp_path_factory):
    return R.summary_index(O.factory, str(tmp_path_factory.mktemp("summaries")))


def chunk_floats(c):
    return (c.chunk_id, c.text, c.document_path, c.chunk_nature, c.chunk_index, c.confidence, c.distance, repr(float(c.bm25_score)),
            c.semantic_score, c.hybrid_score, json.dumps(c.metadata, sort_keys=True))


def test_pack_round_trip():
    rng = np.random.default_rng(3)
    questions = [c["lists"] for c in M.named_cases().values()] + [M.random_question(rng, 3, 9) for _ in range(20)]
    filters = [c["allowed"] for c in M.named_cases().values()] + [M.random_filter(rng) for _ in range(20)]
    p = M.pack(questions, 6, 12, filters)
    assert p.keys.shape == (len(questions), 6, 12) and p.keys.dtype == np.int64 and p.dist.dtype == np.float32 and p.score.dtype == np.float64
    for q, (lists, flt) in enumerate(zip(questions, filters)):
        assert p.lists_of(q) == list(lists) + [None] * (6 - len(lists))
        assert p.allowed_groups_of(q) == (None if flt is None else sorted(flt))
    assert p.group_words == 2 and p.allow.shape == (len(questions), 2)
    assert (p.count[0] == [5, -1, -1, -1, -1, -1]).all()                         # never set = absent
    for bad in ((17, 8), (8, 513), (16, 65), (0, 8), (8, 0)):                   # lists, entries per list, entries per question
        with pytest.raises(ValueError, match="limits"):
            F.PackedLists(1, *bad)
    assert F.fits(8, 128, 100) and F.fits(16, 64, 1024) and F.fits(2, 512, 1)
    assert not F.fits(8, 128, 1025) and not F.fits(8, 128, 0) and not F.fits(8, 129, 10)
    with pytest.raises(ValueError):
        p.set_list(0, 0, F.DENSE, 2.0, list(range(13)), [0.0] * 13)


def test_unpack_reads_the_output_layout():
    nq, top_n = 3, 4
    lay, nbytes = F._out_layout(nq, top_n)
    buf = np.zeros(nbytes, np.uint8)
    want = []
    for q, c in enumerate((0, 2, 4)):
        np.frombuffer(buf, np.int32, nq, lay["count"][0])[q] = c
        ws = []
        for j in range(c):
            w = F.Winner(key=100 * q + j - 3, distance=float(np.float32(0.1 * j + q)), semantic_score=1.0 / (3 + j), bm25_score=2.5 * j,
                         hybrid_score=0.01 * (q + 1) / (j + 1), first_list=j % 3, first_rank=7 * j)
            for name, val in (("key", w.key), ("distance", w.distance), ("semantic", w.semantic_score), ("bm25", w.bm25_score),
                              ("hybrid", w.hybrid_score), ("list", w.first_list), ("rank", w.first_rank)):
                off, dt, shape = lay[name]
                np.frombuffer(buf, dt, nq * top_n, off).reshape(shape)[q, j] = val
            ws.append(w)
        want.append(ws)
    assert F.unpack(buf, nq, top_n) == want
    assert all(off % dt.itemsize == 0 for off, dt, _ in lay.values())


def small_collection():
    col = Collection("c", engine_factory=dense_cpu)
    rng = np.random.default_rng(0)
    paths = ["b.html", "a.html", "b.html", None, "c.html", "a.html"]
    col.add(ids=[f"id{i}" for i in range(6)], embeddings=rng.standard_normal((6, 8)).astype(np.float32).tolist(),
            documents=[f"texte {i}" for i in range(6)],
            metadatas=[{"document_path": p, "n": i} if p else {"n": i} for i, p in enumerate(paths)])
    return col, rng


def test_rows_of_is_the_inverse_of_ids_of():
    col, _ = small_collection()
    assert col.rows_of(["id3", "nope", "id0", "id5"]) == [3, -1, 0, 5]
    assert col.rows_of([]) == []
    assert col.ids_of([col.rows_of(["id4", "id1"])]) == [["id4", "id1"]]
    col.delete(ids=["id3"])
    assert col.rows_of(["id3", "id4"]) == [-1, 4]
    ids, docs, metas = col.payload_of([4, 0])
    assert ids == ["id4", "id0"] and docs == ["texte 4", "texte 0"] and metas == [{"document_path": "c.html", "n": 4}, {"document_path": "b.html", "n": 0}]


def test_every_write_invalidates_the_group_table():
    col, rng = small_collection()
    t = F.row_tables(col)
    assert t.group_of == {"b.html": 0, "a.html": 1, "": 2, "c.html": 3}          # first-appearance order; no path = ""
    assert t.row_group.tolist() == [0, 1, 0, 2, 3, 1] and t.row_group.dtype == np.int32 and t.n_groups == 4
    assert sorted(t.groups_allowed({"a.html", "zzz", "c.html"})) == [1, 3]
    assert F.row_tables(col) is t                                               # no write: the same table
    vec = lambda n: rng.standard_normal((n, 8)).astype(np.float32).tolist()
    writes = [lambda: col.add(ids=["id6"], embeddings=vec(1), metadatas=[{"document_path": "d.html"}]),
              lambda: col.update(ids=["id0"], metadatas=[{"document_path": "c.html"}]),
              lambda: col.upsert(ids=["id1", "id7"], embeddings=vec(2), metadatas=[{"document_path": "e.html"}, {"document_path": "a.html"}]),
              lambda: col.delete(ids=["id2"])]
    for w in writes:
        before = col.write_count
        w()
        assert col.write_count > before
        t2 = F.row_tables(col)
        assert t2 is not t and t2.write_count == col.write_count
        t = t2
    assert t.row_group.tolist()[:2] == [0, 1] and t.group_of["c.html"] == 0 and t.group_of["e.html"] == 1   # rows 0 and 1 changed their path
    before = col.write_count
    col.add(ids=["id0"], embeddings=vec(1))                                     # an existing id: add skips it, nothing was written
    col.update(ids=["nope"], metadatas=[{"x": 1}])
    col.delete(ids=["nope"])
    assert col.write_count == before and F.row_tables(col) is t
    col._compact()
    assert col.write_count > before and len(F.row_tables(col).row_group) == col.count()
    # the BM25 row -> key table: the collection row, or a distinct negative key for an id the collection no longer holds

    class Ix:
        chunk_ids = ["id5", "id2", "id0", "gone"]
    assert F.row_tables(col).bm25_keys(col, Ix).tolist() == [col.rows_of(["id5"])[0], -3, col.rows_of(["id0"])[0], -5]


def test_batch_on_the_host_path_equals_the_loop(summ, chunk):
    col = W.build_collection(dense_cpu)
    queries = [c["query"] for c in W.RETRIEVER_QUERIES[:3]] + ["biométrie badge salariés", "zzzinconnu"]
    wheres = [None, {"chunk_nature": {"$in": ["GUIDE", "DOCTRINE"]}}, None, None, {"source": "CNIL"}]
    for fusion in ("host", "auto"):         # (the oracle engine has no device search: "auto" takes the host path)
        r = DenseRetriever(col, W.HashEmbedder(), query_expander=W.expander, summary_bm25_index=summ, chunk_bm25_index=chunk, fusion=fusion)
        got = r.retrieve_candidates_batch(queries, n_candidates=40, where_filter=wheres)
        loop = [r.retrieve_candidates(q, n_candidates=40, where_filter=w) for q, w in zip(queries, wheres)]
        assert [[chunk_floats(c) for c in g] for g in got] == [[chunk_floats(c) for c in g] for g in loop]
        assert all(len(g) > 0 for g in got[:4])
        one = r.retrieve_candidates_batch(queries[:2], n_candidates=40, where_filter=wheres[1])       # one filter for every question
        assert [chunk_floats(c) for c in one[1]] == [chunk_floats(c) for c in loop[1]]
    assert r.retrieve_candidates_batch([], n_candidates=40) == []
    with pytest.raises(ValueError, match="filters"):
        r.retrieve_candidates_batch(queries, where_filter=[None])
    with pytest.raises(ValueError, match="fusion"):
        DenseRetriever(col, W.HashEmbedder(), fusion="gpu")


def test_device_fusion_without_a_gpu_collection_raises():
    col, _ = small_collection()
    r = DenseRetriever(col, W.HashEmbedder(), fusion="device")
    with pytest.raises(RuntimeError):       # RdxUnavailable without a GPU; with one, the oracle engine has no device search
        r.retrieve_candidates_batch(["question"])


def test_batch_replays_the_bm25_fixture(summ, chunk):
    """tests/golden/bm25_golden.json's retrieve_candidates, to the reference's floats, all cases of one configuration in one batch"""
    cases = R.GOLD["retriever"]
    for key in sorted({(c["expand"], c["prefilter"], tuple(c["poison_sub"]), c["n_candidates"]) for c in cases}):
        group = [c for c in cases if (c["expand"], c["prefilter"], tuple(c["poison_sub"]), c["n_candidates"]) == key]
        r = DenseRetriever(W.build_collection(dense_cpu), W.HashEmbedder(key[2]), query_expander=W.expander if key[0] else None,
                           summary_bm25_index=summ, chunk_bm25_index=chunk, enable_summary_prefilter=key[1], fusion="host")
        got = r.retrieve_candidates_batch([c["query"] for c in group], n_candidates=key[3], where_filter=[c["where"] for c in group])
        for cands, case in zip(got, group):
            assert len(cands) == len(case["candidates"])
            for c, g in zip(cands, case["candidates"]):
                R._same_chunk(c, g)


def test_batch_replays_the_retriever_fixture():
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import fixture_world as FW
    import test_retriever_golden as T
    cases = T.GOLD["cases"]
    for key in sorted({(c["expand"], c["n_candidates"]) for c in cases}):
        group = [c for c in cases if (c["expand"], c["n_candidates"]) == key]
        r = DenseRetriever(FW.build_collection(dense_cpu), FW.HashEmbedder(), query_expander=FW.expander if key[0] else None, fusion="host")
        got = r.retrieve_candidates_batch([c["query"] for c in group], n_candidates=key[1], where_filter=[c["where"] for c in group])
        for cands, case in zip(got, group):
            gold = case["retrieve_candidates"]["chunks"]
            assert len(cands) == len(gold)
            for c, g in zip(cands, gold):
                T._same_chunk(c, g)


def test_model_is_fuse_itself():
    """the model of the GPU tests drives DenseRetriever._fuse: two hand-checked answers pin the plumbing around it"""
    c = M.named_cases()["BM25 first, then dense above 1.0"]
    out, distinct = M.run_model(c["lists"])
    by_key = {o[0]: o for o in out}
    assert distinct == 2 and by_key[7][1] == np.float32(1.0) and by_key[7][2] == 1.0 / (1.0 + float(np.float32(1.2))) and by_key[7][5:] == (1, 0)
    assert by_key[7][4] == 3.0 / 61 + 1.0 / 61 and by_key[1][4] == 2.0 / 61
    c = M.named_cases()["filter keeps min_semantic - 1"]
    out, distinct = M.run_model(c["lists"], c["allowed"], c["min_semantic"])
    dense_first = [o[0] for o in sorted(out, key=lambda o: o[6]) if o[5] == 0]
    assert len(dense_first) == 4 and distinct == 4 + 1     # three allowed, one refused entry tops the list up; one BM25-only key


def test_summary_filters_of_a_batch_equal_the_single_searches(summ, chunk):
    queries = [q for q, _ in W.SUMMARY_QUERIES] + [W.Q0]
    assert summ.get_relevant_doc_paths_batch(queries, top_k=20) == [summ.get_relevant_doc_paths(q, top_k=20) for q in queries]
    r = DenseRetriever(None, None, summary_bm25_index=summ)
    assert r._doc_filters(queries) == [r._doc_filter(q) for q in queries]
    assert DenseRetriever(None, None, summary_bm25_index=summ, enable_summary_prefilter=False)._doc_filters(queries) == [None] * len(queries)
    live, sc, ro, cn = chunk.search_batch_arrays(queries, top_k=30)
    objs = chunk.search_batch(queries, top_k=30)
    for j, i in enumerate(live):
        assert [chunk.result_of(int(x), float(s)) for x, s in zip(ro[j, :cn[j]], sc[j, :cn[j]])] == objs[i]
    assert all(objs[i] == [] for i in range(len(queries)) if i not in live)
    assert chunk.search_batch_arrays(queries, top_k=30, doc_filter=set())[0] == []


def test_the_entry_point_validates_before_it_touches_a_device():
    """no GPU needed: every refusal comes before the first HIP call"""
    import ctypes
    from rag_dpo_amd import _lib
    from rag_dpo_amd.build import build_lib
    build_lib()
    lib = _lib.load(require_gpu=False)
    buf = (ctypes.c_uint8 * (1 << 16))()
    p = ctypes.addressof(buf)

    def rc(nq=1, n_lists=8, stride=50, top_n=40, min_semantic=10, keep=1, rrf=60, space=_lib.RDX_HOST, keys=p, weight=p, filter_on=None, allow=None):
        vp = ctypes.c_void_p
        return lib.rdx_fuse_rankings(0, nq, n_lists, stride, vp(p), vp(weight), vp(p), vp(keys), vp(p), vp(p), None, 0, filter_on, allow, 0,
                                     min_semantic, keep, rrf, top_n, vp(p), vp(p), vp(p), vp(p), vp(p), vp(p), vp(p), vp(p), space, None)
    for kw, msg in ((dict(n_lists=17), "n_lists"), (dict(n_lists=0), "n_lists"), (dict(stride=513), "list_stride"), (dict(stride=0), "list_stride"),
                    (dict(n_lists=16, stride=65), "entries per question"), (dict(n_lists=8, stride=129), "entries per question"),
                    (dict(top_n=1025), "top_n"), (dict(top_n=0), "top_n"), (dict(nq=-1), "nq"), (dict(min_semantic=-1), "min_semantic"),
                    (dict(keep=2), "bm25_keep_max"), (dict(rrf=-1), "RRF"), (dict(space=7), "space"), (dict(keys=None), "null"),
                    (dict(weight=p + 4), "misaligned"), (dict(filter_on=ctypes.c_void_p(p)), "filter_on")):
        assert rc(**kw) == _lib.RDX_ERR_INVALID and msg in _lib.last_error(), (kw, _lib.last_error())
    assert rc(nq=0) == _lib.RDX_OK                                     # nothing to do: nothing is touched
    assert bytes(buf) == bytes(1 << 16)                                 # and nothing was written
    assert (_lib.FUSE_MAX_LISTS, _lib.FUSE_MAX_LIST_ENTRIES, _lib.FUSE_MAX_ENTRIES) == (16, 512, 1024)
    header = open(os.path.join(os.path.dirname(HERE), "include", "rdx.h")).read()
    for name, val in (("RDX_FUSE_MAX_LISTS", 16), ("RDX_FUSE_MAX_LIST_ENTRIES", 512), ("RDX_FUSE_MAX_ENTRIES", 1024), ("RDX_FUSE_DENSE", 0), ("RDX_FUSE_BM25", 1)):
        assert f"#define {name} {val}\n" in header
