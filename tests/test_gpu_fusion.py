"""GPU: rdx_fuse_rankings (csrc/fuse_kernel.hpp through include/rdx.h) against DenseRetriever._fuse itself (tests/fusion_model.py), bit
for bit: order, count, the fp32 distance, the fp64 semantic / BM25 / hybrid scores and the first-appearance positions — at the
smallest list sets at which each rule of the contract can go wrong, at the kernel's limits, and across question
counts; then DenseRetriever.retrieve_candidates_batch(fusion="device") against the per-question retrieve_candidates."""
import ctypes
import json

import numpy as np
import pytest

import bm25_replay as R
import fusion_model as M
from bm25_replay import W
from rag_dpo_amd import _lib as L
from rag_dpo_amd import fusion as F
from rag_dpo_amd.retriever import DenseRetriever

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib_():
    return L.load(require_gpu=True)


def fuse_device(lib, packed, min_semantic, keep_max, top_n, out_fill=0):
    """the kernel on device pointers (RDX_DEVICE), on torch's current stream -> (winners, the raw output buffer)"""
    import torch
    dev = torch.device("cuda", 0)
    t = {name: torch.from_numpy(getattr(packed, name)).to(dev) for name in ("kind", "weight", "count", "keys", "dist", "score", "filter_on", "allow")}
    rg = torch.from_numpy(M.ROW_GROUP).to(dev)
    p = {name: t[name].data_ptr() for name in ("kind", "weight", "count", "keys", "dist", "score")}
    if packed.filter_on.any():
        p.update(filter_on=t["filter_on"].data_ptr(), allow=t["allow"].data_ptr(), row_group=rg.data_ptr())
    _, nbytes = F._out_layout(packed.nq, top_n)
    out = torch.full((max(nbytes, 8),), out_fill, dtype=torch.uint8, device=dev)
    F.call_kernel(lib, 0, packed.nq, packed.n_lists, packed.list_stride, p, M.N_ROWS, packed.group_words, min_semantic, keep_max, top_n,
                  out.data_ptr(), L.RDX_DEVICE, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    raw = out.cpu().numpy()
    return F.unpack(raw, packed.nq, top_n), raw


def check(lib, questions, n_lists, stride, filters=None, min_semantic=10, keep_max=True, top_n=100):
    packed = M.pack(questions, n_lists, stride, filters)
    winners, raw = fuse_device(lib, packed, min_semantic, keep_max, top_n)
    for q, lists in enumerate(questions):
        lists = list(lists) + [None] * (n_lists - len(lists))
        model, distinct = M.run_model(lists, None if filters is None else filters[q], min_semantic, keep_max, top_n)
        M.same_as_model(winners[q], model, distinct, top_n)
    lay, _ = F._out_layout(len(questions), top_n)                      # slots past the count: key -1
    keys = np.frombuffer(raw, np.int64, len(questions) * top_n, lay["key"][0]).reshape(len(questions), top_n)
    for q, ws in enumerate(winners):
        assert (keys[q, len(ws):] == -1).all()
    return winners


CASES = M.named_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_contract_case(lib_, name):
    c = CASES[name]
    n_lists = len(c["lists"])
    stride = max([len(e[2]) for e in c["lists"] if e is not None] + [1])
    filters = None if c["allowed"] is None else [c["allowed"]]
    for pad_lists, pad_stride in ((0, 0), (2, 3)):                     # the same question in a roomier layout: absent lists, unused slots
        check(lib_, [c["lists"]], n_lists + pad_lists, stride + pad_stride, filters, c["min_semantic"], c["keep_max"], c["top_n"])


def test_entry_counts_and_the_maximum(lib_):
    rng = np.random.default_rng(21)
    for name, (lists, stride) in M.sized_cases(rng).items():
        for filt in (None, sorted(rng.choice(M.N_GROUPS, 9, replace=False).tolist())):
            for top_n in (1024, 40):
                check(lib_, [lists], len(lists), stride, None if filt is None else [filt], 10, True, top_n)


def test_question_counts(lib_):
    """nq = 1, 3 and more questions than the chip holds workgroups of 1024 threads at once (256 CUs x 2); a question's result does not
    depend on its neighbours or on nq"""
    rng = np.random.default_rng(22)
    questions = [M.random_question(rng, 3, 12) for _ in range(1100)]
    filters = [M.random_filter(rng) for _ in questions]
    big = check(lib_, questions, 6, 12, filters, 4, True, 20)
    assert check(lib_, questions[:1], 6, 12, filters[:1], 4, True, 20) == big[:1]
    assert check(lib_, questions[5:8], 6, 12, filters[5:8], 4, True, 20) == big[5:8]
    again = check(lib_, questions[::-1], 6, 12, filters[::-1], 4, True, 20)
    assert again[::-1] == big
    check(lib_, questions[:64], 6, 12, filters[:64], 0, False, 7)


def test_host_space_gives_the_same_bits(lib_):
    rng = np.random.default_rng(23)
    questions = [M.random_question(rng, 2, 30) for _ in range(5)]
    filters = [M.random_filter(rng) for _ in questions]
    packed = M.pack(questions, 4, 30, filters)
    dev, _ = fuse_device(lib_, packed, 6, True, 25)
    assert F.fuse_host(packed, M.ROW_GROUP, 6, True, 25) == dev
    packed.count[2, 1] = 31                                            # RDX_HOST reads the counts: beyond list_stride is refused
    with pytest.raises(ValueError, match="count"):
        F.fuse_host(packed, M.ROW_GROUP, 6, True, 25)


def test_limits_are_refused_and_nothing_is_written(lib_):
    import torch
    rng = np.random.default_rng(24)
    packed = M.pack([M.random_question(rng, 2, 8)], 4, 8, [None])
    good, _ = fuse_device(lib_, packed, 10, True, 8)
    dev = torch.device("cuda", 0)
    room = torch.zeros(1 << 20, dtype=torch.uint8, device=dev)        # inputs large enough for every refused shape
    out = torch.full((1 << 20,), 0xAB, dtype=torch.uint8, device=dev)
    p = {name: room.data_ptr() for name in ("kind", "weight", "count", "keys", "dist", "score")}
    st = torch.cuda.current_stream(dev).cuda_stream
    for n_lists, stride, top_n, msg in ((17, 8, 8, "n_lists"), (0, 8, 8, "n_lists"), (2, 513, 8, "list_stride"), (2, 0, 8, "list_stride"),
                                        (16, 65, 8, "entries per question"), (9, 128, 8, "entries per question"),
                                        (4, 8, 1025, "top_n"), (4, 8, 0, "top_n")):
        with pytest.raises(ValueError, match=msg):
            F.call_kernel(lib_, 0, 1, n_lists, stride, p, M.N_ROWS, 1, 10, True, top_n, out.data_ptr(), L.RDX_DEVICE, st)
    with pytest.raises(ValueError, match="nq"):
        F.call_kernel(lib_, 0, -1, 4, 8, p, M.N_ROWS, 1, 10, True, 8, out.data_ptr(), L.RDX_DEVICE, st)
    with pytest.raises(ValueError, match="space"):
        F.call_kernel(lib_, 0, 1, 4, 8, p, M.N_ROWS, 1, 10, True, 8, out.data_ptr(), 2, st)
    with pytest.raises(ValueError, match="min_semantic"):
        F.call_kernel(lib_, 0, 1, 4, 8, p, M.N_ROWS, 1, -1, True, 8, out.data_ptr(), L.RDX_DEVICE, st)
    with pytest.raises(ValueError, match="null"):
        F.call_kernel(lib_, 0, 1, 4, 8, dict(p, keys=0), M.N_ROWS, 1, 10, True, 8, out.data_ptr(), L.RDX_DEVICE, st)
    with pytest.raises(ValueError, match="misaligned"):
        F.call_kernel(lib_, 0, 1, 4, 8, dict(p, weight=room.data_ptr() + 4), M.N_ROWS, 1, 10, True, 8, out.data_ptr(), L.RDX_DEVICE, st)
    with pytest.raises(ValueError, match="filter_on"):
        F.call_kernel(lib_, 0, 1, 4, 8, dict(p, filter_on=room.data_ptr()), M.N_ROWS, 1, 10, True, 8, out.data_ptr(), L.RDX_DEVICE, st)
    torch.cuda.synchronize()
    assert bool((out == 0xAB).all())                                  # nothing was launched with the bad arguments
    assert fuse_device(lib_, packed, 10, True, 8)[0] == good
    # the widest shapes inside the limits are accepted
    for n_lists, stride in ((16, 64), (8, 128), (2, 512)):
        F.call_kernel(lib_, 0, 1, n_lists, stride, p, M.N_ROWS, 1, 10, True, 1024, out.data_ptr(), L.RDX_DEVICE, st)
    torch.cuda.synchronize()


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
class DeviceHashEmbedder(W.HashEmbedder):
    """EmbeddingProvider's contract on the hash embedder: embed_device = the raw rows on the GPU, embed = those rows through
    rdx_l2_normalize, as lists"""

    def raw(self, texts):
        import zlib
        out = []
        for t in texts:
            h = zlib.crc32(t.encode("utf-8"))
            out.append(3.0 * (self.c[h % W.N] + 0.8 * np.random.default_rng(h).standard_normal(W.DIM).astype(np.float32)))
        return np.asarray(out, dtype=np.float32)

    def embed_device(self, texts):
        import torch
        return torch.from_numpy(self.raw(texts)).to("cuda:0")

    def embed(self, texts):
        import torch
        self.calls.append(list(texts))
        raw = self.embed_device(texts)
        out = torch.empty_like(raw)
        L.check(L.load().rdx_l2_normalize(0, ctypes.c_void_p(raw.data_ptr()), raw.shape[0], raw.shape[1], ctypes.c_void_p(out.data_ptr()),
                                          L.RDX_DEVICE, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return out.cpu().numpy().tolist()


def chunk_values(c):
    return (c.chunk_id, c.text, c.document_path, c.chunk_nature, c.chunk_index, c.confidence, np.float32(c.distance).tobytes(),
            np.float64(c.bm25_score).tobytes(), np.float64(c.semantic_score).tobytes(), np.float64(c.hybrid_score).tobytes(),
            json.dumps(c.metadata, sort_keys=True))


def test_retrieve_candidates_batch_on_the_device(tmp_path):
    col = W.build_collection(None)                                     # librdx on cuda:0: 3000 rows, 150 document paths and the "" group
    chunk = R.chunk_index(None)
    summ = R.summary_index(None, str(tmp_path))
    queries = [W.Q0, "registre des traitements du sous-traitant article 28", "notification d'une violation en 72 heures",
               "biométrie badge salariés", "zzzinconnu qqqabsent"]
    wheres = [None, {"chunk_nature": {"$in": ["GUIDE", "DOCTRINE"]}}, None, None, None]
    r = DenseRetriever(col, DeviceHashEmbedder(), query_expander=W.expander, summary_bm25_index=summ, chunk_bm25_index=chunk, fusion="device")
    filters = [r._doc_filter(r._expand(q)[0]) for q in queries]
    assert sum(1 for f in filters if f) >= 2 and len({frozenset(f) for f in filters if f}) >= 2     # the summary filter separates groups
    calls = []
    real = F.call_kernel

    def spy(*a, **kw):
        calls.append(a[2])
        return real(*a, **kw)
    F.call_kernel = spy
    try:
        for step in ("built", "after a delete"):
            calls.clear()
            got = r.retrieve_candidates_batch(queries, n_candidates=40, where_filter=wheres)
            assert calls == [5]                                        # one launch for the five questions: no fall-back
            loop = [r.retrieve_candidates(q, n_candidates=40, where_filter=w) for q, w in zip(queries, wheres)]
            assert [len(g) for g in got] == [len(g) for g in loop] and all(len(g) > 0 for g in got[:4])
            for g, l in zip(got, loop):
                assert [chunk_values(c) for c in g] == [chunk_values(c) for c in l], step
            if step == "built":
                # delete chunks the BM25 index still holds: one that only BM25 finds stays a candidate, under a key of its own
                sparse_only = [c.chunk_id for c in got[0] if c.semantic_score == 0.0][:2]
                assert sparse_only
                col.delete(ids=sparse_only + [got[0][0].chunk_id])
    finally:
        F.call_kernel = real
    assert any(c.chunk_id in sparse_only for c in got[0])
    host = DenseRetriever(col, DeviceHashEmbedder(), query_expander=W.expander, summary_bm25_index=summ, chunk_bm25_index=chunk, fusion="host")
    assert [[chunk_values(c) for c in g] for g in host.retrieve_candidates_batch(queries, 40, wheres)] == [[chunk_values(c) for c in g] for g in got]
