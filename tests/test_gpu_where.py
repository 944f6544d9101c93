"""GPU: the metadata store and the `where` predicate scan (meta_kernel.hpp) against the host evaluator — whole uint32 words of
W.pack_bits(W.evaluate(...) & alive), tail bits included — at the word / wave / block / grid-stride boundaries, the argument
checks of rdx_meta_*, and Collection's device path against a second collection kept on the host path through every write."""
import numpy as np
import pytest

from rag_dpo_amd import where as W
from rag_dpo_amd import where_device as WV

from test_where_device import BIG, STRS, make_columns, nested, stack_depth

pytestmark = pytest.mark.gpu

# word, wave (64 lanes x 4 rows = 256) and block (1024 rows) boundaries, several blocks
ROWS = [1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, 100_003]
GRID_ROWS = 256 * 8 * 1024 + 1024 + 77          # past one pass of a full grid (8 blocks of 1024 rows on each of 256 CUs)
STORE_KEYS = ["s", "i", "f", "b", "mix"]          # one column of each kind plus one of mixed kinds, a fifth of the rows missing

# every leaf op, NOT / AND / OR, stack depth 16, both kernels (at most 64 leaves: sorted by column; more: program order)
TREES = [
    {"s": "GUIDE"}, {"s": {"$ne": "not in any vocabulary"}}, {"i": {"$gt": 0}}, {"i": {"$gte": BIG}}, {"f": {"$lt": 0.5}},
    {"f": {"$lte": -0.0}}, {"b": True}, {"mix": {"$nin": [1, 2, 7]}}, {"f": float("nan")}, {"i": True}, {"absent": {"$ne": 1}},
    {"$and": [{"s": {"$in": ["GUIDE", "DOCTRINE", "SANCTION"]}}, {"$or": [{"i": {"$ne": 1}}, {"b": True}, {"mix": True}, {"absent": True}]}]},
    {"$or": [{"mix": "é’"}, {"$and": [{"i": {"$lt": 2}}, {"mix": {"$gte": -2.25}}, {"s": {"$nin": ["", "GUIDE"]}}]}, {"mix": {"$lte": 1}}]},
    nested(15, leaf=lambda i: [{"i": {"$ne": i % 3}}, {"b": i % 4 == 0}, {"mix": {"$gt": 0.5 - i}}, {"s": STRS[i % 5]}][i % 4]),
    {"mix": {"$in": list(range(-30, 34))}},                                                          # 64 leaves
    {"mix": {"$in": list(range(-30, 35))}},                                                          # 65
    {"$and": [{"$or": [{"i": {"$ne": j}}, {"mix": j}, {"f": {"$gt": j / 4}}, {"i": {"$lte": j}}]} for j in range(-9, 9)]},   # 72, interleaved
]


@pytest.fixture(scope="module")
def world():
    """the columns at the largest size, a tombstone bitmap, and the expected rows of every tree: computed once, never changed"""
    n = max(ROWS)
    small = make_columns(4097)
    cols = {}
    rng = np.random.default_rng(7)
    pick = rng.integers(0, 4097, size=n)
    pick[:4097] = np.arange(4097)
    for k in STORE_KEYS:                              # the large columns repeat the small ones' rows at random (same vocabulary)
        c = W.Column(0)
        c.kind, c.num, c.code = small[k].kind[pick].copy(), small[k].num[pick].copy(), small[k].code[pick].copy()
        c.vocab, c._lookup = list(small[k].vocab), dict(small[k]._lookup)
        cols[k] = c
    alive = rng.random(n) < 0.8
    want = [W.evaluate(t, cols, n) for t in TREES]
    compiled = [WV.compile_where(t, cols) for t in TREES]
    assert all(c is not None for c in compiled)
    assert max(stack_depth(c.program) for c in compiled) == 16
    assert sorted(c.leaves.shape[0] for c in compiled)[-3:] == [64, 65, 72]
    assert {int(o) for c in compiled for o in c.leaves["op"]} == set(range(7))
    return cols, alive, want, compiled


def load(cols, rows, split=True):
    from rag_dpo_amd.engine import MetaStore
    st = MetaStore(0)
    assert st.stats() == {"columns": 0, "bytes": 0}
    cut = rows // 2 if split else rows
    for slot, k in enumerate(STORE_KEYS):
        c = cols[k]
        if cut:
            st.set_rows(slot, 0, c.kind[:cut], c.num[:cut], c.code[:cut])
        st.set_rows(slot, cut, c.kind[cut:rows], c.num[cut:rows], c.code[cut:rows])     # the tail, as after an append
    assert st.stats()["columns"] == len(STORE_KEYS) and st.stats()["bytes"] >= 9 * rows * len(STORE_KEYS)
    return st


def slotted(c):
    lv = c.leaves.copy()
    named = lv["col"] >= 0
    lv["col"][named] = np.array([STORE_KEYS.index(k) for k in c.keys], dtype=np.int32)[lv["col"][named]]
    return lv


@pytest.mark.parametrize("rows", ROWS)
def test_filter_words_equal_the_host_evaluator(world, rows):
    import torch
    cols, alive, want, compiled = world
    st = load(cols, rows)
    base = W.pack_bits(alive[:rows])
    base_t = torch.from_numpy(base.view(np.int32)).cuda()
    side = torch.cuda.Stream()
    for tree, full, c in zip(TREES, want, compiled):
        st.set_query(slotted(c), c.program)
        plain, masked = W.pack_bits(full[:rows]), W.pack_bits(full[:rows] & alive[:rows])
        got = st.filter(rows)                                                  # RDX_HOST, base_bits NULL
        assert got.dtype == np.uint32 and got.shape == plain.shape and (got == plain).all(), tree
        assert (st.filter(rows, base) == masked).all(), tree                   # RDX_HOST with base_bits
        o = [torch.full((plain.shape[0],), -1, dtype=torch.int32, device="cuda") for _ in range(4)]
        st.filter_device(rows, o[0])                                           # RDX_DEVICE, NULL
        st.filter_device(rows, o[1], base_t)                                   # RDX_DEVICE with base_bits, twice,
        st.filter_device(rows, o[2], base_t)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                                          # and on a caller's stream
            st.filter_device(rows, o[3], base_t)
        torch.cuda.synchronize()
        assert (o[0].cpu().numpy().view(np.uint32) == plain).all(), tree
        for t in o[1:]:
            assert (t.cpu().numpy().view(np.uint32) == masked).all(), tree
    st.close()


def test_grid_stride(world):
    """more rows than one pass of the grid covers: the blocks come round again, and the last pass is a partial one"""
    import torch
    cols, alive, want, compiled = world
    n, reps = max(ROWS), -(-GRID_ROWS // max(ROWS))
    big = {}
    for k in STORE_KEYS:
        c = W.Column(0)
        c.kind, c.num, c.code = (np.tile(a[:n], reps)[:GRID_ROWS] for a in (cols[k].kind, cols[k].num, cols[k].code))
        big[k] = c
    st = load(big, GRID_ROWS)
    base = W.pack_bits(np.tile(alive, reps)[:GRID_ROWS])
    base_t = torch.from_numpy(base.view(np.int32)).cuda()
    for t in (11, 13, 16):                                  # the reference's shape, the 16-deep tree, 72 interleaved leaves
        c = compiled[t]
        st.set_query(slotted(c), c.program)
        full = W.pack_bits(np.tile(want[t], reps)[:GRID_ROWS])
        out = torch.full((full.shape[0],), -1, dtype=torch.int32, device="cuda")
        st.filter_device(GRID_ROWS, out, base_t)
        torch.cuda.synchronize()
        assert (out.cpu().numpy().view(np.uint32) == (full & base)).all(), TREES[t]
        assert (st.filter(GRID_ROWS) == full).all(), TREES[t]
    st.close()


def test_store_rewrite_gap_truncate_and_drop(world):
    cols, alive, want, compiled = world
    rows = 1000
    st = load(cols, rows, split=False)
    t = TREES.index({"mix": {"$nin": [1, 2, 7]}})
    c = compiled[t]
    # rows 100..199 of "mix" rewritten in place with other kinds
    mix = W.Column(0)
    mix.kind, mix.num, mix.code = (a[:rows].copy() for a in (cols["mix"].kind, cols["mix"].num, cols["mix"].code))
    mix.vocab, mix._lookup = cols["mix"].vocab, cols["mix"]._lookup
    for r in range(100, 200):
        mix.set(r, [1, 2.0, True, "GUIDE", None, 7][r % 6])
    st.set_rows(4, 100, mix.kind[100:200], mix.num[100:200], mix.code[100:200])
    with pytest.raises(Exception, match="no query set"):          # a change of the store unsets the query
        st.filter(rows)
    st.set_query(slotted(c), c.program)
    assert (st.filter(rows) == W.pack_bits(W.evaluate(TREES[t], {"mix": mix}, rows))).all()
    # a write past the end: the gap is "missing"
    st.set_rows(4, rows + 50, mix.kind[:10], mix.num[:10], mix.code[:10])
    mix.resize(rows + 60)
    mix.kind[rows: rows + 50] = W.K_MISSING
    mix.kind[rows + 50: rows + 60], mix.num[rows + 50: rows + 60], mix.code[rows + 50: rows + 60] = mix.kind[:10], mix.num[:10], mix.code[:10]
    st.set_query(slotted(c), c.program)
    assert (st.filter(rows + 60) == W.pack_bits(W.evaluate(TREES[t], {"mix": mix}, rows + 60))).all()
    st.truncate(rows)
    st.set_query(slotted(c), c.program)
    assert (st.filter(rows) == W.pack_bits(W.evaluate(TREES[t], {"mix": mix}, rows))).all()
    before = st.stats()
    st.drop_column(4)
    after = st.stats()
    assert after["columns"] == before["columns"] - 1 and after["bytes"] < before["bytes"]
    with pytest.raises(ValueError, match="holds no rows"):
        st.set_query(slotted(c), c.program)
    st.close()


def test_bad_arguments_are_refused_before_anything_is_launched(world):
    from rag_dpo_amd import _lib as L
    from rag_dpo_amd._lib import RdxError
    cols, alive, want, compiled = world
    rows = 300
    st = load(cols, rows, split=False)
    with pytest.raises(RdxError, match="error 4.*no query set"):                 # RDX_ERR_STATE: no query yet
        st.filter(rows)
    N, A, O = WV.OP_NOT, WV.OP_AND, WV.OP_OR
    lv = np.zeros(17, dtype=WV.LEAF)
    lv["col"], lv["op"], lv["kind"], lv["num"] = 1, WV.EQ, W.K_INT, 1.0

    def refused(leaves, prog, match):
        with pytest.raises(ValueError, match=match):
            st.set_query(leaves, prog)

    refused(lv, [0, A], "pops an empty stack")                                   # stack underflow
    refused(lv, [N], "pops an empty stack")
    refused(lv, [0, 1], "exactly one value")                                     # two entries left
    refused(lv, list(range(17)) + [O] * 16, "more than 16 stack entries")        # 17 entries
    st.set_query(lv, list(range(16)) + [O] * 15)                                 # 16 are fine
    refused(lv, [0, N] * 2049, "n_ops")                                          # n_ops = 4098 > 4096
    refused(lv, [17], "neither a leaf")
    refused(lv, [-4], "neither a leaf")
    refused(lv[:0], [0], "n_leaves")
    refused(np.zeros(1025, dtype=WV.LEAF), [0], "n_leaves")
    empty = lv.copy()
    empty["col"][3] = 9
    refused(empty, [3], "holds no rows")                                         # a leaf on an empty slot
    for field, value, match in (("op", 7, "unknown op"), ("kind", 0, "kind"), ("kind", 5, "kind"), ("col", -1, "out of range"),
                                ("col", L.META_MAX_COLUMNS, "out of range")):
        bad = lv.copy()
        bad[field][0] = value
        refused(bad, [0], match)
    strs = lv.copy()
    strs["kind"][0], strs["op"][0] = W.K_STR, WV.GT
    refused(strs, [0], "EQ only")
    with pytest.raises(ValueError, match="not one of 0 .. 4"):
        st.set_rows(0, 0, np.array([5], dtype=np.uint8), np.zeros(1), np.zeros(1, dtype=np.int32))
    with pytest.raises(ValueError, match="out of range"):
        st.set_rows(L.META_MAX_COLUMNS, 0, np.zeros(1, dtype=np.uint8), np.zeros(1), np.zeros(1, dtype=np.int32))
    # a refused query leaves the one before it in place (16 leaves ORed), and a refused call launches and writes nothing
    assert (st.filter(rows) == W.pack_bits(W.evaluate({"i": 1}, cols, rows))).all()
    import torch
    out = torch.full(((rows + 31) // 32 + 1,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    with pytest.raises(RdxError, match="error 4.*holds 300 rows"):               # a rows mismatch
        st.filter_device(rows + 32, out)
    with pytest.raises(RdxError, match="error 4.*holds 300 rows"):
        st.filter(rows - 1)
    torch.cuda.synchronize()
    assert (out == 0x5A5A5A5A).all()
    const = np.zeros(1, dtype=WV.LEAF)                                           # a CONST leaf reads no column: any row count
    const["op"], const["col"] = WV.CONST1, -1
    st.set_query(const, [0])
    assert (st.filter(70) == W.pack_bits(np.ones(70, dtype=bool))).all()
    assert st.filter(0).shape == (0,)
    st.close()


# ---- Collection: the device path against a second collection kept on the host path ------------------------------------------
NAT = ["GUIDE", "DOCTRINE", "SANCTION", "TECHNIQUE"]
FILTERS = [
    {"chunk_nature": "GUIDE"},
    {"chunk_nature": {"$in": ["GUIDE", "DOCTRINE", "TECHNIQUE"]}},                                     # pages/1_Chat.py
    {"tag_rh": True},
    {"source": {"$ne": "ENTREPRISE"}},
    {"$and": [{"chunk_nature": {"$in": ["GUIDE", "DOCTRINE", "SANCTION"]}},                            # build_enterprise_where_filter
              {"$or": [{"source": {"$ne": "ENTREPRISE"}}, {"tag_rh": True}, {"tag_securite": True}, {"tag_cookies": True}]}]},
    {"chunk_index": {"$gte": 100}}, {"$and": [{"chunk_index": {"$gt": 10}}, {"chunk_index": {"$lt": 2500}}, {"confidence": {"$lte": 0.7}}]},
    {"chunk_index": {"$nin": list(range(0, 3000, 3))}},                                                # 1000 leaves: the unsorted kernel
    {"chunk_index": True}, {"is_priority": 1}, {"confidence": 1}, {"odd": 1}, {"odd": 1.0}, {"odd": True}, {"odd": "1"},
    {"confidence": float("nan")}, {"confidence": {"$ne": float("nan")}}, {"odd": -0.0}, {"odd": {"$gte": -0.0}},
    {"big": BIG}, {"big": {"$lt": BIG}}, {"big": {"$gt": -BIG}},
    {"source": "a string no row holds"}, {"source": {"$nin": ["a string no row holds"]}},
    {"never_a_key": 1}, {"never_a_key": {"$ne": 1}}, {"$or": [{"never_a_key": {"$nin": [1]}}, {"tag_rh": True}]},
    {"added_later": "fresh value"}, {"added_later": {"$ne": "fresh value"}}, {"source": "NEW SOURCE"},
    nested(15, leaf=lambda i: [{"chunk_index": {"$ne": i}}, {"is_priority": i % 4 == 0}, {"confidence": {"$gt": 0.6}}][i % 3]),
]


def meta_of(i):
    m = {"document_path": f"p{i % 20}", "chunk_nature": NAT[i % 4], "chunk_index": i, "source": "ENTREPRISE" if i % 10 == 0 else "CNIL",
         "confidence": 0.5 + (i % 5) / 10, "is_priority": i % 3 == 0, "odd": [1, 1.0, True, "1", 0.0, -0.0][i % 6],
         "big": [BIG, -BIG, 0][i % 3]}
    for j, tag in enumerate(("tag_rh", "tag_securite", "tag_cookies")):
        if i % (7 + 2 * j) == 0:
            m[tag] = True
    if i % 11 == 0:
        del m["confidence"]
    return m


class Pair:
    """the same writes to a collection on the device path and to one forced onto the host evaluator"""

    def __init__(self, dev, host):
        self.dev, self.host = dev, host
        dev._WHERE_DEVICE_MIN_ROWS = 0
        host._WHERE_DEVICE_MIN_ROWS = 1 << 62

    def __getattr__(self, name):
        def both(*a, **kw):
            getattr(self.host, name)(*a, **kw)
            return getattr(self.dev, name)(*a, **kw)
        return both

    def check(self, q, named_before=None):
        from rag_dpo_amd.engine import ResidentMask
        for f in FILTERS:
            a = self.dev.query(query_embeddings=q, n_results=50, where=f, include=["distances"])
            b = self.host.query(query_embeddings=q, n_results=50, where=f, include=["distances"])
            assert a["ids"] == b["ids"] and a["distances"] == b["distances"], f
        assert self.host._meta_store is None and self.dev._meta_store is not None
        assert all(isinstance(r, ResidentMask) for _, r in self.dev._mask_cache.values())
        named = {k for f in FILTERS for k in WV.compile_where(f, self.dev._cols).keys}
        assert set(self.dev._meta_res) == named and self.dev._meta_store.stats()["columns"] == len(named)
        assert all(r == self.dev._rows for _, r in self.dev._meta_res.values())
        return named


def test_collection_device_path_follows_every_write(tmp_path):
    from rag_dpo_amd import synth
    from rag_dpo_amd.collection import PersistentClient
    n = 3000
    emb = synth.make_corpus(n + 600, 64)
    q = synth.make_queries(3, 64, emb)
    clients = PersistentClient(str(tmp_path / "dev")), PersistentClient(str(tmp_path / "host"))
    p = Pair(*(c.create_collection("rag_dpo_chunks") for c in clients))
    ids = [f"c{i}" for i in range(n)]
    for a in range(0, n, 1000):
        p.add(ids=ids[a: a + 1000], embeddings=emb[a: a + 1000], metadatas=[meta_of(i) for i in range(a, a + 1000)])
    p.dev.query(query_embeddings=q, n_results=5)
    p.dev.get(where={"chunk_nature": "GUIDE"}, limit=3)                      # get keeps the host evaluator
    assert p.dev._meta_store is None                                       # nothing before the first query(where=)
    p.dev.query(query_embeddings=q, n_results=5, where={"tag_rh": True})
    assert p.dev._meta_store.stats()["columns"] == 1 and list(p.dev._meta_res) == ["tag_rh"]   # only the named column
    named = p.check(q)
    assert "document_path" not in named and "never_a_key" not in named

    def new_meta(i):
        m = meta_of(i)
        if i % 2:
            m["added_later"] = "fresh value" if i % 4 == 1 else 7          # a new key, first seen mid-batch
        if i % 50 == 0:
            m["source"] = "NEW SOURCE"                                     # a new string in a resident column
        return m

    p.add(ids=[f"c{i}" for i in range(n, n + 500)], embeddings=emb[n: n + 500], metadatas=[new_meta(i) for i in range(n, n + 500)])
    assert all(r == n for _, r in p.dev._meta_res.values())                # resident columns wait for the next filter: the tail only
    assert "added_later" in p.check(q)
    # update of 50 rows' metadata, changing kinds
    upd = [f"c{i}" for i in range(40, 3040, 60)]
    p.update(ids=upd, metadatas=[{"chunk_index": str(j), "confidence": j, "is_priority": 0.5, "chunk_nature": j % 2 == 0, "tag_rh": "yes"}
                                 for j in range(len(upd))])
    assert p.dev._meta_res["chunk_index"][1] == 40 and p.dev._meta_res["source"][1] == n + 500
    p.check(q)
    p.upsert(ids=["c7", "c8", "u0", "u1"], embeddings=emb[n + 500: n + 504],
             metadatas=[{"chunk_nature": "GUIDE", "odd": 1}, {"source": "NEW SOURCE"}, meta_of(1), {"chunk_index": 5, "tag_cookies": True}])
    p.check(q)
    p.delete(ids=[f"c{i}" for i in range(0, 1200, 3)])                     # 400 rows: tombstones, below the compaction threshold
    assert p.dev._n_dead == 400 and p.dev._meta_store is not None
    p.check(q)
    p.delete(where={"chunk_index": {"$gte": 2500}})                        # over a fifth of the rows dead: compaction
    assert p.dev._n_dead == 0 and p.dev._meta_store is None and not p.dev._meta_res
    p.check(q)
    for c in clients:
        c.persist()
    again = PersistentClient(str(tmp_path / "dev")), PersistentClient(str(tmp_path / "host"))
    p2 = Pair(*(c.get_collection("rag_dpo_chunks") for c in again))
    assert p2.dev._meta_store is None and p2.dev.count() == p.dev.count()
    p2.check(q)
    for f in FILTERS[:6]:                                                  # and the reloaded store answers as the first one does
        assert p2.dev.query(query_embeddings=q, n_results=50, where=f)["ids"] == p.dev.query(query_embeddings=q, n_results=50, where=f)["ids"]


def test_where_and_where_document_together():
    from rag_dpo_amd import synth
    from rag_dpo_amd.collection import Collection
    from rag_dpo_amd.engine import ResidentMask
    n = 3000
    emb = synth.make_corpus(n, 64)
    q = synth.make_queries(2, 64, emb)
    p = Pair(Collection("dev"), Collection("host"))
    p.add(ids=[f"c{i}" for i in range(n)], embeddings=emb, metadatas=[meta_of(i) for i in range(n)],
          documents=[f"chunk {i} about {'cookies' if i % 3 == 0 else 'registre'} and {NAT[i % 4].lower()}" for i in range(n)])
    p.delete(ids=[f"c{i}" for i in range(0, 300, 2)])
    docs = [{"$contains": "cookies"}, {"$and": [{"$not_contains": "guide"}, {"$contains": " 1"}]}]
    for wd in docs:
        for f in FILTERS[:8] + FILTERS[-1:]:
            a = p.dev.query(query_embeddings=q, n_results=50, where=f, where_document=wd, include=["distances"])
            b = p.host.query(query_embeddings=q, n_results=50, where=f, where_document=wd, include=["distances"])
            assert a["ids"] == b["ids"] and a["distances"] == b["distances"], (f, wd)
    assert p.dev._meta_store is not None and p.host._meta_store is None
    assert len(p.dev._mask_cache) >= 9 and all(k.startswith("wd:") for k in p.dev._mask_cache)
    assert all(bits is None and isinstance(r, ResidentMask) for bits, r in p.dev._mask_cache.values())
    # query_device takes the same path
    import torch
    d, rr, cc = p.dev.query_device(torch.from_numpy(q).cuda(), 50, where=FILTERS[4], where_document=docs[0])
    torch.cuda.synchronize()
    assert p.dev.ids_of(rr.cpu()) == p.host.query(query_embeddings=q, n_results=50, where=FILTERS[4], where_document=docs[0])["ids"]
