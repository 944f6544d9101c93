"""GPU: where_document's document store and substring scan (doc_kernel.hpp) against `needle in document`, the boolean program
with a base bitmap, and the Collection contract of test_where_document.py on HipIndex (and a two-shard rehearsal on one GPU)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ALPHA = np.frombuffer("ab \x00é’".encode("utf-8"), dtype=np.uint8)   # few symbols: patterns recur; multi-byte UTF-8 and NUL


def rand_bytes(rng, n):
    return ALPHA[rng.integers(0, ALPHA.shape[0], size=n)].tobytes()


def unpack(words, n):
    return np.unpackbits(np.ascontiguousarray(words, dtype=np.uint32).view(np.uint8), bitorder="little")[:n].astype(bool)


STAGE_MAX = 256   # doc_kernel.hpp DOC_STAGE_MAX: longer patterns take the long-pattern kernel
PASS = 32         # doc_kernel.hpp DOC_LEAVES_PER_PASS


def fuzz_case(seed):
    """documents of edge lengths with patterns planted at row start / end, across 16-B and segment (1024 B) boundaries ->
    (docs, pools): "planted" and "substr" (cut out of the rows: they occur), "span" (the end of a row whose length is a multiple
    of 16, so that no padding separates it from the next row in the arena, followed by the start of that next row: `pat in d`
    is the truth, and a scan that ran across row ends would find them), "long" (over STAGE_MAX bytes)"""
    rng = np.random.default_rng(seed)
    lens = [0, 1, 15, 16, 17, 1023, 1024, 1025, 2047, 2048, 2049, 3071, 200_000, 0, 5, 33, 1000, 1100, 6000, 7000]
    lens += [int(x) for x in rng.integers(0, 3000, size=60)]
    lens += [16 * int(x) for x in rng.integers(1, 190, size=50)] + [int(x) for x in rng.integers(1, 3000, size=30)]
    order = rng.permutation(len(lens) - 20) + 20          # edge lengths stay first; the others interleave
    lens = lens[:20] + [lens[i] for i in order]
    docs = [bytearray(rand_bytes(rng, n)) for n in lens]
    pools = {"planted": [], "substr": [], "span": [], "long": []}
    plens = [1, 2, 3, 4, 5, 15, 16, 17, 31, 64, 100, 255, 256, 257, 300, 5200]
    for pl in plens:
        p = rand_bytes(rng, pl)
        pools["planted" if pl <= STAGE_MAX else "long"].append(p)
        for _ in range(3):
            cands = [i for i, d in enumerate(docs) if len(d) >= pl]
            i = cands[int(rng.integers(0, len(cands)))]
            L = len(docs[i])
            spots = [0, L - pl] + [b - int(rng.integers(1, pl + 1)) for b in (16, 32, 1024, 2048, 3072) if b < L] + \
                    [int(rng.integers(0, L - pl + 1))]
            s = max(0, min(L - pl, spots[int(rng.integers(0, len(spots)))]))
            docs[i][s: s + pl] = p
    docs = [bytes(d) for d in docs]
    for _ in range(40):
        i = int(rng.choice([i for i, d in enumerate(docs) if len(d) >= 8]))
        pl = int(rng.integers(1, min(STAGE_MAX, len(docs[i])) + 1))
        s = int(rng.integers(0, len(docs[i]) - pl + 1))
        pools["substr"].append(docs[i][s: s + pl])
    for i in range(len(docs) - 1):
        a, b = docs[i], docs[i + 1]
        if a and b and len(a) % 16 == 0:
            pools["span"].append(a[-min(len(a), int(rng.integers(1, 40))):] + b[: min(len(b), int(rng.integers(1, 40)))])
    pools["planted"] += ["’é".encode("utf-8"), b"\x00\x00"]
    return docs, pools


def choose(rng, pools, P, trial):
    """P patterns of <= STAGE_MAX bytes (trial 1: the row-spanning ones first), at least one that occurs (unless P = 1 and
    trial 1), and the long patterns on top in trial 0"""
    short = pools["planted"] + pools["substr"] + pools["span"]
    first = pools["span"][:P] if trial == 1 else []
    rest = [p for p in short if p not in first]
    chosen = first + [rest[int(i)] for i in rng.choice(len(rest), size=P - len(first), replace=False)]
    if not (P == 1 and trial == 1) and not any(p in pools["substr"] for p in chosen):
        chosen[-1] = pools["substr"][int(rng.integers(0, len(pools["substr"])))]
    if trial == 0:
        chosen += pools["long"]
    return chosen


def check_leaves(st, docs, chosen):
    st.set_query(chosen)
    got = st.contains()
    assert got.shape == (len(chosen), (len(docs) + 31) // 32)
    for p, pat in enumerate(chosen):
        want = np.array([pat in d for d in docs])
        assert (unpack(got[p], len(docs)) == want).all(), (p, len(pat))
        assert (unpack(got[p], got.shape[1] * 32)[len(docs):] == 0).all()
    return got


@pytest.mark.parametrize("P", [1, 7, 32, 33])
def test_leaf_bitmaps_equal_needle_in_doc(P):
    """P short leaves: one pass (P <= 32, at capacity for 32) or two (33), plus the long-pattern kernel in trial 0"""
    from rag_dpo_amd.engine import DocStore
    docs, pools = fuzz_case(P)
    assert len(pools["span"]) >= 33 and len(pools["long"]) == 3
    rng = np.random.default_rng(100 + P)
    st = DocStore(0)
    st.append(docs[:50])
    st.append(docs[50:])
    assert len(st) == len(docs)
    hits = spans_checked = 0
    for trial in range(4):
        chosen = choose(rng, pools, P, trial)
        assert sum(len(p) <= STAGE_MAX for p in chosen) == P                     # the short leaves the passes take
        assert len(chosen) == P + (3 if trial == 0 else 0)
        got = check_leaves(st, docs, chosen)
        hits += int(np.unpackbits(got.view(np.uint8)).sum())
        spans_checked += sum(p in pools["span"] for p in chosen)
        assert (st.contains() == got).all()                                     # a second call: the same bits
    assert hits > 0 and spans_checked >= min(P, 33)
    # rows appended after the store has been scanned (the row table and work list grow in place)
    more, _ = fuzz_case(1000 + P)
    st.append(more[:40])
    docs = docs + more[:40]
    check_leaves(st, docs, choose(rng, pools, P, 2))
    st.close()


def test_store_replace_and_compact():
    from rag_dpo_amd.engine import DocStore
    docs, pools = fuzz_case(9)
    st = DocStore(0)
    st.append(docs)
    rng = np.random.default_rng(3)
    old = pools["substr"][:10]
    rows = rng.choice(len(docs), size=25, replace=False)
    for r in rows:
        docs[r] = rand_bytes(rng, int(rng.integers(0, 4000)))
    st.replace(rows, [docs[r] for r in rows])
    s = st.stats()
    assert s["rows"] == len(docs) and s["arena_bytes"] >= s["live_bytes"]
    check_leaves(st, docs, old + pools["span"][:10] + pools["planted"][:10])
    keep = np.flatnonzero(rng.random(len(docs)) < 0.6)
    st.compact(keep)
    docs = [docs[i] for i in keep]
    s = st.stats()
    assert s["rows"] == len(docs) and s["arena_bytes"] == s["live_bytes"] == sum((len(d) + 15) // 16 * 16 for d in docs)
    check_leaves(st, docs, old + pools["span"][:10] + pools["planted"][:10])
    st.append(docs[:5])                              # append after a compaction
    docs = docs + docs[:5]
    check_leaves(st, docs, old + pools["span"][:5])
    st.close()


def test_store_replace_rewrites_the_arena():
    """replace keeps writing at the tail; once dead bytes exceed both the live bytes and 16 MiB the arena is rewritten densely"""
    from rag_dpo_amd.engine import DocStore
    rng = np.random.default_rng(11)
    docs = [rand_bytes(rng, int(rng.integers(0, 3000))) for _ in range(40)]
    st = DocStore(0)
    st.append(docs)
    replaced = []
    rewrites, prev = 0, st.stats()["arena_bytes"]
    for step in range(24):
        r = step % 4
        replaced.append(docs[r])
        docs[r] = rand_bytes(rng, (3 << 19) + int(rng.integers(0, 4096)))     # ~1.5 MiB each
        st.replace([r], [docs[r]])
        s = st.stats()
        assert s["rows"] == 40 and s["live_bytes"] == sum((len(d) + 15) // 16 * 16 for d in docs)
        assert s["arena_bytes"] - s["live_bytes"] <= max(s["live_bytes"], 16 << 20)
        rewrites += s["arena_bytes"] < prev
        prev = s["arena_bytes"]
    assert rewrites >= 1
    pats = [d[1000:1040] for d in docs[:4]] + [d[5000:5030] for d in replaced[4:10]] + [d[:20] for d in docs[4:12] if len(d) >= 20]
    check_leaves(st, docs, pats)
    st.close()


def test_depth3_tree_with_base_bits():
    import torch
    from rag_dpo_amd import where_document as WD
    from rag_dpo_amd.where import pack_bits
    from rag_dpo_amd.engine import DocStore
    from test_where_document import TREES, bf_match, make_docs
    docs = make_docs(1000, seed=4)          # 1000 rows: the last word has 8 rows, 24 tail bits
    st = DocStore(0)
    st.append(docs)
    base = np.random.default_rng(5).random(1000) < 0.7
    for tree in TREES:
        leaves, prog = WD.compile_tree(tree)
        st.set_query(leaves, prog)
        want = np.array([bf_match(tree, d) for d in docs]) & base
        words = st.filter(pack_bits(base))
        assert (unpack(words, 1000) == want).all(), tree
        assert (unpack(words, 32 * words.shape[0])[1000:] == 0).all()
        full = st.filter()                  # no base: $not_contains sets every row without the text, tail still zero
        assert (unpack(full, 1000) == np.array([bf_match(tree, d) for d in docs])).all()
        assert (unpack(full, 32 * full.shape[0])[1000:] == 0).all()
        # device pointers on the current stream, twice, and on a side stream: identical bits
        b_t = torch.from_numpy(pack_bits(base).view(np.int32)).cuda()
        o1 = torch.zeros(words.shape[0], dtype=torch.int32, device="cuda")
        o2 = torch.zeros_like(o1)
        o3 = torch.zeros_like(o1)
        st.filter_device(o1, b_t)
        st.filter_device(o2, b_t)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            st.filter_device(o3, b_t)
        torch.cuda.synchronize()
        for o in (o1, o2, o3):
            assert (o.cpu().numpy().view(np.uint32) == words).all()
    st.close()


@pytest.mark.parametrize("rows", [0, 1, 32, 33, 1025])
def test_filter_words_are_the_same_in_both_spaces(rows):
    """host bitmaps are staged through the store's own buffers, device ones are taken as they are: both give the words of the
    host model, with and without base_bits. No rows (nothing is launched, nothing written), one row, a full word, a second word,
    more than 1024 rows; row 0 is longer than 1024 bytes, with a pattern across the start of its second segment."""
    import ctypes
    import torch
    from rag_dpo_amd import _lib as L
    from rag_dpo_amd import where_document as WD
    from rag_dpo_amd.where import pack_bits
    from rag_dpo_amd.engine import DocStore
    from test_where_document import TREES, make_docs
    docs = make_docs(rows, seed=6)
    if rows:
        docs[0] = "x" * 1019 + "article 28 … CNIL"
    words = (rows + 31) // 32
    base = np.random.default_rng(8).random(rows) < 0.7
    back = torch.from_numpy(np.append(pack_bits(base), np.uint32(0)).view(np.int32)).cuda()   # one word more: the base of no rows has an address too
    base_t = back[:words]
    st = DocStore(0)
    st.append(docs)
    for tree in TREES:
        st.set_query(*WD.compile_tree(tree))
        want = WD.evaluate_host(tree, docs)
        for b, b_t, expect in ((None, None, pack_bits(want)), (pack_bits(base), base_t, pack_bits(want & base))):
            host = st.filter(b)
            assert host.dtype == np.uint32 and host.shape == (words,) and (host == expect).all(), tree
            room = torch.full((words + 1,), -1, dtype=torch.int32, device="cuda")
            if rows:
                st.filter_device(room[:words], b_t)
            else:       # a tensor of no words has no address: the call itself, with the address of the word that must stay as it is
                L.check(st._lib.rdx_docs_filter(st._h, ctypes.c_void_p(back.data_ptr()) if b is not None else None, ctypes.c_void_p(room.data_ptr()),
                                                L.RDX_DEVICE, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
            torch.cuda.synchronize()
            got = room.cpu().numpy().view(np.uint32)
            assert (got[:words] == host).all() and got[words] == 0xFFFFFFFF, tree
    st.close()


def test_collection_contract_on_hipindex(tmp_path):
    from test_where_document import run_wd_contract
    from rag_dpo_amd.collection import _default_engine_factory
    col = run_wd_contract(_default_engine_factory, tmp_path)
    assert col._doc_store is not None and len(col._doc_store) == col._rows


def test_query_bit_identical_to_explicit_bitmap():
    from rag_dpo_amd import synth
    from rag_dpo_amd.where import pack_bits
    from test_where_document import TREES, bf_match, build
    col, emb = build(None, n=3000)
    q = synth.make_queries(4, emb.shape[1], emb)
    docs = col.get(include=["documents"])["documents"]
    for tree in TREES:
        allow = pack_bits(np.array([bf_match(tree, d) for d in docs]))
        s, r, c = col._engine.search(q, 50, allow_bits=allow)
        res = col.query(query_embeddings=q, n_results=50, where_document=tree, include=["distances"])
        for b in range(q.shape[0]):
            assert res["ids"][b] == [f"c{x}" for x in r[b, : c[b]]]
            assert res["distances"][b] == [float(np.float32(1.0) - x) for x in s[b, : c[b]]]
        # query_device: same rows and floats, twice
        import torch
        for _ in range(2):
            d, rr, cc = col.query_device(torch.from_numpy(q).cuda(), 50, where_document=tree)
            torch.cuda.synchronize()
            assert col.ids_of(rr.cpu()) == res["ids"]
            for b in range(q.shape[0]):
                assert d[b, : cc[b]].cpu().tolist() == res["distances"][b]


def test_multi_device_rehearsal():
    from rag_dpo_amd.collection import Collection
    from test_where_document import TREES, bf_match, make_docs, check_get
    from rag_dpo_amd import synth
    from oracle import oracle as O
    import torch
    n = 2500
    emb = synth.make_corpus(n, 64)
    docs = make_docs(n, seed=7)
    col = Collection("md", devices=[0, 0])
    col.add(ids=[f"c{i}" for i in range(n)], embeddings=emb, documents=docs)
    col.delete(ids=[f"c{i}" for i in range(0, n, 11)])
    q = synth.make_queries(2, 64, emb)
    alive = np.ones(n, dtype=bool)
    alive[::11] = False
    for tree in TREES:
        check_get(col, tree)
        allow = np.array([bf_match(tree, d) for d in docs]) & alive
        sc, rr, cn = O.cosine_topk(O.normalize_rows(emb), q, 30, allow)
        res = col.query(query_embeddings=q, n_results=30, where_document=tree, include=["distances"])
        for b in range(2):
            assert res["ids"][b] == [f"c{x}" for x in rr[b, : cn[b]]]
            assert res["distances"][b] == [float(np.float32(1.0) - s) for s in sc[b, : cn[b]]]
        d, r, c = col.query_device(torch.from_numpy(q).cuda(), 30, where_document=tree)
        torch.cuda.synchronize()
        assert col.ids_of(r.cpu()) == res["ids"]


def test_collection_without_where_document_allocates_no_store():
    from rag_dpo_amd import synth
    from rag_dpo_amd.collection import Collection
    from test_where_document import make_docs
    emb = synth.make_corpus(600, 64)
    col = Collection("plain")
    col.add(ids=[f"c{i}" for i in range(600)], embeddings=emb, documents=make_docs(600), metadatas=[{"i": i % 3} for i in range(600)])
    col.query(query_embeddings=emb[:2], n_results=10, where={"i": 1})
    col.get(where={"i": 2}, limit=5)
    col.update(ids=["c3"], documents=["new text"])
    col.upsert(ids=["c4", "x"], embeddings=emb[4:6], documents=["a", "b"])
    col.delete(ids=["c5"])
    col.get(where_document={})                 # {} is no filter: still nothing
    assert col._doc_store is None
    col.get(where_document={"$contains": "new"})
    assert col._doc_store is not None and len(col._doc_store) == col._rows
