"""where_document on the Chroma-shaped Collection: grammar, get / query / delete against brute force, and the C-ABI's argument
checks (no GPU needed). The oracle is written here: a recursive `needle in document` evaluator plus the exact-cosine oracle.
The same contract runs on the GPU engine in test_gpu_where_document.py."""
import ctypes

import numpy as np
import pytest

from rag_dpo_amd import synth
from rag_dpo_amd.collection import Collection, PersistentClient

from oracle_engine import factory as oracle_factory

WORDS = ["article 28", "AIPD", "sous-traitant", "données", "l’employeur", "RGPD", "CNIL", "durée de conservation",
         "consentement", "intérêt légitime", "Article 28", "sous-traitance", "é", "traitant"]


def bf_match(tree, doc):
    (op, val), = tree.items()
    if op == "$contains":
        return doc is not None and val in doc
    if op == "$not_contains":
        return not (doc is not None and val in doc)
    if op == "$and":
        return all(bf_match(t, doc) for t in val)
    return any(bf_match(t, doc) for t in val)


def make_docs(n, seed=0):
    rng = np.random.default_rng(seed)
    docs = []
    for i in range(n):
        if i % 17 == 3:
            docs.append(None)
        elif i % 17 == 5:
            docs.append("")
        else:
            k = int(rng.integers(1, 6))
            docs.append(f"chunk {i}: " + " … ".join(WORDS[j] for j in rng.integers(0, len(WORDS), size=k)))
    return docs


TREES = [
    {"$contains": "article 28"},
    {"$contains": "é"},
    {"$not_contains": "AIPD"},
    {"$contains": "l’employeur"},
    {"$and": [{"$contains": "sous-traitant"}, {"$not_contains": "RGPD"}]},
    {"$or": [{"$contains": "CNIL"}, {"$contains": "Article 28"}, {"$contains": "durée"}]},
    {"$and": [{"$or": [{"$contains": "données"}, {"$not_contains": "traitant"}]},
              {"$or": [{"$contains": "consentement"}, {"$and": [{"$contains": "intérêt"}, {"$not_contains": "CNIL"}]}]}]},
    {"$contains": "absent from every document"},
]


def build(factory, n=700, dim=32, seed=0):
    col = Collection("wd", metadata={"hnsw:space": "cosine"}, engine_factory=factory)
    emb = synth.make_corpus(n, dim)
    docs = make_docs(n, seed)
    ids = [f"c{i}" for i in range(n)]
    metas = [{"nat": ["GUIDE", "DOCTRINE", "SANCTION"][i % 3], "i": i} for i in range(n)]
    for a in range(0, n, 100):
        col.add(ids=ids[a:a + 100], embeddings=emb[a:a + 100], documents=docs[a:a + 100], metadatas=metas[a:a + 100])
    return col, emb


def state(col):
    """ids / documents / metadata of the live rows, in row order, straight from a full get()"""
    g = col.get(include=["documents", "metadatas"])
    return g["ids"], g["documents"], g["metadatas"]


def check_get(col, tree, where=None):
    ids, docs, metas = state(col)
    want = [i for i, d, m in zip(ids, docs, metas)
            if bf_match(tree, d) and (where is None or all((m or {}).get(k) == v for k, v in where.items()))]
    got = col.get(where=where, where_document=tree, include=["documents"])
    assert got["ids"] == want, tree
    assert got["documents"] == [docs[ids.index(i)] for i in want]
    return want


def check_query(col, emb_of, tree, q, k=25, where=None):
    from oracle import oracle as O
    ids, docs, metas = state(col)
    allow = np.array([bf_match(tree, d) and (where is None or all((m or {}).get(kk) == v for kk, v in where.items()))
                      for d, m in zip(docs, metas)], dtype=bool)
    rows = O.normalize_rows(np.stack([emb_of[i] for i in ids]).astype(np.float32))
    sc, rr, cn = O.cosine_topk(rows, q[None, :], k, allow)
    res = col.query(query_embeddings=[q.tolist()], n_results=k, where=where, where_document=tree,
                    include=["distances", "documents"])
    assert res["ids"][0] == [ids[r] for r in rr[0, : cn[0]]], tree
    assert res["distances"][0] == [float(np.float32(1.0) - s) for s in sc[0, : cn[0]]]
    return res


def run_wd_contract(factory, tmp_path=None, persist_factory=None):
    """the where_document contract on one engine factory (CPU: the oracle engine; GPU: HipIndex)"""
    col, emb = build(factory, n=2400)     # enough rows that deleting half of them compacts (> 1024 dead)
    emb_of = {f"c{i}": emb[i] for i in range(emb.shape[0])}
    q = synth.make_queries(3, emb.shape[1], emb)
    for t in TREES:
        check_get(col, t)
        check_query(col, emb_of, t, q[0])
    # with where, ids, paging
    t = TREES[1]
    check_get(col, t, where={"nat": "GUIDE"})
    check_query(col, emb_of, t, q[1], where={"nat": "DOCTRINE"})
    want = check_get(col, t)
    assert col.get(where_document=t, limit=7, offset=5)["ids"] == want[5:12]
    some = [f"c{i}" for i in range(0, 2400, 3)]
    assert col.get(ids=some, where_document=t)["ids"] == [i for i in want if i in set(some)]
    assert col.get(where_document={})["ids"] == col.get()["ids"]            # {} = no filter
    # update changes a document's text (and the filter answer), upsert adds and replaces
    col.update(ids=["c10", "c11"], documents=["now about article 28", None])
    col.upsert(ids=["c12", "new1"], embeddings=[emb[12], emb[13] * 0.5 + emb[14]], documents=["AIPD only", "article 28 AIPD"])
    emb_of["new1"] = emb[13] * 0.5 + emb[14]
    for t in TREES[:4]:
        check_get(col, t)
    assert "c10" in col.get(where_document={"$contains": "article 28"})["ids"]
    assert "c11" in col.get(where_document={"$not_contains": "article 28"})["ids"]
    # delete by where_document (alone, and narrowing ids=)
    before = col.count()
    gone = check_get(col, {"$contains": "AIPD"})
    col.delete(where_document={"$contains": "AIPD"})
    assert col.count() == before - len(gone)
    assert col.get(where_document={"$contains": "AIPD"})["ids"] == []
    col.delete(ids=["c0", "c1", "c2", "c4"], where_document={"$contains": "RGPD"})
    for t in TREES:
        check_get(col, t)
        check_query(col, emb_of, t, q[2])
    # enough deletes to compact the rows
    live = col.get()["ids"]
    col.delete(ids=live[: len(live) // 2])
    assert col._n_dead == 0 and col.count() == len(live) - len(live) // 2   # the deletes compacted the rows
    for t in TREES:
        check_get(col, t)
        check_query(col, emb_of, t, q[0], where={"nat": "SANCTION"})
    if tmp_path is not None:
        cl = PersistentClient(path=str(tmp_path), engine_factory=persist_factory or factory)
        c2 = cl.create_collection("p", metadata={"hnsw:space": "cosine"})
        g = col.get(include=["embeddings", "documents", "metadatas"])
        c2.add(ids=g["ids"], embeddings=g["embeddings"], documents=g["documents"], metadatas=g["metadatas"])
        c2.get(where_document=TREES[0])                                    # the store exists before the writes below
        c2.update(ids=[g["ids"][0]], documents=["article 28 after the store"])
        c2.delete(ids=[g["ids"][1]])
        want = {t_i: c2.get(where_document=t)["ids"] for t_i, t in enumerate(TREES)}
        cl.persist()
        c3 = PersistentClient(path=str(tmp_path), engine_factory=persist_factory or factory).get_collection("p")
        for t_i, t in enumerate(TREES):
            assert c3.get(where_document=t)["ids"] == want[t_i]
            check_get(c3, t)
    return col


# ---- grammar -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tree", TREES + [{"$and": [{"$contains": "a"}, {"$contains": "b"}, {"$contains": "c"}]}])
def test_grammar_accepts(tree):
    from rag_dpo_amd import where_document as WD
    WD.validate(tree)
    leaves, prog = WD.compile_tree(tree)
    assert all(isinstance(b, bytes) and b for b in leaves) and prog


@pytest.mark.parametrize("tree", [
    {"$regex": "a.*b"}, {"$not_regex": "x"},
    {"$contains": ""}, {"$contains": 3}, {"$not_contains": None},
    {"$and": [{"$contains": "a"}]}, {"$or": []}, {"$and": {"$contains": "a"}},
    {"$contains": "a", "$not_contains": "b"}, {"$in": ["a"]}, {"contains": "a"}, "article", ["$contains", "a"],
    {"$and": [{"$contains": "a"}, {"$regex": "b"}]},
])
def test_grammar_rejects(tree):
    col, _ = build(oracle_factory, n=40)
    with pytest.raises(ValueError):
        col.get(where_document=tree)
    with pytest.raises(ValueError):
        col.query(query_embeddings=[[0.1] * 32], n_results=3, where_document=tree)
    with pytest.raises(ValueError):
        col.delete(where_document=tree)
    assert col.count() == 40


def test_regex_says_not_implemented():
    col, _ = build(oracle_factory, n=10)
    with pytest.raises(ValueError, match="not implemented"):
        col.get(where_document={"$regex": "art.*28"})


def test_empty_where_document_is_no_filter():
    col, emb = build(oracle_factory, n=60)
    assert col.get(where_document={})["ids"] == col.get()["ids"]
    a = col.query(query_embeddings=[emb[3]], n_results=9, where_document={})
    b = col.query(query_embeddings=[emb[3]], n_results=9)
    assert a["ids"] == b["ids"] and a["distances"] == b["distances"]


def test_needle_rules():
    """byte-exact, case-sensitive, UTF-8; None and "" contain nothing and match $not_contains"""
    col = Collection("t", engine_factory=oracle_factory)
    docs = ["Élève", "eleve", None, "", "a’b", "x\x00y", "surrogat \udcff"]
    col.add(ids=[str(i) for i in range(len(docs))], embeddings=np.eye(len(docs), 8, dtype=np.float32) + 0.1, documents=docs)
    assert col.get(where_document={"$contains": "É"})["ids"] == ["0"]
    assert col.get(where_document={"$contains": "e"})["ids"] == ["0", "1"]
    assert col.get(where_document={"$contains": "’"})["ids"] == ["4"]
    assert col.get(where_document={"$contains": "\x00"})["ids"] == ["5"]
    assert col.get(where_document={"$contains": "\udcff"})["ids"] == ["6"]
    assert col.get(where_document={"$not_contains": "e"})["ids"] == ["2", "3", "4", "5", "6"]
    assert col.get(where_document={"$contains": "E"})["ids"] == []


# ---- the contract on the oracle engine --------------------------------------------------------------------
def test_contract_oracle_engine(tmp_path):
    run_wd_contract(oracle_factory, tmp_path)


# ---- C-ABI argument checks (no GPU) --------------------------------------------------------------------------
def _abi():
    from rag_dpo_amd import _lib
    from rag_dpo_amd.build import build_lib
    build_lib()
    return _lib, _lib.load(require_gpu=False)


def _arr(a, dt):
    a = np.ascontiguousarray(a, dtype=dt)
    return a, ctypes.c_void_p(a.ctypes.data)


def test_cabi_rejects_bad_arguments_without_gpu():
    _lib, L = _abi()
    INV = _lib.RDX_ERR_INVALID
    pat, pp = _arr(np.frombuffer(b"article28", dtype=np.uint8), np.uint8)
    off, po = _arr([0, 7, 9], np.int64)
    prog, pg = _arr([0, 1, _lib.DOCS_OP_AND], np.int32)
    h = ctypes.c_void_p()

    def rej(rc, words):
        assert rc == INV, rc
        msg = _lib.last_error()
        assert msg and words in msg, msg

    rej(L.rdx_docs_create(0, None), "null")
    rej(L.rdx_docs_set_query(h, pp, po, 0, pg, 3), "P must be")                       # P = 0
    rej(L.rdx_docs_set_query(h, None, po, 2, pg, 3), "null")                          # null bytes
    rej(L.rdx_docs_set_query(h, pp, None, 2, pg, 3), "null offsets")                  # null offsets
    e, pe = _arr([0, 0, 9], np.int64)
    rej(L.rdx_docs_set_query(h, pp, pe, 2, pg, 3), "strictly increasing")             # empty pattern
    d, pd = _arr([0, 7, 5], np.int64)
    rej(L.rdx_docs_set_query(h, pp, pd, 2, pg, 3), "strictly increasing")             # non-increasing offsets
    z, pz = _arr([1, 7, 9], np.int64)
    rej(L.rdx_docs_set_query(h, pp, pz, 2, pg, 3), "offsets[0]")
    bad, pb = _arr([0, _lib.DOCS_OP_AND], np.int32)
    rej(L.rdx_docs_set_query(h, pp, po, 2, pb, 2), "empty stack")                     # AND with one operand
    big, pbg = _arr([0, 5], np.int32)
    rej(L.rdx_docs_set_query(h, pp, po, 2, pbg, 2), "leaf")                           # leaf index >= P
    two, p2 = _arr([0, 1], np.int32)
    rej(L.rdx_docs_set_query(h, pp, po, 2, p2, 2), "exactly one")                     # two values left
    deep = [0] * 17 + [_lib.DOCS_OP_AND] * 16
    dp, pdp = _arr(deep, np.int32)
    rej(L.rdx_docs_set_query(h, pp, po, 2, pdp, len(deep)), "stack")
    rej(L.rdx_docs_set_query(h, pp, po, 2, None, 3), "program")
    rej(L.rdx_docs_set_query(None, pp, po, 2, pg, 3), "null store")                   # valid query, no store
    rej(L.rdx_docs_append(None, pp, pd, 2), "non-decreasing")
    rej(L.rdx_docs_append(None, pp, None, 2), "null offsets")
    rej(L.rdx_docs_append(None, None, po, 2), "null bytes")
    rej(L.rdx_docs_append(None, pp, po, -1), "n < 0")
    rej(L.rdx_docs_append(None, pp, po, 2), "null store")
    rej(L.rdx_docs_replace(None, None, pp, po, 2), "bad argument")
    rej(L.rdx_docs_compact(None, None, 0), "bad argument")
    x = ctypes.c_int64()
    rej(L.rdx_docs_stats(None, ctypes.byref(x), ctypes.byref(x), ctypes.byref(x)), "null")
    out, po2 = _arr(np.zeros(4), np.uint32)
    rej(L.rdx_docs_contains(None, po2, _lib.RDX_HOST, None), "null")
    rej(L.rdx_docs_filter(None, None, po2, _lib.RDX_HOST, None), "null")
    assert L.rdx_docs_destroy(None) == 0


def test_c_abi_argument_checks_under_asan_and_ubsan(tmp_path):
    """rdx_docs_* validate before they use the handle or touch a device: a stand-alone C program, built with the sanitizers,
    run on the CPU"""
    import os
    import subprocess
    from rag_dpo_amd import build
    here = os.path.dirname(os.path.abspath(__file__))
    lib_dir = os.path.dirname(build.build_lib())
    exe = str(tmp_path / "docs_errors")
    subprocess.check_call(["gcc", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1", "-std=c11",
                           "-Wall", "-I", os.path.join(os.path.dirname(here), "include"), os.path.join(here, "c_abi", "docs_errors.c"),
                           "-L", lib_dir, "-l:librdx.so", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    # (leak detection off: the HIP runtime librdx links keeps allocations of its own until process exit)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert "docs error paths ok: 35 checks" in r.stdout, r.stdout


def test_size_limits_hold_on_every_engine():
    """the device program's limits (16 stack entries, 1024 patterns, 4096 operations) apply to the host evaluator as well"""
    from rag_dpo_amd import where_document as WD
    col, _ = build(oracle_factory, n=50)
    deep = {"$contains": "x"}
    for i in range(20):                        # 20 levels of $and, each with a leaf beside the nested tree
        deep = {"$and": [{"$contains": f"w{i}"}, deep]}
    wide = {"$or": [{"$contains": f"p{i}"} for i in range(1025)]}
    for tree in (deep, wide):
        with pytest.raises(ValueError, match="too large"):
            WD.validate(tree)
        with pytest.raises(ValueError, match="too large"):
            col.get(where_document=tree)
        with pytest.raises(ValueError, match="too large"):
            col.query(query_embeddings=[[0.1] * 32], n_results=3, where_document=tree)
    ok = {"$or": [{"$contains": f"p{i}"} for i in range(1024)]}
    WD.validate(ok)
    assert col.get(where_document=ok)["ids"] == []


def test_store_failure_does_not_fail_the_write():
    """the device store is a cache of the documents: if keeping it in step fails, it is dropped and the write goes on"""
    col, emb = build(oracle_factory, n=30)

    class Broken:
        closed = False

        def append(self, docs):
            raise MemoryError("device out of memory")

        def replace(self, rows, docs):
            raise RuntimeError("device error")

        def close(self):
            Broken.closed = True

    for op in ("add", "update"):
        col._doc_store = Broken()
        if op == "add":
            col.add(ids=["z1"], embeddings=emb[:1], documents=["qqq late"])
        else:
            col.update(ids=["c1"], documents=["qqq updated"])
        assert col._doc_store is None and Broken.closed
    assert col.get(where_document={"$contains": "qqq"})["ids"] == ["c1", "z1"]
