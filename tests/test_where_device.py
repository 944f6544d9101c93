"""CPU: the `where` compiler of rag_dpo_amd/where_device.py against its model, rag_dpo_amd/where.py — the compiled form, run by
the numpy interpreter that states what the device kernel computes, gives W.evaluate's rows bit for bit; trees over the device's
limits are "not compilable" and still answered by the host; engines without a device store never construct one."""
import os

import numpy as np
import pytest

from rag_dpo_amd import synth
from rag_dpo_amd import where as W
from rag_dpo_amd import where_device as WV
from rag_dpo_amd.collection import Collection

from oracle_engine import OracleEngine, factory as oracle_factory

BIG = 2 ** 53 - 1
STRS = ["GUIDE", "DOCTRINE", "SANCTION", "TECHNIQUE", "", "é’", "guide"]
INTS = [0, 1, -1, 2, 7, BIG, -BIG]
FLOATS = [0.0, -0.0, 1.0, 0.5, -2.25, 1e300, float("inf"), float("nan")]
KEYS = ["s", "i", "f", "b", "mix", "sparse", "absent"]      # "absent" is in no row


def make_columns(n, seed=0):
    """one column per kind with a fifth of the rows missing, "mix" with every kind in one column, "sparse" nearly empty"""
    rng = np.random.default_rng(seed)
    pools = {"s": STRS[:6], "i": INTS, "f": FLOATS, "b": [True, False]}
    cols = {k: W.Column(n) for k in KEYS if k != "absent"}
    for r in range(n):
        for k, pool in pools.items():
            if rng.random() < 0.8:
                cols[k].set(r, pool[int(rng.integers(0, len(pool)))])
        if rng.random() < 0.85:
            pool = pools["sibf"[int(rng.integers(0, 4))]]
            cols["mix"].set(r, pool[int(rng.integers(0, len(pool)))])
        if rng.random() < 0.03:
            cols["sparse"].set(r, 1)
    return cols


def operand(rng, kind=None):
    """an operand of any kind, whatever the column holds: a string the vocabulary lacks, NaN, -0.0, True against ints, +-(2^53 - 1)"""
    kind = "sifb"[int(rng.integers(0, 4))] if kind is None else kind
    if kind == "s":
        return (STRS + ["not in any vocabulary"])[int(rng.integers(0, len(STRS) + 1))]
    if kind == "i":
        return INTS[int(rng.integers(0, len(INTS)))]
    if kind == "f":
        return FLOATS[int(rng.integers(0, len(FLOATS)))]
    return bool(rng.integers(0, 2))


def random_tree(rng, depth):
    if depth > 0 and rng.random() < 0.6:
        return {("$and", "$or")[int(rng.integers(0, 2))]: [random_tree(rng, depth - 1) for _ in range(int(rng.integers(2, 5)))]}
    key = KEYS[int(rng.integers(0, len(KEYS)))]
    op = ("$eq", "$ne", "$gt", "$gte", "$lt", "$lte", "$in", "$nin", None)[int(rng.integers(0, 9))]
    if op is None:
        return {key: operand(rng)}
    if op in ("$in", "$nin"):
        kind = "sifb"[int(rng.integers(0, 4))]
        return {key: {op: [operand(rng, kind) for _ in range(int(rng.integers(1, 41)))]}}
    if op in ("$gt", "$gte", "$lt", "$lte"):
        return {key: {op: operand(rng, "if"[int(rng.integers(0, 2))])}}
    return {key: {op: operand(rng)}}


def count_leaves(tree):
    (key, val), = tree.items()
    if key in ("$and", "$or"):
        return sum(count_leaves(x) for x in val)
    if isinstance(val, dict) and next(iter(val)) in ("$in", "$nin") and key != "absent":
        return len(next(iter(val.values())))
    return 1


def run_compiled(tree, cols, n):
    c = WV.compile_where(tree, cols)
    assert c is not None, tree
    return WV.run_program_host(c.leaves, c.program, [cols[k] for k in c.keys], n), c


def nested(levels, leaf=lambda i: {"i": i}):
    """`levels` operators nested in the SECOND operand: the postfix form holds one entry per level before the first fold"""
    t = leaf(levels)
    for i in range(levels - 1, -1, -1):
        t = {("$or", "$and")[i % 2]: [leaf(i), t]}
    return t


def stack_depth(program):
    d = top = 0
    for op in program.tolist():
        d += 1 if op >= 0 else (0 if op == WV.OP_NOT else -1)
        top = max(top, d)
    return top


def test_compiled_form_equals_the_host_evaluator_on_random_trees():
    n = 257
    cols = make_columns(n)
    assert {int(k) for k in np.unique(cols["mix"].kind[:n])} == {0, 1, 2, 3, 4} and "absent" not in cols
    rng = np.random.default_rng(1)
    ops_seen, passing, too_big = set(), 0, 0
    for t in range(300):
        tree = random_tree(rng, int(rng.integers(0, 7)))
        want = W.evaluate(tree, cols, n)
        if count_leaves(tree) > WV.MAX_LEAVES:             # a few of the deepest trees: over the device's limit, the host's business
            assert WV.compile_where(tree, cols) is None
            too_big += 1
            continue
        got, c = run_compiled(tree, cols, n)
        assert got.dtype == bool and np.array_equal(got, want), tree
        ops_seen |= set(c.leaves["op"].tolist()) | set(c.program[c.program < 0].tolist())
        passing += int(want.any() and not want.all())
    assert ops_seen == {WV.EQ, WV.GT, WV.GE, WV.LT, WV.LE, WV.CONST0, WV.CONST1, WV.OP_NOT, WV.OP_AND, WV.OP_OR}
    assert passing >= 50 and too_big < 15                  # a good share of the trees pass some rows and not others; nearly all compile


@pytest.mark.parametrize("tree", [
    {"i": True}, {"i": {"$ne": True}}, {"b": 1}, {"i": 1.0}, {"f": 1}, {"mix": 1}, {"mix": True}, {"mix": 1.0},   # one kind only
    {"f": float("nan")}, {"f": {"$ne": float("nan")}}, {"f": {"$gte": float("nan")}}, {"f": {"$in": [float("nan"), 0.5]}},
    {"f": -0.0}, {"f": 0.0}, {"f": {"$lt": -0.0}}, {"f": {"$lte": -0.0}}, {"f": {"$gt": 0.0}}, {"mix": {"$nin": [0.0]}},
    {"i": BIG}, {"i": -BIG}, {"i": {"$gt": BIG - 1}}, {"i": {"$lt": -BIG + 1}}, {"i": {"$gte": BIG}}, {"mix": {"$lte": -BIG}},
    {"s": "not in any vocabulary"}, {"s": {"$ne": "not in any vocabulary"}}, {"s": {"$in": ["nope", "GUIDE", "never"]}},
    {"s": {"$nin": ["nope"]}}, {"s": ""}, {"mix": "é’"}, {"i": "GUIDE"},
    {"absent": 1}, {"absent": {"$ne": 1}}, {"absent": {"$in": [1, 2]}}, {"absent": {"$nin": ["x"]}}, {"absent": {"$gt": 0}},
    {"sparse": 1}, {"sparse": {"$ne": 1}},
], ids=repr)
def test_operand_edges(tree):
    n = 257
    cols = make_columns(n)
    got, _ = run_compiled(tree, cols, n)
    assert np.array_equal(got, W.evaluate(tree, cols, n))


def test_lowering_of_the_reference_filter():
    cols = make_columns(64)
    w = {"$and": [{"s": {"$in": ["GUIDE", "DOCTRINE", "nope"]}}, {"$or": [{"i": {"$ne": 1}}, {"b": True}, {"absent": True}]}]}
    c = WV.compile_where(w, cols)
    assert c.keys == ("s", "i", "b")
    lv = c.leaves
    assert lv["op"].tolist() == [WV.EQ] * 5 + [WV.CONST0] and lv["col"].tolist() == [0, 0, 0, 1, 2, -1]
    assert lv["kind"].tolist()[:5] == [W.K_STR] * 3 + [W.K_INT, W.K_BOOL]
    assert lv["code"].tolist()[:3] == [cols["s"]._lookup["GUIDE"], cols["s"]._lookup["DOCTRINE"], -2]
    assert lv["num"].tolist()[3:5] == [1.0, 1.0]
    N, A, O = WV.OP_NOT, WV.OP_AND, WV.OP_OR
    assert c.program.tolist() == [0, 1, O, 2, O, 3, N, 4, O, 5, O, A]
    assert lv.dtype.itemsize == 24 and lv.dtype == WV.LEAF


def test_limits_are_not_compilable_not_errors():
    cols = make_columns(64)
    t16, t17 = nested(15), nested(16)                      # 16 and 17 operands on the stack
    c = WV.compile_where(t16, cols)
    assert c is not None and stack_depth(c.program) == WV.MAX_STACK == 16
    assert np.array_equal(WV.run_program_host(c.leaves, c.program, [cols[k] for k in c.keys], 64), W.evaluate(t16, cols, 64))
    assert WV.compile_where(t17, cols) is None
    assert WV.compile_where(nested(17), cols) is None      # 17 nested levels
    assert WV.compile_where({"i": {"$in": list(range(1024))}}, cols) is not None
    assert WV.compile_where({"i": {"$in": list(range(1100))}}, cols) is None
    assert WV.compile_where({"i": {"$nin": list(range(1025))}}, cols) is None
    # 1000 leaves under 500 + 499 + 1000 operators: the lowering spends at most 3 ops per leaf, so 1024 leaves stay under 4096 ops
    many = {"$or": [{"$and": [{"i": {"$ne": j}}, {"f": {"$ne": 0.5}}]} for j in range(500)]}
    c = WV.compile_where(many, cols)
    assert c is not None and c.leaves.shape[0] == 1000 and c.program.shape[0] == 2999 <= WV.MAX_OPS
    assert np.array_equal(WV.run_program_host(c.leaves, c.program, [cols[k] for k in c.keys], 64), W.evaluate(many, cols, 64))


BAD = [None, [], "x", {}, {"a": 1, "b": 2}, {1: 2}, {"$xor": [{"a": 1}, {"b": 2}]}, {"$and": [{"a": 1}]}, {"$or": {"a": 1}},
       {"$and": [{"a": 1}, {"b": {"$like": 1}}]}, {"a": {"$in": []}}, {"a": {"$in": [1, "x"]}}, {"a": {"$nin": 3}},
       {"a": {"$gt": "x"}}, {"a": {"$lte": True}}, {"a": {"$eq": None}}, {"a": [1]}, {"a": {"$eq": 1, "$ne": 2}},
       {"$or": [{"i": 1}, {"$and": [{"i": 2}, {"i": {"$gt": [1]}}]}]}]


@pytest.mark.parametrize("bad", BAD, ids=repr)
def test_malformed_filters_raise_what_validate_where_raises(bad):
    with pytest.raises(ValueError) as model:
        W.validate_where(bad)
    with pytest.raises(ValueError) as got:
        WV.compile_where(bad, make_columns(8))
    assert str(got.value) == str(model.value)


class NoStore:
    def __init__(self, *a, **kw):
        raise AssertionError("a MetaStore was constructed")


class StoreEngine(OracleEngine):
    has_device_meta = True          # an engine that says it has a device store: only the filter decides


def fill(col, n=400):
    emb = synth.make_corpus(n, 64)
    col.add(ids=[f"c{i}" for i in range(n)], embeddings=emb,
            metadatas=[{"i": i % 7, "s": STRS[i % 4], **({"tag": True} if i % 5 == 0 else {})} for i in range(n)])
    return emb


def test_not_compilable_filters_take_the_host_path(monkeypatch):
    import rag_dpo_amd.engine as E
    monkeypatch.setattr(E, "MetaStore", NoStore)
    plain = Collection("plain", engine_factory=oracle_factory)
    col = Collection("dev", engine_factory=lambda dim, device=0: StoreEngine(dim, device))
    col._WHERE_DEVICE_MIN_ROWS = 0
    emb = fill(plain)
    fill(col)
    q = synth.make_queries(2, 64, emb)
    deep = nested(17, leaf=lambda i: {"i": {"$ne": i % 3}} if i % 2 else {"tag": True})
    for w in (deep, {"i": {"$in": list(range(3, 1103))}}):
        assert WV.compile_where(w, col._cols) is None
        a = col.query(query_embeddings=q, n_results=20, where=w)
        b = plain.query(query_embeddings=q, n_results=20, where=w)
        assert a["ids"] == b["ids"] and a["distances"] == b["distances"] and len(a["ids"][0]) > 0
    assert col._meta_store is None
    with pytest.raises(AssertionError, match="MetaStore was constructed"):   # a compilable one does reach for the store
        col.query(query_embeddings=q, n_results=20, where={"i": 1})
    assert col._meta_store is None and not col._meta_res


def test_a_failing_store_is_closed_and_the_host_answers(monkeypatch):
    import rag_dpo_amd.engine as E
    made = []

    class FullCard:
        device = 0

        def __init__(self, device=0):
            made.append(self)
            self.closed = False

        def set_rows(self, *a):
            raise MemoryError("hipMalloc(90000000): out of memory")

        def close(self):
            self.closed = True

    monkeypatch.setattr(E, "MetaStore", FullCard)
    plain = Collection("plain", engine_factory=oracle_factory)
    col = Collection("dev", engine_factory=lambda dim, device=0: StoreEngine(dim, device))
    col._WHERE_DEVICE_MIN_ROWS = 0
    emb = fill(plain)
    fill(col)
    q = synth.make_queries(2, 64, emb)
    for w in ({"i": 1}, {"$or": [{"s": "GUIDE"}, {"tag": True}]}):
        a = col.query(query_embeddings=q, n_results=20, where=w)
        b = plain.query(query_embeddings=q, n_results=20, where=w)
        assert a["ids"] == b["ids"] and a["distances"] == b["distances"] and len(a["ids"][0]) > 0
        assert col._meta_store is None and not col._meta_res
    assert len(made) == 2 and all(m.closed for m in made)      # each filter tried to build the store again


def test_oracle_engine_never_constructs_a_store(monkeypatch):
    import rag_dpo_amd.engine as E
    monkeypatch.setattr(E, "MetaStore", NoStore)
    col = Collection("plain", engine_factory=oracle_factory)
    col._WHERE_DEVICE_MIN_ROWS = 0
    emb = fill(col)
    q = synth.make_queries(1, 64, emb)
    r = col.query(query_embeddings=q, n_results=400, where={"$and": [{"s": {"$in": STRS[:2]}}, {"$or": [{"i": {"$ne": 3}}, {"tag": True}]}]})
    assert sorted(r["ids"][0]) == sorted(f"c{i}" for i in range(400) if i % 4 < 2 and (i % 7 != 3 or i % 5 == 0))
    col.query(query_embeddings=q, n_results=5, where={"i": 2}, where_document={"$not_contains": "x"})
    col.update(ids=["c3"], metadatas=[{"i": "now a string"}])
    col.delete(where={"i": 1})
    col.query(query_embeddings=q, n_results=5, where={"i": {"$gte": 2}})
    assert col._meta_store is None and not col._meta_res


def test_a_key_first_seen_mid_batch_is_missing_in_the_rest_of_the_batch():
    col = Collection("plain", engine_factory=oracle_factory)
    emb = synth.make_corpus(300, 64)
    col.add(ids=[f"a{i}" for i in range(200)], embeddings=emb[:200], metadatas=[{"k": i} for i in range(200)])
    col.add(ids=[f"b{i}" for i in range(100)], embeddings=emb[200:], metadatas=[{"k": i, **({"new": 1} if i == 0 else {})} for i in range(100)])
    r = col.query(query_embeddings=emb[:1], n_results=300, where={"new": {"$ne": 1}})
    assert len(r["ids"][0]) == 299 and "b0" not in r["ids"][0]
    assert col.get(where={"new": 1})["ids"] == ["b0"]


def test_c_abi_argument_checks_under_asan_and_ubsan(tmp_path):
    """rdx_meta_* validate before they use the handle or touch a device: a stand-alone C program, built with the sanitizers,
    run on the CPU"""
    import subprocess
    from rag_dpo_amd import build
    here = os.path.dirname(os.path.abspath(__file__))
    lib_dir = os.path.dirname(build.build_lib())
    exe = str(tmp_path / "meta_errors")
    subprocess.check_call(["gcc", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1", "-std=c11",
                           "-Wall", "-I", os.path.join(os.path.dirname(here), "include"), os.path.join(here, "c_abi", "meta_errors.c"),
                           "-L", lib_dir, "-l:librdx.so", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    # (leak detection off: the HIP runtime librdx links keeps allocations of its own until process exit)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert "meta error paths ok: 39 checks" in r.stdout, r.stdout
