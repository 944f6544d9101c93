"""TEST-ONLY: random write histories of a Collection, replayed against a from-scratch rebuild (plain Python and numpy).

A Collection keeps derived copies of its rows (mask cache, per-row metadata cache, MetaStore, DocStore, GroupTables, the engine's scan
copies), each with a rule of its own for when a write invalidates it. What a caller can see must not depend on any of them: after ANY
sequence of writes a collection answers as a collection that was given the surviving content, in row order, by one add.

  Model       the content: an ordered map id -> [raw embedding, metadata dict or None, document], in row order
  History     a seeded generator of write steps; every step is applied to the generator's own Model as it is yielded
  checks      the fixed list of calls made after every write (so every filter is warm from the step before)
  diff/same   deep equality: floats by their bits, arrays by dtype, shape and bytes, exceptions by type and message
  replay      applies a history to a live collection and compares it, check by check, with Model.fresh() after every write

Every host-list method answers in ids, never in row numbers; group and facet codes are numbered by first appearance among the live
rows; a compaction keeps the row order. So the comparison is exact, and there is no tolerance anywhere in this file.
"""
import struct
from collections import OrderedDict

import numpy as np

SRC = ("alpha", "beta", "gamma", "delta")
MIXED = (1, True, 1.0, "1", "x", 2)           # one key holding every kind: 1, True and 1.0 are three values
GROUP_KEY = "doc"                             # six rows per value: what query_groups groups by, and the group a step deletes whole
PLATEAU_KEY = "plateau"                       # nine values of (nearly) equal counts: the order inside a tie is the first appearance
BAD_WHERE = {"mixed": {"$in": [1, "a"]}}      # refused by every family: the operands of $in are of two kinds

# (name, where, where_document): every family is asked under each of them
FILTERS = (
    ("none", None, None),
    ("str", {"src": "beta"}, None),
    ("num", {"n": {"$gte": 200}}, None),
    ("doc", None, {"$contains": "cookies"}),
    ("both", {"src": {"$ne": "alpha"}}, {"$not_contains": "cookies"}),
)

WRITE_KINDS = ("add", "update_emb", "update_meta", "update_doc", "upsert", "delete_ids", "delete_where", "delete_where_doc", "readd",
               "reload_journal", "reload_persist")
EDGES = ("cross32", "cross_capacity", "first_of_value", "whole_group", "delete_all", "add_after_empty", "dup_row", "unknown_id",
         "new_key", "kind_change", "new_string", "upsert_mixed")

# Deliberate differences between a live collection and its rebuild: (check name or prefix, reason). replay() reads this table and
# leaves the named checks out of the comparison; it is empty because no difference found so far was deliberate.
DELIBERATE = ()


def meta_of(i: int) -> dict:
    m = {"src": SRC[i % 4], "n": i, GROUP_KEY: f"d{i // 6}", PLATEAU_KEY: f"p{i % 9}"}
    if i % 5:
        m["mixed"] = MIXED[i % 6]
    return m


def text_of(i: int):
    if i % 13 in (7, 8):                      # a row without a document, and one whose document is empty
        return None if i % 13 == 7 else ""
    return f"chunk {i} about {'cookies' if i % 3 == 0 else 'registre'} in {SRC[i % 4]}"


# ---- the filters, restated over dicts and strings (the model's delete(where=, where_document=)) -----------------------------------
def _kind(v):
    return "b" if isinstance(v, bool) else "i" if isinstance(v, int) else "f" if isinstance(v, float) else "s"


def _eq(v, x) -> bool:
    return v is not None and _kind(v) == _kind(x) and v == x


def match_where(where, meta) -> bool:
    if where in (None, {}):
        return True
    (key, val), = where.items()
    if key == "$and":
        return all(match_where(w, meta) for w in val)
    if key == "$or":
        return any(match_where(w, meta) for w in val)
    op, x = next(iter(val.items())) if isinstance(val, dict) else ("$eq", val)
    v = (meta or {}).get(key)
    if op in ("$eq", "$ne"):
        return _eq(v, x) == (op == "$eq")
    if op in ("$in", "$nin"):
        return any(_eq(v, y) for y in x) == (op == "$in")
    if v is None or _kind(v) != _kind(x):
        return False
    return {"$gt": v > x, "$gte": v >= x, "$lt": v < x, "$lte": v <= x}[op]


def match_document(tree, doc) -> bool:
    if not tree:
        return True
    (op, val), = tree.items()
    if op == "$contains":
        return doc is not None and val in doc
    if op == "$not_contains":
        return not (doc is not None and val in doc)
    parts = [match_document(t, doc) for t in val]
    return all(parts) if op == "$and" else any(parts)


class Model:
    """id -> [raw embedding, metadata, document] in row order, with Collection's write methods (the keyword arguments replay uses)"""

    def __init__(self):
        self.rows = OrderedDict()

    def __len__(self):
        return len(self.rows)

    def ids(self):
        return list(self.rows)

    def add(self, ids, embeddings, metadatas=None, documents=None):
        for j, s in enumerate(ids):
            if s not in self.rows:                       # add never overwrites; a deleted id that comes back goes to the end
                m = metadatas[j] if metadatas is not None else None
                m = {k: v for k, v in (m or {}).items() if v is not None}
                self.rows[s] = [np.array(embeddings[j], dtype=np.float32), m or None, documents[j] if documents is not None else None]

    def update(self, ids, embeddings=None, metadatas=None, documents=None):
        for j, s in enumerate(ids):
            row = self.rows.get(s)
            if row is None:                              # unknown ids are ignored
                continue
            if embeddings is not None:
                row[0] = np.array(embeddings[j], dtype=np.float32)
            if metadatas is not None and metadatas[j]:   # merged; None takes the key away
                m = dict(row[1] or {})
                for k, v in metadatas[j].items():
                    if v is None:
                        m.pop(k, None)
                    else:
                        m[k] = v
                row[1] = m or None
            if documents is not None:
                row[2] = documents[j]

    def upsert(self, ids, embeddings=None, metadatas=None, documents=None):
        old = [j for j, s in enumerate(ids) if s in self.rows]
        new = [j for j, s in enumerate(ids) if s not in self.rows]
        pick = lambda lst, idx: None if lst is None else [lst[j] for j in idx]   # noqa: E731
        if old:
            self.update(pick(ids, old), pick(embeddings, old), pick(metadatas, old), pick(documents, old))
        if new:
            self.add(pick(ids, new), pick(embeddings, new), pick(metadatas, new), pick(documents, new))

    def matching(self, where=None, where_document=None):
        return [s for s, (_, m, d) in self.rows.items() if match_where(where, m) and match_document(where_document, d)]

    def delete(self, ids=None, where=None, where_document=None):
        gone = self.matching(where, where_document)
        if ids is not None:
            keep = set(ids)
            gone = [s for s in gone if s in keep]
        for s in gone:
            del self.rows[s]

    def fresh(self, factory, name: str = "fresh"):
        """a new Collection holding the map, given to it by a single add"""
        from rag_dpo_amd.collection import Collection
        col = Collection(name, engine_factory=factory)
        if self.rows:
            col.add(ids=list(self.rows), embeddings=np.stack([r[0] for r in self.rows.values()]),
                    metadatas=[dict(r[1]) if r[1] else None for r in self.rows.values()], documents=[r[2] for r in self.rows.values()])
        return col


# ---- the histories -----------------------------------------------------------------------------------------------------------------
def _round256(n: int) -> int:
    return (n + 255) // 256 * 256


class History:
    """history(seed, dim, rows0, steps): iterating yields `steps` + 1 write steps (the first adds rows0 rows), each a dict
    {"kind", "op": the Collection method or "reload", "kwargs", "edges": [names of EDGES this step is an instance of]} that has been
    applied to self.model when it is yielded. self.log keeps the steps. The generator follows the physical state the writes leave
    behind (rows with tombstones `phys`, dead rows `dead`, the engine's capacity `cap`: a multiple of 256 that grows by half) by the
    rules of Collection and csrc/index_state.hpp; replay() compares phys and dead with the live collection after every step."""

    BASE = (["add"] * 8 + ["update_emb"] * 2 + ["update_meta"] * 4 + ["update_doc"] * 2 + ["upsert"] * 3
            + ["delete_ids", "delete_first", "delete_where", "delete_group", "delete_where_doc", "reload_journal", "reload_persist"])
    PAIRS = ("readd", "delete_all")             # kinds of two steps each: 26 + 2 * 2 = 30 steps

    def __init__(self, seed: int, dim: int, rows0: int = 300, steps: int = 30):
        if steps < len(self.BASE) + 2 * len(self.PAIRS):
            raise ValueError("a history needs 30 steps to hold every write kind and edge")
        self.seed, self.dim, self.rows0, self.steps = seed, dim, rows0, steps
        self.rng = np.random.default_rng(seed)
        self.centres = self.rng.standard_normal((4, dim)).astype(np.float32)
        self.q = (self.centres[:3] + 0.7 * self.rng.standard_normal((3, dim))).astype(np.float32)
        self.model = Model()
        self.log = []
        self.serial = 0
        self.phys = self.dead = self.cap = 0
        self.grown = self.crossed32 = self.dup_done = False

    # -- content
    def _emb(self, i: int):
        return (self.centres[i % 4] + 0.7 * self.rng.standard_normal(self.dim)).astype(np.float32)

    def _new_rows(self, n: int) -> dict:
        ii = list(range(self.serial, self.serial + n))
        self.serial += n
        return {"ids": [f"r{i}" for i in ii], "embeddings": np.stack([self._emb(i) for i in ii]), "metadatas": [meta_of(i) for i in ii],
                "documents": [text_of(i) for i in ii]}

    def _pick(self, n: int):
        ids = self.model.ids()
        return [ids[j] for j in sorted(self.rng.choice(len(ids), size=min(n, len(ids)), replace=False).tolist())]

    # -- the physical state
    def _added(self, n: int, edges: list):
        before, self.phys = self.phys, self.phys + n
        if before and before // 32 < (self.phys - 1) // 32:   # before < 32 m < phys: the add ends inside a new word of every bitmap
            edges.append("cross32")
            self.crossed32 = True
        if self.phys > self.cap:
            if self.cap:
                edges.append("cross_capacity")
                self.grown = True
            self.cap = _round256(max(self.phys, self.cap + self.cap // 2))

    def _deleted(self, n: int):
        self.dead += n
        if n and self.dead > max(1024, self.phys // 5):       # Collection._maybe_compact
            self.phys, self.dead = self.phys - self.dead, 0
            self.cap = max(256, _round256(self.phys))

    # -- one step per kind
    def _step(self, kind: str, op: str, kwargs: dict, edges=()):
        live0 = len(self.model)
        if op != "reload":
            getattr(self.model, op)(**kwargs)
        edges = list(edges)
        if op in ("add", "upsert"):
            self._added(len(self.model) - live0, edges)
        elif op == "delete":
            self._deleted(live0 - len(self.model))
        elif kind == "reload_persist":                         # the snapshot is written compacted and read back by one add
            self.phys, self.dead = len(self.model), 0
            self.cap = _round256(self.phys)
        step = {"kind": kind, "op": op, "kwargs": kwargs, "edges": edges}
        self.log.append(step)
        return step

    def _add(self, kind="add", edges=()):
        edges = list(edges)
        if not self.crossed32 and self.phys % 32:
            n = 32 - self.phys % 32 + 1                        # one row past the next multiple of 32
        elif not self.grown:
            n = 40                                             # towards the capacity
        else:
            n = int(self.rng.integers(1, 41))
        kw = self._new_rows(n)
        if not self.dup_done and len(self.model) and n >= 3:   # an exact copy of a stored row, one of a new row, and a near-copy
            src = self.model.rows[self._pick(1)[0]][0]
            kw["embeddings"][0] = src
            kw["embeddings"][2] = kw["embeddings"][1]
            if n >= 4:
                kw["embeddings"][3] = kw["embeddings"][1] + np.float32(0.01) * self.rng.standard_normal(self.dim).astype(np.float32)
            self.dup_done = True
            edges.append("dup_row")
        return self._step(kind, "add", kw, edges)

    def _update_emb(self):
        ids = self._pick(4) + ["no such id"]
        return self._step("update_emb", "update", {"ids": ids, "embeddings": np.stack([self._emb(j) for j in range(len(ids))])}, ["unknown_id"])

    def _update_meta(self):
        ids = self._pick(7)
        t = len(self.log)
        changes = [{"late": t}, {"n": 1000.5 + t}, {"n": f"n{t}"}, {"src": f"epsilon{t % 2}"}, {"src": "beta", "mixed": None},
                   {PLATEAU_KEY: "p0", GROUP_KEY: "d0"}, {"mixed": 1.0, "n": 7}]
        return self._step("update_meta", "update", {"ids": ids, "metadatas": changes[: len(ids)]}, ["new_key", "kind_change", "new_string"])

    def _update_doc(self):
        ids = self._pick(5)
        docs = [f"chunk {s} rewritten about {'registre' if 'cookies' in (self.model.rows[s][2] or '') else 'cookies'}"
                for s in ids]                                   # every row changes sides of "cookies"
        if len(docs) > 3:
            docs[3] = None                                      # and one loses its document
        return self._step("update_doc", "update", {"ids": ids, "documents": docs})

    def _upsert(self):
        old = self._pick(4)
        kw = self._new_rows(6)
        for j, s in enumerate(old):                             # known and new ids interleaved
            at = 2 * j
            kw["ids"].insert(at, s)
            kw["embeddings"] = np.insert(kw["embeddings"], at, self._emb(j), axis=0)
            kw["metadatas"].insert(at, {"src": SRC[(j + 1) % 4], "n": 150 + 100 * (j % 2)})
            kw["documents"].insert(at, f"upserted {s} about {'cookies' if j % 2 else 'registre'}")
        return self._step("upsert", "upsert", kw, ["upsert_mixed"])

    def _delete_ids(self):
        return self._step("delete_ids", "delete", {"ids": self._pick(5) + ["no such id"]}, ["unknown_id"])

    def _delete_first(self):
        """the first live row of the second plateau value met in row order: the value's code, and its place among equal counts, change"""
        seen, victim = [], None
        for s, (_, m, _) in self.model.rows.items():
            v = (m or {}).get(PLATEAU_KEY)
            if v is not None and v not in seen:
                seen.append(v)
                if len(seen) == 2:
                    victim = s
                    break
        victim = victim or self.model.ids()[0]
        return self._step("delete_ids", "delete", {"ids": [victim]}, ["first_of_value"])

    def _delete_where(self):
        m = self.model.rows[self._pick(1)[0]][1] or {}
        where = {"$and": [{"src": m.get("src", "gamma")}, {PLATEAU_KEY: m.get(PLATEAU_KEY, "p4")}]}
        return self._step("delete_where", "delete", {"where": where})

    def _delete_group(self):
        groups = [m[GROUP_KEY] for _, m, _ in self.model.rows.values() if m and isinstance(m.get(GROUP_KEY), str)]
        g = groups[int(self.rng.integers(len(groups)))]
        assert len(self.model.matching({GROUP_KEY: g})) >= 1
        return self._step("delete_where", "delete", {"where": {GROUP_KEY: g}}, ["whole_group"])

    def _delete_where_doc(self):
        d = int(self.rng.integers(10))
        return self._step("delete_where_doc", "delete", {"where": {"src": {"$in": ["delta", "beta"]}}, "where_document": {"$contains": f"{d} about"}})

    def _readd(self):
        s = self._pick(1)[0]
        emb, meta, doc = self.model.rows[s]
        yield self._step("delete_ids", "delete", {"ids": [s]})
        yield self._step("readd", "add", {"ids": [s], "embeddings": emb[None, :].copy(), "metadatas": [dict(meta) if meta else None],
                                          "documents": [doc]})

    def _delete_all(self):
        yield self._step("delete_ids", "delete", {"ids": self.model.ids()}, ["delete_all"])
        yield self._add(edges=["add_after_empty"])

    def __iter__(self):
        rng = self.rng
        yield self._step("add", "add", self._new_rows(self.rows0))
        kinds = list(self.BASE) + ["readd"]
        simple = ("add", "update_emb", "update_meta", "update_doc", "upsert", "delete_ids")
        kinds += [simple[int(rng.integers(len(simple)))] for _ in range(self.steps - len(kinds) - 3)]
        kinds = [kinds[j] for j in rng.permutation(len(kinds))]
        a, b = kinds.index("reload_journal"), kinds.index("reload_persist")
        if a > b:                                               # first from the journal alone: no snapshot has been written yet
            kinds[a], kinds[b] = kinds[b], kinds[a]
        kinds.insert(int(rng.integers(len(kinds) * 2 // 3, len(kinds))), "delete_all")    # late: most steps see a populated collection
        for kind in kinds:
            if kind in self.PAIRS:
                yield from getattr(self, "_" + kind)()
            elif kind.startswith("reload"):
                yield self._step(kind, "reload", {})
            else:
                yield getattr(self, "_" + kind)()


def history(seed: int, dim: int, rows0: int = 300, steps: int = 30) -> History:
    return History(seed, dim, rows0, steps)


class CompactionHistory(History):
    """1 300 rows; one delete that leaves exactly 1 024 dead rows (the threshold: no compaction); one more (1 025: compaction); one more
    write. Four steps, four checks."""

    def __init__(self, seed: int, dim: int):
        super().__init__(seed, dim, rows0=1300)

    def __iter__(self):
        yield self._step("add", "add", self._new_rows(self.rows0))
        yield self._step("delete_ids", "delete", {"ids": self._pick(1024)})
        yield self._step("delete_ids", "delete", {"ids": self._pick(1)})
        yield self._update_meta()


# ---- the checks ------------------------------------------------------------------------------------------------------------------------
ROW_INCLUDE = ["metadatas", "documents", "distances", "embeddings"]
RANGE = [0.3, 0.45, 2.0]                      # per query: part of its cluster, most of it, every allowed row


def checks(q, centres):
    """-> [(name, fn(collection))]: the twelve families under every filter, with everything each admits in `include`; the grouped and
    counted families on the mixed-kind and the plateau key; one query_filtered with three filters; one refused call per family"""
    out = []
    for name, w, wd in FILTERS:
        f = {"where": w, "where_document": wd}
        out += [
            (f"query/{name}", lambda c, f=f: c.query(query_embeddings=q, n_results=10, include=ROW_INCLUDE, **f)),
            (f"get/{name}", lambda c, f=f: c.get(include=["embeddings", "metadatas", "documents"], **f)),
            (f"count/{name}", lambda c, f=f: c.count(**f)),
            (f"query_groups/{name}", lambda c, f=f: c.query_groups(q, GROUP_KEY, n_groups=5, group_size=3, **f)),
            (f"query_mmr/{name}", lambda c, f=f: c.query_mmr(q, n_results=8, fetch_k=30, lambda_mult=0.5, include=ROW_INCLUDE, **f)),
            (f"query_range/{name}", lambda c, f=f: c.query_range(q, RANGE, max_results=20, include=ROW_INCLUDE, **f)),
            (f"near_duplicates/{name}", lambda c, f=f: c.near_duplicates(0.05, **f)),
            (f"kmeans/{name}", lambda c, f=f: c.kmeans(init=centres, max_iter=4, **f)),
            (f"assign_clusters/{name}", lambda c, f=f: c.assign_clusters(centres, **f)),
            (f"facets/{name}", lambda c, f=f: c.facets("src", **f)),
            (f"query_facets/{name}", lambda c, f=f: c.query_facets(q, "src", RANGE, limit=3, **f)),
        ]
    for key in ("mixed", PLATEAU_KEY):
        out += [
            (f"query_groups/{key}", lambda c, key=key: c.query_groups(q, key, n_groups=6, group_size=2)),
            (f"facets/{key}", lambda c, key=key: c.facets(key)),
            (f"facets/{key}/limit", lambda c, key=key: c.facets(key, where=FILTERS[1][1], limit=4)),
            (f"query_facets/{key}", lambda c, key=key: c.query_facets(q, key, RANGE, limit=4)),
        ]
    three = [x[1] for x in (FILTERS[1], FILTERS[2], FILTERS[4])], [None, FILTERS[3][2], FILTERS[4][2]]
    out.append(("query_filtered/three", lambda c: c.query_filtered(q, three[0], n_results=10, where_documents=three[1], include=ROW_INCLUDE)))
    B = BAD_WHERE
    out += [
        ("refused/query", lambda c: c.query(query_embeddings=q, n_results=10, where=B)),
        ("refused/query_filtered", lambda c: c.query_filtered(q, [None, B, None], n_results=10)),
        ("refused/get", lambda c: c.get(where=B)),
        ("refused/count", lambda c: c.count(where=B)),
        ("refused/query_groups", lambda c: c.query_groups(q, GROUP_KEY, where=B)),
        ("refused/query_mmr", lambda c: c.query_mmr(q, where=B)),
        ("refused/query_range", lambda c: c.query_range(q, 0.5, where=B)),
        ("refused/near_duplicates", lambda c: c.near_duplicates(0.05, where=B)),
        ("refused/kmeans", lambda c: c.kmeans(init=centres, max_iter=1, where=B)),
        ("refused/assign_clusters", lambda c: c.assign_clusters(centres, where=B)),
        ("refused/facets", lambda c: c.facets("src", where=B)),
        ("refused/query_facets", lambda c: c.query_facets(q, "src", 0.5, where=B)),
    ]
    return out


FAMILIES = ("query", "query_filtered", "get", "count", "query_groups", "query_mmr", "query_range", "near_duplicates", "kmeans",
            "assign_clusters", "facets", "query_facets")


class Raised:
    """what a check that raised left behind: equal to another of the same type and message"""

    def __init__(self, e: BaseException):
        self.type, self.message = type(e).__name__, str(e)

    def __repr__(self):
        return f"<raised {self.type}: {self.message}>"


def run(check_list, col, after=None) -> dict:
    out = {}
    for name, fn in check_list:
        try:
            out[name] = fn(col)
        except Exception as e:                                   # noqa: BLE001 - a refusal is an answer like any other
            out[name] = Raised(e)
        if after is not None:
            after(name, col)
    return out


def diff(a, b, at: str = ""):
    """None when a and b are deeply equal, else where they first differ and how"""
    if isinstance(a, Raised) or isinstance(b, Raised):
        ok = isinstance(a, Raised) and isinstance(b, Raised) and (a.type, a.message) == (b.type, b.message)
        return None if ok else f"{at}: {a!r} != {b!r}"
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        if not (isinstance(a, np.ndarray) and isinstance(b, np.ndarray)):
            return f"{at}: {type(a).__name__} != {type(b).__name__}"
        if a.dtype != b.dtype or a.shape != b.shape:
            return f"{at}: {a.dtype}{a.shape} != {b.dtype}{b.shape}"
        if a.tobytes() != b.tobytes():
            j = int(np.flatnonzero(np.frombuffer(a.tobytes(), np.uint8) != np.frombuffer(b.tobytes(), np.uint8))[0]) // a.itemsize
            return f"{at}: arrays differ from element {j} on: {a.reshape(-1)[j]!r} != {b.reshape(-1)[j]!r}"
        return None
    if type(a) is not type(b):
        return f"{at}: {type(a).__name__} {a!r} != {type(b).__name__} {b!r}"
    if isinstance(a, dict):
        if list(a) != list(b):
            return f"{at}: keys {list(a)} != {list(b)}"
        for k in a:
            d = diff(a[k], b[k], f"{at}[{k!r}]")
            if d:
                return d
        return None
    if isinstance(a, (list, tuple)):
        if len(a) != len(b):
            return f"{at}: {len(a)} entries != {len(b)}"
        for j, (x, y) in enumerate(zip(a, b)):
            d = diff(x, y, f"{at}[{j}]")
            if d:
                return d
        return None
    if isinstance(a, float):
        return None if struct.pack("<d", a) == struct.pack("<d", b) else f"{at}: {a!r} != {b!r}"
    return None if a == b else f"{at}: {a!r} != {b!r}"


def same(a, b) -> bool:
    return diff(a, b) is None


# ---- the replay ------------------------------------------------------------------------------------------------------------------------
class Hooks:
    """what a test wants to see of a replay; every method may assert"""

    def opened(self, col):
        """a live collection was created or reopened"""

    def before_write(self, col, step):
        pass

    def after_write(self, col, step):
        pass

    def after_check(self, name, col):
        pass

    def after_checks(self, col, step, live: dict):
        pass


def release(col):
    """give back what a collection holds on a device (the collection is not used again)"""
    col._drop_masks()
    if col._doc_store is not None:
        col._doc_store.close()
        col._doc_store = None
    col._meta_close()
    if col._engine is not None and hasattr(col._engine, "close"):
        col._engine.close()
    col._engine = None


def replay(hist: History, path, live_factory, fresh_factory, hooks: Hooks = None, stop_at_first: bool = False):
    """apply the history to a persistent collection under `path` and compare it with the model's rebuild after EVERY write
    -> (mismatches: [(step number, kind, check name, where and how)], facts: per step {"kind", "edges", "rows", "dead", "live",
    "matched": {filter: rows it matches}})"""
    from rag_dpo_amd.collection import PersistentClient
    hooks = hooks or Hooks()
    check_list = checks(hist.q, hist.centres)
    skip = tuple(name for name, _ in DELIBERATE)
    client = PersistentClient(str(path), engine_factory=live_factory)
    col = client.create_collection("history")
    hooks.opened(col)
    mismatches, facts = [], []
    try:
        for t, step in enumerate(hist):
            hooks.before_write(col, step)
            try:
                if step["op"] == "reload":
                    if step["kind"] == "reload_persist":
                        client.persist()
                    release(col)
                    client = PersistentClient(str(path), engine_factory=live_factory)
                    col = client.get_collection("history")
                    hooks.opened(col)
                else:
                    getattr(col, step["op"])(**step["kwargs"])
            except Exception as e:                               # noqa: BLE001 - the model took the write: the live collection must too
                mismatches.append((t, step["kind"], "the write itself", repr(Raised(e))))
                break
            hooks.after_write(col, step)
            if (col._rows, col._n_dead) != (hist.phys, hist.dead):
                mismatches.append((t, step["kind"], "physical state", f"rows, dead = {(col._rows, col._n_dead)}, the generator follows {(hist.phys, hist.dead)}"))
            live = run(check_list, col, hooks.after_check)
            fresh_col = hist.model.fresh(fresh_factory)
            try:
                fresh = run(check_list, fresh_col)
            finally:
                release(fresh_col)
            for name, _ in check_list:
                if skip and name.startswith(skip):
                    continue
                d = diff(live[name], fresh[name], name)
                if d:
                    mismatches.append((t, step["kind"], name, d))
            facts.append({"kind": step["kind"], "edges": step["edges"], "rows": col._rows, "dead": col._n_dead, "live": len(hist.model),
                          "matched": {f[0]: fresh[f"count/{f[0]}"] for f in FILTERS}})
            hooks.after_checks(col, step, live)
            if mismatches and stop_at_first:
                break
    finally:
        release(col)
    return mismatches, facts
