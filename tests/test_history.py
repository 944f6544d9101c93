"""Random write histories replayed against a from-scratch rebuild, on the CPU (tests/history_model.py states the model).

Live and rebuilt collection both run on the test-only oracle engine: what is under test is Collection's own state between calls (the
mask cache, the per-row metadata cache, the group tables keyed on write_count, the journal and the snapshot, the compaction), compared
after every single write. tests/test_gpu_history.py replays the same histories against the device's copies."""
import pytest

import history_model as H
from oracle_engine import factory as oracle_factory
from rag_dpo_amd.collection import Collection

SEEDS = (1, 2)
DIMS = (64, 260)
_replays = {}


def replayed(tmp_path_factory, seed, dim):
    """one replay per (seed, dim), shared by the tests that read it"""
    if (seed, dim) not in _replays:
        hist = H.history(seed, dim)
        _replays[seed, dim] = hist, *H.replay(hist, tmp_path_factory.mktemp(f"h{seed}_{dim}"), oracle_factory, oracle_factory)
    return _replays[seed, dim]


def test_the_model_filters_as_the_collection_does(oracle):
    """the model's own restatement of `where` / `where_document` (its delete) against Collection.get, on every kind of value"""
    hist = H.history(0, 8, rows0=120)
    next(iter(hist))
    col = hist.model.fresh(oracle_factory)
    col.update(ids=["r3", "r4", "r5"], metadatas=[{"n": 3.5}, {"n": "four"}, {"mixed": None, "src": "epsilon"}])
    hist.model.update(ids=["r3", "r4", "r5"], metadatas=[{"n": 3.5}, {"n": "four"}, {"mixed": None, "src": "epsilon"}])
    wheres = [w for _, w, _ in H.FILTERS] + [{"mixed": 1}, {"mixed": True}, {"mixed": 1.0}, {"mixed": {"$ne": "1"}}, {"n": {"$lt": 3.6}},
                                             {"n": {"$in": [4, 5, 6]}}, {"n": {"$nin": ["four"]}}, {"absent": {"$ne": 1}}, {"absent": 1},
                                             {"$or": [{"src": "epsilon"}, {"$and": [{"n": {"$gt": 100}}, {"mixed": {"$lte": 2}}]}]}]
    docs = [None, {"$contains": "cookies"}, {"$not_contains": "7 about"}, {"$or": [{"$contains": "in beta"}, {"$and": [{"$contains": "1"}, {"$not_contains": "2"}]}]}]
    for w in wheres:
        for wd in docs:
            got = hist.model.matching(w, wd)
            assert got == col.get(where=w, where_document=wd, include=[])["ids"], (w, wd)
    assert 0 < len(hist.model.matching(wheres[-1])) < 120


def test_same_compares_bits_types_and_refusals():
    import numpy as np
    a = {"x": [1.0, np.float32(2)], "y": np.zeros((2, 3), np.float32)}
    assert H.same(a, {"x": [1.0, np.float32(2)], "y": np.zeros((2, 3), np.float32)})
    assert not H.same(0.0, -0.0) and H.same(float("nan"), float("nan"))
    assert not H.same([1], [True]) and not H.same([1], [1.0]) and not H.same([1], (1,))
    assert not H.same(np.zeros((0, 4), np.float32), np.zeros((0, 0), np.float32))
    assert not H.same(np.zeros(2, np.float32), np.zeros(2, np.int32))
    assert not H.same(np.array([0.0], np.float32), np.array([-0.0], np.float32))
    assert not H.same({"a": 1, "b": 2}, {"b": 2, "a": 1})                      # a result's keys come in one order
    r = lambda e: H.Raised(e)                                                   # noqa: E731
    assert H.same(r(ValueError("x")), r(ValueError("x"))) and not H.same(r(ValueError("x")), r(ValueError("y")))
    assert not H.same(r(ValueError("x")), r(TypeError("x"))) and not H.same(r(ValueError("x")), None)
    assert "['y']" in H.diff(a, {"x": [1.0, np.float32(2)], "y": np.ones((2, 3), np.float32)})


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("seed", SEEDS)
def test_a_history_answers_as_its_rebuild(oracle, tmp_path_factory, seed, dim):
    hist, mismatches, facts = replayed(tmp_path_factory, seed, dim)
    assert len(facts) == 31 and hist.serial > 300                              # the first add and 30 steps, each checked
    assert mismatches == []


def test_the_compaction_history(oracle, tmp_path):
    hist = H.CompactionHistory(3, 64)
    seen = []

    class Watch(H.Hooks):
        def after_write(self, col, step):
            seen.append((col._rows, col._n_dead, col.write_count))

    mismatches, facts = H.replay(hist, tmp_path, oracle_factory, oracle_factory, Watch())
    assert mismatches == [] and len(facts) == 4
    assert seen[1][:2] == (1300, 1024)                                          # exactly at the threshold: no compaction
    assert seen[2][:2] == (1300 - 1025, 0) and seen[2][2] == seen[1][2] + 2     # one more: the delete and the compaction
    assert seen[3][:2] == (275, 0)
    for name, _, _ in H.FILTERS[1:]:
        assert all(0 < f["matched"][name] < f["live"] for f in facts), name


def test_the_histories_hold_every_write_kind_and_edge(oracle, tmp_path_factory):
    """from the generator's own log and the counts of the replays: by construction, not by luck"""
    for seed in SEEDS:
        for dim in DIMS:
            hist, _, facts = replayed(tmp_path_factory, seed, dim)
            kinds = {s["kind"] for s in hist.log}
            edges = {e for s in hist.log for e in s["edges"]}
            assert kinds == set(H.WRITE_KINDS), (seed, dim, set(H.WRITE_KINDS) - kinds)
            assert edges == set(H.EDGES), (seed, dim, set(H.EDGES) - edges)
            order = [s["kind"] for s in hist.log]
            assert order.index("reload_journal") < order.index("reload_persist")     # the first reload had the journal alone
            for t, s in enumerate(hist.log):
                if "delete_all" in s["edges"]:                                    # every live row gone, a check step, then rows again
                    assert facts[t]["live"] == 0 and facts[t]["rows"] > 0 and "add_after_empty" in hist.log[t + 1]["edges"]
                if "cross32" in s["edges"]:
                    assert facts[t - 1]["rows"] // 32 < (facts[t]["rows"] - 1) // 32
                if "whole_group" in s["edges"] or "first_of_value" in s["edges"]:
                    assert facts[t]["live"] < facts[t - 1]["live"]
                if s["kind"] == "add":
                    assert 1 <= len(s["kwargs"]["ids"]) <= 40 or t == 0
            for name, _, _ in H.FILTERS[1:]:                                      # every filter has had something to decide
                assert any(0 < f["matched"][name] < f["live"] for f in facts), (seed, dim, name)
    assert [name.split("/")[0] for name, _ in H.checks(None, None) if name.startswith("refused/")] == ["refused"] * 12
    families = {name.split("/")[0] for name, _ in H.checks(None, None)} - {"refused"}
    assert families == set(H.FAMILIES)
    for fam in set(H.FAMILIES) - {"query_filtered"}:
        assert {f"{fam}/{f[0]}" for f in H.FILTERS} <= {name for name, _ in H.checks(None, None)}


# ---- planted defects: each must make the replay report a mismatch ------------------------------------------------------------------
def plant_drop_masks(mp):
    mp.setattr(Collection, "_drop_masks", lambda self: None)


def plant_write_count(mp):
    mp.setattr(Collection, "write_count", property(lambda self: 0))


def plant_meta_cache(mp):
    real = Collection._set_meta

    def set_meta(self, row, meta, replace):
        had = row in self._meta_cache
        kept = self._meta_cache.get(row)
        real(self, row, meta, replace)
        if had:
            self._meta_cache[row] = kept
    mp.setattr(Collection, "_set_meta", set_meta)


def plant_wd_masks(mp):
    real_update, real_evict = Collection.update, Collection._evict_mask

    def update(self, ids, embeddings=None, metadatas=None, documents=None, **kw):
        self._planted = documents is not None and metadatas is None
        try:
            return real_update(self, ids, embeddings, metadatas, documents, **kw)
        finally:
            self._planted = False

    def evict(self, key):
        if not (getattr(self, "_planted", False) and key.startswith("wd:")):
            real_evict(self, key)
    mp.setattr(Collection, "update", update)
    mp.setattr(Collection, "_evict_mask", evict)


def plant_compact(mp):
    real = Collection._compact

    def compact(self):
        kept = dict(self._meta_cache)
        real(self)
        self._meta_cache.update(kept)
    mp.setattr(Collection, "_compact", compact)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("plant", [plant_drop_masks, plant_write_count, plant_meta_cache, plant_wd_masks])
def test_a_planted_defect_is_reported(oracle, tmp_path, monkeypatch, plant, seed):
    plant(monkeypatch)
    mismatches, _ = H.replay(H.history(seed, 64), tmp_path, oracle_factory, oracle_factory, stop_at_first=True)
    assert mismatches, plant.__name__
    if plant is plant_wd_masks:                                                  # found at the write it belongs to, by a family that reads masks
        assert mismatches[0][1] == "update_doc" and all("doc" in m[2] or "both" in m[2] or "three" in m[2] for m in mismatches)


def test_a_compaction_that_keeps_the_metadata_cache_is_reported(oracle, tmp_path, monkeypatch):
    plant_compact(monkeypatch)
    mismatches, _ = H.replay(H.CompactionHistory(3, 64), tmp_path, oracle_factory, oracle_factory, stop_at_first=True)
    assert mismatches and mismatches[0][0] == 2 and "metadatas" in mismatches[0][3]
