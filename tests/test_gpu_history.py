"""Random write histories on the device, replayed against a from-scratch rebuild on the CPU (tests/history_model.py states the model,
tests/test_history.py runs the same histories with both sides on the CPU).

Live is a Collection on librdx with every `where` evaluated in HBM (_WHERE_DEVICE_MIN_ROWS = 0): its mask cache holds resident masks,
its MetaStore follows the columns by a low-water mark, its DocStore is appended to, replaced in and compacted, its group tables have a
copy in HBM. The rebuild is made after every write on the test-only oracle engine, which shares nothing with the device. Everything
is compared with history_model.diff: there is no tolerance.

Two of the device's caches hide their own failures by design (_where_device answers on the host after a RuntimeError, _docs_write
drops the store after any exception), so after every check step the test also asserts that neither happened."""
import pytest

import history_model as H
from oracle_engine import factory as oracle_factory

pytestmark = pytest.mark.gpu
SEEDS = (1, 2)                          # tests/test_history.py's


def host_counters(col):
    g = col.group_stats
    return {"kmeans": col.kmeans_stats["host"], "facets": col.facet_stats["host"], "counts": col.facet_stats["calls_host"],
            "range": col.range_stats["host"], "dedup": col.dedup_stats["host"],
            "groups": g["queries"] - g["proven_first_fetch"] - g["second_fetch"]}    # a query of the device ladder is one or the other


class OnDevice(H.Hooks):
    """the assertions that keep a replay from passing on a silent fallback, and the count of the paths query() took"""

    def __init__(self, force_fast: bool = False):
        self.force_fast = force_fast
        self.paths = []                 # rdx_search_stats.path of every query() check that had rows to search
        self.steps = 0

    def opened(self, col):
        col._WHERE_DEVICE_MIN_ROWS = 0
        self.armed = False
        self.fresh_object = True        # a new Collection: its stores and counters start anew

    def before_write(self, col, step):
        self.doc_store = None if self.fresh_object else col._doc_store
        self.host = {k: 0 for k in host_counters(col)} if self.fresh_object else host_counters(col)

    def after_write(self, col, step):
        if step["op"] == "reload":
            self.doc_store, self.host = None, {k: 0 for k in self.host}
        self.fresh_object = False
        if self.force_fast and not self.armed and col._engine is not None:
            col._engine.set_option("force_fast", 1)            # the MFMA scan and the exact re-score, whatever the size
            self.armed = True

    def after_check(self, name, col):
        if name.startswith("query/") and not col._no_rows():
            self.paths.append(col._engine.last_stats()["path"])

    def after_checks(self, col, step, live):
        from rag_dpo_amd.engine import DocStore, MetaStore, ResidentMask
        self.steps += 1
        assert host_counters(col) == self.host, (step["kind"], host_counters(col), self.host)
        assert all(isinstance(r, ResidentMask) for _, r in col._mask_cache.values())
        if col._no_rows():              # nothing was asked of the device
            return
        assert len(col._mask_cache) >= 4, list(col._mask_cache)
        assert isinstance(col._meta_store, MetaStore) and {"src", "n"} <= set(col._meta_res)
        assert all(r == col._rows for _, r in col._meta_res.values())          # every resident column is up to date
        assert isinstance(col._doc_store, DocStore) and len(col._doc_store) == col._rows
        if self.doc_store is not None:                                          # the store followed the write: it was not dropped and rebuilt
            assert col._doc_store is self.doc_store, step["kind"]


def report(mismatches):
    return f"{len(mismatches)} mismatches, the first: " + "; ".join(f"step {t} ({kind}) {d[:300]}" for t, kind, _, d in mismatches[:5])


@pytest.mark.parametrize("seed", SEEDS)
def test_a_history_on_the_exact_path(oracle, tmp_path, seed):
    """dim 64: at these sizes every search is the exact scan"""
    watch = OnDevice()
    hist = H.history(seed, 64)
    mismatches, facts = H.replay(hist, tmp_path, None, oracle_factory, watch)
    assert not mismatches, report(mismatches)
    assert len(facts) == 31 and watch.steps == 31
    assert watch.paths and set(watch.paths) == {1}


@pytest.mark.parametrize("seed", SEEDS)
def test_a_history_behind_the_mfma_scan(oracle, tmp_path, seed):
    """dim 260 (a ragged last k-step) with force_fast, set after the first add and again after each reload: query() runs the MFMA scan
    and the exact re-score. With force_fast the plan takes that path from one row on, so every query() that had rows is counted."""
    watch = OnDevice(force_fast=True)
    hist = H.history(seed, 260)
    mismatches, facts = H.replay(hist, tmp_path, None, oracle_factory, watch)
    assert not mismatches, report(mismatches)
    assert len(facts) == 31 and watch.steps == 31
    assert len(watch.paths) >= 5 * 28 and 2 * watch.paths.count(0) >= len(watch.paths), watch.paths


def test_the_compaction_history_on_the_device(oracle, tmp_path):
    """1 024 dead rows (no compaction), 1 025 (the engine, the DocStore and the columns are compacted), one more write"""
    watch = OnDevice()
    seen = []
    real = watch.after_write
    watch.after_write = lambda col, step: (seen.append((col._rows, col._n_dead, col._meta_store is None)), real(col, step))
    mismatches, facts = H.replay(H.CompactionHistory(3, 64), tmp_path, None, oracle_factory, watch)
    assert not mismatches, report(mismatches)
    assert len(facts) == 4 and watch.steps == 4
    assert seen[1] == (1300, 1024, False) and seen[2] == (275, 0, True) and seen[3][:2] == (275, 0)


# ---- defects of the device's own copies, planted: the replay must report them, or it would also pass on a stale copy -------------------
class DeviceWhere(H.Hooks):
    def opened(self, col):
        col._WHERE_DEVICE_MIN_ROWS = 0


def plant_low_water_mark(mp):
    """_set_meta leaves the MetaStore's marks where they were: rows changed in place are not uploaded again"""
    from rag_dpo_amd.collection import Collection
    real = Collection._set_meta

    def set_meta(self, row, meta, replace):
        marks = {k: ent[1] for k, ent in self._meta_res.items()}
        real(self, row, meta, replace)
        for k, r in marks.items():
            self._meta_res[k][1] = r
    mp.setattr(Collection, "_set_meta", set_meta)


def plant_doc_replace(mp):
    """update(documents=) does not reach the DocStore"""
    from rag_dpo_amd.engine import DocStore
    mp.setattr(DocStore, "replace", lambda self, rows, docs: None)


@pytest.mark.parametrize("plant,kinds,names", [(plant_low_water_mark, ("update_meta", "upsert"), ("str", "num", "both", "three", "limit")),
                                               (plant_doc_replace, ("update_doc", "upsert"), ("doc", "both", "three"))])
def test_a_stale_device_copy_is_reported(oracle, tmp_path, monkeypatch, plant, kinds, names):
    plant(monkeypatch)
    mismatches, _ = H.replay(H.history(1, 64), tmp_path, None, oracle_factory, DeviceWhere(), stop_at_first=True)
    assert mismatches and mismatches[0][1] in kinds, mismatches[:3]
    assert all(m[2].split("/")[-1] in names for m in mismatches), [m[2] for m in mismatches]
