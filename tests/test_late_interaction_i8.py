"""CPU: the int8 token-vector store (rag_dpo_amd/late_interaction.py) — quantize_model against a restatement in Python
floats and fractions, maxsim_i8_model against the fp64 MaxSim of the fp16 vectors within quant_bound, MultiVectorStore(dtype="int8")
through its writes and files, and the rerankers on a CPU int8 store (which score through the model)."""
import json
import os
import struct
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_late_interaction import DIM, Boost, ScriptedProvider, chunk, ranked, unit16  # noqa: E402

from rag_dpo_amd import late_interaction as LI  # noqa: E402
from rag_dpo_amd.reranker import select_host  # noqa: E402


# ---- quantize_model -------------------------------------------------------------------------------------------------------------------
def f32(x: float) -> float:
    """a Python float rounded once to fp32 (struct rounds to nearest even)"""
    return struct.unpack("f", struct.pack("f", x))[0]


def quantize_restated(row):
    """the rule of the module's docstring with Python floats (fp64) for the arithmetic and fractions for the rounding of the quotient"""
    xs = [float(v) for v in row]
    if any(v != v or v in (float("inf"), float("-inf")) for v in xs) or max(abs(v) for v in xs) == 0.0:
        return [0] * len(xs), 0.0
    scale = f32(max(abs(v) for v in xs) / 127.0)
    codes = []
    for v in xs:
        t = Fraction(v / scale)                    # the fp64 quotient, exactly
        lo = t.numerator // t.denominator
        frac = t - lo
        n = lo + (1 if frac > Fraction(1, 2) or (frac == Fraction(1, 2) and lo % 2) else 0)   # ties to even
        codes.append(max(-127, min(127, n)))
    return codes, scale


def test_quantize_model_equals_the_restatement():
    rng = np.random.default_rng(0)
    rows = [unit16(rng, 1, 32)[0], unit16(rng, 1, 96)[0], (rng.standard_normal(64) * 100).astype(np.float16),
            (rng.standard_normal(32) * 1e-6).astype(np.float16),                                   # fp16 subnormals
            np.full(32, 65504.0, dtype=np.float16), np.asarray([6e-8] + [0.0] * 31, dtype=np.float16)]
    for x in rows:
        c, s = LI.quantize_model(x)
        wc, ws = quantize_restated(x)
        assert c.dtype == np.int8 and s.dtype == np.float32 and c.tolist() == wc and float(s) == ws, (x[:4], float(s), ws)
        assert np.abs(c).max() == 127                                                               # the largest element takes the full range
    many = np.concatenate([unit16(rng, 50, 64), (rng.standard_normal((50, 64)) * 7).astype(np.float16)])
    c, s = LI.quantize_rows_model(many)
    for i in range(len(many)):
        ci, si = LI.quantize_model(many[i])
        assert c[i].tobytes() == ci.tobytes() and s[i].tobytes() == si.tobytes()                   # rows are independent


def tie_row(dim=32):
    """maximum 127 * 2^-10, so scale = 2^-10 exactly; the elements (n + 1/2) * 2^-10 are ties"""
    x = np.zeros(dim, dtype=np.float16)
    x[:6] = np.asarray([127.0, 0.5, 1.5, 2.5, -0.5, -3.5]) * 2.0 ** -10
    return x


def test_the_tie_probe_rounds_to_even():
    c, s = LI.quantize_model(tie_row())
    assert float(s) == 2.0 ** -10
    assert c[:6].tolist() == [127, 0, 2, 2, 0, -4] and not c[6:].any()
    assert np.frombuffer(c.tobytes(), dtype=np.uint8)[4] == 0                                       # -0.5 -> -0.0, stored as 0


def test_zero_and_non_finite_rows_are_zero_rows():
    for bad in (0.0, np.inf, -np.inf, np.nan):
        x = unit16(np.random.default_rng(1), 1, 64)[0]
        if bad == 0.0:
            x[:] = 0
            x[3] = -0.0
        else:
            x[17] = bad
        c, s = LI.quantize_model(x)
        assert not c.any() and s.tobytes() == np.float32(0.0).tobytes(), bad                        # +0.0
    rows = unit16(np.random.default_rng(2), 3, 32)
    rows[1, 5] = np.nan
    c, s = LI.quantize_rows_model(rows)                                                             # a bad row leaves its neighbours alone
    assert not c[1].any() and s[1] == 0 and c[0].tobytes() == LI.quantize_model(rows[0])[0].tobytes() and s[2] == LI.quantize_model(rows[2])[1]


def test_codes_stay_within_127_on_random_rows():
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((10_000, 32)) * np.exp(rng.uniform(-12, 9, size=(10_000, 1)))).astype(np.float16)
    x = x[np.isfinite(x).all(axis=1)]
    c, s = LI.quantize_rows_model(x)
    assert c.min() >= -127 and c.max() <= 127 and (s >= 0).all() and np.isfinite(s).all()
    live = np.abs(x).max(axis=1) > 0
    assert (np.abs(c[live].astype(np.int32)).max(axis=1) == 127).all()
    # |x - s c| <= s / 2 (the premise of quant_bound), up to the rounding of the fp64 quotient
    err = np.abs(x.astype(np.float64) - s.astype(np.float64)[:, None] * c)
    assert (err <= s.astype(np.float64)[:, None] * (0.5 + 2.0 ** -30)).all()


# ---- the score ------------------------------------------------------------------------------------------------------------------------
def maxsim64(q, d):
    """the fp64 MaxSim of the fp16 vectors, not rounded"""
    m = (q.astype(np.float64) @ d.astype(np.float64).T).max(axis=1)
    return float(np.sum(m) / len(m))


def corpus(rng, dim, outliers, n_q=30, n_d=300):
    def rows(n):
        v = rng.standard_normal((n, dim))
        if outliers:
            v[:, rng.choice(dim, size=max(1, dim // 50), replace=False)] *= 10.0                   # 2 % of the dimensions ten times larger
        return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float16)
    q, d = rows(n_q), rows(n_d)
    d[::37] = q[:len(d[::37])]                                                                      # some chunk tokens equal question tokens
    return q, d


def test_pairs_model_restated_with_integers():
    rng = np.random.default_rng(4)
    q, d = corpus(rng, 64, False, 5, 9)
    (cq, sq), (cd, sd) = LI.quantize_rows_model(q), LI.quantize_rows_model(d)
    total = 0.0
    for i in range(5):
        best = -np.inf
        for j in range(9):
            acc = sum(int(a) * int(b) for a, b in zip(cq[i], cd[j]))
            best = max(best, f32(f32(float(acc)) * float(sd[j])))
        total += float(sq[i]) * best
    got = LI.maxsim_i8_model(cq, sq, cd, sd)
    assert got.dtype == np.float32 and float(got) == f32(total / 5)
    # the pairs form, and what is out of range
    q_off = np.array([0, 2, 5], dtype=np.int32)
    start, length = np.array([0, 4, 7, 8], dtype=np.int64), np.array([4, 3, 2, 0], dtype=np.int32)
    out = LI.maxsim_pairs((cq, sq), q_off, (cd, sd), start, length, np.array([0, 1, 2, -1, 0, 1, 0], dtype=np.int32), np.array([0, 1, 0, 0, 4, 2, 3], dtype=np.int64))
    assert out[0] == LI.maxsim_i8_model(cq[:2], sq[:2], cd[:4], sd[:4]) and out[5] == LI.maxsim_i8_model(cq[2:], sq[2:], cd[7:9], sd[7:9])
    assert np.isnan(out[[2, 3, 4, 6]]).all()
    # an all-negative slot scores negative; a zero row in the slot scores +0.0 against it
    qn, dn = np.zeros((2, 32), dtype=np.float16), np.zeros((3, 32), dtype=np.float16)
    qn[:, 0], dn[:, 0] = 1.0, [-0.5, -0.25, -1.0]
    assert LI.maxsim_i8_model(*LI.quantize_rows_model(qn), *LI.quantize_rows_model(dn)) == np.float32(-0.25)
    dn[1] = 0
    z = LI.maxsim_i8_model(*LI.quantize_rows_model(qn), *LI.quantize_rows_model(dn))
    assert z.tobytes() == np.float32(0.0).tobytes()


@pytest.mark.parametrize("outliers", [False, True])
@pytest.mark.parametrize("dim", [32, 128, 1024])
def test_i8_score_lies_within_quant_bound_of_the_fp64_maxsim(dim, outliers):
    rng = np.random.default_rng(dim + outliers)
    q, d = corpus(rng, dim, outliers)
    (cq, sq), (cd, sd) = LI.quantize_rows_model(q), LI.quantize_rows_model(d)
    worst = (0.0, 0.0, 0.0)
    for a, b, n in ((0, 30, 300), (0, 1, 300), (3, 30, 1), (5, 12, 40), (0, 30, 37)):
        got = float(LI.maxsim_i8_model(cq[a:b], sq[a:b], cd[:n], sd[:n]))
        err = abs(got - maxsim64(q[a:b], d[:n]))
        bound = LI.quant_bound(cq[a:b], sq[a:b], cd[:n], sd[:n])
        worst = max(worst, (err / bound, err, bound))
        assert err <= bound, (dim, outliers, a, b, n, err, bound)
    print(f"int8 maxsim dim {dim} outliers {outliers}: worst err/bound {worst[0]:.3g} (err {worst[1]:.3g}, bound {worst[2]:.3g})")


# ---- the store ------------------------------------------------------------------------------------------------------------------------
def holds(st, mats):
    for k, m in mats.items():
        c, s = st.get_codes(k)
        wc, ws = LI.quantize_rows_model(m)
        assert c.dtype == np.int8 and s.dtype == np.float32 and c.tobytes() == wc.tobytes() and s.tobytes() == ws.tobytes(), k
        assert st.get(k).dtype == np.float32 and st.get(k).tobytes() == (wc.astype(np.float32) * ws[:, None]).tobytes()
    return True


def scaled16(rng, n, dim=DIM):
    """unit rows times a row-specific factor: every row has a scale of its own, so a scale that strays from its codes shows"""
    return (unit16(rng, n, dim).astype(np.float32) * np.exp(rng.uniform(-3, 3, size=(n, 1)))).astype(np.float16)


def test_int8_store_keeps_scales_with_codes(tmp_path):
    rng = np.random.default_rng(5)
    st = LI.MultiVectorStore(DIM, "cpu", dtype="int8")
    mats = {f"c{i}": scaled16(rng, n) for i, n in enumerate((3, 1, 7, 2))}
    st.add(list(mats), list(mats.values()))
    assert st.dtype == "int8" and len(st) == 4 and holds(st, mats)
    s = st.stats()
    assert s["dtype"] == "int8" and s["live_tokens"] == 13 and s["bytes"] == 1024 * (DIM + 4) + 4 * (8 + 4)
    assert "dtype" not in LI.MultiVectorStore(DIM).stats()                                           # the default store's stats are unchanged
    mats["c1"] = scaled16(rng, 2)
    st.add(["c1"], (mats["c1"], np.array([0, 2])))                                                   # replace: the slot stays, the old row is dead
    assert st.slots_of(["c1"]).tolist() == [1] and st.stats()["dead_tokens"] == 1 and holds(st, mats)
    st.delete(["c0", "nope"])
    del mats["c0"]
    assert st.stats()["dead_tokens"] == 4 and holds(st, mats)
    st.compact()
    (codes, scales), start, length = st.tables()
    assert codes.shape == (11, DIM) and codes.dtype == np.int8 and scales.shape == (11,) and scales.dtype == np.float32
    assert length.tolist() == [0, 2, 7, 2] and start[1:].tolist() == [0, 2, 9] and holds(st, mats)
    mats["c9"] = scaled16(rng, 4)
    st.add(["c9"], [mats["c9"]])
    assert st.slots_of(["c9"]).tolist() == [0] and holds(st, mats)
    st.add(["c2"], [scaled16(rng, 1)])                                                               # dead 7, live 9 ... then one more replace compacts by itself
    mats["c2"] = scaled16(rng, 1)
    st.add(["c2"], [mats["c2"]])
    mats["c9"] = scaled16(rng, 1)
    st.add(["c9"], [mats["c9"]])
    assert st.stats()["dead_tokens"] == 0 and holds(st, mats)
    # growth past the first reservation moves both arrays
    big = {f"g{i}": scaled16(rng, 300) for i in range(5)}
    st.add(list(big), list(big.values()))
    mats.update(big)
    assert st.stats()["live_tokens"] == 6 + 1500 and holds(st, mats)
    # files
    freed = st.slots_of(["g1"]).tolist()
    st.delete(["g1"])
    del mats["g1"]
    st.save(str(tmp_path / "mv8"))
    assert sorted(os.listdir(tmp_path / "mv8")) == ["codes.npy", "scales.npy", "slots.npy", "store.json"]
    meta = json.load(open(tmp_path / "mv8" / "store.json"))
    assert meta["format"] == 2 and meta["dtype"] == "int8" and meta["dim"] == DIM
    back = LI.MultiVectorStore.load(str(tmp_path / "mv8"), "cpu")
    assert back.dtype == "int8" and back.slots_of(list(mats) + ["g1"]).tolist() == st.slots_of(list(mats) + ["g1"]).tolist() and holds(back, mats)
    back.add(["new"], [scaled16(rng, 1)])
    assert back.slots_of(["new"]).tolist() == freed                                                  # the free slot survived the round trip
    with pytest.raises(ValueError, match="dtype"):
        LI.MultiVectorStore(DIM, dtype="int4")
    with pytest.raises(TypeError):
        LI.MultiVectorStore(DIM).get_codes("x")


def test_to_int8_equals_the_store_built_directly(tmp_path):
    rng = np.random.default_rng(6)
    f16, direct = LI.MultiVectorStore(DIM), LI.MultiVectorStore(DIM, dtype="int8")
    mats = {f"c{i}": scaled16(rng, n) for i, n in enumerate((5, 2, 9, 1, 3))}
    for st in (f16, direct):
        st.add(list(mats), list(mats.values()))
        st.delete(["c1"])
        st.add(["c3"], [mats["c0"][:2]])
    mats["c3"] = mats["c0"][:2]
    del mats["c1"]
    conv = f16.to_int8()
    assert conv.dtype == "int8" and conv.device == f16.device and len(conv) == 4 and holds(conv, mats) and holds(direct, mats)
    ids = list(mats) + ["c1"]
    assert conv.slots_of(ids).tolist() == f16.slots_of(ids).tolist() == direct.slots_of(ids).tolist()
    conv.add(["late"], [scaled16(rng, 2)])
    assert conv.slots_of(["late"]).tolist() == [1] and "late" not in f16                              # the free slot came along; the source is its own store
    assert f16.get("c0").tobytes() == mats["c0"].tobytes()
    with pytest.raises(TypeError):
        conv.to_int8()
    # a format-1 directory still loads, as an fp16 store
    f16.save(str(tmp_path / "mv"))
    assert sorted(os.listdir(tmp_path / "mv")) == ["slots.npy", "store.json", "vecs.npy"]
    assert json.load(open(tmp_path / "mv" / "store.json")) == {"format": 1, "dim": DIM, "ids": f16._ids}
    back = LI.MultiVectorStore.load(str(tmp_path / "mv"))
    assert back.dtype == "float16" and back.get("c2").tobytes() == mats["c2"].tobytes()
    json.dump({"format": 3, "dim": DIM, "ids": []}, open(tmp_path / "mv" / "store.json", "w"))
    with pytest.raises(ValueError, match="unknown format"):
        LI.MultiVectorStore.load(str(tmp_path / "mv"))


def test_add_refuses_non_finite_input_and_changes_nothing():
    rng = np.random.default_rng(7)
    st = LI.MultiVectorStore(DIM, dtype="int8")
    mats = {"a": scaled16(rng, 3), "b": scaled16(rng, 2)}
    st.add(list(mats), list(mats.values()))
    before = (st.stats(), st.tables()[0][0].tobytes(), st.tables()[0][1].tobytes(), st.slots_of(["a", "b", "c"]).tolist())
    for bad in (np.inf, -np.inf, np.nan):
        m = scaled16(rng, 4)
        m[2, 7] = bad
        with pytest.raises(ValueError, match="non-finite"):
            st.add(["a", "c"], [scaled16(rng, 1), m])
        assert (st.stats(), st.tables()[0][0].tobytes(), st.tables()[0][1].tobytes(), st.slots_of(["a", "b", "c"]).tolist()) == before
    assert holds(st, mats)


# ---- the rerankers --------------------------------------------------------------------------------------------------------------------
def expected_i8(rr, prov, query, chunks, top_k, boosts=None, min_score=float("-inf")):
    cq, sq = LI.quantize_rows_model(prov.vectors(query))
    scores = [LI.maxsim_i8_model(cq, sq, *LI.quantize_rows_model(prov.vectors(rr.chunk_text(c)))) for c in chunks]
    order, final, count = select_host(scores, boosts, top_k, min_score)
    return [(chunks[i].chunk_id, final[i], i) for i in order[:count]]


def test_cpu_reranker_on_an_int8_store_equals_the_model_pair_by_pair():
    chunks = [chunk(i, " ".join(f"mot{(i * 7 + j) % 23}" for j in range(3 + i % 5)), heading="Titre" if i % 3 == 0 else "",
                    tags="cookies" if i % 4 == 0 else "") for i in range(12)]
    prov = ScriptedProvider()
    store = LI.MultiVectorStore(DIM, dtype="int8")
    rr = LI.LateInteractionReranker(prov, store)
    rr.index_chunks(chunks[::2])                                                                      # the odd ones go through the scratch arena
    assert store.get_codes("chunk_4")[0].tobytes() == LI.quantize_rows_model(prov.vectors(rr.chunk_text(chunks[4])))[0].tobytes()
    before = store.stats()
    q = "durée de conservation des cookies"
    out = rr.rerank(q, chunks, top_k=12)
    assert ranked(out) == expected_i8(rr, prov, q, chunks, 12) and len(out) == 12                      # stored or not, a chunk scores the same
    assert rr.last_rerank_stats["path"] == "maxsim-i8-model" and rr.last_rerank_stats["encoded"] == 6 and rr._model.calls == 2
    assert store.stats() == before
    boosts = [Boost().topic_boost(["cookies"], c.metadata["rgpd_topics"]) for c in chunks]
    assert ranked(rr.rerank(q, chunks, top_k=8, topic_matcher=Boost(), question_topics=["cookies"])) == expected_i8(rr, prov, q, chunks, 8, boosts)
    queries, lists = [q, "registre", q], [chunks[:8], [], chunks[3:4]]
    got = rr.rerank_batch(queries, lists, top_k=4)
    assert [ranked(g) for g in got] == [expected_i8(rr, prov, qq, cc, 4) if cc else [] for qq, cc in zip(queries, lists)]
    # the scores differ from the fp16 store's, by no more than the bound
    f16 = LI.LateInteractionReranker(prov, LI.MultiVectorStore(DIM))
    a = {r.chunk_id: r.rerank_score for r in f16.rerank(q, chunks, top_k=12)}
    cq, sq = LI.quantize_rows_model(prov.vectors(q))
    for r in out:
        cd, sd = LI.quantize_rows_model(prov.vectors(rr.chunk_text(chunks[r.original_rank])))
        assert abs(r.rerank_score - a[r.chunk_id]) <= LI.quant_bound(cq, sq, cd, sd) + 2.0 ** -23


def test_m3_reranker_takes_an_int8_store():
    from test_m3 import ScriptedM3, build_sources, make_chunks, text_of
    from rag_dpo_amd import m3 as M3
    prov = ScriptedM3()
    chunks = make_chunks(12)
    col, ix, f16 = build_sources(prov, chunks, "cpu", stored=lambda i: i % 3 != 1)                    # a third goes through the scratch arena
    store = f16.to_int8()
    q = "durée de conservation des cookies"
    cq, sq = LI.quantize_rows_model(prov.vectors(q))
    s, r, _ = col._engine.search(prov.dense(q)[None, :], col.count())
    dense_of = dict(zip(r[0].tolist(), s[0]))
    for w in (M3.DEFAULT_WEIGHTS, (0, 0, 1), (1, 0.3, 0)):
        rr = M3.M3Reranker(prov, col, ix, store, weights=w)
        out = rr.rerank(q, chunks, top_k=12)
        finals = []
        for i, c in enumerate(chunks):                                                                # the definition, pair by pair: only the colbert component's source differs
            dense = np.asarray([dense_of[col.rows_of([c.chunk_id])[0]]], dtype=np.float32) if w[0] else None
            d_terms = prov.terms(text_of(c)) if i % 3 != 1 else (np.zeros(0, np.int32), np.zeros(0, np.float16))
            sparse = np.asarray([M3.LX.score_model(*prov.terms(q), *d_terms)], dtype=np.float64) if w[1] else None
            colbert = np.asarray([LI.maxsim_i8_model(cq, sq, *LI.quantize_rows_model(prov.vectors(text_of(c))))], dtype=np.float32) if w[2] else None
            finals.append(M3.combine_model(dense, sparse, colbert, w)[1][0])
        order, final, count = select_host(finals, None, 12, float("-inf"))
        assert ranked(out) == [(chunks[i].chunk_id, final[i], i) for i in order[:count]], w
        assert rr.last_rerank_stats["path"] == "m3-model" and rr.last_rerank_stats["encoded"] == (4 if w[2] else 0)
        if w[2]:
            assert rr._model._maxsim.path == "maxsim-i8-model" and rr._model.last["colbert"].dtype == np.float32
