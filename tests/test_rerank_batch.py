"""CPU: CrossEncoderReranker.rerank_batch, DenseRetriever.retrieve_reranked_batch and the packing TopicMatcher.topic_boosts_device_batch
uploads. On the CPU rerank_batch is the loop of rerank; the golden fixture of the reference's own rerank
(tests/golden/reranker_golden.json) is run through it in batches, one per top_k of the fixture (rerank_batch takes one top_k for all
its questions), each case under a question of its own so that one scripted model (a question's k-th pair -> its k-th score) serves them all.
The helpers here also drive the same batches on the GPU (tests/test_gpu_rerank_batch.py)."""
import os
import sys
import zlib

import numpy as np
import pytest

from rag_dpo_amd import reranker as RR
from rag_dpo_amd.retriever import documents_from_ranked_chunks

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import reranker_world as W  # noqa: E402
import topic_model as M  # noqa: E402
from test_reranker import GOLDEN, case_chunks  # noqa: E402


class TextModel:
    """a model with only predict(): the k-th pair of a question within a call -> that question's k-th scripted float32 score (the
    fixture repeats chunks within a case under different scores: the text alone does not name the score); a question listed in
    `raising` raises"""

    def __init__(self, table, raising=()):
        self.table, self.raising, self.calls = dict(table), set(raising), []

    def predict(self, pairs, batch_size=32, show_progress_bar=True):
        self.calls.append(len(pairs))
        if any(p[0] in self.raising for p in pairs):
            raise RuntimeError("scripted model failure")
        seen, out = {}, []
        for q, _ in pairs:
            k = seen[q] = seen.get(q, -1) + 1
            out.append(self.table[q][k])
        return np.asarray(out, dtype=np.float32)


class TableMatcher:
    """the boosts the reference's TopicMatcher returned, keyed by (topics, tags): only topic_boost, the per-candidate host path"""

    def __init__(self, table):
        self.table = table

    def topic_boost(self, question_topics, chunk_tags_str):
        return self.table[(tuple(question_topics), chunk_tags_str)]


def golden_batches():
    """-> [(top_k, [(case, gold, question)])]: the fixture's cases grouped by top_k, the cases whose model raises in batches of their
    own (one raising pair sends its whole device call through the loop, which would hide the batched path from the others)"""
    groups = {}
    for i, (case, gold) in enumerate(zip(W.cases(), GOLDEN["cases"])):
        groups.setdefault((case["top_k"], bool(case["raises"])), []).append((case, gold, f"{W.QUERY} [{i}]"))
    for (top_k, raises), members in list(groups.items()):           # a raising batch takes a healthy neighbour along
        if raises and (top_k, False) in groups:
            members.append(groups[(top_k, False)][0])
    return [(k[0], v) for k, v in sorted(groups.items(), key=lambda kv: (kv[0][0], kv[0][1]))]


def golden_world(reranker):
    """the scripted model and matcher of ALL fixture cases: (model, matcher)"""
    scores, raising, boosts = {}, set(), {}
    for i, (case, gold) in enumerate(zip(W.cases(), GOLDEN["cases"])):
        scores[f"{W.QUERY} [{i}]"] = list(case["scores"])
        if case["raises"]:
            raising.add(f"{W.QUERY} [{i}]")
        for topics, tags, b in gold["boosts"] or []:
            assert boosts.setdefault((tuple(topics), tags), float(b)) == float(b)
    return TextModel(scores, raising), TableMatcher(boosts)


def check_golden_batches(device):
    seen = 0
    for top_k, members in golden_batches():
        r = RR.CrossEncoderReranker(device=device, min_score=0.08)
        r._model, matcher = golden_world(r)
        out = r.rerank_batch([q for _, _, q in members], [case_chunks(c) for c, _, _ in members], top_k=top_k, topic_matcher=matcher,
                             question_topics=[c["topics"] for c, _, _ in members])
        assert len(out) == len(members)
        for (case, gold, _), got in zip(members, out):
            seen += 1
            if "raises" in gold:                                      # documented difference: the reference's log line raises
                assert got == [], case["name"]
                continue
            chunks = case_chunks(case)
            assert [{"chunk_id": x.chunk_id, "rerank_score": repr(float(x.rerank_score)), "original_rank": x.original_rank,
                     "document_path": x.document_path, "text_is_input": x.text == chunks[x.original_rank].text} for x in got] == gold["result"], case["name"]
            assert all(type(x.rerank_score) is float and type(x.original_rank) is int for x in got)
            docs = documents_from_ranked_chunks(got)
            assert [{"document_path": d.document_path, "avg_similarity": repr(float(d.avg_similarity)), "primary_nature": d.primary_nature,
                     "chunks": [[c.chunk_id, repr(float(c.hybrid_score)), repr(float(c.distance)), c.chunk_nature, c.chunk_index, c.confidence]
                                for c in d.chunks]} for d in docs] == gold["documents"], case["name"]
    assert seen >= len(GOLDEN["cases"])
    return seen


def ranked_values(ranked):
    return [(x.chunk_id, x.text, x.document_path, np.float64(x.rerank_score).tobytes(), x.original_rank, sorted(x.metadata.items())) for x in ranked]


def test_golden_cases_in_batches_on_cpu():
    assert check_golden_batches("cpu") >= 22
    kinds = [(k, [c["name"] for c, _, _ in m]) for k, m in golden_batches()]
    assert any(len(names) >= 5 and "n_0" in names for _, names in kinds)           # an empty candidate list inside a batch


def test_rerank_batch_on_cpu_equals_the_loop_and_validates():
    r = RR.CrossEncoderReranker(device="cpu", min_score=0.08)
    r._model, matcher = golden_world(r)
    members = [m for k, ms in golden_batches() if k == 8 and not any(c["raises"] for c, _, _ in ms) for m in ms]
    queries, chunks, topics = [q for _, _, q in members], [case_chunks(c) for c, _, _ in members], [c["topics"] for c, _, _ in members]
    assert any(t for t in topics) and any(t is None for t in topics) and any(not c for c in chunks)
    got = r.rerank_batch(queries, chunks, top_k=8, topic_matcher=matcher, question_topics=topics)
    want = [r.rerank(q, c, top_k=8, topic_matcher=matcher, question_topics=t) for q, c, t in zip(queries, chunks, topics)]
    assert [ranked_values(g) for g in got] == [ranked_values(w) for w in want] and sum(len(g) for g in got) > 10
    assert r.rerank_batch([], []) == []
    assert r.rerank_batch(queries, chunks, top_k=8) == [r.rerank(q, c, top_k=8) for q, c in zip(queries, chunks)]   # question_topics=None
    with pytest.raises(ValueError, match="candidate lists"):
        r.rerank_batch(queries, chunks[:-1])
    with pytest.raises(ValueError, match="question_topics"):
        r.rerank_batch(queries, chunks, topic_matcher=matcher, question_topics=topics[:-1])
    assert RR.MAX_BATCH_PAIRS == 65536


def test_retrieve_reranked_batch_on_a_host_collection_with_a_reranker_without_rerank_batch():
    from rag_dpo_amd.retriever import DenseRetriever, RetrievedDocument

    rng = np.random.default_rng(9)
    n, d = 120, 16
    emb = rng.standard_normal((n, d)).astype(np.float32)
    emb /= np.linalg.norm(emb, axis=1, keepdims=True)
    ids = [f"chunk_{i}" for i in range(n)]
    metas = [{"document_path": f"doc_{i % 11}", "chunk_nature": ["GUIDE", "DOCTRINE"][i % 2], "chunk_index": i // 11,
              "rgpd_topics": "cookies" if i % 5 == 0 else ""} for i in range(n)]

    class HostCollection:
        """collection.query on numpy: cosine distances, `where` on chunk_nature"""

        def query(self, query_embeddings, n_results, where=None, include=None):
            out = {"ids": [], "documents": [], "metadatas": [], "distances": []}
            for q in query_embeddings:
                q = np.asarray(q, dtype=np.float32)
                dist = 1.0 - emb @ (q / np.linalg.norm(q))
                rows = [i for i in np.argsort(dist, kind="stable") if where is None or metas[i]["chunk_nature"] == where["chunk_nature"]][:n_results]
                out["ids"].append([ids[i] for i in rows])
                out["documents"].append([f"texte {i} conservation" for i in rows])
                out["metadatas"].append([metas[i] for i in rows])
                out["distances"].append([float(dist[i]) for i in rows])
            return out

    class Provider:
        def embed(self, texts):
            return [list(np.random.default_rng(zlib.crc32(t.encode())).standard_normal(d)) for t in texts]

    class LoopOnly:
        """rerank() only: scores from the text, the reference's boost"""
        calls = 0

        def rerank(self, query, chunks, top_k=8, topic_matcher=None, question_topics=None):
            LoopOnly.calls += 1
            r = RR.CrossEncoderReranker(device="cpu")
            r._model = type("M", (), {"predict": staticmethod(lambda pairs, batch_size=32, show_progress_bar=True: np.asarray(
                [(zlib.crc32((p[0] + p[1]).encode()) % 1000) / 1000.0 for p in pairs], dtype=np.float32))})()
            return r.rerank(query, chunks, top_k=top_k, topic_matcher=topic_matcher, question_topics=question_topics)

    class Boost:
        def topic_boost(self, topics, tags):
            return 0.15 if tags == "cookies" else 0.0

    ret = DenseRetriever(HostCollection(), Provider())
    queries = ["durée de conservation", "cookies et traceurs", "registre"]
    wheres = [None, {"chunk_nature": "GUIDE"}, {"chunk_nature": "ABSENT"}]
    topics = [["cookies"], None, ["cookies"]]
    got = ret.retrieve_reranked_batch(queries, LoopOnly(), n_candidates=40, top_k=10, where_filter=wheres, topic_matcher=Boost(), question_topics=topics)
    assert LoopOnly.calls == 2                                                      # the question without candidates never reaches the reranker
    want = [ret.retrieve_reranked(q, LoopOnly(), n_candidates=40, top_k=10, where_filter=w, topic_matcher=Boost(), question_topics=t)
            for q, w, t in zip(queries, wheres, topics)]
    assert got == want and got[2] == [] and all(isinstance(x, RetrievedDocument) for g in got for x in g)
    assert sum(len(x.chunks) for x in got[0]) == 10 and sum(len(x.chunks) for x in got[1]) == 10
    cpu = RR.CrossEncoderReranker(device="cpu")                                     # a reranker WITH rerank_batch (the loop, on the CPU): the same documents
    cpu._model = type("M", (), {"predict": staticmethod(lambda pairs, batch_size=32, show_progress_bar=True: np.asarray(
        [(zlib.crc32((p[0] + p[1]).encode()) % 1000) / 1000.0 for p in pairs], dtype=np.float32))})()
    assert ret.retrieve_reranked_batch(queries, cpu, n_candidates=40, top_k=10, where_filter=wheres, topic_matcher=Boost(), question_topics=topics) == want
    with pytest.raises(ValueError, match="question_topics"):
        ret.retrieve_reranked_batch(queries, cpu, question_topics=[None])


def test_plan_packing_of_a_batch_replays_to_the_single_question_results():
    """pack_plans (what topic_boosts_device_batch uploads) against a numpy restatement of the replay: every question's slice of the
    packed arrays, replayed by tests/topic_model.py, gives what the question's own plan gives; offsets run on, indices stay local"""
    from rag_dpo_amd import _lib as L
    from rag_dpo_amd.topics import _Plan, pack_plans

    rng = np.random.default_rng(12)
    vocab = [a + b for a in "bcdfglmnprst" for b in "aeiou"]
    dim = 24
    vec = {w: (lambda v: (v / np.linalg.norm(v)).astype(np.float32))(rng.standard_normal(dim) + 1.5) for w in vocab}
    slots = {w: i for i, w in enumerate(vocab)}
    table = np.stack([vec[w] for w in vocab])
    questions = []
    for T, n in ((3, 7), (0, 4), (2, 0), (32, 9), (1, 1)):
        topics = [str(t) for t in rng.choice(vocab, T)]
        tags = [", ".join(str(t) for t in rng.choice(vocab, int(rng.integers(0, 5)))) for _ in range(n)]
        if n > 2:
            tags[1] = topics[-1].upper() + ", " + vocab[0] if topics else tags[1]    # an exact pair ignoring case
            tags[2] = ""                                                             # a candidate without tags
        questions.append((topics, tags))
    questions[0][1][3] = "inconnu, " + questions[0][1][3]                            # a tag without an embedding: slot -1
    plans = [_Plan(t, c) for t, c in questions]
    p = pack_plans(plans, lambda s: slots.get(s, -1))
    nq = len(plans)
    assert p["cand_off"].tolist() == [0, 7, 11, 11, 20, 21] and p["cand_off"].dtype == np.int32
    assert p["topic_off"].tolist() == [0, 3, 3, 5, 37, 38] and p["sim_off"].dtype == np.int64 and p["pair_off"].dtype == np.int64
    assert p["sim_off"].tolist() == np.concatenate([[0], np.cumsum([len(pl.topics) * len(pl.tags) for pl in plans])]).tolist()
    assert len(p["pair_off"]) == p["cand_off"][-1] + 1 and p["pair_off"][0] == 0 and p["pair_off"][-1] == len(p["pairs"])
    assert (np.diff(p["pair_off"]) >= 0).all() and -1 in p["tag_slots"]
    unpack = lambda w: (int(w) & 31, int(np.uint32(w)) >> 8, bool((int(w) >> 7) & 1))   # noqa: E731  (include/rdx.h RDX_TOPIC_PAIR)
    assert L.topic_pair(5, 77, True) == (77 << 8) | 128 | 5
    some_boost = False
    for q, (plan, (topics, tags)) in enumerate(zip(plans, questions)):
        ts = p["topic_slots"][p["topic_off"][q]:p["topic_off"][q + 1]].tolist()
        us = p["tag_slots"][p["tag_off"][q]:p["tag_off"][q + 1]].tolist()
        lo, hi = int(p["cand_off"][q]), int(p["cand_off"][q + 1])
        off = p["pair_off"][lo:hi + 1]
        words = [unpack(w) for w in p["pairs"][int(off[0]):int(off[-1])]]
        assert all(t < max(1, len(ts)) and u < max(1, len(us)) for t, u, _ in words)                 # local indices
        assert words == [tuple(w) for w in plan.pairs] and (off - off[0]).tolist() == plan.offsets
        got = M.kernel_model(table, ts, us, (off - off[0]).tolist(), words, 0.65)
        want = M.boosts_for_strings(vec, topics, tags, 0.65)
        assert got == want, q
        some_boost |= any(b > 0 for b in got[0])
    assert some_boost
