"""Cost of the topic boost in front of a rerank: one question, 40 candidates x 3 tags, 3 topics (the reference's rerank_candidates,
src/rag/pipeline.py:128; at most 3 tags per chunk, src/utils/rgpd_topics.py:131). BGE-M3's architecture for the tags (XLM-R-large,
random-init fp16, hashing tokenizer) and bge-reranker-v2-m3's for the pairs.

Three ways to the 40 boosts, each timed alone and as CrossEncoderReranker.rerank(top_k=10) end to end:
  per_tag_cold   a matcher that works as the reference's class does against this provider: one embed([text]) per string it has not
                 seen, np.dot of the cached float64 arrays per (topic, tag); every string of the question is new
  batched_cold   rag_dpo_amd.topics.TopicMatcher, every string new: one embed_device batch, rdx_topic_boost
  warm           both, every string seen before
Cold repetitions use fresh strings each time. Reported: ms per call (median, min). The run ends itself after --limit seconds.

    python tools/topic_boost_bench.py [--reps 7] [--warm-reps 30] [--limit 300] [--out profiles/topics/topic_boost_bench.json]
"""
import argparse
import json
import os
import signal
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from rag_dpo_amd.embedding_provider import EmbeddingProvider
from rag_dpo_amd.reranker import CrossEncoderReranker
from rag_dpo_amd.retriever import RetrievedChunk
from rag_dpo_amd.topics import TopicMatcher

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warm-reps", type=int, default=30)
ap.add_argument("--limit", type=int, default=300)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topics", "topic_boost_bench.json"))
args = ap.parse_args()
signal.alarm(args.limit)                                   # the tool's own time limit: SIGALRM ends the process

N_CAND, N_TAGS, N_TOPICS, TOP_K = 40, 3, 3, 10
VOCAB = [a + b + c for a in "bcdfglmnprst" for b in "aeiou" for c in "nrst"]
rng = np.random.default_rng(2026)
QUERY = " ".join(rng.choice(VOCAB, 12))


class PerTagMatcher:
    """the reference's way: a dict of float64 arrays filled by one embed([text]) per miss, np.dot per pair, the same loops"""

    def __init__(self, provider):
        self.provider, self.cache = provider, {}

    def vec(self, text):
        if text not in self.cache:
            self.cache[text] = np.array(self.provider.embed([text])[0])
        return self.cache[text]

    def topic_boost(self, question_topics, chunk_tags_str, threshold=0.65):
        tags = [t.strip() for t in chunk_tags_str.split(",") if t.strip()]
        best = 0.0
        for topic in question_topics:
            for tag in tags:
                if topic.lower() == tag.lower():
                    best = 1.0
                    break
                sim = float(np.dot(self.vec(topic), self.vec(tag)))
                if sim > best:
                    best = sim
            if best >= 1.0:
                break
        return 0.0 if best < threshold else 0.15 * (best - threshold) / (1.0 - threshold)


def question(salt):
    """3 topics and 40 x 3 tags from a pool of 100 strings of one to three words; `salt` makes every string new"""
    g = np.random.default_rng(1000 + salt)
    pool = [" ".join(g.choice(VOCAB, int(g.integers(1, 4)))) + f" {salt}" for _ in range(100)]
    topics = [" ".join(g.choice(VOCAB, 2)) + f" {salt}" for _ in range(N_TOPICS)]
    tags = [", ".join(pool[int(i)] for i in g.integers(0, len(pool), N_TAGS)) for _ in range(N_CAND)]
    return topics, tags


def chunks_for(tags):
    return [RetrievedChunk(chunk_id=f"c{i}", text=" ".join(rng.choice(VOCAB, 230)), document_path=f"doc{i % 9}", chunk_nature="GUIDE",
                           chunk_index=i, confidence="high", distance=0.3, metadata={"rgpd_topics": t}) for i, t in enumerate(tags)]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def summary(ms):
    return {"ms_median": round(statistics.median(ms), 3), "ms_min": round(min(ms), 3), "reps": len(ms)}


provider = EmbeddingProvider(model_name="random-init:xlm-roberta-large", device="cuda", dtype=torch.float16).load()
reranker = CrossEncoderReranker("random-init:xlm-roberta-large", device="cuda", dtype=torch.float16, min_score=0.0)
reranker._load_model()
ours, theirs = TopicMatcher(provider), PerTagMatcher(provider)
topics0, tags0 = question(0)
chunks0 = chunks_for(tags0)
for _ in range(3):                                           # warm-up: kernels, graphs, pinned buffers, the question-0 strings
    ours.topic_boosts(topics0, tags0)
    [theirs.topic_boost(topics0, t) for t in tags0]
    reranker.rerank(QUERY, chunks0, top_k=TOP_K, topic_matcher=ours, question_topics=topics0)
    reranker.rerank(QUERY, chunks0, top_k=TOP_K, topic_matcher=theirs, question_topics=topics0)

res = {"boosts": {}, "rerank": {}}
cold = {"per_tag_cold": [], "batched_cold": [], "rerank_per_tag_cold": [], "rerank_batched_cold": []}
distinct = []
agree = []
for rep in range(1, args.reps + 1):
    ta, ga = question(4 * rep)
    distinct.append(len(set(ta + [t.strip() for s in ga for t in s.split(",")])))
    ms, a = timed(lambda: [theirs.topic_boost(ta, t) for t in ga])
    cold["per_tag_cold"].append(ms)
    tb, gb = question(4 * rep + 1)
    ms, _ = timed(lambda: ours.topic_boosts_device(tb, gb))
    cold["batched_cold"].append(ms)
    agree.append(float(np.abs(np.asarray(ours.topic_boosts(ta, ga)) - np.asarray(a)).max()))   # same strings, both matchers (a sanity figure)
    tc, gc = question(4 * rep + 2)
    cc = chunks_for(gc)
    ms, _ = timed(lambda: reranker.rerank(QUERY, cc, top_k=TOP_K, topic_matcher=theirs, question_topics=tc))
    cold["rerank_per_tag_cold"].append(ms)
    td, gd = question(4 * rep + 3)
    cd = chunks_for(gd)
    ms, _ = timed(lambda: reranker.rerank(QUERY, cd, top_k=TOP_K, topic_matcher=ours, question_topics=td))
    cold["rerank_batched_cold"].append(ms)
warm = {"per_tag_warm": [], "batched_warm_device": [], "batched_warm_host_list": [], "rerank_per_tag_warm": [], "rerank_batched_warm": [],
        "rerank_no_boost": []}
for rep in range(args.warm_reps):
    warm["per_tag_warm"].append(timed(lambda: [theirs.topic_boost(topics0, t) for t in tags0])[0])
    warm["batched_warm_device"].append(timed(lambda: ours.topic_boosts_device(topics0, tags0))[0])
    warm["batched_warm_host_list"].append(timed(lambda: ours.topic_boosts(topics0, tags0))[0])
    warm["rerank_per_tag_warm"].append(timed(lambda: reranker.rerank(QUERY, chunks0, top_k=TOP_K, topic_matcher=theirs, question_topics=topics0))[0])
    warm["rerank_batched_warm"].append(timed(lambda: reranker.rerank(QUERY, chunks0, top_k=TOP_K, topic_matcher=ours, question_topics=topics0))[0])
    warm["rerank_no_boost"].append(timed(lambda: reranker.rerank(QUERY, chunks0, top_k=TOP_K))[0])
for k, v in {**cold, **warm}.items():
    res["rerank" if k.startswith("rerank") else "boosts"][k] = summary(v)
    print(k, json.dumps(summary(v)), flush=True)
out = {"workload": f"one question: {N_CAND} candidates x {N_TAGS} tags, {N_TOPICS} topics, ~{int(statistics.median(distinct))} distinct strings when cold; "
                   "tags embedded by XLM-R-large (BGE-M3 shape), pairs scored by XLM-R-large (bge-reranker-v2-m3 shape, ~250 tokens a pair), "
                   "random-init fp16, hashing tokenizer; wall ms per call with a device synchronise at both ends",
       "device": torch.cuda.get_device_name(0), "max_abs_boost_difference_between_the_two_matchers": max(agree), **res}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
print("wrote", args.out)
