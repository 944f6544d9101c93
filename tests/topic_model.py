"""A numpy restatement of rdx_topic_boost's arithmetic (rag_dpo_amd/csrc/topic_kernel.hpp), written from its documentation and
independent of the product code (which never imports it): the similarity's summation order element by element, and the pair replay
as the reference's two loops (src/utils/rgpd_topics.py:203-222). Python floats and numpy float64 are IEEE doubles: every addition
below rounds exactly as the kernel's does, and the products of two fp32 values are exact."""
import numpy as np

MAX_BOOST = 0.15


def similarities(table, topic_slots, tag_slots):
    """fp64 [T][U]: for every (topic, tag) 64 partial sums, element i added to partial i % 64 in ascending i, then the butterfly
    part[l] += part[l ^ m] for m = 32, 16, 8, 4, 2, 1 and partial 0 is the result; a slot outside the table gives +0.0"""
    table = np.asarray(table, dtype=np.float32)
    rows = table.shape[0]
    T, U = len(topic_slots), len(tag_slots)
    out = np.zeros((T, U), dtype=np.float64)
    ok_t = [t for t in range(T) if 0 <= topic_slots[t] < rows]
    ok_u = [u for u in range(U) if 0 <= tag_slots[u] < rows]
    if not ok_t or not ok_u:
        return out
    a = table[[topic_slots[t] for t in ok_t]].astype(np.float64)           # [t][dim]
    b = table[[tag_slots[u] for u in ok_u]].astype(np.float64)             # [u][dim]
    part = np.zeros((len(ok_t), len(ok_u), 64), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(table.shape[1]):                                     # one element at a time, in the kernel's order
            part[:, :, i % 64] = part[:, :, i % 64] + np.multiply.outer(a[:, i], b[:, i])
        for m in (32, 16, 8, 4, 2, 1):
            part = np.stack([part[:, :, l] + part[:, :, l ^ m] for l in range(64)], axis=2)
    out[np.ix_(ok_t, ok_u)] = part[:, :, 0]
    return out


def boost_of(best, threshold, max_boost=MAX_BOOST):
    best, threshold = float(best), float(threshold)
    if best < threshold:
        return 0.0
    return max_boost * (best - threshold) / (1.0 - threshold)


def replay(sims, offsets, pairs, threshold, max_boost=MAX_BOOST):
    """pairs: (topic index, tag index, exact) in loop order; -> (boosts, best similarities) as Python floats"""
    boosts, bests = [], []
    T, U = sims.shape if sims is not None else (0, 0)
    for c in range(len(offsets) - 1):
        best, prev = 0.0, None
        for t, u, exact in pairs[offsets[c]:offsets[c + 1]]:
            if prev is not None and t != prev and best >= 1.0:
                break
            prev = t
            if exact:
                best = 1.0
                break
            sim = float(sims[t, u]) if t < T and u < U else 0.0
            if sim > best:
                best = sim
        bests.append(best)
        boosts.append(boost_of(best, threshold, max_boost))
    return boosts, bests


def kernel_model(table, topic_slots, tag_slots, offsets, pairs, threshold, max_boost=MAX_BOOST):
    sims = similarities(table, topic_slots, tag_slots) if len(topic_slots) and len(tag_slots) else np.zeros((0, 0))
    return replay(sims, offsets, pairs, threshold, max_boost)


def boosts_for_strings(vectors, question_topics, chunk_tags_strs, threshold=0.65):
    """the reference's topic_boost for every candidate, its loops as written there, the similarity in the kernel's order.
    vectors: text -> fp32 vector, a text without an entry has no embedding. -> (boosts, best similarities)"""
    texts = list(vectors)
    slot = {t: i for i, t in enumerate(texts)}
    table = np.asarray([vectors[t] for t in texts], dtype=np.float32) if texts else np.zeros((0, 1), dtype=np.float32)
    memo = {}

    def sim(x, y):
        if (x, y) not in memo:
            memo[(x, y)] = float(similarities(table, [slot.get(x, -1)], [slot.get(y, -1)])[0, 0])
        return memo[(x, y)]

    boosts, bests = [], []
    for s in chunk_tags_strs:
        best = 0.0
        tags = [t.strip() for t in s.split(',') if t.strip()] if (question_topics and s) else []
        for topic in (question_topics if tags else []):
            for tag in tags:
                if topic.lower() == tag.lower():
                    best = 1.0
                    break
                v = sim(topic, tag)
                if v > best:
                    best = v
            if best >= 1.0:
                break
        bests.append(best)
        boosts.append(boost_of(best, threshold))
    return boosts, bests
