"""GPU: rdx_topic_boost against the numpy restatement of its arithmetic (tests/topic_model.py), bit for bit, across dims, candidate
counts, topic counts and tags per candidate, with the edge inputs inside those shapes; its writes; its repeatability; TopicMatcher on
a GPU provider and the reranker's device-boost path end to end."""
import logging
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import topic_model as M  # noqa: E402

pytestmark = pytest.mark.gpu

T32 = float(np.float32(0.65))
SENTINEL, GUARD = -7.0, 8
NAN_ROW, NEG_ROW, ULP_A, ULP_B, THR_ROW, E1_ROW, FIRST_RANDOM = 0, 2, 3, 4, 5, 6, 7
ROWS = 48


def lib():
    from rag_dpo_amd import _lib
    return _lib, _lib.load()


def make_table(dim, seed):
    """rows around a common direction (cosines on both sides of the threshold), and the edge rows: NaN, -e1, two identical rows whose
    dot product is above 1.0 (1 + 2^-52 from dim 2 on), [fp32(0.65), 0, ...] and e1"""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal(dim)
    x = base[None, :] / np.linalg.norm(base) + 0.73 * rng.standard_normal((ROWS, dim)) / dim ** 0.5
    t = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    e1 = np.zeros(dim, dtype=np.float32)
    e1[0] = 1.0
    t[NAN_ROW] = np.nan
    t[1] = e1
    t[NEG_ROW] = -e1
    t[ULP_A] = e1
    t[ULP_A, 0] = np.nextafter(np.float32(1.0), np.float32(2.0)) if dim == 1 else 1.0
    if dim > 1:
        t[ULP_A, 1] = 2.0 ** -26
    t[ULP_B] = t[ULP_A]
    t[THR_ROW] = e1 * np.float32(0.65)
    t[E1_ROW] = e1
    return t


def make_inputs(dim, n, T, K, variant):
    rng = np.random.default_rng(1000 * dim + 10 * n + T + K + 7919 * variant)
    table = make_table(dim, dim)
    topic_slots = rng.integers(FIRST_RANDOM, ROWS, T).tolist()
    fixed = [E1_ROW, ULP_A, NAN_ROW, -1, ROWS + 5, NEG_ROW] if T > 1 else [[E1_ROW, ULP_A, NAN_ROW, FIRST_RANDOM][variant % 4]]
    topic_slots[:len(fixed)] = fixed[:T]
    U = max(8, min(60, n * max(K, 1)))
    tag_slots = rng.integers(FIRST_RANDOM, ROWS, U).tolist()
    tag_slots[:8] = [ULP_B, THR_ROW, NEG_ROW, NAN_ROW, -1, ROWS, E1_ROW, ULP_A]
    ulp_t = 1 if T > 1 else 0
    crafted = [[(0, 1, False)],                                                  # e1 . [fp32(0.65), 0, ...]: exactly the threshold
               [(0, 2, False), (0, 3, False), (0, 4, False), (0, 5, False)],     # negative, NaN, no slot, a slot past the table
               [(ulp_t, 0, False), (ulp_t, 1, True)],                            # above 1.0, then an exact pair under the same topic
               [(ulp_t, 0, False), (ulp_t, 2, False)]]                           # above 1.0 stays
    if T > 1:
        crafted += [[(1, 0, False), (1, 2, False), (2, 1, True)],                # above 1.0, then an exact pair under a LATER topic: not reached
                    [(0, 5, True), (1, 0, False)],                               # an exact pair first: the pair above 1.0 is not reached
                    [(0, 6, False), (0, 1, False), (1, 0, False)]]               # exactly 1.0 ends the topics as well
    offsets, pairs = [0], []
    for c in range(n):
        if K > 0 and c < len(crafted):
            pairs += crafted[(c + variant) % len(crafted)]
        elif K > 0 and rng.uniform() > 0.1:                                      # (one candidate in ten has no pairs)
            tags = rng.integers(0, U, K).tolist()
            exact_at = int(rng.integers(0, 40 * T * K))                          # seldom inside the list: pairs behind it must not count
            pairs += [(t, u, t * K + j == exact_at) for t in range(T) for j, u in enumerate(tags)]
        offsets.append(len(pairs))
    return table, topic_slots, tag_slots, offsets, pairs


def run_kernel(table, topic_slots, tag_slots, offsets, pairs, threshold, stream=None, table_dev=None):
    L, lib_ = lib()
    n, T, U = len(offsets) - 1, len(topic_slots), len(tag_slots)
    dev = "cuda"
    tab = table_dev if table_dev is not None else torch.from_numpy(table).to(dev)
    words = np.asarray(list(topic_slots) + list(tag_slots) + list(offsets) + [L.topic_pair(t, u, e) for t, u, e in pairs] + [0], dtype=np.int32)
    d = torch.from_numpy(words).to(dev)
    sims = torch.full((max(1, T * U) + GUARD,), SENTINEL, dtype=torch.float64, device=dev)
    boosts = torch.full((n + GUARD,), SENTINEL, dtype=torch.float64, device=dev)
    best = torch.full((n + GUARD,), SENTINEL, dtype=torch.float64, device=dev)
    st = stream or torch.cuda.current_stream()
    p = d.data_ptr()
    rc = lib_.rdx_topic_boost(0, tab.data_ptr(), tab.shape[0], tab.shape[1], p, T, p + 4 * T, U, p + 4 * (T + U), p + 4 * (T + U + n + 1),
                              len(pairs), n, float(threshold), 0.15, sims.data_ptr(), boosts.data_ptr(), best.data_ptr(), st.cuda_stream)
    assert rc == 0, L.last_error()
    st.synchronize()
    return boosts.cpu().numpy(), best.cpu().numpy(), sims.cpu().numpy()


DIMS = (1, 63, 64, 65, 512, 513, 1024, 4096)    # 512: one full round of TOPIC_KU loads a lane; 513: a second round of one element; 1024: two; 4096: eight
# (n, topics, tags per candidate, variants): every n, topic count and tag count of the grid, the largest of each together once per
# dim class; n = 1 runs four variants so that each crafted pair list lands on its only candidate
SHAPES = [(1, 1, 0, 1), (1, 1, 1, 4), (1, 32, 3, 4), (1, 32, 64, 2), (40, 1, 1, 2), (40, 1, 3, 2), (40, 32, 3, 2), (40, 32, 64, 1), (40, 1, 64, 1),
          (1024, 1, 0, 1), (1024, 1, 1, 1), (1024, 32, 1, 1), (1024, 1, 3, 1), (1024, 32, 3, 1)]


@pytest.mark.parametrize("dim", DIMS)
def test_kernel_equals_the_model_bit_for_bit(dim):
    shapes = SHAPES + ([(1024, 32, 64, 1)] if dim == 65 else [(1024, 1, 64, 1)])         # the full limits once (2 M pairs to replay)
    table_dev = torch.from_numpy(make_table(dim, dim)).cuda()
    seen = set()
    for n, T, K, variants in shapes:
        for v in range(variants):
            table, ts, us, offsets, pairs = make_inputs(dim, n, T, K, v)
            boosts, best, sims = run_kernel(table, ts, us, offsets, pairs, T32, table_dev=table_dev)
            want_b, want_s = M.kernel_model(table, ts, us, offsets, pairs, T32)
            where = (dim, n, T, K, v)
            assert (boosts[n:] == SENTINEL).all() and (best[n:] == SENTINEL).all() and (sims[T * len(us):] == SENTINEL).all(), where   # guard words
            assert not (boosts[:n] == SENTINEL).any() and not (best[:n] == SENTINEL).any(), where                       # every entry written
            np.testing.assert_array_equal(best[:n].view(np.int64), np.asarray(want_s, dtype=np.float64).view(np.int64), err_msg=str(where))
            np.testing.assert_array_equal(boosts[:n].view(np.int64), np.asarray(want_b, dtype=np.float64).view(np.int64), err_msg=str(where))
            assert (boosts[:n].view(np.int64)[boosts[:n] == 0] == 0).all(), where        # a non-match is +0.0: sign bit clear
            assert not np.isnan(best[:n]).any()
            b = best[:n]
            seen |= {"zero"} if (b == 0).any() else set()
            seen |= {"threshold"} if (b == T32).any() else set()
            seen |= {"above one"} if (b > 1.0).any() else set()
            seen |= {"one"} if (b == 1.0).any() else set()
            seen |= {"between"} if ((b > T32) & (b < 1.0)).any() else set()
            seen |= {"below"} if ((b > 0) & (b < T32)).any() else set()
    # (in one dimension every unit row is +1 or -1: no best similarity lies strictly between 0 and the threshold)
    assert seen == {"zero", "threshold", "above one", "one", "between"} | ({"below"} if dim > 1 else set()), (dim, seen)


def test_edge_pairs_give_the_documented_results():
    table, ts, us, offsets, pairs = make_inputs(64, 40, 32, 3, 0)
    boosts, best, _ = run_kernel(table, ts, us, offsets, pairs, T32)
    ulp = 1.0 + 2.0 ** -52
    assert best[:7].tolist() == [T32, 0.0, 1.0, ulp, ulp, 1.0, 1.0]
    assert boosts[0] == 0.0 and boosts[1] == 0.0 and boosts[2] == 0.15 * (1.0 - T32) / (1.0 - T32) and boosts[3] == 0.15 * (ulp - T32) / (1.0 - T32)


def test_two_calls_and_a_second_stream_give_identical_bits():
    table, ts, us, offsets, pairs = make_inputs(1024, 40, 32, 3, 0)
    a = run_kernel(table, ts, us, offsets, pairs, 0.65)
    b = run_kernel(table, ts, us, offsets, pairs, 0.65)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = run_kernel(table, ts, us, offsets, pairs, 0.65, stream=side)
    torch.cuda.current_stream().wait_stream(side)
    for x, y, z in zip(a, b, c):
        assert np.array_equal(x.view(np.int64), y.view(np.int64)) and np.array_equal(x.view(np.int64), z.view(np.int64))
    assert (a[0][:40] > 0).any() and (a[0][:40] == 0).any()


def test_invalid_arguments_on_device():
    L, lib_ = lib()
    x = torch.zeros(4096, dtype=torch.float64, device="cuda")
    p, st = x.data_ptr(), torch.cuda.current_stream().cuda_stream
    ok = dict(rows=4, dim=8, T=1, U=1, P=1, n=1)
    for bad in (dict(n=0), dict(n=1025), dict(dim=0), dict(dim=4097), dict(T=33), dict(T=-1), dict(U=-1), dict(U=65537), dict(P=-1), dict(P=2049), dict(rows=-1)):
        a = dict(ok, **bad)
        rc = lib_.rdx_topic_boost(0, p, a["rows"], a["dim"], p, a["T"], p, a["U"], p, p, a["P"], a["n"], 0.65, 0.15, p, p, p, st)
        assert rc == L.RDX_ERR_INVALID and L.last_error(), bad
    assert lib_.rdx_topic_boost(0, p, 4, 8, p, 1, p, 1, p, p, 1, 1, 0.65, 0.15, None, p, p, st) == L.RDX_ERR_INVALID      # sims missing
    assert lib_.rdx_topic_boost(0, p, 4, 8, p, 1, p, 1, p + 2, p, 1, 1, 0.65, 0.15, p, p, p, st) == L.RDX_ERR_INVALID    # misaligned
    assert lib_.rdx_topic_boost(0, p, 4, 8, p, 1, p, 1, p, p, 1, 1, 0.65, 0.15, p, p + 4, p, st) == L.RDX_ERR_INVALID
    assert "misaligned" in L.last_error()
    # no table at all (a matcher without embeddings): every similarity is +0.0, exact pairs still count
    d = torch.tensor([-1, -1, 0, 1, 2, L.topic_pair(0, 0, False), L.topic_pair(0, 0, True)], dtype=torch.int32, device="cuda")
    q = d.data_ptr()
    out = torch.full((4,), SENTINEL, dtype=torch.float64, device="cuda")
    assert lib_.rdx_topic_boost(0, None, 0, 8, q, 1, q + 4, 1, q + 8, q + 20, 2, 2, 0.65, 0.15, p, out.data_ptr(), None, st) == 0, L.last_error()
    assert out.cpu().tolist() == [0.0, 0.15, SENTINEL, SENTINEL]


# ---- TopicMatcher and the reranker on the GPU ------------------------------------------------------------------------------------

def question40():
    rng = np.random.default_rng(5)
    vocab = [a + b + c for a in "bcdfglmnprst" for b in "aeiou" for c in "nrst"]
    pool = [" ".join(rng.choice(vocab, int(rng.integers(1, 4)))) for _ in range(30)]
    topics = [" ".join(rng.choice(vocab, 2)) for _ in range(3)]
    tags = [", ".join(pool[int(i)] for i in rng.integers(0, 30, int(rng.integers(0, 4)))) for _ in range(40)]
    tags[4] = topics[1].upper() + ", " + pool[0]                                  # an exact match ignoring case
    return topics, tags, pool


@pytest.fixture(scope="module")
def provider():
    from rag_dpo_amd.embedding_provider import EmbeddingProvider
    return EmbeddingProvider(model_name="random-init:mid", device="cuda:0", dtype=torch.float16).load()


def test_matcher_on_a_gpu_provider_one_batched_embed_device_and_host_equal_bits(provider):
    from rag_dpo_amd.topics import TopicMatcher
    topics, tags, pool = question40()
    calls = []

    class Spy:
        device = provider.device

        def embed_device(self, texts):
            calls.append(list(texts))
            return provider.embed_device(texts)

        def embed(self, texts):
            raise AssertionError("embed_device is there: embed() is not to be called")

    tm = TopicMatcher(Spy())
    assert tm.on_gpu and tm.device == torch.device("cuda", 0)
    dev = tm.topic_boosts_device(topics, tags)
    assert dev.is_cuda and dev.dtype == torch.float64 and dev.shape == (40,)
    distinct = list(dict.fromkeys(topics + [t.strip() for s in tags for t in s.split(",") if t.strip()]))
    assert len(calls) == 1 and sorted(calls[0]) == sorted(distinct) and len(distinct) > 20          # one batch for the cold question
    got = dev.cpu().numpy()
    plan = tm._plan(topics, tags)
    host, host_best = tm._host(plan, 0.65)
    assert np.array_equal(got.view(np.int64), np.asarray(host, dtype=np.float64).view(np.int64))
    _, kernel_best = tm._device(plan, 0.65, want_best=True)
    assert np.array_equal(kernel_best.cpu().numpy().view(np.int64), np.asarray(host_best, dtype=np.float64).view(np.int64))
    vec = {t: tm._get_embedding(t) for t in distinct}
    want, _ = M.boosts_for_strings(vec, topics, tags, 0.65)                         # the independent model on the table's rows
    assert np.array_equal(got.view(np.int64), np.asarray(want, dtype=np.float64).view(np.int64))
    assert got[4] == 0.15 and (got == 0).any()
    assert tm.topic_boosts(topics, tags) == got.tolist() and tm.topic_boost(topics, tags[7]) == got[7]
    assert len(calls) == 1 and tm.stats["device_calls"] >= 3                        # warm: nothing more is embedded
    # the rows are the provider's embed() rows: embed_device's raw rows normalised by the same kernel
    ref = np.asarray(provider.embed(calls[0]), dtype=np.float32)                    # (the same batch: the same forward)
    assert np.array_equal(np.stack([vec[t] for t in calls[0]]), ref)
    norms = np.linalg.norm(np.stack(list(vec.values())).astype(np.float64), axis=1)
    assert np.abs(norms - 1).max() < 1e-6


def test_rerank_with_device_boosts_equals_rerank_with_the_same_host_boosts(provider, caplog):
    from rag_dpo_amd import reranker as RR
    from rag_dpo_amd.retriever import RetrievedChunk
    from rag_dpo_amd.topics import TopicMatcher
    topics, tags, pool = question40()
    rng = np.random.default_rng(6)
    vocab = [a + b for a in "abcdefghijklmnopqrstuvwxyz" for b in "aeiou"]
    chunks = [RetrievedChunk(f"c{i}", " ".join(rng.choice(vocab, int(rng.integers(8, 60)))), f"doc{i % 7}", "GUIDE", i, "high", 0.5,
                             {"rgpd_topics": tags[i]}) for i in range(40)]
    tm = TopicMatcher(provider)
    boosts = tm.topic_boosts(topics, tags)

    class HostMatcher:                                   # only topic_boost: the per-candidate host path, scripted with the same boosts
        def __init__(self):
            self.i = 0

        def topic_boost(self, question_topics, chunk_tags_str):
            assert chunk_tags_str == tags[self.i]
            self.i += 1
            return boosts[self.i - 1]

    r = RR.CrossEncoderReranker("random-init:mid", device="cuda:0", dtype=torch.float16, min_score=0.0)
    assert r._boosts_on_device(tm, 40) and not r._boosts_on_device(HostMatcher(), 40)
    before = dict(tm.stats)
    with caplog.at_level(logging.INFO, logger="rag_dpo_amd.reranker"):
        a = r.rerank("question sur les cookies", chunks, top_k=10, topic_matcher=tm, question_topics=topics)
    hits = sum(1 for b in boosts if b > 0)
    assert 0 < hits < 40 and f"topic boost applied to {hits}/40 chunks" in caplog.text
    assert tm.stats["device_calls"] == before["device_calls"] + 1 and tm.stats["host_calls"] == before["host_calls"]
    b = r.rerank("question sur les cookies", chunks, top_k=10, topic_matcher=HostMatcher(), question_topics=topics)
    plain = r.rerank("question sur les cookies", chunks, top_k=10)
    assert len(a) == 10 and [x.chunk_id for x in a] == [x.chunk_id for x in b] and [x.original_rank for x in a] == [x.original_rank for x in b]
    assert np.array_equal(np.asarray([x.rerank_score for x in a]).view(np.int64), np.asarray([x.rerank_score for x in b]).view(np.int64))
    assert [x.chunk_id for x in plain] != [x.chunk_id for x in a] or [x.rerank_score for x in plain] != [x.rerank_score for x in a]
    cpu_tm = TopicMatcher(None)
    assert not r._boosts_on_device(cpu_tm, 40)           # a matcher on another device takes the per-candidate path
