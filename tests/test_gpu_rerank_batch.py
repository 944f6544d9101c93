"""GPU: the reranker for a batch of questions. rdx_rerank_head_rows_f16, rdx_topic_boost_batch and
rdx_rerank_select_batch, called through ctypes, against the single-question entry points bit for bit (and against the Python
restatements those are pinned to); their writes and argument checks; then rerank_batch and retrieve_reranked_batch against the loop
of rerank / retrieve_reranked, and the fused path against transformers' fp32 module forward with test_gpu_reranker's tolerance.

The shape arrays (cand_off, topic_off, tag_off, sim_off) are pinned host memory, as include/rdx.h asks."""
import copy
import os
import sys
import zlib

import numpy as np
import pytest
import torch

from rag_dpo_amd import reranker as RR

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import topic_model as M  # noqa: E402
from test_gpu_reranker import head, head_reference, make_head, module_cls32, pairs_of_lengths, select, spread_head_along_pairs  # noqa: E402
from test_gpu_topics import ROWS, make_table, run_kernel  # noqa: E402
from test_rerank_batch import check_golden_batches, golden_batches, golden_world, ranked_values  # noqa: E402
from test_reranker import case_chunks  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 8
SENT_I, SENT_F = -7, -7.0


def lib():
    from rag_dpo_amd import _lib
    return _lib, _lib.load()


def pinned(values, dtype):
    return torch.tensor(list(values), dtype=dtype).pin_memory()


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.int64)


# ---- head ----------------------------------------------------------------------------------------------------------------------------

def head_rows(cls, wd, bd, wo, bo):
    """-> (scores [n], the guard words behind the scores, the guard words behind the workspace)"""
    L, lib_ = lib()
    n, H = cls.shape
    words = (H // L.RERANK_FEATURES) * n
    ws = torch.full((words + GUARD,), SENT_F, dtype=torch.float64, device="cuda")
    out = torch.full((n + GUARD,), SENT_F, dtype=torch.float32, device="cuda")
    rc = lib_.rdx_rerank_head_rows_f16(0, cls.data_ptr(), n, H, wd.data_ptr(), bd.data_ptr(), wo.data_ptr(), bo.data_ptr(), ws.data_ptr(),
                                       out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.last_error()
    return out[:n], out[n:].cpu().numpy(), ws[words:].cpu().numpy()


@pytest.mark.parametrize("H", [64, 512, 1024])
def test_head_rows_equals_the_single_call_on_slices(H):
    """(a workgroup of the new launch takes ONE 64-row block, as rdx_rerank_head_f16's does: the grid grows, no workgroup walks)"""
    w = make_head(H, H)
    g = torch.Generator().manual_seed(H + 3)
    for n in (1, 63, 64, 65, 1024, 1025, 2113):
        cls = torch.randn(n, H, generator=g).cuda()
        cls[n - 1] = cls[0]                                                 # duplicate rows 0 and n - 1
        got, guard_s, guard_w = head_rows(cls, *w)
        assert (guard_s == SENT_F).all() and (guard_w == SENT_F).all(), (H, n)
        want = torch.cat([head(cls[a:a + 1024].contiguous(), *w) for a in range(0, n, 1024)])
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (H, n)
        assert got[0].item() == got[n - 1].item()
        if n == 2113:                                                       # another cut of the same rows: a row's bits do not depend on its call
            other = torch.cat([head(cls[a:a + 700].contiguous(), *w) for a in range(0, n, 700)])
            assert torch.equal(got.view(torch.int32), other.view(torch.int32))
            assert torch.equal(head_rows(cls, *w)[0], got)                  # and not on the call's number either
            ref, bound = head_reference(cls, *w)
            assert (np.abs(got.double().cpu().numpy() - ref) <= 1.0001 * bound).all()


def test_head_rows_one_row_past_the_single_call_at_hidden_2048():
    """n = 1025 at H = 2048: 17 row blocks, the last holding one row, and two passes of the k0 loop in each"""
    H, n = 2048, 1025
    w = make_head(H, H)
    cls = torch.randn(n, H, generator=torch.Generator().manual_seed(H + 3)).cuda()
    cls[n - 1] = cls[0]
    got, guard_s, guard_w = head_rows(cls, *w)
    assert (guard_s == SENT_F).all() and (guard_w == SENT_F).all()
    want = torch.cat([head(cls[a:a + 1024].contiguous(), *w) for a in range(0, n, 1024)])
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert got[0].item() == got[n - 1].item()
    ref, bound = head_reference(cls, *w)
    err = np.abs(got.double().cpu().numpy() - ref)
    assert (err <= 1.0001 * bound).all(), float((err / bound).max())
    assert np.ptp(ref) > 0.3


# ---- selection -----------------------------------------------------------------------------------------------------------------------

def select_batch(scores, boosts, lengths, top_k, min_score, keep_min=3, want_boosted=True):
    """one rdx_rerank_select_batch call -> (order, final, count, boosted) as host arrays, guard words checked"""
    L, lib_ = lib()
    nq, n = len(lengths), int(sum(lengths))
    off = pinned(np.concatenate([[0], np.cumsum(lengths)]), torch.int32)
    s = torch.as_tensor(np.asarray(scores, dtype=np.float32)).cuda() if n else torch.zeros(1, dtype=torch.float32, device="cuda")
    b = (torch.as_tensor(np.asarray(boosts, dtype=np.float64)).cuda() if n else torch.zeros(1, dtype=torch.float64, device="cuda")) if boosts is not None else None
    order = torch.full((n + GUARD,), SENT_I, dtype=torch.int32, device="cuda")
    final = torch.full((n + GUARD,), SENT_F, dtype=torch.float64, device="cuda")
    count = torch.full((nq + GUARD,), SENT_I, dtype=torch.int32, device="cuda")
    boosted = torch.full((nq + GUARD,), SENT_I, dtype=torch.int32, device="cuda")
    rc = lib_.rdx_rerank_select_batch(0, s.data_ptr(), b.data_ptr() if b is not None else None, nq, off.data_ptr(), top_k, float(min_score), keep_min,
                                      order.data_ptr(), final.data_ptr(), count.data_ptr(), boosted.data_ptr() if want_boosted else None,
                                      torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.last_error()
    torch.cuda.synchronize()
    o, f, c, h = order.cpu().numpy(), final.cpu().numpy(), count.cpu().numpy(), boosted.cpu().numpy()
    assert (o[n:] == SENT_I).all() and (f[n:] == SENT_F).all() and (c[nq:] == SENT_I).all() and (h[nq:] == SENT_I).all()
    if not want_boosted:
        assert (h == SENT_I).all()
    return o[:n], f[:n], c[:nq], h[:nq]


MIN_SCORE = 0.3


def segment_data(n, seed, nan):
    """scores with ties, +0.0 and -0.0, values on both sides of MIN_SCORE (and NaN); boosts negative, zero and positive"""
    rng = np.random.default_rng(seed)
    levels = np.asarray([0.0, -0.0, 0.1, 0.29999, 0.3, 0.30001, 0.7, 0.7, 0.95], dtype=np.float32)
    s = levels[rng.integers(0, len(levels), n)] if seed % 2 else rng.uniform(0, 1, n).astype(np.float32)
    if n >= 2:
        s[0], s[n - 1] = 0.0, -0.0                                          # the +-0.0 tie: equal, input order decides
    if nan and n >= 3:
        s[rng.integers(0, n, max(1, n // 9))] = np.nan
    b = rng.choice([0.15, 0.05, -0.1, 0.0, 0.0, 0.2 - 0.7], n)              # (0.7 + (0.2 - 0.7) would tie 0.2: never added, it is negative)
    if n >= 4:
        b[1], b[2], b[3] = -0.1, 0.0, 0.15
    return s, b


LENGTHS = [0, 1, 2, 3, 40, 63, 64, 65, 1024, 0, 5]


def check_segments(lengths, top_k, nan, host_too, boosts_on=True):
    data = [segment_data(n, 100 + i + 7 * n, nan) for i, n in enumerate(lengths)]
    results = []
    for order_of_segments in (list(range(len(lengths))), list(reversed(range(len(lengths))))):
        lens = [lengths[i] for i in order_of_segments]
        scores = np.concatenate([data[i][0] for i in order_of_segments] + [np.zeros(0, np.float32)])
        boosts = np.concatenate([data[i][1] for i in order_of_segments] + [np.zeros(0)]) if boosts_on else None
        o, f, c, h = select_batch(scores, boosts, lens, top_k, MIN_SCORE)
        off = np.concatenate([[0], np.cumsum(lens)])
        per = {}
        for q, i in enumerate(order_of_segments):
            per[i] = (o[off[q]:off[q + 1]].tolist(), f[off[q]:off[q + 1]], int(c[q]), int(h[q]))
        results.append(per)
    for i, n in enumerate(lengths):
        got, rev = results[0][i], results[1][i]
        assert got[0] == rev[0] and np.array_equal(bits(got[1]), bits(rev[1])) and got[2:] == rev[2:], (i, n, top_k)   # whatever its neighbours are
        s, b = data[i]
        assert got[3] == (int((b > 0).sum()) if boosts_on else 0), (i, n)
        if n == 0:
            assert got[2] == 0 and got[0] == []
            continue
        want = select(s, b if boosts_on else None, top_k, MIN_SCORE)
        assert got[0] == want[0] and got[2] == want[2] and np.array_equal(bits(got[1]), bits(want[1])), (i, n, top_k)
        assert sorted(got[0]) == list(range(n))
        if host_too:
            host = RR.select_host(s, b if boosts_on else None, top_k, MIN_SCORE)
            assert got[0] == host[0] and got[2] == host[2] and np.array_equal(bits(got[1]), bits(host[1])), (i, n, top_k)
    return results[0]


@pytest.mark.parametrize("top_k", [0, 1, 3, 10, 2000])
def test_select_batch_equals_the_single_call_per_segment(top_k):
    """NaN scores are compared with rdx_rerank_select only (it ranks them last; Python's sort, which select_host is, leaves them where
    its comparisons happen to: undefined there); the same segments without NaN are compared with select_host as well"""
    per = check_segments(LENGTHS, top_k, nan=True, host_too=False)
    assert any(np.isnan(per[i][1]).any() for i in per)
    per = check_segments(LENGTHS, top_k, nan=False, host_too=True)
    counts = [per[i][2] for i in range(len(LENGTHS))]
    assert counts[0] == 0 and counts[9] == 0
    if top_k in (0, 1):
        assert counts[3] == 3 and counts[4] == 3 and counts[1] <= top_k and counts[2] <= top_k     # keep_min when n >= 3, even above top_k
    check_segments(LENGTHS[:5], top_k, nan=False, host_too=True, boosts_on=False)                   # boosts = NULL


def test_select_batch_at_the_edges_of_its_workgroup_widths():
    from rag_dpo_amd import _lib as L
    assert L.RERANK_SELECT_WIDTHS == (64, 256, 1024)
    for w in L.RERANK_SELECT_WIDTHS:
        for longest in (w, w + 1):
            if longest > 1024:
                continue
            check_segments([5, longest, 0, 3], 10, nan=True, host_too=False)
            check_segments([longest], 3, nan=False, host_too=True)
    counts = select_batch(np.zeros(0), None, [0, 0], 5, 0.1, want_boosted=False)[2]                # nothing but empty segments
    assert counts.tolist() == [0, 0]


# ---- topic boost ---------------------------------------------------------------------------------------------------------------------

QUESTIONS = [(3, 7, 9), (0, 4, 4), (2, 0, 3), (32, 64, 40), (1, 1, 1)]     # (topics, distinct tags, candidates)


def topic_inputs(dim):
    rng = np.random.default_rng(dim)
    table = make_table(dim, dim)
    out = []
    for qi, (T, U, n) in enumerate(QUESTIONS):
        ts = rng.integers(7, ROWS, T).tolist()
        us = rng.integers(7, ROWS, U).tolist()
        if T >= 3:
            ts[1] = -1                                                      # a topic without an embedding
        if U >= 4:
            us[0], us[1], us[2], us[3] = 4, 5, -1, ROWS + 3                 # |row|^2 above 1.0 against topic row 3, the threshold row, no slot, a slot past the table
        if T >= 32:
            ts[0], ts[2] = 6, 3                                             # e1 and the row whose square is 1 + 2^-52
        offsets, pairs = [0], []
        for c in range(n):
            if c % 4 != 3:                                                  # (every fourth candidate has no tags: no pairs)
                k = int(rng.integers(1, 4))
                tags = rng.integers(0, max(U, 1), k).tolist()
                exact_at = int(rng.integers(0, 6 * max(T, 1) * k))          # now and then inside the list: an exact pair ends the replay
                pairs += [(t, u, t * k + j == exact_at) for t in range(max(T, 1)) for j, u in enumerate(tags)]
            offsets.append(len(pairs))
        out.append((ts, us, offsets, pairs))
    return table, out


@pytest.mark.parametrize("dim", [64, 100, 1024, 4096])
def test_topic_boost_batch_equals_the_single_call_per_question(dim):
    L, lib_ = lib()
    table, questions = topic_inputs(dim)
    tab = torch.from_numpy(table).cuda()
    nq = len(questions)
    topic_off = np.concatenate([[0], np.cumsum([len(q[0]) for q in questions])])
    tag_off = np.concatenate([[0], np.cumsum([len(q[1]) for q in questions])])
    cand_off = np.concatenate([[0], np.cumsum([len(q[2]) - 1 for q in questions])])
    sim_off = np.concatenate([[0], np.cumsum([len(q[0]) * len(q[1]) for q in questions])])
    pair_off, words = [0], []
    for ts, us, offsets, pairs in questions:
        base = len(words)
        words += [L.topic_pair(t, u, e) for t, u, e in pairs]
        pair_off += [base + o for o in offsets[1:]]
    n, S = int(cand_off[-1]), int(sim_off[-1])
    shapes = [pinned(topic_off, torch.int32), pinned(tag_off, torch.int32), pinned(sim_off, torch.int64), pinned(cand_off, torch.int32)]
    d_ts = torch.tensor([s for q in questions for s in q[0]], dtype=torch.int32, device="cuda")
    d_us = torch.tensor([s for q in questions for s in q[1]], dtype=torch.int32, device="cuda")
    d_po = torch.tensor(pair_off, dtype=torch.int64, device="cuda")
    d_pw = torch.tensor(words + [0], dtype=torch.int32, device="cuda")
    sims = torch.full((S + GUARD,), SENT_F, dtype=torch.float64, device="cuda")
    boosts = torch.full((n + GUARD,), SENT_F, dtype=torch.float64, device="cuda")
    best = torch.full((n + GUARD,), SENT_F, dtype=torch.float64, device="cuda")
    T32 = float(np.float32(0.65))
    rc = lib_.rdx_topic_boost_batch(0, tab.data_ptr(), tab.shape[0], dim, nq, shapes[0].data_ptr(), d_ts.data_ptr(), shapes[1].data_ptr(), d_us.data_ptr(),
                                    shapes[2].data_ptr(), shapes[3].data_ptr(), d_po.data_ptr(), d_pw.data_ptr(), len(words), T32, 0.15,
                                    sims.data_ptr(), boosts.data_ptr(), best.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.last_error()
    torch.cuda.synchronize()
    sims, boosts, best = sims.cpu().numpy(), boosts.cpu().numpy(), best.cpu().numpy()
    assert (sims[S:] == SENT_F).all() and (boosts[n:] == SENT_F).all() and (best[n:] == SENT_F).all()
    assert not (boosts[:n] == SENT_F).any() and not (best[:n] == SENT_F).any()                     # every entry written
    seen = set()
    for q, (ts, us, offsets, pairs) in enumerate(questions):
        lo, hi = int(cand_off[q]), int(cand_off[q + 1])
        one_b, one_s, one_sims = run_kernel(table, ts, us, offsets, pairs, T32, table_dev=tab)
        m = hi - lo
        assert np.array_equal(bits(boosts[lo:hi]), bits(one_b[:m])) and np.array_equal(bits(best[lo:hi]), bits(one_s[:m])), (dim, q)
        TU = len(ts) * len(us)
        assert np.array_equal(bits(sims[int(sim_off[q]):int(sim_off[q]) + TU]), bits(one_sims[:TU])), (dim, q)
        want_b, want_s = M.kernel_model(table, ts, us, offsets, pairs, T32)
        assert np.array_equal(bits(boosts[lo:hi]), bits(want_b)) and np.array_equal(bits(best[lo:hi]), bits(want_s)), (dim, q)
        if not ts or not us:
            assert set(boosts[lo:hi].tolist()) <= {0.0, 0.15} and (bits(boosts[lo:hi])[boosts[lo:hi] == 0] == 0).all()   # +0.0 unless a pair is exact
        seen |= {"zero"} if (best[lo:hi] == 0).any() else set()
        seen |= {"one"} if (best[lo:hi] == 1.0).any() else set()
        seen |= {"between"} if ((best[lo:hi] > T32) & (best[lo:hi] < 1.0)).any() else set()
    assert seen == {"zero", "one", "between"}
    # best_sim = NULL, and the same bits on a second call
    again = torch.full((n,), SENT_F, dtype=torch.float64, device="cuda")
    sims2 = torch.empty((S,), dtype=torch.float64, device="cuda")
    rc = lib_.rdx_topic_boost_batch(0, tab.data_ptr(), tab.shape[0], dim, nq, shapes[0].data_ptr(), d_ts.data_ptr(), shapes[1].data_ptr(), d_us.data_ptr(),
                                    shapes[2].data_ptr(), shapes[3].data_ptr(), d_po.data_ptr(), d_pw.data_ptr(), len(words), T32, 0.15,
                                    sims2.data_ptr(), again.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.last_error()
    assert np.array_equal(bits(again.cpu().numpy()), bits(boosts[:n]))


# ---- argument checks -----------------------------------------------------------------------------------------------------------------

def test_invalid_arguments_are_refused_before_any_launch():
    L, lib_ = lib()
    x = torch.full((4096,), SENT_F, dtype=torch.float64, device="cuda")
    p, st = x.data_ptr(), torch.cuda.current_stream().cuda_stream
    bad = L.RDX_ERR_INVALID
    # head: n, hidden, null and misaligned pointers
    for n, H in ((0, 64), (L.RERANK_BATCH_MAX_ROWS + 1, 64), (4, 96), (4, 4160), (4, 0)):
        assert lib_.rdx_rerank_head_rows_f16(0, p, n, H, p, p, p, p, p, p, st) == bad and L.last_error(), (n, H)
    assert lib_.rdx_rerank_head_rows_f16(0, p, 4, 64, p, p, p, p, None, p, st) == bad and "null" in L.last_error()
    assert lib_.rdx_rerank_head_rows_f16(0, p + 4, 4, 64, p, p, p, p, p, p, st) == bad and "aligned" in L.last_error()
    assert lib_.rdx_rerank_head_rows_f16(0, p, 4, 64, p, p, p, p, p + 4, p, st) == bad
    # selection (the pinned arrays are held in `keep` until the end: the calls read them)
    keep = []

    def pinned_(values, dtype):
        keep.append(pinned(values, dtype))
        return keep[-1]
    ok = pinned([0, 3, 5], torch.int32)
    sel = lambda nq, off, top_k=3, keep=3, order=p, count=p: lib_.rdx_rerank_select_batch(0, p, None, nq, off, top_k, 0.08, keep, order, p, count, None, st)   # noqa: E731
    assert sel(0, ok.data_ptr()) == bad and "nq" in L.last_error()
    assert sel(2, ok.data_ptr(), top_k=-1) == bad and "top_k" in L.last_error()
    assert sel(2, ok.data_ptr(), keep=-1) == bad
    assert sel(2, None) == bad and sel(2, ok.data_ptr(), order=None) == bad and sel(2, ok.data_ptr(), count=None) == bad
    assert sel(2, ok.data_ptr() + 2) == bad and sel(2, ok.data_ptr(), order=p + 2) == bad and "misaligned" in L.last_error()
    assert sel(2, pinned_([0, 5, 3], torch.int32).data_ptr()) == bad and "decrease" in L.last_error()
    assert sel(2, pinned_([0, 1025, 1030], torch.int32).data_ptr()) == bad and "1024" in L.last_error()
    assert sel(2, pinned_([1, 3, 5], torch.int32).data_ptr()) == bad and "start at 0" in L.last_error()
    on_device = torch.tensor([0, 3, 5], dtype=torch.int32, device="cuda")
    assert sel(2, on_device.data_ptr()) == bad and "pinned" in L.last_error()                     # a shape array the host cannot read
    # topic boost
    z3, z3l = pinned_([0, 0, 0], torch.int32), pinned_([0, 0, 0], torch.int64)

    def boost(nq=2, dim=8, topic_off=z3, tag_off=z3, sim_off=z3l, cand_off=ok, n_pairs=0, pair_off=p, boosts=p):
        return lib_.rdx_topic_boost_batch(0, p, 4, dim, nq, topic_off.data_ptr(), p, tag_off.data_ptr(), p, sim_off.data_ptr(), cand_off.data_ptr(), pair_off, p,
                                          n_pairs, 0.65, 0.15, p, boosts, None, st)
    assert boost(nq=0) == bad and "nq" in L.last_error()
    assert boost(dim=0) == bad and boost(dim=4097) == bad and boost(n_pairs=-1) == bad
    assert boost(topic_off=pinned_([0, 33, 33], torch.int32), sim_off=pinned_([0, 4000, 4000], torch.int64), tag_off=pinned_([0, 1, 1], torch.int32)) == bad and "32 topics" in L.last_error()
    assert boost(topic_off=pinned_([0, 2, 1], torch.int32)) == bad
    assert boost(cand_off=pinned_([0, 5, 3], torch.int32)) == bad and "decrease" in L.last_error()
    assert boost(cand_off=pinned_([0, 1025, 1025], torch.int32)) == bad and "1024" in L.last_error()
    assert boost(topic_off=pinned_([0, 2, 2], torch.int32), tag_off=pinned_([0, 3, 3], torch.int32)) == bad and "sim_off" in L.last_error()   # a block too small
    assert boost(pair_off=None) == bad and boost(boosts=None) == bad and boost(pair_off=p + 4) == bad
    assert boost(cand_off=on_device) == bad and "pinned" in L.last_error()
    torch.cuda.synchronize()
    assert (x.cpu().numpy() == SENT_F).all()                                                       # nothing was launched: nothing was written


# ---- rerank_batch --------------------------------------------------------------------------------------------------------------------

def test_golden_cases_in_batches_on_the_gpu():
    assert check_golden_batches("cuda") >= 22


class ScriptedEmbedder:
    """a provider with embed() only: a unit vector per text, from its crc32"""
    device = "cuda:0"

    def __init__(self):
        self.calls = []

    def embed(self, texts):
        self.calls.append(list(texts))
        out = []
        for t in texts:
            v = np.random.default_rng(zlib.crc32(t.lower().encode("utf-8")) % 7).standard_normal(32) + 0.35 * np.random.default_rng(zlib.crc32(t.encode("utf-8"))).standard_normal(32)
            out.append((v / np.linalg.norm(v)).astype(np.float32).tolist())
        return out


def test_rerank_batch_with_scripted_scores_equals_the_loop_field_for_field(caplog):
    import logging
    from rag_dpo_amd.topics import TopicMatcher
    members = [m for k, ms in golden_batches() if k == 8 and not any(c["raises"] for c, _, _ in ms) for m in ms]
    queries, chunks = [q for _, _, q in members], [case_chunks(c) for c, _, _ in members]
    big = max(range(len(chunks)), key=lambda i: len(chunks[i]))
    topics = [None] * len(members)
    topics[big] = ["durée de conservation", "Cookies", "sécurité des données"]
    for i, c in enumerate(chunks):
        if i != big and len(c) >= 2 and i % 2:
            topics[i] = ["vidéosurveillance", "consentement"]
    assert any(not c for c in chunks) and any(t is None and c for t, c in zip(topics, chunks)) and sum(1 for t in topics if t) >= 2
    r = RR.CrossEncoderReranker(device="cuda", min_score=0.08)
    r._model, _ = golden_world(r)
    # no matcher; a matcher with only topic_boost (host boosts, uploaded); a TopicMatcher on the GPU (one batched device call)
    plain = r.rerank_batch(queries, chunks, top_k=8)
    assert [ranked_values(g) for g in plain] == [ranked_values(r.rerank(q, c, top_k=8)) for q, c in zip(queries, chunks)]
    assert r._model.calls[0] == sum(len(c) for c in chunks)                                        # ONE predict over all pairs

    class Tagged:
        def topic_boost(self, question_topics, tags):
            return 0.15 * ((zlib.crc32((question_topics[0] + tags).encode()) % 3) / 2.0)

    hosted = r.rerank_batch(queries, chunks, top_k=8, topic_matcher=Tagged(), question_topics=topics)
    assert [ranked_values(g) for g in hosted] == [ranked_values(r.rerank(q, c, top_k=8, topic_matcher=Tagged(), question_topics=t))
                                                  for q, c, t in zip(queries, chunks, topics)]
    assert [ranked_values(g) for g in hosted] != [ranked_values(g) for g in plain]
    emb = ScriptedEmbedder()
    tm = TopicMatcher(emb, device="cuda:0")
    with caplog.at_level(logging.INFO, logger="rag_dpo_amd.reranker"):
        got = r.rerank_batch(queries, chunks, top_k=8, topic_matcher=tm, question_topics=topics)
    assert len(emb.calls) == 1 and tm.stats["device_calls"] == 1 and tm.stats["host_calls"] == 0   # one embed, one rdx_topic_boost_batch
    st = r.last_rerank_stats
    assert st["device_calls"] == 1 and st["questions"] == sum(1 for c in chunks if c) and st["pairs"] == sum(len(c) for c in chunks)
    batch_log = sorted(m for m in caplog.messages if "topic boost applied" in m)
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="rag_dpo_amd.reranker"):
        want = [r.rerank(q, c, top_k=8, topic_matcher=tm, question_topics=t) for q, c, t in zip(queries, chunks, topics)]
    assert [ranked_values(g) for g in got] == [ranked_values(w) for w in want]
    assert batch_log == sorted(m for m in caplog.messages if "topic boost applied" in m) and batch_log
    assert [ranked_values(g) for g in got] != [ranked_values(g) for g in plain]                    # the boosts moved something
    assert got[[i for i, c in enumerate(chunks) if not c][0]] == []
    # the batched boosts alone, against the single-question call
    tags = [[c.metadata.get("rgpd_topics", "") for c in cs] for cs in chunks]
    dev = tm.topic_boosts_device_batch([t or [] for t in topics], tags).cpu().numpy()
    one = np.concatenate([tm.topic_boosts_device(t or [], g).cpu().numpy() if g else np.zeros(0) for t, g in zip(topics, tags)])
    assert np.array_equal(bits(dev), bits(one)) and (dev > 0).any() and (dev == 0).any()


def test_rerank_batch_mid_fused_against_the_fp32_module_forward():
    """test_gpu_reranker.check_end_to_end's comparison for three questions in one batch: per pair |score - fp32 module score| within
    the <s>-row difference pushed through the head plus the head's bound; the order wherever reference gaps exceed twice that; and
    |1 - cos| of every <s> row against the module forward's row of THE SAME pair (a row on the wrong pair cannot hide)"""
    r = RR.CrossEncoderReranker("random-init:mid", device="cuda", dtype=torch.float16, min_score=0.0)
    r._load_model()
    m = r._model
    assert m.path == "fused"
    ref = copy.deepcopy(m.model).float()
    # 10 .. 300 tokens, the three questions' lengths interleaved once sorted: q0 takes ranks 0, 3, 6, ... of the ladder, and so on
    ladder = np.linspace(300, 10, 57).astype(int).tolist()
    take = {0: [], 1: [], 2: []}
    sizes = {0: 12, 1: 40, 2: 5}
    k = 0
    while any(len(take[q]) < sizes[q] for q in take):
        for q in take:
            if len(take[q]) < sizes[q]:
                take[q].append(ladder[k])
                k += 1
    rng = np.random.default_rng(8)
    groups = []
    for q in range(3):
        lengths = [take[q][i] for i in rng.permutation(sizes[q])]
        groups.append((lengths, pairs_of_lengths(lengths, 20 + q)))
    assert len({g[1][0][0] for g in groups}) == 3                                                   # three different questions
    every = [p for _, ps in groups for p in ps]
    cls32 = module_cls32(ref, m.tokenize, every)
    spread_head_along_pairs(m, ref, cls32)
    from rag_dpo_amd.retriever import RetrievedChunk
    chunk_lists = [[RetrievedChunk(f"q{q}c{i}", d, f"doc{i % 7}", "GUIDE", i, "high", 0.5, {}) for i, (_, d) in enumerate(ps)]
                   for q, (_, ps) in enumerate(groups)]
    out = r.rerank_batch([ps[0][0] for _, ps in groups], chunk_lists, top_k=40)
    st = r.last_rerank_stats
    assert st["path"] == "fused" and st["questions"] == 3 and st["pairs"] == 57 and st["device_calls"] == 1
    assert st["tokens"] == sum(max(L, 17) for ls, _ in groups for L in ls) and st["ms_forward"] > 0 and st["ms_head_select"] > 0
    assert [len(o) for o in out] == [12, 40, 5]
    got = np.empty(57)
    base = 0
    for o, (_, ps) in zip(out, groups):
        assert sorted(x.original_rank for x in o) == list(range(len(ps)))
        for x in o:
            got[base + x.original_rank] = x.rerank_score
        base += len(ps)
    with torch.no_grad():
        cls16 = m._cls_rows(every, 32).double()
        cos = torch.nn.functional.cosine_similarity(cls16, cls32, dim=1)
        assert float((1 - cos).max()) <= 1e-4, float((1 - cos).max())
        c = m.model.classifier
        hw = (c.dense.weight.half(), c.dense.bias.half(), c.out_proj.weight.half().reshape(-1), c.out_proj.bias.half())
        want, _ = head_reference(cls32, *hw)
        _, head_bound = head_reference(cls16, *hw)
        dz = ((cls16 - cls32) @ hw[0].double().T).abs()
        tol = (0.25 * (dz @ hw[2].double().abs())).cpu().numpy() + head_bound + 1e-9
    err = np.abs(got - want)
    print(f"rerank_batch mid: max err {err.max():.3e}, max err/tol {float((err / tol).max()):.3f}, tol max {tol.max():.3e}, spread {np.ptp(want):.3f}")
    assert (err <= tol).all(), (float((err / tol).max()), float(err.max()))
    T = float(tol.max())
    assert T <= 0.1 and np.ptp(want) > 0.3, (T, np.ptp(want))
    base = 0
    for o, (_, ps) in zip(out, groups):
        w, g = want[base:base + len(ps)], got[base:base + len(ps)]
        idx = np.argsort(-w, kind="stable")
        for a, b in zip(idx[:-1], idx[1:]):
            if w[a] - w[b] > 2 * T:
                assert g[a] > g[b]
        assert [x.rerank_score for x in o] == sorted((x.rerank_score for x in o), reverse=True)
        base += len(ps)


def test_retrieve_reranked_batch_equals_the_loop_on_the_gpu_collection(tmp_path):
    import bm25_replay as R
    from bm25_replay import W
    from rag_dpo_amd.retriever import DenseRetriever
    from test_gpu_fusion import DeviceHashEmbedder

    col = W.build_collection(None)
    chunk = R.chunk_index(None)
    summ = R.summary_index(None, str(tmp_path))
    queries = [W.Q0, "registre des traitements du sous-traitant article 28", "notification d'une violation en 72 heures",
               "biométrie badge salariés", "zzzinconnu qqqabsent"]
    wheres = [None, {"chunk_nature": {"$in": ["GUIDE", "DOCTRINE"]}}, None, {"chunk_nature": "NO_SUCH_NATURE"}, None]
    topics = [["cookies"], None, ["sécurité"], ["cookies"], None]
    ret = DenseRetriever(col, DeviceHashEmbedder(), query_expander=W.expander, summary_bm25_index=summ, chunk_bm25_index=chunk, fusion="device")

    class Model:
        def predict(self, pairs, batch_size=32, show_progress_bar=True):
            return np.asarray([(zlib.crc32((p[0] + p[1]).encode()) % 1000) / 1000.0 for p in pairs], dtype=np.float32)

    class Boost:
        def topic_boost(self, question_topics, tags):
            return 0.15 * ((zlib.crc32((question_topics[0] + str(tags)).encode()) % 4) / 3.0)

    gpu = RR.CrossEncoderReranker(device="cuda")
    gpu._model = Model()
    got = ret.retrieve_reranked_batch(queries, gpu, n_candidates=40, top_k=10, where_filter=wheres, topic_matcher=Boost(), question_topics=topics)
    assert gpu.last_rerank_stats["questions"] >= 3 and gpu.last_rerank_stats["device_calls"] == 1
    want = [ret.retrieve_reranked(q, gpu, n_candidates=40, top_k=10, where_filter=w, topic_matcher=Boost(), question_topics=t)
            for q, w, t in zip(queries, wheres, topics)]
    assert got == want                                                                              # dataclass equality: paths, chunk ids, order, every float
    assert sum(len(d.chunks) for d in got[0]) == 10
    flat = lambda docs: [(d.document_path, np.float64(d.avg_similarity).tobytes(), [(c.chunk_id, np.float64(c.hybrid_score).tobytes(), np.float64(c.distance).tobytes()) for c in d.chunks]) for d in docs]   # noqa: E731
    assert [flat(g) for g in got] == [flat(w) for w in want]
