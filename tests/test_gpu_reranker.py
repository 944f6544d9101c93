"""GPU: the reranker's librdx kernels (rdx_rerank_head_f16, rdx_rerank_select) against fp64 references with derived error bounds,
exact-answer probes and the golden fixture of the reference's own rerank; the reranker end to end against transformers' fp32 module
forward of the same weights; DenseRetriever.retrieve_reranked against its parts."""
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
sys.path.insert(0, os.path.join(HERE, "golden"))
import rerank_head_model as HM  # noqa: E402
import reranker_world as W  # noqa: E402
from test_reranker import GOLDEN, check_against_gold, run_case  # noqa: E402

pytestmark = pytest.mark.gpu
U32 = 2.0 ** -24
head_reference = HM.reference                                                # (score, derived bound): test_gpu_rerank_batch imports it from here


def lib():
    from rag_dpo_amd import _lib
    return _lib, _lib.load()


def head(cls, wd, bd, wo, bo, stream=None):
    L, lib_ = lib()
    n, H = cls.shape
    ws = torch.empty(((H // L.RERANK_FEATURES) * n,), dtype=torch.float64, device="cuda")
    out = torch.empty((n,), dtype=torch.float32, device="cuda")
    st = (stream or torch.cuda.current_stream()).cuda_stream
    rc = lib_.rdx_rerank_head_f16(0, cls.data_ptr(), n, H, wd.data_ptr(), bd.data_ptr(), wo.data_ptr(), bo.data_ptr(), ws.data_ptr(),
                                  out.data_ptr(), st)
    assert rc == 0, L.last_error()
    return out


def select(scores, boosts, top_k, min_score, keep_min=3):
    L, lib_ = lib()
    n = len(scores)
    s = torch.as_tensor(np.asarray(scores, dtype=np.float32)).cuda()
    b = torch.as_tensor(np.asarray(boosts, dtype=np.float64)).cuda() if boosts is not None else None
    order = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    final = torch.empty((n,), dtype=torch.float64, device="cuda")
    count = torch.empty((1,), dtype=torch.int32, device="cuda")
    rc = lib_.rdx_rerank_select(0, s.data_ptr(), b.data_ptr() if b is not None else None, n, top_k, float(min_score), keep_min,
                                order.data_ptr(), final.data_ptr(), count.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.last_error()
    return order.cpu().tolist(), final.cpu().tolist(), int(count.item())


def make_head(H, seed, scale=3.0):
    return tuple(t.cuda() for t in HM.random_head(H, seed, scale))


def on_gpu(arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


HIDDEN = [64, 512, 768, 1024, 1088, 2048, 4096]     # the ends of the admitted range, the tested models' sizes, one and more passes of the k0 loop
RATIOS = {}                                          # (bound, H) -> max(err / bound) seen: printed by test_report_head_ratios


@pytest.mark.parametrize("H", HIDDEN)
def test_head_against_fp64_with_derived_bound(H):
    """n = 65 and 129: a second / third row block of one row, whose wave has no second row (two == false). H > 1024: the k0 loop's second
    and later passes; H = 4096 asks for 64 KiB of dynamic LDS beside the kernel's 2 KiB of static LDS"""
    w = make_head(H, H)
    worst = 0.0
    for n, rows in HM.random_rows(H, (1, 3, 40, 100, 1024, 65, 129) if H <= 1024 else (1, 65, 130)):
        cls = rows.cuda()
        got = head(cls, *w).double().cpu().numpy()
        want, bound = head_reference(cls, *w)
        err = np.abs(got - want)
        worst = max(worst, float((err / bound).max()))
        assert (err <= 1.0001 * bound).all(), (H, n, float((err / bound).max()))
        assert np.ptp(want) > 0.3 if n >= 40 else True
        again = head(cls, *w)                                               # no atomics: bit-identical on every call
        assert torch.equal(again, head(cls, *w)) and np.array_equal(again.double().cpu().numpy(), got)
    RATIOS[("derived", H)] = worst
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = head(cls, *w, stream=side)
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(other, again)


@pytest.mark.parametrize("H", HIDDEN)
def test_head_exact_probes_every_hidden(H):
    """inputs whose every partial sum is exact in fp32 (tests/rerank_head_model.py exact_probe): the whole error allowance is the score's one
    rounding to fp32 and the fp64 tail. tests/test_rerank_head_model.py shows what that rejects: an fp16 accumulator, a dropped k-round,
    exchanged w_o entries, a row pair reading one row twice and a missing b_d all miss it by factors of 1e5 and more"""
    worst = 0.0
    for n in (1, 2, 65):
        p = HM.exact_probe(H, n, n)
        got = head(*on_gpu(p)).double().cpu().numpy()
        want, tight = HM.tight_reference(*p)
        err = np.abs(got - want)
        worst = max(worst, float((err / tight).max()))
        assert (err <= tight).all(), (H, n, float((err / tight).max()))
    RATIOS[("tight", H)] = worst


def test_report_head_ratios():
    """(prints what the two tests above measured in this run: max(err / bound) per hidden size)"""
    for kind in ("derived", "tight"):
        print(kind + ": " + ", ".join(f"H={H}: {RATIOS[(kind, H)]:.3g}" for H in HIDDEN if (kind, H) in RATIOS))


def one_hot_weights(H):
    """W_d[f][k] in multiples of 1/32 within +-1.5 such that moving f by 1 or k by 1, 64 or 1024 changes the entry"""
    f = np.arange(H, dtype=np.int64)[:, None]
    k = np.arange(H, dtype=np.int64)[None, :]
    return (((7 * f + 13 * k + 5 * (k // 64) + 3 * (k // 1024)) % 97 - 48) / 32.0).astype(np.float16)


@pytest.mark.parametrize("H", [1088, 4096])
def test_head_one_hot_probes_reach_every_k_round_and_feature_block(H):
    """cls row = e_k, w_o = c e_f: score = sigmoid(c tanh(W_d[f][k] + b_d[f]) + b_o), z exact up to the one fp32 add of b_d. k: the first and
    last column of every 1024-wide pass of the k0 loop; f: first and last feature of the first and last block, and one mid-block"""
    c, b_o = 2.0, 0.25
    Wn = one_hot_weights(H)
    W64 = Wn.astype(np.float64)
    rng = np.random.default_rng(H)
    bn = (rng.standard_normal(H) * 0.1).astype(np.float16)
    ks = sorted({k for a in range(0, H, 1024) for k in (a, min(a + 1023, H - 1))})
    fs = [0, 7, 8 * (H // 16) + 3, H - 8, H - 1]
    assert H - 1 in ks and 1024 in ks and len(ks) == 2 * ((H + 1023) // 1024)
    cls_n = np.zeros((len(ks), H), dtype=np.float32)
    cls_n[np.arange(len(ks)), ks] = 1.0
    wd, bd, cls, bo = on_gpu((Wn, bn, cls_n, np.asarray([b_o], dtype=np.float16)))
    score_of = lambda z: 1.0 / (1.0 + np.exp(-(c * np.tanh(z) + b_o)))      # noqa: E731
    for f in fs:
        wo_n = np.zeros(H, dtype=np.float16)
        wo_n[f] = c
        got = head(cls, wd, bd, on_gpu((wo_n,))[0], bo).double().cpu().numpy()
        z = W64[f, ks] + float(bn[f])
        want = score_of(z)
        bound = U32 * want + 1e-12 * (abs(c) + abs(b_o)) / 4 + 1e-15 + U32 * np.abs(z) * abs(c) / 4
        assert (np.abs(got - want) <= bound).all(), (H, f, (np.abs(got - want) / bound).max())
        for i, k in enumerate(ks):                                          # a wrong (f, k) would show: every neighbour scores differently
            for f2, k2 in ((f - 1, k), (f + 1, k), (f, k - 1), (f, k + 1), (f, k - 64), (f, k + 64), (f, k - 1024), (f, k + 1024)):
                if 0 <= f2 < H and 0 <= k2 < H:
                    assert abs(score_of(W64[f2, k2] + float(bn[f2])) - want[i]) > 100 * bound[i], (H, f, k, f2, k2)


def test_head_saturates_to_exact_zero_and_one_and_never_to_nan():
    """|z| >= 40: tanh = +-1 exactly. logit >= 40: 1.0f. logit <= -800: exp overflows to inf and 1 / (1 + inf) = 0.0f. fp16 w_o reaches
    65504, so a checkpoint can get there. Finite inputs whose dot products stay finite in fp32 never give NaN"""
    H = 1088
    rng = np.random.default_rng(7)
    sign = rng.choice([-1.0, 1.0], H)
    Wn = np.zeros((H, H), dtype=np.float16)
    Wn[:, 1030] = sign                                                      # z_f = +-v + b_d[f], the column in the second pass of the k0 loop
    bn = (rng.standard_normal(H) * 0.1).astype(np.float16)
    v = np.asarray([40.5, -40.5, 1e3, -1e3, 1e30, -1e30, 3e38, -3e38], dtype=np.float32)
    cls_n = np.zeros((len(v), H), dtype=np.float32)
    cls_n[:, 1030] = v
    wd, bd, cls = on_gpu((Wn, bn, cls_n))
    t = np.sign(v)[:, None] * sign[None, :]                                 # tanh(z) exactly
    for w0, b0 in ((40.0, 0.0), (-800.0, 0.0), (65504.0, 0.0), (-65504.0, 65504.0), (40.0, 0.5)):
        wo_n = np.zeros(H, dtype=np.float16)
        wo_n[H - 3] = w0                                                    # one feature: logit = +-w0 + b0, exact in any order
        got = head(cls, wd, bd, *on_gpu((wo_n, np.asarray([b0], dtype=np.float16)))).cpu().numpy()
        logit = t[:, H - 3] * w0 + b0
        assert not np.isnan(got).any() and ((got == 0.0) | (got == 1.0))[np.abs(logit) >= 800].all()
        assert (got[logit >= 40] == 1.0).all() and (got[logit <= -800] == 0.0).all() and (logit >= 40).any(), (w0, b0)
        mid = (logit > -800) & (logit < 40)
        want = 1.0 / (1.0 + np.exp(-logit[mid]))
        assert (np.abs(got[mid].astype(np.float64) - want) <= U32 * want + 1e-45).all()   # (-40 and -65504 + 65504 = 0 land here)
    wo_n = (rng.choice([-1.0, 1.0], H) * rng.choice([65504.0, 800.0, 40.0, 0.5], H)).astype(np.float16)   # every feature saturated, logits in the millions
    got = head(cls, wd, bd, *on_gpu((wo_n, np.zeros(1, dtype=np.float16)))).cpu().numpy()
    logit = t @ wo_n.astype(np.float64)                                     # exact: 1088 fp16 values in fp64
    assert (np.abs(logit) >= 800).all() and not np.isnan(got).any()
    assert np.array_equal(got, (logit > 0).astype(np.float32))


def test_head_non_finite_rows_touch_no_other_row():
    """NaN and +-Inf rows at the even and the odd place of a wave's row pair, and in the last row of a block with an odd row count: every
    other row keeps its bits; the poisoned rows score NaN or something in [0, 1]"""
    H, n = 1088, 64 + 3
    w = make_head(H, 3)
    g = torch.Generator().manual_seed(17)
    clean = torch.randn(n, H, generator=g)
    nan_row = clean[0].clone()
    nan_row[[5, 1029]] = float("nan")
    inf_row = clean[1].clone()
    inf_row[[0, 63, 1087]] = torch.tensor([float("inf"), float("-inf"), float("inf")])
    bad = clean.clone()
    poisoned = {10: nan_row, 11: inf_row, 20: inf_row, 21: nan_row, 33: inf_row, 66: nan_row}   # (10, 11) and (20, 21) are pairs of one wave; 66: block 1's third row
    for r, row in poisoned.items():
        bad[r] = row
    want = head(clean.cuda(), *w).cpu()
    got = head(bad.cuda(), *w).cpu()
    others = [r for r in range(n) if r not in poisoned]
    assert torch.equal(got[others].view(torch.int32), want[others].view(torch.int32))
    mine = got[sorted(poisoned)].numpy()
    assert (np.isnan(mine) | ((mine >= 0) & (mine <= 1))).all()
    assert np.isnan(got[[10, 21, 66]].numpy()).all()                        # a NaN in cls reaches every z of its row: its score is NaN
    assert torch.equal(head(bad[66:67].contiguous().cuda(), *w).cpu().view(torch.int32), got[66:67].view(torch.int32))   # the same bits alone


def test_head_exact_probes():
    H = 1024
    wd, bd, wo, bo = make_head(H, 5)
    zero = torch.zeros_like(wd)
    cls = torch.randn(100, H).cuda()
    s = head(cls, zero, bd, wo, bo).cpu().numpy()
    assert (s == s[0]).all()                                                # W_d = 0: every pair scores sigmoid(w_o . tanh(b_d) + b_o)
    t = np.tanh(bd.double().cpu().numpy())
    want = 1.0 / (1.0 + np.exp(-(t @ wo.double().cpu().numpy() + bo.double().item())))
    assert abs(float(s[0]) - want) <= 2 * U32 * want
    order, final, count = select(s, None, 10, 0.08)
    assert order == list(range(100)) and count == 10 and final == [float(s[0])] * 100   # all tied: input order
    dup = cls[[7, 3, 7, 7, 3]].contiguous()                                 # duplicate rows: bit-equal scores
    d = head(dup, wd, bd, wo, bo).cpu().numpy()
    assert d[0] == d[2] == d[3] and d[1] == d[4]
    full = head(cls, wd, bd, wo, bo).cpu().numpy()
    assert d[0] == full[7] and d[1] == full[3]                              # a row's score does not depend on its neighbours


def test_select_reproduces_golden_fixture():
    for case, gold in zip(W.cases(), GOLDEN["cases"]):
        if case["raises"] or not case["idx"]:
            continue
        boosts = [float(b[2]) for b in gold["boosts"]] if gold["boosts"] else None
        order, final, count = select(case["scores"], boosts, case["top_k"], case["min_score"])
        want = [] if "raises" in gold else gold["result"]
        assert count == len(want), case["name"]
        assert order[:count] == [r["original_rank"] for r in want], case["name"]
        assert [repr(final[i]) for i in order[:count]] == [r["rerank_score"] for r in want], case["name"]
        assert sorted(order) == list(range(len(case["idx"])))


def fuzz_select(keep_min_of):
    rng = np.random.default_rng(11)
    for it in range(60):
        n = int(rng.choice([1, 2, 3, 4, 17, 40, 100, 513, 1000, 1024]))
        levels = rng.uniform(0, 1, int(rng.integers(1, 6))).astype(np.float32)     # few distinct values: heavy ties
        scores = levels[rng.integers(0, len(levels), n)] if it % 3 else rng.uniform(0, 1, n).astype(np.float32)
        boosts = None
        if it % 2:
            boosts = np.where(rng.uniform(size=n) < 0.4, rng.choice([0.15, 0.05, -0.1, 0.0, 0.15 * 0.5], n), 0.0)
        top_k = int(rng.choice([0, 1, 2, 3, 8, 10, n, n + 5]))
        min_score = float(rng.choice([0.08, 0.0, 0.5, float(levels[0]), 2.0]))
        keep_min = keep_min_of(n)
        want = RR.select_host(scores, boosts, top_k, min_score, keep_min)
        got = select(scores, boosts, top_k, min_score, keep_min)
        assert got[0] == want[0] and got[2] == want[2], (it, n, top_k, min_score, keep_min)
        assert np.array_equal(np.asarray(got[1]).view(np.int64), np.asarray(want[1]).view(np.int64)), it
        assert HM.select_model(scores, boosts, top_k, min_score, keep_min)[::2] == want[::2]


def test_select_fuzz_against_python_restatement():
    fuzz_select(lambda n: 3)


KEEP_MIN = {"0": lambda n: 0, "1": lambda n: 1, "n": lambda n: n, "n + 1": lambda n: n + 1}


@pytest.mark.parametrize("keep_min", list(KEEP_MIN))
def test_select_fuzz_over_keep_min(keep_min):
    fuzz_select(KEEP_MIN[keep_min])


@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 1024])
def test_select_with_nan_equals_the_stated_order(n):
    """numbers first and descending, NaN finals last, ties and NaN among themselves in input order (rerank_head_model.select_model);
    `boost > 0.0` is false for a NaN boost: that final is the plain score. count = min(top_k, #{final >= min_score}) lifted to keep_min"""
    rng = np.random.default_rng(n)
    nan = np.float32("nan")
    levels = np.asarray([0.0, -0.0, 0.1, 0.29999, 0.3, 0.30001, 0.7, 0.7, 0.95], dtype=np.float32)
    cases = []
    for variant in range(3):
        s = levels[rng.integers(0, len(levels), n)] if variant else rng.uniform(0, 1, n).astype(np.float32)
        b = rng.choice([0.15, 0.05, -0.1, 0.0, 0.6], n)
        if variant == 0:
            s[rng.integers(0, n, max(1, n // 7))] = nan                     # NaN scores (a positive boost on one stays NaN)
        elif variant == 1:
            b[rng.integers(0, n, max(1, n // 5))] = np.nan                  # NaN boosts
        else:
            s[::2] = nan                                                    # both, NaN first and on every other candidate
            b[rng.integers(0, n, max(1, n // 5))] = np.nan
        cases.append((s, b))
    cases.append((np.full(n, nan, dtype=np.float32), None))                # nothing but NaN
    seen_nan_kept = False
    for s, b in cases:
        for keep_min in (0, 1, 3, n, n + 1):
            for top_k in (0, 1, n, n + 5):
                want = HM.select_model(s, b, top_k, 0.3, keep_min)
                got = select(s, b, top_k, 0.3, keep_min)
                where = (n, keep_min, top_k)
                assert got[0] == want[0] and got[2] == want[2], where
                assert np.array_equal(np.asarray(got[1]).view(np.int64), np.asarray(want[1]).view(np.int64)), where   # (NaN bits too: the score's, widened)
                seen_nan_kept |= any(np.isnan(got[1][i]) for i in got[0][:got[2]])
    assert seen_nan_kept or n < 2                                           # keep_min reaches into the NaN tail somewhere


def test_invalid_arguments_on_device():
    L, lib_ = lib()
    x = torch.zeros(4096, dtype=torch.float64, device="cuda")
    p = x.data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    for n, H in ((0, 1024), (1025, 1024), (4, 1000), (4, 4160), (4, 0)):
        assert lib_.rdx_rerank_head_f16(0, p, n, H, p, p, p, p, p, p, st) == L.RDX_ERR_INVALID and L.last_error()
    for n, top_k in ((0, 3), (1025, 3), (4, -1)):
        assert lib_.rdx_rerank_select(0, p, None, n, top_k, 0.08, 3, p, p, p, st) == L.RDX_ERR_INVALID and L.last_error()
    assert "top_k" in L.last_error()


# ---- end to end --------------------------------------------------------------------------------------------------------------

def pairs_of_lengths(lengths, seed):
    rng = np.random.default_rng(seed)
    vocab = [a + b for a in "abcdefghijklmnopqrstuvwxyz" for b in "abcdefghijklmnopqrstuvwxyz"]   # 3 characters a word: 512 tokens fit the 2048-character cut
    q = " ".join(rng.choice(vocab, 12))
    return [(q, " ".join(rng.choice(vocab, max(1, L - 16)))) for L in lengths]


def module_cls32(ref, tokenize, pairs):
    enc = tokenize([p[0] for p in pairs], [p[1] for p in pairs])
    with torch.no_grad():
        out = []
        for a in range(0, len(pairs), 8):
            ids, att = enc["input_ids"][a:a + 8].cuda(), enc["attention_mask"][a:a + 8].cuda()
            w = int(att.sum(1).max())
            out.append(ref.roberta(input_ids=ids[:, :w], attention_mask=att[:, :w]).last_hidden_state[:, 0].double())
    return torch.cat(out)


def spread_head_along_pairs(m, ref, cls32):
    """point out_proj along the direction the pairs' tanh(z) rows differ most, scaled to a logit spread of ~2 (a random-init head
    barely separates them); the same fp16 values in the kernel's weights (views of the module's) and in the fp32 reference"""
    c = ref.classifier
    t = torch.tanh(cls32 @ c.dense.weight.double().T + c.dense.bias.double())
    tc = t - t.mean(0)
    v = torch.linalg.svd(tc, full_matrices=False).Vh[0]
    k = 2.0 / float((tc @ v).std().detach())
    w = (v * k).half()
    with torch.no_grad():
        m.model.classifier.out_proj.weight.copy_(w[None, :].to(m.model.dtype))
        m.model.classifier.out_proj.bias.fill_(float(-(t @ w.double()).mean()))
        c.out_proj.weight.copy_(m.model.classifier.out_proj.weight.float())
        c.out_proj.bias.copy_(m.model.classifier.out_proj.bias.float())
    assert m.w_o.data_ptr() == m.model.classifier.out_proj.weight.data_ptr() or m.model.dtype != torch.float16
    if m.model.dtype != torch.float16:
        m.w_o.copy_(m.model.classifier.out_proj.weight.reshape(-1).half())
        m.b_o.copy_(m.model.classifier.out_proj.bias.half())


def check_end_to_end(spec, lengths, want_path, seed=0):
    r = RR.CrossEncoderReranker(f"random-init:{spec}", device="cuda", dtype=torch.float16, min_score=0.0)
    r._load_model()
    m = r._model
    assert m.path == want_path
    ref = copy.deepcopy(m.model).float()
    pairs = pairs_of_lengths(lengths, seed)
    cls32 = module_cls32(ref, m.tokenize, pairs)
    spread_head_along_pairs(m, ref, cls32)
    from rag_dpo_amd.retriever import RetrievedChunk
    chunks = [RetrievedChunk(f"c{i}", d, f"doc{i % 7}", "GUIDE", i, "high", 0.5, {}) for i, (_, d) in enumerate(pairs)]
    out = r.rerank(pairs[0][0], chunks, top_k=len(pairs))
    st = r.last_rerank_stats
    assert st["path"] == want_path and st["pairs"] == len(pairs) and st["tokens"] == sum(max(L, 17) for L in lengths)   # (12 query pieces + 1 text piece + 4 specials at least)
    assert st["ms_forward"] > 0 and st["ms_head_select"] > 0
    got = np.empty(len(pairs))
    for o in out:
        got[o.original_rank] = o.rerank_score
    assert len(out) == len(pairs)
    with torch.no_grad():
        cls16 = m._cls_rows(pairs, 32).double()
        cos = torch.nn.functional.cosine_similarity(cls16, cls32, dim=1)
        assert float((1 - cos).max()) <= 1e-4, float((1 - cos).max())          # the fp16 backbone against the fp32 module forward
        c = m.model.classifier
        hw = (c.dense.weight.half(), c.dense.bias.half(), c.out_proj.weight.half().reshape(-1), c.out_proj.bias.half())
        want, _ = head_reference(cls32, *hw)                     # the fp32 module backbone, its head in fp64
        _, head_bound = head_reference(cls16, *hw)               # the kernel's own rounding on the rows it was given
        # tolerance: the two backbones' difference pushed through the head (tanh 1-Lipschitz, sigmoid 1/4-Lipschitz) + the head's rounding
        dz = ((cls16 - cls32) @ hw[0].double().T).abs()
        tol = (0.25 * (dz @ hw[2].double().abs())).cpu().numpy() + head_bound + 1e-9
    err = np.abs(got - want)
    assert (err <= tol).all(), (spec, float((err / tol).max()), float(err.max()))
    T = float(tol.max())
    assert T <= 0.1 and np.ptp(want) > 0.3, (T, np.ptp(want))
    idx = np.argsort(-want, kind="stable")
    for a, b in zip(idx[:-1], idx[1:]):
        if want[a] - want[b] > 2 * T:
            assert got[a] > got[b]
    return T


def test_end_to_end_mid_fused_both_attention_paths():
    rng = np.random.default_rng(3)
    T1 = check_end_to_end("mid", [int(x) for x in rng.integers(10, 513, 40)], "fused", seed=1)        # > 64 tokens: MFMA attention
    T2 = check_end_to_end("mid", [int(x) for x in rng.integers(10, 65, 12)], "fused", seed=2)         # all <= 64: VALU attention
    print(f"mid: score tolerance {T1:.2e} (mixed lengths), {T2:.2e} (short)")


def test_end_to_end_xlm_roberta_large_fused():
    rng = np.random.default_rng(4)
    T = check_end_to_end("xlm-roberta-large", [int(x) for x in rng.integers(10, 513, 40)], "fused", seed=3)
    print(f"xlm-roberta-large: score tolerance {T:.2e}")


def test_end_to_end_xlm_roberta_base_module_backbone_with_head_kernels():
    rng = np.random.default_rng(5)
    T = check_end_to_end("xlm-roberta-base", [int(x) for x in rng.integers(10, 513, 24)], "module+kernels", seed=4)
    print(f"xlm-roberta-base: score tolerance {T:.2e}")


def test_fake_model_on_gpu_equals_cpu_result():
    for case, gold in zip(W.cases(), GOLDEN["cases"]):
        check_against_gold(case, gold, *run_case(case, gold, device="cuda"))


def test_retrieve_reranked_equals_its_parts():
    from rag_dpo_amd.collection import Collection
    from rag_dpo_amd.retriever import DenseRetriever, documents_from_ranked_chunks

    rng = np.random.default_rng(9)
    n, d = 300, 64
    emb = rng.standard_normal((n, d)).astype(np.float32)
    col = Collection("rerank_test", metadata={"hnsw:space": "cosine"})
    col.add(ids=[f"chunk_{i}" for i in range(n)], embeddings=emb, documents=[f"texte {i} conservation" for i in range(n)],
            metadatas=[{"document_path": f"doc_{i % 23}", "chunk_nature": ["GUIDE", "DOCTRINE"][(i % 23) % 2], "chunk_index": i // 23,
                        "rgpd_topics": "cookies" if i % 5 == 0 else ""} for i in range(n)])

    class Provider:
        def embed(self, texts):
            return [list(np.random.default_rng(zlib.crc32(t.encode())).standard_normal(d)) for t in texts]

    class Model:
        def predict(self, pairs, batch_size=32, show_progress_bar=True):
            return np.asarray([(zlib.crc32(p[1].encode()) % 1000) / 1000.0 for p in pairs], dtype=np.float32)

    class Boost:
        def topic_boost(self, topics, tags):
            return 0.15 if tags == "cookies" else 0.0

    ret = DenseRetriever(col, Provider())
    gpu = RR.CrossEncoderReranker(device="cuda")
    cpu = RR.CrossEncoderReranker(device="cpu")
    gpu._model = cpu._model = Model()
    got = ret.retrieve_reranked("durée de conservation", gpu, n_candidates=40, top_k=10, topic_matcher=Boost(), question_topics=["cookies"])
    cands = ret.retrieve_candidates("durée de conservation", n_candidates=40)
    want = documents_from_ranked_chunks(cpu.rerank("durée de conservation", cands, top_k=10, topic_matcher=Boost(), question_topics=["cookies"]))
    assert len(cands) == 40 and got == want and sum(len(x.chunks) for x in got) == 10
