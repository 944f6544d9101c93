"""GPU: rdx_lex_reduce (csrc/lex_kernel.hpp k_lex_reduce) against the numpy model of rag_dpo_amd/lexical.py, on bits: token ids as int32,
weights as the uint16 bits of their fp16 value, counts, and every word of the outputs the kernel must not touch."""
import numpy as np
import pytest
import torch

import lexical_world as LW
from rag_dpo_amd import engine
from rag_dpo_amd import lexical as LX

pytestmark = pytest.mark.gpu

VOCAB = 250002
SKIP = (0, 1, 2, 3)
LENGTHS = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 8192]
CANARY_TOK, CANARY_W, PAD = -77, 0x7E55, 64        # 0x7E55 is a NaN: the kernel never writes one


def text(n, rng, kind="mixed"):
    """-> (ids int32 [n], fp32 weights [n])"""
    if kind == "repeated":
        tok = np.full(n, 4242, np.int32)
    elif kind == "distinct":
        tok = rng.permutation(np.arange(4, 4 + n)).astype(np.int32)
    elif kind == "special":
        tok = rng.integers(0, 4, n).astype(np.int32)
    else:   # duplicates, specials, the smallest and the largest admitted ids
        tok = rng.choice(np.concatenate([np.arange(0, 40), [VOCAB - 1, VOCAB - 2, 4]]), size=n).astype(np.int32)
    w = rng.standard_normal(n).astype(np.float32) * rng.choice([1e-7, 1e-3, 1.0, 300.0, 1e5], size=n).astype(np.float32)
    return tok, w


def run(texts, vocab=VOCAB, skip=SKIP):
    """the kernel on the texts, outputs pre-filled with canaries and padded on both sides -> (out_tok, out_w bits, out_n) numpy, checked
    against the model word for word"""
    off = np.zeros(len(texts) + 1, np.int64)
    np.cumsum([len(t[0]) for t in texts], out=off[1:])
    T = int(off[-1])
    tok = np.concatenate([t[0] for t in texts]).astype(np.int32) if T else np.zeros(0, np.int32)
    w = np.concatenate([t[1] for t in texts]).astype(np.float32) if T else np.zeros(0, np.float32)
    want_tok, want_w, want_n = np.full(T, CANARY_TOK, np.int32), np.full(T, CANARY_W, np.uint16), np.zeros(len(texts), np.int32)
    for i in range(len(texts)):
        try:
            a, b = LX.terms_model(tok[off[i]:off[i + 1]], w[off[i]:off[i + 1]], vocab, skip)
        except ValueError:
            want_n[i] = -1
            continue
        want_n[i] = len(a)
        want_tok[off[i]:off[i] + len(a)] = a
        want_w[off[i]:off[i] + len(a)] = b.view(np.uint16)
    big_tok = torch.full((T + 2 * PAD,), CANARY_TOK, dtype=torch.int32, device="cuda")
    big_w = torch.full((T + 2 * PAD,), CANARY_W, dtype=torch.int16, device="cuda").view(torch.float16)
    big_n = torch.full((len(texts) + 2 * PAD,), -99, dtype=torch.int32, device="cuda")
    off_p = torch.from_numpy(off).pin_memory()
    engine.lex_reduce(torch.from_numpy(tok).cuda(), torch.from_numpy(w).cuda(), off_p, vocab, skip,
                      big_tok[PAD:PAD + T], big_w[PAD:PAD + T], big_n[PAD:PAD + len(texts)])
    torch.cuda.synchronize()
    g_tok, g_w, g_n = big_tok.cpu().numpy(), big_w.view(torch.int16).cpu().numpy().view(np.uint16), big_n.cpu().numpy()
    for g, canary in ((g_tok, CANARY_TOK), (g_w, CANARY_W), (g_n, -99)):                # around the arrays
        assert (g[:PAD] == np.array(canary).astype(g.dtype)).all() and (g[len(g) - PAD:] == np.array(canary).astype(g.dtype)).all()
    g_tok, g_w, g_n = g_tok[PAD:PAD + T], g_w[PAD:PAD + T], g_n[PAD:PAD + len(texts)]
    assert g_n.tolist() == want_n.tolist()
    assert np.array_equal(g_tok, want_tok) and np.array_equal(g_w, want_w)            # the terms, and the canaries past each out_n[i]
    return g_tok, g_w, g_n


def test_every_length_in_order_and_shuffled():
    rng = np.random.default_rng(0)
    texts = [text(n, rng) for n in LENGTHS]
    _, _, n = run(texts)
    assert n[0] == 0 and n[-1] > 30
    order = rng.permutation(len(texts))
    run([texts[i] for i in order])
    run(texts[:9])                                                                       # the narrow workgroup: no text above 1024 tokens


def test_token_and_id_cases():
    rng = np.random.default_rng(1)
    for n in (1, 65, 1025, 8192):
        tok, w = text(n, rng, "repeated")
        _, _, cnt = run([(tok, np.abs(w) % np.float32(60000) + np.float32(1e-3))])
        assert cnt.tolist() == [1]
        tok, w = text(n, rng, "distinct")
        _, _, cnt = run([(tok, np.abs(w) % np.float32(60000) + np.float32(1e-3))])
        assert cnt.tolist() == [n]                                                       # every token its own term
        _, _, cnt = run([text(n, rng, "special")])
        assert cnt.tolist() == [0]
    got_tok, _, cnt = run([(np.array([VOCAB - 1, 4, VOCAB - 1, 4], np.int32), np.array([1, 2, 3, 0.5], np.float32))])
    assert cnt.tolist() == [2] and got_tok[:2].tolist() == [4, VOCAB - 1]
    # other skip ids, eight of them; none at all; a small vocabulary
    run([text(300, rng)], skip=(5, 6, 7, 8, 9, 10, 11, VOCAB - 1))
    run([text(300, rng)], skip=())
    with pytest.raises(ValueError, match="n_skip"):
        run([text(3, rng)], skip=tuple(range(9)))


def test_rounding_edges():
    edges = [w for w, _ in LW.ROUNDING_EDGES]
    tok = np.arange(100, 100 + len(edges), dtype=np.int32)
    got_tok, got_w, cnt = run([(tok, np.array(edges, np.float32))])
    kept = [(100 + i, b) for i, (_, b) in enumerate(LW.ROUNDING_EDGES) if b is not None]
    assert cnt.tolist() == [len(kept)] and list(zip(got_tok[:len(kept)].tolist(), got_w[:len(kept)].tolist())) == kept
    # an edge inside a run of one id: the maximum is over the rounded, kept weights
    run([(np.full(4, 9, np.int32), np.array([70000.0, 1 + 2.0 ** -11, 1.0, np.nan], np.float32)),
         (np.full(3, 9, np.int32), np.array([2.0 ** -25, -0.0, np.nextafter(np.float32(2.0 ** -25), np.float32(1))], np.float32))])


def test_duplicates_whose_maximum_is_first_middle_and_last():
    tok = np.array([5, 7, 5, 9, 0, 7, 9, 5, 2, 7, 11, 9, 12], np.int32)
    w = np.array([0.5, 0.25, 0.25, 0.125, 3.0, 1.0, 0.25, 0.125, 4.0, 0.5, 0.0, 2.0, -1.0], np.float32)
    got_tok, got_w, cnt = run([(tok, w)])
    assert cnt.tolist() == [3] and got_tok[:3].tolist() == [5, 7, 9] and got_w[:3].tolist() == [int(LW.f16(x)) for x in (0.5, 1.0, 2.0)]
    rng = np.random.default_rng(2)
    for where in (0, 500, 999):                                                          # the same in a long run
        w = rng.random(1000).astype(np.float32)
        w[where] = 7.0
        got_tok, got_w, cnt = run([(np.full(1000, 31, np.int32), w)])
        assert cnt.tolist() == [1] and got_w[0] == LW.f16(7.0)


def test_an_id_outside_the_vocabulary_costs_its_text_alone():
    rng = np.random.default_rng(3)
    texts = [text(n, rng) for n in (300, 700, 65)]
    good = run(texts)
    for bad_id in (VOCAB, -1, 2 ** 31 - 1):
        tok, w = texts[1][0].copy(), texts[1][1]
        tok[350] = bad_id
        got = run([texts[0], (tok, w), texts[2]])
        assert got[2].tolist() == [good[2][0], -1, good[2][2]]
        assert np.array_equal(got[0][:300], good[0][:300]) and np.array_equal(got[0][1000:], good[0][1000:])
        assert np.array_equal(got[1][:300], good[1][:300]) and np.array_equal(got[1][1000:], good[1][1000:])
        assert (got[0][300:1000] == CANARY_TOK).all()                                    # the refused text writes nothing
    tok, w = text(50, rng)
    tok[49] = 40
    assert run([(tok, w), texts[2]], vocab=40)[2][0] == -1                               # vocab is the call's: 40 is outside a vocabulary of 40


def test_refused_before_launch():
    rng = np.random.default_rng(4)
    tok, w = text(8193, rng)
    out = [torch.full((8193,), CANARY_TOK, dtype=torch.int32, device="cuda"), torch.zeros(8193, dtype=torch.float16, device="cuda"),
           torch.full((1,), -99, dtype=torch.int32, device="cuda")]
    args = (torch.from_numpy(tok).cuda(), torch.from_numpy(w).cuda())
    with pytest.raises(ValueError, match="text 0 has 8193 tokens"):
        engine.lex_reduce(*args, torch.tensor([0, 8193]).pin_memory(), VOCAB, SKIP, *out)
    with pytest.raises(ValueError, match="pinned host memory"):
        engine.lex_reduce(*args, torch.tensor([0, 100]), VOCAB, SKIP, *out)                # pageable
    with pytest.raises(ValueError, match="behind n_tok"):
        engine.lex_reduce(args[0][:50], args[1][:50], torch.tensor([0, 100]).pin_memory(), VOCAB, SKIP, *out)
    with pytest.raises(ValueError, match="must not decrease"):
        engine.lex_reduce(*args, torch.tensor([0, 100, 50]).pin_memory(), VOCAB, SKIP, out[0], out[1], torch.zeros(2, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    assert (out[0] == CANARY_TOK).all() and out[2].tolist() == [-99]
    # no texts: nothing to do
    engine.lex_reduce(args[0][:0], args[1][:0], torch.zeros(1, dtype=torch.int64).pin_memory(), VOCAB, SKIP)
