"""GPU: rdx_maxsim_f16 (csrc/maxsim_kernel.hpp) against the fp64 model on the same fp16 inputs (rag_dpo_amd/late_interaction.py).

The bound, nothing fitted: per dot product the fp32 MFMA accumulation term of tests/enc_reference.py's `linear` (ACC32_REL * sum|q d|: the
same instruction family, the same rule); per question token the largest of those over the slot's tokens (the kernel's maximum is the
exact maximum of its own fp32 dots, each within its term of the model's); for the score their mean plus one fp32 rounding. Exact probes
(one-hot and power-of-two vectors: every dot has one term, every sum is exact) must give the model's bits."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import enc_reference as ER  # noqa: E402

from rag_dpo_amd import late_interaction as LI  # noqa: E402

pytestmark = pytest.mark.gpu

SLOT_TOKENS = (1, 31, 32, 33, 63, 64, 65, 129, 300)
Q_TOKENS = (1, 31, 32, 33, 64, 65, 256)


def lib():
    from rag_dpo_amd import _lib
    return _lib, _lib.load()


class Call:
    """one rdx_maxsim_f16 call assembled from lists of fp16 matrices; `lead` / `tail` rows of `fill` surround the slots in the arena"""

    def __init__(self, questions, slots, pairs, lead=0, tail=0, fill=np.nan, gap=0):
        self.dim = questions[0].shape[1]
        self.questions, self.slots, self.pairs = questions, slots, pairs
        self.q_off = np.zeros(len(questions) + 1, dtype=np.int32)
        np.cumsum([len(q) for q in questions], out=self.q_off[1:])
        rows, start = [np.full((lead, self.dim), fill, dtype=np.float16)], []
        at = lead
        for s in slots:
            start.append(at)
            rows += [s, np.full((gap, self.dim), fill, dtype=np.float16)]
            at += len(s) + gap
        rows.append(np.full((tail, self.dim), fill, dtype=np.float16))
        self.arena = np.concatenate(rows)
        self.start = np.asarray(start, dtype=np.int64)
        self.length = np.asarray([len(s) for s in slots], dtype=np.int32)
        self.pair_q = np.asarray([p[0] for p in pairs], dtype=np.int32)
        self.pair_slot = np.asarray([p[1] for p in pairs], dtype=np.int64)

    def device(self):
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
        return dict(q_vecs=up(np.concatenate(self.questions)), q_off=torch.from_numpy(self.q_off).pin_memory(), d_vecs=up(self.arena),
                    start=up(self.start), length=up(self.length), pair_q=up(self.pair_q), pair_slot=up(self.pair_slot))

    def run(self, extra=0, stream=None, t=None):
        """-> fp32 numpy [n_pairs + extra]: the scores, and `extra` NaN-filled entries behind them the call must leave alone"""
        L, so = lib()
        t = t or self.device()
        n = len(self.pairs)
        st = stream if stream is not None else torch.cuda.current_stream()
        with torch.cuda.stream(st):
            scores = torch.full((n + extra,), float("nan"), dtype=torch.float32, device="cuda")
            rc = so.rdx_maxsim_f16(0, t["q_vecs"].data_ptr(), t["q_off"].data_ptr(), len(self.questions), t["d_vecs"].data_ptr(), t["d_vecs"].shape[0],
                                   t["start"].data_ptr(), t["length"].data_ptr(), len(self.slots), t["pair_q"].data_ptr(), t["pair_slot"].data_ptr(),
                                   n, self.dim, scores.data_ptr(), st.cuda_stream)
        assert rc == 0, L.last_error()
        st.synchronize()
        return scores.cpu().numpy()

    def model(self):
        return np.asarray([LI.maxsim_model(self.questions[q], self.slots[s]) for q, s in self.pairs], dtype=np.float32)


def exact_and_bound(q, d):
    """the fp64 score (not rounded) and the bound on the kernel's fp32 score"""
    q64, d64 = q.astype(np.float64), d.astype(np.float64)
    s = q64 @ d64.T
    dot_bound = ER.ACC32_REL * (np.abs(q64) @ np.abs(d64).T)       # per dot: fp32 MFMA accumulation
    tok_bound = dot_bound.max(axis=1)                              # per question token: the largest over j
    acc = 0.0
    for x in s.max(axis=1):
        acc += float(x)
    exact = acc / len(q)
    other = float(tok_bound.mean())
    return exact, other + ER.U32 * (abs(exact) + other)            # their mean plus one fp32 rounding


def unit16(rng, n, dim):
    v = rng.standard_normal((n, dim))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float16)


@pytest.fixture(scope="module")
def world():
    """per dim: the questions and slots of the shape test, made once"""
    out = {}
    for dim in (32, 64, 96, 1024):
        rng = np.random.default_rng(dim)
        out[dim] = ([unit16(rng, n, dim) for n in Q_TOKENS], [unit16(rng, n, dim) for n in SLOT_TOKENS])
    return out


@pytest.mark.parametrize("which", ["upto32", "all"])               # questions of at most 32 tokens stage 32 LDS rows, longer ones 64
@pytest.mark.parametrize("dim", [32, 64, 96, 1024])                # one 32-dimension step, two, three, 32
def test_shapes_within_the_bound(world, dim, which):
    questions, slots = world[dim]
    if which == "upto32":
        questions = questions[:3]
    pairs = [(q, s) for q in range(len(questions)) for s in range(len(slots))]
    c = Call(questions, slots, pairs, lead=3, tail=5, gap=1)
    got = c.run()
    worst = 0.0
    for (q, s), g in zip(pairs, got):
        exact, bound = exact_and_bound(questions[q], slots[s])
        ratio = abs(float(g) - exact) / bound
        worst = max(worst, ratio)
        assert np.isfinite(g) and ratio <= 1.0, (dim, len(questions[q]), len(slots[s]), float(g), exact, bound, ratio)
    print(f"maxsim dim {dim} {which}: {len(pairs)} pairs, worst err/bound {worst:.3g}")


def onehot(n, dim, col, val):
    m = np.zeros((n, dim), dtype=np.float16)
    m[np.arange(n), col] = val
    return m


@pytest.mark.parametrize("dim", [64, 96])
def test_exact_probes(dim):
    questions, slots, pairs, want = [], [], [], []
    # the winning document token is first, last, or at a tile's last row
    q = onehot(1, dim, 0, 1.0)
    questions.append(q)
    for n, w in ((300, 0), (300, 299), (300, 31), (300, 63), (300, 287), (33, 32), (1, 0)):
        d = onehot(n, dim, 0, 0.25)
        d[w, 0] = 1.0
        pairs.append((0, len(slots)))
        slots.append(d)
        want.append(1.0)
    # the winner for each question token lies in a different wave's tiles (256 tokens: wave w owns tiles w and w + 4), asymmetric values
    q4 = onehot(8, dim, np.arange(8), 1.0)
    d = onehot(256, dim, 40, 0.5)                                  # nobody's column: similarity 0 to every question token
    for i in range(8):
        d[32 * i + (5 * i + 3) % 32] = 0
        d[32 * i + (5 * i + 3) % 32, i] = 2.0 ** -(i + 1)
    questions.append(q4)
    pairs.append((1, len(slots)))
    slots.append(d)
    want.append(sum(2.0 ** -(i + 1) for i in range(8)) / 8)
    # all similarities negative: a padded zero row (33 tokens: 31 padded rows in the second tile; 33 question tokens) must not win
    qn = onehot(33, dim, 0, 1.0)
    dn = onehot(33, dim, 0, -0.5)
    dn[32, 0] = -2.0 ** -8
    dn[7, 0] = -2.0 ** -6
    questions.append(qn)
    pairs.append((2, len(slots)))
    slots.append(dn)
    want.append(-2.0 ** -8)
    pairs.append((0, len(slots) - 1))                              # (one question token against the same slot)
    want.append(-2.0 ** -8)
    c = Call(questions, slots, pairs, lead=2, tail=2, fill=1.0)    # (neighbouring rows of 1.0 would win every probe if they were read)
    got = c.run()
    model = c.model()
    assert model.tolist() == [np.float32(w) for w in want]         # the probes say what they claim, on the model
    assert got.tobytes() == model.tobytes(), (got.tolist(), model.tolist())


def test_isolation_and_the_arena_s_last_row():
    rng = np.random.default_rng(5)
    dim = 96
    questions = [unit16(rng, 40, dim), unit16(rng, 3, dim)]
    slots = [unit16(rng, 65, dim), unit16(rng, 32, dim), unit16(rng, 1, dim)]
    pairs = [(0, 0), (1, 1), (0, 2), (1, 0)]
    runs = [Call(questions, slots, pairs, lead=4, tail=tail, gap=2, fill=fill).run(extra=3)
            for fill, tail in ((np.nan, 4), (60000.0, 4), (np.nan, 0))]       # tail 0 with gap 0 below: a slot ends at the arena's last row
    last = Call(questions, slots, pairs, lead=1, tail=0, gap=0, fill=np.nan)
    assert last.start[-1] + last.length[-1] == last.arena.shape[0]
    runs.append(last.run(extra=3))
    for r in runs:
        assert np.isfinite(r[:4]).all() and np.isnan(r[4:]).all()             # nothing behind n_pairs is written
        assert r[:4].tobytes() == runs[0][:4].tobytes()
    for (q, s), g in zip(pairs, runs[0]):
        exact, bound = exact_and_bound(questions[q], slots[s])
        assert abs(float(g) - exact) <= bound


def test_position_independence():
    rng = np.random.default_rng(6)
    dim = 1024
    questions = [unit16(rng, 30, dim), unit16(rng, 70, dim)]
    slots = [unit16(rng, 300, dim), unit16(rng, 45, dim)]
    alone = Call(questions, slots, [(0, 0)]).run()
    two = Call(questions, slots, [(0, 0), (1, 1)]).run()
    many = Call(questions, slots, [(1, 1)] * 100 + [(1, 0)] * 156 + [(0, 0)])
    t = many.device()
    first = many.run(t=t)
    assert first.shape == (257,)
    assert alone[0].tobytes() == two[0].tobytes() == first[256].tobytes()
    assert len({x.tobytes() for x in first[:100]}) == 1 and len({x.tobytes() for x in first[100:256]}) == 1
    # across two calls and two streams
    assert many.run(t=t).tobytes() == first.tobytes()
    assert many.run(t=t, stream=torch.cuda.Stream()).tobytes() == first.tobytes()
    assert many.run(t=t, stream=torch.cuda.Stream()).tobytes() == first.tobytes()


def test_refusals_and_out_of_range_pairs():
    L, so = lib()
    rng = np.random.default_rng(7)
    dim = 64
    questions = [unit16(rng, 5, dim), unit16(rng, 33, dim)]
    slots = [unit16(rng, 10, dim), unit16(rng, 40, dim)]
    c = Call(questions, slots, [(0, 0), (1, 1)])
    t = c.device()
    scores = torch.full((8,), float("nan"), dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def rc(dim=dim, nq=2, n_pairs=2, q_off=None, rows=None, n_slots=2):
        q_off = t["q_off"] if q_off is None else q_off
        return so.rdx_maxsim_f16(0, t["q_vecs"].data_ptr(), q_off.data_ptr(), nq, t["d_vecs"].data_ptr(), t["d_vecs"].shape[0] if rows is None else rows,
                                 t["start"].data_ptr(), t["length"].data_ptr(), n_slots, t["pair_q"].data_ptr(), t["pair_slot"].data_ptr(), n_pairs,
                                 dim, scores.data_ptr(), st)

    pin = lambda a: torch.tensor(a, dtype=torch.int32).pin_memory()   # noqa: E731
    assert rc() == 0, L.last_error()
    for kw, word in ((dict(dim=0), "dim"), (dict(dim=16), "dim"), (dict(dim=1056), "dim"), (dict(nq=0), "nq"), (dict(nq=65536), "nq"),
                     (dict(n_pairs=0), "n_pairs"), (dict(n_pairs=(1 << 20) + 1), "n_pairs"),
                     (dict(q_off=pin([0, 0, 38])), "token vectors"),           # a question of 0 tokens
                     (dict(q_off=pin([0, 257, 290])), "token vectors"),        # a question of 257 tokens
                     (dict(q_off=pin([-1, 5, 38])), "q_off"),
                     (dict(q_off=torch.tensor([0, 5, 38], dtype=torch.int32).cuda()), "pinned"),      # q_off in device memory
                     (dict(q_off=torch.tensor([0, 5, 38], dtype=torch.int32)), "pinned")):            # pageable host memory
        assert rc(**kw) == L.RDX_ERR_INVALID and word in L.last_error(), (kw, L.last_error())
    torch.cuda.synchronize()
    assert np.isnan(scores.cpu().numpy()[2:]).all()
    # out-of-range pairs: NaN for that pair, the neighbours correct
    good = c.run()
    bad = Call(questions, slots, [(0, 0), (2, 0), (1, 1), (-1, 1), (0, 2), (1, -1), (1, 1)])
    got = bad.run(extra=2)
    assert np.isnan(got[[1, 3, 4, 5]]).all() and np.isnan(got[7:]).all()
    assert got[[0, 2, 6]].tobytes() == good[[0, 1, 1]].tobytes()
    # a slot that reaches outside [0, d_rows), starts below 0, or has no or too many rows
    for start, length in (([0, 15], [10, 40]), ([0, -1], [10, 40]), ([0, 10], [10, 0]), ([0, 10], [10, 8193]), ([0, 1 << 40], [10, 40])):
        e = Call(questions, slots, [(0, 0), (1, 1), (0, 0)])
        te = e.device()
        te["start"], te["length"] = torch.tensor(start, dtype=torch.int64).cuda(), torch.tensor(length, dtype=torch.int32).cuda()
        r = e.run(t=te)
        assert np.isnan(r[1]) and r[[0, 2]].tobytes() == good[[0, 0]].tobytes(), (start, length, r)
