"""A/B of librdx's encoder GEMM (rdx_enc_gemm_f16, csrc/enc_gemm.hpp) against the BLAS path it can replace, ONE process,
device events around HIP-graph replays, the two arms alternated round by round, warmed; seeded random operands (zero-filled ones read high).

  shapes   per projection shape (N, K) and token count T: F.linear (the parent path's GEMM: bias in its epilogue) beside rdx_enc_gemm_f16
           epilogue 0, and with the epilogue the encoder runs on that shape; kernel microseconds (median and minimum over the rounds) and TFLOP/s = 2 T N K / time.
  layer    one encoder layer's token-wise work at the same T: parent = four F.linear + torch GELU + two rdx_enc_add_layernorm_f16; new =
           four rdx_enc_gemm_f16 (epilogues 0, 2, 1, 2) + two rdx_enc_layernorm_f16 (attention is the same kernel in both and left out:
           the O projection reads a random ctx). Reports the ratio new / parent and the lowest T at which new is not slower.
  e2e      EmbeddingProvider.embed_device alternating gemm="blas" and "rdx" (GEMM_MIN_TOKENS 33): the c5 encode (1024 questions) in ms,
           XLM-R-large, random-init fp16. (Ingest: tools/ingest_bench.py with RDX_ENC_GEMM=rdx RDX_ENC_GEMM_MIN=33 against the default.)
  trace    a few rdx_enc_gemm_f16 launches of every shape at T = 21 504 and nothing else: run it under rocprofv3 --kernel-trace --stats.

  python tools/enc_gemm_bench.py shapes|layer|e2e|trace [--rounds R] [--out FILE]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from rag_dpo_amd import _lib

SHAPES = [("qkv", 3072, 1024), ("o", 1024, 1024), ("ffn_up", 4096, 1024), ("ffn_down", 1024, 4096)]
TOKENS = [257, 1000, 4096, 20649, 21504, 30720]
EPI = {"qkv": 0, "o": 2, "ffn_up": 1, "ffn_down": 2}     # the epilogue the encoder runs behind each projection
F = torch.nn.functional


def rnd(gen, *shape, scale=1.0):
    return (torch.randn(*shape, generator=gen, device="cuda", dtype=torch.float32) * scale).to(torch.float16)


def ab(arms: dict, rounds: int, inner: int):
    """{name: fn} -> {name: (median us, min us)} per call. Every arm is warmed, then captured `inner` times back to back into a HIP graph
    (the provider replays its forwards the same way; an eager loop of 10 - 20 us kernels times the host's enqueue, not the GPU), and
    the graphs are replayed `rounds` times, the arms alternated inside each round, device events around each replay."""
    graphs = {}
    side = torch.cuda.Stream()
    for k, fn in arms.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        side.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for _ in range(inner):
                fn()
        torch.cuda.current_stream().wait_stream(side)
        g.replay()
        graphs[k] = g
    torch.cuda.synchronize()
    t = {k: [] for k in arms}
    for _ in range(rounds):
        for k, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            e1.synchronize()
            t[k].append(e0.elapsed_time(e1) * 1e3 / inner)
    return {k: (float(np.median(v)), float(np.min(v))) for k, v in t.items()}


class Lib:
    def __init__(self):
        self.L = _lib.load()

    def gemm(self, x, w, b, epi, out, res=None):
        rc = self.L.rdx_enc_gemm_f16(0, x.data_ptr(), w.data_ptr(), b.data_ptr(), res.data_ptr() if res is not None else None, x.shape[0],
                                     w.shape[0], w.shape[1], epi, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, _lib.last_error()
        return out

    def ln(self, s, g, b, out):
        rc = self.L.rdx_enc_layernorm_f16(0, s.data_ptr(), g.data_ptr(), b.data_ptr(), 1e-5, s.shape[0], s.shape[1], out.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream)
        assert rc == 0, _lib.last_error()
        return out

    def add_ln(self, a, r, g, b, out):
        rc = self.L.rdx_enc_add_layernorm_f16(0, a.data_ptr(), r.data_ptr(), g.data_ptr(), b.data_ptr(), 1e-5, a.shape[0], a.shape[1],
                                              out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, _lib.last_error()
        return out


def inner_for(T):
    return 20 if T <= 4096 else 6


def run_shapes(rounds, emit):
    lib, gen = Lib(), torch.Generator(device="cuda").manual_seed(2026)
    emit("per shape: F.linear (BLAS, bias epilogue) | rdx_enc_gemm_f16 epilogue 0; us = median (min) over %d alternated rounds; random N(0,1) x, N(0,1/K) W" % rounds)
    emit(f"{'shape':9s} {'N':>5s} {'K':>5s} {'T':>6s} | {'blas us':>16s} {'TF':>7s} | {'rdx us':>16s} {'TF':>7s} | rdx/blas  tile")
    for name, N, K in SHAPES:
        w, b = rnd(gen, N, K, scale=K ** -0.5), rnd(gen, N, scale=0.1)
        for T in TOKENS:
            x = rnd(gen, T, K)
            out = torch.empty((T, N), dtype=torch.float16, device="cuda")
            ref = F.linear(x, w, b)
            lib.gemm(x, w, b, 0, out)
            torch.cuda.synchronize()
            err = float((out.float() - ref.float()).abs().max())            # same inputs, the sizes that are timed: a few fp16 ulps
            epi = EPI[name]
            res = rnd(gen, T, N) if epi == 2 else None
            arms = {"blas": lambda: F.linear(x, w, b), "rdx": lambda: lib.gemm(x, w, b, 0, out)}
            if epi:
                arms["epi"] = lambda: lib.gemm(x, w, b, epi, out, res=res)       # the epilogue the encoder runs on this shape: its cost beside epilogue 0
            r = ab(arms, rounds, inner_for(T))
            fl = 2.0 * T * N * K
            tile = "128x128" if -(-T // 128) * -(-N // 128) >= 256 else "64x64"
            emit(f"{name:9s} {N:5d} {K:5d} {T:6d} | {r['blas'][0]:8.1f} ({r['blas'][1]:6.1f}) {fl / r['blas'][0] / 1e6:7.1f} | "
                 f"{r['rdx'][0]:8.1f} ({r['rdx'][1]:6.1f}) {fl / r['rdx'][0] / 1e6:7.1f} | {r['rdx'][0] / r['blas'][0]:8.3f}  {tile}  max|diff| {err:.2e}"
                 + (f"  | epilogue {epi}: {r['epi'][0]:8.1f} ({r['epi'][1]:6.1f}) us" if epi else ""))


def run_layer(rounds, emit):
    lib, gen = Lib(), torch.Generator(device="cuda").manual_seed(2027)
    H, I = 1024, 4096
    wqkv, bqkv = rnd(gen, 3 * H, H, scale=H ** -0.5), rnd(gen, 3 * H, scale=0.1)
    wo, bo = rnd(gen, H, H, scale=H ** -0.5), rnd(gen, H, scale=0.1)
    w1, b1 = rnd(gen, I, H, scale=H ** -0.5), rnd(gen, I, scale=0.1)
    w2, b2 = rnd(gen, H, I, scale=I ** -0.5), rnd(gen, H, scale=0.1)
    g, bt = rnd(gen, H, scale=0.1) + 1, rnd(gen, H, scale=0.1)
    emit("per layer (attention left out of both): parent = 4 F.linear + torch GELU + 2 rdx_enc_add_layernorm_f16 | new = 4 rdx_enc_gemm_f16 "
         "(epilogues 0, 2, 1, 2) + 2 rdx_enc_layernorm_f16; us = median (min) over %d alternated rounds" % rounds)
    emit(f"{'T':>6s} | {'parent us':>18s} | {'new us':>18s} | new/parent")
    first_ok = None
    for T in TOKENS:
        x, ctx = rnd(gen, T, H), rnd(gen, T, H)
        bufs = {k: torch.empty((T, n), dtype=torch.float16, device="cuda") for k, n in (("qkv", 3 * H), ("s1", H), ("x1", H), ("f", I), ("s2", H), ("x2", H))}

        def parent():
            F.linear(x, wqkv, bqkv)
            lib.add_ln(F.linear(ctx, wo, bo), x, g, bt, bufs["x1"])
            lib.add_ln(F.linear(F.gelu(F.linear(bufs["x1"], w1, b1)), w2, b2), bufs["x1"], g, bt, bufs["x2"])

        def new():
            lib.gemm(x, wqkv, bqkv, 0, bufs["qkv"])
            lib.ln(lib.gemm(ctx, wo, bo, 2, bufs["s1"], res=x), g, bt, bufs["x1"])
            lib.gemm(bufs["x1"], w1, b1, 1, bufs["f"])
            lib.ln(lib.gemm(bufs["f"], w2, b2, 2, bufs["s2"], res=bufs["x1"]), g, bt, bufs["x2"])

        parent()
        want = bufs["x2"].float().clone()
        new()
        torch.cuda.synchronize()
        err = float((bufs["x2"].float() - want).abs().max())
        r = ab({"parent": parent, "new": new}, rounds, 10 if T <= 4096 else 3)
        ratio = r["new"][0] / r["parent"][0]
        if ratio <= 1.0 and first_ok is None:
            first_ok = T
        emit(f"{T:6d} | {r['parent'][0]:9.1f} ({r['parent'][1]:7.1f}) | {r['new'][0]:9.1f} ({r['new'][1]:7.1f}) | {ratio:8.3f}   max|diff| of the layer output {err:.2e}")
    emit(f"lowest T at which the new path is not slower: {first_ok if first_ok is not None else 'none of the measured token counts'}")


def run_e2e(rounds, emit):
    """the c5 encode. (Ingest end to end is tools/ingest_bench.py itself, run once per arm with RDX_ENC_GEMM=blas / RDX_ENC_GEMM=rdx
    RDX_ENC_GEMM_MIN=33 in the environment, the runs alternated in one call.)"""
    from rag_dpo_amd import synth
    from rag_dpo_amd.embedding_provider import EmbeddingProvider
    import time
    prov = {}
    for gm in ("blas", "rdx"):
        p = EmbeddingProvider(model_name="random-init:xlm-roberta-large", device="cuda:0", dtype=torch.float16, batch_size=1024, gemm=gm).load()
        p._packed.GEMM_MIN_TOKENS = 33
        prov[gm] = p
    qs = synth.query_texts(1024, seed=5)

    def wall(p):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        p.embed_device(qs)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for p in prov.values():
        for _ in range(3):
            wall(p)
    t = {k: [] for k in prov}
    for _ in range(rounds):
        for k, p in prov.items():
            t[k].append(wall(p))
    med = {k: float(np.median(v)) for k, v in t.items()}
    emit(f"c5 encode of 1024 questions ({prov['blas'].last_encode_stats['tokens_real']} real tokens), embed_device, wall incl. synchronise: "
         f"blas {med['blas']:.2f} ms (min {min(t['blas']):.2f}) | rdx {med['rdx']:.2f} ms (min {min(t['rdx']):.2f}) | rdx/blas {med['rdx'] / med['blas']:.3f}")
    a, b = prov["blas"].embed_device(qs[:256]), prov["rdx"].embed_device(qs[:256])
    cos = F.cosine_similarity(a.double(), b.double(), dim=1)
    emit(f"same questions through both providers: max |1 - cos| {float((1 - cos).abs().max()):.2e}")


def run_trace(rounds, emit):
    lib, gen = Lib(), torch.Generator(device="cuda").manual_seed(2028)
    T = 21504
    for name, N, K in SHAPES:
        x, w, b = rnd(gen, T, K), rnd(gen, N, K, scale=K ** -0.5), rnd(gen, N, scale=0.1)
        out, res = torch.empty((T, N), dtype=torch.float16, device="cuda"), rnd(gen, T, N)
        epi = EPI[name]
        for _ in range(rounds):
            lib.gemm(x, w, b, epi, out, res=res)
            F.linear(x, w, b)
    torch.cuda.synchronize()
    emit(f"trace: {rounds} launches of rdx_enc_gemm_f16 and of F.linear per shape at T = {T}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["shapes", "layer", "e2e", "trace"])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("enc_gemm_bench: needs the GPU (no CPU path: a CPU timing says nothing about it)")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    emit(f"# tools/enc_gemm_bench.py {a.mode} --rounds {a.rounds}   device: {torch.cuda.get_device_name(0)}")
    {"shapes": run_shapes, "layer": run_layer, "e2e": run_e2e, "trace": run_trace}[a.mode](a.rounds, emit)
