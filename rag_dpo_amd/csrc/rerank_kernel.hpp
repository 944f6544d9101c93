// rerank_kernel.hpp — the cross-encoder reranker's classification head and candidate selection (gfx950). Serves the reference's
// CrossEncoderReranker.rerank (src/rag/reranker.py:112-216): sentence-transformers' CrossEncoder.predict on an
// XLMRobertaForSequenceClassification checkpoint with one label ends in
//     z = W_d h + b_d,  t = tanh(z),  logit = w_o . t + b_o,  score = sigmoid(logit)
// on the final hidden state h of each pair's <s> token; rerank then adds the topic boost, sorts and filters.
//
// Head (K_R1 + K_R2). W_d is [H][H] fp16, row f = output feature f: the 8 rows of a feature block are contiguous, so workgroup
// (feature block b, row block y) stages its 16 * H bytes of W_d in LDS once and every one of its rows reads them from there. With
// n <= RERANK_ROWS_PER_BLOCK pairs (the reference's 40) each byte of W_d leaves HBM once. Per (row, feature) the dot product is
// fp32: lane l accumulates k = l, l + 64, ... with fmaf in that order, the 64 lane sums are combined by a fixed xor butterfly.
// The block's partial logit sum_f w_o[f] * tanh(z_f) is fp64 (tanh in fp64), written to a caller-provided workspace
// [H / 8][n]; K_R2 (one wave per row) adds the H / 8 partials of a row in a fixed order, then b_o, and applies the sigmoid in fp64,
// rounded once to fp32. No atomics anywhere: the same inputs give the same bits on every call, on any stream.
//
// Selection (rerank_select_segment: K_R3, one workgroup, n <= 1024). final[p] = (double)score[p] (+ boost[p] when boost[p] > 0: one fp64 add, as
// `float(np.float32) + boost` in the reference); rank[p] = #{q : final[q] > final[p] or (final[q] == final[p] and q < p)} —
// Python's stable sort(reverse=True); NaN finals rank after every number (Python's sort leaves them where the comparisons
// happen to put them: undefined there). order[rank[p]] = p. count = min(top_k, #{final >= min_score}), raised to keep_min
// when it is below and n >= keep_min (reranker.py:201-206: the "keep at least 3" fallback, applied even when top_k < 3).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rdx {

constexpr int RERANK_FEATURES = 8;          // output features per head workgroup (= the header's RDX_RERANK_WORKSPACE_BYTES)
constexpr int RERANK_ROWS_PER_BLOCK = 64;   // pairs per head workgroup; more pairs add row blocks (W_d re-read per row block)
constexpr int RERANK_THREADS = 256;        // K_R2
constexpr int RERANK_HEAD_THREADS = 512;   // K_R1: 8 waves, two rows each per step
constexpr int RERANK_KU = 16;              // K_R1: loads of a row in flight per lane (H <= 1024: the whole row at once)
constexpr int RERANK_MAX_N = 1024;
constexpr int RERANK_MAX_HIDDEN = 4096;

// K_R1: grid (H / 8, ceil(n / 64)), 512 threads, dynamic LDS 16 * H bytes (the block's W_d rows). A wave takes two rows at a time and
// issues RERANK_KU loads of each before it uses one: the x rows come from L2/HBM. (The first version, one row per wave, a load waited
// for in every k-step and a combine that summed the H / 8 partials of a row in one thread, measured ~125 us for head + select at
// 40 pairs and H = 1024: latency, not work.)
__global__ void __launch_bounds__(RERANK_HEAD_THREADS) k_rerank_head(const float* __restrict__ cls, int n, int H,
                                                                    const _Float16* __restrict__ wd, const _Float16* __restrict__ bd,
                                                                    const _Float16* __restrict__ wo, double* __restrict__ part) {
    extern __shared__ __align__(16) unsigned char rerank_lds[];
    _Float16* w = reinterpret_cast<_Float16*>(rerank_lds);
    __shared__ float z[RERANK_FEATURES][RERANK_ROWS_PER_BLOCK];
    const int f0 = blockIdx.x * RERANK_FEATURES;
    const int r0 = blockIdx.y * RERANK_ROWS_PER_BLOCK;
    const int rows = min(RERANK_ROWS_PER_BLOCK, n - r0);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int WAVES = RERANK_HEAD_THREADS / 64;

    // the 8 contiguous rows f0..f0+7 of W_d: 16 * H bytes, as 16-byte words
    const uint4* src = reinterpret_cast<const uint4*>(wd + (size_t)f0 * H);
    uint4* dst = reinterpret_cast<uint4*>(w);
    for (int i = tid; i < H; i += RERANK_HEAD_THREADS) dst[i] = src[i];   // (8 * H halves = H words of 8 halves)
    __syncthreads();

    for (int lr0 = 2 * wave; lr0 < rows; lr0 += 2 * WAVES) {
        const bool two = lr0 + 1 < rows;
        const float* x0 = cls + (size_t)(r0 + lr0) * H;
        const float* x1 = two ? x0 + H : x0;                              // (no second row: row 0 again, its sums are dropped)
        float a0[RERANK_FEATURES], a1[RERANK_FEATURES];
#pragma unroll
        for (int f = 0; f < RERANK_FEATURES; ++f) a0[f] = a1[f] = 0.0f;
        for (int k0 = 0; k0 < H; k0 += 64 * RERANK_KU) {
            float v0[RERANK_KU], v1[RERANK_KU];
#pragma unroll
            for (int u = 0; u < RERANK_KU; ++u) {
                const int k = k0 + 64 * u + lane;
                v0[u] = k < H ? x0[k] : 0.0f;
                v1[u] = k < H ? x1[k] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < RERANK_KU; ++u) {
                const int k = k0 + 64 * u + lane;
                if (k < H) {                                                // (H % 64 == 0: the whole wave agrees)
#pragma unroll
                    for (int f = 0; f < RERANK_FEATURES; ++f) {
                        const float wf = (float)w[f * H + k];
                        a0[f] = fmaf(wf, v0[u], a0[f]);                     // per lane: k ascending, one fma each
                        a1[f] = fmaf(wf, v1[u], a1[f]);
                    }
                }
            }
        }
#pragma unroll
        for (int f = 0; f < RERANK_FEATURES; ++f) {
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                a0[f] += __shfl_xor(a0[f], m, 64);
                a1[f] += __shfl_xor(a1[f], m, 64);
            }
        }
        if (lane == 0) {
#pragma unroll
            for (int f = 0; f < RERANK_FEATURES; ++f) {
                z[f][lr0] = a0[f] + (float)bd[f0 + f];
                if (two) z[f][lr0 + 1] = a1[f] + (float)bd[f0 + f];
            }
        }
    }
    __syncthreads();
    if (tid < rows) {
        double p = 0.0;
#pragma unroll
        for (int f = 0; f < RERANK_FEATURES; ++f) p += (double)(float)wo[f0 + f] * tanh((double)z[f][tid]);
        part[(size_t)blockIdx.x * n + r0 + tid] = p;
    }
}

// K_R2: one wave per row: scores[r] = sigmoid(sum_b part[b][r] + b_o). Lane l adds the partials b = l, l + 64, ... in that order, the 64
// lane sums meet in a fixed xor butterfly (every lane then holds the same bits), lane 0 adds b_o
__global__ void __launch_bounds__(RERANK_THREADS) k_rerank_combine(const double* __restrict__ part, int n, int blocks,
                                                                  const _Float16* __restrict__ bo, float* __restrict__ scores) {
    const int r = blockIdx.x * (RERANK_THREADS / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= n) return;                                                     // (whole waves: r is uniform in a wave)
    double s = 0.0;
    for (int b = lane; b < blocks; b += 64) s += part[(size_t)b * n + r];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    if (lane == 0) {
        s += (double)(float)bo[0];
        scores[r] = (float)(1.0 / (1.0 + exp(-s)));
    }
}

// strict "a comes before b" of the selection order for two finals of DIFFERENT candidates, a's index below b's when
// a_first: a number before NaN, then descending, then input order
__device__ __forceinline__ bool rerank_before(double a, double b, bool a_first) {
    const bool na = a != a, nb = b != b;
    if (na || nb) return nb && (!na || a_first);
    return a > b || (a == b && a_first);
}

// The selection of one segment of n <= W candidates by a workgroup of W threads, thread p = candidate p (K_R3's arithmetic above).
// The pointers are already advanced to the segment; order holds indices local to it. boosted (nullptr, or where to count the
// candidates a boost lifted) is uniform in the workgroup. Every thread of the workgroup must call this: it holds barriers.
template <int W>
__device__ __forceinline__ void rerank_select_segment(const float* __restrict__ scores, const double* __restrict__ boosts, int n, int top_k,
                                                      double min_score, int keep_min, int32_t* __restrict__ order,
                                                      double* __restrict__ final_out, int32_t* count, int32_t* boosted) {
    __shared__ double fin[W];
    const int p = threadIdx.x;
    double f = 0.0;
    bool lifted = false;
    if (p < n) {
        f = (double)scores[p];
        if (boosts) {
            const double b = boosts[p];
            if (b > 0.0) {
                f += b;
                lifted = true;
            }
        }
        fin[p] = f;
        final_out[p] = f;
    }
    const int passing = __syncthreads_count(p < n && f >= min_score);   // (also the barrier behind the fin[] stores)
    const int lifts = boosted ? __syncthreads_count(lifted) : 0;         // (boosted is uniform: every thread takes the same side)
    if (p < n) {
        int rank = 0;
        for (int q = 0; q < n; ++q) rank += (q != p && rerank_before(fin[q], f, q < p)) ? 1 : 0;
        order[rank] = p;
    }
    if (p == 0) {
        int c = min(top_k, passing);
        if (c < keep_min && n >= keep_min) c = keep_min;
        *count = c;                                                      // (0 for an empty segment: top_k and keep_min are >= 0, the launchers see to it)
        if (boosted) *boosted = lifts;
    }
}

// K_R3: one workgroup of 1024 threads over the call's n candidates
__global__ void __launch_bounds__(RERANK_MAX_N) k_rerank_select(const float* __restrict__ scores, const double* __restrict__ boosts,
                                                               int n, int top_k, double min_score, int keep_min,
                                                               int32_t* __restrict__ order, double* __restrict__ final_out,
                                                               int32_t* __restrict__ count) {
    rerank_select_segment<RERANK_MAX_N>(scores, boosts, n, top_k, min_score, keep_min, order, final_out, count, nullptr);
}

}  // namespace rdx
