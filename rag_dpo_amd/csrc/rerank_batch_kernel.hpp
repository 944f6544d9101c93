// rerank_batch_kernel.hpp — the reranker's topic boost and selection for a BATCH of questions in one pass (gfx950): what
// rdx_topic_boost (topic_kernel.hpp) and rdx_rerank_select (rerank_kernel.hpp) do for one question, done for nq questions whose
// candidates lie side by side on one axis. Question q is the segment [cand_off[q], cand_off[q + 1]) of that axis; a segment may be
// empty and holds at most 1024 candidates. The head needs no kernel of its own: k_rerank_head and k_rerank_combine index rows
// with size_t and take any n their grid can hold, and a row's arithmetic in them never depended on n (rdx_rerank_head_rows_f16).
//
// The arithmetic is shared, not repeated: topic_sim_wave, topic_replay_one and rerank_select_segment are the cores the
// single-question kernels call; a kernel here only finds its question's operands. A question's outputs are therefore the bits
// and integers of the single-question call on that question alone, whatever its neighbours are.
//
// The shape arrays (cand_off, topic_off, tag_off, sim_off) are read by the launcher on the host, which checks them and sizes the
// grids, and by the kernels through the same words: they live in pinned host memory. A workgroup reads the handful of words of
// its own question, nothing else.
//
// Similarities (K_B1): grid (ceil(max_q T_q U_q / 4), nq), one wave per (q, topic, tag); a workgroup past its question's T_q U_q
//   leaves at once.
// Replay (K_B2): grid (ceil(longest segment / 256), nq), one thread per candidate.
// Selection (K_B3<W>): grid nq, one workgroup of W threads per question, thread p = candidate p of the segment. W is the
//   smallest of RERANK_BATCH_WIDTHS (64, 256, 1024) that holds the call's longest segment: at the reference's 40 candidates a
//   question is one wave instead of sixteen, fifteen of which would only meet barriers. The rank loop reads the segment's finals
//   from LDS (8 W bytes).
// No atomics anywhere: the same inputs give the same bits on every call, on any stream.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rerank_kernel.hpp"
#include "topic_kernel.hpp"

namespace rdx {

constexpr int64_t RERANK_BATCH_MAX_ROWS = (int64_t)1 << 20;   // candidates per call (the header's RDX_RERANK_BATCH_MAX_ROWS)
constexpr int RERANK_BATCH_MAX_QUESTIONS = 65535;             // questions per call: the y extent of a grid
constexpr int RERANK_BATCH_WIDTHS[3] = {64, 256, 1024};       // K_B3's compiled workgroup widths

// K_B1: k_topic_sims for question blockIdx.y: sims + sim_off[q] is its [T_q][U_q] block
__global__ void __launch_bounds__(TOPIC_THREADS) k_topic_sims_batch(const float* __restrict__ table, int64_t rows, int dim,
                                                                   const int32_t* __restrict__ topic_off, const int32_t* __restrict__ topic_slots,
                                                                   const int32_t* __restrict__ tag_off, const int32_t* __restrict__ tag_slots,
                                                                   const int64_t* __restrict__ sim_off, double* __restrict__ sims) {
    const int q = blockIdx.y;
    const int t0 = topic_off[q], T = topic_off[q + 1] - t0;
    const int u0 = tag_off[q], U = tag_off[q + 1] - u0;
    const int64_t pair = (int64_t)blockIdx.x * (TOPIC_THREADS / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (pair >= (int64_t)T * U) return;                                  // (whole waves: pair is uniform in a wave)
    const double s = topic_sim_wave(table, rows, dim, topic_slots[t0 + pair / U], tag_slots[u0 + pair % U], lane);
    if (lane == 0) sims[sim_off[q] + pair] = s;
}

// K_B2: k_topic_replay for candidate blockIdx.x * 256 + threadIdx.x of question blockIdx.y. A question without topics or without
// tags has no similarities (T = U = 0 below, as rdx_topic_boost passes them): only exact pairs can lift its best
__global__ void __launch_bounds__(TOPIC_THREADS) k_topic_replay_batch(const double* __restrict__ sims, const int32_t* __restrict__ topic_off,
                                                                     const int32_t* __restrict__ tag_off, const int64_t* __restrict__ sim_off,
                                                                     const int32_t* __restrict__ cand_off, const int64_t* __restrict__ pair_off,
                                                                     const int32_t* __restrict__ pairs, int64_t n_pairs, double threshold,
                                                                     double max_boost, double* __restrict__ boosts, double* __restrict__ best_sim) {
    const int q = blockIdx.y;
    const int c0 = cand_off[q], n = cand_off[q + 1] - c0;
    const int local = blockIdx.x * TOPIC_THREADS + threadIdx.x;
    if (local >= n) return;
    int T = topic_off[q + 1] - topic_off[q], U = tag_off[q + 1] - tag_off[q];
    if (T <= 0 || U <= 0) T = U = 0;
    const int64_t c = (int64_t)c0 + local;
    const int64_t lo = max(pair_off[c], (int64_t)0), hi = min(pair_off[c + 1], n_pairs);
    topic_replay_one(sims + sim_off[q], T, U, pairs, lo, hi, threshold, max_boost, boosts + c, best_sim ? best_sim + c : nullptr);
}

// K_B3: k_rerank_select for the segment of question blockIdx.x, W >= its length. No thread leaves before the core's barriers.
template <int W>
__global__ void __launch_bounds__(W) k_rerank_select_batch(const float* __restrict__ scores, const double* __restrict__ boosts,
                                                          const int32_t* __restrict__ cand_off, int top_k, double min_score, int keep_min,
                                                          int32_t* __restrict__ order, double* __restrict__ final_out,
                                                          int32_t* __restrict__ count, int32_t* __restrict__ boosted) {
    const int seg = blockIdx.x;
    const int c0 = cand_off[seg];
    const int n = min(cand_off[seg + 1] - c0, W);                        // (the launcher refused a longer segment)
    rerank_select_segment<W>(scores + c0, boosts ? boosts + c0 : nullptr, n, top_k, min_score, keep_min, order + c0, final_out + c0,
                             count + seg, boosted ? boosted + seg : nullptr);
}

}  // namespace rdx
