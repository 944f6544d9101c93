// topic_kernel.hpp — the topic boost of a question's candidates (gfx950). Serves the reference's TopicMatcher.topic_boost
// (src/utils/rgpd_topics.py:178-222), which CrossEncoderReranker.rerank calls once per candidate (src/rag/reranker.py:168-176):
//     best = 0.0
//     for topic in question_topics:
//         for tag in chunk_tags:
//             if topic.lower() == tag.lower(): best = 1.0; break
//             sim = dot(embedding(topic), embedding(tag));  if sim > best: best = sim
//         if best >= 1.0: break
//     boost = 0.0 if best < threshold else max_boost * (best - threshold) / (1.0 - threshold)
// The strings stay on the host (rag_dpo_amd/topics.py): it hands over the slots of the call's topics and distinct tags in a table of
// fp32 embeddings [rows][dim], and per candidate the (topic, tag, exact) pairs of the two loops in their order.
//
// Similarities (topic_sim_wave: K_T1, one wave per (topic, tag)). sim = sum_i (double)a[i] * (double)b[i] in THIS order: lane l of the wave starts
// from +0.0 and adds the products of elements l, l + 64, l + 128, ... one after the other; the 64 lane sums then meet in a xor
// butterfly, s += shfl_xor(s, m) for m = 32, 16, 8, 4, 2, 1, after which every lane holds the same bits. The product of two fp32
// values is exact in fp64 (48 significant bits), so an fma and a multiply followed by an add round alike: only the additions round, and
// tests/topic_model.py restates them bit for bit. A slot that is negative or not below `rows` (a string without an embedding) gives
// exactly +0.0, as the reference's similarity() does.
//
// Replay (topic_replay_one: K_T2, one thread per candidate). The pairs are taken in order with the reference's comparisons: an exact pair sets best to
// 1.0 and ends the replay (the inner `break`, and the outer one that 1.0 >= 1.0 then takes); when the topic index changes and best
// >= 1.0 the replay ends (the outer `break`: a dot product one ulp above 1.0 stops the topics but not its own topic's remaining tags);
// `sim > best` is false for a NaN and for anything <= 0.0. The boost is evaluated in fp64 in the reference's operation order: a
// subtraction, a multiplication, a division — nothing an fma could contract. A best below the threshold stores the literal +0.0.
// No atomics: the same inputs give the same bits on every call, on any stream. The two functions are the only copy of this
// arithmetic: the kernels of a batch of questions (rerank_batch_kernel.hpp) call them too.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rdx {

constexpr int TOPIC_THREADS = 256;         // both kernels: 4 waves = 4 (topic, tag) pairs, or 256 candidates
constexpr int TOPIC_KU = 8;                // K_T1: elements of each row a lane has in flight (dim 1024: 16 per lane, two rounds)
constexpr int TOPIC_MAX_N = 1024;         // candidates per call (the reranker's limit)
constexpr int TOPIC_MAX_TOPICS = 32;       // topics per call: 5 bits of a pair word
constexpr int TOPIC_MAX_TAGS = 64;         // tags per candidate
constexpr int TOPIC_MAX_DIM = 4096;
constexpr int TOPIC_MAX_CALL_TAGS = TOPIC_MAX_N * TOPIC_MAX_TAGS;   // distinct tags per call: 16 bits of a pair word are enough, 23 are there

// a pair word (the header's RDX_TOPIC_PAIR): bits 0-4 topic index, bit 7 exact flag, bits 8-30 tag index
__device__ __forceinline__ int topic_pair_topic(int32_t w) { return w & 31; }
__device__ __forceinline__ bool topic_pair_exact(int32_t w) { return (w >> 7) & 1; }
__device__ __forceinline__ int topic_pair_tag(int32_t w) { return (int)((uint32_t)w >> 8); }

// The similarity of table rows sa and sb, computed by one wave (K_T1's arithmetic above: every lane of the wave calls this with the
// same sa and sb and gets the same bits back). A slot outside [0, rows) gives +0.0
__device__ __forceinline__ double topic_sim_wave(const float* __restrict__ table, int64_t rows, int dim, int64_t sa, int64_t sb, int lane) {
    double s = 0.0;
    if (sa >= 0 && sa < rows && sb >= 0 && sb < rows) {                  // (uniform in the wave)
        const float* a = table + sa * dim;
        const float* b = table + sb * dim;
        for (int i0 = lane; i0 < dim; i0 += 64 * TOPIC_KU) {             // TOPIC_KU loads of each row in flight, added in index order
            float av[TOPIC_KU], bv[TOPIC_KU];
#pragma unroll
            for (int k = 0; k < TOPIC_KU; ++k) {
                const int i = i0 + 64 * k;
                av[k] = i < dim ? a[i] : 0.0f;
                bv[k] = i < dim ? b[i] : 0.0f;
            }
#pragma unroll
            for (int k = 0; k < TOPIC_KU; ++k)
                if (i0 + 64 * k < dim) s += (double)av[k] * (double)bv[k];   // (guarded: an element past dim adds nothing, not even +0.0)
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    }
    return s;
}

// One candidate's replay and boost (K_T2's arithmetic above): pairs[lo .. hi) in order against sims [T][U]
__device__ __forceinline__ void topic_replay_one(const double* __restrict__ sims, int T, int U, const int32_t* __restrict__ pairs, int64_t lo,
                                                 int64_t hi, double threshold, double max_boost, double* boost_out, double* best_out) {
    double best = 0.0;
    int prev = -1;
    for (int64_t p = lo; p < hi; ++p) {
        const int32_t w = pairs[p];
        const int t = topic_pair_topic(w), u = topic_pair_tag(w);
        if (t != prev && prev >= 0 && best >= 1.0) break;                // `if best_sim >= 1.0: break` behind a topic's tags
        prev = t;
        if (topic_pair_exact(w)) {
            best = 1.0;
            break;
        }
        const double sim = (t < T && u < U) ? sims[(int64_t)t * U + u] : 0.0;
        if (sim > best) best = sim;
    }
    double boost = 0.0;
    if (!(best < threshold)) boost = max_boost * (best - threshold) / (1.0 - threshold);
    *boost_out = boost;
    if (best_out) *best_out = best;
}

// K_T1: grid ceil(T * U / 4), wave w of the grid = pair (w / U, w % U); sims [T][U]
__global__ void __launch_bounds__(TOPIC_THREADS) k_topic_sims(const float* __restrict__ table, int64_t rows, int dim,
                                                             const int32_t* __restrict__ topic_slots, int T,
                                                             const int32_t* __restrict__ tag_slots, int U, double* __restrict__ sims) {
    const int64_t pair = (int64_t)blockIdx.x * (TOPIC_THREADS / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (pair >= (int64_t)T * U) return;                                  // (whole waves: pair is uniform in a wave)
    const double s = topic_sim_wave(table, rows, dim, topic_slots[pair / U], tag_slots[pair % U], lane);
    if (lane == 0) sims[pair] = s;
}

// K_T2: thread c = candidate c: pairs[offsets[c] .. offsets[c + 1]) (clamped to [0, n_pairs]) replayed in order
__global__ void __launch_bounds__(TOPIC_THREADS) k_topic_replay(const double* __restrict__ sims, int T, int U,
                                                               const int32_t* __restrict__ offsets, const int32_t* __restrict__ pairs,
                                                               int64_t n_pairs, int n, double threshold, double max_boost,
                                                               double* __restrict__ boosts, double* __restrict__ best_sim) {
    const int c = blockIdx.x * TOPIC_THREADS + threadIdx.x;
    if (c >= n) return;
    const int64_t lo = max((int64_t)offsets[c], (int64_t)0), hi = min((int64_t)offsets[c + 1], n_pairs);
    topic_replay_one(sims, T, U, pairs, lo, hi, threshold, max_boost, boosts + c, best_sim ? best_sim + c : nullptr);
}

}  // namespace rdx
