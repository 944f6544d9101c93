// mmr_kernel.hpp — K5d: diversity-aware selection (maximal marginal relevance) over a search's candidate lists.
// Included by rdx_derived.hip only; MasterRow, lane_groups, exact_dot4 and exact_score are rows_core.hpp.
//
// One workgroup per query. Its list's live entries (position < count, 0 <= row < rows) sit in LDS as s (the query score), m (the
// largest pair score with a picked entry so far), row and a picked flag. Pick 0 is the first live position; every later round
//   1. scores the row picked last against every live unpicked candidate: the waves share the positions (position p belongs to wave
//      p % MMR_WAVES, in every round), the picked row stays in each lane's registers (U float4 groups per lane, dim <= 1024), the next
//      candidate's loads are issued before the current one is summed, and the sum is exact_score's — lane order, fp64, one rounding —
//      so p(i, j) has the bits of the engine's exact score of row j as the query against row i. U = 0 (longer rows) calls exact_score
//      itself with the picked row's MasterRow as the query view. Lane 0 folds the pair score into m[i];
//   2. after a barrier every thread evaluates v = lambda s - (1 - lambda) m for its positions: three fp64 operations, each rounded
//      once, never fused (mmr_value);
//   3. shuffles, then the waves' partial results in LDS, name the largest v, the smaller position winning ties.
// Nothing leaves the workgroup between rounds and no float is ever added atomically: the same list gives the same bits whatever the
// batch around it.
#pragma once
#include "rows_core.hpp"

namespace rdx {

constexpr int MMR_MAX_FETCH = 1024;
constexpr int MMR_MAX_K = 64;
// The waves of a workgroup. The rounds of one query run one after the other on one CU and every pair score waits for a row from
// memory, so more waves mean more pair scores in flight: 16 measured faster than k_group_fill's 4 at one query and at four (0.17
// against 0.22 ms per call at fetch_k = 50, 0.30 against 0.59 ms at 256; DESIGN.md §22, profiles/mmr/waves.txt). -DRDX_MMR_WAVES=n
// builds the other one to compare.
#ifndef RDX_MMR_WAVES
#define RDX_MMR_WAVES 16
#endif
constexpr int MMR_WAVES = RDX_MMR_WAVES;
static_assert(MMR_WAVES >= 1 && MMR_WAVES <= 16, "a workgroup holds at most 16 waves");

struct MmrParams {
    MasterView master; int64_t rows; int dim;
    const float* cand_score; const int64_t* cand_row; const int32_t* cand_count;   // [nq][fetch_k], [nq][fetch_k], [nq]
    int fetch_k, k;
    double lambda;
    int32_t* out_pos; int64_t* out_row; float* out_score; double* out_value;       // [nq][k], padding -1 / -1 / -inf / -inf
    int32_t* out_count; int32_t* out_bad;                                          // [nq]; [1]
};

// v = lambda s - (1 - lambda) m, the operations of the definition: a product, a product, a difference, each rounded to fp64 once
__device__ __forceinline__ double mmr_value(double lambda, double one_minus, float s, float m) {
#pragma clang fp contract(off)
    const double a = lambda * (double)s;
    const double b = one_minus * (double)m;
    return a - b;
}

struct MmrBest {   // the best (v descending, position ascending) entry met so far; pos < 0 = none
    double v;
    int pos;
    __device__ __forceinline__ void meet(double ov, int op) {
        if (op >= 0 && (pos < 0 || ov > v || (ov == v && op < pos))) {
            v = ov;
            pos = op;
        }
    }
};

template <int U>
__global__ __launch_bounds__(64 * MMR_WAVES) void k_mmr(const MmrParams p) {
    __shared__ float c_s[MMR_MAX_FETCH];
    __shared__ float c_m[MMR_MAX_FETCH];
    __shared__ int64_t c_row[MMR_MAX_FETCH];        // -1: the entry is padding, never read through
    __shared__ uint8_t c_picked[MMR_MAX_FETCH];
    __shared__ double part_v[MMR_WAVES];
    __shared__ int part_pos[MMR_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t q = blockIdx.x;   // (the grid is the queries: every wave of the workgroup reaches every barrier below)
    const int dim = p.dim, n4 = dim >> 2, F = p.fetch_k, k = p.k;
    const double lambda = p.lambda;
    double one_minus;
    {
#pragma clang fp contract(off)
        one_minus = 1.0 - lambda;
    }
    int n = p.cand_count[q];
    n = n < 0 ? 0 : (n > F ? F : n);
    for (int i = threadIdx.x; i < n; i += 64 * MMR_WAVES) {
        int64_t r = p.cand_row[q * F + i];
        if (r >= p.rows) {   // a row the index does not hold: reported, and skipped before any address is formed from it
            atomicOr(p.out_bad, 1);
            r = -1;
        }
        if (r < 0) r = -1;
        c_row[i] = r;
        c_s[i] = p.cand_score[q * F + i];
        c_m[i] = -INFINITY;
        c_picked[i] = 0;
    }
    constexpr int UR = U > 0 ? U : 1;
    const lane_groups<UR> grp(lane, n4);
    float4 qr[UR], cur[UR], nxt[UR];
    int32_t* o_pos = p.out_pos + q * k;
    int64_t* o_row = p.out_row + q * k;
    float* o_s = p.out_score + q * k;
    double* o_v = p.out_value + q * k;
    int last = -1;      // the position picked in the round before
    int t = 0;
    for (; t < k; ++t) {
        if (t > 0) {
            // 1. pair scores with the row picked last; lane l of wave w looks at position (64 c + l) MMR_WAVES + w
            const MasterRow pick4 = master_row(p.master, c_row[last], dim);
            if constexpr (U > 0) grp.load(pick4, qr);
            for (int base = 0; base * MMR_WAVES < n; base += 64) {
                const int at = (base + lane) * MMR_WAVES + wave;
                int64_t my = at < n && at != last && !c_picked[at] ? c_row[at] : -1;
                unsigned long long live = __ballot(my >= 0);
                if (!live) continue;
                if constexpr (U > 0) grp.load(master_row(p.master, __shfl(my, __ffsll((long long)live) - 1, 64), dim), cur);
                while (live) {
                    const int src = __ffsll((long long)live) - 1;
                    live &= live - 1;
                    float ps;
                    if constexpr (U > 0) {
                        const int64_t rn = __shfl(my, live ? __ffsll((long long)live) - 1 : src, 64);   // (the last one re-reads its own row)
                        grp.load(master_row(p.master, rn, dim), nxt);
                        double acc = 0.0;
#pragma unroll
                        for (int u = 0; u < U; ++u)
                            if (grp.gv[u]) exact_dot4(acc, qr[u], cur[u]);
                        ps = (float)wave_sum(acc);
#pragma unroll
                        for (int u = 0; u < U; ++u) cur[u] = nxt[u];
                    } else {
                        ps = exact_score(master_row(p.master, __shfl(my, src, 64), dim), pick4, n4, lane);
                    }
                    if (lane == 0) {
                        const int i = (base + src) * MMR_WAVES + wave;
                        const float mi = c_m[i];
                        c_m[i] = ps > mi ? ps : mi;
                    }
                }
            }
        }
        __syncthreads();   // the list (t = 0) or this round's m, and the flag of the pick before last, are in LDS
        // 2. every thread's best position; round 0 has no arithmetic: every live entry is worth the same, the first one wins
        MmrBest best = {0.0, -1};
        for (int i = threadIdx.x; i < n; i += 64 * MMR_WAVES) {
            if (c_row[i] < 0 || c_picked[i] || i == last) continue;
            best.meet(t > 0 ? mmr_value(lambda, one_minus, c_s[i], c_m[i]) : 0.0, i);
        }
        // 3. the wave's best by shuffles, the workgroup's through LDS; every thread folds the waves in the same order
#pragma unroll
        for (int msk = 32; msk >= 1; msk >>= 1) {
            const double ov = __shfl_xor(best.v, msk, 64);
            const int op = __shfl_xor(best.pos, msk, 64);
            best.meet(ov, op);
        }
        if (lane == 0) {
            part_v[wave] = best.v;
            part_pos[wave] = best.pos;
        }
        __syncthreads();
        MmrBest all = {0.0, -1};
#pragma unroll
        for (int w = 0; w < MMR_WAVES; ++w) all.meet(part_v[w], part_pos[w]);
        if (all.pos < 0) break;   // (uniform) the list has no unpicked entry left
        if (threadIdx.x == 0) {
            const float s = c_s[all.pos];
            o_pos[t] = all.pos;
            o_row[t] = c_row[all.pos];
            o_s[t] = s;
            o_v[t] = t > 0 ? all.v : lambda * (double)s;   // pick 0 has no picked entry to be near
            c_picked[all.pos] = 1;   // read from the next round's barrier on; until then `last` stands for it
        }
        last = all.pos;
    }
    for (int i = t + threadIdx.x; i < k; i += 64 * MMR_WAVES) {
        o_pos[i] = -1;
        o_row[i] = -1;
        o_s[i] = -INFINITY;
        o_v[i] = -INFINITY;
    }
    if (threadIdx.x == 0) p.out_count[q] = t;
}

}  // namespace rdx
