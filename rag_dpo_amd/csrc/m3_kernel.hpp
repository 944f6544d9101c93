// m3_kernel.hpp — the two small kernels of the combined BGE-M3 score (gfx950): the exact dense score of NAMED
// (query, row) pairs (include/rdx.h rdx_index_score_pairs) and the weighted sum of the three components (rdx_m3_combine). Included by
// rdx_m3.hip only; MasterRow, exact_dot4 and exact_score are rows_core.hpp.
#pragma once
#include "rows_core.hpp"

namespace rdx {

constexpr int PAIRS_WAVES = 4;                             // pairs per workgroup
constexpr int64_t PAIRS_MAX_PAIRS = (int64_t)1 << 20;
constexpr int64_t PAIRS_MAX_QUERIES = 65535;
constexpr int M3_THREADS = 256;

struct ScorePairsParams {
    MasterView master; int64_t rows; int dim;
    const float* queries; int64_t nq;                      // raw, [nq][dim]
    const int32_t* pair_q; const int64_t* pair_row; int64_t n_pairs;
    float* out;                                            // [n_pairs]
};

// One wave per pair, no barrier and no LDS. The wave normalises the pair's query as K1 does (k_rows.hpp k_normalize: the squares per lane
// in the order of exact_dot4, the butterfly of wave_sum, den = max(sqrt, 1e-12), y = (float)((double)x / den) — the same operands and
// operations, hence qhat's bits) and scores the stored row with exact_score. A query holding NaN or Inf, which a search refuses as a
// whole, gives its pairs NaN here.
struct NormalisedQuery {
    const float4* raw;
    double den;
    __device__ __forceinline__ float4 operator[](int g) const {
        const float4 v = raw[g];
        float4 y;
        y.x = (float)((double)v.x / den);
        y.y = (float)((double)v.y / den);
        y.z = (float)((double)v.z / den);
        y.w = (float)((double)v.w / den);
        return y;
    }
};

// Grid: ceil(n_pairs / PAIRS_WAVES) workgroups of 64 * PAIRS_WAVES threads.
__global__ __launch_bounds__(64 * PAIRS_WAVES) void k_score_pairs(const ScorePairsParams p) {
    const int lane = threadIdx.x & 63;
    const int64_t pair = (int64_t)blockIdx.x * PAIRS_WAVES + (threadIdx.x >> 6);
    if (pair >= p.n_pairs) return;   // (no barrier below)
    const int64_t q = p.pair_q[pair], r = p.pair_row[pair];
    if (q < 0 || q >= p.nq || r < 0 || r >= p.rows) {   // nothing is read through such a pair
        if (lane == 0) p.out[pair] = __builtin_nanf("");
        return;
    }
    const int n4 = p.dim >> 2;
    NormalisedQuery qn;
    qn.raw = reinterpret_cast<const float4*>(p.queries + q * (int64_t)p.dim);
    double acc = 0.0;
    for (int g = lane; g < n4; g += 64) {
        const float4 v = qn.raw[g];
        acc += (double)v.x * (double)v.x;
        acc += (double)v.y * (double)v.y;
        acc += (double)v.z * (double)v.z;
        acc += (double)v.w * (double)v.w;
    }
    const double n2 = wave_sum(acc);
    if (!(n2 < 1.0e300)) {   // NaN or Inf somewhere in the query (uniform)
        if (lane == 0) p.out[pair] = __builtin_nanf("");
        return;
    }
    qn.den = sqrt(n2);
    if (qn.den < 1e-12) qn.den = 1e-12;
    const float s = exact_score(master_row(p.master, r, p.dim), qn, n4, lane);
    if (lane == 0) p.out[pair] = s;
}

// value = ((w_d (double)dense + w_s sparse) + w_c (double)colbert) / W: a product per component, the sums in that order, one
// division, each rounded to fp64 once and never fused (as mmr_kernel.hpp mmr_value is written). A component whose pointer is null
// (its weight is 0) is skipped: not read, and no 0 x added. final = (float)value. One thread per element.
__global__ __launch_bounds__(M3_THREADS) void k_m3_combine(const float* __restrict__ dense, const double* __restrict__ sparse,
                                                           const float* __restrict__ colbert, int64_t n, double w_dense, double w_sparse,
                                                           double w_colbert, double w_sum, float* __restrict__ out_final,
                                                           double* __restrict__ out_value) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * M3_THREADS + threadIdx.x;
    if (i >= n) return;
    double v = 0.0;
    bool any = false;
    if (dense) {
        v = w_dense * (double)dense[i];
        any = true;
    }
    if (sparse) {
        const double t = w_sparse * sparse[i];
        v = any ? v + t : t;
        any = true;
    }
    if (colbert) {
        const double t = w_colbert * (double)colbert[i];
        v = any ? v + t : t;
    }
    v = v / w_sum;
    out_final[i] = (float)v;
    if (out_value) out_value[i] = v;
}

}  // namespace rdx
