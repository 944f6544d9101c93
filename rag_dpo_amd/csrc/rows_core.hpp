// rows_core.hpp — what every kernel that reads the stored rows or ranks a list shares, and no kernel: the master view and its rows,
// the returned row ids and a search's answers, the exact score's arithmetic (exact_dot4, lane_groups, exact_score), rank_and_write and
// the selection key of an exact score. Included by k_rows.hpp (the core unit's row kernels) and by the kernel headers of the other
// units (mmr_kernel.hpp, kmeans_kernel.hpp, group_fill_kernel.hpp, merge_kernel.hpp): it holds no __global__ function.
#pragma once
#include "rdx_common.hpp"

namespace rdx {

// The exact copy of the corpus rows ("master"): what the exact re-score K4, the exact scan K5 and get() read.
//   default : fp32 [cap][dim], the L2-normalised rows (4 B/element)
//   compact : the raw bf16 rows as delivered (2 B/element) + each row's divisor den = max(|x|_2, 1e-12) as a double. The
//             normalised element y_i = (float)((double)x_i / den) is RECOMPUTED wherever it is needed — the same two
//             operands and the same operation K1 uses, hence the same bits (oracle/rdx_oracle.c) — instead of being stored:
//             a bf16 corpus (BASELINE config 5) then costs 2 (raw) + 2 (fp16 scan copy) B/element instead of 4 + 2.
struct MasterView {
    float* f32;
    uint16_t* raw16;
    double* den;
};
struct MasterRow {
    const float4* p32;
    const ushort4* p16;
    double den;
    __device__ __forceinline__ float4 operator[](int g) const {
        if (p32) return p32[g];
        const ushort4 u = p16[g];
        float4 y;
        y.x = (float)((double)__uint_as_float((uint32_t)u.x << 16) / den);
        y.y = (float)((double)__uint_as_float((uint32_t)u.y << 16) / den);
        y.z = (float)((double)__uint_as_float((uint32_t)u.z << 16) / den);
        y.w = (float)((double)__uint_as_float((uint32_t)u.w << 16) / den);
        return y;
    }
};
__device__ __forceinline__ MasterRow master_row(const MasterView& mv, int64_t r, int dim) {
    MasterRow m;
    m.p32 = mv.f32 ? reinterpret_cast<const float4*>(mv.f32 + r * (int64_t)dim) : nullptr;
    m.p16 = mv.f32 ? nullptr : reinterpret_cast<const ushort4*>(mv.raw16 + r * (int64_t)dim);
    m.den = mv.f32 ? 1.0 : mv.den[r];
    return m;
}

// The id a search returns for a local row: through the shard's (strictly increasing) row-id map, or local + base without one.
// The one place that says so: k_refine's ranking and k_select_dense's three collections go through of().
struct RowIds {
    int64_t base;
    const int64_t* map;
    __device__ __forceinline__ int64_t of(int64_t local) const { return map ? map[local] : local + base; }
};
struct TopkOut { float* score; int64_t* row; int32_t* count; };   // a search's answers: [nq][k], [nq][k] returned ids, [nq]
constexpr int SELECT_MAX_K = 4096;   // the largest k of a search (K5b's lists, k_rows.hpp), and so of the lists a merge is given

// The exact score's arithmetic, stated once. oracle/rdx_oracle.c sums a row's products per LANE — lane l takes the float4 groups
// l, l + 64, ... in increasing order, and within a group x, y, z, w — into one fp64 accumulator, then adds the 64 lanes by the
// butterfly of wave_sum. A product of two floats is exact in fp64 (fused or not), so the score's bits depend only on the ORDER of
// the additions. Every site that scores a row keeps that order and therefore those bits: exact_score, k_exact_scores and
// k_refine's re-score through exact_dot4; k_exact_scores_reg with the query widened to doubles beforehand (the same operands).
// A group past the row's end (lane_groups) multiplies by a zero query: it adds zeros, which leave a sum that started at +0.0 as it is.
__device__ __forceinline__ void exact_dot4(double& acc, const float4& q, const float4& c) {
    acc += (double)q.x * (double)c.x;
    acc += (double)q.y * (double)c.y;
    acc += (double)q.z * (double)c.z;
    acc += (double)q.w * (double)c.w;
}

// A lane's U float4 groups of a row of n4 <= 64 U groups kept in registers: gi = lane + 64 u, clamped (a group past the row's end
// re-reads the last one: no branch around loads), gv = whether the group exists (its query values are zeros where it does not).
template <int U>
struct lane_groups {
    int gi[U];
    bool gv[U];
    __device__ __forceinline__ lane_groups(int lane, int n4) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            gv[u] = lane + 64 * u < n4;
            gi[u] = gv[u] ? lane + 64 * u : n4 - 1;
        }
    }
    __device__ __forceinline__ void load(const MasterRow& row4, float4 (&c)[U]) const {
#pragma unroll
        for (int u = 0; u < U; ++u) c[u] = row4[gi[u]];
    }
};

// exact score of one normalised query (float4 view, global or LDS) against one master row, all 64 lanes get it
template <class Q4>
__device__ __forceinline__ float exact_score(const MasterRow& row4, Q4 q4, int n4, int lane) {
    double acc = 0.0;
    for (int g = lane; g < n4; g += 64) exact_dot4(acc, q4[g], row4[g]);
    return (float)wave_sum(acc);
}

// rank entries (score desc, row asc) held in LDS and write the best k; all threads of the block call it.
// Wave-parallel: a wave takes entry i, its lanes take the entries j it is compared with (64 at a time), the rank is the
// population count of the ballots — p/64 LDS reads per entry instead of p dependent ones per thread (p = 50: 5.2 -> ~1 us in
// k_select_dense; the same routine ends k_refine and k_merge).
__device__ __forceinline__ void rank_and_write(const float* __restrict__ s, const int64_t* __restrict__ r, int p, int k,
                                               float* __restrict__ out_score, int64_t* __restrict__ out_row,
                                               int32_t* __restrict__ out_count) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int i = wave; i < p; i += nw) {
        const float si = s[i];
        const int64_t ri = r[i];
        int rank = 0;
        for (int j0 = 0; j0 < p; j0 += 64) {
            const int j = j0 + lane;
            bool before = false;
            if (j < p) {
                const float sj = s[j];
                before = (sj > si) || (sj == si && r[j] < ri);
            }
            rank += __popcll(__ballot(before));
        }
        if (lane == 0 && rank < k) {
            out_score[rank] = si;
            out_row[rank] = ri;
        }
    }
    const int c = p < k ? p : k;
    for (int i = c + threadIdx.x; i < k; i += blockDim.x) {
        out_score[i] = -INFINITY;
        out_row[i] = -1;
    }
    if (threadIdx.x == 0) *out_count = c;
}

// Selection key of an EXACT score: f2key with -0.0 put onto +0.0. The documented order (include/rdx.h) compares scores as floats,
// so the two zeros are one value and row ids decide among them; f2key alone keeps every -0.0 strictly below every +0.0. The
// selects that choose a k-th exact score and its ties use this key; what they return is the row's own score, read back from where
// it is stored (the key of a zero does not say which zero it was). The scan's thresholds keep f2key (rdx_common.hpp).
constexpr uint32_t SEL_KEY_ZERO = 0x80000000u;   // f2key(+0.0f)
__device__ __forceinline__ uint32_t f2key_sel(float f) {
    return __float_as_uint(f) == 0x80000000u ? SEL_KEY_ZERO : f2key(f);
}

}  // namespace rdx
