// group_fill_kernel.hpp — K5c, the grouped search's fill: k_group_fill and its parameters. Included by rdx_index.hip only
// (rdx_index.hpp says why the fill stays in the core unit).
#pragma once
#include "rows_core.hpp"

namespace rdx {

// K5c. Grouped search's fill: job j = the best m <= 16 allowed rows of group_rows[begin[j], end[j]) for query
// job_query[j], by (exact score descending, row ascending) — the order of every search. One workgroup of GROUP_FILL_WAVES waves per job, wave w taking
// the listed rows [64 (w + 4 i), 64 (w + 4 i) + 64); a job spans at most GROUP_FILL_SPAN rows (the host splits longer groups and merges
// the parts), so no wave walks an unbounded range. A wave takes 64 listed rows at a time (lane l tests row l against the bitmap), then
// scores the allowed ones in list order; the waves' lists meet in LDS, where wave 0 ranks their 4 m <= 64 entries, one per lane. U = float4 groups per
// lane kept in registers (dim <= 1024): the next allowed row's loads are issued before the current row is summed, and the sum adds a
// lane's groups in increasing order through exact_dot4 — the order exact_score states. U = 0 (longer rows) calls exact_score itself.
// The list lives in lanes 0..m-1, best first: a new entry's place is the number of entries before it (one ballot), the rest shift up.
constexpr int GROUP_FILL_SPAN = 4096;
constexpr int GROUP_FILL_MAX_M = 16;
constexpr int GROUP_FILL_WAVES = 4;
struct GroupFillParams {
    MasterView master; int64_t rows; int dim;
    const float* qhat;                                  // the normalised queries [nq][dim]
    const uint32_t* allow;                              // the `where` bitmap or NULL
    const int32_t* job_query; const int64_t* job_begin; const int64_t* job_end; int64_t n_jobs;
    const int64_t* group_rows; int m;
    float* out_score; int64_t* out_row; int32_t* out_count;   // [n_jobs][m] (padding -inf / -1), [n_jobs]
};

template <int U>
__global__ __launch_bounds__(64 * GROUP_FILL_WAVES) void k_group_fill(const GroupFillParams p) {
    __shared__ float part_s[GROUP_FILL_WAVES * GROUP_FILL_MAX_M];
    __shared__ int64_t part_r[GROUP_FILL_WAVES * GROUP_FILL_MAX_M];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t j = blockIdx.x;   // (the grid is the jobs: every wave of the workgroup reaches the barrier below)
    const int dim = p.dim, n4 = dim >> 2, m = p.m;
    const float4* q4 = reinterpret_cast<const float4*>(p.qhat + (int64_t)p.job_query[j] * dim);
    const int64_t begin = p.job_begin[j], end = p.job_end[j];
    constexpr int UR = U > 0 ? U : 1;
    const lane_groups<UR> grp(lane, n4);
    float4 qr[UR], cur[UR], nxt[UR];
    if constexpr (U > 0) {
#pragma unroll
        for (int u = 0; u < U; ++u) qr[u] = q4[grp.gi[u]];
    }
    float best_s = -INFINITY;   // lane l < have: the list's entry l
    int64_t best_r = -1;
    int have = 0;
    for (int64_t base = begin + 64 * wave; base < end; base += 64 * GROUP_FILL_WAVES) {
        const int64_t at = base + lane;
        int64_t my = at < end ? p.group_rows[at] : -1;
        if (my < 0 || my >= p.rows) my = -1;   // (a row the index does not hold is never read)
        if (my >= 0 && p.allow && !((p.allow[my >> 5] >> (my & 31)) & 1u)) my = -1;
        unsigned long long live = __ballot(my >= 0);
        if (!live) continue;
        if constexpr (U > 0) grp.load(master_row(p.master, __shfl(my, __ffsll((long long)live) - 1, 64), dim), cur);
        while (live) {
            const int src = __ffsll((long long)live) - 1;
            live &= live - 1;
            const int64_t r = __shfl(my, src, 64);
            float s;
            if constexpr (U > 0) {
                const int64_t rn = __shfl(my, live ? __ffsll((long long)live) - 1 : src, 64);   // (the last one re-reads its own row)
                grp.load(master_row(p.master, rn, dim), nxt);
                double acc = 0.0;
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (grp.gv[u]) exact_dot4(acc, qr[u], cur[u]);
                s = (float)wave_sum(acc);
#pragma unroll
                for (int u = 0; u < U; ++u) cur[u] = nxt[u];
            } else {
                s = exact_score(master_row(p.master, r, dim), q4, n4, lane);
            }
            const bool before = lane < have && (best_s > s || (best_s == s && best_r < r));
            const int pos = __popcll(__ballot(before));
            if (pos < m) {
                const float up_s = __shfl_up(best_s, 1, 64);
                const int64_t up_r = __shfl_up(best_r, 1, 64);
                if (lane > pos) {
                    best_s = up_s;
                    best_r = up_r;
                } else if (lane == pos) {
                    best_s = s;
                    best_r = r;
                }
                if (have < m) ++have;
            }
        }
    }
    if (lane < m) {
        part_s[wave * m + lane] = lane < have ? best_s : -INFINITY;
        part_r[wave * m + lane] = lane < have ? best_r : -1;
    }
    __syncthreads();
    if (wave != 0) return;
    // the best m of the waves' lists: lane l ranks entry l among the n = 4 m entries (equal entries, which only a row listed twice
    // can make, keep their list order)
    const int n = GROUP_FILL_WAVES * m;
    const float s = lane < n ? part_s[lane] : -INFINITY;
    const int64_t r = lane < n ? part_r[lane] : -1;
    int rank = 0;
    for (int t = 0; t < n; ++t) {
        const float st = part_s[t];
        const int64_t rt = part_r[t];
        rank += rt >= 0 && (st > s || (st == s && (rt < r || (rt == r && t < lane))));
    }
    const int found = __popcll(__ballot(r >= 0));
    const int cnt = found < m ? found : m;
    if (r >= 0 && rank < m) {
        p.out_score[j * m + rank] = s;
        p.out_row[j * m + rank] = r;
    }
    if (lane >= cnt && lane < m) {
        p.out_score[j * m + lane] = -INFINITY;
        p.out_row[j * m + lane] = -1;
    }
    if (lane == 0) p.out_count[j] = cnt;
}

}  // namespace rdx
