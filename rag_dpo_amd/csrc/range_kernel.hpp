// range_kernel.hpp — the threshold search rdx_index_range: every allowed row whose exact score reaches the query's
// threshold t, counted exactly, the best max_results of them returned in the order of every search (score descending, row ascending).
//   k_range_tau          the main scan's threshold from the user's: no sample, no k_tau
//   k_range_refine       re-scores the scan's hits exactly, counts those with exact >= t and orders the best of them (MFMA path)
//   k_range_select_dense the same answer from the dense exact scores of k_exact_scores / k_exact_scores_reg (exact path, fallback)
// Both are templates: <FACET = false> is the threshold search (rdx_index_range, rdx_index_near_dup); <FACET = true> counts the rows in
// range by their code in a row -> code table instead of ranking them (rdx_index_range_facets, facet_count.hpp).
// Included by rdx_index.hip only. The main scan between the first two is the search's own (scan_kernel.hpp), untouched.
#pragma once
#include "facet_count.hpp"
#include "refine_kernel.hpp"

namespace rdx {

struct RangeCounters {   // one per index, zeroed before every chunk of a range search; nothing of a search's RefineCounters is used
    int n_fallback;      // queries k_range_refine handed to the exact scan
    int bad;             // set by K1 when a query embedding holds NaN/Inf, by k_range_tau when a threshold is NaN
    int oob;             // RDX_CHECK_BOUNDS builds: the scan computed a corpus address outside the scan copy
    int pad;
};

// tau[q] = (t_q - E) * 4^scale_log2, the subtraction rounded toward -inf (a threshold may only move down: a lower one emits more);
// the product with a power of two is exact. Why no row is lost: a row with exact score s >= t has coarse >= s - E >= t - E
// (|coarse - exact| <= E, DESIGN.md §5, for the sums of k_scan and of k_scan_small alike: E bounds fp32 accumulation in any order),
// the scan compares coarse * 4^scale_log2 (exact) with tau, and fl_down(t - E) <= t - E. t = -inf: every allowed row; t = +inf and
// padding queries q >= nq: +inf, nothing is emitted. A NaN threshold raises `bad` and emits nothing.
__global__ __launch_bounds__(256) void k_range_tau(const float* __restrict__ thr, int nq, int nq_pad, float e, float scale2,
                                                   float* __restrict__ tau, int* __restrict__ bad) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq_pad) return;
    float v = INFINITY;
    if (q < nq) {
        const float t = thr[q];
        if (t != t) atomicOr(bad, 1);
        else if (t == INFINITY || t == -INFINITY) v = t;
        else v = sub_down(t, e) * scale2;
    }
    tau[q] = v;
}

struct RangeParams {
    RefineParams r;            // the hit segments, the list's size, k = max_results, qhat / master / dim, ids, out (refine_kernel.hpp); the
                               // fields of a top-k search's thresholds and bands (two_e, tau, pilot, spill) are not read
    const float* thr;          // [nq] score thresholds t
    int64_t* total;            // [nq] rows in range
    int32_t* fallback_list;    // queries handed to the exact scan (RangeCounters::n_fallback of them)
    RangeCounters* ctr;
};

// One block per query (1024 threads: the exact re-score runs one wave per hit).
//   The scan left, per (query, stream), every allowed row whose coarse score >= t - E: a superset of the rows in range. They are
//   gathered into the LDS list (gather_hits), EVERY one is re-scored exactly in place (exact score over coarse score; rescore_rows:
//   the oracle's bits), those with exact >= t are counted — the query's total — and the best k of them are ranked. More than k in
//   range: the k-th largest exact score by the radix select, everything above it and its ties, ties cut by row where identical rows
//   outnumber the ranking arrays (the crowded band's statements, refine_kernel.hpp). Entries below t never reach the ranking: total
//   > k puts the k-th key at or above t.
//   A query with an overflowed segment or more hits than the list holds is appended to the fallback list (one atomic) and answered by
//   the exact scan.
//   FACET: every hit with exact >= t adds one to its code's cell of the query's table row (fc.table) or to fc.missing[q], beside the
//   total; nothing is ranked and no list is written. A query handed to the fallback list returns BEFORE it has counted anything: its
//   table row is written by the dense stage alone, so it is counted exactly once.
template <bool FACET>
__global__ __launch_bounds__(1024) void k_range_refine(const RangeParams args, const FacetIO fc) {
    extern __shared__ __attribute__((aligned(16))) char smem[];   // [list_cap] hits
    __shared__ RefineLds L;
    RefineParams p = args.r;
    p.master = MasterView{held_in_sgprs(args.r.master.f32), held_in_sgprs(args.r.master.raw16), held_in_sgprs(args.r.master.den)};
    p.dim = held_in_sgprs(args.r.dim);
    const int q = (int)blockIdx.x, k = p.k;
    const int n_streams = p.n_streams;
    const int lane = threadIdx.x & 63;
    uint32_t* const seg_off = L.seg_off;
    if (threadIdx.x == 0) L.overflow = 0;
    __syncthreads();
    // segment sizes -> exclusive prefix (refine_block's statements)
    for (int w = threadIdx.x; w < n_streams; w += blockDim.x) {
        const uint32_t cw = p.cntw[(int64_t)q * n_streams + w];
        if (cw > p.capw) L.overflow = 1;
        seg_off[w + 1] = cw > p.capw ? p.capw : cw;
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        uint32_t carry = 0;
        for (int base = 0; base < n_streams; base += 64) {
            const int w = base + lane;
            uint32_t v = w < n_streams ? seg_off[w + 1] : 0u;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const uint32_t t = __shfl_up(v, off, 64);
                if (lane >= off) v += t;
            }
            if (w < n_streams) seg_off[w + 1] = carry + v;
            carry += __shfl(v, 63, 64);
        }
        if (lane == 0) seg_off[0] = 0;
    }
    __syncthreads();
    const uint32_t m = seg_off[n_streams];
    if (L.overflow != 0 || m > p.list_cap) {
        if (threadIdx.x == 0) args.fallback_list[atomicAdd(&args.ctr->n_fallback, 1)] = q;
        return;
    }
    float* const o_s = p.out.score + (int64_t)q * k;
    int64_t* const o_r = p.out.row + (int64_t)q * k;
    if (m == 0) {
        if (threadIdx.x == 0) args.total[q] = 0;
        if constexpr (FACET) {
            if (threadIdx.x == 0) fc.missing[q] = 0;
        } else {
            rank_and_write(L.s_s, L.s_r, 0, k, o_s, o_r, p.out.count + q);
        }
        return;
    }
    uint2* const list = reinterpret_cast<uint2*>(smem);
    const RefineQuery c = {L, list, m, q};
    gather_hits(p, c);
    rescore_rows(p, q, (int)m, [&](int i) { return (int64_t)list[i].y; }, [&](int i, float sx) { list[i].x = __float_as_uint(sx); });
    __syncthreads();
    // total = hits with exact >= t: per-lane counts, one shuffle reduction per wave, one LDS add per wave
    const float t = args.thr[q];
    if constexpr (FACET) {
        facet_count_block(fc, q, (int64_t)m, args.total, [&](int64_t i) { return __uint_as_float(list[i].x) >= t; },
                          [&](int64_t i) { return (int64_t)list[i].y; });
        return;
    }
    reset_count(L);
    int loc = 0;
    for (uint32_t i = threadIdx.x; i < m; i += blockDim.x) loc += __uint_as_float(list[i].x) >= t ? 1 : 0;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) loc += __shfl_xor(loc, off, 64);
    if (lane == 0 && loc) atomicAdd(&L.n_p, loc);
    __syncthreads();
    const int total = L.n_p;
    __syncthreads();   // (everybody has read the count before it is reset)
    if (threadIdx.x == 0) args.total[q] = total;
    if (total == 0) {
        rank_and_write(L.s_s, L.s_r, 0, k, o_s, o_r, p.out.count + q);
        return;
    }
    int n2;
    if (total <= k) {   // (k <= REFINE_PMAX: all of them fit the ranking arrays)
        reset_count(L);
        for (uint32_t i = threadIdx.x; i < m; i += blockDim.x) {
            const uint2 e = list[i];
            if (__uint_as_float(e.x) >= t) {
                const int at = atomicAdd(&L.n_p, 1);
                L.s_s[at] = __uint_as_float(e.x);
                L.s_r[at] = (int64_t)e.y;
            }
        }
        __syncthreads();
        n2 = total;
    } else {
        int64_t n_gt;
        const uint32_t kth = block_kth_largest([&](int64_t i) { return f2key_sel(__uint_as_float(list[i].x)); }, (int64_t)m, (int64_t)k, L.hist, L.bc, &n_gt);
        n2 = take_reaching(c, (int)m, kth, 0u);
        if (n2 > REFINE_PMAX) {   // identical rows: of the ties the k - n_gt with the lowest rows (crowded_band's second select)
            int64_t n_gt_r;
            const uint32_t rkey = block_kth_largest(
                [&](int64_t i) {
                    const uint2 e = list[i];
                    return f2key_sel(__uint_as_float(e.x)) == kth ? ~e.y : 0u;
                },
                (int64_t)m, (int64_t)k - n_gt, L.hist, L.bc, &n_gt_r);
            n2 = take_reaching(c, (int)m, kth, rkey);
        }
    }
    rank_rows(p, c, n2);
}

// The exact path's last stage, one block of 1024 threads per listed query, over the dense exact scores K5a left ([gridDim.x][rows],
// -inf = excluded by the `where` pre-filter, never counted and never returned): total = rows with score >= t; the best k rows by
// select_dense_query, of which the first min(k, total) are in range (the list is sorted, and every row in range is an allowed row):
// the rest becomes padding.
// FACET: the rows with score >= t are counted by code into the query's table row (or fc.missing[q]) in the same walk; no list.
template <bool FACET>
__global__ __launch_bounds__(1024) void k_range_select_dense(const SelectParams p, const float* __restrict__ thr,
                                                             int64_t* __restrict__ total, const FacetIO fc) {
    if constexpr (FACET) {
        const int q = p.q_list[blockIdx.x];
        const float t = thr[q];
        const float* __restrict__ sc = p.scores + (int64_t)blockIdx.x * p.rows;
        facet_count_block(fc, q, p.rows, total, [&](int64_t i) { return sc[i] > -INFINITY && sc[i] >= t; }, [](int64_t i) { return i; });
        return;
    }
    __shared__ unsigned int s_total;
    const int j = blockIdx.x;
    const int q = p.q_list[j];
    const int64_t rows = p.rows;
    const float t = thr[q];
    const float* __restrict__ sc = p.scores + (int64_t)j * rows;
    if (threadIdx.x == 0) s_total = 0;
    __syncthreads();
    unsigned int loc = 0;
    for (int64_t i = threadIdx.x; i < rows; i += blockDim.x) {
        const float s = sc[i];
        loc += (s > -INFINITY && s >= t) ? 1u : 0u;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) loc += __shfl_xor(loc, off, 64);
    if ((threadIdx.x & 63) == 0 && loc) atomicAdd(&s_total, loc);
    __syncthreads();
    const unsigned int tot = s_total;
    select_dense_query(p);
    // select_dense_query's stores have landed before other threads of the block write over them
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const int k = p.k;
    const int cnt = tot < (unsigned int)k ? (int)tot : k;
    for (int i = cnt + threadIdx.x; i < k; i += blockDim.x) {
        p.out.score[(int64_t)q * k + i] = -INFINITY;
        p.out.row[(int64_t)q * k + i] = -1;
    }
    if (threadIdx.x == 0) {
        p.out.count[q] = cnt;
        total[q] = (int64_t)tot;
    }
}

}  // namespace rdx
