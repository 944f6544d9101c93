// facet_kernel.hpp — exact value counts: how many allowed rows carry each value of a metadata key, over the corpus
// (rdx_index_facet_count) and over the rows within a distance of a query (rdx_index_range_facets).
//   k_facet_count   the masked histogram of the row -> code table: counts per code, rows without a code, allowed rows
//   k_facet_top     one query's table row -> its best `limit` cells by (count descending, code ascending)
// The rows in range are counted by the counting variants of the threshold search's last stages (range_kernel.hpp, <FACET = true>);
// what they and k_facet_count share is facet_count.hpp. Included by rdx_derived.hip only. Every result is an integer: sums of ones in any order, so nothing here depends on a
// schedule. No kernel waits for another thread, workgroup or launch.
#pragma once
#include "facet_count.hpp"
#include "rdx_common.hpp"

namespace rdx {

constexpr int FACET_LDS_GROUPS = 4096;   // k_facet_count: the most codes a workgroup counts in a table of its own in LDS (16 KiB)
constexpr int FACET_MAX_LIMIT = 1024;    // k_facet_top: the most cells listed per query (include/rdx.h RDX_FACET_MAX_LIMIT)

struct FacetCounters {            // one per index, zeroed before every call
    unsigned long long missing;   // k_facet_count: allowed rows without a code
    unsigned long long total;     //                allowed rows
    int bad;                      // a code outside -1 .. n_groups - 1 was met (nothing was read or written through it)
    int pad;
};

struct FacetCountParams {
    const uint32_t* allow;        // [ceil(rows / 32)] or NULL: every row
    const int32_t* code;          // [rows] or NULL: no table (every allowed row counts as missing)
    int64_t rows, n_groups;
    unsigned long long* counts;   // [n_groups], zeroed by the caller
    FacetCounters* ctr;
    int64_t span;                 // rows per workgroup (a multiple of the block size)
};

// One thread per row, one mask word per 32 rows; a workgroup walks `span` consecutive rows. n_groups <= FACET_LDS_GROUPS: the counts
// go into the workgroup's own table in LDS, flushed with one global atomic per non-zero cell; more codes go straight to global
// memory. missing / total: per-lane counts, one shuffle reduction per wave at the end, one atomic per wave.
__global__ __launch_bounds__(256) void k_facet_count(const FacetCountParams p) {
    __shared__ uint32_t tab[FACET_LDS_GROUPS];
    const bool in_lds = p.n_groups <= FACET_LDS_GROUPS;
    const int ng = (int)(in_lds ? p.n_groups : 0);
    for (int i = threadIdx.x; i < ng; i += blockDim.x) tab[i] = 0;
    __syncthreads();
    const int64_t r0 = (int64_t)blockIdx.x * p.span;
    const int64_t r1 = r0 + p.span < p.rows ? r0 + p.span : p.rows;
    unsigned int n_missing = 0, n_total = 0;   // (span < 2^32)
    for (int64_t base = r0; base < r1; base += blockDim.x) {   // uniform trips: facet_add is called by whole waves
        const int64_t r = base + threadIdx.x;
        const bool in = r < r1;
        const bool ok = in && (!p.allow || ((p.allow[r >> 5] >> (r & 31)) & 1u));
        const int code = (in && p.code) ? p.code[r] : -1;
        const bool keyed = facet_code_ok(code, p.n_groups, &p.ctr->bad);   // (every row's code is judged, allowed or not)
        n_total += ok ? 1u : 0u;
        n_missing += (ok && !keyed) ? 1u : 0u;
        if (in_lds) facet_add(tab, code, ok && keyed);
        else facet_add(p.counts, code, ok && keyed);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        n_missing += __shfl_xor(n_missing, off, 64);
        n_total += __shfl_xor(n_total, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (n_missing) atomicAdd(&p.ctr->missing, (unsigned long long)n_missing);
        if (n_total) atomicAdd(&p.ctr->total, (unsigned long long)n_total);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < ng; i += blockDim.x) {
        const uint32_t v = tab[i];
        if (v) atomicAdd(&p.counts[i], (unsigned long long)v);
    }
}

struct FacetTopParams {
    const uint32_t* table;   // [gridDim.x][n_groups]
    int64_t n_groups;
    int limit;
    int32_t* out_code;       // [gridDim.x][limit]
    int64_t* out_n;          // [gridDim.x][limit]
    int32_t* out_found;      // [gridDim.x] cells with a non-zero count
};

// One block of 1024 threads per query over its table row, streamed from global memory in every pass (n_groups may exceed what LDS
// holds). n_values = the non-zero cells; the list is the best kk = min(limit, n_values) of them: the kk-th largest count by the radix
// select, every cell above it, and of the cells equal to it the kk - n_gt with the lowest codes — a second select, over ~code, as the
// crowded band cuts its ties by row (refine_kernel.hpp). A zero never enters: kk <= n_values puts the kk-th count at 1 or above. The kk
// cells are ranked by counting (kk <= 1024: one cell per thread); padding is code -1, count 0.
__global__ __launch_bounds__(1024) void k_facet_top(const FacetTopParams p) {
    __shared__ __attribute__((aligned(16))) uint32_t hist[HIST_WORDS];
    __shared__ uint32_t bc[4];
    __shared__ uint32_t s_n[FACET_MAX_LIMIT];
    __shared__ int32_t s_c[FACET_MAX_LIMIT];
    __shared__ unsigned int n_nonzero, n_taken;
    const int q = blockIdx.x;
    const int64_t G = p.n_groups;
    const uint32_t* __restrict__ row = p.table + (int64_t)q * G;
    int32_t* const o_c = p.out_code + (int64_t)q * p.limit;
    int64_t* const o_n = p.out_n + (int64_t)q * p.limit;
    if (threadIdx.x == 0) {
        n_nonzero = 0;
        n_taken = 0;
    }
    __syncthreads();
    unsigned int loc = 0;
    for (int64_t i = threadIdx.x; i < G; i += blockDim.x) loc += row[i] != 0u ? 1u : 0u;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) loc += __shfl_xor(loc, off, 64);
    if ((threadIdx.x & 63) == 0 && loc) atomicAdd(&n_nonzero, loc);
    __syncthreads();
    const unsigned int n_values = n_nonzero;
    const int kk = n_values < (unsigned int)p.limit ? (int)n_values : p.limit;
    for (int i = kk + threadIdx.x; i < p.limit; i += blockDim.x) {
        o_c[i] = -1;
        o_n[i] = 0;
    }
    if (threadIdx.x == 0) p.out_found[q] = (int32_t)n_values;
    if (kk == 0) return;
    int64_t n_gt, n_gt_c;
    const uint32_t kth = block_kth_largest([&](int64_t i) { return row[i]; }, G, (int64_t)kk, hist, bc, &n_gt);
    const uint32_t ckey = block_kth_largest([&](int64_t i) { return row[i] == kth ? ~(uint32_t)i : 0u; }, G, (int64_t)kk - n_gt, hist, bc, &n_gt_c);
    for (int64_t i = threadIdx.x; i < G; i += blockDim.x) {
        const uint32_t v = row[i];
        if (v > kth || (v == kth && ~(uint32_t)i >= ckey)) {
            const unsigned int at = atomicAdd(&n_taken, 1u);
            if (at < (unsigned int)kk) {   // (exactly kk cells pass: codes are distinct; the bound keeps a broken table inside the arrays)
                s_n[at] = v;
                s_c[at] = (int32_t)i;
            }
        }
    }
    __syncthreads();
    const int n = n_taken < (unsigned int)kk ? (int)n_taken : kk;
    if ((int)threadIdx.x < n) {
        const uint32_t v = s_n[threadIdx.x];
        const int32_t c = s_c[threadIdx.x];
        int rank = 0;
        for (int f = 0; f < n; ++f) rank += (s_n[f] > v || (s_n[f] == v && s_c[f] < c)) ? 1 : 0;
        o_c[rank] = c;
        o_n[rank] = (int64_t)v;
    }
}

}  // namespace rdx
