// facet_count.hpp — the device helpers the value counts' kernels share: k_facet_count (facet_kernel.hpp) and the
// counting variants of the threshold search's last stages (range_kernel.hpp, <FACET = true>). No kernel is defined here.
#pragma once
#include "rdx_common.hpp"

namespace rdx {

constexpr int FACET_ROUNDS = 4;   // facet_add: codes a wave adds with one atomic each before its lanes add their own

// A code of the table, as the kernels take it: -1 = no value; anything else outside [0, n_groups) raises the flag and counts nowhere.
__device__ __forceinline__ bool facet_code_ok(int code, int64_t n_groups, int* bad) {
    if ((uint64_t)(int64_t)code < (uint64_t)n_groups) return true;
    if (code != -1) atomicOr(bad, 1);
    return false;
}

// tab[code] += 1 for every lane with `on`; ALL lanes of the wave call it (ballots and shuffles). A skewed key — most rows hold one of
// a few values — would queue 64 atomics on one address: the wave's first FACET_ROUNDS distinct codes are added by one lane each, with
// the number of lanes that hold them; the lanes left after that add their own one.
template <class T>
__device__ __forceinline__ void facet_add(T* tab, int code, bool on) {
    const int lane = threadIdx.x & 63;
    unsigned long long left = __ballot(on);
    for (int round = 0; round < FACET_ROUNDS && left != 0; ++round) {
        const int lead = __ffsll((long long)left) - 1;
        const int c = __shfl(code, lead, 64);
        const unsigned long long same = __ballot(on && code == c) & left;
        if (lane == lead) atomicAdd(&tab[c], (T)__popcll(same));
        left &= ~same;
    }
    if ((left >> lane) & 1ull) atomicAdd(&tab[code], (T)1);
}

// What the counting variants of k_range_refine / k_range_select_dense are told beside their own parameters: q is the query's place in
// the sub-chunk whose table this is.
struct FacetIO {
    const int32_t* code;    // [rows of the index] -1 or a code < n_groups
    int64_t n_groups;
    uint32_t* table;        // [queries of the sub-chunk][n_groups], zeroed before the sub-chunk
    int64_t* missing;       // [queries] rows in range without a code
    int* bad;               // FacetCounters::bad
};

// What the two counting stages share, one block per query: of the n candidates i, those with in_range(i) are counted by the code of
// row_at(i) into the query's table row, or as missing; total[q] and fc.missing[q] are written (per-lane counts, one shuffle reduction
// and one LDS add per wave). All threads of the block call it.
template <class InRange, class RowAt>
__device__ __forceinline__ void facet_count_block(const FacetIO& fc, int q, int64_t n, int64_t* total, InRange in_range, RowAt row_at) {
    __shared__ unsigned int s_fac[2];   // rows in range, and those of them without a code
    if (threadIdx.x < 2) s_fac[threadIdx.x] = 0;
    __syncthreads();
    uint32_t* const tab = fc.table + (int64_t)q * fc.n_groups;
    unsigned int n_in = 0, n_mis = 0;
    for (int64_t base = 0; base < n; base += blockDim.x) {   // uniform trips: facet_add is called by whole waves
        const int64_t i = base + threadIdx.x;
        const bool in = i < n && in_range(i);
        const int code = in ? fc.code[row_at(i)] : -1;
        const bool keyed = facet_code_ok(code, fc.n_groups, fc.bad);
        n_in += in ? 1u : 0u;
        n_mis += (in && !keyed) ? 1u : 0u;
        facet_add(tab, code, in && keyed);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        n_in += __shfl_xor(n_in, off, 64);
        n_mis += __shfl_xor(n_mis, off, 64);
    }
    if ((threadIdx.x & 63) == 0 && n_in) atomicAdd(&s_fac[0], n_in);
    if ((threadIdx.x & 63) == 0 && n_mis) atomicAdd(&s_fac[1], n_mis);
    __syncthreads();
    if (threadIdx.x == 0) {
        total[q] = (int64_t)s_fac[0];
        fc.missing[q] = (int64_t)s_fac[1];
    }
}

}  // namespace rdx
