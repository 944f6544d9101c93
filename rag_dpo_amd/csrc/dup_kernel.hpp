// dup_kernel.hpp — near-duplicate clustering rdx_index_near_dup: the connected components of "row j is within the
// distance of row i", stored rows against stored rows, labelled by their smallest row.
//   k_dup_init        parent[r] = r for an allowed row, -1 otherwise; total[r] = 0
//   k_dup_link_lists  one batch of rows as queries, answered by the threshold search (range_kernel.hpp): the rows whose whole
//                     neighbourhood is listed (total <= list_cap) are united with their list; the others are "heavy" and are handed on
//   k_dup_link_dense  heavy rows: united with every row whose dense exact score (k_exact_scores / k_exact_scores_reg) reaches t
//   k_dup_labels      label[r] = root of r, in a launch of its own
// Included by rdx_derived.hip only. The union-find itself is dup_union.hpp (HIP-free, rehearsed on the host); its termination argument
// is written there. No kernel here waits for another thread, workgroup or launch.
//
// Visibility. Workgroups on different XCDs link the same components at the same time. The XCDs' L2s are not coherent with each other
// and a CU's L1 is never refreshed by another CU's stores, so inside the linking launches parent[] is read ONLY through the
// agent-scope atomic load and written ONLY through the agent-scope compare-and-swap (DupDevicePolicy): both are performed at the
// device's coherence point, whichever XCD issues them. A plain load could return a cached word of any age. An old word is still a
// former ancestor (words only decrease, dup_union.hpp), so it could not break a result — but nothing here relies on that. Relaxed
// order suffices: no other data is published through these words. k_dup_init writes parent[] plainly BEFORE the linking launches and
// k_dup_labels runs AFTER them: kernel boundaries on one stream order those.
#pragma once
#include "dup_union.hpp"
#include "rdx_common.hpp"

namespace rdx {

struct DupDevicePolicy {
    using word = int32_t;
    static __device__ __forceinline__ int32_t load(const word* p) {
        return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    static __device__ __forceinline__ int32_t cas(word* p, int32_t expected, int32_t desired) {
        (void)__hip_atomic_compare_exchange_strong(p, &expected, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return expected;   // what the word held: `expected` itself when the swap took place
    }
};

struct DupCounters {   // zeroed before every batch
    int n_heavy;       // queries of the batch appended to the heavy list
    int pad[3];
};

// unite with the read-only question first: the rows of a dense cluster are mostly united already, and asking costs no write
__device__ __forceinline__ void dup_link(int32_t* parent, int32_t a, int32_t b) {
    if (!dup_same<DupDevicePolicy>(parent, a, b)) (void)dup_unite<DupDevicePolicy>(parent, a, b);
}

__global__ __launch_bounds__(256) void k_dup_init(int32_t* __restrict__ parent, const uint32_t* __restrict__ allow, int64_t rows,
                                                  int64_t* __restrict__ total) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const bool ok = !allow || ((allow[r >> 5] >> (r & 31)) & 1u);
    parent[r] = ok ? (int32_t)r : -1;
    total[r] = 0;
}

struct DupListParams {
    int32_t* parent;            // [rows]
    int64_t rows;
    const int64_t* qrow;        // [nq] the batch's query rows (ascending allowed rows)
    int nq, list_cap;
    const int64_t* row;         // [nq][list_cap] the threshold search's lists ...
    const int32_t* count;       // [nq] ... their lengths ...
    const int64_t* total;       // [nq] ... and the exact number of rows in range
    int64_t* out_total;         // [rows]
    int32_t* heavy;             // [nq] positions (in the batch) of the heavy queries, in no particular order
    DupCounters* ctr;
};

// One wave per query of the batch. total <= list_cap: the list is the whole neighbourhood, its lanes unite the query row with the
// listed rows. total > list_cap: NONE of the list is used (the rows beyond it would be lost, and which ones the list holds depends on
// list_cap: a partial answer must not leak into the result) — the query's position goes to the heavy list with one atomic.
__global__ __launch_bounds__(256) void k_dup_link_lists(const DupListParams p) {
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (j >= p.nq) return;
    const int64_t qr = p.qrow[j];
    if (qr < 0 || qr >= p.rows) return;
    const int64_t tot = p.total[j];
    if (lane == 0) p.out_total[qr] = tot;
    if (tot > (int64_t)p.list_cap) {
        if (lane == 0) p.heavy[atomicAdd(&p.ctr->n_heavy, 1)] = j;
        return;
    }
    int cnt = p.count[j];
    cnt = cnt < p.list_cap ? cnt : p.list_cap;
    const int64_t* __restrict__ list = p.row + (int64_t)j * p.list_cap;
    for (int i = lane; i < cnt; i += 64) {
        const int64_t r = list[i];
        if (r >= 0 && r < p.rows && r != qr) dup_link(p.parent, (int32_t)qr, (int32_t)r);
    }
}

struct DupDenseParams {
    int32_t* parent;
    int64_t rows;
    const float* scores;        // [nq][rows] dense exact scores, -inf = excluded row
    const int32_t* q_list;      // [nq] the heavy queries' positions in the batch (what the scores were computed for) ...
    const int64_t* qrow;        // ... and the batch's query rows
    int nq;                     // <= QX
    float t;
};

// Grid-stride over the rows, for each of the group's heavy queries: unite the query row with every row in range.
__global__ __launch_bounds__(256) void k_dup_link_dense(const DupDenseParams p) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int j = 0; j < p.nq; ++j) {
        const int64_t qr = p.qrow[p.q_list[j]];
        if (qr < 0 || qr >= p.rows) continue;
        const float* __restrict__ sc = p.scores + (int64_t)j * p.rows;
        for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < p.rows; r += stride) {
            const float s = sc[r];
            if (s > -INFINITY && s >= p.t && r != qr) dup_link(p.parent, (int32_t)qr, (int32_t)r);
        }
    }
}

__global__ __launch_bounds__(256) void k_dup_labels(int32_t* __restrict__ parent, int64_t rows, int64_t* __restrict__ label) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    label[r] = (int64_t)dup_find<DupDevicePolicy, false>(parent, (int32_t)r);   // (-1 for a row outside)
}

}   // namespace rdx
