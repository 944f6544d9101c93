// rdx_index.hpp — the dense index as the units of librdx that work on it see it: rdx_index.hip, which owns it (lifecycle, writes, the
// search pipeline, the threshold search, the grouped fill), and rdx_derived.hip, whose calls are built on those. Private to csrc/; not index_state.hpp,
// which stays HIP-free.
//
// ONE DEFINITION. Every __global__ function and every __device__ variable of librdx is defined in exactly one translation unit (a
// non-template kernel in a header can be linked from one unit only, and a template instantiated in two would be two kernels of one
// name). So a header that more than one unit includes holds no kernel: this one, rows_core.hpp, rdx_common.hpp, facet_count.hpp. A
// header with kernels says, in its first lines, which one unit includes it. What another unit needs of a kernel it reaches through
// a host function of the owning unit, declared at the end of this header.
//
// Three decisions that follow:
//   * k_normalize (k_rows.hpp) stays rdx_index.hip's. The k-means reaches it through normalize_queries<true>, which the core
//     instantiates; its initial centroids are that call with `out` given.
//   * dispatch_u is a host template that launches whatever kernel its caller names: it lives here.
//   * The grouped fill (rdx_index_group_fill, group_fill_kernel.hpp) stays in rdx_index.hip. k_group_fill<0> and the long-row re-score of
//     k_refine / k_range_refine call the same instantiation of exact_score (rows_core.hpp), and the compiler specialises a device function
//     over the callers it sees in a unit: k_refine tells it n4 > 256, k_group_fill<0> nothing. Without the fill in the unit the four refine
//     kernels come out different (a loop compare turns unsigned) — equivalent code, but not the code that was measured and ISA-checked.
//     A unit's kernels are byte-for-byte a function of which kernels it holds: tools/compare_listings.py after every move.
#pragma once
#include "rdx_host.hpp"

#include <cmath>
#include <functional>
#include <mutex>
#include <type_traits>
#include <vector>

#include "index_state.hpp"
#include "rows_core.hpp"
#include "search_plan.hpp"

namespace rdx {
struct Mailbox;   // refine_kernel.hpp
struct FacetIO;   // facet_count.hpp
}
using namespace rdx;

// Which rows a search's queries may return (device addresses): one bitmap for all of them or none — the shared form, what a plain
// pointer converts to — or a bitmap per query (rdx_search_filtered): query q is held to ftab[qf[q]], to none when qf[q] < 0.
struct RowFilter {
    const uint32_t* allow = nullptr;
    const uint32_t* const* ftab = nullptr;
    const int32_t* qf = nullptr;   // NULL: the shared form
    RowFilter(const uint32_t* a = nullptr) : allow(a) {}
    RowFilter(const uint32_t* const* t, const int32_t* q) : ftab(t), qf(q) {}
};

// the caller's buffers of one search chunk (device addresses)
struct SearchIO {
    const float* queries;
    RowFilter allow;
    float* score;
    int64_t* row;
    int32_t* count;
    int32_t* flags;   // rdx_search_async(out_flags): the "incomplete" word of the packed partial, or NULL
};

// A search whose kernels (up to k_finish) are enqueued and whose host half — waiting for the mailbox, copying small
// results out, re-weighting the XCD shares, the fallback passes for overflowed queries, the statistics — has not run yet.
// rdx_search runs that half at once; rdx_search_async leaves it to rdx_search_wait, so that the caller can enqueue what
// consumes the results (the RCCL all-gather and the merge) while the scan is still running.
struct PendingSearch {
    bool active = false;
    SearchPlan plan;
    SearchIO io = {};
    hipStream_t st = nullptr;
    unsigned long long seq = 0;
    rdx_search_stats stats = {};   // rdx_search_async only: the statistics of the deferred search
};

// ------------------------------------------------------------------------------------------------
// the index: one corpus shard resident in one GPU's HBM
// ------------------------------------------------------------------------------------------------
// The rows, allocated for `cap` of them (a multiple of 256; the policy: index_state.hpp). grow() and rdx_index_compact() fill a
// fresh store and move it into place once everything enqueued on it has run: leaving early frees the fresh one, and the index
// stands as it was.
struct RowStore {
    int compact = 0;   // option "compact_master" (settable while the index is empty): 4 instead of 6 B/element
    int64_t cap = 0;
    DevBuf master;     // [cap][dim] normalised fp32 rows (default), or none with compact_master:
    DevBuf raw16;      //   [cap][dim] raw bf16 rows as delivered ...
    DevBuf den;        //   [cap] ... and their divisors max(|x|, 1e-12); rows_core.hpp MasterView
    DevBuf shadow;     // [cap][dim_pad] fp16 scan copy in MFMA fragment order (rdx_common.hpp corpus_off)
    DevBuf row_map;    // [cap] local row -> returned row id (strictly increasing), or none = local + row_base

    MasterView mv() const { return MasterView{master.as<float>(), raw16.as<uint16_t>(), den.as<double>()}; }
    const int64_t* ids() const { return row_map.as<int64_t>(); }
    // master (in this store's mode) and shadow for ncap rows; all or nothing
    hipError_t alloc_rows(int64_t ncap, int dim, int dim_pad) {
        hipError_t e = compact ? raw16.alloc((size_t)ncap * dim * 2) : master.alloc((size_t)ncap * dim * 4);
        if (e == hipSuccess && compact) e = den.alloc((size_t)ncap * 8);
        if (e == hipSuccess) e = shadow.alloc((size_t)ncap * dim_pad * 2);
        if (e != hipSuccess)
            for (DevBuf* b : {&master, &raw16, &den, &shadow}) b->release();
        cap = e == hipSuccess ? ncap : 0;
        return e;
    }
    hipError_t alloc_ids() { return row_map.alloc((size_t)std::max<int64_t>(cap, 256) * 8); }
};

// The int8 coarse pass's copy of the corpus, built by the first search that takes the path and brought up to date by every later
// one (prepare_i8); not persisted. Which rows of it are current is the watermark's to say (index_state.hpp).
struct I8Copy {
    DevBuf c8;      // [cap][dim_pad] in corpus_off8 order
    DevBuf sblk;    // s_b per 32-row block
    DevBuf eps8;    // the largest eps_b
    // the classes of block error: eps_b per block, the EPS_CLASSES - 1 stored edges (taken at a full quantisation), a class byte per block
    DevBuf epsb, edge8, cls8;
    I8Watermark mark;

    // room for cap rows; a buffer that had to be allocated anew lost its contents, and the watermark is told
    int ensure(int64_t cap, int dim_pad) {
        const size_t need[6] = {(size_t)cap * dim_pad, (size_t)(cap / 32) * 4, 4, (size_t)(cap / 32) * 4, (size_t)EPS_CLASSES * 4,
                                (size_t)(cap / 32 + 3) / 4 * 4};   // (cls8: k_scan<I8> reads whole dwords)
        DevBuf* const buf[6] = {&c8, &sblk, &eps8, &epsb, &edge8, &cls8};
        for (int i = 0; i < 6; ++i) {
            const void* was = buf[i]->p;
            RDX_TRY(buf[i]->ensure(need[i]));
            if (buf[i]->p != was) mark.reallocated();
        }
        return RDX_OK;
    }
};

constexpr int64_t RANGE_CHUNK = 4096;   // queries per pipeline pass of rdx_index_range, as a search chunks them (search_impl)

// rdx_index_near_dup's scratch (grow-only): the parent array, and per batch the query rows, the gathered queries, their thresholds, the
// threshold search's answers, the heavy list and the counter block (dup_kernel.hpp); sized by rdx_derived.hip's dup_ensure
struct DupScratch {
    DevBuf parent, ids, q, thr, score, row, count, total, heavy, ctr;
};

// rdx_index_kmeans' scratch (grow-only): the histograms / offsets, the order, the two tables, the segments' totals, the counters, and
// the pinned word the host reads once per assignment; sized by rdx_derived.hip's km_ensure
struct KmScratch {
    DevBuf hist, order, cluster_off, seg_off, segsum, ctr;
    MappedPin<unsigned long long> mail;
    unsigned long long seq = 0;   // number of the last word asked for
};

struct rdx_index {
    int device = 0;
    int dim = 0, dim_pad = 0, ksteps = 0, scale_log2 = 0;
    int n_cu = 256;
    int64_t rows = 0;
    RowStore store;
    hipStream_t own_stream = nullptr;
    std::mutex mu;

    // what a plan reads (search_plan.hpp), beside shape()
    SearchOptions opt;      // the search options of rdx_index_set_option
    SearchAdapt adapt;      // what finished searches feed back
    int coarse_bits = 0;    // the last search's coarse pass: 16, 8, or 0 (exact path only); rdx_search_last_coarse_bits
    int64_t row_base = 0;   // added to every returned row id (global ids of a shard)

    // scratch (grow-only; never allocated inside a warmed-up search)
    DevBuf r_list, r_q, r_s, r_r, r_c;   // second-chance batch of overflowed queries
    DevBuf r_qf;                         //   ... and their filter indices (a filter per query)
    DevBuf fq;                           // rdx_search_filtered: the masks' device pointers | the queries' filter indices
    std::vector<char> fq_host;           //   ... and what they are uploaded from (kept until the next call)
    DevBuf wgt;                          // [grid][2] workgroup time stamps of the main scan
    DevBuf staging, qraw, qhat, qshadow, tau, cntw, cand, setmax, exact_list, iota, dense, ctr, bad, o_score, o_row,
        o_count, mask, ids;
    I8Copy i8;
    // the int8 pass's per-search query copy, scales, bounds, thresholds (nothing of it outlives a search)
    DevBuf qshadow8, tq8, eq8, nq8, thr8, taus8, twoe8;
    DevBuf gjobs;            // rdx_index_group_fill: the call's jobs (query | begin | end)
    DevBuf rng_ctr;          // rdx_index_range: its own counter block (range_kernel.hpp RangeCounters)
    DupScratch dup;          // rdx_index_near_dup
    int dup_batch = 0;       // option "dup_batch": rows per batch of rdx_index_near_dup, 0 = the range chunk (tests lower it)
    KmScratch km;            // rdx_index_kmeans
    int km_tiles = 0;        // option "km_tiles": tiles of 256 rows per block of rdx_index_kmeans' order, 0 = km_block_span (tests raise it)
    DevBuf fct_ctr, fct_tab; // rdx_index_facet_count / rdx_index_range_facets: the counter block, a sub-chunk's tables (facet_kernel.hpp)
    int64_t facet_table_kb = 0;   // option "facet_table_kb": the tables' budget, 0 = FACET_TABLE_KB
    DevBuf spill;            // k_refine<true>: [nq_pad][spill_cap] hit lists of the queries that outgrow the LDS list (first spilling plan)
    // end-of-search mailbox in pinned host memory (k_finish writes it over PCIe; the host spins on its sequence number)
    MappedPin<Mailbox> mbox;
    unsigned long long seq = 0;       // number of the last search enqueued on this index
    MappedPin<char> pin_out;          // pinned staging for the small results of host callers (score | row | count)
    bool ctr_ready = false;           // the counter block was zeroed once; afterwards every k_finish re-zeroes it
    PendingSearch pending;            // rdx_search_async: the search whose host half is still to run
    hipEvent_t ev[8] = {};
    bool ev_ok = false;
    rdx_search_stats stats = {};

    MasterView mv() const { return store.mv(); }
    float scale() const { return std::ldexp(1.0f, scale_log2); }
    float two_e() const { return 2.0f * (1.0e-3f + 2.5e-7f * (float)dim_pad); }   // see DESIGN.md "error bound"
    PlanShape shape() const { return PlanShape{rows, dim_pad, ksteps, n_cu, two_e()}; }
};

// a `where` bitmap kept resident in HBM between searches (the reference's filters are a handful of fixed shapes)
struct rdx_mask {
    int device = 0;
    int64_t rows = 0;   // row count of the index when the mask was made: a mask never outlives a write to the index
    DevBuf words;
};

// the caller's buffers of one chunk of a range search (device addresses)
struct RangeIO {
    const float* queries;
    const float* thr;
    const uint32_t* allow;
    float* score;
    int64_t* row;
    int32_t* count;
    int64_t* total;
};

// f(std::integral_constant<int, U>) for the kernels that hold a row's float4 groups in registers, U per lane: 1..4 up to dim 1024,
// U = 0 (their form for any dim) beyond
template <class F>
static void dispatch_u(int dim, F f) {
    const int u = dim <= 1024 ? (dim / 4 + 63) / 64 : 0;
    if (u == 1) f(std::integral_constant<int, 1>{});
    else if (u == 2) f(std::integral_constant<int, 2>{});
    else if (u == 3) f(std::integral_constant<int, 3>{});
    else if (u == 4) f(std::integral_constant<int, 4>{});
    else f(std::integral_constant<int, 0>{});
}

// ------------------------------------------------------------------------------------------------
// what rdx_index.hip defines for rdx_derived.hip: inside the library only (hidden), every one called with h->mu held
// ------------------------------------------------------------------------------------------------
#pragma GCC visibility push(hidden)
namespace rdx {

int set_device(const rdx_index* h);
// run the host half of a search left pending by rdx_search_async
int finish_pending(rdx_index* h, bool* redone);
// a resident mask is the index's, as it stands; code: RDX_ERR_STATE, or RDX_ERR_INVALID from the threshold search and the clustering (include/rdx.h)
int check_mask(const rdx_index* h, const rdx_mask* mask, const char* who, int code);
// calls that take or return the index's own rows are not a shard's; tail: what the caller is told instead
int check_own_rows(const rdx_index* h, const char* who, const char* tail);

// K1 on nq caller queries: into h->qhat (fp32, what every exact score is taken against), or into `out` when given, and, with qshadow, their tiled fp16
// copy for the scan, padded to nq_pad queries (0: none). QUERY: the call site's instantiation; the query form is told the scan copy's geometry
// whether or not it writes one.
template <bool QUERY>
int normalize_queries(rdx_index* h, const float* queries, int64_t nq, int64_t nq_pad, _Float16* qshadow, int* d_bad, int verbatim, hipStream_t st,
                      float* out = nullptr);

// out[i] = the stored row d_ids[i], i < n (k_gather_rows: rdx_index_get, the clustering's queries)
int gather_rows(const rdx_index* h, const int64_t* d_ids, int64_t n, float* out, hipStream_t st);

// The exact full scan for the queries of qhat listed in d_list[0..n_list), QX at a time: a group's scores land in h->dense [nq][rows], then
// after(q_list, nq, last) launches what consumes them (for_exact_groups, for a consumer in another unit)
int exact_groups(rdx_index* h, const int32_t* d_list, int n_list, const RowFilter& allow, hipStream_t st,
                 const std::function<void(const int32_t*, int, bool)>& after);

// One chunk (nq <= RANGE_CHUNK) of a range search; returns with the stream drained and qhat holding K1 of the chunk's queries. paths[0] / [1]
// take the chunk's queries by path. fc: the counting variants of the two last stages instead (rdx_index_range_facets): io's lists are not
// written, k is 1.
int range_chunk(rdx_index* h, const RangeIO& io, int64_t nq, int k, hipStream_t st, int32_t* paths, const FacetIO* fc = nullptr);

}   // namespace rdx
#pragma GCC visibility pop
