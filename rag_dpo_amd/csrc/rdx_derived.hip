// rdx_derived.hip — what librdx builds on a dense index and its searches (struct rdx_index: rdx_index.hpp): the MMR selection, the
// near-duplicate clustering, the k-means and the value counts of include/rdx.h, each with its own kernels. The index, its write path, the
// search pipeline, the threshold search and the grouped fill are rdx_index.hip; this unit reaches them through the host functions
// rdx_index.hpp declares and includes none of that unit's kernel headers (k_rows.hpp, scan_kernel.hpp, refine_kernel.hpp, range_kernel.hpp,
// group_fill_kernel.hpp).
#include "rdx_index.hpp"

#include <cstddef>

#include "dup_kernel.hpp"
#include "facet_kernel.hpp"
#include "kmeans_kernel.hpp"
#include "mmr_kernel.hpp"

// ---- diversity-aware selection ---------------------------------------------------------------------------------
static_assert(MMR_MAX_FETCH == RDX_MMR_MAX_FETCH && MMR_MAX_K == RDX_MMR_MAX_K, "mmr_kernel.hpp and include/rdx.h disagree");

extern "C" int rdx_index_mmr(rdx_index* h, const float* cand_score, const int64_t* cand_row, const int32_t* cand_count, int64_t nq,
                             int fetch_k, int k, double lambda, int32_t* out_pos, int64_t* out_row, float* out_score, double* out_value,
                             int32_t* out_count, int32_t* out_bad, void* stream) {
    if (!h) return fail(RDX_ERR_INVALID, "rdx_index_mmr: null index");
    if (nq < 0 || nq > 65535) return fail(RDX_ERR_INVALID, "rdx_index_mmr: nq must be in [0, 65535]");
    if (k < 1 || k > MMR_MAX_K) return fail(RDX_ERR_INVALID, "rdx_index_mmr: k (the picks per query) must be in [1, 64]");
    if (fetch_k < k || fetch_k > MMR_MAX_FETCH) return fail(RDX_ERR_INVALID, "rdx_index_mmr: fetch_k (the entries per list) must be in [k, 1024]");
    if (!(lambda >= 0.0 && lambda <= 1.0)) return fail(RDX_ERR_INVALID, "rdx_index_mmr: lambda must be in [0, 1]");
    if (nq == 0) return RDX_OK;
    if (!cand_score || !cand_row || !cand_count) return fail(RDX_ERR_INVALID, "rdx_index_mmr: null input pointer");
    if (!out_pos || !out_row || !out_score || !out_value || !out_count || !out_bad) return fail(RDX_ERR_INVALID, "rdx_index_mmr: null output pointer");
    if (((uintptr_t)cand_row | (uintptr_t)out_row | (uintptr_t)out_value) & 7) return fail(RDX_ERR_INVALID, "rdx_index_mmr: misaligned pointer");
    if (((uintptr_t)cand_score | (uintptr_t)cand_count | (uintptr_t)out_pos | (uintptr_t)out_score | (uintptr_t)out_count | (uintptr_t)out_bad) & 3)
        return fail(RDX_ERR_INVALID, "rdx_index_mmr: misaligned pointer");
    std::lock_guard<std::mutex> lk(h->mu);
    RDX_TRY(check_own_rows(h, "rdx_index_mmr", "cand_row must be the index's own rows"));
    RDX_TRY(set_device(h));
    MmrParams mp = {};
    mp.master = h->mv();
    mp.rows = h->rows;
    mp.dim = h->dim;
    mp.cand_score = cand_score;
    mp.cand_row = cand_row;
    mp.cand_count = cand_count;
    mp.fetch_k = fetch_k;
    mp.k = k;
    mp.lambda = lambda;
    mp.out_pos = out_pos;
    mp.out_row = out_row;
    mp.out_score = out_score;
    mp.out_value = out_value;
    mp.out_count = out_count;
    mp.out_bad = out_bad;
    hipStream_t st = (hipStream_t)stream;
    dispatch_u(h->dim, [&](auto u) {   // one workgroup per query
        hipLaunchKernelGGL(k_mmr<decltype(u)::value>, dim3((unsigned)nq), dim3(64 * MMR_WAVES), 0, st, mp);
    });
    HIP_TRY(hipGetLastError());
    return RDX_OK;
}

// ---- near-duplicate clustering ------------------------------------------------------------------------------------
// Batches of allowed rows, ascending: gather the stored rows as queries (they never leave the device), the threshold search of the
// batch with lists of list_cap, k_dup_link_lists; then, while the chunk's qhat is still resident, the exact scores of the batch's heavy
// rows per group of QX and k_dup_link_dense; k_dup_labels after the last batch. DupRun: one call's arguments, and what its batches add up to.
struct DupRun {
    float threshold;
    const uint32_t* allow;
    int list_cap;
    int64_t max_dense;
    int64_t* out_total;
    hipStream_t st;
    unsigned row_blocks;   // blocks of 256 threads, one thread per row
    int64_t n_heavy = 0, n_batches = 0;
};

// the allowed rows, ascending: from the bitmap (the only thing of the call the host reads beside counters)
static int dup_allowed_rows(int64_t rows, const DupRun& run, std::vector<int64_t>* ids) {
    if (run.allow) {
        std::vector<uint32_t> words((size_t)((rows + 31) / 32));
        HIP_TRY(hipMemcpyAsync(words.data(), run.allow, words.size() * 4, hipMemcpyDeviceToHost, run.st));
        HIP_TRY(hipStreamSynchronize(run.st));
        for (int64_t r = 0; r < rows; ++r)
            if ((words[(size_t)(r >> 5)] >> (r & 31)) & 1u) ids->push_back(r);
    } else {
        ids->resize((size_t)rows);
        for (int64_t r = 0; r < rows; ++r) (*ids)[(size_t)r] = r;
    }
    return RDX_OK;
}

// DupScratch for batches of `batch` rows
static int dup_ensure(DupScratch& d, int64_t batch, int64_t rows, int list_cap, int dim) {
    const size_t B = (size_t)batch;
    DevBuf* const buf[10] = {&d.parent, &d.ids, &d.q, &d.thr, &d.score, &d.row, &d.count, &d.total, &d.heavy, &d.ctr};
    const size_t need[10] = {(size_t)rows * 4, B * 8, B * dim * 4, B * 4, B * list_cap * 4, B * list_cap * 8, B * 4, B * 8, B * 4, sizeof(DupCounters)};
    for (int i = 0; i < 10; ++i) RDX_TRY(buf[i]->ensure(need[i]));
    return RDX_OK;
}

// before the first batch: the scratch for batches of B rows, every allowed row a cluster of its own, the batch's thresholds
static int dup_begin(rdx_index* h, const DupRun& run, int64_t B) {
    RDX_TRY(dup_ensure(h->dup, B, h->rows, run.list_cap, h->dim));
    hipLaunchKernelGGL(k_dup_init, dim3(run.row_blocks), dim3(256), 0, run.st, h->dup.parent.as<int32_t>(), run.allow, h->rows, run.out_total);
    HIP_TRY(hipGetLastError());
    const std::vector<float> thr((size_t)B, run.threshold);
    HIP_TRY(hipMemcpyAsync(h->dup.thr.p, thr.data(), (size_t)B * 4, hipMemcpyHostToDevice, run.st));
    HIP_TRY(hipStreamSynchronize(run.st));
    return RDX_OK;
}

// one batch of m allowed rows: gathered as queries, searched, linked from their lists; *heavy = its rows left to the dense pass
static int dup_batch_lists(rdx_index* h, DupRun& run, const int64_t* ids, int64_t m, int* heavy) {
    DupScratch& d = h->dup;
    const hipStream_t st = run.st;
    HIP_TRY(hipMemcpyAsync(d.ids.p, ids, (size_t)m * 8, hipMemcpyHostToDevice, st));
    RDX_TRY(gather_rows(h, d.ids.as<int64_t>(), m, d.q.as<float>(), st));
    const RangeIO io = {d.q.as<float>(), d.thr.as<float>(), run.allow, d.score.as<float>(), d.row.as<int64_t>(), d.count.as<int32_t>(),
                        d.total.as<int64_t>()};
    int32_t paths[2] = {0, 0};
    RDX_TRY(range_chunk(h, io, m, run.list_cap, st, paths));
    HIP_TRY(hipMemsetAsync(d.ctr.p, 0, sizeof(DupCounters), st));
    DupListParams lp = {};
    lp.parent = d.parent.as<int32_t>();
    lp.rows = h->rows;
    lp.qrow = d.ids.as<int64_t>();
    lp.nq = (int)m;
    lp.list_cap = run.list_cap;
    lp.row = io.row;
    lp.count = io.count;
    lp.total = io.total;
    lp.out_total = run.out_total;
    lp.heavy = d.heavy.as<int32_t>();
    lp.ctr = d.ctr.as<DupCounters>();
    hipLaunchKernelGGL(k_dup_link_lists, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, st, lp);
    HIP_TRY(hipGetLastError());
    DupCounters c = {};
    HIP_TRY(hipMemcpyAsync(&c, d.ctr.p, sizeof(c), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (c.n_heavy < 0 || c.n_heavy > m) return fail(RDX_ERR_STATE, "internal: more heavy rows than rows in the batch");
    run.n_heavy += c.n_heavy;
    ++run.n_batches;
    if (run.n_heavy > run.max_dense)
        return fail(RDX_ERR_INVALID, "rdx_index_near_dup: " + std::to_string(run.n_heavy) + " rows so far have more than list_cap = " +
                                         std::to_string(run.list_cap) + " rows within the distance (max_dense = " +
                                         std::to_string(run.max_dense) + "): the distance is too loose for duplicate detection");
    *heavy = c.n_heavy;
    return RDX_OK;
}

// the dense pass of a batch's `heavy` heavy rows (the chunk's qhat — K1 of the gathered rows — is still what range_chunk left)
static int dup_dense_pass(rdx_index* h, const DupRun& run, int heavy) {
    const unsigned link_blocks = (unsigned)std::min<int64_t>(run.row_blocks, (int64_t)h->n_cu * 4);
    return exact_groups(h, h->dup.heavy.as<int32_t>(), heavy, run.allow, run.st, [&](const int32_t* q_list, int nq, bool) {
        const DupDenseParams dp = {h->dup.parent.as<int32_t>(), h->rows, h->dense.as<float>(), q_list, h->dup.ids.as<int64_t>(), nq, run.threshold};
        hipLaunchKernelGGL(k_dup_link_dense, dim3(link_blocks), dim3(256), 0, run.st, dp);
    });
}

// after the last batch: every row's label, the smallest row of its cluster
static int dup_labels(rdx_index* h, const DupRun& run, int64_t* out_label) {
    hipLaunchKernelGGL(k_dup_labels, dim3(run.row_blocks), dim3(256), 0, run.st, h->dup.parent.as<int32_t>(), h->rows, out_label);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(run.st));
    return RDX_OK;
}

extern "C" int rdx_index_near_dup(rdx_index* h, float threshold, const rdx_mask* mask, int list_cap, int64_t max_dense, int64_t* out_label,
                                  int64_t* out_total, int64_t* out_stats, void* stream) {
    if (!h) return fail(RDX_ERR_INVALID, "rdx_index_near_dup: null index");
    if (list_cap < 1 || list_cap > RDX_RANGE_MAX_RESULTS)
        return fail(RDX_ERR_INVALID, "rdx_index_near_dup: list_cap must be in [1, " + std::to_string(RDX_RANGE_MAX_RESULTS) + "]");
    if (threshold != threshold) return fail(RDX_ERR_INVALID, "rdx_index_near_dup: the threshold is NaN");
    if (max_dense < 0) return fail(RDX_ERR_INVALID, "rdx_index_near_dup: max_dense must be >= 0");
    if (out_stats) out_stats[0] = out_stats[1] = out_stats[2] = out_stats[3] = 0;
    std::lock_guard<std::mutex> lk(h->mu);
    RDX_TRY(check_mask(h, mask, "rdx_index_near_dup", RDX_ERR_INVALID));
    RDX_TRY(check_own_rows(h, "rdx_index_near_dup", "not available"));
    if (h->rows >= ((int64_t)1 << 31)) return fail(RDX_ERR_INVALID, "rdx_index_near_dup: the parent array holds int32 rows: fewer than 2^31 rows");
    RDX_TRY(finish_pending(h, nullptr));
    if (h->rows == 0) return RDX_OK;
    if (!out_label || !out_total) return fail(RDX_ERR_INVALID, "rdx_index_near_dup: null pointer");
    if (((uintptr_t)out_label | (uintptr_t)out_total) & 7) return fail(RDX_ERR_INVALID, "rdx_index_near_dup: misaligned pointer");
    RDX_TRY(set_device(h));
    DupRun run = {threshold, mask ? mask->words.as<uint32_t>() : nullptr, list_cap, max_dense, out_total, (hipStream_t)stream, (unsigned)((h->rows + 255) / 256)};
    std::vector<int64_t> ids;
    RDX_TRY(dup_allowed_rows(h->rows, run, &ids));
    const int64_t n = (int64_t)ids.size();
    const int64_t B = std::min<int64_t>(h->dup_batch > 0 ? h->dup_batch : RANGE_CHUNK, std::max<int64_t>(n, 1));
    RDX_TRY(dup_begin(h, run, B));
    for (int64_t b0 = 0; b0 < n; b0 += B) {
        int heavy = 0;
        RDX_TRY(dup_batch_lists(h, run, ids.data() + b0, std::min(B, n - b0), &heavy));
        if (heavy > 0) RDX_TRY(dup_dense_pass(h, run, heavy));
    }
    RDX_TRY(dup_labels(h, run, out_label));
    if (out_stats) {
        out_stats[0] = n;
        out_stats[1] = n - run.n_heavy;
        out_stats[2] = run.n_heavy;
        out_stats[3] = run.n_batches;
    }
    return RDX_OK;
}

// ---- k-means of the stored rows -------------------------------------------------------------------------------------
// C = K1(init) in out_centroid; an assignment = K1 of the centroids into qhat (the call a search makes on its queries), k_km_assign,
// k_km_publish; an update = the order of rows by label (k_km_hist, k_km_scan, k_km_place), the tables (k_km_seg_table),
// k_km_segment_sums, k_km_finish. The host reads one pinned word per assignment: the changed labels and K1's flag.
static_assert(RDX_KMEANS_MAX_CLUSTERS <= KM_MAX_HIST && RDX_KMEANS_MAX_CLUSTERS <= 4096, "k_km_seg_table holds the clusters in one tile of 4 096");

struct KmRun {
    int n_clusters;
    const uint32_t* allow;
    int64_t* label; float* score; float* centroid; int64_t* count;
    hipStream_t st;
    KmOrderParams order;
};

// KmScratch for `rows` rows in n_blocks blocks
static int km_ensure(KmScratch& km, int64_t rows, int n_clusters, int dim, int64_t n_blocks) {
    DevBuf* const buf[6] = {&km.hist, &km.order, &km.cluster_off, &km.seg_off, &km.segsum, &km.ctr};
    const size_t need[6] = {((size_t)n_clusters * n_blocks + 1) * 4, (size_t)rows * 4, ((size_t)n_clusters + 1) * 4, ((size_t)n_clusters + 1) * 4,
                            (size_t)km_max_segments(rows, n_clusters) * dim * 8, sizeof(KmCounters)};
    for (int i = 0; i < 6; ++i) RDX_TRY(buf[i]->ensure(need[i]));
    if (!km.mail.host) RDX_TRY(km.mail.map(64));
    return RDX_OK;
}

// the word of the work enqueued so far: *changed = labels the last assignment changed, *bad = K1 met a NaN or Inf
static int km_read_word(rdx_index* h, const KmRun& run, unsigned int* changed, bool* bad) {
    KmScratch& km = h->km;
    const unsigned long long seq = ++km.seq;
    hipLaunchKernelGGL(k_km_publish, dim3(1), dim3(1), 0, run.st, km.ctr.as<KmCounters>(), km.mail.dev, seq);
    HIP_TRY(hipGetLastError());
    unsigned long long w = 0;
    const int rc = wait_word([&] { return ((w = __atomic_load_n(km.mail.host, __ATOMIC_ACQUIRE)) >> 33) == seq; }, run.st);
    if (rc == 1) return fail(RDX_ERR_HIP, "internal: rdx_index_kmeans' assignment completed without publishing its word");
    if (rc != 0) return rc;
    *changed = (unsigned int)(w & 0xffffffffull);
    *bad = ((w >> 32) & 1ull) != 0;
    return RDX_OK;
}

static int km_assign(rdx_index* h, const KmRun& run) {
    int* const d_bad = reinterpret_cast<int*>(h->km.ctr.as<char>() + offsetof(KmCounters, bad));
    RDX_TRY(normalize_queries<true>(h, run.centroid, run.n_clusters, 0, nullptr, d_bad, 0, run.st));
    KmAssignParams ap = {};
    ap.master = h->mv();
    ap.rows = h->rows;
    ap.dim = h->dim;
    ap.qhat = h->qhat.as<float>();
    ap.n_clusters = run.n_clusters;
    ap.allow = run.allow;
    ap.label = run.label;
    ap.score = run.score;
    ap.ctr = h->km.ctr.as<KmCounters>();
    int rc = RDX_OK;
    dispatch_u(h->dim, [&](auto u) {
        constexpr int U = decltype(u)::value;
        constexpr int R = U == 0 ? 1 : (U <= 2 ? 4 : 2);   // rows per wave: each LDS read of a centroid serves R rows
        const size_t per_centroid = (size_t)(U > 0 ? 64 * U : h->dim / 4) * 32;
        const int k4 = (run.n_clusters + 3) / 4 * 4;
        ap.chunk = std::max(4, std::min(k4, (int)(KM_ASSIGN_LDS / per_centroid) / 4 * 4));
        const size_t lds = (size_t)ap.chunk * per_centroid;
        rc = dynamic_lds(h->device, (const void*)k_km_assign<U, R>, lds);
        if (rc != RDX_OK) return;
        const int64_t per_block = (int64_t)KM_ASSIGN_WAVES * R;
        hipLaunchKernelGGL((k_km_assign<U, R>), dim3((unsigned)((h->rows + per_block - 1) / per_block)), dim3(64 * KM_ASSIGN_WAVES), lds, run.st, ap);
    });
    RDX_TRY(rc);
    HIP_TRY(hipGetLastError());
    return RDX_OK;
}

// the order of rows by label and its tables; counts: the members per cluster into out_count as well
static int km_order(rdx_index* h, const KmRun& run, bool place, int64_t* counts) {
    KmScratch& km = h->km;
    const KmOrderParams& op = run.order;
    const size_t lds = (size_t)run.n_clusters * 4;
    hipLaunchKernelGGL(k_km_hist, dim3((unsigned)op.n_blocks), dim3(KM_TILE), lds, run.st, op);
    hipLaunchKernelGGL(k_km_scan, dim3(1), dim3(1024), 0, run.st, op.hist, (int64_t)run.n_clusters * op.n_blocks);
    if (place) hipLaunchKernelGGL(k_km_place, dim3((unsigned)op.n_blocks), dim3(KM_TILE), lds, run.st, op);
    hipLaunchKernelGGL(k_km_seg_table, dim3(1), dim3(1024), 0, run.st, op.hist, op.n_blocks, run.n_clusters, km.cluster_off.as<int32_t>(),
                       km.seg_off.as<int32_t>(), counts);
    HIP_TRY(hipGetLastError());
    return RDX_OK;
}

static int km_update(rdx_index* h, const KmRun& run) {
    KmScratch& km = h->km;
    RDX_TRY(km_order(h, run, true, nullptr));
    const KmSumParams sp = {h->mv(), h->dim, run.n_clusters, km.seg_off.as<int32_t>(), km.cluster_off.as<int32_t>(), km.order.as<int32_t>(),
                            km.segsum.as<double>(), run.centroid};
    hipLaunchKernelGGL(k_km_segment_sums, dim3((unsigned)km_max_segments(h->rows, run.n_clusters)), dim3(h->dim / 4 <= 64 ? 64 : 256), 0, run.st, sp);
    hipLaunchKernelGGL(k_km_finish, dim3(run.n_clusters), dim3(64), 0, run.st, sp);
    HIP_TRY(hipGetLastError());
    return RDX_OK;
}

extern "C" int rdx_index_kmeans(rdx_index* h, const float* init, int n_clusters, int max_iter, const rdx_mask* mask, int64_t* out_label,
                                float* out_score, float* out_centroid, int64_t* out_count, int32_t* out_info, void* stream) {
    if (!h) return fail(RDX_ERR_INVALID, "rdx_index_kmeans: null index");
    if (n_clusters < 1 || n_clusters > RDX_KMEANS_MAX_CLUSTERS)
        return fail(RDX_ERR_INVALID, "rdx_index_kmeans: n_clusters must be in [1, " + std::to_string(RDX_KMEANS_MAX_CLUSTERS) + "]");
    if (max_iter < 0 || max_iter > RDX_KMEANS_MAX_ITER)
        return fail(RDX_ERR_INVALID, "rdx_index_kmeans: max_iter must be in [0, " + std::to_string(RDX_KMEANS_MAX_ITER) + "]");
    std::lock_guard<std::mutex> lk(h->mu);
    RDX_TRY(check_mask(h, mask, "rdx_index_kmeans", RDX_ERR_INVALID));
    RDX_TRY(check_own_rows(h, "rdx_index_kmeans", "not available"));
    if (h->rows >= ((int64_t)1 << 31)) return fail(RDX_ERR_INVALID, "rdx_index_kmeans: the order holds int32 rows: fewer than 2^31 rows");
    if (h->rows == 0) return fail(RDX_ERR_INVALID, "rdx_index_kmeans: the index is empty");
    if (!init || !out_label || !out_score || !out_centroid || !out_count || !out_info) return fail(RDX_ERR_INVALID, "rdx_index_kmeans: null pointer");
    if ((((uintptr_t)init | (uintptr_t)out_centroid) & 15) || (((uintptr_t)out_label | (uintptr_t)out_count) & 7) || ((uintptr_t)out_score & 3))
        return fail(RDX_ERR_INVALID, "rdx_index_kmeans: misaligned pointer");
    RDX_TRY(finish_pending(h, nullptr));
    RDX_TRY(set_device(h));
    KmScratch& km = h->km;
    KmRun run = {n_clusters, mask ? mask->words.as<uint32_t>() : nullptr, out_label, out_score, out_centroid, out_count, (hipStream_t)stream, {}};
    const int64_t span = std::max<int64_t>(km_block_span(h->rows, n_clusters), (int64_t)h->km_tiles * KM_TILE), n_blocks = (h->rows + span - 1) / span;
    RDX_TRY(km_ensure(km, h->rows, n_clusters, h->dim, n_blocks));
    RDX_TRY(h->qhat.ensure((size_t)n_clusters * h->dim * 4));
    run.order = KmOrderParams{out_label, h->rows, n_clusters, span, n_blocks, km.hist.as<int32_t>(), km.order.as<int32_t>()};
    const hipStream_t st = run.st;
    HIP_TRY(hipMemsetAsync(km.ctr.p, 0, sizeof(KmCounters), st));
    // C = K1(init): the kernel and the instantiation a search's queries go through, written to the caller's centroids
    int* const d_bad = reinterpret_cast<int*>(km.ctr.as<char>() + offsetof(KmCounters, bad));
    RDX_TRY(normalize_queries<true>(h, init, n_clusters, 0, nullptr, d_bad, 0, st, out_centroid));
    unsigned int changed = 0;
    bool bad = false;
    RDX_TRY(km_read_word(h, run, &changed, &bad));
    if (bad) return fail(RDX_ERR_INVALID, "rdx_index_kmeans: init contains NaN or Inf");
    RDX_TRY(km_assign(h, run));
    RDX_TRY(km_read_word(h, run, &changed, &bad));   // (the first assignment's count compares with what the caller's buffer held: not used)
    int n_iter = 0, converged = 0;
    while (n_iter < max_iter) {
        RDX_TRY(km_update(h, run));
        ++n_iter;
        RDX_TRY(km_assign(h, run));
        RDX_TRY(km_read_word(h, run, &changed, &bad));
        if (bad) return fail(RDX_ERR_STATE, "internal: rdx_index_kmeans produced a centroid with NaN or Inf");
        if (changed == 0) {
            converged = 1;
            break;
        }
    }
    RDX_TRY(km_order(h, run, false, out_count));
    HIP_TRY(hipStreamSynchronize(st));
    out_info[0] = n_iter;
    out_info[1] = converged;
    return RDX_OK;
}

// ---- value counts ---------------------------------------------------------------------------------------------------
static_assert(FACET_MAX_LIMIT == RDX_FACET_MAX_LIMIT, "facet_kernel.hpp and include/rdx.h disagree");
constexpr int64_t FACET_TABLE_KB = 262144;   // the default budget of a pass's tables: 256 MiB (DESIGN.md §28 says why)

// what the two calls check alike before anything is enqueued (the caller holds the lock); on success the device is selected and the counters are zeroed
static int facet_begin(rdx_index* h, const char* who, const rdx_mask* mask, hipStream_t st) {
    RDX_TRY(check_mask(h, mask, who, RDX_ERR_INVALID));
    RDX_TRY(check_own_rows(h, who, "not available"));
    if (h->rows >= ((int64_t)1 << 31)) return fail(RDX_ERR_INVALID, std::string(who) + ": the table holds int32 codes per row: fewer than 2^31 rows");
    RDX_TRY(finish_pending(h, nullptr));
    RDX_TRY(set_device(h));
    RDX_TRY(h->fct_ctr.ensure(sizeof(FacetCounters)));
    HIP_TRY(hipMemsetAsync(h->fct_ctr.p, 0, sizeof(FacetCounters), st));
    return RDX_OK;
}

// the counters back on the host, the stream drained; a code outside the table's range fails the call
static int facet_end(rdx_index* h, const char* who, int64_t n_groups, hipStream_t st, FacetCounters* c) {
    HIP_TRY(hipMemcpyAsync(c, h->fct_ctr.p, sizeof(*c), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (c->bad)
        return fail(RDX_ERR_INVALID, std::string(who) + ": row_group holds a code outside -1 .. n_groups - 1 = " + std::to_string(n_groups - 1) +
                                         " (nothing was counted through it; the outputs are undefined)");
    return RDX_OK;
}

extern "C" int rdx_index_facet_count(rdx_index* h, const rdx_mask* mask, const int32_t* row_group, int64_t n_groups, int64_t* out_counts,
                                     int64_t* out_missing, int64_t* out_total, void* stream) {
    if (!h) return fail(RDX_ERR_INVALID, "rdx_index_facet_count: null index");
    if (n_groups < 0 || n_groups >= ((int64_t)1 << 31)) return fail(RDX_ERR_INVALID, "rdx_index_facet_count: n_groups must be in [0, 2^31)");
    if (!out_missing || !out_total || (n_groups > 0 && (!row_group || !out_counts))) return fail(RDX_ERR_INVALID, "rdx_index_facet_count: null pointer");
    if (((uintptr_t)row_group & 3) || ((uintptr_t)out_counts & 7)) return fail(RDX_ERR_INVALID, "rdx_index_facet_count: misaligned pointer");
    std::lock_guard<std::mutex> lk(h->mu);
    hipStream_t st = (hipStream_t)stream;
    RDX_TRY(facet_begin(h, "rdx_index_facet_count", mask, st));
    if (n_groups > 0) HIP_TRY(hipMemsetAsync(out_counts, 0, (size_t)n_groups * 8, st));
    if (h->rows > 0) {
        // a workgroup walks a span of rows, so that its table in LDS is zeroed and flushed once per span: eight workgroups per CU
        const int64_t tiles = (h->rows + 255) / 256;
        const int64_t span = (tiles + std::min<int64_t>(tiles, (int64_t)h->n_cu * 8) - 1) / std::min<int64_t>(tiles, (int64_t)h->n_cu * 8) * 256;
        const FacetCountParams fp = {mask ? mask->words.as<uint32_t>() : nullptr, n_groups > 0 ? row_group : nullptr, h->rows, n_groups,
                                     reinterpret_cast<unsigned long long*>(out_counts), h->fct_ctr.as<FacetCounters>(), span};
        hipLaunchKernelGGL(k_facet_count, dim3((unsigned)((h->rows + span - 1) / span)), dim3(256), 0, st, fp);
        HIP_TRY(hipGetLastError());
    }
    FacetCounters c = {};
    RDX_TRY(facet_end(h, "rdx_index_facet_count", n_groups, st, &c));
    *out_missing = (int64_t)c.missing;
    *out_total = (int64_t)c.total;
    return RDX_OK;
}

extern "C" int rdx_index_range_facets(rdx_index* h, const float* queries, int64_t nq, const float* thresholds, const rdx_mask* mask,
                                      const int32_t* row_group, int64_t n_groups, int limit, int32_t* out_code, int64_t* out_n,
                                      int32_t* out_found, int64_t* out_missing, int64_t* out_total, int32_t* out_paths, void* stream) {
    if (!h) return fail(RDX_ERR_INVALID, "rdx_index_range_facets: null index");
    if (limit < 1 || limit > RDX_FACET_MAX_LIMIT)
        return fail(RDX_ERR_INVALID, "rdx_index_range_facets: limit must be in [1, " + std::to_string(RDX_FACET_MAX_LIMIT) + "]");
    if (nq < 0 || nq > 65535) return fail(RDX_ERR_INVALID, "rdx_index_range_facets: nq must be in [0, 65535]");
    if (n_groups < 0 || n_groups >= ((int64_t)1 << 31)) return fail(RDX_ERR_INVALID, "rdx_index_range_facets: n_groups must be in [0, 2^31)");
    int32_t paths[2] = {0, 0};
    if (out_paths) out_paths[0] = out_paths[1] = 0;
    if (nq == 0) return RDX_OK;
    if (!queries || !thresholds || !row_group || !out_code || !out_n || !out_found || !out_missing || !out_total)
        return fail(RDX_ERR_INVALID, "rdx_index_range_facets: null pointer");
    if (((uintptr_t)queries & 15) || (((uintptr_t)out_n | (uintptr_t)out_missing | (uintptr_t)out_total) & 7) ||
        (((uintptr_t)thresholds | (uintptr_t)row_group | (uintptr_t)out_code | (uintptr_t)out_found) & 3))
        return fail(RDX_ERR_INVALID, "rdx_index_range_facets: misaligned pointer");
    std::lock_guard<std::mutex> lk(h->mu);
    hipStream_t st = (hipStream_t)stream;
    RDX_TRY(facet_begin(h, "rdx_index_range_facets", mask, st));
    // the queries of a pass share one table of n_groups cells each: as many queries as the budget holds, one at the least
    const int64_t budget = (h->facet_table_kb > 0 ? h->facet_table_kb : FACET_TABLE_KB) * 1024;
    const int64_t sub = std::max<int64_t>(1, std::min<int64_t>(RANGE_CHUNK, budget / std::max<int64_t>(n_groups * 4, 1)));
    const size_t row_bytes = (size_t)n_groups * 4;
    RDX_TRY(h->fct_tab.ensure(std::max<size_t>((size_t)std::min<int64_t>(sub, nq) * row_bytes, 16)));
    int* const d_bad = reinterpret_cast<int*>(h->fct_ctr.as<char>() + offsetof(FacetCounters, bad));
    for (int64_t q0 = 0; q0 < nq; q0 += sub) {
        const int64_t m = std::min(sub, nq - q0);
        if (row_bytes) HIP_TRY(hipMemsetAsync(h->fct_tab.p, 0, (size_t)m * row_bytes, st));
        const RangeIO io = {queries + (size_t)q0 * h->dim, thresholds + q0, mask ? mask->words.as<uint32_t>() : nullptr, nullptr, nullptr, nullptr,
                            out_total + q0};
        const FacetIO fc = {row_group, n_groups, h->fct_tab.as<uint32_t>(), out_missing + q0, d_bad};
        RDX_TRY(range_chunk(h, io, m, 1, st, paths, &fc));
        const FacetTopParams tp = {h->fct_tab.as<uint32_t>(), n_groups, limit, out_code + (size_t)q0 * limit, out_n + (size_t)q0 * limit, out_found + q0};
        hipLaunchKernelGGL(k_facet_top, dim3((unsigned)m), dim3(1024), 0, st, tp);
        HIP_TRY(hipGetLastError());
    }
    FacetCounters c = {};
    RDX_TRY(facet_end(h, "rdx_index_range_facets", n_groups, st, &c));
    if (out_paths) {
        out_paths[0] = paths[0];
        out_paths[1] = paths[1];
    }
    return RDX_OK;
}
