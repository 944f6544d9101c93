// rdx_bm25.hip — sparse retrieval over a CSR-by-term index: BM25 (rdx_bm25_*) and BGE-M3 lexical weights (rdx_lex_create / _destroy /
// _search / _score_pairs) of include/rdx.h. Both indexes are one host core (SparseIndex: create, upload, search) and one merge; they differ in what a
// posting holds and in the scoring kernel (bm25_kernel.hpp k_bm25_score / k_lex_score). The score of named (question, row) pairs of a
// lexical index (lex_pairs_kernel.hpp k_lex_score_pairs) is here because the handle is.
#include "rdx_host.hpp"

#include <cmath>
#include <mutex>
#include <vector>

#include "bm25_kernel.hpp"
#include "lex_pairs_kernel.hpp"

using namespace rdx;

// ------------------------------------------------------------------------------------------------
// the immutable index both kinds share: rebuilt to refresh, as in the reference
// ------------------------------------------------------------------------------------------------
struct SparseIndex {
    int device = 0;
    int64_t n_rows = 0, n_terms = 0, nnz = 0, n_dir = 0;
    int32_t n_groups = 0;
    int n_tiles = 0;
    DevBuf post_off, post_row, post_val, dir_off, dir_tile, dir_pos, group;   // post_val: uint16 per posting (tf, or fp16 weight bits)
    DevBuf idf, denom;             // BM25's own tables (empty in a lexical index): here, so that one destructor frees everything on `device`
    DevBuf in, part, out;          // per search: packed inputs, tile partials, packed outputs
    PinnedBuf h_in, h_out;
    hipStream_t own_stream = nullptr;
    std::mutex mu;                 // searches are synchronous: one at a time owns the buffers
    ~SparseIndex() {
        (void)hipSetDevice(device);
        if (own_stream) {
            (void)hipStreamSynchronize(own_stream);
            (void)hipStreamDestroy(own_stream);
        }
    }
};

struct rdx_bm25 : SparseIndex {};

struct rdx_lex : SparseIndex {};

static size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

static int sparse_upload(DevBuf& d, const void* src, size_t bytes) {
    RDX_TRY(d.ensure(std::max(bytes, (size_t)16)));
    if (bytes) HIP_TRY(hipMemcpy(d.p, src, bytes, hipMemcpyHostToDevice));
    return RDX_OK;
}

// The checks and the uploads of a create that both kinds share: the shape, the groups, the postings (term_ok(t) and value_ok(v) are the
// kind's own checks of a term and of a posting's 16-bit value; bad_value names a refused one) and the per-term tile directory, built in
// the same pass. `me` = "rdx_x_create".
template <class TermOk, class ValueOk>
static int sparse_create(const std::string& me, SparseIndex* h, int device, int64_t n_rows, int64_t n_terms, const int64_t* post_off,
                         const int32_t* post_row, const uint16_t* post_val, const int32_t* row_group, int32_t n_groups, TermOk term_ok,
                         ValueOk value_ok, const char* bad_value) {
    const int64_t nnz = post_off[n_terms];
    std::vector<int64_t> h_dir_off((size_t)n_terms + 1), h_dir_pos;
    std::vector<int32_t> h_dir_tile;
    for (int64_t t = 0; t < n_terms; ++t) {
        RDX_TRY(term_ok(t));
        const int64_t b = post_off[t], e = post_off[t + 1];
        if (e < b || e > nnz) return fail(RDX_ERR_INVALID, me + ": post_off must be non-decreasing up to post_off[n_terms]");
        h_dir_off[(size_t)t] = (int64_t)h_dir_tile.size();
        int32_t prev_row = -1, prev_tile = -1;
        for (int64_t p = b; p < e; ++p) {
            const int32_t r = post_row[p];
            if (r <= prev_row || r >= n_rows)
                return fail(RDX_ERR_INVALID, me + ": term " + std::to_string(t) + ": rows must be strictly ascending and < n_rows");
            if (!value_ok(post_val[p])) return fail(RDX_ERR_INVALID, me + ": term " + std::to_string(t) + ": " + bad_value);
            prev_row = r;
            const int32_t tile = r / BM25_TILE;
            if (tile != prev_tile) {
                h_dir_tile.push_back(tile);
                h_dir_pos.push_back(p);
                prev_tile = tile;
            }
        }
    }
    h_dir_off[(size_t)n_terms] = (int64_t)h_dir_tile.size();
    h_dir_pos.push_back(nnz);

    HIP_TRY(hipSetDevice(device));
    h->device = device;
    h->n_rows = n_rows;
    h->n_terms = n_terms;
    h->nnz = nnz;
    h->n_dir = (int64_t)h_dir_tile.size();
    h->n_groups = n_groups;
    h->n_tiles = (int)((n_rows + BM25_TILE - 1) / BM25_TILE);
    RDX_TRY(sparse_upload(h->post_off, post_off, (size_t)(n_terms + 1) * 8));
    RDX_TRY(sparse_upload(h->post_row, post_row, (size_t)nnz * 4));
    RDX_TRY(sparse_upload(h->post_val, post_val, (size_t)nnz * 2));
    RDX_TRY(sparse_upload(h->dir_off, h_dir_off.data(), h_dir_off.size() * 8));
    RDX_TRY(sparse_upload(h->dir_tile, h_dir_tile.data(), h_dir_tile.size() * 4));
    RDX_TRY(sparse_upload(h->dir_pos, h_dir_pos.data(), h_dir_pos.size() * 8));
    if (row_group) RDX_TRY(sparse_upload(h->group, row_group, (size_t)n_rows * 4));
    hipError_t e = hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking);
    if (e != hipSuccess) return fail(RDX_ERR_HIP, me + ": " + hipGetErrorString(e));
    return RDX_OK;
}

// the argument checks every create starts with; tables_missing: a table of the kind's own is a null pointer
static int sparse_create_args(const std::string& me, int64_t n_rows, int64_t n_terms, const int64_t* post_off, const int32_t* post_row,
                              const uint16_t* post_val, const int32_t* row_group, int32_t n_groups, bool tables_missing) {
    if (n_rows < 1 || n_rows > INT32_MAX - BM25_TILE || n_terms < 0 || n_terms >= INT32_MAX)
        return fail(RDX_ERR_INVALID, me + ": n_rows must be in [1, 2^31 - 4097] and n_terms in [0, 2^31 - 1)");
    if (!post_off || tables_missing) return fail(RDX_ERR_INVALID, me + ": null pointer");
    if ((row_group == nullptr) != (n_groups == 0) || n_groups < 0)
        return fail(RDX_ERR_INVALID, me + ": row_group and n_groups > 0 go together");
    const int64_t nnz = post_off[n_terms];
    if (post_off[0] != 0 || nnz < 0) return fail(RDX_ERR_INVALID, me + ": post_off must start at 0");
    if (nnz > 0 && (!post_row || !post_val)) return fail(RDX_ERR_INVALID, me + ": null postings");
    if (row_group)
        for (int64_t r = 0; r < n_rows; ++r)
            if (row_group[r] < 0 || row_group[r] >= n_groups)
                return fail(RDX_ERR_INVALID, me + ": row_group[" + std::to_string(r) + "] out of [0, n_groups)");
    return RDX_OK;
}

extern "C" int rdx_bm25_create(int device, int64_t n_rows, int64_t n_terms, const int64_t* post_off, const int32_t* post_row,
                               const uint16_t* post_tf, const double* idf, const double* row_denom, const int32_t* row_group,
                               int32_t n_groups, rdx_bm25** out) {
    const std::string me = "rdx_bm25_create";
    if (!out) return fail(RDX_ERR_INVALID, me + ": null out pointer");
    *out = nullptr;
    RDX_TRY(sparse_create_args(me, n_rows, n_terms, post_off, post_row, post_tf, row_group, n_groups, !row_denom || (n_terms > 0 && !idf)));
    for (int64_t r = 0; r < n_rows; ++r)
        if (!(row_denom[r] > 0.0) || !std::isfinite(row_denom[r]))
            return fail(RDX_ERR_INVALID, me + ": row_denom[" + std::to_string(r) + "] is not a positive finite number");
    rdx_bm25* h = new rdx_bm25();
    int rc = sparse_create(
        me, h, device, n_rows, n_terms, post_off, post_row, post_tf, row_group, n_groups,
        [&](int64_t t) { return std::isfinite(idf[t]) ? RDX_OK : fail(RDX_ERR_INVALID, me + ": idf[" + std::to_string(t) + "] is not finite"); },
        [](uint16_t tf) { return tf != 0; }, "tf 0 in a posting");
    if (rc == RDX_OK) rc = sparse_upload(h->idf, idf, (size_t)n_terms * 8);
    if (rc == RDX_OK) rc = sparse_upload(h->denom, row_denom, (size_t)n_rows * 8);
    if (rc != RDX_OK) {
        delete h;
        return rc;
    }
    *out = h;
    return RDX_OK;
}

extern "C" int rdx_bm25_destroy(rdx_bm25* h) {
    delete h;
    return RDX_OK;
}

// fp16 bits of a finite value > 0: sign clear, not zero, exponent below the infinities'
static bool lex_weight_ok(uint16_t bits) { return bits >= 1 && bits <= 0x7BFF; }

extern "C" int rdx_lex_create(int device, int64_t n_rows, int64_t n_terms, const int64_t* post_off, const int32_t* post_row,
                              const uint16_t* post_w, const int32_t* row_group, int32_t n_groups, rdx_lex** out) {
    const std::string me = "rdx_lex_create";
    if (!out) return fail(RDX_ERR_INVALID, me + ": null out pointer");
    *out = nullptr;
    RDX_TRY(sparse_create_args(me, n_rows, n_terms, post_off, post_row, post_w, row_group, n_groups, false));
    rdx_lex* h = new rdx_lex();
    const int rc = sparse_create(me, h, device, n_rows, n_terms, post_off, post_row, post_w, row_group, n_groups,
                                 [](int64_t) { return RDX_OK; }, lex_weight_ok, "a weight that is not a finite fp16 above 0");
    if (rc != RDX_OK) {
        delete h;
        return rc;
    }
    *out = h;
    return RDX_OK;
}

extern "C" int rdx_lex_destroy(rdx_lex* h) {
    delete h;
    return RDX_OK;
}

// The one search behind rdx_bm25_search, rdx_bm25_search_filtered and rdx_lex_search (`who` names the caller in messages). The filters
// are a table of n_filters bitsets and, per query, its row of the table or -1; query_filter == nullptr gives every query
// `uniform_filter`. term_w != nullptr is the lexical search: a weight per term travels behind the ids, the ids of a query must be
// strictly ascending and the weights finite and positive. `score(nqc, ...)` launches the kind's scoring kernel for one chunk of queries.
template <class Score>
static int sparse_search(const char* who, SparseIndex* h, const int64_t* term_offsets, const int32_t* term_ids, const uint16_t* term_w,
                         bool weighted, int64_t nq, int k, const uint32_t* filter_sets, int32_t n_filters, const int32_t* query_filter,
                         int32_t uniform_filter, double* out_score, int64_t* out_row, int32_t* out_count, int space, void* stream,
                         Score score) {
    const std::string me = who;
    if (!h) return fail(RDX_ERR_INVALID, me + ": null index");
    if (nq < 0 || k < 1 || k > BM25_MAX_K)
        return fail(RDX_ERR_INVALID, me + ": need nq >= 0 and 1 <= k <= " + std::to_string(BM25_MAX_K) + " (got k = " +
                                         std::to_string(k) + ")");
    if (space != RDX_HOST) return fail(RDX_ERR_INVALID, me + ": space must be RDX_HOST (the terms are checked on the host)");
    if (n_filters < 0) return fail(RDX_ERR_INVALID, me + ": n_filters = " + std::to_string(n_filters) + " is negative");
    if (n_filters > 0 && h->n_groups == 0) return fail(RDX_ERR_INVALID, me + ": a group filter on an index without groups");
    if (n_filters > 0 && !filter_sets)
        return fail(RDX_ERR_INVALID, me + ": null filter_sets with n_filters = " + std::to_string(n_filters));
    if (nq == 0) return RDX_OK;
    if (!term_offsets || !out_score || !out_row || !out_count) return fail(RDX_ERR_INVALID, me + ": null pointer");
    if (query_filter)
        for (int64_t q = 0; q < nq; ++q)
            if (query_filter[q] < -1 || query_filter[q] >= n_filters)
                return fail(RDX_ERR_INVALID, me + ": query_filter[" + std::to_string(q) + "] = " + std::to_string(query_filter[q]) +
                                                 " out of [-1, " + std::to_string(n_filters) + ")");
    std::lock_guard<std::mutex> lock(h->mu);
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = stream ? (hipStream_t)stream : h->own_stream;

    // the query terms are checked before anything is enqueued
    const int64_t* off = term_offsets;
    if (off[0] != 0) return fail(RDX_ERR_INVALID, me + ": term_offsets[0] must be 0");
    for (int64_t q = 0; q < nq; ++q) {
        const int64_t T = off[q + 1] - off[q];
        if (T < 0 || T > BM25_MAX_TERMS)
            return fail(RDX_ERR_INVALID, me + ": query " + std::to_string(q) + " has " + std::to_string(T) + " terms (0.." +
                                             std::to_string(BM25_MAX_TERMS) + ")");
    }
    const int64_t n_ids = off[nq];
    if (n_ids > 0 && (!term_ids || (weighted && !term_w))) return fail(RDX_ERR_INVALID, me + (term_ids ? ": null term_w" : ": null term_ids"));
    for (int64_t i = 0; i < n_ids; ++i)
        if (term_ids[i] < 0 || term_ids[i] >= h->n_terms)
            return fail(RDX_ERR_INVALID, me + ": term id " + std::to_string(term_ids[i]) + " out of [0, " +
                                             std::to_string(h->n_terms) + ")");
    if (weighted)
        for (int64_t q = 0; q < nq; ++q)
            for (int64_t i = off[q]; i < off[q + 1]; ++i) {
                if (i > off[q] && term_ids[i] <= term_ids[i - 1])
                    return fail(RDX_ERR_INVALID, me + ": query " + std::to_string(q) + ": term id " + std::to_string(term_ids[i]) + " after " +
                                                     std::to_string(term_ids[i - 1]) + " (the ids of a query must be strictly ascending)");
                if (!lex_weight_ok(term_w[i]))
                    return fail(RDX_ERR_INVALID, me + ": query " + std::to_string(q) + ": term id " + std::to_string(term_ids[i]) +
                                                     " has weight bits " + std::to_string(term_w[i]) + " (not a finite fp16 above 0)");
            }

    // one upload through pinned staging: offsets | ids | weights (the lexical search's) | query_filter | filter sets
    const size_t allow_words = (size_t)(h->n_groups + 31) / 32;
    const size_t b_off = align16((size_t)(nq + 1) * 8), b_ids = align16((size_t)std::max<int64_t>(n_ids, 1) * 4);
    const size_t b_w = weighted ? align16((size_t)std::max<int64_t>(n_ids, 1) * 2) : 0;
    const size_t b_qf = align16((size_t)nq * 4), n_set_bytes = (size_t)n_filters * allow_words * 4;
    const size_t b_in = b_off + b_ids + b_w + b_qf + align16(n_set_bytes);
    RDX_TRY(h->h_in.ensure(b_in));
    RDX_TRY(h->in.ensure(b_in));
    char* hp = (char*)h->h_in.p;
    std::memcpy(hp, term_offsets, (size_t)(nq + 1) * 8);
    if (n_ids) std::memcpy(hp + b_off, term_ids, (size_t)n_ids * 4);
    if (weighted && n_ids) std::memcpy(hp + b_off + b_ids, term_w, (size_t)n_ids * 2);
    int32_t* h_qf = (int32_t*)(hp + b_off + b_ids + b_w);
    if (query_filter) std::memcpy(h_qf, query_filter, (size_t)nq * 4);
    else std::fill(h_qf, h_qf + nq, uniform_filter);
    if (n_set_bytes) std::memcpy(hp + b_off + b_ids + b_w + b_qf, filter_sets, n_set_bytes);
    HIP_TRY(hipMemcpyAsync(h->in.p, hp, b_in, hipMemcpyHostToDevice, st));
    const int64_t* d_off = (const int64_t*)h->in.p;
    const int32_t* d_ids = (const int32_t*)((char*)h->in.p + b_off);
    const uint16_t* d_w = (const uint16_t*)((char*)h->in.p + b_off + b_ids);                 // never read when not weighted
    const int32_t* d_qf = (const int32_t*)((char*)h->in.p + b_off + b_ids + b_w);
    const uint32_t* d_sets = (const uint32_t*)((char*)h->in.p + b_off + b_ids + b_w + b_qf);   // never read when n_filters = 0
    const size_t b_score = align16((size_t)nq * k * 8), b_row = align16((size_t)nq * k * 8), b_cnt = align16((size_t)nq * 4);
    RDX_TRY(h->out.ensure(b_score + b_row + b_cnt));
    double* o_score = (double*)h->out.p;
    int64_t* o_row = (int64_t*)((char*)h->out.p + b_score);
    int32_t* o_cnt = (int32_t*)((char*)h->out.p + b_score + b_row);
    // queries go in chunks whose tile partials fit 256 MiB
    const size_t per_query = (size_t)h->n_tiles * k * 12 + (size_t)h->n_tiles * 4;
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>({nq, (int64_t)((size_t)256 << 20) / (int64_t)per_query, 65535}));
    const size_t c_score = align16((size_t)chunk * h->n_tiles * k * 8), c_row = align16((size_t)chunk * h->n_tiles * k * 4);
    RDX_TRY(h->part.ensure(c_score + c_row + align16((size_t)chunk * h->n_tiles * 4)));
    double* p_score = h->part.as<double>();
    int32_t* p_row = (int32_t*)((char*)h->part.p + c_score);
    int32_t* p_cnt = (int32_t*)((char*)h->part.p + c_score + c_row);
    for (int64_t q0 = 0; q0 < nq; q0 += chunk) {
        const int nqc = (int)std::min<int64_t>(chunk, nq - q0);
        score(nqc, st, d_sets, (int)allow_words, d_qf + q0, d_off + q0, d_ids, d_w, k, p_score, p_row, p_cnt);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_bm25_merge, dim3(nqc), dim3(BM25_MERGE_THREADS), 0, st, p_score, p_row, p_cnt, h->n_tiles, k,
                           o_score + (size_t)q0 * k, o_row + (size_t)q0 * k, o_cnt + q0);
        HIP_TRY(hipGetLastError());
    }
    // one download, then out of the pinned staging
    RDX_TRY(h->h_out.ensure(b_score + b_row + b_cnt));
    HIP_TRY(hipMemcpyAsync(h->h_out.p, h->out.p, b_score + b_row + b_cnt, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const char* ho = (const char*)h->h_out.p;
    std::memcpy(out_score, ho, (size_t)nq * k * 8);
    std::memcpy(out_row, ho + b_score, (size_t)nq * k * 8);
    std::memcpy(out_count, ho + b_score + b_row, (size_t)nq * 4);
    return RDX_OK;
}

static int bm25_search(const char* who, rdx_bm25* h, const int64_t* term_offsets, const int32_t* term_ids, int64_t nq, int k,
                       const uint32_t* filter_sets, int32_t n_filters, const int32_t* query_filter, int32_t uniform_filter,
                       double* out_score, int64_t* out_row, int32_t* out_count, int space, void* stream) {
    return sparse_search(who, h, term_offsets, term_ids, nullptr, false, nq, k, filter_sets, n_filters, query_filter, uniform_filter,
                         out_score, out_row, out_count, space, stream,
                         [h](int nqc, hipStream_t st, const uint32_t* d_sets, int allow_words, const int32_t* d_qf, const int64_t* d_off,
                             const int32_t* d_ids, const uint16_t*, int k, double* p_score, int32_t* p_row, int32_t* p_cnt) {
                             hipLaunchKernelGGL(k_bm25_score, dim3(h->n_tiles, nqc), dim3(BM25_THREADS), 0, st, h->dir_off.as<int64_t>(),
                                                h->dir_tile.as<int32_t>(), h->dir_pos.as<int64_t>(), h->post_row.as<int32_t>(),
                                                h->post_val.as<uint16_t>(), h->idf.as<double>(), h->denom.as<double>(),
                                                h->group.as<int32_t>(), d_sets, allow_words, d_qf, d_off, d_ids, h->n_rows, k, h->n_tiles,
                                                p_score, p_row, p_cnt);
                         });
}

extern "C" int rdx_bm25_search(rdx_bm25* h, const int64_t* term_offsets, const int32_t* term_ids, int64_t nq, int k,
                               const uint32_t* allow_groups, double* out_score, int64_t* out_row, int32_t* out_count, int space,
                               void* stream) {
    // one bitset for every query = a table of one row
    return bm25_search("rdx_bm25_search", h, term_offsets, term_ids, nq, k, allow_groups, allow_groups ? 1 : 0, nullptr,
                       allow_groups ? 0 : -1, out_score, out_row, out_count, space, stream);
}

extern "C" int rdx_bm25_search_filtered(rdx_bm25* h, const int64_t* term_offsets, const int32_t* term_ids, int64_t nq, int k,
                                        const uint32_t* filter_sets, int32_t n_filters, const int32_t* query_filter,
                                        double* out_score, int64_t* out_row, int32_t* out_count, int space, void* stream) {
    if (nq > 0 && !query_filter) return fail(RDX_ERR_INVALID, "rdx_bm25_search_filtered: null query_filter with nq = " + std::to_string(nq));
    return bm25_search("rdx_bm25_search_filtered", h, term_offsets, term_ids, nq, k, filter_sets, n_filters, query_filter, -1,
                       out_score, out_row, out_count, space, stream);
}

extern "C" int rdx_lex_search(rdx_lex* h, const int64_t* term_offsets, const int32_t* term_ids, const uint16_t* term_w, int64_t nq, int k,
                              const uint32_t* filter_sets, int32_t n_filters, const int32_t* query_filter, double* out_score,
                              int64_t* out_row, int32_t* out_count, int space, void* stream) {
    if (nq > 0 && !query_filter) return fail(RDX_ERR_INVALID, "rdx_lex_search: null query_filter with nq = " + std::to_string(nq));
    return sparse_search("rdx_lex_search", h, term_offsets, term_ids, term_w, true, nq, k, filter_sets, n_filters, query_filter, -1,
                         out_score, out_row, out_count, space, stream,
                         [h](int nqc, hipStream_t st, const uint32_t* d_sets, int allow_words, const int32_t* d_qf, const int64_t* d_off,
                             const int32_t* d_ids, const uint16_t* d_w, int k, double* p_score, int32_t* p_row, int32_t* p_cnt) {
                             hipLaunchKernelGGL(k_lex_score, dim3(h->n_tiles, nqc), dim3(BM25_THREADS), 0, st, h->dir_off.as<int64_t>(),
                                                h->dir_tile.as<int32_t>(), h->dir_pos.as<int64_t>(), h->post_row.as<int32_t>(),
                                                h->post_val.as<uint16_t>(), h->group.as<int32_t>(), d_sets, allow_words, d_qf, d_off, d_ids,
                                                d_w, h->n_rows, k, h->n_tiles, p_score, p_row, p_cnt);
                         });
}

// ---- the lexical score of named pairs --------------------------------------------------------------------------------
static_assert(LEX_PAIRS_MAX_TERMS == BM25_MAX_TERMS, "a question the pair call admits is one the search admits");

extern "C" int rdx_lex_score_pairs(rdx_lex* h, const int64_t* term_offsets, const int32_t* term_ids, const uint16_t* term_w, int64_t nq,
                                   const int32_t* pair_q, const int64_t* pair_row, int64_t n_pairs, double* out_score, void* stream) {
    static const char* fn = "rdx_lex_score_pairs";
    if (!h) return fail(RDX_ERR_INVALID, "rdx_lex_score_pairs: null index");
    if (nq < 1 || nq > LEX_PAIRS_MAX_QUESTIONS) return fail(RDX_ERR_INVALID, "rdx_lex_score_pairs: nq must be in [1, 65535]");
    if (n_pairs < 1 || n_pairs > LEX_PAIRS_MAX_PAIRS) return fail(RDX_ERR_INVALID, "rdx_lex_score_pairs: n_pairs must be in [1, 2^20]");
    if (!pair_q || !pair_row || !out_score) return fail(RDX_ERR_INVALID, "rdx_lex_score_pairs: null pointer");
    if ((((uintptr_t)pair_row | (uintptr_t)out_score) & 7) || (((uintptr_t)pair_q | (uintptr_t)term_ids) & 3) || ((uintptr_t)term_w & 1))
        return fail(RDX_ERR_INVALID, "rdx_lex_score_pairs: misaligned pointer");
    HIP_TRY(hipSetDevice(h->device));
    const void* d_off;
    RDX_TRY(shape_array(fn, "term_offsets", term_offsets, 8, &d_off));
    if (term_offsets[0] < 0) return fail(RDX_ERR_INVALID, "rdx_lex_score_pairs: term_offsets must start at 0 or above");
    for (int64_t q = 0; q < nq; ++q) {
        const int64_t T = term_offsets[q + 1] - term_offsets[q];
        if (T < 0 || T > LEX_PAIRS_MAX_TERMS)
            return fail(RDX_ERR_INVALID, "rdx_lex_score_pairs: question " + std::to_string(q) + " has " + std::to_string(T) + " terms (0.." +
                                             std::to_string(LEX_PAIRS_MAX_TERMS) + "; term_offsets must not decrease)");
    }
    if (term_offsets[nq] > 0 && (!term_ids || !term_w)) return fail(RDX_ERR_INVALID, "rdx_lex_score_pairs: null term_ids or term_w");
    LexPairsParams lp = {};
    lp.post_off = h->post_off.as<int64_t>();
    lp.post_row = h->post_row.as<int32_t>();
    lp.post_w = h->post_val.as<uint16_t>();
    lp.dir_off = h->dir_off.as<int64_t>();
    lp.dir_tile = h->dir_tile.as<int32_t>();
    lp.dir_pos = h->dir_pos.as<int64_t>();
    lp.n_rows = h->n_rows;
    lp.n_terms = h->n_terms;
    lp.q_off = (const int64_t*)d_off;
    lp.q_terms = term_ids;
    lp.q_w = term_w;
    lp.nq = nq;
    lp.pair_q = pair_q;
    lp.pair_row = pair_row;
    lp.n_pairs = n_pairs;
    lp.out = out_score;
    hipLaunchKernelGGL(k_lex_score_pairs, dim3((unsigned)((n_pairs + LEX_PAIRS_WAVES - 1) / LEX_PAIRS_WAVES)), dim3(64 * LEX_PAIRS_WAVES), 0,
                       (hipStream_t)stream, lp);
    HIP_TRY(hipGetLastError());
    return RDX_OK;
}
