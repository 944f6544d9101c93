// rdx_m3.hip — the dense half and the sum of the combined BGE-M3 score (include/rdx.h rdx_index_score_pairs, rdx_m3_combine; kernels:
// m3_kernel.hpp). A unit of its own beside rdx_derived.hip: it reaches the index through rdx_index.hpp's host
// functions, includes no other unit's kernel header, and so leaves every other unit's kernels as they were. The lexical half
// (rdx_lex_score_pairs) lives with its handle in rdx_bm25.hip.
#include "rdx_index.hpp"

#include "m3_kernel.hpp"

extern "C" int rdx_index_score_pairs(rdx_index* h, const float* queries, int64_t nq, const int32_t* pair_q, const int64_t* pair_row,
                                     int64_t n_pairs, float* out_score, void* stream) {
    if (!h) return fail(RDX_ERR_INVALID, "rdx_index_score_pairs: null index");
    if (nq < 1 || nq > PAIRS_MAX_QUERIES) return fail(RDX_ERR_INVALID, "rdx_index_score_pairs: nq must be in [1, 65535]");
    if (n_pairs < 1 || n_pairs > PAIRS_MAX_PAIRS) return fail(RDX_ERR_INVALID, "rdx_index_score_pairs: n_pairs must be in [1, 2^20]");
    if (!queries || !pair_q || !pair_row || !out_score) return fail(RDX_ERR_INVALID, "rdx_index_score_pairs: null pointer");
    if (((uintptr_t)queries & 15) || ((uintptr_t)pair_row & 7) || (((uintptr_t)pair_q | (uintptr_t)out_score) & 3))
        return fail(RDX_ERR_INVALID, "rdx_index_score_pairs: misaligned pointer (the queries are read in 16-byte pieces)");
    std::lock_guard<std::mutex> lk(h->mu);
    RDX_TRY(check_own_rows(h, "rdx_index_score_pairs", "pair_row must be the index's own rows"));
    RDX_TRY(set_device(h));
    ScorePairsParams sp = {};
    sp.master = h->mv();
    sp.rows = h->rows;
    sp.dim = h->dim;
    sp.queries = queries;
    sp.nq = nq;
    sp.pair_q = pair_q;
    sp.pair_row = pair_row;
    sp.n_pairs = n_pairs;
    sp.out = out_score;
    hipLaunchKernelGGL(k_score_pairs, dim3((unsigned)((n_pairs + PAIRS_WAVES - 1) / PAIRS_WAVES)), dim3(64 * PAIRS_WAVES), 0, (hipStream_t)stream, sp);
    HIP_TRY(hipGetLastError());
    return RDX_OK;
}

extern "C" int rdx_m3_combine(int device, const float* dense, const double* sparse, const float* colbert, int64_t n, double w_dense,
                              double w_sparse, double w_colbert, float* out_final, double* out_value, void* stream) {
    static const char* fn = "rdx_m3_combine";
    if (n < 1 || n > PAIRS_MAX_PAIRS) return fail(RDX_ERR_INVALID, "rdx_m3_combine: n must be in [1, 2^20]");
    const double w[3] = {w_dense, w_sparse, w_colbert};
    for (double x : w)
        if (!std::isfinite(x) || x < 0.0) return fail(RDX_ERR_INVALID, "rdx_m3_combine: every weight must be finite and at least 0");
    const double w_sum = (w_dense + w_sparse) + w_colbert;
    if (!(w_sum > 0.0) || !std::isfinite(w_sum)) return fail(RDX_ERR_INVALID, "rdx_m3_combine: the weights' sum must be finite and above 0");
    if ((dense == nullptr) != (w_dense == 0.0) || (sparse == nullptr) != (w_sparse == 0.0) || (colbert == nullptr) != (w_colbert == 0.0))
        return fail(RDX_ERR_INVALID, "rdx_m3_combine: a component is a null pointer exactly when its weight is 0");
    if (!out_final) return fail(RDX_ERR_INVALID, "rdx_m3_combine: null out_final");
    if ((((uintptr_t)sparse | (uintptr_t)out_value) & 7) || (((uintptr_t)dense | (uintptr_t)colbert | (uintptr_t)out_final) & 3))
        return fail(RDX_ERR_INVALID, "rdx_m3_combine: misaligned pointer");
    RDX_TRY(check_device_index(fn, device));
    HIP_TRY(hipSetDevice(device));
    hipLaunchKernelGGL(k_m3_combine, dim3((unsigned)((n + M3_THREADS - 1) / M3_THREADS)), dim3(M3_THREADS), 0, (hipStream_t)stream, dense, sparse,
                       colbert, n, w_dense, w_sparse, w_colbert, w_sum, out_final, out_value);
    HIP_TRY(hipGetLastError());
    return RDX_OK;
}
