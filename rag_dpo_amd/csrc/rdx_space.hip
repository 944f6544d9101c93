// rdx_space.hip — the launchers of the inner-product / squared-L2 spaces (rdx_space_*) of include/rdx.h: space_kernel.hpp's
// kernels behind argument checks that run before the device is touched.
#include "rdx_host.hpp"

#include "space_kernel.hpp"

using namespace rdx;

static int space_common(const char* fn, int device, int kind, int dim) {
    if (kind != SPACE_IP && kind != SPACE_L2) return fail(RDX_ERR_INVALID, std::string(fn) + ": space_kind must be RDX_SPACE_IP or RDX_SPACE_L2");
    if (dim < 4 || dim % 4 != 0 || space_lifted_dim(kind, dim) > SPACE_MAX_DIM)
        return fail(RDX_ERR_INVALID, std::string(fn) + ": dim must be a positive multiple of 4 whose lifted form is at most 4096");
    return check_device_index(fn, device);
}

static unsigned space_grid(int64_t waves) { return (unsigned)((waves + SPACE_WAVES - 1) / SPACE_WAVES); }

extern "C" int rdx_space_measure(int device, int space_kind, const float* rows, int64_t n, int dim, double* lifted_sq, int32_t* bad,
                                 void* stream) {
    RDX_TRY(space_common("rdx_space_measure", device, space_kind, dim));
    if (n < 0 || n > (int64_t)1 << 31) return fail(RDX_ERR_INVALID, "rdx_space_measure: n must be in [0, 2^31]");
    if (n == 0) return RDX_OK;
    if (!rows || !lifted_sq || !bad) return fail(RDX_ERR_INVALID, "rdx_space_measure: null pointer");
    if (((uintptr_t)rows & 15) || ((uintptr_t)lifted_sq & 7) || ((uintptr_t)bad & 3)) return fail(RDX_ERR_INVALID, "rdx_space_measure: misaligned pointer");
    HIP_TRY(hipSetDevice(device));
    hipLaunchKernelGGL(k_space_measure, dim3(space_grid(n)), dim3(SPACE_THREADS), 0, (hipStream_t)stream, rows, n, dim, space_kind, lifted_sq, bad);
    HIP_TRY(hipGetLastError());
    return RDX_OK;
}

extern "C" int rdx_space_lift(int device, int space_kind, int is_query, const float* rows, int64_t n, int dim, int scale_exp, float* out,
                              int32_t* bad, void* stream) {
    RDX_TRY(space_common("rdx_space_lift", device, space_kind, dim));
    if (n < 0 || n > (int64_t)1 << 31) return fail(RDX_ERR_INVALID, "rdx_space_lift: n must be in [0, 2^31]");
    if (is_query != 0 && is_query != 1) return fail(RDX_ERR_INVALID, "rdx_space_lift: is_query must be 0 or 1");
    if (scale_exp < -300 || scale_exp > 300 || (is_query && scale_exp != 0))
        return fail(RDX_ERR_INVALID, "rdx_space_lift: scale_exp must be in [-300, 300], and 0 for queries");
    if (n == 0) return RDX_OK;
    if (!rows || !out || !bad) return fail(RDX_ERR_INVALID, "rdx_space_lift: null pointer");
    if ((((uintptr_t)rows | (uintptr_t)out) & 15) || ((uintptr_t)bad & 3)) return fail(RDX_ERR_INVALID, "rdx_space_lift: misaligned pointer");
    HIP_TRY(hipSetDevice(device));
    hipLaunchKernelGGL(k_space_lift, dim3(space_grid(n)), dim3(SPACE_THREADS), 0, (hipStream_t)stream, rows, n, dim, space_kind, is_query, scale_exp,
                       out, bad);
    HIP_TRY(hipGetLastError());
    return RDX_OK;
}

extern "C" int rdx_space_rescore(int device, int space_kind, const float* queries, int64_t nq, int dim, const float* cand_vecs,
                                 const int64_t* cand_rows, const float* cand_scores, const int32_t* cand_counts, int kp, int k,
                                 int scale_exp, double guard, float* work_dist, float* out_dist, int64_t* out_row, int32_t* out_count,
                                 int32_t* out_proven, void* stream) {
    RDX_TRY(space_common("rdx_space_rescore", device, space_kind, dim));
    if (nq < 0 || nq > 65535) return fail(RDX_ERR_INVALID, "rdx_space_rescore: nq must be in [0, 65535]");
    if (kp < 1 || kp > SPACE_MAX_CAND) return fail(RDX_ERR_INVALID, "rdx_space_rescore: the candidates per query must be in [1, 4096]");
    if (k < 1 || k > kp) return fail(RDX_ERR_INVALID, "rdx_space_rescore: k must be in [1, candidates per query]");
    if (scale_exp < -300 || scale_exp > 300) return fail(RDX_ERR_INVALID, "rdx_space_rescore: scale_exp must be in [-300, 300]");
    if (!(guard >= 0.0 && guard <= 1.0)) return fail(RDX_ERR_INVALID, "rdx_space_rescore: guard must be in [0, 1]");
    if (nq == 0) return RDX_OK;
    if (!queries || !cand_vecs || !cand_rows || !cand_scores || !cand_counts || !work_dist || !out_dist || !out_row || !out_count || !out_proven)
        return fail(RDX_ERR_INVALID, "rdx_space_rescore: null pointer");
    if (((uintptr_t)queries | (uintptr_t)cand_vecs) & 15) return fail(RDX_ERR_INVALID, "rdx_space_rescore: queries and cand_vecs must be 16-byte aligned");
    if (((uintptr_t)cand_rows | (uintptr_t)out_row) & 7) return fail(RDX_ERR_INVALID, "rdx_space_rescore: misaligned pointer");
    if (((uintptr_t)cand_scores | (uintptr_t)cand_counts | (uintptr_t)work_dist | (uintptr_t)out_dist | (uintptr_t)out_count | (uintptr_t)out_proven) & 3)
        return fail(RDX_ERR_INVALID, "rdx_space_rescore: misaligned pointer");
    HIP_TRY(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_space_cand, dim3(space_grid(nq * kp)), dim3(SPACE_THREADS), 0, st, queries, nq, dim, space_kind, cand_vecs, cand_counts,
                       kp, scale_exp, work_dist);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_space_select, dim3((unsigned)nq), dim3(SPACE_THREADS), 0, st, queries, dim, space_kind, (const float*)work_dist, cand_rows,
                       cand_scores, cand_counts, kp, k, scale_exp, guard, out_dist, out_row, out_count, out_proven);
    HIP_TRY(hipGetLastError());
    return RDX_OK;
}

extern "C" int rdx_space_distances(int device, int space_kind, const float* queries, int nq, int dim, const float* vecs, int64_t n,
                                   int scale_exp, const uint32_t* allow_bits, int64_t first_row, float* out, int64_t out_stride,
                                   void* stream) {
    RDX_TRY(space_common("rdx_space_distances", device, space_kind, dim));
    if (nq < 0 || nq > SPACE_MAX_PAGE_QUERIES) return fail(RDX_ERR_INVALID, "rdx_space_distances: nq must be in [0, 64]");
    if (n < 0 || n > (int64_t)1 << 24) return fail(RDX_ERR_INVALID, "rdx_space_distances: a page holds at most 2^24 rows");
    if (first_row < 0 || out_stride < n) return fail(RDX_ERR_INVALID, "rdx_space_distances: first_row must be >= 0 and out_stride >= n");
    if (scale_exp < -300 || scale_exp > 300) return fail(RDX_ERR_INVALID, "rdx_space_distances: scale_exp must be in [-300, 300]");
    if (nq == 0 || n == 0) return RDX_OK;
    if (!queries || !vecs || !out) return fail(RDX_ERR_INVALID, "rdx_space_distances: null pointer");
    if (((uintptr_t)queries | (uintptr_t)vecs) & 15) return fail(RDX_ERR_INVALID, "rdx_space_distances: queries and vecs must be 16-byte aligned");
    if (((uintptr_t)allow_bits | (uintptr_t)out) & 3) return fail(RDX_ERR_INVALID, "rdx_space_distances: misaligned pointer");
    HIP_TRY(hipSetDevice(device));
    hipLaunchKernelGGL(k_space_page, dim3(space_grid(n * nq)), dim3(SPACE_THREADS), 0, (hipStream_t)stream, queries, nq, dim, space_kind, vecs, n,
                       scale_exp, allow_bits, first_row, out, out_stride);
    HIP_TRY(hipGetLastError());
    return RDX_OK;
}
