// rdx_maxsim.hip — the late-interaction scoring entry points (include/rdx.h rdx_maxsim_f16; kernel: maxsim_kernel.hpp) and their int8
// twins (rdx_maxsim_quantize_i8, rdx_maxsim_i8; kernels: maxsim_i8_kernel.hpp)
#include "maxsim_i8_kernel.hpp"
#include "maxsim_kernel.hpp"
#include "rdx_host.hpp"

using namespace rdx;

extern "C" int rdx_maxsim_f16(int device, const void* q_vecs, const int32_t* q_off, int nq, const void* d_vecs, int64_t d_rows,
                              const int64_t* slot_start, const int32_t* slot_len, int64_t n_slots, const int32_t* pair_q,
                              const int64_t* pair_slot, int64_t n_pairs, int dim, float* scores, void* stream) {
    static const char* fn = "rdx_maxsim_f16";
    if (dim < 32 || dim > MAXSIM_MAX_DIM || dim % 32) return fail(RDX_ERR_INVALID, "rdx_maxsim_f16: dim must be a multiple of 32 in [32, 1024]");
    if (nq < 1 || nq > MAXSIM_MAX_QUESTIONS) return fail(RDX_ERR_INVALID, "rdx_maxsim_f16: nq must be in [1, 65535]");
    if (n_pairs < 1 || n_pairs > MAXSIM_MAX_PAIRS) return fail(RDX_ERR_INVALID, "rdx_maxsim_f16: n_pairs must be in [1, 2^20]");
    if (d_rows < 1 || n_slots < 1) return fail(RDX_ERR_INVALID, "rdx_maxsim_f16: d_rows and n_slots must be at least 1");
    if (!q_vecs || !d_vecs || !slot_start || !slot_len || !pair_q || !pair_slot || !scores) return fail(RDX_ERR_INVALID, "rdx_maxsim_f16: null pointer");
    if ((((uintptr_t)q_vecs | (uintptr_t)d_vecs) & 15) || (((uintptr_t)slot_start | (uintptr_t)pair_slot) & 7) ||
        (((uintptr_t)slot_len | (uintptr_t)pair_q | (uintptr_t)scores) & 3))
        return fail(RDX_ERR_INVALID, "rdx_maxsim_f16: misaligned pointer (the token vectors are read in 16-byte pieces)");
    RDX_TRY(check_device_index(fn, device));
    HIP_TRY(hipSetDevice(device));
    const void* d_qoff;
    RDX_TRY(shape_array(fn, "q_off", q_off, 4, &d_qoff));
    if (q_off[0] < 0) return fail(RDX_ERR_INVALID, "rdx_maxsim_f16: q_off must start at 0 or above");
    int longest = 0;
    for (int q = 0; q < nq; ++q) {
        const int64_t n = (int64_t)q_off[q + 1] - q_off[q];
        if (n < 1 || n > MAXSIM_MAX_Q_TOKENS) return fail(RDX_ERR_INVALID, "rdx_maxsim_f16: a question has 1 to 256 token vectors (q_off must increase)");
        longest = std::max(longest, (int)n);
    }
    const int q_rows = longest > 32 ? MAXSIM_Q_BLOCK : 32;
    const size_t lds = maxsim_lds_bytes(dim, q_rows);
    RDX_TRY(dynamic_lds(device, reinterpret_cast<const void*>(k_maxsim), lds));
    hipLaunchKernelGGL(k_maxsim, dim3((unsigned)n_pairs), dim3(MAXSIM_THREADS), lds, (hipStream_t)stream, (const _Float16*)q_vecs,
                       (const int32_t*)d_qoff, nq, (const _Float16*)d_vecs, d_rows, slot_start, slot_len, n_slots, pair_q, pair_slot, dim, q_rows,
                       scores);
    HIP_TRY(hipGetLastError());
    return RDX_OK;
}

extern "C" int rdx_maxsim_quantize_i8(int device, const void* vecs_f16, int64_t rows, int dim, int8_t* codes, float* scales, void* stream) {
    static const char* fn = "rdx_maxsim_quantize_i8";
    if (dim < 32 || dim > MAXSIM_MAX_DIM || dim % 32) return fail(RDX_ERR_INVALID, "rdx_maxsim_quantize_i8: dim must be a multiple of 32 in [32, 1024]");
    if (rows < 1 || rows > (int64_t)INT32_MAX) return fail(RDX_ERR_INVALID, "rdx_maxsim_quantize_i8: rows must be in [1, 2^31 - 1]");
    if (!vecs_f16 || !codes || !scales) return fail(RDX_ERR_INVALID, "rdx_maxsim_quantize_i8: null pointer");
    if ((((uintptr_t)vecs_f16 | (uintptr_t)codes) & 15) || ((uintptr_t)scales & 3))
        return fail(RDX_ERR_INVALID, "rdx_maxsim_quantize_i8: misaligned pointer (vectors and codes move in 16- and 8-byte pieces)");
    RDX_TRY(check_device_index(fn, device));
    HIP_TRY(hipSetDevice(device));
    const unsigned grid = (unsigned)((rows + MAXSIM_QUANT_WAVES - 1) / MAXSIM_QUANT_WAVES);
    hipLaunchKernelGGL(k_maxsim_quant, dim3(grid), dim3(64 * MAXSIM_QUANT_WAVES), 0, (hipStream_t)stream, (const _Float16*)vecs_f16, rows, dim, codes,
                       scales);
    HIP_TRY(hipGetLastError());
    return RDX_OK;
}

extern "C" int rdx_maxsim_i8(int device, const int8_t* q_codes, const float* q_scales, const int32_t* q_off, int nq, const int8_t* d_codes,
                             const float* d_scales, int64_t d_rows, const int64_t* slot_start, const int32_t* slot_len, int64_t n_slots,
                             const int32_t* pair_q, const int64_t* pair_slot, int64_t n_pairs, int dim, float* scores, void* stream) {
    static const char* fn = "rdx_maxsim_i8";
    if (dim < 32 || dim > MAXSIM_MAX_DIM || dim % 32) return fail(RDX_ERR_INVALID, "rdx_maxsim_i8: dim must be a multiple of 32 in [32, 1024]");
    if (nq < 1 || nq > MAXSIM_MAX_QUESTIONS) return fail(RDX_ERR_INVALID, "rdx_maxsim_i8: nq must be in [1, 65535]");
    if (n_pairs < 1 || n_pairs > MAXSIM_MAX_PAIRS) return fail(RDX_ERR_INVALID, "rdx_maxsim_i8: n_pairs must be in [1, 2^20]");
    if (d_rows < 1 || n_slots < 1) return fail(RDX_ERR_INVALID, "rdx_maxsim_i8: d_rows and n_slots must be at least 1");
    if (!q_codes || !q_scales || !d_codes || !d_scales || !slot_start || !slot_len || !pair_q || !pair_slot || !scores)
        return fail(RDX_ERR_INVALID, "rdx_maxsim_i8: null pointer");
    if ((((uintptr_t)q_codes | (uintptr_t)d_codes) & 15) || (((uintptr_t)slot_start | (uintptr_t)pair_slot) & 7) ||
        (((uintptr_t)q_scales | (uintptr_t)d_scales | (uintptr_t)slot_len | (uintptr_t)pair_q | (uintptr_t)scores) & 3))
        return fail(RDX_ERR_INVALID, "rdx_maxsim_i8: misaligned pointer (the codes are read in 16-byte pieces)");
    RDX_TRY(check_device_index(fn, device));
    HIP_TRY(hipSetDevice(device));
    const void* d_qoff;
    RDX_TRY(shape_array(fn, "q_off", q_off, 4, &d_qoff));
    if (q_off[0] < 0) return fail(RDX_ERR_INVALID, "rdx_maxsim_i8: q_off must start at 0 or above");
    int longest = 0;
    for (int q = 0; q < nq; ++q) {
        const int64_t n = (int64_t)q_off[q + 1] - q_off[q];
        if (n < 1 || n > MAXSIM_MAX_Q_TOKENS) return fail(RDX_ERR_INVALID, "rdx_maxsim_i8: a question has 1 to 256 token vectors (q_off must increase)");
        longest = std::max(longest, (int)n);
    }
    const int q_rows = longest > 32 ? MAXSIM_Q_BLOCK : 32;
    const size_t lds = maxsim_i8_lds_bytes(dim, q_rows);
    RDX_TRY(dynamic_lds(device, reinterpret_cast<const void*>(k_maxsim_i8), lds));
    hipLaunchKernelGGL(k_maxsim_i8, dim3((unsigned)n_pairs), dim3(MAXSIM_THREADS), lds, (hipStream_t)stream, q_codes, q_scales, (const int32_t*)d_qoff,
                       nq, d_codes, d_scales, d_rows, slot_start, slot_len, n_slots, pair_q, pair_slot, dim, q_rows, scores);
    HIP_TRY(hipGetLastError());
    return RDX_OK;
}
