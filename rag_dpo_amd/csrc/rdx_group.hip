// rdx_group.hip — the launcher of rdx_group_select (include/rdx.h): group_kernel.hpp's kernel behind argument checks that run before
// the device is touched. Device pointers only, one launch on the caller's stream, nothing allocated or synchronised; independent of
// any index, like rdx_rerank_select.
#include "rdx_host.hpp"

#include "group_kernel.hpp"

using namespace rdx;

static_assert(GROUP_MAX_K == RDX_GROUP_MAX_K && GROUP_MAX_GROUPS == RDX_GROUP_MAX_GROUPS && GROUP_MAX_SIZE == RDX_GROUP_MAX_SIZE,
              "group_kernel.hpp and include/rdx.h disagree");

extern "C" int rdx_group_select(int device, const float* scores, const int64_t* rows, const int32_t* counts, int64_t nq, int k,
                                const int32_t* row_group, int64_t n_rows, const int64_t* group_off, int64_t n_groups, int n_want,
                                int group_size, float* out_score, int64_t* out_row, int32_t* out_count, int32_t* out_code,
                                int32_t* out_complete, int32_t* out_found, int32_t* out_short, int32_t* out_bad, void* stream) {
    RDX_TRY(check_device_index("rdx_group_select", device));
    if (nq < 0 || nq > 65535) return fail(RDX_ERR_INVALID, "rdx_group_select: nq must be in [0, 65535]");
    if (k < 1 || k > GROUP_MAX_K) return fail(RDX_ERR_INVALID, "rdx_group_select: k (the entries per list) must be in [1, 4096]");
    if (n_want < 1 || n_want > GROUP_MAX_GROUPS) return fail(RDX_ERR_INVALID, "rdx_group_select: the groups per query must be in [1, 64]");
    if (group_size < 1 || group_size > GROUP_MAX_SIZE) return fail(RDX_ERR_INVALID, "rdx_group_select: the rows per group must be in [1, 16]");
    if (n_rows < 0 || n_groups < 0 || n_groups > 0x7fffffff) return fail(RDX_ERR_INVALID, "rdx_group_select: n_rows must be >= 0 and n_groups in [0, 2^31)");
    if (nq == 0) return RDX_OK;
    if (!scores || !rows || !counts || !group_off || (n_rows > 0 && !row_group)) return fail(RDX_ERR_INVALID, "rdx_group_select: null input pointer");
    if (!out_score || !out_row || !out_count || !out_code || !out_complete || !out_found || !out_short || !out_bad)
        return fail(RDX_ERR_INVALID, "rdx_group_select: null output pointer");
    if (((uintptr_t)rows | (uintptr_t)group_off | (uintptr_t)out_row) & 7) return fail(RDX_ERR_INVALID, "rdx_group_select: misaligned pointer");
    if (((uintptr_t)scores | (uintptr_t)counts | (uintptr_t)row_group | (uintptr_t)out_score | (uintptr_t)out_count | (uintptr_t)out_code |
         (uintptr_t)out_complete | (uintptr_t)out_found | (uintptr_t)out_short | (uintptr_t)out_bad) & 3)
        return fail(RDX_ERR_INVALID, "rdx_group_select: misaligned pointer");
    GroupSelectArgs a;
    a.scores = scores;
    a.rows = rows;
    a.counts = counts;
    a.k = k;
    a.row_group = row_group;
    a.n_rows = n_rows;
    a.group_off = group_off;
    a.n_groups = n_groups;
    a.G = n_want;
    a.m = group_size;
    a.out_score = out_score;
    a.out_row = out_row;
    a.out_count = out_count;
    a.out_code = out_code;
    a.out_complete = out_complete;
    a.out_found = out_found;
    a.out_short = out_short;
    a.out_bad = out_bad;
    HIP_TRY(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    // four positions per thread: the narrowest workgroup that covers the list
    if (k <= 1024) hipLaunchKernelGGL(k_group_select<256>, dim3((unsigned)nq), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_group_select<1024>, dim3((unsigned)nq), dim3(1024), 0, st, a);
    HIP_TRY(hipGetLastError());
    return RDX_OK;
}
