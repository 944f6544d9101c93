// rdx_fuse.hip — the launcher of rdx_fuse_rankings (include/rdx.h): fuse_kernel.hpp's kernel behind argument checks that run before
// the device is touched. RDX_DEVICE: one launch on the caller's stream, nothing allocated or synchronised. RDX_HOST: the inputs are
// staged through device memory of the call's own and the results are on the host on return.
#include "rdx_host.hpp"

#include "fuse_kernel.hpp"

using namespace rdx;

static_assert(FUSE_MAX_LISTS == RDX_FUSE_MAX_LISTS && FUSE_MAX_LIST_ENTRIES == RDX_FUSE_MAX_LIST_ENTRIES &&
                  FUSE_MAX_ENTRIES == RDX_FUSE_MAX_ENTRIES && FUSE_DENSE == RDX_FUSE_DENSE && FUSE_BM25 == RDX_FUSE_BM25,
              "fuse_kernel.hpp and include/rdx.h disagree");

namespace {

// one staged array of a RDX_HOST call
struct Staged {
    DevBuf buf;
    int up(const void* host, size_t bytes, hipStream_t st) {
        RDX_TRY(buf.ensure(std::max(bytes, (size_t)16)));
        if (bytes) HIP_TRY(hipMemcpyAsync(buf.p, host, bytes, hipMemcpyHostToDevice, st));
        return RDX_OK;
    }
    int room(size_t bytes) { return buf.ensure(std::max(bytes, (size_t)16)); }
    int down(void* host, size_t bytes, hipStream_t st) {
        if (bytes) HIP_TRY(hipMemcpyAsync(host, buf.p, bytes, hipMemcpyDeviceToHost, st));
        return RDX_OK;
    }
};

int fuse_host(int device, int64_t nq, FuseArgs a, hipStream_t st) {
    const size_t nl = (size_t)nq * a.n_lists, ne = nl * a.list_stride, no = (size_t)nq * a.top_n;
    // counts and kinds are readable here: hold them to the header's words before anything is staged
    for (size_t i = 0; i < nl; ++i) {
        if (a.list_count[i] < -1 || a.list_count[i] > a.list_stride)
            return fail(RDX_ERR_INVALID, "rdx_fuse_rankings: a list's count must be -1 (absent) or in [0, list_stride]");
        if (a.list_kind[i] != FUSE_DENSE && a.list_kind[i] != FUSE_BM25)
            return fail(RDX_ERR_INVALID, "rdx_fuse_rankings: a list's kind must be RDX_FUSE_DENSE or RDX_FUSE_BM25");
    }
    HIP_TRY(hipSetDevice(device));
    Staged kind, weight, count, keys, dist, score, group, fon, allow, o_key, o_dist, o_sem, o_bm, o_hyb, o_list, o_rank, o_count;
    RDX_TRY(kind.up(a.list_kind, nl * 4, st));
    RDX_TRY(weight.up(a.list_weight, nl * 8, st));
    RDX_TRY(count.up(a.list_count, nl * 4, st));
    RDX_TRY(keys.up(a.keys, ne * 8, st));
    RDX_TRY(dist.up(a.dense_dist, ne * 4, st));
    RDX_TRY(score.up(a.bm25_score, ne * 8, st));
    if (a.filter_on) {
        RDX_TRY(group.up(a.row_group, (size_t)a.n_rows * 4, st));
        RDX_TRY(fon.up(a.filter_on, (size_t)nq * 4, st));
        RDX_TRY(allow.up(a.allow_groups, (size_t)nq * a.group_words * 4, st));
    }
    RDX_TRY(o_key.room(no * 8));
    RDX_TRY(o_dist.room(no * 4));
    RDX_TRY(o_sem.room(no * 8));
    RDX_TRY(o_bm.room(no * 8));
    RDX_TRY(o_hyb.room(no * 8));
    RDX_TRY(o_list.room(no * 4));
    RDX_TRY(o_rank.room(no * 4));
    RDX_TRY(o_count.room((size_t)nq * 4));
    FuseArgs d = a;
    d.list_kind = kind.buf.as<int32_t>();
    d.list_weight = weight.buf.as<double>();
    d.list_count = count.buf.as<int32_t>();
    d.keys = keys.buf.as<int64_t>();
    d.dense_dist = dist.buf.as<float>();
    d.bm25_score = score.buf.as<double>();
    d.row_group = a.filter_on ? group.buf.as<int32_t>() : nullptr;
    d.filter_on = a.filter_on ? fon.buf.as<int32_t>() : nullptr;
    d.allow_groups = a.filter_on ? allow.buf.as<uint32_t>() : nullptr;
    d.out_key = o_key.buf.as<int64_t>();
    d.out_distance = o_dist.buf.as<float>();
    d.out_semantic = o_sem.buf.as<double>();
    d.out_bm25 = o_bm.buf.as<double>();
    d.out_hybrid = o_hyb.buf.as<double>();
    d.out_list = o_list.buf.as<int32_t>();
    d.out_rank = o_rank.buf.as<int32_t>();
    d.out_count = o_count.buf.as<int32_t>();
    hipLaunchKernelGGL(k_fuse_rankings, dim3((unsigned)nq), dim3(FUSE_THREADS), 0, st, d);
    HIP_TRY(hipGetLastError());
    RDX_TRY(o_key.down(a.out_key, no * 8, st));
    RDX_TRY(o_dist.down(a.out_distance, no * 4, st));
    RDX_TRY(o_sem.down(a.out_semantic, no * 8, st));
    RDX_TRY(o_bm.down(a.out_bm25, no * 8, st));
    RDX_TRY(o_hyb.down(a.out_hybrid, no * 8, st));
    RDX_TRY(o_list.down(a.out_list, no * 4, st));
    RDX_TRY(o_rank.down(a.out_rank, no * 4, st));
    RDX_TRY(o_count.down(a.out_count, (size_t)nq * 4, st));
    HIP_TRY(hipStreamSynchronize(st));       // (the staging buffers are freed behind this)
    return RDX_OK;
}

}  // namespace

extern "C" int rdx_fuse_rankings(int device, int64_t nq, int n_lists, int list_stride, const int32_t* list_kind,
                                 const double* list_weight, const int32_t* list_count, const int64_t* keys, const float* dense_dist,
                                 const double* bm25_score, const int32_t* row_group, int64_t n_rows, const int32_t* filter_on,
                                 const uint32_t* allow_groups, int group_words, int min_semantic, int bm25_keep_max, int rrf_k,
                                 int top_n, int64_t* out_key, float* out_distance, double* out_semantic, double* out_bm25,
                                 double* out_hybrid, int32_t* out_list, int32_t* out_rank, int32_t* out_count, int space,
                                 void* stream) {
    RDX_TRY(check_space(space));
    RDX_TRY(check_device_index("rdx_fuse_rankings", device));
    if (nq < 0 || nq > (int64_t)1 << 24) return fail(RDX_ERR_INVALID, "rdx_fuse_rankings: nq must be in [0, 2^24]");
    if (n_lists < 1 || n_lists > FUSE_MAX_LISTS) return fail(RDX_ERR_INVALID, "rdx_fuse_rankings: n_lists must be in [1, 16]");
    if (list_stride < 1 || list_stride > FUSE_MAX_LIST_ENTRIES)
        return fail(RDX_ERR_INVALID, "rdx_fuse_rankings: list_stride (the entries per list) must be in [1, 512]");
    if (n_lists * list_stride > FUSE_MAX_ENTRIES)
        return fail(RDX_ERR_INVALID, "rdx_fuse_rankings: n_lists * list_stride (the entries per question) must be at most 1024");
    if (top_n < 1 || top_n > FUSE_MAX_ENTRIES) return fail(RDX_ERR_INVALID, "rdx_fuse_rankings: top_n must be in [1, 1024]");
    if (min_semantic < 0 || min_semantic > FUSE_MAX_ENTRIES) return fail(RDX_ERR_INVALID, "rdx_fuse_rankings: min_semantic must be in [0, 1024]");
    if (bm25_keep_max != 0 && bm25_keep_max != 1) return fail(RDX_ERR_INVALID, "rdx_fuse_rankings: bm25_keep_max must be 0 or 1");
    if (rrf_k < 0 || rrf_k > 1 << 20) return fail(RDX_ERR_INVALID, "rdx_fuse_rankings: the RRF constant must be in [0, 2^20]");
    if (n_rows < 0 || group_words < 0 || group_words > 1 << 20)
        return fail(RDX_ERR_INVALID, "rdx_fuse_rankings: n_rows must be >= 0 and group_words in [0, 2^20]");
    if (nq == 0) return RDX_OK;
    if (!list_kind || !list_weight || !list_count || !keys || !dense_dist || !bm25_score)
        return fail(RDX_ERR_INVALID, "rdx_fuse_rankings: null input pointer");
    if (!out_key || !out_distance || !out_semantic || !out_bm25 || !out_hybrid || !out_list || !out_rank || !out_count)
        return fail(RDX_ERR_INVALID, "rdx_fuse_rankings: null output pointer");
    if (filter_on && (!allow_groups || group_words < 1 || (n_rows > 0 && !row_group)))
        return fail(RDX_ERR_INVALID, "rdx_fuse_rankings: filter_on needs allow_groups, group_words >= 1 and row_group");
    if (((uintptr_t)list_weight | (uintptr_t)keys | (uintptr_t)bm25_score | (uintptr_t)out_key | (uintptr_t)out_semantic | (uintptr_t)out_bm25 |
         (uintptr_t)out_hybrid) & 7)
        return fail(RDX_ERR_INVALID, "rdx_fuse_rankings: misaligned pointer");
    if (((uintptr_t)list_kind | (uintptr_t)list_count | (uintptr_t)dense_dist | (uintptr_t)row_group | (uintptr_t)filter_on | (uintptr_t)allow_groups |
         (uintptr_t)out_distance | (uintptr_t)out_list | (uintptr_t)out_rank | (uintptr_t)out_count) & 3)
        return fail(RDX_ERR_INVALID, "rdx_fuse_rankings: misaligned pointer");
    FuseArgs a;
    a.n_lists = n_lists;
    a.list_stride = list_stride;
    a.list_kind = list_kind;
    a.list_weight = list_weight;
    a.list_count = list_count;
    a.keys = keys;
    a.dense_dist = dense_dist;
    a.bm25_score = bm25_score;
    a.row_group = row_group;
    a.n_rows = row_group ? n_rows : 0;
    a.filter_on = filter_on;
    a.allow_groups = allow_groups;
    a.group_words = group_words;
    a.min_semantic = min_semantic;
    a.bm25_keep_max = bm25_keep_max;
    a.rrf_k = rrf_k;
    a.top_n = top_n;
    a.out_key = out_key;
    a.out_distance = out_distance;
    a.out_semantic = out_semantic;
    a.out_bm25 = out_bm25;
    a.out_hybrid = out_hybrid;
    a.out_list = out_list;
    a.out_rank = out_rank;
    a.out_count = out_count;
    if (space == RDX_HOST) return fuse_host(device, nq, a, (hipStream_t)stream);
    HIP_TRY(hipSetDevice(device));
    hipLaunchKernelGGL(k_fuse_rankings, dim3((unsigned)nq), dim3(FUSE_THREADS), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return RDX_OK;
}
