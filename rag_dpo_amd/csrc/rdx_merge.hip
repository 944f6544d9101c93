// rdx_merge.hip — C1 of include/rdx.h: the merge of per-shard partial top-k lists (rdx_merge_topk, rdx_merge_topk_packed) and the
// signal a packed merge publishes to the host (rdx_signal_*). No rdx_index is involved: the unit works against rdx_host.hpp and
// merge_kernel.hpp only.
#include "rdx_host.hpp"

#include <memory>

#include "merge_kernel.hpp"

using namespace rdx;

// a pinned, device-visible word the merge kernel publishes ((sequence << 1) | value) and the host waits on
struct rdx_signal {
    int device = 0;
    MappedPin<unsigned long long> word;
    unsigned long long seq = 0;   // number of the last merge that was given this signal
};

extern "C" int rdx_merge_topk(int device, const float* part_score, const int64_t* part_row, const int32_t* part_count, int n_parts,
                              int64_t nq, int k, float* out_score, int64_t* out_row, int32_t* out_count, int space, void* stream) {
    if (n_parts < 1 || n_parts > 64 || nq < 0 || k < 0 || k > SELECT_MAX_K) return fail(RDX_ERR_INVALID, "rdx_merge_topk: bad shape");
    RDX_TRY(check_space(space));
    if (nq == 0) return RDX_OK;
    if (!part_count || !out_count || (k > 0 && (!part_score || !part_row || !out_score || !out_row)))
        return fail(RDX_ERR_INVALID, "rdx_merge_topk: null pointer");
    HIP_TRY(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    const size_t np = (size_t)n_parts * nq;
    const int kk = std::max(k, 1);
    DevBuf ps, pr, pc, os, orow, oc;
    const float* d_ps = part_score;
    const int64_t* d_pr = part_row;
    const int32_t* d_pc = part_count;
    float* d_os = out_score;
    int64_t* d_or = out_row;
    int32_t* d_oc = out_count;
    if (space == RDX_HOST) {
        RDX_TRY(ps.ensure(np * kk * 4));
        RDX_TRY(pr.ensure(np * kk * 8));
        RDX_TRY(pc.ensure(np * 4));
        RDX_TRY(os.ensure((size_t)nq * kk * 4));
        RDX_TRY(orow.ensure((size_t)nq * kk * 8));
        RDX_TRY(oc.ensure((size_t)nq * 4));
        if (k > 0) {
            HIP_TRY(hipMemcpyAsync(ps.p, part_score, np * k * 4, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(pr.p, part_row, np * k * 8, hipMemcpyHostToDevice, st));
        }
        HIP_TRY(hipMemcpyAsync(pc.p, part_count, np * 4, hipMemcpyHostToDevice, st));
        d_ps = ps.as<float>();
        d_pr = pr.as<int64_t>();
        d_pc = pc.as<int32_t>();
        d_os = os.as<float>();
        d_or = orow.as<int64_t>();
        d_oc = oc.as<int32_t>();
    }
    DevBuf t_s[2], t_r[2], t_c[2];   // the fold's intermediate lists (large k only)
    if ((int64_t)n_parts * k <= MERGE_MAX) {
        hipLaunchKernelGGL(k_merge, dim3((int)nq), dim3(256), 0, st, d_ps, d_pr, d_pc, (int64_t)nq * k, (int64_t)nq * k, (int64_t)nq, n_parts, nq, k,
                           d_os, d_or, d_oc);
        HIP_TRY(hipGetLastError());
    } else {
        // more candidates per query than k_merge ranks in LDS (several shards at k > 2048 / n_parts): fold the parts pairwise
        const size_t nk = (size_t)nq * k;
        for (int j = 0; j < 2 && n_parts > 2; ++j) {
            RDX_TRY(t_s[j].ensure(nk * 4));
            RDX_TRY(t_r[j].ensure(nk * 8));
            RDX_TRY(t_c[j].ensure((size_t)nq * 4));
        }
        const float* a_s = d_ps;
        const int64_t* a_r = d_pr;
        const int32_t* a_c = d_pc;
        for (int p = 1; p < n_parts; ++p) {
            const bool last = p == n_parts - 1;
            float* o_s = last ? d_os : t_s[p & 1].as<float>();
            int64_t* o_r = last ? d_or : t_r[p & 1].as<int64_t>();
            int32_t* o_c = last ? d_oc : t_c[p & 1].as<int32_t>();
            hipLaunchKernelGGL(k_merge_pair, dim3((int)nq), dim3(256), 0, st, a_s, a_r, a_c, d_ps + (size_t)p * nk, d_pr + (size_t)p * nk,
                               d_pc + (size_t)p * nq, k, o_s, o_r, o_c);
            HIP_TRY(hipGetLastError());
            a_s = o_s;
            a_r = o_r;
            a_c = o_c;
        }
        if (space == RDX_DEVICE && n_parts > 2) HIP_TRY(hipStreamSynchronize(st));   // the intermediates are freed on return
    }
    if (space == RDX_HOST) {
        RDX_TRY(copy_results_to_host(HostOut{out_score, out_row, out_count, false}, d_os, d_or, d_oc, nq, k, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (DevBuf* b : {&ps, &pr, &pc, &os, &orow, &oc}) b->release();
    }
    return RDX_OK;
}

extern "C" int rdx_signal_create(int device, rdx_signal** out) {
    if (!out) return fail(RDX_ERR_INVALID, "rdx_signal_create: null out pointer");
    HIP_TRY(hipSetDevice(device));
    auto s = std::make_unique<rdx_signal>();
    s->device = device;
    RDX_TRY(s->word.map(64));
    *out = s.release();
    return RDX_OK;
}

extern "C" int rdx_signal_destroy(rdx_signal* s) {
    if (!s) return RDX_OK;
    (void)hipSetDevice(s->device);
    const std::unique_ptr<rdx_signal> owner(s);
    return RDX_OK;
}

extern "C" int rdx_signal_wait(rdx_signal* s, void* stream, int32_t* value) {
    if (!s || !value) return fail(RDX_ERR_INVALID, "rdx_signal_wait: null pointer");
    if (s->seq == 0) return fail(RDX_ERR_STATE, "rdx_signal_wait: no merge has been given this signal");
    HIP_TRY(hipSetDevice(s->device));
    unsigned long long w = 0;
    const int rc = wait_word([&] { return ((w = __atomic_load_n(s->word.host, __ATOMIC_ACQUIRE)) >> 1) == s->seq; }, (hipStream_t)stream);
    if (rc == 1) return fail(RDX_ERR_HIP, "internal: the merge completed without publishing its signal");
    if (rc != 0) return rc;
    *value = (int32_t)(w & 1ull);
    return RDX_OK;
}

// the packed layout one rank contributes to the all-gather: rows i64[nq][k] | scores f32[nq][k] | counts i32[nq] | flags i32[4]
extern "C" int rdx_merge_topk_packed(int device, const void* packed, int64_t part_stride, int n_parts, int64_t nq, int k,
                                     float* out_score, int64_t* out_row, int32_t* out_count, rdx_signal* sig, void* stream) {
    if (n_parts < 1 || n_parts > 64 || nq < 0 || k < 1) return fail(RDX_ERR_INVALID, "rdx_merge_topk_packed: bad shape");
    if ((int64_t)n_parts * k > MERGE_MAX) return fail(RDX_ERR_INVALID, "rdx_merge_topk_packed: n_parts * k exceeds " + std::to_string(MERGE_MAX));
    const int64_t flags_off = nq * k * 12 + nq * 4;
    if (part_stride % 16 != 0 || part_stride < flags_off + 4 * RDX_PACKED_FLAGS)
        return fail(RDX_ERR_INVALID, "rdx_merge_topk_packed: part_stride must be a multiple of 16 covering one packed partial (rows | scores | counts | flags)");
    if (sig && sig->device != device) return fail(RDX_ERR_INVALID, "rdx_merge_topk_packed: the signal belongs to another device");
    if (nq == 0) {
        if (sig) return fail(RDX_ERR_INVALID, "rdx_merge_topk_packed: a signal needs nq >= 1");
        return RDX_OK;
    }
    if (!packed || !out_score || !out_row || !out_count) return fail(RDX_ERR_INVALID, "rdx_merge_topk_packed: null pointer");
    HIP_TRY(hipSetDevice(device));
    const char* b = reinterpret_cast<const char*>(packed);
    const unsigned long long seq = sig ? ++sig->seq : 0;
    hipLaunchKernelGGL(k_merge, dim3((int)nq), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const float*>(b + nq * k * 8),
                       reinterpret_cast<const int64_t*>(b), reinterpret_cast<const int32_t*>(b + nq * k * 12), part_stride / 4,
                       part_stride / 8, part_stride / 4, n_parts, nq, k, out_score, out_row, out_count,
                       reinterpret_cast<const int32_t*>(b + flags_off), part_stride / 4, sig ? sig->word.dev : (unsigned long long*)nullptr, seq);
    HIP_TRY(hipGetLastError());
    return RDX_OK;
}
