// rdx_store.hpp — the host code the row-filter stores share (rdx_docs.hip: where_document, rdx_meta.hip: `where`): the store's
// device, stream, "last use" event and lock; the one check of a postfix filter program; and the staging of a filter call's
// bitmaps, which may live on either side. Host code only: the kernels are in doc_kernel.hpp and meta_kernel.hpp.
#pragma once
#include "rdx_host.hpp"

#include <mutex>

#include "rdx_common.hpp"

static_assert(rdx::OP_NOT == RDX_DOCS_OP_NOT && rdx::OP_AND == RDX_DOCS_OP_AND && rdx::OP_OR == RDX_DOCS_OP_OR &&
                  rdx::OP_NOT == RDX_META_OP_NOT && rdx::OP_AND == RDX_META_OP_AND && rdx::OP_OR == RDX_META_OP_OR,
              "the program ops of include/rdx.h and the kernels' must agree");

// A store lives on one device; filters run on the caller's stream or, for host callers, on the store's own.
struct StoreBase {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipEvent_t last_use = nullptr;   // recorded behind the last kernel that read the store: writes and re-allocations wait for it
    std::mutex mu;

    int open(const char* who, int device) {   // who = "rdx_x_create"; on failure the caller destroys the store, which close()s what exists
        HIP_TRY(hipSetDevice(device));
        this->device = device;
        hipError_t e = hipStreamCreateWithFlags(&own_stream, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&last_use, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventRecord(last_use, own_stream);
        return e == hipSuccess ? RDX_OK : fail(RDX_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
    }
    void close() {
        (void)hipSetDevice(device);
        if (last_use) (void)hipEventSynchronize(last_use), (void)hipEventDestroy(last_use);
        if (own_stream) (void)hipStreamSynchronize(own_stream), (void)hipStreamDestroy(own_stream);
    }
    int wait() {   // until the last kernel that read the store has finished
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(hipEventSynchronize(last_use));
        return RDX_OK;
    }
    hipStream_t stream_for(int space, void* stream) const { return space == RDX_HOST ? own_stream : (hipStream_t)stream; }
    int finish(int space, hipStream_t st) {   // behind the last kernel of a call that read the store; a host caller's call is complete on return
        HIP_TRY(hipEventRecord(last_use, st));
        if (space == RDX_HOST) HIP_TRY(hipStreamSynchronize(st));
        return RDX_OK;
    }
};

// The one check between a caller's postfix program and the kernels, which index LDS by the stack depth (k_docs_eval) or shift a
// register by it (k_meta_filter) without looking: every op is a leaf < n_leaves or NOT / AND / OR, the stack never underflows,
// never holds more than FILTER_MAX_STACK entries, and a program (n_ops > 0) leaves exactly one. The caller has checked n_ops
// against its own range and FILTER_MAX_OPS. who = "rdx_x_set_query: ", count_name = what include/rdx.h calls the leaf count.
RDX_HOST_SHARED int check_program(const std::string& who, const char* count_name, const int32_t* program, int n_ops, int n_leaves) {
    int depth = 0;
    for (int i = 0; i < n_ops; ++i) {
        const int32_t op = program[i];
        if (op >= n_leaves || op < rdx::OP_OR)
            return fail(RDX_ERR_INVALID, who + "op " + std::to_string(i) + " is neither a leaf < " + count_name + " nor NOT / AND / OR");
        const int need = op >= 0 ? 0 : (op == rdx::OP_NOT ? 1 : 2);
        if (depth < need) return fail(RDX_ERR_INVALID, who + "op " + std::to_string(i) + " pops an empty stack");
        depth += op >= 0 ? 1 : (op == rdx::OP_NOT ? 0 : -1);
        if (depth > rdx::FILTER_MAX_STACK)
            return fail(RDX_ERR_INVALID, who + "the program needs more than " + std::to_string(rdx::FILTER_MAX_STACK) + " stack entries");
    }
    if (n_ops > 0 && depth != 1) return fail(RDX_ERR_INVALID, who + "the program must leave exactly one value");
    return RDX_OK;
}

// The bitmaps of a filter call, base_bits (may be null) in and out_bits out, `words` words each, in either space. begin() gives
// the stream and the device pointers base / out for the kernel: the caller's own for RDX_DEVICE; for RDX_HOST the store's tmp_in
// (base_bits uploaded) / tmp_out, kept at one word at least. end() copies out back for a host caller and finishes the call.
// words == 0 copies nothing.
struct BitmapStage {
    hipStream_t st = nullptr;
    const uint32_t* base = nullptr;
    uint32_t* out = nullptr;

    int begin(StoreBase& s, int space, void* stream, int64_t words, const uint32_t* base_bits, uint32_t* out_bits, DevBuf& tmp_in, DevBuf& tmp_out) {
        st = s.stream_for(space, stream), base = base_bits, out = out_bits;
        if (space != RDX_HOST) return RDX_OK;
        RDX_TRY(tmp_in.ensure((size_t)std::max<int64_t>(words, 1) * 4));
        RDX_TRY(tmp_out.ensure((size_t)std::max<int64_t>(words, 1) * 4));
        if (base_bits && words) HIP_TRY(hipMemcpyAsync(tmp_in.p, base_bits, (size_t)words * 4, hipMemcpyHostToDevice, st));
        base = base_bits ? tmp_in.as<uint32_t>() : nullptr;
        out = tmp_out.as<uint32_t>();
        return RDX_OK;
    }
    int end(StoreBase& s, int space, int64_t words, uint32_t* out_bits) {
        if (space == RDX_HOST && words) HIP_TRY(hipMemcpyAsync(out_bits, out, (size_t)words * 4, hipMemcpyDeviceToHost, st));
        return s.finish(space, st);
    }
};
