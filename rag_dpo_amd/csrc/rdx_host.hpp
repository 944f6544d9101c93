// rdx_host.hpp — what the host units of librdx (rdx_index.hip, rdx_derived.hip, rdx_merge.hip, rdx_enc.hip, rdx_bm25.hip, rdx_docs.hip,
// rdx_meta.hip, rdx_maxsim.hip) share: the error string behind rdx_last_error(), the checks of `space`, `device` and a call's shape arrays,
// the device / pinned buffers, the copy of a host caller's results, the dynamic-LDS limit of a kernel, and the wait on a word in pinned
// memory. It holds no kernel (the rule: rdx_index.hpp "ONE DEFINITION"). What only the row-filter stores share (rdx_docs.hip, rdx_meta.hip) is in rdx_store.hpp.
#pragma once
#include "../../include/rdx.h"
#include "rdx_limits.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <sched.h>

#include <immintrin.h>

// one definition for the whole library (inline), invisible outside it (hidden)
#define RDX_HOST_SHARED inline __attribute__((visibility("hidden")))

// ------------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------------
RDX_HOST_SHARED thread_local std::string g_err;

RDX_HOST_SHARED int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) {                                                                    \
            const int _code = (_e == hipErrorOutOfMemory) ? RDX_ERR_NOMEM : RDX_ERR_HIP;           \
            return fail(_code, std::string(#expr) + ": " + hipGetErrorString(_e));                \
        }                                                                                          \
    } while (0)

#define RDX_TRY(expr)              \
    do {                           \
        int _r = (expr);           \
        if (_r != RDX_OK) return _r; \
    } while (0)

// the `space` argument of every entry point whose pointers may live on either side
RDX_HOST_SHARED int check_space(int space) {
    if (space != RDX_HOST && space != RDX_DEVICE) return fail(RDX_ERR_INVALID, "space must be RDX_HOST or RDX_DEVICE");
    return RDX_OK;
}

// the `device` argument of a *_create; prefix = "" or "rdx_x_create: "
RDX_HOST_SHARED int check_device(const char* prefix, int device) {
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev)
        return fail(RDX_ERR_INVALID, std::string(prefix) + "device " + std::to_string(device) + " out of range (" + std::to_string(ndev) + " visible)");
    return RDX_OK;
}

// the `device` argument of an entry point that keeps state per device (tables of rdx::MAX_DEVICES entries); who = the entry point
RDX_HOST_SHARED int check_device_index(const char* who, int device) {
    if (device < 0 || device >= rdx::MAX_DEVICES) return fail(RDX_ERR_INVALID, std::string(who) + ": device out of range");
    return RDX_OK;
}

// A shape array of a batched call (rdx_enc.hip's reranker batch, rdx_maxsim.hip) is read by the library, to check the call and size
// its grids, and by the kernels: it has to lie in pinned host memory (hipHostMalloc / hipHostRegister), which both sides address.
// -> *dev = the address the kernels use. Anything else (device memory, pageable host memory) is refused: nothing is copied and
// nothing waited for.
RDX_HOST_SHARED int shape_array(const char* fn, const char* name, const void* p, size_t align, const void** dev) {
    if (!p) return fail(RDX_ERR_INVALID, std::string(fn) + ": null pointer (" + name + ")");
    if ((uintptr_t)p & (align - 1)) return fail(RDX_ERR_INVALID, std::string(fn) + ": misaligned pointer (" + name + ")");
    hipPointerAttribute_t attr;
    hipError_t e = hipPointerGetAttributes(&attr, p);
    if (e != hipSuccess || attr.type != hipMemoryTypeHost) {
        (void)hipGetLastError();
        return fail(RDX_ERR_INVALID, std::string(fn) + ": " + name + " must lie in pinned host memory (the library reads it to check the "
                                     "call and size the launch, the kernels read the same words)");
    }
    void* d = nullptr;
    e = hipHostGetDevicePointer(&d, const_cast<void*>(p), 0);
    if (e != hipSuccess || !d) {
        (void)hipGetLastError();
        return fail(RDX_ERR_INVALID, std::string(fn) + ": " + name + " is pinned host memory that is not mapped to the device");
    }
    *dev = d;
    return RDX_OK;
}

// owning device buffer: grow-only scratch (ensure), or an allocation of exactly the size asked for (alloc) that a caller fills
// and then moves into place
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    hipError_t alloc(size_t need) {   // what it held is freed first
        release();
        const hipError_t e = hipMalloc(&p, need);
        if (e != hipSuccess) p = nullptr;
        else bytes = need;
        return e;
    }
    int ensure(size_t need) {
        if (need <= bytes) return RDX_OK;
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
        size_t want = need + need / 4;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) {
            want = need;
            e = hipMalloc(&p, want);
        }
        if (e != hipSuccess) {
            p = nullptr;
            return fail(RDX_ERR_NOMEM, std::string("hipMalloc(") + std::to_string(need) + "): " + hipGetErrorString(e));
        }
        bytes = want;
        return RDX_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    template <class T>
    T* as() const { return reinterpret_cast<T*>(p); }
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr, o.bytes = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {   // (o takes what this held, and frees it when it goes)
        std::swap(p, o.p);
        std::swap(bytes, o.bytes);
        return *this;
    }
    ~DevBuf() { release(); }   // error paths that return early do not leak scratch
};

struct PinnedBuf {   // grow-only pinned host staging
    void* p = nullptr;
    size_t bytes = 0;
    int ensure(size_t need) {
        if (need <= bytes) return RDX_OK;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        bytes = 0;
        const size_t want = std::max(need + need / 4, (size_t)4096);
        hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
        if (e != hipSuccess) {
            p = nullptr;
            return fail(RDX_ERR_NOMEM, std::string("hipHostMalloc(") + std::to_string(want) + "): " + hipGetErrorString(e));
        }
        bytes = want;
        return RDX_OK;
    }
    ~PinnedBuf() {
        if (p) (void)hipHostFree(p);
    }
};

// grow a device buffer to `need` bytes, keeping its first `keep` (geometric: appends in small batches stay linear)
RDX_HOST_SHARED int grow_keep(DevBuf& b, size_t keep, size_t need, const char* what) {
    if (need <= b.bytes) return RDX_OK;
    size_t want = std::max(need, b.bytes + b.bytes / 2);
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess && want > need) e = hipMalloc(&p, want = need);
    if (e != hipSuccess) return fail(RDX_ERR_NOMEM, std::string("growing the ") + what + " to " + std::to_string(need) + " bytes: " + hipGetErrorString(e));
    if (keep > 0) e = hipMemcpy(p, b.p, keep, hipMemcpyDeviceToDevice);
    if (e != hipSuccess) {
        (void)hipFree(p);
        return fail(RDX_ERR_HIP, std::string("growing the ") + what + ": " + hipGetErrorString(e));
    }
    b.release();
    b.p = p;
    b.bytes = want;
    return RDX_OK;
}

// zeroed pinned host memory the device reaches over PCIe: its host address and the device's address of the same bytes
template <class T>
struct MappedPin {
    T* host = nullptr;
    T* dev = nullptr;
    int map(size_t bytes) {
        void* p = nullptr;
        HIP_TRY(hipHostMalloc(&p, bytes, hipHostMallocMapped | hipHostMallocCoherent));
        std::memset(p, 0, bytes);
        void* d = nullptr;
        hipError_t e = hipHostGetDevicePointer(&d, p, 0);
        if (e != hipSuccess) {
            (void)hipHostFree(p);
            return fail(RDX_ERR_HIP, std::string("hipHostGetDevicePointer: ") + hipGetErrorString(e));
        }
        host = static_cast<T*>(p);
        dev = static_cast<T*>(d);
        return RDX_OK;
    }
    MappedPin() = default;
    MappedPin(const MappedPin&) = delete;
    MappedPin& operator=(const MappedPin&) = delete;
    ~MappedPin() {
        if (host) (void)hipHostFree(host);
    }
};

// Host callers: where the results go (rdx_index.hip search_chunk, rdx_merge.hip)
struct HostOut {
    float* score;
    int64_t* row;
    int32_t* count;
    bool stale;
};

// Host callers (HostOut): small results travel with the end-of-search kernel into pinned staging and are copied to the
// caller's buffers by the CPU once the mailbox says the search is complete; large ones use D2H copies. When a fallback pass
// had to rewrite some results afterwards they are copied again (HostOut::stale). (PIN_MAX: search_plan.hpp)
RDX_HOST_SHARED int copy_results_to_host(const HostOut& ho, const float* d_score, const int64_t* d_row, const int32_t* d_count, int64_t nq,
                                         int k, hipStream_t st) {
    if (k > 0) {
        HIP_TRY(hipMemcpyAsync(ho.score, d_score, (size_t)nq * k * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(ho.row, d_row, (size_t)nq * k * 8, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipMemcpyAsync(ho.count, d_count, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
    return RDX_OK;
}

// Kernels that use more than 64 KiB of dynamic LDS need the limit raised, once per kernel and device and again when the need
// grows. The limits already raised on a device are a table that is replaced, never changed: a launch reads the current one
// without a lock (one lookup); whoever has to raise a limit takes the lock, sets the kernel's attribute and publishes a copy. (The
// tables it replaces are left standing for their readers: a handful per kernel in the life of a process.)
using LdsLimits = std::unordered_map<const void*, size_t>;
RDX_HOST_SHARED std::atomic<const LdsLimits*> g_lds_limits[rdx::MAX_DEVICES];
RDX_HOST_SHARED std::mutex g_lds_limits_mu;

RDX_HOST_SHARED int dynamic_lds(int device, const void* func, size_t bytes) {
    if (bytes <= 65536) return RDX_OK;
    RDX_TRY(check_device_index("dynamic_lds", device));
    const auto raised = [&](const LdsLimits* t) {
        if (!t) return false;
        const auto it = t->find(func);
        return it != t->end() && it->second >= bytes;
    };
    if (raised(g_lds_limits[device].load(std::memory_order_acquire))) return RDX_OK;
    std::lock_guard<std::mutex> lk(g_lds_limits_mu);
    const LdsLimits* cur = g_lds_limits[device].load(std::memory_order_acquire);
    if (raised(cur)) return RDX_OK;
    HIP_TRY(hipFuncSetAttribute(func, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    LdsLimits* next = cur ? new LdsLimits(*cur) : new LdsLimits();
    (*next)[func] = bytes;
    g_lds_limits[device].store(next, std::memory_order_release);
    return RDX_OK;
}

// Waits until ready() says a word in pinned host memory has arrived — never for the stream: an asynchronous caller may have enqueued
// other work behind the search or merge that publishes the word (BASELINE config 5: the next batch's query encode, 15 ms of kernels),
// and a stream synchronise would wait for that too. Hot spin for 0.4 ms (a small search ends inside it), then poll with a yield
// between looks (a 0.6 - 25 ms search is noticed within a microsecond; measured with 20 us sleeps instead: +30 us on a 0.56 ms search,
// +170 us on a 2.2 ms one), after 200 ms with 50 us sleeps. The stream is only QUERIED, every 50 ms, to turn a failed or vanished
// launch into an error instead of an endless wait. 0 = arrived, 1 = the stream ran dry without the word, < 0 = error code.
// Wait policy (rdx_set_wait_policy; environment RDX_WAIT_SPIN_US / RDX_WAIT_SLEEP_US at load): the default burns a host core for the
// length of a search — right for a benchmark or one rank per GPU, wrong for a server whose sessions share the cores (the reference
// serves concurrent Streamlit sessions from one process, app.py:42-43). sleep_us > 0: after the hot spin the waiter SLEEPS that long
// between looks (a 15 ms scan then costs the core ~1 % instead of 100 %; the result is noticed up to sleep_us later).
RDX_HOST_SHARED std::atomic<int> g_wait_spin_us{[] {
    const char* e = std::getenv("RDX_WAIT_SPIN_US");
    return e ? std::atoi(e) : 400;
}()};
RDX_HOST_SHARED std::atomic<int> g_wait_sleep_us{[] {
    const char* e = std::getenv("RDX_WAIT_SLEEP_US");
    return e ? std::max(0, std::atoi(e)) : 0;
}()};
template <class F>
RDX_HOST_SHARED int wait_word(F ready, hipStream_t st) {
    const auto t0 = std::chrono::steady_clock::now();
    const int spin_us = g_wait_spin_us.load(std::memory_order_relaxed), sleep_us = g_wait_sleep_us.load(std::memory_order_relaxed);
    for (unsigned spins = 1;; ++spins) {
        if (ready()) return 0;
        if (spin_us == 0) break;
        _mm_pause();
        if ((spins & 255u) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(spin_us)) break;
    }
    auto next_query = t0 + std::chrono::milliseconds(50);
    const auto t_sleep = t0 + std::chrono::milliseconds(200);
    for (unsigned n = 1;; ++n) {
        if (ready()) return 0;
        if (sleep_us > 0) {
            std::this_thread::sleep_for(std::chrono::microseconds(sleep_us));
            if (ready()) return 0;
        } else if ((n & 15u) != 0) {
            sched_yield();
            continue;
        }
        const auto now = std::chrono::steady_clock::now();
        if (sleep_us == 0 && now >= t_sleep) std::this_thread::sleep_for(std::chrono::microseconds(50));
        if (now >= next_query) {
            const hipError_t e = hipStreamQuery(st);
            if (e == hipSuccess) return ready() ? 0 : 1;   // everything enqueued has run: the word must be there
            if (e != hipErrorNotReady) return fail(RDX_ERR_HIP, std::string("hipStreamQuery: ") + hipGetErrorString(e));
            next_query = now + std::chrono::milliseconds(50);
        }
    }
}
