// lex_kernel.hpp — the term reduction of BGE-M3's lexical weights (gfx950): a text's (token id, weight) pairs to its terms, one entry
// per distinct id carrying the largest weight, ascending by id. The rule is rag_dpo_amd/lexical.py's `terms_model`, bit for bit
// (DESIGN.md §30):
//   the fp32 weight is rounded once to fp16 (v_cvt_f16_f32, round to nearest even, fp16 denormals kept); a token is dropped when the fp16
//   value is not finite and above 0 (bits outside [0x0001, 0x7BFF]) or when its id is one of the skip ids; an id outside [0, vocab)
//   makes the whole text an error (out_n = -1, nothing written).
//
// Method. One workgroup per text. Every token becomes a 64-bit key (id << 16) | fp16 bits — the bits of positive fp16 values order as
// the values do — or the all-ones sentinel when it is dropped; the keys are sorted ascending by a bitonic network in LDS (8 B per token:
// 64 KiB at the 8 192-token cap), so the last key of a run of equal ids holds the run's maximum; one block scan per LEX_THREADS keys
// compacts those to out_*[off[i] ..). Integer compares only: no float atomics, no dependence on the order of a text's tokens or of the
// texts in the call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rdx {

constexpr int LEX_MAX_TOKENS = 8192;   // per text (the encoder's cap)
constexpr int LEX_MAX_SKIP = 8;
constexpr int LEX_THREADS_SMALL = 256, LEX_THREADS = 1024;   // by the call's longest text: up to 1024 tokens / more
constexpr int LEX_SCRATCH_WORDS = 32;  // ints behind the keys: per-wave scan totals [16], the running output count, the error flag

struct LexSkip {
    int32_t n;
    int32_t id[LEX_MAX_SKIP];
};

__host__ __device__ inline int lex_pow2_at_least(int n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

// dynamic LDS of a launch whose longest text has `longest` tokens
__host__ __device__ inline size_t lex_lds_bytes(int longest) {
    return (size_t)lex_pow2_at_least(longest < 1 ? 1 : longest) * 8 + LEX_SCRATCH_WORDS * 4;
}

// Grid: one block per text, blockDim.x a multiple of 64 up to LEX_THREADS; dynamic LDS lex_lds_bytes(the longest text of the call), of
// which the keys take `key_cap` entries. off is read as the host checked it; a text whose range does not lie in [0, n_tok) with 0 to
// min(LEX_MAX_TOKENS, key_cap) tokens is treated like one with a bad id: out_n = -1, nothing written.
__global__ __launch_bounds__(LEX_THREADS) void k_lex_reduce(const int32_t* __restrict__ tok, const float* __restrict__ w,
                                                            const int64_t* __restrict__ off, int64_t n_tok, int vocab, LexSkip skip,
                                                            int key_cap, int32_t* __restrict__ out_tok, uint16_t* __restrict__ out_w,
                                                            int32_t* __restrict__ out_n) {
    extern __shared__ uint64_t lex_keys[];
    int* scratch = reinterpret_cast<int*>(lex_keys + key_cap);
    int* s_wave = scratch;            // [16]
    int* s_base = scratch + 16;       // terms written so far
    int* s_bad = scratch + 17;
    constexpr uint64_t DROPPED = ~(uint64_t)0;

    const int text = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int lane = tid & 63, wave = tid >> 6, n_waves = nt >> 6;
    const int64_t b = off[text], e = off[text + 1];
    const bool range_ok = b >= 0 && e >= b && e <= n_tok && e - b <= LEX_MAX_TOKENS && e - b <= key_cap;
    const int len = range_ok ? (int)(e - b) : 0;
    if (tid == 0) {
        *s_bad = range_ok ? 0 : 1;
        *s_base = 0;
    }
    __syncthreads();
    const int n = lex_pow2_at_least(len);   // <= key_cap: key_cap is a power of two
    for (int j = tid; j < n; j += nt) {
        uint64_t key = DROPPED;
        if (j < len) {
            const int32_t id = tok[b + j];
            if (id < 0 || id >= vocab) *s_bad = 1;
            const _Float16 h = (_Float16)w[b + j];
            const uint16_t bits = __builtin_bit_cast(uint16_t, h);
            bool keep = bits >= 1 && bits <= 0x7BFF;
            for (int s = 0; s < skip.n; ++s) keep = keep && id != skip.id[s];
            if (keep) key = ((uint64_t)(uint32_t)id << 16) | bits;
        }
        lex_keys[j] = key;
    }
    __syncthreads();
    if (*s_bad) {   // uniform: every thread reads the flag behind the barrier
        if (tid == 0) out_n[text] = -1;
        return;
    }
    // bitonic sort, ascending
    for (int size = 2; size <= n; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = tid; i < (n >> 1); i += nt) {
                const int lo = 2 * i - (i & (stride - 1));
                const int hi = lo + stride;
                const uint64_t x = lex_keys[lo], y = lex_keys[hi];
                if (((lo & size) == 0) == (x > y)) {
                    lex_keys[lo] = y;
                    lex_keys[hi] = x;
                }
            }
            __syncthreads();
        }
    }
    // compaction: the last key of every run of one id, nt keys per round
    for (int j0 = 0; j0 < n; j0 += nt) {
        const int j = j0 + tid;
        uint64_t key = DROPPED;
        int last = 0;
        if (j < n) {
            key = lex_keys[j];
            last = key != DROPPED && (j + 1 == n || (lex_keys[j + 1] >> 16) != (key >> 16));
        }
        int x = last;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int y = __shfl_up(x, d, 64);
            if (lane >= d) x += y;
        }
        if (lane == 63) s_wave[wave] = x;
        __syncthreads();
        int before = *s_base, all = 0;
        for (int v = 0; v < n_waves; ++v) {
            const int s = s_wave[v];
            before += v < wave ? s : 0;
            all += s;
        }
        if (last) {   // position < len: at most one term per token
            const int pos = before + x - 1;
            out_tok[b + pos] = (int32_t)(key >> 16);
            out_w[b + pos] = (uint16_t)(key & 0xFFFF);
        }
        __syncthreads();   // everyone has read s_base and s_wave
        if (tid == 0) *s_base += all;
        __syncthreads();
    }
    if (tid == 0) out_n[text] = *s_base;
}

}  // namespace rdx
