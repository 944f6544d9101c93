// doc_kernel.hpp — the device document store behind `where_document` ($contains / $not_contains, include/rdx.h rdx_docs_*).
//
// Arena layout (one per device store, owned by rdx_docs in rdx_docs.hip):
//   every row's UTF-8 text starts on a 16-byte boundary and is zero-padded to the next one; the per-row table is
//   (start int64, len int32); the arena ends with DOC_TAIL zero bytes. Rows without text have len 0 and no bytes.
//
// Substring scan (k_docs_contains): the work list is one (row, segment) unit per DOC_SEG start positions of a row, so a
// 200 KB document is ~200 units and a 1 KB chunk one or two: the units are alike in cost whatever the length mix, and the
// waves take them grid-stride. A wave stages its unit in LDS with one coalesced 16 B/lane load (64 lanes x 16 B = DOC_SEG)
// plus the overlap the pass's longest pattern needs (max_len - 1 bytes, never past the row's own padded end: a match never
// spans two rows and no load leaves the arena). Lane l then owns start positions 16 l .. 16 l + 15: each is tested against
// every leaf's first min(len, 4) bytes (a 32-bit window cut out of two dwords by a funnel shift), and a candidate is verified
// byte by byte out of LDS. A (unit, leaf) that has a hit costs one ballot and one atomicOr of the row's bit; OR is idempotent,
// so a match found by two units (overlap) gives the same bits, and the result does not depend on the schedule.
// Patterns longer than DOC_STAGE_MAX take k_docs_contains_long (same units, compared straight from global memory).
//
// Boolean tree (k_docs_eval): a postfix program over the leaf bitmaps, one thread per 32-row word, the stack in LDS.
#pragma once
#include "rdx_common.hpp"

namespace rdx {

constexpr int DOC_ALIGN = 16;
constexpr int DOC_TAIL = 64;                 // zero bytes behind the last row
constexpr int DOC_SEG = 1024;                // start positions per work unit = 64 lanes x 16 B
constexpr int DOC_STAGE_MAX = 256;           // longest pattern staged in LDS; longer ones take k_docs_contains_long
constexpr int DOC_LEAVES_PER_PASS = 32;      // leaves one pass of k_docs_contains tests
constexpr int DOC_THREADS = 256;
constexpr int DOC_WAVES = DOC_THREADS / 64;
constexpr int DOC_EXT_CHUNKS = DOC_STAGE_MAX / 16;              // overlap chunks behind a segment (bytes up to 1023 + 255)
constexpr int DOC_CHUNKS = DOC_SEG / 16 + DOC_EXT_CHUNKS;       // 80 x 16 B of LDS per wave
constexpr int DOC_EVAL_THREADS = 256;

// one leaf as the scan sees it: bytes pat[off, off + len); prefix / pmask = its first min(len, 4) bytes (little-endian)
struct DocLeaf {
    int64_t off;
    int32_t len;
    int32_t slot;      // which leaf bitmap the hits go to
    uint32_t prefix;
    uint32_t pmask;
};

// the wave's LDS writes are visible to its other lanes (the compiler may not move the reads above the writes)
__device__ __forceinline__ void doc_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// units[u] = (row, segment): start positions [seg * DOC_SEG, min(len, (seg + 1) * DOC_SEG)) of that row.
// ext_chunks in [1, DOC_EXT_CHUNKS]: 16-byte chunks staged behind the segment, >= ceil((1023 + max_len) / 16) - 64.
__global__ __launch_bounds__(DOC_THREADS) void k_docs_contains(const uint8_t* __restrict__ arena, const int64_t* __restrict__ row_start,
                                                               const int32_t* __restrict__ row_len, const int2* __restrict__ units,
                                                               int64_t n_units, const DocLeaf* __restrict__ leaves, int n_leaves,
                                                               const uint8_t* __restrict__ pat, int ext_chunks, uint32_t* __restrict__ bits,
                                                               int64_t words) {
    __shared__ __attribute__((aligned(16))) uint8_t s_pat[DOC_LEAVES_PER_PASS * DOC_STAGE_MAX];
    __shared__ __attribute__((aligned(16))) uint8_t s_doc[DOC_WAVES][DOC_CHUNKS * 16];
    __shared__ DocLeaf s_leaf[DOC_LEAVES_PER_PASS];
    for (int i = threadIdx.x; i < n_leaves * DOC_STAGE_MAX; i += DOC_THREADS) {
        const int p = i / DOC_STAGE_MAX, b = i % DOC_STAGE_MAX;
        const DocLeaf lf = leaves[p];
        s_pat[i] = b < lf.len ? pat[lf.off + b] : (uint8_t)0;
    }
    if (threadIdx.x < n_leaves) s_leaf[threadIdx.x] = leaves[threadIdx.x];
    __syncthreads();

    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint8_t* buf = s_doc[w];
    const int64_t n_waves = (int64_t)gridDim.x * DOC_WAVES;
    for (int64_t u = (int64_t)blockIdx.x * DOC_WAVES + w; u < n_units; u += n_waves) {
        const int2 un = units[u];
        const uint8_t* doc = arena + row_start[un.x];
        const int32_t L = row_len[un.x];
        const int32_t padded = (L + 15) & ~15;
        const int32_t s0 = un.y * DOC_SEG;
        {
            const int32_t rel = s0 + lane * 16;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (rel < padded) v = *reinterpret_cast<const uint4*>(doc + rel);
            *reinterpret_cast<uint4*>(buf + lane * 16) = v;
            if (lane < ext_chunks) {
                const int32_t r2 = s0 + DOC_SEG + lane * 16;
                uint4 v2 = make_uint4(0, 0, 0, 0);
                if (r2 < padded) v2 = *reinterpret_cast<const uint4*>(doc + r2);
                *reinterpret_cast<uint4*>(buf + DOC_SEG + lane * 16) = v2;
            }
        }
        doc_wave_sync();
        const uint4 a = *reinterpret_cast<const uint4*>(buf + lane * 16);
        const uint32_t d[5] = {a.x, a.y, a.z, a.w, *reinterpret_cast<const uint32_t*>(buf + lane * 16 + 16)};
        const int32_t pos0 = s0 + lane * 16;
        const int row = un.x;
        for (int p = 0; p < n_leaves; ++p) {
            const DocLeaf lf = s_leaf[p];
            const int32_t lim = L - lf.len - pos0;   // start j of this lane is valid while j <= lim (the match ends inside the row)
            uint32_t cand = 0;
            if (lim >= 0) {
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const uint32_t win = (uint32_t)((((uint64_t)d[(j >> 2) + 1] << 32) | d[j >> 2]) >> (8 * (j & 3)));
                    cand |= ((j <= lim) & ((win & lf.pmask) == lf.prefix)) ? (1u << j) : 0u;
                }
            }
            bool hit = false;
            if (lf.len <= 4) {
                hit = cand != 0;
            } else {
                const uint8_t* pp = s_pat + p * DOC_STAGE_MAX;
                while (cand && !hit) {
                    const int j = __builtin_ctz(cand);
                    cand &= cand - 1;
                    const uint8_t* q = buf + lane * 16 + j;
                    int k = 4;
                    while (k < lf.len && q[k] == pp[k]) ++k;
                    hit = k == lf.len;
                }
            }
            if (__ballot(hit) && lane == 0) atomicOr(&bits[(int64_t)lf.slot * words + (row >> 5)], 1u << (row & 31));
        }
        doc_wave_sync();   // every lane is done with buf before the next unit overwrites it
    }
}

// patterns longer than DOC_STAGE_MAX: lane l of the unit's wave tests starts s0 + l, s0 + l + 64, ... against global memory
__global__ __launch_bounds__(DOC_THREADS) void k_docs_contains_long(const uint8_t* __restrict__ arena, const int64_t* __restrict__ row_start,
                                                                    const int32_t* __restrict__ row_len, const int2* __restrict__ units,
                                                                    int64_t n_units, const DocLeaf* __restrict__ leaves, int n_leaves,
                                                                    const uint8_t* __restrict__ pat, uint32_t* __restrict__ bits, int64_t words) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t n_waves = (int64_t)gridDim.x * DOC_WAVES;
    for (int p = 0; p < n_leaves; ++p) {
        const DocLeaf lf = leaves[p];
        const uint8_t* pp = pat + lf.off;
        for (int64_t u = (int64_t)blockIdx.x * DOC_WAVES + w; u < n_units; u += n_waves) {
            const int2 un = units[u];
            const uint8_t* doc = arena + row_start[un.x];
            const int32_t L = row_len[un.x];
            const int32_t s0 = un.y * DOC_SEG;
            bool hit = false;
            for (int32_t s = s0 + lane; s < s0 + DOC_SEG && s + lf.len <= L && !hit; s += 64) {
                int32_t k = 0;
                while (k < lf.len && doc[s + k] == pp[k]) ++k;
                hit = k == lf.len;
            }
            if (__ballot(hit) && lane == 0) atomicOr(&bits[(int64_t)lf.slot * words + (un.x >> 5)], 1u << (un.x & 31));
        }
    }
}

// out[w] = program(leaf bitmaps)[w] & base[w] (base may be null); bits past `rows` cleared. The program was checked on the
// host (check_program, rdx_store.hpp): every op is a leaf index < P or OP_NOT / OP_AND / OP_OR, the stack never underflows, never
// exceeds FILTER_MAX_STACK, ends at 1.
__global__ __launch_bounds__(DOC_EVAL_THREADS) void k_docs_eval(const uint32_t* __restrict__ leaf_bits, int64_t words, int64_t rows,
                                                                const int32_t* __restrict__ prog, int n_ops, const uint32_t* __restrict__ base,
                                                                uint32_t* __restrict__ out) {
    __shared__ int32_t s_prog[FILTER_MAX_OPS];
    __shared__ uint32_t s_stack[FILTER_MAX_STACK - 1][DOC_EVAL_THREADS];   // below the top, which stays in a register
    for (int i = threadIdx.x; i < n_ops; i += DOC_EVAL_THREADS) s_prog[i] = prog[i];
    __syncthreads();
    const int t = threadIdx.x;
    const int64_t wd = (int64_t)blockIdx.x * DOC_EVAL_THREADS + t;
    if (wd >= words) return;
    uint32_t top = 0;
    int sp = 0;   // entries below the top
    for (int i = 0; i < n_ops; ++i) {
        const int32_t op = s_prog[i];
        if (op >= 0) {
            if (i > 0) s_stack[sp++][t] = top;
            top = leaf_bits[(int64_t)op * words + wd];
        } else if (op == OP_NOT) {
            top = ~top;
        } else {
            const uint32_t b = s_stack[--sp][t];
            top = op == OP_AND ? (b & top) : (b | top);
        }
    }
    if (base) top &= base[wd];
    if (wd == words - 1 && (rows & 31)) top &= (1u << (rows & 31)) - 1u;
    out[wd] = top;
}

// compaction: row i's padded bytes move from src + src_start[i] to dst + dst_start[i] (one block per row, 16 B per thread)
__global__ __launch_bounds__(256) void k_docs_gather(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                     const int64_t* __restrict__ src_start, const int64_t* __restrict__ dst_start,
                                                     const int32_t* __restrict__ len, int64_t n) {
    for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
        const int64_t padded = (len[i] + 15) & ~15;
        const uint4* s = reinterpret_cast<const uint4*>(src + src_start[i]);
        uint4* d = reinterpret_cast<uint4*>(dst + dst_start[i]);
        for (int64_t c = threadIdx.x; c < padded / 16; c += blockDim.x) d[c] = s[c];
    }
}

}  // namespace rdx
