// meta_kernel.hpp — the device metadata store behind Chroma's `where` filter (include/rdx.h rdx_meta_*).
//
// Column layout (one pair of arrays per column slot, owned by rdx_meta in rdx_meta.hip, in the collection's row order):
//   kind  uint8  [rows]   0 missing, 1 str, 2 int, 3 float, 4 bool (rag_dpo_amd/where.py K_*)
//   pay   double [rows]   int / float / bool rows: the value as where.py's Column.num holds it; str rows: (double)code, the
//                         string's index in the column's host vocabulary (an int32 >= 0: exact); missing rows: +0.0
//   A leaf is true for a row iff kind == leaf.kind and `pay <op> leaf.num` in IEEE double arithmetic. Codes being exact in a
//   double, `code == leaf.code` is that same comparison, so one test serves every kind: a NaN operand matches nothing,
//   -0.0 == 0.0, and a row of another kind (an int 1 against a bool True) never matches. 9 bytes are read per row and column.
//
// Predicate scan (k_meta_filter): a lane owns META_ROWS rows at a time, a wave 64 META_ROWS consecutive rows (lane l: rows
// r0 + 64 u + l, so that each of a column's META_ROWS loads is coalesced and all are in flight together), and the waves take
// the rows grid-stride. The leaf table, the column table and the postfix program are indexed by wave-uniform values only, so
// they are read through scalar loads (the scalar cache keeps them; no LDS), and their cost is shared by the lane's rows. A
// column's kind and payload are loaded when a leaf names another column than the one held in registers:
//   SORTED (at most META_SORTED_LEAVES leaves, the host has ordered them by column and renumbered the program): every leaf is
//     tested first, its verdict kept as bit i of one 64-bit register per row — every column is loaded exactly once per row —
//     and the program then runs on those bits;
//   otherwise the leaves are tested in program order: once per run of leaves on one column (a `$in` of any length is one
//     run); a column named again later is loaded again (from the caches).
// The boolean stack is one 32-bit register per row (bit 0 = top, at most FILTER_MAX_STACK entries). Each 64 verdicts become one
// ballot; lanes 0 .. 2 META_ROWS - 1 store the ballots' halves (ANDed with base_bits) with plain vector stores: every output
// word has exactly one writer, so no atomics and no dependence on the schedule. Rows past `rows` vote 0: the tail bits are zero.
#pragma once
#include "rdx_common.hpp"

namespace rdx {

constexpr int META_THREADS = 256;
constexpr int META_ROWS = 4;                 // rows per lane and pass: a wave takes 256 consecutive rows, four loads in flight per column
constexpr int META_MAX_LEAVES = 1024;
constexpr int META_SORTED_LEAVES = 64;
constexpr int32_t META_EQ = 0, META_GT = 1, META_GE = 2, META_LT = 3, META_LE = 4, META_CONST0 = 5, META_CONST1 = 6;

struct MetaLeaf {      // include/rdx.h rdx_meta_leaf, with num = (double)code for a str leaf and col = -1 for a CONST leaf
    int32_t col;       // index into the launch's column table
    int32_t op;
    int32_t kind;
    int32_t code;
    double num;
};

struct MetaCol {
    const uint8_t* kind;
    const double* pay;
};

// a column pointer read out of the column table is a generic one to the compiler; both arrays are hipMalloc'ed: as global
// pointers the loads are global_load (one wait counter) instead of flat_load
typedef const __attribute__((address_space(1))) uint8_t* meta_kind_ptr;
typedef const __attribute__((address_space(1))) double* meta_pay_ptr;

// one leaf against the lane's META_ROWS rows; everything but k and x is wave-uniform, so the op is one scalar branch per leaf
__device__ __forceinline__ void meta_test(int32_t op, int32_t kind, double num, const int (&k)[META_ROWS], const double (&x)[META_ROWS],
                                          uint32_t (&v)[META_ROWS]) {
#pragma unroll
    for (int u = 0; u < META_ROWS; ++u) v[u] = 0;
    if (op == META_EQ) {
#pragma unroll
        for (int u = 0; u < META_ROWS; ++u) v[u] = x[u] == num;
    } else if (op == META_GT) {
#pragma unroll
        for (int u = 0; u < META_ROWS; ++u) v[u] = x[u] > num;
    } else if (op == META_GE) {
#pragma unroll
        for (int u = 0; u < META_ROWS; ++u) v[u] = x[u] >= num;
    } else if (op == META_LT) {
#pragma unroll
        for (int u = 0; u < META_ROWS; ++u) v[u] = x[u] < num;
    } else if (op == META_LE) {
#pragma unroll
        for (int u = 0; u < META_ROWS; ++u) v[u] = x[u] <= num;
    }
#pragma unroll
    for (int u = 0; u < META_ROWS; ++u) v[u] = op == META_CONST1 ? 1u : (v[u] & (uint32_t)(k[u] == kind));
}

// NOT / AND / OR on the lane's bit stacks (bit 0 = top)
__device__ __forceinline__ void meta_fold(int32_t op, uint32_t (&st)[META_ROWS]) {
#pragma unroll
    for (int u = 0; u < META_ROWS; ++u) {
        if (op == OP_NOT) {
            st[u] ^= 1u;
        } else {
            const uint32_t a = st[u] & 1u;
            st[u] >>= 1;
            st[u] = op == OP_AND ? (st[u] & (a | ~1u)) : (st[u] | a);
        }
    }
}

// The query was checked on the host (rdx_meta_set_query; the program by check_program, rdx_store.hpp): every program op is a leaf
// index < n_leaves or OP_NOT / OP_AND / OP_OR, the stack never underflows, never exceeds FILTER_MAX_STACK and ends at one entry; every leaf's col is -1 or a column of
// exactly `rows` rows. words = ceil(rows / 32); base may be null.
template <bool SORTED>
__global__ __launch_bounds__(META_THREADS) void k_meta_filter(const MetaCol* __restrict__ cols, const MetaLeaf* __restrict__ leaves,
                                                              int n_leaves, const int32_t* __restrict__ prog, int n_ops, int64_t rows,
                                                              int64_t words, const uint32_t* __restrict__ base, uint32_t* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (META_THREADS / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t step = (int64_t)gridDim.x * META_THREADS * META_ROWS;
    for (int64_t r0 = wave * (64 * META_ROWS); r0 < rows; r0 += step) {   // r0 is the same in every lane of the wave: all 64 reach the ballots
        int32_t cur = -1;
        int k[META_ROWS];
        double x[META_ROWS];
        uint32_t st[META_ROWS], v[META_ROWS];
#pragma unroll
        for (int u = 0; u < META_ROWS; ++u) k[u] = 0, x[u] = 0.0, st[u] = 0;
        // the lane's rows are r0 + 64 u + lane: the loads of one column are META_ROWS coalesced, independent requests
        auto load = [&](int32_t col) {
            cur = col;
            const MetaCol c = cols[col];
#pragma unroll
            for (int u = 0; u < META_ROWS; ++u) {
                const int64_t row = r0 + 64 * u + lane;
                if (row < rows) {
                    k[u] = ((meta_kind_ptr)c.kind)[row];
                    x[u] = ((meta_pay_ptr)c.pay)[row];
                }
            }
        };
        if (SORTED) {
            uint64_t lv[META_ROWS];
#pragma unroll
            for (int u = 0; u < META_ROWS; ++u) lv[u] = 0;
            for (int i = 0; i < n_leaves; ++i) {
                const MetaLeaf lf = leaves[i];
                if (lf.col >= 0 && lf.col != cur) load(lf.col);
                meta_test(lf.op, lf.kind, lf.num, k, x, v);
#pragma unroll
                for (int u = 0; u < META_ROWS; ++u) lv[u] |= (uint64_t)v[u] << i;
            }
            for (int j = 0; j < n_ops; ++j) {
                const int32_t op = prog[j];
                if (op >= 0) {
#pragma unroll
                    for (int u = 0; u < META_ROWS; ++u) st[u] = (st[u] << 1) | (uint32_t)((lv[u] >> op) & 1u);
                } else {
                    meta_fold(op, st);
                }
            }
        } else {
            for (int j = 0; j < n_ops; ++j) {
                const int32_t op = prog[j];
                if (op >= 0) {
                    const MetaLeaf lf = leaves[op];
                    if (lf.col >= 0 && lf.col != cur) load(lf.col);
                    meta_test(lf.op, lf.kind, lf.num, k, x, v);
#pragma unroll
                    for (int u = 0; u < META_ROWS; ++u) st[u] = (st[u] << 1) | v[u];
                } else {
                    meta_fold(op, st);
                }
            }
        }
        // 2 META_ROWS output words per wave: lane l < 2 META_ROWS stores half (l & 1) of the ballot over rows r0 + 64 (l >> 1) + 0..63
        uint32_t mine = 0;
#pragma unroll
        for (int u = 0; u < META_ROWS; ++u) {
            const unsigned long long votes = __ballot((r0 + 64 * u + lane < rows) && (st[u] & 1u));
            if ((lane >> 1) == u) mine = (uint32_t)(votes >> (32 * (lane & 1)));
        }
        const int64_t w = (r0 >> 5) + lane;
        if (lane < 2 * META_ROWS && w < words) {
            if (base) mine &= base[w];
            out[w] = mine;
        }
    }
}

}  // namespace rdx
