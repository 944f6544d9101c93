// k_rows.hpp — row-wise kernels: K1 L2-normalise (+ tiled fp16 scan copy), gather, exact scoring, dense select.
// One 64-lane wavefront owns one row: 16 B/lane coalesced loads, fp64 lane-order sums (oracle/rdx_oracle.c: see exact_dot4).
// The exact path's kernels take ExactParams / SelectParams; RowIds and TopkOut are the value types they share with k_refine.
// The device helpers without a kernel (MasterView, exact_score, rank_and_write, ...) are rows_core.hpp, which other units include too;
// this header holds kernels, so rdx_index.hip alone includes it.
#pragma once
#include "rows_core.hpp"

namespace rdx {

// write the 4 consecutive elements k..k+3 of a normalised row into a scan copy (corpus: fragment order, queries: LDS images)
template <bool QUERY>
__device__ __forceinline__ void shadow_store4(_Float16* __restrict__ shadow, int64_t row, int k, int ksteps,
                                              float scale, float4 y) {
    half4 h;
    h[0] = (_Float16)(y.x * scale);   // RNE; y * 2^s is exact
    h[1] = (_Float16)(y.y * scale);
    h[2] = (_Float16)(y.z * scale);
    h[3] = (_Float16)(y.w * scale);
    *reinterpret_cast<half4*>(shadow + (QUERY ? query_off(row, k, ksteps) : corpus_off(row, k, ksteps))) = h;
}

// K1. out = in / max(|in|_2, 1e-12)  — SentenceTransformer.encode(normalize_embeddings=True),
// reference src/utils/embedding_provider.py:139-145; also what `collection.add` needs for the cosine
// space (reference src/processing/create_chromadb_index.py:100-106,374-379).
// Destination row of input row i is dst_rows ? dst_rows[i] : row0 + i.
template <bool QUERY>
__global__ __launch_bounds__(256) void k_normalize(const float* __restrict__ in, const uint16_t* __restrict__ in_bf16,
                                                   int64_t n, int dim, const int64_t* __restrict__ dst_rows,
                                                   int64_t row0, MasterView master,
                                                   _Float16* __restrict__ shadow, int ksteps, float scale,
                                                   int* __restrict__ bad, int64_t n_pad = 0, int verbatim = 0) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if constexpr (QUERY) {
        // the query scan copy is rebuilt for every search: padding rows [n, n_pad) and padding columns [dim, 64*ksteps) are
        // written as zeros here (no separate memset launch)
        if (i >= n) {
            if (i < n_pad && shadow)
                for (int g = lane; g < ksteps * 16; g += 64) shadow_store4<true>(shadow, row0 + i, 4 * g, ksteps, scale, make_float4(0.f, 0.f, 0.f, 0.f));
            return;
        }
        if (shadow)
            for (int g = (dim >> 2) + lane; g < ksteps * 16; g += 64)
                shadow_store4<true>(shadow, row0 + i, 4 * g, ksteps, scale, make_float4(0.f, 0.f, 0.f, 0.f));
    }
    if (i >= n) return;
    const int n4 = dim >> 2;
    auto load4 = [&](int g) -> float4 {
        if (in_bf16) {
            const ushort4 u = reinterpret_cast<const ushort4*>(in_bf16 + i * (int64_t)dim)[g];
            return make_float4(__uint_as_float((uint32_t)u.x << 16), __uint_as_float((uint32_t)u.y << 16),
                               __uint_as_float((uint32_t)u.z << 16), __uint_as_float((uint32_t)u.w << 16));
        }
        return reinterpret_cast<const float4*>(in + i * (int64_t)dim)[g];
    };
    // dim <= 1024: the row's (up to) four float4 groups per lane are requested together and kept in registers for the second
    // pass — one memory round trip instead of four dependent ones plus four re-reads (a query batch is a handful of rows: the
    // kernel is all latency). Same additions in the same order per lane, same butterfly: the same bits.
    const bool in_regs = n4 <= 256;
    float4 rv[4];
    if (in_regs) {
#pragma unroll
        for (int u = 0; u < 4; ++u) rv[u] = load4(lane + 64 * u < n4 ? lane + 64 * u : n4 - 1);
    }
    double acc = 0.0;
    if (in_regs) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (lane + 64 * u < n4) {
                acc += (double)rv[u].x * (double)rv[u].x;
                acc += (double)rv[u].y * (double)rv[u].y;
                acc += (double)rv[u].z * (double)rv[u].z;
                acc += (double)rv[u].w * (double)rv[u].w;
            }
        }
    } else {
        for (int g = lane; g < n4; g += 64) {
            const float4 v = load4(g);
            acc += (double)v.x * (double)v.x;
            acc += (double)v.y * (double)v.y;
            acc += (double)v.z * (double)v.z;
            acc += (double)v.w * (double)v.w;
        }
    }
    const double n2 = wave_sum(acc);
    if (!(n2 < 1.0e300)) {   // NaN or Inf somewhere in the row: reject the whole call
        if (lane == 0) atomicOr(bad, 1);
        return;
    }
    double den = sqrt(n2);
    if (den < 1e-12) den = 1e-12;
    if (verbatim) den = 1.0;   // rows that ARE stored values (snapshot reload): x / 1.0 == x, kept bit for bit
    const int64_t dst = dst_rows ? dst_rows[i] : row0 + i;
    if (master.raw16 && lane == 0) master.den[dst] = den;   // compact master: the raw row + its divisor
    auto emit = [&](int g, const float4& v) __attribute__((always_inline)) {
        float4 y;
        y.x = (float)((double)v.x / den);
        y.y = (float)((double)v.y / den);
        y.z = (float)((double)v.z / den);
        y.w = (float)((double)v.w / den);
        if (master.f32) reinterpret_cast<float4*>(master.f32 + dst * (int64_t)dim)[g] = y;
        if (master.raw16) reinterpret_cast<ushort4*>(master.raw16 + dst * (int64_t)dim)[g] = reinterpret_cast<const ushort4*>(in_bf16 + i * (int64_t)dim)[g];
        if (shadow) shadow_store4<QUERY>(shadow, dst, 4 * g, ksteps, scale, y);
    };
    if (in_regs) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (lane + 64 * u < n4) emit(lane + 64 * u, rv[u]);
    } else {
        for (int g = lane; g < n4; g += 64) emit(g, load4(g));
    }
}

// row_map[first + i] = base + first + i (identity part of a shard's local -> global row id map)
__global__ __launch_bounds__(256) void k_iota64(int64_t* __restrict__ out, int64_t first, int64_t n, int64_t base) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[first + i] = base + first + i;
}

// rebuild the scan copy of rows [row0, row0+n) from the (already normalised) master copy
__global__ __launch_bounds__(256) void k_reshadow(MasterView master, int64_t row0, int64_t n, int dim,
                                                  _Float16* __restrict__ shadow, int ksteps, float scale) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (i >= n) return;
    const int64_t r = row0 + i;
    const int n4 = dim >> 2;
    const MasterRow row = master_row(master, r, dim);
    for (int g = lane; g < n4; g += 64) shadow_store4<false>(shadow, r, 4 * g, ksteps, scale, row[g]);
}

// out[i] = master[rows[i]]  (collection.get(include=["embeddings"]), compaction)
__global__ __launch_bounds__(256) void k_gather_rows(MasterView master, const int64_t* __restrict__ rows,
                                                     int64_t n, int dim, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (i >= n) return;
    const MasterRow src = master_row(master, rows[i], dim);
    float4* dst = reinterpret_cast<float4*>(out + i * (int64_t)dim);
    for (int g = lane; g < (dim >> 2); g += 64) dst[g] = src[g];
}

// compaction of a compact master: raw rows and divisors move as they are
__global__ __launch_bounds__(256) void k_gather_raw(MasterView master, const int64_t* __restrict__ rows, int64_t n, int dim,
                                                    MasterView out) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (i >= n) return;
    const int64_t r = rows[i];
    const ushort4* src = reinterpret_cast<const ushort4*>(master.raw16 + r * (int64_t)dim);
    ushort4* dst = reinterpret_cast<ushort4*>(out.raw16 + i * (int64_t)dim);
    for (int g = lane; g < (dim >> 2); g += 64) dst[g] = src[g];
    if (lane == 0) out.den[i] = master.den[r];
}

// K5a. Exact scores of up to QX queries against EVERY row (small problems, huge k, overflow fallback):
// out[j][r] = score(q_list[j], r), or -inf when the row fails the `where` pre-filter.
constexpr int QX = 4;
struct ExactParams {   // of k_exact_scores and k_exact_scores_reg<U>; run_exact changes q_list and nq per group of QX queries
    MasterView master; int64_t rows; int dim;
    const float* qhat; const int32_t* q_list; int nq;   // the normalised queries [..][dim], and which nq <= QX of them
    const uint32_t* allow; float* out;                  // the `where` bitmap or NULL; [nq][rows]
    unsigned long long* t_first_inv;                    // profile = 3: max(~clock) over the blocks' starts (RefineCounters), or NULL
    // a filter per query (rdx_search_filtered; the PERQ instantiations, which do not read `allow`): query q is held to
    // bitmap ftab[qf[q]], or to none when qf[q] < 0
    const uint32_t* const* ftab; const int32_t* qf;
};

// PERQ: the bitmaps of the group's queries (NULL: no filter; j >= nq: the group's first query, never written) ...
__device__ __forceinline__ void exact_group_masks(const ExactParams& p, const uint32_t* (&mk)[QX]) {
#pragma unroll
    for (int j = 0; j < QX; ++j) {
        const int f = p.qf[p.q_list[j < p.nq ? j : 0]];
        mk[j] = f < 0 ? nullptr : p.ftab[f];
    }
}
// ... and which of them allow row r: bit j = query j of the group
__device__ __forceinline__ uint32_t exact_group_ok(const uint32_t* const (&mk)[QX], int64_t r) {
    uint32_t ok = 0;
#pragma unroll
    for (int j = 0; j < QX; ++j) ok |= (mk[j] ? ((mk[j][r >> 5] >> (r & 31)) & 1u) : 1u) << j;
    return ok;
}

// (PERQ = false: the shared bitmap or none, the kernel as it always was)
template <bool PERQ = false>
__global__ __launch_bounds__(256) void k_exact_scores(const ExactParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (p.t_first_inv && threadIdx.x == 0) atomicMax(p.t_first_inv, ~wall_clock64());   // profile = 3: earliest block start
    float4* q4 = reinterpret_cast<float4*>(smem);   // [nq][dim/4]
    const int n4 = p.dim >> 2, nq = p.nq;
    const int64_t rows = p.rows;
    for (int j = 0; j < nq; ++j) {
        const float4* src = reinterpret_cast<const float4*>(p.qhat + (int64_t)p.q_list[j] * p.dim);
        for (int g = threadIdx.x; g < n4; g += blockDim.x) q4[j * n4 + g] = src[g];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
    const uint32_t* mk[QX] = {};
    if constexpr (PERQ) exact_group_masks(p, mk);
    // A wave owns rows wave0, wave0 + nwaves, ...; the loads of a row's next four float4 groups are all issued before the
    // first of them is used (four independent 1 KiB requests in flight per wave instead of one: the kernel is latency-bound
    // at the reference's 16,919 rows). Per lane the groups are still added in increasing g: the oracle's lane order (exact_dot4).
    for (int64_t r = wave0; r < rows; r += nwaves) {
        // okq: bit j = query j of the group may have the row; the row is read and summed when any of them may
        uint32_t okq = 0;
        bool ok;
        if constexpr (PERQ) {
            okq = exact_group_ok(mk, r);
            ok = okq != 0;
        } else ok = !p.allow || ((p.allow[r >> 5] >> (r & 31)) & 1u);
        const MasterRow row4 = master_row(p.master, r, p.dim);
        double acc[QX];
#pragma unroll
        for (int j = 0; j < QX; ++j) acc[j] = 0.0;
        if (ok) {
            for (int g0 = lane; g0 < n4; g0 += 256) {
                float4 c[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) c[u] = g0 + 64 * u < n4 ? row4[g0 + 64 * u] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (g0 + 64 * u < n4) {
#pragma unroll
                        for (int j = 0; j < QX; ++j)
                            if (j < nq) exact_dot4(acc[j], q4[j * n4 + g0 + 64 * u], c[u]);
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < QX; ++j) {
            if (j < nq) {
                const float s = (float)wave_sum(acc[j]);
                if (lane == 0) p.out[(int64_t)j * rows + r] = (PERQ ? ((okq >> j) & 1u) != 0 : ok) ? s : -INFINITY;
            }
        }
    }
}

// K5a for dim <= 1024 (U = float4 groups per lane, 1..4): the same scores, bit for bit, with three changes that matter at the
// reference's own shape (16,919 rows, 4 queries, where this kernel IS the search). (1) The queries live in REGISTERS as
// doubles (64 per lane at d = 1024) instead of being re-read from LDS and re-converted for every row: the grid is small enough
// (2 blocks per CU) that a wave keeps them over ~8 rows. (2) The next row's loads are issued before the current row is
// summed (two rows in flight per wave). (3) The four per-query butterflies run as ONE transposed butterfly: after the m = 32
// stage a lane keeps two of the four partial sums, after m = 16 one, so 14 cross-lane dword moves and 7 additions replace 48
// and 24 — every addition pairs the same two values as wave_sum's butterfly (the order stated at exact_dot4), so the bits
// are the same. The sum of query j ends on lanes with (lane >> 4) == j.
// PERQ: a filter per query (ExactParams::qf); the row is loaded and summed either way, -inf is written per query.
template <int U, bool PERQ = false>
__global__ __launch_bounds__(256, 2) void k_exact_scores_reg(const ExactParams p) {
    if (p.t_first_inv && threadIdx.x == 0) atomicMax(p.t_first_inv, ~wall_clock64());   // profile = 3: earliest block start
    const int dim = p.dim, n4 = dim >> 2, nq = p.nq;
    const int64_t rows = p.rows;
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
    if (wave0 >= rows) return;
    const lane_groups<U> grp(lane, n4);
    float4 cur[U], nxt[U];
    grp.load(master_row(p.master, wave0, dim), cur);
    double qd[QX][U][4];
#pragma unroll
    for (int j = 0; j < QX; ++j) {
        const float4* src = reinterpret_cast<const float4*>(p.qhat + (int64_t)p.q_list[j < nq ? j : 0] * dim);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float4 q = src[grp.gi[u]];
            const bool on = j < nq && grp.gv[u];
            qd[j][u][0] = on ? (double)q.x : 0.0;
            qd[j][u][1] = on ? (double)q.y : 0.0;
            qd[j][u][2] = on ? (double)q.z : 0.0;
            qd[j][u][3] = on ? (double)q.w : 0.0;
        }
    }
    const bool hi32 = (lane & 32) != 0, hi16 = (lane & 16) != 0;
    const uint32_t* mk[QX] = {};
    if constexpr (PERQ) exact_group_masks(p, mk);
    for (int64_t r = wave0; r < rows; r += nwaves) {
        const int64_t rn = r + nwaves < rows ? r + nwaves : r;   // (the last iteration re-reads its own row: no branch around loads)
        grp.load(master_row(p.master, rn, dim), nxt);
        bool ok;   // of the query whose sum ends on this lane, j = lane >> 4
        if constexpr (PERQ) ok = (exact_group_ok(mk, r) >> (lane >> 4)) & 1u;
        else ok = !p.allow || ((p.allow[r >> 5] >> (r & 31)) & 1u);
        double acc[QX];
#pragma unroll
        for (int j = 0; j < QX; ++j) acc[j] = 0.0;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const double cx = (double)cur[u].x, cy = (double)cur[u].y, cz = (double)cur[u].z, cw = (double)cur[u].w;
#pragma unroll
            for (int j = 0; j < QX; ++j) {
                acc[j] += qd[j][u][0] * cx;   // (products of two floats are exact in double: fused or not, the same bits)
                acc[j] += qd[j][u][1] * cy;
                acc[j] += qd[j][u][2] * cz;
                acc[j] += qd[j][u][3] * cw;
            }
        }
        // transposed butterfly: m = 32 (keep queries {0,1} on lanes < 32, {2,3} on the others), m = 16, then m = 8..1 on the one left
        const double s0 = hi32 ? acc[0] : acc[2], s1 = hi32 ? acc[1] : acc[3];   // what the partner keeps
        double k0 = hi32 ? acc[2] : acc[0], k1 = hi32 ? acc[3] : acc[1];
        k0 += __shfl_xor(s0, 32, 64);
        k1 += __shfl_xor(s1, 32, 64);
        const double s2 = hi16 ? k0 : k1;
        double v = hi16 ? k1 : k0;
        v += __shfl_xor(s2, 16, 64);
#pragma unroll
        for (int m = 8; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
        const int j = lane >> 4;
        if ((lane & 15) == 0 && j < nq) p.out[(int64_t)j * rows + r] = ok ? (float)v : -INFINITY;
#pragma unroll
        for (int u = 0; u < U; ++u) cur[u] = nxt[u];
    }
}


// K5b. top-k of a dense score row (one block per listed query): radix select of the k-th largest score, then
// everything above it plus the LOWEST-row entries equal to it (ties -> ascending row id), then a rank sort.
// -inf marks rows excluded by the `where` pre-filter; they are never returned. (SELECT_MAX_K: rows_core.hpp)
#ifdef RDX_SELECT_STAMPS   // developer build (tools/select_stamps.py): where k_select_dense spends its time
__device__ unsigned long long g_select_stamps[16];
#define RDX_STAMP(i) do { __syncthreads(); if (blockIdx.x == 0 && threadIdx.x == 0) g_select_stamps[i] = wall_clock64(); } while (0)
#else
#define RDX_STAMP(i) do { } while (0)
#endif
struct SelectParams {   // of select_dense_query / k_select_dense; run_exact changes q_list per group of QX queries
    const float* scores; int64_t rows; const int32_t* q_list; int k;   // what K5a left [gridDim.x][rows]; the query of each block
    RowIds ids; TopkOut out;
    unsigned long long* t_last;                                        // profile = 3: latest block end (RefineCounters), or NULL
};

__device__ __forceinline__ void select_dense_query(const SelectParams& p) {
    __shared__ __attribute__((aligned(16))) uint32_t hist[HIST_WORDS];
    __shared__ uint32_t bc[4];
    __shared__ float s_s[SELECT_MAX_K];
    __shared__ int64_t s_r[SELECT_MAX_K];
    __shared__ int n_sel, n_eq_taken, wave_tot[16];
    const int j = blockIdx.x;
    const int q = p.q_list[j];
    const int64_t rows = p.rows;
    const int k = p.k;
    const RowIds ids = p.ids;
    const float* __restrict__ sc = p.scores + (int64_t)j * rows;
    float* o_s = p.out.score + (int64_t)q * k;
    int64_t* o_r = p.out.row + (int64_t)q * k;
    int32_t* o_c = p.out.count + q;
    if (rows == 0 || k == 0) {
        rank_and_write(s_s, s_r, 0, k, o_s, o_r, o_c);
        return;
    }
    RDX_STAMP(0);
    const int64_t kk = k < rows ? k : rows;
    int64_t n_gt;
    // Up to 32 Ki rows the block keeps the whole score row in REGISTERS (32 keys per thread, loaded once); longer rows are
    // re-read from global memory in every pass.
    constexpr int RN = 32;
    const bool in_regs = rows <= (int64_t)RN * 1024 && blockDim.x == 1024;
    uint32_t kreg[RN];
    if (in_regs) {
        // unconditional loads (clamped index), all in flight at once: written as "value or padding" the compiler guards every
        // load with its own branch and waits for each (17 L2 round trips at the reference's 16,919 rows: 5 us)
        float vreg[RN];
#pragma unroll
        for (int j = 0; j < RN; ++j) {
            const int64_t i = (int64_t)j * 1024 + threadIdx.x;
            vreg[j] = sc[i < rows ? i : rows - 1];
        }
#pragma unroll
        for (int j = 0; j < RN; ++j) asm volatile("" : "+v"(vreg[j]));   // the loads stay where they are
#pragma unroll
        for (int j = 0; j < RN; ++j) {
            const int64_t i = (int64_t)j * 1024 + threadIdx.x;
            kreg[j] = i < rows ? f2key_sel(vreg[j]) : 0u;   // padding key 0 sorts below every real score (finite or -inf)
        }
    }
    RDX_STAMP(1);
    const uint32_t kth = in_regs ? block_kth_largest_scan(
                                       [&](auto f) {
#pragma unroll
                                           for (int j = 0; j < RN; ++j)
                                               if ((int64_t)j * 1024 + threadIdx.x < rows) f(kreg[j]);
                                       },
                                       kk, hist, bc, &n_gt)
                                 : block_kth_largest([&](int64_t i) { return f2key_sel(sc[i]); }, rows, kk, hist, bc, &n_gt);
    RDX_STAMP(2);
    const int need_eq = (int)(kk - n_gt);   // >= 1
    constexpr int EQ_CAP = 1024;
    __shared__ int64_t eq_idx[EQ_CAP];
    __shared__ int n_eq;
    if (threadIdx.x == 0) {
        n_sel = 0;
        n_eq_taken = 0;
        n_eq = 0;
    }
    __syncthreads();
    // ONE more pass: entries strictly above the k-th key go to the list in any order; entries equal to it (normally one)
    // are collected on the side
    auto collect = [&](int64_t i, uint32_t key) {
        if (key > kth) {
            const int pos = atomicAdd(&n_sel, 1);
            s_s[pos] = key == SEL_KEY_ZERO ? sc[i] : key2f(key);   // (a zero keeps its own sign)
            s_r[pos] = ids.of(i);
        } else if (key == kth) {
            const int e = atomicAdd(&n_eq, 1);
            if (e < EQ_CAP) eq_idx[e] = i;
        }
    };
    if (in_regs) {
#pragma unroll
        for (int j = 0; j < RN; ++j) {
            const int64_t i = (int64_t)j * 1024 + threadIdx.x;
            if (i < rows) collect(i, kreg[j]);
        }
    } else {
        for (int64_t i = threadIdx.x; i < rows; i += blockDim.x) collect(i, f2key_sel(sc[i]));
    }
    __syncthreads();
    RDX_STAMP(3);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    if (n_eq <= EQ_CAP) {
        // of the equal entries the need_eq with the LOWEST rows belong to the answer (ties -> ascending row id)
        const int ne = n_eq;
        for (int e = threadIdx.x; e < ne; e += blockDim.x) {
            const int64_t i = eq_idx[e];
            int rank = 0;
            for (int f = 0; f < ne; ++f) rank += eq_idx[f] < i;
            if (rank < need_eq) {
                s_s[(int)n_gt + rank] = sc[i];
                s_r[(int)n_gt + rank] = ids.of(i);
            }
        }
    } else {
        // thousands of identical scores: walk the rows in order until need_eq equal entries are taken
        for (int64_t base = 0; base < rows; base += blockDim.x) {
            if (n_eq_taken >= need_eq) break;   // uniform: read after the barrier below
            const int64_t i = base + threadIdx.x;
            const bool eq = i < rows && f2key_sel(sc[i]) == kth;
            const unsigned long long m = __ballot(eq);
            if (lane == 0) wave_tot[wave] = __popcll(m);
            __syncthreads();
            int before = n_eq_taken;
            for (int w = 0; w < wave; ++w) before += wave_tot[w];
            const int my = before + __popcll(m & ((1ull << lane) - 1ull));
            if (eq && my < need_eq) {
                s_s[(int)n_gt + my] = sc[i];
                s_r[(int)n_gt + my] = ids.of(i);
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                int t = 0;
                for (int w = 0; w < nw; ++w) t += wave_tot[w];
                n_eq_taken += t;
            }
            __syncthreads();
        }
    }
    __syncthreads();
    RDX_STAMP(4);
    // drop -inf (filtered) entries: they sort last, so count the finite prefix after ranking
    const int n_top = (int)kk;
    __shared__ int n_fin;
    if (threadIdx.x == 0) n_fin = 0;
    __syncthreads();
    int loc = 0;
    for (int i = threadIdx.x; i < n_top; i += blockDim.x) loc += (s_s[i] > -INFINITY);
    if (loc) atomicAdd(&n_fin, loc);
    __syncthreads();
    const int valid = n_fin;
    RDX_STAMP(5);
    rank_and_write(s_s, s_r, n_top, valid < k ? valid : k, o_s, o_r, o_c);
    if (p.t_last) {   // profile = 3: latest block end
        __syncthreads();
        if (threadIdx.x == 0) atomicMax(p.t_last, wall_clock64());
    }
    RDX_STAMP(6);
    // rank_and_write filled [valid, k) only up to its own k argument; pad the rest
    for (int i = valid + threadIdx.x; i < k; i += blockDim.x) {
        o_s[i] = -INFINITY;
        o_r[i] = -1;
    }
}

// ---- int8 coarse pass (DESIGN.md §5 "int8 coarse pass"): block-scaled copies and their error terms ----------------------------
__device__ __forceinline__ float wave_max_f(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
    return v;
}
// a float >= x (x >= 0): the error terms are rounded up, never down
__device__ __forceinline__ float f32_up(double x) {
    float f = (float)x;
    if ((double)f < x) f = nextafterf(f, INFINITY);
    return f;
}
__device__ __forceinline__ int8_t q8(float y, float inv) {
    const float t = rintf(y * inv);
    return (int8_t)fminf(fmaxf(t, -127.f), 127.f);
}

// Corpus copy, one wave per 32-row block b (the rows one wave of k_scan owns in a tile): s_b = max |y| over the block / 127,
// c8 = rint(y / s_b) in fragment order (corpus_off8), eps_b = max over the block's rows of ||y - s_b c8||_2 (fp64, rounded up).
// y is the normalised row exactly as k_refine re-scores it (MasterRow: the fp32 master, or the compact master's bf16 / divisor).
// Rows past `rows` and columns past dim are zeros. eps_max (the bits of a float >= 0) takes the largest eps_b (atomicMax); epsb[b]
// keeps eps_b itself (what k_eps_edges and k_eps_classify sort the blocks into classes by).
__global__ __launch_bounds__(256) void k_quant8_corpus(MasterView master, int dim, int64_t rows, int64_t blk0, int64_t nblk,
                                                       int8_t* __restrict__ c8, int ksteps8, float* __restrict__ sblk,
                                                       unsigned int* __restrict__ eps_max, float* __restrict__ epsb) {
    const int lane = threadIdx.x & 63;
    const int64_t b = blk0 + (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (b >= blk0 + nblk) return;
    const int n4 = dim >> 2, np4 = ksteps8 * 32;   // float4 groups of a row: real, padded
    const int64_t r0 = b * 32;
    const int nr = (int)(rows - r0 < 32 ? rows - r0 : 32);
    float mx = 0.f;
    for (int r = 0; r < nr; ++r) {
        const MasterRow row = master_row(master, r0 + r, dim);
        for (int g = lane; g < n4; g += 64) {
            const float4 y = row[g];
            mx = fmaxf(mx, fmaxf(fmaxf(fabsf(y.x), fabsf(y.y)), fmaxf(fabsf(y.z), fabsf(y.w))));
        }
    }
    mx = wave_max_f(mx);
    const float s = mx / 127.f;
    const float inv = mx > 0.f ? 1.f / s : 0.f;   // (the rounding of inv is harmless: eps_b is measured on the c8 actually stored)
    double worst = 0.0;
    for (int r = 0; r < 32; ++r) {
        const MasterRow row = master_row(master, r0 + (r < nr ? r : 0), dim);
        double e2 = 0.0;
        for (int g = lane; g < np4; g += 64) {
            char4 v = make_char4(0, 0, 0, 0);
            if (r < nr && g < n4) {
                const float4 y = row[g];
                v = make_char4(q8(y.x, inv), q8(y.y, inv), q8(y.z, inv), q8(y.w, inv));
                const double d0 = (double)y.x - (double)s * v.x, d1 = (double)y.y - (double)s * v.y;
                const double d2 = (double)y.z - (double)s * v.z, d3 = (double)y.w - (double)s * v.w;
                e2 += d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
            }
            *reinterpret_cast<char4*>(c8 + corpus_off8(r0 + r, 4 * g, ksteps8)) = v;
        }
        worst = fmax(worst, wave_sum(e2));
    }
    if (lane == 0) {
        sblk[b] = s;
        const float eps = f32_up(sqrt(worst) * (1.0 + 1e-12));
        atomicMax(eps_max, __float_as_uint(eps));
        epsb[b] = eps;
    }
}

// Classes of block error (DESIGN.md §5 "classes of eps_b"). The int8 scan charges a block the edge of its class instead of the
// corpus' largest eps_b: edge[c], c < EPS_CLASSES - 1, is the ceil((1 - 2^-(c+1)) nb)-th smallest eps_b of the nb blocks of a full
// quantisation (an exact order statistic: the bits of floats >= 0 order as uint32), and the top class's edge is the live eps_max
// (never stored: k_tau8 reads it where it always did). A search with C <= EPS_CLASSES classes uses edges 0..C-2 and eps_max, and
// puts block b into class min(cls[b], C - 1): the edges nest, so one table of classes serves every C.
// One workgroup per stored edge.
__global__ __launch_bounds__(1024) void k_eps_edges(const float* __restrict__ epsb, int64_t nb, float* __restrict__ edge) {
    __shared__ __attribute__((aligned(16))) uint32_t hist[HIST_WORDS];
    __shared__ uint32_t bc[4];
    const int c = blockIdx.x;
    const int64_t tail = nb >> (c + 1);                       // floor(nb / 2^(c+1)): rank = nb - tail = ceil((1 - 2^-(c+1)) nb), 1-based
    int64_t n_gt;
    const uint32_t key = block_kth_largest([&](int64_t i) { return __float_as_uint(epsb[i]); }, nb, tail + 1, hist, bc, &n_gt);
    if (threadIdx.x == 0) edge[c] = __uint_as_float(key);
}

// cls[b] = the smallest c < EPS_CLASSES - 1 with eps_b <= edge[c], or EPS_CLASSES - 1 (whose edge is eps_max >= every eps_b). Blocks
// quantised after the edges were taken (appends) are classified against the same edges.
__global__ __launch_bounds__(256) void k_eps_classify(const float* __restrict__ epsb, int64_t blk0, int64_t nblk,
                                                      const float* __restrict__ edge, uint8_t* __restrict__ cls) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nblk) return;
    const float e = epsb[blk0 + i];
    int c = 0;
    while (c < EPS_CLASSES - 1 && !(e <= edge[c])) ++c;
    cls[blk0 + i] = (uint8_t)c;
}

// Query copy, one wave per query: t_q = max |q| / 127, q8 = rint(q / t_q) in the query-image order (query_off8), and, in fp64
// rounded up, e_q >= ||q - t_q q8||_2 and n_q >= ||t_q q8||_2. Padding queries [n, n_pad) and padding columns are zeros.
__global__ __launch_bounds__(256) void k_quant8_query(const float* __restrict__ qhat, int64_t n, int64_t n_pad, int dim,
                                                      int8_t* __restrict__ qs8, int ksteps8, float* __restrict__ tq,
                                                      float* __restrict__ eq, float* __restrict__ nqn) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (i >= n_pad) return;
    const int n4 = dim >> 2, np4 = ksteps8 * 32;
    const float4* q4 = reinterpret_cast<const float4*>(qhat + i * (int64_t)dim);
    const bool real = i < n;
    float mx = 0.f;
    if (real)
        for (int g = lane; g < n4; g += 64) {
            const float4 y = q4[g];
            mx = fmaxf(mx, fmaxf(fmaxf(fabsf(y.x), fabsf(y.y)), fmaxf(fabsf(y.z), fabsf(y.w))));
        }
    mx = wave_max_f(mx);
    const float t = mx > 0.f ? mx / 127.f : 1.f;
    const float inv = mx > 0.f ? 1.f / t : 0.f;
    double e2 = 0.0, n2 = 0.0;
    for (int g = lane; g < np4; g += 64) {
        char4 v = make_char4(0, 0, 0, 0);
        if (real && g < n4) {
            const float4 y = q4[g];
            v = make_char4(q8(y.x, inv), q8(y.y, inv), q8(y.z, inv), q8(y.w, inv));
            const double a0 = (double)t * v.x, a1 = (double)t * v.y, a2 = (double)t * v.z, a3 = (double)t * v.w;
            const double d0 = (double)y.x - a0, d1 = (double)y.y - a1, d2 = (double)y.z - a2, d3 = (double)y.w - a3;
            e2 += d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
            n2 += a0 * a0 + a1 * a1 + a2 * a2 + a3 * a3;
        }
        *reinterpret_cast<char4*>(qs8 + query_off8(i, 4 * g, ksteps8)) = v;
    }
    e2 = wave_sum(e2);
    n2 = wave_sum(n2);
    if (lane == 0) {
        tq[i] = t;
        eq[i] = f32_up(sqrt(e2) * (1.0 + 1e-12));
        nqn[i] = f32_up(sqrt(n2) * (1.0 + 1e-12));
    }
}

// Per query, from the fp16 bootstrap's threshold T (k_tau, fp16 accumulator units): the int8 pass' error bound
//   E_q = e_q (1 + 1e-6) + n_q eps_max + 1e-6                 (||y|| <= 1 + 1e-6, 1e-6 for the fp32 roundings)
// and its three thresholds: thr (int8 accumulator units D s_b, what k_scan<I8> compares: coarse + E_q >= T), tau_s (score
// units, what k_refine verifies c_k - 2E_q against: every row whose coarse score reaches tau_s was emitted) and 2E_q.
// With ncls > 1 classes of block error (k_eps_edges) thr is [ncls][nq_pad]: the top class ncls - 1 is the bound above with eps_max,
// to the statement; class c below it charges edge[c] instead, E_{q,c} = e_q (1 + 1e-6) + n_q edge[c] + 1e-6 <= E_q, and compares
// thr_c = fl_down((T - E_{q,c}) / t_q). A row of class c that was not emitted has coarse < tau_c = thr_c t_q + 1e-6 and so
// exact < tau_c + E_{q,c}: tau_s = max_c (tau_c + E_{q,c}) - E_q (fp64, rounded up) keeps k_refine's check X - E_q >= tau_s
// sufficient; 2E_q stays the band with eps_max.
__global__ __launch_bounds__(256) void k_tau8(const float* __restrict__ tau16, float inv_scale2, const float* __restrict__ tq,
                                              const float* __restrict__ eq, const float* __restrict__ nqn,
                                              const unsigned int* __restrict__ eps_max, int nq, int nq_pad,
                                              float* __restrict__ thr_all, float* __restrict__ tau_s, float* __restrict__ two_e,
                                              const float* __restrict__ edge, int ncls) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq_pad) return;
    float* const thr = thr_all + (size_t)(ncls - 1) * nq_pad;   // the top class: today's table
    if (i >= nq) {   // padding query: never emits
        for (int c = 0; c < ncls - 1; ++c) thr_all[(size_t)c * nq_pad + i] = INFINITY;
        thr[i] = INFINITY;
        tau_s[i] = INFINITY;
        two_e[i] = 0.f;
        return;
    }
    const double E = (double)eq[i] * (1.0 + 1e-6) + (double)nqn[i] * (double)__uint_as_float(*eps_max) + 1e-6;
    const float Ef = f32_up(E);
    two_e[i] = f32_up(2.0 * (double)Ef);
    const float T = tau16[i] * inv_scale2;   // (a power of two: exact; -inf stays -inf)
    if (!(T > -INFINITY)) {
        for (int c = 0; c < ncls - 1; ++c) thr_all[(size_t)c * nq_pad + i] = -INFINITY;
        thr[i] = -INFINITY;
        tau_s[i] = -INFINITY;
        return;
    }
    const double t = (double)tq[i];
    float th = (float)(((double)T - (double)Ef) / t);
    if ((double)th * t > (double)T - (double)Ef) th = nextafterf(th, -INFINITY);   // rounded down: a lower threshold only emits more
    thr[i] = th;
    const double ts = (double)th * t + 1e-6;
    float tsf = (float)ts;
    if ((double)tsf < ts) tsf = nextafterf(tsf, INFINITY);
    tau_s[i] = tsf;
    if (ncls == 1) return;
    double worst = (double)tsf + (double)Ef;   // max over the classes of tau_c + E_{q,c}; the top class's is tau_s + E_q
    bool lower = false;
    for (int c = 0; c < ncls - 1; ++c) {
        const float Ec = f32_up((double)eq[i] * (1.0 + 1e-6) + (double)nqn[i] * (double)edge[c] + 1e-6);
        float thc = (float)(((double)T - (double)Ec) / t);
        if ((double)thc * t > (double)T - (double)Ec) thc = nextafterf(thc, -INFINITY);
        thr_all[(size_t)c * nq_pad + i] = thc;
        const float tc = f32_up((double)thc * t + 1e-6);
        if ((double)tc + (double)Ec > worst) {
            worst = (double)tc + (double)Ec;
            lower = true;
        }
    }
    if (lower) {
        const double x = worst - (double)Ef;
        float f = (float)x;
        if ((double)f < x) f = nextafterf(f, INFINITY);
        tau_s[i] = f;
    }
}

}  // namespace rdx
