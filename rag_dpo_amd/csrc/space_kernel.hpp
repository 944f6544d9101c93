// space_kernel.hpp — the inner-product and squared-L2 spaces on top of the cosine engine (gfx950). DESIGN.md §17 states the
// reduction and the proof; rag_dpo_amd/spaces.py is the model these kernels are pinned to, bit for bit.
//
// A collection in the "ip" or "l2" space keeps LIFTED rows in the cosine engine, stored verbatim: y = 2^e x (ip), or
// y = 2^e (x, a, 0, 0, 0) with a = (float)(-|x|^2 / 2) (l2). The engine returns candidates by <p^, y>; these kernels turn them into
// the space's own distances, computed from the raw query and x = 2^-e y (exact), and order them.
//
// The sum (space_sum). Every distance and every squared norm is a sum of dim terms in fp64, added in ONE order: 64 partial sums,
// partial l takes the terms j = l, l + 64, ... in that order from +0.0; the partials meet in a xor butterfly, s[l] += s[l ^ m] for
// m = 32, 16, 8, 4, 2, 1 (the order rdx_topic_boost documents). ip terms are (double)q_j * (double)x_j (exact: 48 significant bits);
// l2 terms are diff = (double)q_j - (double)x_j, sq = diff * diff, each rounded once, never fused: contraction is switched off in
// space_sum, since numpy cannot fuse and the two must agree.
// Lane l owns partial l, but a lane loads 16 bytes (elements 4l .. 4l + 3 of a 256-element chunk), so a chunk goes through the
// wave's own 2 KiB of LDS: written as float4, read back as the scalars l, l + 64, l + 128, l + 192 (both conflict-free).
// No atomics: the same inputs give the same bits on every call, on any stream.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rdx {

constexpr int SPACE_IP = 0, SPACE_L2 = 1;
constexpr int SPACE_THREADS = 256;         // 4 waves = 4 rows or 4 (query, row) pairs
constexpr int SPACE_WAVES = SPACE_THREADS / 64;
constexpr int SPACE_MAX_DIM = 4096;        // the engine's MAX_DIM; an l2 collection has 4 columns less
constexpr int SPACE_MAX_CAND = 4096;       // candidates per query in rdx_space_rescore (the engine's largest k)
constexpr int SPACE_MAX_PAGE_QUERIES = 64; // queries per rdx_space_distances call

// the lifted dimension: what the cosine engine is created with
__host__ __device__ __forceinline__ int space_lifted_dim(int kind, int dim) { return kind == SPACE_L2 ? dim + 4 : dim; }

// MODE 0: sum of q_j * x_j; MODE 1: sum of (q_j - x_j)^2; x_j = ldexpf(y_j, -yexp). Every wave of the block calls it with the same
// dim (the barriers are the block's); q and y are 16-byte aligned, dim a multiple of 4; stage = this wave's 512 floats of LDS.
// All 64 lanes return the same bits.
template <int MODE>
__device__ __forceinline__ double space_sum(const float* __restrict__ q, const float* __restrict__ y, int yexp, int dim, int lane,
                                            float* __restrict__ stage) {
#pragma clang fp contract(off)
    float* sq = stage;
    float* sx = stage + 256;
    double acc = 0.0;
    for (int j0 = 0; j0 < dim; j0 += 256) {
        const int j = j0 + 4 * lane;
        float4 qv = make_float4(0.f, 0.f, 0.f, 0.f), yv = qv;
        if (j < dim) {
            qv = *reinterpret_cast<const float4*>(q + j);
            yv = *reinterpret_cast<const float4*>(y + j);
        }
        __syncthreads();   // the previous chunk has been read
        reinterpret_cast<float4*>(sq)[lane] = qv;
        reinterpret_cast<float4*>(sx)[lane] = make_float4(ldexpf(yv.x, -yexp), ldexpf(yv.y, -yexp), ldexpf(yv.z, -yexp), ldexpf(yv.w, -yexp));
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (j0 + 64 * i + lane < dim) {   // (guarded: a term past dim adds nothing, not even +0.0)
                const double a = (double)sq[64 * i + lane], b = (double)sx[64 * i + lane];
                if (MODE == 0) {
                    const double t = a * b;
                    acc = acc + t;
                } else {
                    const double df = a - b;
                    const double t = df * df;
                    acc = acc + t;
                }
            }
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc = acc + __shfl_xor(acc, m, 64);
    return acc;
}

// the lifted coordinate of an l2 row and the row's lifted squared norm 4^-e |y|^2, from n2 = |x|^2 (space_sum<0>(x, x))
__device__ __forceinline__ float space_l2_coord(double n2) { return (float)(n2 * -0.5); }
__device__ __forceinline__ double space_lifted_sq(int kind, double n2) {
#pragma clang fp contract(off)
    if (kind != SPACE_L2) return n2;
    const double a = (double)space_l2_coord(n2);
    const double a2 = a * a;   // exact (48 bits)
    return n2 + a2;
}

// K_S0 (measure): one wave per raw row: lifted_sq[i] (fp64, before scaling) and bad[i] = the row cannot be lifted (NaN / Inf in
// it, or a lifted coordinate that is not finite in fp32). The host picks the scale from the largest lifted_sq.
__global__ void __launch_bounds__(SPACE_THREADS) k_space_measure(const float* __restrict__ rows, int64_t n, int dim, int kind,
                                                                double* __restrict__ lifted_sq, int32_t* __restrict__ bad) {
    __shared__ __attribute__((aligned(16))) float stage[SPACE_WAVES][512];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * SPACE_WAVES + wave;
    const bool on = i < n;
    const float* x = rows + (on ? i : 0) * (int64_t)dim;
    const double n2 = space_sum<0>(x, x, 0, dim, lane, stage[wave]);
    const double L = space_lifted_sq(kind, n2);
    if (on && lane == 0) {
        lifted_sq[i] = L;
        bad[i] = !(L < 1.0e300) || (kind == SPACE_L2 && !(fabsf(space_l2_coord(n2)) <= 3.4028234663852886e38f));
    }
}

// K_S1 (lift): one wave per raw row -> engine row [dim_e]: y_j = ldexpf(x_j, e); for l2 the columns dim .. dim + 3 are
// (ldexpf(a, e), 0, 0, 0), or (1, 0, 0, 0) for a query (is_query: e = 0). bad[i] = some ldexpf(y_j, -e) does not give x_j's bits
// back (the scaling lost bits or overflowed): such a row is refused by the host.
__global__ void __launch_bounds__(SPACE_THREADS) k_space_lift(const float* __restrict__ rows, int64_t n, int dim, int kind, int is_query,
                                                             int e, float* __restrict__ out, int32_t* __restrict__ bad) {
    __shared__ __attribute__((aligned(16))) float stage[SPACE_WAVES][512];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * SPACE_WAVES + wave;
    const bool on = i < n;
    const float* x = rows + (on ? i : 0) * (int64_t)dim;
    double n2 = 0.0;
    if (kind == SPACE_L2 && !is_query) n2 = space_sum<0>(x, x, 0, dim, lane, stage[wave]);   // (kind and is_query are uniform)
    if (!on) return;
    const int dim_e = space_lifted_dim(kind, dim);
    float* y = out + i * (int64_t)dim_e;
    bool lost = false;
    auto scaled = [&](float v) {
        const float s = ldexpf(v, e);
        lost |= __float_as_uint(ldexpf(s, -e)) != __float_as_uint(v);
        return s;
    };
    for (int g = lane; g < (dim >> 2); g += 64) {
        const float4 v = reinterpret_cast<const float4*>(x)[g];
        reinterpret_cast<float4*>(y)[g] = make_float4(scaled(v.x), scaled(v.y), scaled(v.z), scaled(v.w));
    }
    if (kind == SPACE_L2 && lane == 0)
        reinterpret_cast<float4*>(y)[dim >> 2] = make_float4(is_query ? 1.0f : scaled(space_l2_coord(n2)), 0.f, 0.f, 0.f);
    const bool any = __ballot(lost) != 0ull;
    if (lane == 0) bad[i] = any;
}

// the distance of the contract from the fp64 sum, rounded to fp32 once
__device__ __forceinline__ float space_distance(int kind, const float* __restrict__ q, const float* __restrict__ y, int e, int dim,
                                                int lane, float* __restrict__ stage) {
#pragma clang fp contract(off)
    if (kind == SPACE_L2) return (float)space_sum<1>(q, y, e, dim, lane, stage);
    const double s = space_sum<0>(q, y, e, dim, lane, stage);
    return (float)(1.0 - s);
}

// K_S2 (candidates): one wave per (query, candidate slot): dist[b][c] of the gathered engine row vecs[b * kp + c], +inf for the
// slots at or past counts[b].
__global__ void __launch_bounds__(SPACE_THREADS) k_space_cand(const float* __restrict__ queries, int64_t nq, int dim, int kind,
                                                             const float* __restrict__ vecs, const int32_t* __restrict__ counts,
                                                             int kp, int e, float* __restrict__ dist) {
    __shared__ __attribute__((aligned(16))) float stage[SPACE_WAVES][512];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t pair = (int64_t)blockIdx.x * SPACE_WAVES + wave, total = nq * kp;
    const bool on = pair < total;
    const int64_t p = on ? pair : 0;
    const int64_t b = p / kp;
    const int dim_e = space_lifted_dim(kind, dim);
    const float d = space_distance(kind, queries + b * dim, vecs + p * dim_e, e, dim, lane, stage[wave]);
    if (on && lane == 0) dist[p] = (int)(p - b * kp) < counts[b] ? d : INFINITY;
}

// K_S3 (page): one wave per (row, query) of a page of engine rows: out[b * stride + r], +inf when bit first_row + r of allow_bits
// is clear (allow_bits == NULL: every row passes). The queries of a row sit in neighbouring waves: the row is read from HBM once.
__global__ void __launch_bounds__(SPACE_THREADS) k_space_page(const float* __restrict__ queries, int nq, int dim, int kind,
                                                             const float* __restrict__ vecs, int64_t n, int e,
                                                             const uint32_t* __restrict__ allow_bits, int64_t first_row,
                                                             float* __restrict__ out, int64_t stride) {
    __shared__ __attribute__((aligned(16))) float stage[SPACE_WAVES][512];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t pair = (int64_t)blockIdx.x * SPACE_WAVES + wave, total = n * nq;
    const bool on = pair < total;
    const int64_t p = on ? pair : 0;
    const int64_t r = p / nq;
    const int b = (int)(p - r * nq);
    const int dim_e = space_lifted_dim(kind, dim);
    const float d = space_distance(kind, queries + (int64_t)b * dim, vecs + r * dim_e, e, dim, lane, stage[wave]);
    if (on && lane == 0) {
        const int64_t g = first_row + r;
        const bool ok = !allow_bits || ((allow_bits[g >> 5] >> (g & 31)) & 1u);
        out[(int64_t)b * stride + r] = ok ? d : INFINITY;
    }
}

// The lower bound (fp32) on the distance of every row the engine did NOT return, from the lowest returned engine score e_last
// (spaces.lower_bound32 is the same arithmetic in numpy). NaN when the query's norm is outside the range the
// guard's derivation covers: nothing is proven then.
constexpr double SPACE_PN2_MIN = 1.0e-18, SPACE_PN2_MAX = 1.0e30;
__device__ __forceinline__ float space_lower_bound32(int kind, float e_last, double n2q, int e, double guard) {
#pragma clang fp contract(off)
    const double UP30 = 1.0 + 0x1p-30, DN30 = 1.0 - 0x1p-30, T40 = 0x1p-40;
    const double pn2 = kind == SPACE_L2 ? n2q + 1.0 : n2q;
    if (!(pn2 >= SPACE_PN2_MIN && pn2 <= SPACE_PN2_MAX)) return __uint_as_float(0x7fc00000u);
    const double P = __dsqrt_rn(pn2);
    const double U = (double)e_last + guard;
    const double Pb = U >= 0.0 ? P * UP30 : P * DN30;
    const double B = ldexp(U * Pb, -e);
    double lb;
    if (kind == SPACE_L2) {
        const double Bup = B + fabs(B) * T40;
        lb = n2q * (1.0 - T40) - 2.0 * Bup;
    } else {
        double Bup = B + ldexp(P * UP30 * T40, -e);
        Bup = Bup + fabs(Bup) * T40;
        lb = 1.0 - Bup;
    }
    lb = lb - fabs(lb) * T40;
    return (float)lb;
}

// K_S4 (select + proof): one block per query. The count candidates are ranked by (distance ascending, row ascending) and the best
// k written (padding +inf / -1); proven[b] = 1 when no row outside the candidates can belong to the answer: fewer candidates than
// slots (the engine returned every allowed row), or the lower bound of the others is strictly above the k-th distance.
__global__ void __launch_bounds__(SPACE_THREADS) k_space_select(const float* __restrict__ queries, int dim, int kind,
                                                               const float* __restrict__ dist, const int64_t* __restrict__ cand_rows,
                                                               const float* __restrict__ cand_scores, const int32_t* __restrict__ counts,
                                                               int kp, int k, int e, double guard, float* __restrict__ out_dist,
                                                               int64_t* __restrict__ out_row, int32_t* __restrict__ out_count,
                                                               int32_t* __restrict__ proven) {
    __shared__ __attribute__((aligned(16))) float stage[SPACE_WAVES][512];
    __shared__ float s_d[SPACE_MAX_CAND];
    __shared__ int64_t s_r[SPACE_MAX_CAND];
    __shared__ float s_kth;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t b = blockIdx.x;
    const float* q = queries + b * dim;
    const double n2q = space_sum<0>(q, q, 0, dim, lane, stage[wave]);
    int c = counts[b];
    c = c < 0 ? 0 : (c > kp ? kp : c);
    for (int i = threadIdx.x; i < c; i += SPACE_THREADS) {
        s_d[i] = dist[b * kp + i];
        s_r[i] = cand_rows[b * kp + i];
    }
    if (threadIdx.x == 0) s_kth = INFINITY;
    __syncthreads();
    const int kk = c < k ? c : k;
    float* o_d = out_dist + b * k;
    int64_t* o_r = out_row + b * k;
    for (int i = wave; i < c; i += SPACE_WAVES) {
        const float di = s_d[i];
        const int64_t ri = s_r[i];
        int rank = 0;
        for (int j0 = 0; j0 < c; j0 += 64) {
            const int j = j0 + lane;
            bool before = false;
            if (j < c) {
                const float dj = s_d[j];
                before = (dj < di) || (dj == di && s_r[j] < ri);
            }
            rank += __popcll(__ballot(before));
        }
        if (lane == 0 && rank < kk) {
            o_d[rank] = di;
            o_r[rank] = ri;
            if (rank == k - 1) s_kth = di;
        }
    }
    for (int i = kk + threadIdx.x; i < k; i += SPACE_THREADS) {
        o_d[i] = INFINITY;
        o_r[i] = -1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        out_count[b] = kk;
        int ok = 1;
        if (c >= kp) ok = space_lower_bound32(kind, cand_scores[b * kp + kp - 1], n2q, e, guard) > s_kth;
        proven[b] = ok;
    }
}

}  // namespace rdx
