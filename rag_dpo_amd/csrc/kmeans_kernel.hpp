// kmeans_kernel.hpp — the kernels of rdx_index_kmeans (rag_dpo_amd/kmeans.py states the definition): the assignment
// (an argmax per stored row over the centroids, in the exact score's arithmetic), the stable order of rows by label (histogram per
// block of rows, one scan, placement by counted ranks: km_order.hpp), the ordered per-cluster sum in segments of KM_SEGMENT members
// and the new centroids. Included by rdx_derived.hip only. No kernel waits for another workgroup or launch.
#pragma once
#include "rows_core.hpp"
#include "km_order.hpp"

namespace rdx {

struct KmCounters {
    unsigned int changed;   // rows whose label the last assignment changed (k_km_publish re-zeroes it)
    int bad;                // K1 met a NaN or Inf in `init`
};

// ---- the assignment ---------------------------------------------------------------------------------------------------------------
constexpr int KM_ASSIGN_WAVES = 4;
constexpr int KM_ASSIGN_LDS = 32768;   // bytes of widened centroids per chunk while a row has U > 0 groups per lane (4 with U = 0)
struct KmAssignParams {
    MasterView master; int64_t rows; int dim;
    const float* qhat; int n_clusters;   // K1 of the centroids [K][dim]
    int chunk;                           // centroids per LDS chunk: a multiple of 4
    const uint32_t* allow;               // the bitmap or NULL
    int64_t* label; float* score;        // [rows]: what the last assignment left is read, this one's written
    KmCounters* ctr;
};

// A wave owns R consecutive rows; with U > 0 it keeps them in registers, U float4 groups per lane (lane_groups, dim <= 1024), with
// U = 0 (any dim) it reads its row again for every four centroids. The block stages p.chunk centroids at a time in LDS, widened to
// doubles as they are written ([chunk][ng][4], ng = 64 U groups, zeros past the row's end — a lane's clamped group then adds
// zeros, as in k_exact_scores_reg — or dim / 4 groups with U = 0). Four centroids are scored at a time: per lane the products of
// group lane, lane + 64, ... (x, y, z, w within a group) into one fp64 accumulator per centroid, then k_exact_scores_reg's transposed
// butterfly, which pairs the same values as wave_sum: the exact score's bits (exact_dot4). The sum of centroid j of the four ends on
// the lanes with (lane >> 4) == j; those lanes keep the best (fp32 score, smallest index) of their centroids, and the four classes
// meet at the end. "Larger score, else smaller index" is a total order on the pairs, so the grouping does not show.
template <int U, int R>
__global__ __launch_bounds__(64 * KM_ASSIGN_WAVES) void k_km_assign(const KmAssignParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* const qd = reinterpret_cast<double*>(smem);
    constexpr int UU = U > 0 ? U : 1;
    const int dim = p.dim, n4 = dim >> 2, K = p.n_clusters;
    const int ng = U > 0 ? 64 * U : n4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r0 = ((int64_t)blockIdx.x * KM_ASSIGN_WAVES + wave) * R;
    bool in[R], ok[R], any = false;
    int64_t rr[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const int64_t r = r0 + i;
        in[i] = r < p.rows;
        rr[i] = in[i] ? r : p.rows - 1;
        ok[i] = in[i] && (!p.allow || ((p.allow[r >> 5] >> (r & 31)) & 1u));
        any = any || ok[i];
    }
    const lane_groups<UU> grp(lane, n4);
    float4 c[R][UU];
    if (U > 0 && any) {
#pragma unroll
        for (int i = 0; i < R; ++i) grp.load(master_row(p.master, rr[i], dim), c[i]);
    }
    float best[R];
    int bidx[R];
#pragma unroll
    for (int i = 0; i < R; ++i) best[i] = -INFINITY, bidx[i] = 0x7fffffff;
    const bool hi32 = (lane & 32) != 0, hi16 = (lane & 16) != 0;
    for (int c0 = 0; c0 < K; c0 += p.chunk) {
        __syncthreads();   // the chunk before has been read
        for (int idx = threadIdx.x; idx < p.chunk * ng; idx += blockDim.x) {
            const int j = idx / ng, g = idx - j * ng;
            float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c0 + j < K && g < n4) q = reinterpret_cast<const float4*>(p.qhat + (int64_t)(c0 + j) * dim)[g];
            double* d = qd + (size_t)idx * 4;
            d[0] = (double)q.x, d[1] = (double)q.y, d[2] = (double)q.z, d[3] = (double)q.w;
        }
        __syncthreads();
        if (!any) continue;   // (wave-uniform: the wave's rows are all disallowed or past the end)
        for (int j0 = 0; j0 < p.chunk && c0 + j0 < K; j0 += 4) {
            double acc[R][4];
#pragma unroll
            for (int i = 0; i < R; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
            const double* const q0 = qd + (size_t)j0 * ng * 4;
            if constexpr (U > 0) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    double q[4][4];
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int e = 0; e < 4; ++e) q[j][e] = q0[((size_t)j * ng + lane + 64 * u) * 4 + e];
#pragma unroll
                    for (int i = 0; i < R; ++i) {
                        const double cx = (double)c[i][u].x, cy = (double)c[i][u].y, cz = (double)c[i][u].z, cw = (double)c[i][u].w;
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            acc[i][j] += q[j][0] * cx;   // (products of two floats are exact in double: fused or not, the same bits)
                            acc[i][j] += q[j][1] * cy;
                            acc[i][j] += q[j][2] * cz;
                            acc[i][j] += q[j][3] * cw;
                        }
                    }
                }
            } else {
                const MasterRow row4 = master_row(p.master, rr[0], dim);
                for (int g = lane; g < n4; g += 64) {
                    const float4 cv = row4[g];
                    const double cx = (double)cv.x, cy = (double)cv.y, cz = (double)cv.z, cw = (double)cv.w;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const double* q = q0 + ((size_t)j * ng + g) * 4;
                        acc[0][j] += q[0] * cx;
                        acc[0][j] += q[1] * cy;
                        acc[0][j] += q[2] * cz;
                        acc[0][j] += q[3] * cw;
                    }
                }
            }
            const int cidx = c0 + j0 + (lane >> 4);
#pragma unroll
            for (int i = 0; i < R; ++i) {
                // k_exact_scores_reg's transposed butterfly: m = 32 (keep {0,1} on lanes < 32, {2,3} on the others), m = 16, then 8..1
                const double s0 = hi32 ? acc[i][0] : acc[i][2], s1 = hi32 ? acc[i][1] : acc[i][3];
                double k0 = hi32 ? acc[i][2] : acc[i][0], k1 = hi32 ? acc[i][3] : acc[i][1];
                k0 += __shfl_xor(s0, 32, 64);
                k1 += __shfl_xor(s1, 32, 64);
                const double s2 = hi16 ? k0 : k1;
                double v = hi16 ? k1 : k0;
                v += __shfl_xor(s2, 16, 64);
#pragma unroll
                for (int m = 8; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
                const float s = (float)v;
                if (cidx < K && s > best[i]) best[i] = s, bidx[i] = cidx;   // (ascending indices per lane: a tie stays with the smaller)
            }
        }
    }
    unsigned int changed = 0;
#pragma unroll
    for (int i = 0; i < R; ++i) {
#pragma unroll
        for (int m = 16; m <= 32; m <<= 1) {
            const float os = __shfl_xor(best[i], m, 64);
            const int oi = __shfl_xor(bidx[i], m, 64);
            if (os > best[i] || (os == best[i] && oi < bidx[i])) best[i] = os, bidx[i] = oi;
        }
        if (lane == 0 && in[i]) {
            const int64_t now = ok[i] ? (int64_t)bidx[i] : -1;
            changed += p.label[r0 + i] != now ? 1u : 0u;
            p.label[r0 + i] = now;
            p.score[r0 + i] = ok[i] ? best[i] : -INFINITY;
        }
    }
    if (lane == 0 && changed) atomicAdd(&p.ctr->changed, changed);   // one add per wave; a count: the order does not show
}

// what the host waits for, once per assignment: (seq << 33) | (bad << 32) | changed into pinned host memory; the count starts over
__global__ void k_km_publish(KmCounters* ctr, unsigned long long* word, unsigned long long seq) {
    const unsigned long long v = (seq << 33) | ((unsigned long long)(ctr->bad != 0) << 32) | (unsigned long long)ctr->changed;
    ctr->changed = 0;
    __hip_atomic_store(word, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---- the stable order of rows by label (km_order.hpp) ------------------------------------------------------------------------------
struct KmOrderParams {
    const int64_t* label; int64_t rows; int n_clusters;
    int64_t span, n_blocks;   // rows per block (a multiple of KM_TILE), blocks
    int32_t* hist;            // [K][n_blocks] + 1: the histograms, then (k_km_scan) their exclusive prefix sums and the total
    int32_t* order;           // [rows]: the allowed rows by (label, row)
};
__device__ __forceinline__ int32_t km_label_of(const KmOrderParams& p, int64_t r, int64_t end) {
    if (r >= end) return -1;
    const int64_t l = p.label[r];
    return l >= 0 && l < p.n_clusters ? (int32_t)l : -1;
}

// hist[c][b] = rows of block b with label c (dynamic LDS: K counters)
__global__ __launch_bounds__(KM_TILE) void k_km_hist(const KmOrderParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int32_t* const cnt = reinterpret_cast<int32_t*>(smem);
    for (int c = threadIdx.x; c < p.n_clusters; c += KM_TILE) cnt[c] = 0;
    __syncthreads();
    const int64_t b = blockIdx.x, begin = b * p.span, end = begin + p.span < p.rows ? begin + p.span : p.rows;
    for (int64_t r = begin + threadIdx.x; r < end; r += KM_TILE) {
        const int32_t l = km_label_of(p, r, end);
        if (l >= 0) atomicAdd(&cnt[l], 1);   // a count: the order does not show
    }
    __syncthreads();
    for (int c = threadIdx.x; c < p.n_clusters; c += KM_TILE) p.hist[km_hist_index(c, b, p.n_blocks)] = cnt[c];
}

// the exclusive prefix sums of four consecutive values per thread over a block of 1 024 threads -> where v[0] begins; *total = their sum
__device__ __forceinline__ int32_t km_block_scan(const int32_t (&v)[4], int32_t* wsum, int32_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int32_t t = v[0] + v[1] + v[2] + v[3];
    int32_t inc = t;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int32_t x = __shfl_up(inc, off, 64);
        if (lane >= off) inc += x;
    }
    __syncthreads();   // wsum's last readers
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
        before += w < wave ? wsum[w] : 0;
        all += wsum[w];
    }
    *total = all;
    return before + inc - t;
}

// a[0..n) -> its exclusive prefix sums, a[n] = the total: one workgroup walks the array in tiles of 4 096 (integers: any order gives the same)
__global__ __launch_bounds__(1024) void k_km_scan(int32_t* __restrict__ a, int64_t n) {
    __shared__ int32_t wsum[16];
    int32_t carry = 0;
    for (int64_t base = 0; base < n; base += 4096) {
        const int64_t i = base + (int64_t)threadIdx.x * 4;
        int32_t v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = i + e < n ? a[i + e] : 0;
        int32_t total;
        int32_t ex = carry + km_block_scan(v, wsum, &total);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (i + e < n) a[i + e] = ex;
            ex += v[e];
        }
        carry += total;
    }
    if (threadIdx.x == 0) a[n] = carry;
}

// cluster_off[c] = where cluster c begins in the order ([K + 1]), seg_off[c] = segments of the clusters before c ([K + 1]), out_count[c] =
// its members (or NULL): one workgroup, the clusters in one tile
__global__ __launch_bounds__(1024) void k_km_seg_table(const int32_t* __restrict__ scanned, int64_t n_blocks, int n_clusters,
                                                       int32_t* __restrict__ cluster_off, int32_t* __restrict__ seg_off,
                                                       int64_t* __restrict__ out_count) {
    __shared__ int32_t wsum[16];
    const int K = n_clusters;
    int32_t v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int c = threadIdx.x * 4 + e;
        v[e] = 0;
        if (c < K) {
            const int32_t begin = scanned[km_hist_index(c, 0, n_blocks)];
            const int32_t end = scanned[c + 1 < K ? km_hist_index(c + 1, 0, n_blocks) : (int64_t)K * n_blocks];
            cluster_off[c] = begin;
            if (c + 1 == K) cluster_off[K] = end;
            if (out_count) out_count[c] = end - begin;
            v[e] = km_segments_of(end - begin);
        }
    }
    int32_t total;
    int32_t ex = km_block_scan(v, wsum, &total);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int c = threadIdx.x * 4 + e;
        if (c < K) seg_off[c] = ex;
        ex += v[e];
    }
    if (threadIdx.x == 0) seg_off[K] = total;
}

// order[offset[c][b] + members of c in the block's earlier tiles + rank in the tile] = r (dynamic LDS: K running positions)
__global__ __launch_bounds__(KM_TILE) void k_km_place(const KmOrderParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int32_t* const run = reinterpret_cast<int32_t*>(smem);
    __shared__ int32_t tile_label[KM_TILE];
    const int64_t b = blockIdx.x, begin = b * p.span, end = begin + p.span < p.rows ? begin + p.span : p.rows;
    for (int c = threadIdx.x; c < p.n_clusters; c += KM_TILE) run[c] = p.hist[km_hist_index(c, b, p.n_blocks)];
    for (int64_t t0 = begin; t0 < end; t0 += KM_TILE) {
        const int n = (int)(end - t0 < KM_TILE ? end - t0 : KM_TILE);
        const int t = threadIdx.x;
        const int32_t l = km_label_of(p, t0 + t, end);
        __syncthreads();   // run[] is set / moved on, the tile before has been read
        tile_label[t] = l;
        __syncthreads();
        bool last = false;
        int rank = 0;
        if (l >= 0) {
            rank = km_tile_rank(tile_label, t, n, &last);
            const int64_t pos = (int64_t)run[l] + rank;
            if (pos >= 0 && pos < p.rows) p.order[pos] = (int32_t)(t0 + t);
        }
        __syncthreads();   // every position of the tile is computed
        if (l >= 0 && last) run[l] += rank + 1;   // one writer per label
    }
}

// ---- the ordered per-cluster sum and the new centroids -----------------------------------------------------------------------------
struct KmSumParams {
    MasterView master; int dim; int n_clusters;
    const int32_t* seg_off; const int32_t* cluster_off; const int32_t* order;
    double* segsum;    // [segments][dim]
    float* centroid;   // [K][dim]
};

// one workgroup per segment: a thread owns float4 columns and adds the segment's members in order, from +0.0
__global__ __launch_bounds__(256) void k_km_segment_sums(const KmSumParams p) {
    const int32_t s = (int32_t)blockIdx.x;
    if (s >= p.seg_off[p.n_clusters]) return;
    const KmSegment seg = km_segment(p.seg_off, p.cluster_off, p.n_clusters, s);
    const int n4 = p.dim >> 2;
    for (int g = threadIdx.x; g < n4; g += blockDim.x) {
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        for (int32_t m = 0; m < seg.length; ++m) {
            const float4 v = master_row(p.master, p.order[seg.first + m], p.dim)[g];
            a0 += (double)v.x, a1 += (double)v.y, a2 += (double)v.z, a3 += (double)v.w;
        }
        double* d = p.segsum + ((size_t)s * n4 + g) * 4;
        d[0] = a0, d[1] = a1, d[2] = a2, d[3] = a3;
    }
}

// one wave per cluster: the segments' totals added in segment order from +0.0, rounded to fp32, then K1 in k_normalize's arithmetic
// (the norm's lane-order fp64 sum — lane l takes groups l, l + 64, ..., x, y, z, w — wave_sum, sqrt, the 1e-12 floor, one division
// per element: k_normalize is a kernel that writes every row it is given, so its arithmetic is restated here for the rows that
// change). A cluster without members keeps its centroid.
__global__ __launch_bounds__(64) void k_km_finish(const KmSumParams p) {
    const int c = blockIdx.x, lane = threadIdx.x;
    const int32_t s0 = p.seg_off[c], s1 = p.seg_off[c + 1];
    if (s0 == s1) return;
    const int n4 = p.dim >> 2;
    float4* const dst = reinterpret_cast<float4*>(p.centroid + (int64_t)c * p.dim);
    double acc = 0.0;
    for (int g = lane; g < n4; g += 64) {
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        for (int32_t s = s0; s < s1; ++s) {
            const double* d = p.segsum + ((size_t)s * n4 + g) * 4;
            a0 += d[0], a1 += d[1], a2 += d[2], a3 += d[3];
        }
        const float4 y = make_float4((float)a0, (float)a1, (float)a2, (float)a3);
        dst[g] = y;
        acc += (double)y.x * (double)y.x;
        acc += (double)y.y * (double)y.y;
        acc += (double)y.z * (double)y.z;
        acc += (double)y.w * (double)y.w;
    }
    double den = sqrt(wave_sum(acc));
    if (den < 1e-12) den = 1e-12;
    for (int g = lane; g < n4; g += 64) {   // (a lane reads back what it wrote itself)
        const float4 v = dst[g];
        dst[g] = make_float4((float)((double)v.x / den), (float)((double)v.y / den), (float)((double)v.z / den), (float)((double)v.w / den));
    }
}

}  // namespace rdx
