// enc_gemm.hpp — E14 k_enc_gemm: out[T][N] = epi(x[T][K] W[N][K]^T + bias[N]) for ANY token count, the encoder's four projections of a
// batch (QKV, O, FFN-up, FFN-down) on the matrix cores with the epilogue the module applies next fused in.
//
//   operands   fp16; W in the checkpoint's own [N][K] layout, so both operands are K-contiguous and a 16-byte piece of a row is an MFMA
//              fragment as it stands. No second copy of the weights exists anywhere.
//   tile       BM tokens x BN features per workgroup of 4 waves (2 x 2), BK = 64 per k-step; a wave owns (BM/2) x (BN/2) as
//              MR x NR accumulators of v_mfma_f32_16x16x32_f16, fp32, summed in k order. Two shapes: 128 x 128 (ingest-size T) and
//              64 x 64 (a few hundred tokens still cover the CUs); enc_gemm_large() is the one place that chooses.
//   A = W      so that D[row = feature 4g + r][col = token l15]: a lane ends with FOUR CONSECUTIVE FEATURES of one token per
//              accumulator: bias, residual and output move as 8-byte pieces.
//   LDS image  one array, two stage buffers; a stage is BM rows of x then BN rows of W, 128 B (64 k) each, written by
//              global_load_lds at 16 B per lane: a wave instruction fills 8 rows linearly. ds_read_b128 of a fragment takes the same
//              16-byte column of 16 rows: 8-way conflicts on a linear image. The image is therefore XOR-swizzled — position p of row r
//              holds the row's 16-byte chunk p ^ ((r >> 1) & 7) — and, the LDS-DMA destination being lane-linear, the permutation
//              is applied to the per-lane SOURCE address and again to the read address (the same involution).
//   loop       the double-buffered form: top of step t: every wave waits for its own DMA of tile t (vmcnt(0)), barrier (tile t is
//              complete, and everyone has finished reading the other buffer in step t - 1), tile t + 1 is requested into the other
//              buffer, the MFMAs of tile t run under it. One barrier per k-step; two or more workgroups per CU overlap the rest.
//   ragged     the last row tile and (N a multiple of 64, not of BN) the last column tile CLAMP their source rows to T - 1 / N - 1:
//              nothing at or past row T of x or res is read, nothing at or past row T of out is written.
//   epilogue   0: half(acc + bias).  1: erf GELU of acc + bias in fp32 (E13's polynomial, enc_kernels.hpp), one rounding to fp16.
//              2: res + half(acc + bias) — the projection rounded to fp16, then an fp16 add: what the module computes
//              (rdx_enc_stage_f16's contract).
//   blocks     1-D grid, remapped so that the workgroups sharing an XCD (ids equal mod 8) hold a contiguous range of tiles (the
//              bijective form: the tile count need not divide by 8), and inside that range 8 row tiles walk together through the
//              column tiles: what an XCD's L2 holds at a time is 8 x panels and the W panels they meet.
// No split-K, no atomics: the same inputs give the same bits on every call and stream.
#pragma once
#include "enc_small.hpp"

namespace rdx {

constexpr int ENC_GEMM_BK = 64;
// the 128 x 128 tile from as many tiles as the chip has CUs (256); below, the 64 x 64 tile makes four times as many workgroups
constexpr int64_t ENC_GEMM_LARGE_MIN_TILES = 256;

// the launcher's only choice, a pure function of the shape
inline bool enc_gemm_large(int64_t T, int N, int K) {
    (void)K;
    return ((T + 127) / 128) * (((int64_t)N + 127) / 128) >= ENC_GEMM_LARGE_MIN_TILES;
}

struct EncGemm {
    const _Float16* x;      // [T][K]
    const _Float16* w;      // [N][K]
    const _Float16* bias;   // [N]
    const _Float16* res;    // EPI 2: [T][N]
    _Float16* out;          // [T][N]
    int64_t T;
    int N, K;
    int tiles_m, tiles_n;
};

template <int BM, int BN, int EPI>
__global__ __launch_bounds__(256) void k_enc_gemm(EncGemm a) {
    extern __shared__ __attribute__((aligned(16))) char gemm_smem[];   // [2 stages][BM + BN rows][128 B]
    constexpr int WM = BM / 2, WN = BN / 2, MR = WM / 16, NR = WN / 16;
    constexpr int ROWS = BM + BN, STAGE_BYTES = ROWS * 128;
    constexpr int NLD = ROWS / 32;                                     // LDS-DMA instructions per thread and stage (256 lanes x 16 B = 32 rows)
    static_assert(BM % 32 == 0 && BN % 32 == 0, "a wave instruction stages 8 whole rows of one operand");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l15 = lane & 15, g = lane >> 4;

    // XCD remap (bijective), then groups of 8 row tiles
    const unsigned nwg = gridDim.x, orig = blockIdx.x;
    const unsigned xq = nwg >> 3, xr = nwg & 7, xcd = orig & 7;
    const unsigned id = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + (orig >> 3);
    const unsigned per_group = 8u * (unsigned)a.tiles_n;
    const unsigned grp = id / per_group, in_grp = id - grp * per_group;
    const unsigned gm = min(8u, (unsigned)a.tiles_m - grp * 8u);
    const int tm = (int)(grp * 8u + in_grp % gm), tn = (int)(in_grp / gm);
    const int64_t m0 = (int64_t)tm * BM;
    const int n0 = tn * BN;
    const int K = a.K;

    // staging: instruction j covers stage rows j * 32 + wave * 8 + (lane >> 3); this lane fetches the chunk its position holds
    const _Float16* src[NLD];
#pragma unroll
    for (int j = 0; j < NLD; ++j) {
        const int rr = j * 32 + wave * 8 + (lane >> 3);
        const int chunk = (lane & 7) ^ ((rr >> 1) & 7);
        if (j < BM / 32) {
            const int64_t t = m0 + rr;
            src[j] = a.x + (t < a.T ? t : a.T - 1) * K + chunk * 8;
        } else {
            const int n = n0 + rr - BM;
            src[j] = a.w + (int64_t)(n < a.N ? n : a.N - 1) * K + chunk * 8;
        }
    }
    auto stage = [&](int kt, int buf) __attribute__((always_inline)) {
        char* dst = gemm_smem + buf * STAGE_BYTES + wave * 1024;
#pragma unroll
        for (int j = 0; j < NLD; ++j)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src[j] + (int64_t)kt * ENC_GEMM_BK),
                                             (__attribute__((address_space(3))) void*)(dst + j * 4096), 16, 0, 0);
    };

    // fragment reads: row (… + l15) of the image, chunk s * 4 + g of k-step s at position chunk ^ ((row >> 1) & 7); every row offset
    // added below is a multiple of 16 rows, so the swizzle term is the lane's own
    const int sw = (l15 >> 1) & 7;
    const int x_off = ((wave >> 1) * WM + l15) * 128;
    const int w_off = (BM + (wave & 1) * WN + l15) * 128;
    const int p0 = (g ^ sw) << 4, p1 = ((4 + g) ^ sw) << 4;

    f32x4 acc[MR][NR];
#pragma unroll
    for (int mi = 0; mi < MR; ++mi)
#pragma unroll
        for (int ni = 0; ni < NR; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nk = K / ENC_GEMM_BK;
    stage(0, 0);
    for (int kt = 0; kt < nk; ++kt) {
        __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): this wave's pieces of tile kt have landed
        __syncthreads();
        if (kt + 1 < nk) stage(kt + 1, (kt + 1) & 1);
        const char* img = gemm_smem + (kt & 1) * STAGE_BYTES;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int p = s ? p1 : p0;
            half8 fw[NR], fx[MR];
#pragma unroll
            for (int ni = 0; ni < NR; ++ni) fw[ni] = *reinterpret_cast<const half8*>(img + w_off + ni * 2048 + p);
#pragma unroll
            for (int mi = 0; mi < MR; ++mi) fx[mi] = *reinterpret_cast<const half8*>(img + x_off + mi * 2048 + p);
#pragma unroll
            for (int mi = 0; mi < MR; ++mi)
#pragma unroll
                for (int ni = 0; ni < NR; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fw[ni], fx[mi], acc[mi][ni], 0, 0, 0);
        }
    }

    // D[feature = 4g + r][token = l15]
    const int nb = n0 + (wave & 1) * WN + 4 * g;
    const int64_t tb = m0 + (wave >> 1) * WM + l15;
#pragma unroll
    for (int ni = 0; ni < NR; ++ni) {
        const int n = nb + ni * 16;
        if (n >= a.N) continue;                // (N is a multiple of 64: the four features are inside or outside together)
        const half4 bv = *reinterpret_cast<const half4*>(a.bias + n);
#pragma unroll
        for (int mi = 0; mi < MR; ++mi) {
            const int64_t t = tb + mi * 16;
            if (t >= a.T) continue;
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = acc[mi][ni][r] + (float)bv[r];
            half4 o;
            if constexpr (EPI == ENC_EPI_GELU) {
                const f32x2 g0 = gelu_poly2(f32x2{v[0], v[1]}), g1 = gelu_poly2(f32x2{v[2], v[3]});
                o = half4{(_Float16)g0[0], (_Float16)g0[1], (_Float16)g1[0], (_Float16)g1[1]};
            } else if constexpr (EPI == ENC_EPI_RESIDUAL) {
                const half4 rv = *reinterpret_cast<const half4*>(a.res + t * a.N + n);
#pragma unroll
                for (int r = 0; r < 4; ++r) o[r] = (_Float16)((float)(_Float16)v[r] + (float)rv[r]);
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) o[r] = (_Float16)v[r];
            }
            *reinterpret_cast<half4*>(a.out + t * a.N + n) = o;
        }
    }
}

}  // namespace rdx
