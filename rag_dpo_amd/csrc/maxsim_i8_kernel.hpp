// maxsim_i8_kernel.hpp — late-interaction scoring over per-token symmetric int8 token vectors (the model is
// rag_dpo_amd/late_interaction.py quantize_model / maxsim_i8_model). Included by rdx_maxsim.hip only.
//
//     a = max_k |x_k|, scale = (float)((double)a / 127.0), c_k = clamp(rint((double)x_k / (double)scale), -127, 127)
//     score(q, d) = (float)((sum_i (double)sq_i * (double)max_j ((float)(cq_i . cd_j) * sd_j)) / n_q)
//
// Every step is either exact (the int32 dot product, the conversion of |acc| < 2^24 to fp32, the maximum, the fp64 products) or one
// IEEE operation on operands the model has too, so the kernels give the model's bits.
//
// k_maxsim_quant: one wave per token row, four rows per workgroup. Lane l holds the 8-half pieces l and l + 64 of the row (dim <=
//   1024: at most 16 halfs per lane). max |x| is a wave butterfly (exact: a maximum of fp16 values); a row that holds a non-finite
//   value, or only zeros, gets codes 0 and scale +0.0. The divisions are fp64 (the idiom of k_normalize: the result does not depend on
//   how an fp32 division is compiled), rint is v_rndne_f64: ties to even. A piece's 8 codes leave as one 8-byte vector store, the
//   scale as one fp32 store by lane 0. No atomics, no LDS.
//
// k_maxsim_i8: k_maxsim's structure (maxsim_kernel.hpp), its bounds and its masking: one workgroup of four waves per pair.
//   Questions. Up to 64 question tokens' codes are staged in LDS (rows of dim bytes + 16: the pad puts the 16 rows a ds_read_b128 lane
//     group reads into 16 different 16-byte bank slots), rows past n_q are zero; a block of at most 32 tokens skips the second column
//     block's MFMAs. The question scales of the whole question go to LDS once.
//   Documents. The waves split the slot's 32-token tiles. A tile is the A operand of v_mfma_i32_32x32x32_i8 straight from global
//     memory: lane (r = l & 31, h = l >> 5) reads the 16 contiguous bytes k = 32 m + 16 h + 0..15 of document row r per 32-dimension
//     step (one global_load_dwordx4), the B operand is the same 16 bytes of question row r from LDS: both operands agree on k whatever
//     the instruction's own k map is, and integer addition makes the order irrelevant. ONE MFMA per 32 dimensions. Steps are loaded
//     eight at a time, two blocks in flight: the bytes in flight per lane of k_maxsim (2 x 128).
//     A row index past the slot is clamped to the slot's last row for the load, of codes and of scale, AND masked out of the maximum.
//   Maximum. D register i of a lane is document token base + (i & 3) + 8 (i >> 2) + 4 h, question token r: v = (float)acc * sd[token],
//     one fp32 multiply; the running maximum starts at -inf; the lane halves meet in one shuffle, the four waves in LDS.
//   Sum. Thread 0 adds sq_i * m_i in fp64 in token order from +0.0, divides by n_q and rounds once to fp32.
// A pair out of range gets NaN and reads nothing, exactly as in k_maxsim. No atomics; a pair's bits depend on its own question and
// slot only.
#pragma once
#include "maxsim_kernel.hpp"

namespace rdx {

constexpr int MAXSIM_QUANT_WAVES = 4;         // token rows per workgroup of k_maxsim_quant
constexpr int MAXSIM_I8_PF = 8;               // 32-dimension steps (16 bytes per lane each) per load block

typedef int8_t char8 __attribute__((ext_vector_type(8)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

// bytes of one staged question row of codes
__host__ __device__ inline int maxsim_i8_row_bytes(int dim) { return dim + 16; }
// dynamic LDS of a launch that stages q_rows (32 or 64) question rows: the rows | red [4][64] fp32 | mtok [256] fp32 | sq [256] fp32
__host__ __device__ inline size_t maxsim_i8_lds_bytes(int dim, int q_rows) {
    return (size_t)q_rows * maxsim_i8_row_bytes(dim) + 4 * MAXSIM_Q_BLOCK * 4 + 2 * MAXSIM_MAX_Q_TOKENS * 4;
}

__global__ __launch_bounds__(64 * MAXSIM_QUANT_WAVES) void k_maxsim_quant(const _Float16* __restrict__ vecs, int64_t rows, int dim,
                                                                          int8_t* __restrict__ codes, float* __restrict__ scales) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * MAXSIM_QUANT_WAVES + (threadIdx.x >> 6);
    if (row >= rows) return;   // (no barrier below)
    const int pieces = dim >> 3;
    const half8* src = reinterpret_cast<const half8*>(vecs + row * dim);
    half8 x[2];
    float a = 0.f;
    bool bad = false;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int p = lane + 64 * s;
        x[s] = half8{0, 0, 0, 0, 0, 0, 0, 0};
        if (p < pieces) x[s] = src[p];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float v = fabsf((float)x[s][k]);
            bad |= !(v <= 65504.f);           // NaN or Inf
            a = fmaxf(a, v);                  // (fmaxf drops a NaN: `bad` keeps it)
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        a = fmaxf(a, __shfl_xor(a, o, 64));
        bad |= (bool)__shfl_xor((int)bad, o, 64);
    }
    const bool zero = bad || a == 0.f;
    const float scale = zero ? 0.f : (float)((double)a / 127.0);
    const double ds = (double)scale;
    char8* dst = reinterpret_cast<char8*>(codes + row * dim);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int p = lane + 64 * s;
        if (p >= pieces) continue;
        char8 c = {0, 0, 0, 0, 0, 0, 0, 0};
        if (!zero) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                double t = rint((double)x[s][k] / ds);
                t = fmin(fmax(t, -127.0), 127.0);
                c[k] = (int8_t)(int)t;
            }
        }
        dst[p] = c;
    }
    if (lane == 0) scales[row] = scale;
}

__global__ __launch_bounds__(MAXSIM_THREADS) void k_maxsim_i8(const int8_t* __restrict__ q_codes, const float* __restrict__ q_scales,
                                                              const int32_t* __restrict__ q_off, int nq, const int8_t* __restrict__ d_codes,
                                                              const float* __restrict__ d_scales, int64_t d_rows,
                                                              const int64_t* __restrict__ slot_start, const int32_t* __restrict__ slot_len,
                                                              int64_t n_slots, const int32_t* __restrict__ pair_q,
                                                              const int64_t* __restrict__ pair_slot, int dim, int q_rows,
                                                              float* __restrict__ scores) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int64_t pair = blockIdx.x;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int row_bytes = maxsim_i8_row_bytes(dim);
    float* red = reinterpret_cast<float*>(smem + (size_t)q_rows * row_bytes);   // [4][64]
    float* mtok = red + 4 * MAXSIM_Q_BLOCK;                                      // [256]
    float* sq = mtok + MAXSIM_MAX_Q_TOKENS;                                      // [256]

    // the pair's question and slot; anything out of range: NaN, nothing read (uniform over the workgroup)
    const int qi = pair_q[pair];
    const int64_t si = pair_slot[pair];
    bool ok = qi >= 0 && qi < nq && si >= 0 && si < n_slots;
    int q0 = 0, n_q = 0, len = 0;
    int64_t start = 0;
    if (ok) {
        q0 = q_off[qi];
        n_q = q_off[qi + 1] - q0;
        start = slot_start[si];
        len = slot_len[si];
        ok = len >= 1 && len <= MAXSIM_MAX_SLOT_TOKENS && start >= 0 && start <= d_rows - len &&
             q0 >= 0 && n_q >= 1 && n_q <= MAXSIM_MAX_Q_TOKENS && (n_q <= 32 || q_rows == MAXSIM_Q_BLOCK);   // (what the host checked before the launch)
    }
    if (!ok) {
        if (tid == 0) scores[pair] = __builtin_nanf("");
        return;
    }
    const int steps = dim >> 5;                      // 32-dimension steps
    const int tiles = (len + 31) >> 5;
    const int8_t* slot = d_codes + start * dim;
    const float* slot_scale = d_scales + start;
    const float NEG_INF = -__builtin_inff();
    if (tid < n_q) sq[tid] = q_scales[q0 + tid];     // (read by thread 0 behind the barriers below)

    for (int qb = 0; qb < n_q; qb += MAXSIM_Q_BLOCK) {
        const int nb = min(MAXSIM_Q_BLOCK, n_q - qb);    // question tokens of this block
        const bool two = nb > 32;                        // (then q_rows is 64: the launch sized the LDS for the longest question)
        // stage the block: 16-byte pieces, rows past the question zero
        const int pieces = dim >> 4, rows = two ? 64 : 32;
        for (int i = tid; i < rows * pieces; i += MAXSIM_THREADS) {
            const int row = i / pieces, c = i - row * pieces;
            i32x4 v = {0, 0, 0, 0};
            if (row < nb) v = *reinterpret_cast<const i32x4*>(q_codes + (int64_t)(q0 + qb + row) * dim + c * 16);
            *reinterpret_cast<i32x4*>(smem + row * row_bytes + c * 16) = v;
        }
        __syncthreads();

        float best0 = NEG_INF, best1 = NEG_INF;
        const unsigned char* qrow0 = smem + r * row_bytes + h * 16;          // this lane's question row, column block 0
        const unsigned char* qrow1 = qrow0 + 32 * row_bytes;                  // column block 1
        for (int t = wave; t < tiles; t += 4) {
            const int base = t << 5;
            const int8_t* arow = slot + (int64_t)min(base + r, len - 1) * dim + h * 16;
            // the scales of this lane's 16 document tokens (clamped like the rows; a clamped token is masked below)
            float sd[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) sd[i] = slot_scale[min(base + (i & 3) + 8 * (i >> 2) + 4 * h, len - 1)];
            i32x16 acc0, acc1;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc0[i] = 0, acc1[i] = 0;
            i32x4 fa[MAXSIM_I8_PF], fb[MAXSIM_I8_PF];
            const auto load_block = [&](i32x4(&f)[MAXSIM_I8_PF], int m0) {
#pragma unroll
                for (int i = 0; i < MAXSIM_I8_PF; ++i)
                    if (m0 + i < steps) f[i] = *reinterpret_cast<const i32x4*>(arow + (m0 + i) * 32);
            };
            const auto mma_block = [&](const i32x4(&f)[MAXSIM_I8_PF], int m0) {
#pragma unroll
                for (int i = 0; i < MAXSIM_I8_PF; ++i)
                    if (m0 + i < steps) {
                        acc0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(f[i], *reinterpret_cast<const i32x4*>(qrow0 + (m0 + i) * 32), acc0, 0, 0, 0);
                        if (two)
                            acc1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(f[i], *reinterpret_cast<const i32x4*>(qrow1 + (m0 + i) * 32), acc1, 0, 0, 0);
                    }
            };
            load_block(fa, 0);
            for (int m0 = 0; m0 < steps; m0 += 2 * MAXSIM_I8_PF) {
                load_block(fb, m0 + MAXSIM_I8_PF);
                mma_block(fa, m0);
                load_block(fa, m0 + 2 * MAXSIM_I8_PF);
                mma_block(fb, m0 + MAXSIM_I8_PF);
            }
            // D register i of this lane is document token base + (i & 3) + 8 (i >> 2) + 4 h, question token r of the column block
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                if (base + (i & 3) + 8 * (i >> 2) + 4 * h < len) {
                    best0 = fmaxf(best0, (float)acc0[i] * sd[i]);
                    if (two) best1 = fmaxf(best1, (float)acc1[i] * sd[i]);
                }
            }
        }
        best0 = fmaxf(best0, __shfl_xor(best0, 32, 64));
        best1 = fmaxf(best1, __shfl_xor(best1, 32, 64));
        if (h == 0) {
            red[wave * MAXSIM_Q_BLOCK + r] = best0;
            red[wave * MAXSIM_Q_BLOCK + 32 + r] = best1;
        }
        __syncthreads();                                  // (every wave is also done with the staged rows)
        if (tid < nb)
            mtok[qb + tid] = fmaxf(fmaxf(red[tid], red[MAXSIM_Q_BLOCK + tid]), fmaxf(red[2 * MAXSIM_Q_BLOCK + tid], red[3 * MAXSIM_Q_BLOCK + tid]));
        __syncthreads();
    }
    if (tid == 0) {
        double acc = 0.0;
        for (int i = 0; i < n_q; ++i) acc += (double)sq[i] * (double)mtok[i];
        scores[pair] = (float)(acc / (double)n_q);
    }
}

}  // namespace rdx
