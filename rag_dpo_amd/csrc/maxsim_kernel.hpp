// maxsim_kernel.hpp — late-interaction (ColBERT-style) scoring of (question, chunk) pairs over fp16 token vectors (DESIGN.md §29;
// the model is rag_dpo_amd/late_interaction.py maxsim_model):
//
//     score(q, d) = (1 / n_q) * sum_i max_j q_i . d_j
//
// k_maxsim: one workgroup of four waves per pair.
//   Questions. Up to 64 question tokens are staged once in LDS (rows of dim halfs + 16 bytes: the pad puts the 16 rows a
//     ds_read_b128 lane group reads into 16 different 16-byte bank slots, whatever multiple of 32 dim is); a question of more tokens
//     runs the whole loop again per 64. Rows past n_q are zero rows whose column maxima nobody reads. The launch sizes the LDS for the
//     call's longest question (32 or 64 rows); a block of at most 32 tokens skips the second column block's MFMAs.
//   Documents. The waves split the slot's 32-token tiles (wave w takes tiles w, w + 4, ...). A tile is the A operand of
//     v_mfma_f32_32x32x16_f16 taken straight from global memory: lane (r = l & 31, h = l >> 5) reads 32 contiguous bytes of document
//     row r per 32-dimension step (k = 32 m + 16 h + 0..15; its two MFMAs take the halves 8 s + 0..7, s = 0, 1) and the B operand is
//     the same 16 bytes of question row r from LDS, so both operands agree on k whatever the instruction's own k map is, and the k
//     order of the fp32 accumulation is fixed: m ascending, s ascending. Steps are loaded four at a time, two blocks in flight.
//     A row index past the slot is clamped to the slot's last row (no load leaves the slot, and a slot may end at the arena's last
//     row) AND its similarities are masked out of the maximum: a padded row never takes part.
//   Maximum. D has the question token on the lane (column) and the document token in the 16 registers (row (reg & 3) + 8 (reg >> 2)
//     + 4 h): each lane keeps one running maximum per column block, started at -inf; the two lane halves meet in one shuffle, the
//     four waves in LDS. Max is order-free: the bits do not depend on which wave saw which tile.
//   Sum. Thread 0 adds the n_q maxima in fp64 in token order, divides by n_q and rounds once to fp32.
// A pair whose question or slot index is out of range, or whose slot does not lie in [0, d_rows) with 1..MAXSIM_MAX_SLOT_TOKENS rows,
// gets NaN and reads nothing. No atomics; a pair's bits depend on its own question and slot only.
#pragma once
#include "rdx_common.hpp"

namespace rdx {

constexpr int MAXSIM_THREADS = 256;
constexpr int MAXSIM_Q_BLOCK = 64;            // question tokens staged in LDS at a time
constexpr int MAXSIM_MAX_Q_TOKENS = 256;
constexpr int MAXSIM_MAX_SLOT_TOKENS = 8192;
constexpr int MAXSIM_MAX_DIM = 1024;
constexpr int MAXSIM_MAX_PAIRS = 1 << 20;
constexpr int MAXSIM_MAX_QUESTIONS = 65535;
constexpr int MAXSIM_PF = 4;                  // 32-dimension steps per load block

// bytes of one staged question row
__host__ __device__ inline int maxsim_row_bytes(int dim) { return dim * 2 + 16; }
// dynamic LDS of a launch that stages q_rows (32 or 64) question rows: the rows | red [4][64] fp32 | mtok [256] fp32
__host__ __device__ inline size_t maxsim_lds_bytes(int dim, int q_rows) {
    return (size_t)q_rows * maxsim_row_bytes(dim) + 4 * MAXSIM_Q_BLOCK * 4 + MAXSIM_MAX_Q_TOKENS * 4;
}

__global__ __launch_bounds__(MAXSIM_THREADS) void k_maxsim(const _Float16* __restrict__ q_vecs, const int32_t* __restrict__ q_off, int nq,
                                                           const _Float16* __restrict__ d_vecs, int64_t d_rows,
                                                           const int64_t* __restrict__ slot_start, const int32_t* __restrict__ slot_len,
                                                           int64_t n_slots, const int32_t* __restrict__ pair_q,
                                                           const int64_t* __restrict__ pair_slot, int dim, int q_rows,
                                                           float* __restrict__ scores) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int64_t pair = blockIdx.x;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int row_bytes = maxsim_row_bytes(dim);
    float* red = reinterpret_cast<float*>(smem + (size_t)q_rows * row_bytes);   // [4][64]
    float* mtok = red + 4 * MAXSIM_Q_BLOCK;                                      // [256]

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
    const _Float16* slot = d_vecs + start * dim;
    const float NEG_INF = -__builtin_inff();

    for (int qb = 0; qb < n_q; qb += MAXSIM_Q_BLOCK) {
        const int nb = min(MAXSIM_Q_BLOCK, n_q - qb);    // question tokens of this block
        const bool two = nb > 32;                        // (then q_rows is 64: the launch sized the LDS for the longest question)
        // stage the block: 16-byte pieces, rows past the question zero
        const int pieces = dim >> 3, rows = two ? 64 : 32;
        for (int i = tid; i < rows * pieces; i += MAXSIM_THREADS) {
            const int row = i / pieces, c = i - row * pieces;
            half8 v = {0, 0, 0, 0, 0, 0, 0, 0};
            if (row < nb) v = *reinterpret_cast<const half8*>(q_vecs + (int64_t)(q0 + qb + row) * dim + c * 8);
            *reinterpret_cast<half8*>(smem + row * row_bytes + c * 16) = v;
        }
        __syncthreads();

        float best0 = NEG_INF, best1 = NEG_INF;
        const unsigned char* qrow0 = smem + r * row_bytes + h * 32;          // this lane's question row, column block 0
        const unsigned char* qrow1 = qrow0 + 32 * row_bytes;                  // column block 1
        for (int t = wave; t < tiles; t += 4) {
            const int base = t << 5;
            const _Float16* arow = slot + (int64_t)min(base + r, len - 1) * dim + h * 16;
            f32x16 acc0, acc1;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc0[i] = 0.f, acc1[i] = 0.f;
            half8 fa[MAXSIM_PF][2], fb[MAXSIM_PF][2];
            const auto load_block = [&](half8(&f)[MAXSIM_PF][2], int m0) {
#pragma unroll
                for (int i = 0; i < MAXSIM_PF; ++i)
                    if (m0 + i < steps) {
                        const half8* p = reinterpret_cast<const half8*>(arow + (m0 + i) * 32);
                        f[i][0] = p[0];
                        f[i][1] = p[1];
                    }
            };
            const auto mma_block = [&](const half8(&f)[MAXSIM_PF][2], int m0) {
#pragma unroll
                for (int i = 0; i < MAXSIM_PF; ++i)
                    if (m0 + i < steps) {
                        const half8* b0 = reinterpret_cast<const half8*>(qrow0 + (m0 + i) * 64);
                        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(f[i][0], b0[0], acc0, 0, 0, 0);
                        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(f[i][1], b0[1], acc0, 0, 0, 0);
                        if (two) {
                            const half8* b1 = reinterpret_cast<const half8*>(qrow1 + (m0 + i) * 64);
                            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(f[i][0], b1[0], acc1, 0, 0, 0);
                            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(f[i][1], b1[1], acc1, 0, 0, 0);
                        }
                    }
            };
            load_block(fa, 0);
            for (int m0 = 0; m0 < steps; m0 += 2 * MAXSIM_PF) {
                load_block(fb, m0 + MAXSIM_PF);
                mma_block(fa, m0);
                load_block(fa, m0 + 2 * MAXSIM_PF);
                mma_block(fb, m0 + MAXSIM_PF);
            }
            // D register i of this lane is document token base + (i & 3) + 8 (i >> 2) + 4 h, question token r of the column block
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                if (base + (i & 3) + 8 * (i >> 2) + 4 * h < len) {
                    best0 = fmaxf(best0, acc0[i]);
                    if (two) best1 = fmaxf(best1, acc1[i]);
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
        for (int i = 0; i < n_q; ++i) acc += (double)mtok[i];
        scores[pair] = (float)(acc / (double)n_q);
    }
}

}  // namespace rdx
