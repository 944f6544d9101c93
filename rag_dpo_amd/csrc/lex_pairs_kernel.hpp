// lex_pairs_kernel.hpp — the lexical score of NAMED (question, row) pairs over an index of BGE-M3 lexical weights (gfx950; include/rdx.h
// rdx_lex_score_pairs). Included by rdx_bm25.hip only, behind bm25_kernel.hpp (BM25_TILE, lex_half_bits).
//
// One wave per pair, four pairs per workgroup, no barrier and no LDS. The wave walks the question's terms 64 at a time in ascending
// position: lane l looks its term's postings up for the pair's row (lex_find, over the term's tile directory first when the term's
// postings span more than one tile of BM25_TILE rows, then over the postings of that tile) and forms the exact fp64 product of the
// two fp16 weights. The products of the lanes that found the row are then added by every lane alike, in ascending lane order, to a
// sum that started at +0.0. A term the row lacks would add +0.0 to a sum that is never negative: it changes no bit and is skipped.
// The additions are those of k_lex_score for that row, in its order (ascending term id), so the bits are rdx_lex_search's and
// rag_dpo_amd/lexical.py score_model's.
//
// A question is checked by every pair that names it, as it is walked: an id outside [0, n_terms), ids not strictly ascending, or
// weight bits outside [0x0001, 0x7BFF] make the pair's score NaN; no posting is read through such a term.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lex_find.hpp"

namespace rdx {

constexpr int LEX_PAIRS_WAVES = 4;             // pairs per workgroup
constexpr int LEX_PAIRS_MAX_TERMS = 4096;      // per question, as rdx_lex_search
constexpr int64_t LEX_PAIRS_MAX_PAIRS = (int64_t)1 << 20;
constexpr int64_t LEX_PAIRS_MAX_QUESTIONS = 65535;

struct LexPairsParams {
    const int64_t* post_off; const int32_t* post_row; const uint16_t* post_w;      // the index (bm25_kernel.hpp)
    const int64_t* dir_off; const int32_t* dir_tile; const int64_t* dir_pos;
    int64_t n_rows, n_terms;
    const int64_t* q_off; const int32_t* q_terms; const uint16_t* q_w; int64_t nq;   // the questions' terms; q_off as the host checked it
    const int32_t* pair_q; const int64_t* pair_row; int64_t n_pairs;
    double* out;                                                                     // [n_pairs]
};

// the position of row r among term t's postings, or -1
__device__ __forceinline__ int64_t lex_posting_of(const LexPairsParams& p, int32_t t, int32_t r) {
    int64_t b = p.post_off[t], e = p.post_off[t + 1];
    const int64_t db = p.dir_off[t], de = p.dir_off[t + 1];
    if (de - db > 1) {   // the postings span several tiles: the row's tile first
        const int64_t at = lex_find(p.dir_tile + db, de - db, r / BM25_TILE);
        if (at < 0) return -1;
        b = p.dir_pos[db + at];
        e = p.dir_pos[db + at + 1];   // (dir_pos has an entry behind the last: nnz)
    }
    const int64_t pos = lex_find(p.post_row + b, e - b, r);
    return pos < 0 ? -1 : b + pos;
}

// Grid: ceil(n_pairs / LEX_PAIRS_WAVES) workgroups of 64 * LEX_PAIRS_WAVES threads.
__global__ __launch_bounds__(64 * LEX_PAIRS_WAVES) void k_lex_score_pairs(const LexPairsParams p) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int64_t pair = (int64_t)blockIdx.x * LEX_PAIRS_WAVES + (threadIdx.x >> 6);
    if (pair >= p.n_pairs) return;   // (no barrier below)
    const int64_t q = p.pair_q[pair], r = p.pair_row[pair];
    if (q < 0 || q >= p.nq || r < 0 || r >= p.n_rows) {   // nothing is read through such a pair
        if (lane == 0) p.out[pair] = __builtin_nan("");
        return;
    }
    const int64_t b = p.q_off[q], e = p.q_off[q + 1];
    double s = 0.0;
    bool bad = false;
    for (int64_t c0 = b; c0 < e; c0 += 64) {
        const int64_t i = c0 + lane;
        double x = 0.0;
        bool have = false, mine_bad = false;
        if (i < e) {
            const int32_t t = p.q_terms[i];
            const uint16_t wb = p.q_w[i];
            mine_bad = t < 0 || t >= p.n_terms || wb < 1 || wb > 0x7BFF || (i > b && p.q_terms[i - 1] >= t);
            if (!mine_bad) {
                const int64_t at = lex_posting_of(p, t, (int32_t)r);
                if (at >= 0) {
                    x = lex_half_bits(wb) * lex_half_bits(p.post_w[at]);
                    have = true;
                }
            }
        }
        if (__ballot(mine_bad)) {   // uniform
            bad = true;
            break;
        }
        unsigned long long live = __ballot(have);
        while (live) {   // ascending lane = ascending term id
            const int src = __ffsll((long long)live) - 1;
            live &= live - 1;
            s = s + __shfl(x, src, 64);
        }
    }
    if (lane == 0) p.out[pair] = bad ? __builtin_nan("") : s;
}

}  // namespace rdx
