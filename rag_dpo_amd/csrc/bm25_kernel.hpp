// bm25_kernel.hpp — BM25 sparse scoring and top-k (gfx950). Serves the reference's ChunkBM25Index.search /
// SummaryBM25Index.search (src/rag/bm25_index.py:126-292), whose scores come from rank_bm25 0.2.2's BM25Okapi.get_scores.
//
// HBM layout of one index (owned by rdx_bm25, rdx_bm25.hip; built by rag_dpo_amd/bm25.py):
//   post_off  int64 [V+1]    CSR by term: term t's postings are [post_off[t], post_off[t+1])
//   post_row  int32 [nnz]    row ids, strictly ascending inside a term
//   post_tf   uint16 [nnz]   term frequency in that row (>= 1; the host refuses an index with a larger tf)
//   idf       f64 [V]        rank_bm25's idf, epsilon floor applied
//   denom     f64 [N]        k1 * ((1 - b) + (b * doc_len) / avgdl), numpy's operation order
//   dir_off   int64 [V+1]    term t's tile directory: entries [dir_off[t], dir_off[t+1])
//   dir_tile  int32 [ndir]   a tile (BM25_TILE rows) holding postings of the term, ascending
//   dir_pos   int64 [ndir+1] the entry's first posting; dir_pos[e+1] ends it (the next entry, of this term or the next one,
//                            starts where it ends; dir_pos[ndir] = nnz)
//   group     int32 [N]      interned document_path of the row (a doc_filter is a bitset over groups)
//
// Filters of one search: a table of n_filters bitsets over the groups, allow_words = (n_groups + 31) / 32 words each, and per query
// the row of the table it is filtered by, or -1 for no filter (query_filter). A search with one bitset for all its queries is a
// table of one row.
//
// Exactness: rank_bm25 adds, for each query token in query order (duplicates kept), the float64 vector
//   idf * ((tf * 2.5) / (tf + denom))
// to a zero score vector. A row without the token adds +-0.0, which changes nothing, so only postings are visited. Each
// product, sum and quotient below is one IEEE double operation in that order: contraction into FMAs is switched off
// (an FMA rounds once where numpy rounds twice), and f64 division is correctly rounded by default. Within one term no
// two postings share a row, so the accumulation needs no atomics; terms are separated by a barrier, which keeps the
// per-row order of additions = query order. The result is bit-identical to the numpy loop.
//
// The index of BGE-M3 lexical weights (rdx_lex, rdx_bm25.hip; rag_dpo_amd/lexical.py) has the same layout with
//   post_w    uint16 [nnz]   the fp16 bits of the term's weight in that row (finite, > 0)
// in place of post_tf, and neither idf nor denom: k_lex_score runs the same core with the LexWeights scorer, and k_bm25_merge serves both.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rdx {

constexpr int BM25_TILE = 4096;          // rows per doc tile = one k_bm25_score block: 32 KiB of f64 accumulators in LDS
constexpr int BM25_THREADS = 256;
constexpr int BM25_PER_THREAD = BM25_TILE / BM25_THREADS;
constexpr int BM25_TERM_CHUNK = 256;     // query terms looked up together (phase A); longer queries loop over chunks
constexpr int BM25_MAX_TERMS = 4096;     // per query
constexpr int BM25_MAX_K = 4096;
constexpr int BM25_MERGE_THREADS = 512;
constexpr int BM25_MERGE_CAP = 8192;     // merge buffer (entries): the k kept so far + at least 4096 new candidates

// result order: score descending, ties by ascending row
__device__ __forceinline__ bool bm25_before(double sa, int ra, double sb, int rb) {
    return sa > sb || (sa == sb && ra < rb);
}

// exclusive prefix sum of v over the block (NT threads, multiple of 64); *total = the sum. Ends with a barrier.
template <int NT>
__device__ __forceinline__ int bm25_block_scan(int v, int* s_wave, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    if (lane == 63) s_wave[wave] = x;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) {
        const int s = s_wave[w];
        before += w < wave ? s : 0;
        all += s;
    }
    __syncthreads();   // s_wave may be reused by the caller
    *total = all;
    return before + x - v;
}

// bitonic sort of (key, row)[0, n), n a power of two, into result order. All threads of the block call it; ends with a barrier.
template <int NT>
__device__ void bm25_block_sort(double* key, int32_t* row, int n) {
    for (int size = 2; size <= n; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = threadIdx.x; i < (n >> 1); i += NT) {
                const int lo = 2 * i - (i & (stride - 1));
                const int hi = lo + stride;
                const double a = key[lo], b = key[hi];
                const int32_t ra = row[lo], rb = row[hi];
                const bool swap = (lo & size) == 0 ? bm25_before(b, rb, a, ra) : bm25_before(a, ra, b, rb);
                if (swap) {
                    key[lo] = b;
                    key[hi] = a;
                    row[lo] = rb;
                    row[hi] = ra;
                }
            }
            __syncthreads();
        }
    }
}

__device__ __forceinline__ int bm25_pow2_at_least(int n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

// What a query term and a posting are worth: the two scorers that share bm25_score_core. `term(...)` is the factor of the query's term
// at position pos (an index into q_terms) with id t; `posting(...)` is the value of posting p, which lies in row r. The core adds
// term * posting to the row, one IEEE double product and one sum, in query order. The tables are the core's own (restrict) arguments,
// handed to the scorer: post_val is post_tf or post_w; idf and denom are BM25's, q_w the lexical search's (the others are null).
struct Bm25Okapi {   // rank_bm25: idf[t] * ((tf * 2.5) / (tf + denom[r]))
    static __device__ __forceinline__ double term(const double* idf, const uint16_t*, int64_t, int t) { return idf[t]; }
    static __device__ __forceinline__ double posting(const uint16_t* post_tf, const double* denom, int64_t p, int32_t r) {
#pragma clang fp contract(off)
        const double tf = (double)post_tf[p];
        return (tf * 2.5) / (tf + denom[r]);
    }
};

__device__ __forceinline__ double lex_half_bits(uint16_t bits) { return (double)__builtin_bit_cast(_Float16, bits); }

struct LexWeights {   // BGE-M3 lexical weights (rag_dpo_amd/lexical.py): float64(wq) * float64(wd), both fp16 bits, the product exact
    static __device__ __forceinline__ double term(const double*, const uint16_t* q_w, int64_t pos, int) { return lex_half_bits(q_w[pos]); }
    static __device__ __forceinline__ double posting(const uint16_t* post_w, const double*, int64_t p, int32_t) { return lex_half_bits(post_w[p]); }
};

// The scorer of one (doc tile, query of this chunk) block. Writes the tile's top-min(k, passing) rows, UNORDERED, to
// part_{score,row}[q][tile][0..count) and the count to part_count[q][tile]; rows are global. q_off and query_filter are the
// chunk's own: entry 0 belongs to the chunk's first query.
template <class Policy>
__device__ __forceinline__ void bm25_score_core(
    const int64_t* __restrict__ dir_off, const int32_t* __restrict__ dir_tile, const int64_t* __restrict__ dir_pos,
    const int32_t* __restrict__ post_row, const uint16_t* __restrict__ post_val, const double* __restrict__ idf,
    const double* __restrict__ denom, const int32_t* __restrict__ row_group, const uint32_t* __restrict__ filter_sets,
    int allow_words, const int32_t* __restrict__ query_filter, const int64_t* __restrict__ q_off, const int32_t* __restrict__ q_terms,
    const uint16_t* __restrict__ q_w, int64_t n_rows, int k, int n_tiles,
    double* __restrict__ part_score, int32_t* __restrict__ part_row, int32_t* __restrict__ part_count) {
#pragma clang fp contract(off)
    __shared__ double acc[BM25_TILE];          // per-row scores; after phase C's compaction: the candidates' scores
    __shared__ int32_t crow[BM25_TILE];        // the candidates' rows (phase C, when the tile has more than k)
    __shared__ int64_t t_beg[BM25_TERM_CHUNK];
    __shared__ int32_t t_len[BM25_TERM_CHUNK];
    __shared__ double t_idf[BM25_TERM_CHUNK];  // the terms' factors (Policy::term)
    __shared__ int s_wave[BM25_THREADS / 64];
    __shared__ int s_any;

    const int tile = blockIdx.x, q = blockIdx.y, tid = threadIdx.x;
    const int64_t base = (int64_t)tile * BM25_TILE;
    const int rows = (int)min((int64_t)BM25_TILE, n_rows - base);
    const size_t part = (size_t)q * n_tiles + tile;
    const int32_t filter = query_filter[q];   // uniform over the block
    const uint32_t* set = filter < 0 ? nullptr : filter_sets + (size_t)filter * allow_words;
    for (int i = tid; i < BM25_TILE; i += BM25_THREADS) acc[i] = 0.0;
    if (tid == 0) s_any = 0;

    const int64_t qb = q_off[q], qe = q_off[q + 1];
    for (int64_t c0 = qb; c0 < qe; c0 += BM25_TERM_CHUNK) {
        const int nt = (int)min((int64_t)BM25_TERM_CHUNK, qe - c0);
        __syncthreads();   // the previous chunk's phase B is done with t_*
        // phase A: each thread finds one term's posting sub-range inside this tile through the term's tile directory
        if (tid < nt) {
            const int t = q_terms[c0 + tid];
            const int64_t end = dir_off[t + 1];
            int64_t lo = dir_off[t], hi = end;
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (dir_tile[mid] < tile) lo = mid + 1;
                else hi = mid;
            }
            int64_t b = 0;
            int len = 0;
            if (lo < end && dir_tile[lo] == tile) {
                b = dir_pos[lo];
                len = (int)(dir_pos[lo + 1] - b);
                s_any = 1;
            }
            t_beg[tid] = b;
            t_len[tid] = len;
            t_idf[tid] = Policy::term(idf, q_w, c0 + tid, t);
        }
        __syncthreads();
        // phase B: terms in query order; a barrier after each term that touched the tile
        for (int j = 0; j < nt; ++j) {
            const int len = t_len[j];
            if (len == 0) continue;
            const int64_t b = t_beg[j];
            const double w = t_idf[j];
            for (int p = tid; p < len; p += BM25_THREADS) {
                const int32_t r = post_row[b + p];
                const double x = Policy::posting(post_val, denom, b + p, r);
                const int l = r - (int)base;
                acc[l] = acc[l] + w * x;
            }
            __syncthreads();
        }
    }
    __syncthreads();
    if (s_any == 0) {   // no posting of any query term in this tile
        if (tid == 0) part_count[part] = 0;
        return;
    }

    // phase C: score > 0 and the group filter, then the tile's top-k
    double v[BM25_PER_THREAD];
    uint32_t ok = 0;
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < BM25_PER_THREAD; ++j) {
        const int l = tid + j * BM25_THREADS;
        v[j] = l < rows ? acc[l] : 0.0;
        bool pass = v[j] > 0.0;
        if (pass && set != nullptr) {
            const int32_t g = row_group[base + l];
            pass = (set[g >> 5] >> (g & 31)) & 1u;
        }
        ok |= (uint32_t)pass << j;
        cnt += pass;
    }
    int total = 0;
    int off = bm25_block_scan<BM25_THREADS>(cnt, s_wave, &total);   // its barriers also end every read of acc above
    if (total <= k) {   // every candidate goes out
        double* ps = part_score + part * k;
        int32_t* pr = part_row + part * k;
#pragma unroll
        for (int j = 0; j < BM25_PER_THREAD; ++j) {
            if ((ok >> j) & 1u) {
                ps[off] = v[j];
                pr[off] = (int32_t)base + tid + j * BM25_THREADS;
                ++off;
            }
        }
        if (tid == 0) part_count[part] = total;
        return;
    }
#pragma unroll
    for (int j = 0; j < BM25_PER_THREAD; ++j) {
        if ((ok >> j) & 1u) {
            acc[off] = v[j];
            crow[off] = (int32_t)base + tid + j * BM25_THREADS;
            ++off;
        }
    }
    const int n = bm25_pow2_at_least(total);
    for (int i = total + tid; i < n; i += BM25_THREADS) {
        acc[i] = -__builtin_huge_val();
        crow[i] = INT32_MAX;
    }
    __syncthreads();
    bm25_block_sort<BM25_THREADS>(acc, crow, n);
    for (int i = tid; i < k; i += BM25_THREADS) {
        part_score[part * k + i] = acc[i];
        part_row[part * k + i] = crow[i];
    }
    if (tid == 0) part_count[part] = k;
}

// Grid (doc tile, query of this chunk): bm25_score_core with rank_bm25's scorer.
__global__ __launch_bounds__(BM25_THREADS) void k_bm25_score(
    const int64_t* __restrict__ dir_off, const int32_t* __restrict__ dir_tile, const int64_t* __restrict__ dir_pos,
    const int32_t* __restrict__ post_row, const uint16_t* __restrict__ post_tf, const double* __restrict__ idf,
    const double* __restrict__ denom, const int32_t* __restrict__ row_group, const uint32_t* __restrict__ filter_sets,
    int allow_words, const int32_t* __restrict__ query_filter, const int64_t* __restrict__ q_off, const int32_t* __restrict__ q_terms, int64_t n_rows, int k, int n_tiles,
    double* __restrict__ part_score, int32_t* __restrict__ part_row, int32_t* __restrict__ part_count) {
    bm25_score_core<Bm25Okapi>(dir_off, dir_tile, dir_pos, post_row, post_tf, idf, denom, row_group, filter_sets, allow_words, query_filter,
                               q_off, q_terms, nullptr, n_rows, k, n_tiles, part_score, part_row, part_count);
}

// The same grid and scheme for an index of lexical weights (rdx_lex_search): the term's factor is the question's weight q_w at that
// position, a posting is worth its stored weight. A term occurs at most once per row (rdx_lex_create checks it), so the per-term
// barrier keeps the additions of a row in the order of the question's terms, which rdx_lex_search requires to be ascending ids.
__global__ __launch_bounds__(BM25_THREADS) void k_lex_score(
    const int64_t* __restrict__ dir_off, const int32_t* __restrict__ dir_tile, const int64_t* __restrict__ dir_pos,
    const int32_t* __restrict__ post_row, const uint16_t* __restrict__ post_w, const int32_t* __restrict__ row_group,
    const uint32_t* __restrict__ filter_sets, int allow_words, const int32_t* __restrict__ query_filter, const int64_t* __restrict__ q_off,
    const int32_t* __restrict__ q_terms, const uint16_t* __restrict__ q_w, int64_t n_rows, int k, int n_tiles,
    double* __restrict__ part_score, int32_t* __restrict__ part_row, int32_t* __restrict__ part_count) {
    bm25_score_core<LexWeights>(dir_off, dir_tile, dir_pos, post_row, post_w, nullptr, nullptr, row_group, filter_sets, allow_words,
                                query_filter, q_off, q_terms, q_w, n_rows, k, n_tiles, part_score, part_row, part_count);
}

// One block per query: the global top-k of the tiles' partials in result order. Candidates stream through an LDS buffer;
// whenever it could overflow it is sorted and cut to k, and from then on only candidates that beat the k-th kept one enter.
// out_count = min(k, rows passing); the slots after it hold score 0 and row -1.
__global__ __launch_bounds__(BM25_MERGE_THREADS) void k_bm25_merge(const double* __restrict__ part_score,
                                                                   const int32_t* __restrict__ part_row,
                                                                   const int32_t* __restrict__ part_count, int n_tiles, int k,
                                                                   double* __restrict__ out_score, int64_t* __restrict__ out_row,
                                                                   int32_t* __restrict__ out_count) {
    constexpr int NT = BM25_MERGE_THREADS;
    __shared__ double key[BM25_MERGE_CAP];
    __shared__ int32_t row[BM25_MERGE_CAP];
    __shared__ int s_off[NT];
    __shared__ int s_wave[NT / 64];
    __shared__ int s_fill;
    const int q = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) s_fill = 0;
    bool have_tau = false;   // the buffer has been cut to k entries: (tau_s, tau_r) is the k-th
    double tau_s = 0.0;
    int32_t tau_r = 0;

    auto cut = [&](int fill) {   // sort the buffer and keep the best k (all threads)
        const int n = bm25_pow2_at_least(fill);
        for (int i = fill + tid; i < n; i += NT) {
            key[i] = -__builtin_huge_val();
            row[i] = INT32_MAX;
        }
        __syncthreads();
        bm25_block_sort<NT>(key, row, n);
        if (fill >= k) {
            have_tau = true;
            tau_s = key[k - 1];
            tau_r = row[k - 1];
        }
        __syncthreads();
        if (tid == 0) s_fill = min(fill, k);
        __syncthreads();
    };

    for (int t0 = 0; t0 < n_tiles; t0 += NT) {
        __syncthreads();
        const int t = t0 + tid;
        const int c = t < n_tiles ? part_count[(size_t)q * n_tiles + t] : 0;
        int total = 0;
        s_off[tid] = bm25_block_scan<NT>(c, s_wave, &total);
        __syncthreads();
        for (int b0 = 0; b0 < total; b0 += NT) {
            const int fill = s_fill;
            __syncthreads();   // every thread has read s_fill before anyone appends
            if (fill + NT > BM25_MERGE_CAP) cut(fill);
            const int j = b0 + tid;
            if (j < total) {
                int lo = 0, hi = NT - 1;   // the last tile whose offset is <= j (it has j - offset < its count)
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    if (s_off[mid] <= j) lo = mid;
                    else hi = mid - 1;
                }
                const size_t src = ((size_t)q * n_tiles + t0 + lo) * k + (j - s_off[lo]);
                const double s = part_score[src];
                const int32_t r = part_row[src];
                if (!have_tau || bm25_before(s, r, tau_s, tau_r)) {
                    const int pos = atomicAdd(&s_fill, 1);
                    key[pos] = s;
                    row[pos] = r;
                }
            }
            __syncthreads();
        }
    }
    __syncthreads();
    const int fill = s_fill;
    __syncthreads();
    cut(fill);
    const int m = min(fill, k);
    for (int i = tid; i < k; i += NT) {
        out_score[(size_t)q * k + i] = i < m ? key[i] : 0.0;
        out_row[(size_t)q * k + i] = i < m ? (int64_t)row[i] : -1;
    }
    if (tid == 0) out_count[q] = m;
}

}  // namespace rdx
