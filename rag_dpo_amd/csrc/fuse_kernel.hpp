// fuse_kernel.hpp — the step that joins the dense and the BM25 rankings of a question (gfx950): DenseRetriever._fuse
// (rag_dpo_amd/retriever.py, reference src/rag/retriever.py:226-300, :391-462) for a batch of questions, one workgroup per question,
// the whole working set in LDS. The Python method is the model, bit for bit; DESIGN.md §18 has the arithmetic contract.
//
// A question is up to FUSE_MAX_LISTS ranked lists in the order _fuse visits them (dense q0, BM25 q0, dense q1, ...), list l of
// question q at [q][l][0 .. list_stride) of keys / dense_dist / bm25_score. Wave w owns list w through the first two steps.
//   1. filter: a dense list of a filtered question becomes its allowed entries in order, topped up with its first refused entries
//      to min_semantic (one ballot per 64 entries, kept in LDS; the list's length follows from the popcounts)
//   2. sequence: the filtered lists are laid end to end in LDS — position p = (list, rank in the filtered list); thread p owns it
//   3. first appearance: thread p walks back to the nearest earlier position with its key and links itself behind it; a position
//      with none is a head (= one entry of _fuse's chunk_map, in insertion order: the heads' prefix count)
//   4. a head walks its chain in sequence order and replays _fuse's updates: min distance (fp32), max semantic, BM25 score, RRF sum
//   5. rank of a head = #{heads before it in Python's stable sort(reverse=True)}; ranks below top_n are written
// Nothing depends on the schedule: no atomics, every value is computed by one thread in one order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rdx {

constexpr int FUSE_MAX_LISTS = 16;           // = include/rdx.h RDX_FUSE_MAX_LISTS (one wave per list)
constexpr int FUSE_MAX_LIST_ENTRIES = 512;   // = RDX_FUSE_MAX_LIST_ENTRIES
constexpr int FUSE_MAX_ENTRIES = 1024;       // = RDX_FUSE_MAX_ENTRIES (one thread per entry)
constexpr int FUSE_THREADS = FUSE_MAX_ENTRIES;
constexpr int FUSE_DENSE = 0, FUSE_BM25 = 1;
constexpr int FUSE_CHUNKS = FUSE_MAX_LIST_ENTRIES / 64;
static_assert(FUSE_THREADS == FUSE_MAX_LISTS * 64, "one wave per list");

struct FuseArgs {
    int n_lists, list_stride;
    const int32_t* list_kind;
    const double* list_weight;
    const int32_t* list_count;
    const int64_t* keys;
    const float* dense_dist;
    const double* bm25_score;
    const int32_t* row_group;
    int64_t n_rows;
    const int32_t* filter_on;
    const uint32_t* allow_groups;
    int group_words;
    int min_semantic, bm25_keep_max, rrf_k, top_n;
    int64_t* out_key;
    float* out_distance;
    double* out_semantic;
    double* out_bm25;
    double* out_hybrid;
    int32_t* out_list;
    int32_t* out_rank;
    int32_t* out_count;
};

// strict "a sorts before b" of Python's stable sort(reverse=True) for the hybrid scores of two DIFFERENT heads, a inserted before b
// when a_first: descending, ties (+0.0 == -0.0 included) in insertion order; a NaN after every number (rdx_rerank_select's rule)
__device__ __forceinline__ bool fuse_before(double a, double b, bool a_first) {
    const bool na = a != a, nb = b != b;
    if (na || nb) return nb && (!na || a_first);
    return a > b || (a == b && a_first);
}

__global__ void __launch_bounds__(FUSE_THREADS) k_fuse_rankings(const FuseArgs a) {
    __shared__ int64_t s_key[FUSE_MAX_ENTRIES];
    __shared__ uint64_t s_val[FUSE_MAX_ENTRIES];    // dense entry: the fp32 distance's bits; BM25 entry: the fp64 score's bits
    __shared__ double s_hyb[FUSE_MAX_ENTRIES];      // by insertion index
    __shared__ int32_t s_src[FUSE_MAX_ENTRIES];     // list << 16 | rank in the INPUT list
    __shared__ int32_t s_next[FUSE_MAX_ENTRIES];    // the next position holding the same key, or -1
    __shared__ uint64_t s_allow[FUSE_MAX_LISTS][FUSE_CHUNKS];
    __shared__ double s_weight[FUSE_MAX_LISTS];
    __shared__ int32_t s_cnt[FUSE_MAX_LISTS], s_nallow[FUSE_MAX_LISTS], s_len[FUSE_MAX_LISTS], s_kind[FUSE_MAX_LISTS];
    __shared__ int32_t s_wave_heads[FUSE_THREADS / 64];

    const int64_t q = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t list0 = q * a.n_lists;
    const bool filtered_q = a.filter_on != nullptr && a.filter_on[q] != 0;
    const uint32_t* allow = a.allow_groups + q * (int64_t)a.group_words;

    // 1. wave w: list w's header and, for a filtered dense list, which entries are allowed
    int cnt = -1, kind = FUSE_BM25, nallow = -1;      // nallow -1: the list is taken as given
    const int64_t base = (list0 + wave) * a.list_stride;
    if (wave < a.n_lists) {
        cnt = a.list_count[list0 + wave];
        cnt = cnt < 0 ? -1 : (cnt > a.list_stride ? a.list_stride : cnt);
        kind = a.list_kind[list0 + wave] == FUSE_DENSE ? FUSE_DENSE : FUSE_BM25;
        if (filtered_q && kind == FUSE_DENSE && cnt > 0) {
            nallow = 0;
            for (int c = 0; c * 64 < cnt; ++c) {
                const int i = c * 64 + lane;
                bool ok = false;
                if (i < cnt) {
                    const int64_t key = a.keys[base + i];
                    if (key >= 0 && key < a.n_rows) {
                        const int32_t g = a.row_group[key];
                        ok = g >= 0 && (g >> 5) < a.group_words && ((allow[g >> 5] >> (g & 31)) & 1u);
                    }
                }
                const unsigned long long m = __ballot(ok);
                if (lane == 0) s_allow[wave][c] = m;
                nallow += __popcll(m);
            }
        }
    }
    if (lane == 0) {
        s_cnt[wave] = cnt;
        s_kind[wave] = kind;
        s_nallow[wave] = nallow;
        s_weight[wave] = wave < a.n_lists ? a.list_weight[list0 + wave] : 0.0;
        // allowed entries, or min_semantic of the list (all of it when it is shorter) when fewer are allowed
        s_len[wave] = cnt < 0 ? 0 : (nallow < 0 ? cnt : (nallow >= a.min_semantic ? nallow : min(a.min_semantic, cnt)));
    }
    s_next[tid] = -1;
    __syncthreads();

    // 2. the sequence: list l starts at off_of(l)
    int my_off = 0, n = 0, present = 0;
#pragma unroll
    for (int l = 0; l < FUSE_MAX_LISTS; ++l) {
        if (l == wave) my_off = n;
        n += s_len[l];
        present += s_cnt[l] >= 0 ? 1 : 0;
    }
    if (cnt > 0) {
        int run_allow = 0;
        for (int c = 0; c * 64 < cnt; ++c) {
            const int i = c * 64 + lane;
            int pos = -1;
            if (nallow < 0) {
                if (i < cnt) pos = my_off + i;
            } else {
                const unsigned long long m = s_allow[wave][c];
                const int a_before = run_allow + __popcll(m & ((1ull << lane) - 1ull));
                const int r_before = i - a_before;              // refused entries in front of entry i
                if ((m >> lane) & 1ull) pos = my_off + a_before;
                else if (i < cnt && nallow + r_before < a.min_semantic) pos = my_off + nallow + r_before;
                run_allow += __popcll(m);
            }
            if (pos >= 0) {
                s_key[pos] = a.keys[base + i];
                s_val[pos] = kind == FUSE_DENSE ? (uint64_t)__float_as_uint(a.dense_dist[base + i])
                                                : (uint64_t)__double_as_longlong(a.bm25_score[base + i]);
                s_src[pos] = (wave << 16) | i;
            }
        }
    }
    __syncthreads();

    // 3. first appearance: link every position behind the nearest earlier one with its key
    const int p = tid;
    bool head = false;
    int64_t key = 0;
    if (p < n) {
        key = s_key[p];
        int prev = -1;
        for (int e = p - 1; e >= 0; --e) {
            if (s_key[e] == key) {
                prev = e;
                break;
            }
        }
        if (prev >= 0) s_next[prev] = p;      // (one writer: p is the nearest later position of prev's key)
        head = prev < 0;
    }
    const unsigned long long hm = __ballot(head);
    if (lane == 0) s_wave_heads[wave] = __popcll(hm);
    __syncthreads();
    int didx = __popcll(hm & ((1ull << lane) - 1ull)), distinct = 0;
#pragma unroll
    for (int w = 0; w < FUSE_THREADS / 64; ++w) {
        if (w < wave) didx += s_wave_heads[w];
        distinct += s_wave_heads[w];
    }

    // 4. a head replays _fuse's updates over its occurrences, in sequence order
    float dist = 0.0f;
    double sem = 0.0, bm = 0.0, hyb = 0.0;
    if (head) {
        // offsets of the lists again (thread p's list is not its wave's)
        for (int o = p; o >= 0; o = s_next[o]) {
            const int l = s_src[o] >> 16;
            int off = 0;
            for (int j = 0; j < l; ++j) off += s_len[j];
            const int rank = o - off;                             // rank in the FILTERED list
            if (s_kind[l] == FUSE_DENSE) {
                const float d = __uint_as_float((uint32_t)s_val[o]);
                const double sd = 1.0 / (1.0 + (double)d);        // RetrievedChunk.similarity_score
                if (o == p) {
                    dist = d;
                    sem = sd;
                } else {
                    if (d < dist) dist = d;
                    if (sd > sem) sem = sd;
                }
            } else {
                const double sc = __longlong_as_double((long long)s_val[o]);
                if (o == p) dist = 1.0f;                          // a chunk BM25 found first: distance 1.0, semantic 0.0
                bm = a.bm25_keep_max ? (sc > bm ? sc : bm) : sc;  // Python's max(old, new) keeps old unless new > old
            }
            hyb += s_weight[l] / (double)(a.rrf_k + rank + 1);
        }
        if (present <= 1) hyb = sem;
        s_hyb[didx] = hyb;
    }
    __syncthreads();

    // 5. the stable descending sort, as ranks
    const int64_t out0 = q * a.top_n;
    if (head) {
        int rank = 0;
        for (int e = 0; e < distinct; ++e) rank += (e != didx && fuse_before(s_hyb[e], hyb, e < didx)) ? 1 : 0;
        if (rank < a.top_n) {
            const int src = s_src[p];
            a.out_key[out0 + rank] = key;
            a.out_distance[out0 + rank] = dist;
            a.out_semantic[out0 + rank] = sem;
            a.out_bm25[out0 + rank] = bm;
            a.out_hybrid[out0 + rank] = hyb;
            a.out_list[out0 + rank] = src >> 16;
            a.out_rank[out0 + rank] = src & 0xffff;
        }
    }
    if (tid >= distinct && tid < a.top_n) {                       // slots past the count: key -1, zeros
        a.out_key[out0 + tid] = -1;
        a.out_distance[out0 + tid] = 0.0f;
        a.out_semantic[out0 + tid] = 0.0;
        a.out_bm25[out0 + tid] = 0.0;
        a.out_hybrid[out0 + tid] = 0.0;
        a.out_list[out0 + tid] = -1;
        a.out_rank[out0 + tid] = -1;
    }
    if (tid == 0) a.out_count[q] = min(a.top_n, distinct);
}

}  // namespace rdx
