// group_kernel.hpp — k_group_select: cut one query's ranked list (score descending, row ascending: include/rdx.h) into the first G
// distinct groups it meets and each group's first m rows (the reference deduplicates n_docs*10 chunks by document on
// the host, src/rag/retriever.py:202, 539-578). One workgroup per query, every step parallel over the list's positions:
//   1. code[i] = row_group[row[i]] (-1: padding, a row without the key, or a row id the table does not cover)
//   2. a position table in LDS, open addressing keyed by code: slot = the SMALLEST position that holds the slot's code
//   3. a position is a group's first when the table says so; a ballot scan over the positions numbers the firsts: the group's rank
//   4. ranks below G win; the table's slots are rewritten to hold the rank (or "lost")
//   5. a member's index inside its group = members of the same group at lower positions: per 64-position chunk by ballots, across
//      chunks by a prefix over a [chunk][rank] table of counts
// Nothing walks the list sequentially: 4096 entries cost a 1024-thread workgroup four passes of each step.
#pragma once
#include "rdx_common.hpp"

namespace rdx {

constexpr int GROUP_MAX_K = 4096;      // entries of a ranked list (rdx_search's largest k)
constexpr int GROUP_MAX_GROUPS = 64;   // G
constexpr int GROUP_MAX_SIZE = 16;     // m
constexpr int GROUP_TABLE = 8192;      // slots of the position table: load factor <= 1/2
constexpr int GROUP_CHUNKS = GROUP_MAX_K / 64;
constexpr int32_t GROUP_EMPTY = 0x7fffffff, GROUP_LOST = -1;

struct GroupSelectArgs {
    const float* scores; const int64_t* rows; const int32_t* counts; int k;    // the ranked lists [nq][k] and their lengths [nq]
    const int32_t* row_group; int64_t n_rows;                                 // row -> group code (-1: none)
    const int64_t* group_off; int64_t n_groups;                               // the CSR offsets [n_groups + 1]: |group|
    int G, m;
    float* out_score; int64_t* out_row;            // [nq][G][m], padding -inf / -1
    int32_t* out_count; int32_t* out_code;         // [nq][G]: members written, the group's code (-1: no such group)
    int32_t* out_complete;                         // [nq][G]: 1 = the members ARE the group's first m rows of the whole ranking
    int32_t* out_found; int32_t* out_short;        // [nq]: groups written; 1 = the list is full and holds fewer than G groups
    int32_t* out_bad;                              // [1]: set when a listed row id is >= n_rows or its code >= n_groups (the entry is ignored)
};

__device__ __forceinline__ int group_slot0(int32_t code) { return (int)(((uint32_t)code * 0x9E3779B1u) >> 19); }   // 13 bits

template <int NT>
__global__ __launch_bounds__(NT) void k_group_select(const GroupSelectArgs a) {
    constexpr int U = 4;   // positions per thread: the launcher picks NT with k <= U * NT
    constexpr int NW = NT / 64;
    __shared__ int32_t code[GROUP_MAX_K];
    __shared__ int32_t tab[GROUP_TABLE];
    __shared__ uint16_t cnt[GROUP_CHUNKS][GROUP_MAX_GROUPS];   // members of rank g in chunk c, then their exclusive prefix over c
    __shared__ int32_t wfirst[U][NW];
    __shared__ int32_t total[GROUP_MAX_GROUPS], wcode[GROUP_MAX_GROUPS];
    const int q = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int k = a.k, G = a.G, m = a.m;
    int n = a.counts[q];
    n = n < 0 ? 0 : (n > k ? k : n);
    const float* __restrict__ sc = a.scores + (int64_t)q * k;
    const int64_t* __restrict__ ro = a.rows + (int64_t)q * k;
    float* o_s = a.out_score + (int64_t)q * G * m;
    int64_t* o_r = a.out_row + (int64_t)q * G * m;

    for (int i = t; i < G * m; i += NT) {
        o_s[i] = -INFINITY;
        o_r[i] = -1;
    }
    for (int i = t; i < GROUP_TABLE; i += NT) tab[i] = GROUP_EMPTY;
    for (int i = t; i < GROUP_CHUNKS * GROUP_MAX_GROUPS; i += NT) (&cnt[0][0])[i] = 0;
    // 1. the codes
    int32_t my_code[U];
    int64_t my_row[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int i = u * NT + t;
        int32_t c = -1;
        int64_t r = -1;
        if (i < n) {
            r = ro[i];
            if (r >= a.n_rows) atomicOr(a.out_bad, 1);
            else if (r >= 0) c = a.row_group[r];
            if (c >= a.n_groups) {
                atomicOr(a.out_bad, 1);
                c = -1;
            }
        }
        my_code[u] = c;
        my_row[u] = r;
        if (i < GROUP_MAX_K) code[i] = c;
    }
    __syncthreads();
    // 2. insert: the slot of a code holds the smallest position of that code (the key of a slot is code[tab[slot]], which an
    //    atomicMin among positions of one code never changes)
    //    Termination: a slot is written once from GROUP_EMPTY (the CAS) and afterwards only by atomicMin among positions of its code,
    //    so it never becomes empty again and its key never changes. A list holds at most GROUP_MAX_K distinct codes and one code
    //    claims at most one slot (below), so at most GROUP_MAX_K = GROUP_TABLE / 2 slots are ever taken: a walk that steps
    //    (s + 1) & (GROUP_TABLE - 1), through the wrap from the last slot to slot 0, meets its own code or an empty slot within
    //    GROUP_TABLE steps.
    //    The outputs do not depend on who wins a slot. A position of code c passes a slot only when another code holds it, and
    //    that slot keeps that code for good; so every position of c passes the same slots and stops at the first slot after them
    //    that is empty or holds c — all positions of c end in ONE slot, and no other code can end there. WHICH slot that is depends
    //    on the order in which the codes of a chain arrive; what the later steps read does not: my_slot[] is used only to reach
    //    tab[my_slot], and after the barrier that is the minimum over the positions of c, whatever the slot.
    //    (Dense codes below 4182 never share a home slot — the multiplier is 2^32 / phi; tests/test_group_table_model.py states it
    //    and tests/test_gpu_group_kernels.py::test_select_on_colliding_codes runs the codes that do.)
    int my_slot[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int i = u * NT + t;
        my_slot[u] = -1;
        if (my_code[u] < 0) continue;
        int s = group_slot0(my_code[u]);
        for (;;) {
            int32_t cur = tab[s];
            if (cur == GROUP_EMPTY) {
                cur = atomicCAS(&tab[s], GROUP_EMPTY, i);
                if (cur == GROUP_EMPTY) break;
            }
            if (code[cur] == my_code[u]) {
                atomicMin(&tab[s], i);
                break;
            }
            s = (s + 1) & (GROUP_TABLE - 1);
        }
        my_slot[u] = s;
    }
    __syncthreads();
    // 3. firsts and their ranks
    bool first[U];
    int rank[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        first[u] = my_slot[u] >= 0 && tab[my_slot[u]] == u * NT + t;
        const unsigned long long b = __ballot(first[u]);
        rank[u] = __popcll(b & ((1ull << lane) - 1ull));
        if (lane == 0) wfirst[u][wave] = __popcll(b);
    }
    __syncthreads();
    int n_distinct = 0;
    {
        int before[U];
#pragma unroll
        for (int u = 0; u < U; ++u) before[u] = 0;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            for (int w = 0; w < NW; ++w) {
                const int c = wfirst[u][w];
                n_distinct += c;
#pragma unroll
                for (int v = 0; v < U; ++v)
                    if (u < v || (u == v && w < wave)) before[v] += c;
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) rank[u] += before[u];
    }
    __syncthreads();   // (every reader of the positions is done: the slots change meaning)
    // 4. the winners' slots hold the rank
#pragma unroll
    for (int u = 0; u < U; ++u) {
        if (first[u]) {
            const bool win = rank[u] < G;
            tab[my_slot[u]] = win ? rank[u] : GROUP_LOST;
            if (win) wcode[rank[u]] = my_code[u];
        }
    }
    __syncthreads();
    // 5. members: index inside the chunk by ballots over the ranks present in it
    int g_of[U], idx[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int i = u * NT + t;
        g_of[u] = my_slot[u] >= 0 ? tab[my_slot[u]] : GROUP_LOST;
        idx[u] = 0;
        unsigned long long todo = __ballot(g_of[u] >= 0);
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const int gl = __shfl(g_of[u], leader, 64);
            const unsigned long long same = __ballot(g_of[u] == gl);
            if (g_of[u] == gl) idx[u] = __popcll(same & ((1ull << lane) - 1ull));
            if (lane == leader) cnt[i >> 6][gl] = (uint16_t)__popcll(same);
            todo &= ~same;
        }
    }
    __syncthreads();
    if (t < G) {   // exclusive prefix over the chunks, per rank
        int run = 0;
        const int chunks = (n + 63) >> 6;
        for (int c = 0; c < chunks; ++c) {
            const int v = cnt[c][t];
            cnt[c][t] = (uint16_t)run;
            run += v;
        }
        total[t] = run;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int i = u * NT + t;
        if (g_of[u] < 0) continue;
        const int at = cnt[i >> 6][g_of[u]] + idx[u];
        if (at < m) {
            o_s[g_of[u] * m + at] = sc[i];
            o_r[g_of[u] * m + at] = my_row[u];
        }
    }
    const bool full = n == k;
    const int found = n_distinct < G ? n_distinct : G;
    if (t < G) {
        int32_t* o_cnt = a.out_count + (int64_t)q * G;
        int32_t* o_cpl = a.out_complete + (int64_t)q * G;
        if (t < found) {
            const int listed = total[t];
            const int32_t c = wcode[t];
            a.out_code[(int64_t)q * G + t] = c;
            const int64_t size = a.group_off[c + 1] - a.group_off[c];
            const int64_t want = size < m ? size : m;
            o_cnt[t] = listed < m ? listed : m;
            o_cpl[t] = (!full || listed >= want) ? 1 : 0;
        } else {
            o_cnt[t] = 0;
            o_cpl[t] = 1;
            a.out_code[(int64_t)q * G + t] = -1;
        }
    }
    if (t == 0) {
        a.out_found[q] = found;
        a.out_short[q] = (full && n_distinct < G) ? 1 : 0;
    }
}

}  // namespace rdx
