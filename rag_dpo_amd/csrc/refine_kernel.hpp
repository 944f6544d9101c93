// refine_kernel.hpp — K4: exact re-score + final ordering of the scan's candidates, and C1's merge of per-shard
// partial results after the RCCL all-gather.
#pragma once
#include "k_rows.hpp"

namespace rdx {

struct RefineCounters {   // one per index, zeroed before every search
    unsigned long long emitted;
    unsigned long long rescored;
    int n_exact;          // queries handed to the exact full scan
    int bad;              // set by K1 when a query embedding holds NaN/Inf
    int oob;              // RDX_CHECK_BOUNDS builds: the scan computed a corpus address outside the scan copy
    int spec_fail;        // queries whose speculative threshold could not be verified (k_refine; they take the fallback passes)
    // option profile = 3 (kernels stamp their own times, no HIP events on the stream): when the first block of the exact path's
    // scoring kernel started (kept as max(~clock): zero = unset) and when the last block of its select kernel ended (100 MHz ticks)
    unsigned long long t_first_inv, t_last;
    int done;             // blocks of the search's last kernel that have finished (the last one runs the end-of-search work)
    int n_spill;          // queries k_refine answered from its spill list in HBM (more hits than the LDS list holds)
    int max_hits;         // most hits of one query (developer: RDX_DEBUG_HITS)
    int pad1;
};

// What the LAST kernel of a search leaves in pinned host memory (written straight over PCIe, no memcpy, no interrupt):
// the host spins on `seq` instead of paying a D2H copy plus hipStreamSynchronize (~25 us of a 0.1 ms search).
struct Mailbox {
    unsigned long long seq;            // written last, system-scope release: search number `seq` is complete
    unsigned long long emitted, rescored;
    int n_exact, bad;
    int oob, spec_fail;
    unsigned long long t_first, t_last;   // profile = 3, exact path (see RefineCounters)
    unsigned long long wg_times[1024]; // [grid][2] start/end stamps of the main scan's workgroups (XCD balancing)
    int n_spill, max_hits;             // (RefineCounters)
};

// K6. End of every search: (1) small results of HOST callers go from the device result buffers to pinned host staging,
// (2) the counters (and the workgroup stamps) go to the mailbox, (3) the counter block is zeroed for the next search
// (searches on one index are serialised by its mutex and each one has completed before the next is enqueued),
// (4) the sequence number is published. The volumes are KBs: ONE block does it — since round 3 the last block to finish of the
// search's last kernel (k_refine / k_select_dense: finish_if_last below), which saves a launch and a gap on every search; the
// stand-alone kernel k_finish remains for option "fuse_finish" = 0.
struct FinishArgs {
    RefineCounters* ctr;     // NULL: this launch does not end a search
    Mailbox* mb;
    unsigned long long seq;
    const unsigned long long* wgt;
    int n_wgt;
    const uint32_t* s0; uint32_t* d0; int64_t w0;
    const uint32_t* s1; uint32_t* d1; int64_t w1;
    const uint32_t* s2; uint32_t* d2; int64_t w2;
    int32_t* out_flags;
    int may_redo;
};

__device__ __forceinline__ void finish_body(const FinishArgs& f) {   // all threads of ONE block
    RefineCounters* ctr = f.ctr;
    Mailbox* mb = f.mb;
    for (int64_t i = threadIdx.x; i < f.w0; i += blockDim.x) f.d0[i] = f.s0[i];
    for (int64_t i = threadIdx.x; i < f.w1; i += blockDim.x) f.d1[i] = f.s1[i];
    for (int64_t i = threadIdx.x; i < f.w2; i += blockDim.x) f.d2[i] = f.s2[i];
    for (int i = threadIdx.x; i < f.n_wgt; i += blockDim.x) mb->wg_times[i] = f.wgt[i];
    // every storing wave waits for its own stores, the barrier collects the waves, and ONE lane makes the block's stores visible to
    // the host (system-scope release) before it publishes the sequence number — not a system-scope fence in all 1024 threads
    // (MI355X_MICROARCH.md, inter-workgroup visibility: "every storing wave's s_waitcnt vmcnt(0) -> __syncthreads() -> lane-0 fence")
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        // rdx_search_async(out_flags): "this partial is incomplete, the host half will redo some queries" — the word travels with
        // the packed partial through the all-gather (include/rdx.h); the same condition complete_search reports as *redone
        if (f.out_flags) {
            f.out_flags[0] = (f.may_redo && ctr->n_exact > 0 && !ctr->bad) ? 1 : 0;
            f.out_flags[1] = 0;
            f.out_flags[2] = 0;
            f.out_flags[3] = 0;
        }
        mb->emitted = ctr->emitted;
        mb->rescored = ctr->rescored;
        mb->n_exact = ctr->n_exact;
        mb->bad = ctr->bad;
        mb->oob = ctr->oob;
        mb->spec_fail = ctr->spec_fail;
        ctr->spec_fail = 0;
        mb->n_spill = ctr->n_spill;
        mb->max_hits = ctr->max_hits;
        ctr->n_spill = 0;
        ctr->max_hits = 0;
        mb->t_first = ~ctr->t_first_inv;
        mb->t_last = ctr->t_last;
        ctr->t_first_inv = 0;
        ctr->t_last = 0;
        ctr->oob = 0;
        ctr->emitted = 0;
        ctr->rescored = 0;
        ctr->n_exact = 0;
        ctr->bad = 0;
        ctr->done = 0;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");          // system scope: the block's stores (L2 written back) before the flag
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // (always, behind a release fence: the compiler may drop its own wait)
        __hip_atomic_store(&mb->seq, f.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

__global__ __launch_bounds__(1024) void k_finish(const FinishArgs f) { finish_body(f); }

// Tail of the search's last kernel (all threads of every block call it, at a point every thread reaches): the block's result
// stores are drained and released at agent scope by one lane, which takes a ticket; the block holding the last ticket acquires
// (its CU's L1 may hold stale lines of what the other blocks wrote) and runs the end-of-search work.
// (MI355X_MICROARCH.md, hand-off forms: storing waves' vmcnt(0) -> barrier -> one lane's release + agent-scope atomic add; the
//  workgroup whose add came last loads after its acquire and a barrier.)
__device__ __forceinline__ void finish_if_last(const FinishArgs& f) {
    if (!f.ctr) return;
    __shared__ int s_last;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        const int t = __hip_atomic_fetch_add(&f.ctr->done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = t == (int)gridDim.x - 1;
        if (last) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        s_last = last;
    }
    __syncthreads();
    if (s_last) finish_body(f);
}

// One block per query (256 threads, 1024 when k is large: the exact re-score runs one wave per candidate row).
//   The scan left, per (query, stream), cntw hits in a segment of capw slots: (coarse score, row) of every allowed row
//   whose coarse score >= tau[q]. They are gathered into LDS; c_k = k-th largest coarse score. Every true top-k row has
//   coarse >= c_k - 2E (|coarse-exact| <= E and k rows reach coarse c_k, hence exact c_k - E), so
//   P = {coarse >= c_k - 2E} contains the exact top-k; P is re-scored exactly from the fp32 master copy (fp64 lane-order
//   sum, oracle/rdx_oracle.c) and ranked (score desc, row asc).
//   A segment, list or P overflow cannot be answered here: the query is flagged for the exact full scan.
//   int8 coarse pass (two_e_q != NULL) with pilot > 0: the band is found in TWO rounds (DESIGN.md §5 "two-round re-score"). 2E_q pays
//   for not knowing the exact k-th score X; so S1 = the hits that reach the k1-th largest coarse score (k1 = min(m, pilot k)) are
//   re-scored first, X1 = the k-th largest exact score in S1 (X1 <= X: S1 is a subset), and only S2 = {coarse >= X1 - E_q} \ S1
//   is re-scored after them: a hit outside S1 and S2 has exact <= coarse + E_q < X1 <= X, strictly below the k-th score.
#ifdef RDX_REFINE_STAMPS   // developer build (tools/refine_stamps.py): where k_refine spends its time (block 0's phases, 100 MHz wall clock)
__device__ unsigned long long g_refine_stamps[16];
#define RDX_RSTAMP(i) do { __syncthreads(); if (blockIdx.x == 0 && threadIdx.x == 0) g_refine_stamps[i] = wall_clock64(); } while (0)
#else
#define RDX_RSTAMP(i) do { } while (0)
#endif

// a - b rounded toward -inf (both finite): a band edge may only move down
__device__ __forceinline__ float sub_down(float a, float b) {
    float d = a - b;
    if ((double)d > (double)a - (double)b) d = nextafterf(d, -INFINITY);
    return d;
}

// The static LDS of a k_refine block. ONE object per kernel, handed to refine_list by reference: the kernel of a spilling plan holds
// both instantiations of refine_list, and arrays declared inside the template would be laid out once for each (22 KiB twice — with
// the 56 KiB list, the second block of a CU would no longer fit).
struct RefineLds {
    __attribute__((aligned(16))) uint32_t hist[HIST_WORDS];
    int64_t s_r[REFINE_PMAX];
    float s_s[REFINE_PMAX];
    uint32_t seg_off[REFINE_STREAMS + 1];
    uint32_t bc[4];
    int wtot[16];
    int n_p, overflow;
};

// A query's m > 0 hits, counted and prefixed by refine_block (L.seg_off), are gathered into `list` and answered. The list lives in
// LDS (SPILL = false: at most list_cap <= REFINE_LIST entries) or in the query's row of the spill buffer in HBM (SPILL = true: at
// most spill_cap entries, L2-resident while the block works on it): the same statements, so which rows are re-scored does not
// depend on where the list lives.
template <bool SPILL>
__device__ __forceinline__ void refine_list(RefineLds& L, uint2* const list, const uint32_t m, const int q,
                                            const uint2* __restrict__ cand, int n_streams, uint32_t capw, int k, float two_e,
                                            const float* __restrict__ two_e_q, const float* __restrict__ qhat, MasterView master, int dim,
                                            int64_t row_base, const int64_t* __restrict__ row_map,
                                            float* __restrict__ out_score, int64_t* __restrict__ out_row,
                                            int32_t* __restrict__ out_count, int32_t* __restrict__ exact_list,
                                            RefineCounters* __restrict__ ctr, const float* __restrict__ tau, float inv_scale2,
                                            int pilot) {
    uint32_t* const hist = L.hist;
    uint32_t* const bc = L.bc;
    const uint32_t* const seg_off = L.seg_off;
    float* const s_s = L.s_s;
    int64_t* const s_r = L.s_r;
    int* const wtot = L.wtot;
    int& n_p = L.n_p;
    float* o_s = out_score + (int64_t)q * k;
    int64_t* o_r = out_row + (int64_t)q * k;
    // gather: one thread per ENTRY — its segment is the last w with seg_off[w] <= i (binary search of the prefix in LDS), so every
    // thread has loads in flight and none depends on another (a thread per segment was 64 of 1024 threads at c4, each walking
    // 40-125 dependent 8-byte loads). The entries keep their order: segment after segment.
    for (uint32_t i = threadIdx.x; i < m; i += blockDim.x) {
        int lo = 0, hi = n_streams;                         // seg_off[lo] <= i < seg_off[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (seg_off[mid] <= i) lo = mid;
            else hi = mid;
        }
        list[i] = cand[((int64_t)q * n_streams + lo) * capw + (i - seg_off[lo])];
    }
    __syncthreads();
    RDX_RSTAMP(2);
    const int64_t kk = (uint32_t)k < m ? k : m;
    // int8 coarse pass: verified AFTER the exact re-score, against the exact k-th score X of the hits (a row that was not emitted
    // scores below tau + E_q exactly: the answer is complete iff X - E_q >= tau). Its E_q is ~14x the fp16 E, and the
    // test before the re-score (c_k - 2E >= tau) would reject most speculative thresholds.
    const bool late = two_e_q != nullptr;
    bool two = late && pilot > 0;                           // two rounds: pilot S1, then the band below X1
    auto coarse_kth = [&](int64_t rank) __attribute__((always_inline)) {
        int64_t n_gt;
        return key2f(block_kth_largest([&](int64_t i) { return f2key(__uint_as_float(list[i].x)); }, m, rank, hist, bc, &n_gt));
    };
    const int64_t k1 = (int64_t)pilot * k < (int64_t)m ? (int64_t)pilot * k : (int64_t)m;
    // lower edge of the first collection: c_k - 2E (one band), or c_k1 itself (S1)
    // (int8 coarse pass: the bound is the query's own, two_e_q[q] = 2 E_q, and tau is already in score units — DESIGN.md §5)
    float t2 = two ? coarse_kth(k1) : coarse_kth(kk) - (two_e_q ? two_e_q[q] : two_e);
    RDX_RSTAMP(3);
    // Verification of the scan's threshold T (score units). The hits are exactly the allowed rows with coarse >= T. The k best of
    // them have exact >= c_k - E, so the exact k-th best of the corpus is >= c_k - E and every true top-k row has coarse >=
    // c_k - 2E: all of those were emitted iff c_k - 2E >= T (and k hits exist at all). A threshold taken from k sampled rows
    // (k_tau with rank k) passes by construction; a SPECULATIVE one (rank < k: an estimate of where the corpus' k-th score
    // lies) passes unless the estimate was too high — then the query goes to the fallback passes, which use
    // the provable threshold. T = -inf (fewer than k sets sampled): every allowed row was emitted, nothing to verify.
    const float tq = tau[q] * inv_scale2;
    auto verify_exact = [&](uint32_t kth_key) __attribute__((always_inline)) {
        if (!late || !(tq > -INFINITY) || key2f(kth_key) - 0.5f * two_e_q[q] >= tq) return true;
        if (threadIdx.x == 0) {
            atomicAdd(&ctr->spec_fail, 1);
            exact_list[atomicAdd(&ctr->n_exact, 1)] = q;
        }
        return false;
    };
    if (tq > -INFINITY && ((int64_t)m < (int64_t)k || (!late && t2 < tq))) {
        if (threadIdx.x == 0) {
            atomicAdd(&ctr->spec_fail, 1);
            exact_list[atomicAdd(&ctr->n_exact, 1)] = q;
        }
        return;
    }
    // rows of the hits with lo <= coarse < hi are appended to s_r (n_p counts them all, the arrays take the first REFINE_PMAX)
    auto collect = [&](float lo, float hi) __attribute__((always_inline)) {
        for (uint32_t i = threadIdx.x; i < m; i += blockDim.x) {
            const uint2 e = list[i];
            const float c = __uint_as_float(e.x);
            if (c >= lo && c < hi) {
                const int pos = atomicAdd(&n_p, 1);
                if (pos < REFINE_PMAX) s_r[pos] = (int64_t)e.y;
            }
        }
        __syncthreads();
        return n_p;
    };
    if (threadIdx.x == 0) n_p = 0;
    __syncthreads();
    int p = collect(t2, INFINITY);
    if (two && p > REFINE_PMAX) {
        // more than the ranking arrays hold tie at the k1-th coarse score (identical rows): the single band, as without a pilot
        two = false;
        t2 = coarse_kth(kk) - two_e_q[q];
        if (threadIdx.x == 0) n_p = 0;
        __syncthreads();
        p = collect(t2, INFINITY);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float4* q4 = reinterpret_cast<const float4*>(qhat + (int64_t)q * dim);
    const int n4 = dim >> 2, nw = (int)(blockDim.x >> 6);
    // exact re-score of `cnt` candidates, one wave per candidate row: row_at(i) = its row, put(i, s) takes its exact score
    auto rescore = [&](int cnt, auto row_at, auto put) __attribute__((always_inline)) {
        if (n4 <= 256) {
            // dim <= 1024: the query sits in registers as doubles (converted once per block, not once per candidate), a row's four
            // 1 KiB pieces are requested together and the NEXT candidate's pieces before this one is summed. Same products, same
            // order per lane, same butterfly as exact_score(): the same bits. (c3: k = 100, ~140 candidates per query = 9 dependent
            // round trips to random HBM rows per wave before.)
            int gi[4];
            bool gv[4];
            float4 qf[4];                                   // (kept as floats, widened at use: 16 registers instead of 32)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                gv[u] = lane + 64 * u < n4;
                gi[u] = gv[u] ? lane + 64 * u : n4 - 1;
                const float4 qq = q4[gi[u]];
                qf[u] = gv[u] ? qq : make_float4(0.f, 0.f, 0.f, 0.f);
            }
            auto load_row = [&](int i, float4 (&c)[4]) __attribute__((always_inline)) {
                const MasterRow row4 = master_row(master, row_at(i), dim);
#pragma unroll
                for (int u = 0; u < 4; ++u) c[u] = row4[gi[u]];
            };
            float4 cur[4], nxt[4];
            if (wave < cnt) load_row(wave, cur);
            for (int i = wave; i < cnt; i += nw) {
                load_row(i + nw < cnt ? i + nw : i, nxt);   // (the last one re-reads its own row: no branch around loads)
                double acc = 0.0;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    acc += (double)qf[u].x * (double)cur[u].x;
                    acc += (double)qf[u].y * (double)cur[u].y;
                    acc += (double)qf[u].z * (double)cur[u].z;
                    acc += (double)qf[u].w * (double)cur[u].w;
                }
                const float sx = (float)wave_sum(acc);
                if (lane == 0) put(i, sx);
#pragma unroll
                for (int u = 0; u < 4; ++u) cur[u] = nxt[u];
            }
            // (a third row in flight per wave — the loop is 9 dependent ~2 us round trips at c3 — needs 16 more registers than the
            //  1024-thread block has: 17 spilled. Measured instead: profiles/r04/refine_stamps.txt)
        } else {
            for (int i = wave; i < cnt; i += nw) {
                const float sx = exact_score(master_row(master, row_at(i), dim), q4, n4, lane);
                if (lane == 0) put(i, sx);
            }
        }
    };
    int done = 0;                                           // entries of s_r / s_s that already hold their exact score (S1)
    float c1 = INFINITY;                                    // the band's upper edge: S1 (coarse >= c1) is not collected twice
    if (two) {
        rescore(p, [&](int i) { return s_r[i]; }, [&](int i, float sx) { s_s[i] = sx; });
        __syncthreads();
        done = p;
        c1 = t2;
        // X1 = k-th largest exact score of S1; fewer than k rows in S1 (then S1 is every hit): no bound, the band is empty anyway.
        // t3 = X1 - E_q rounded DOWN (E_q = two_e_q / 2 is exact): every hit with coarse >= X1 - E_q is inside whatever the rounding
        t2 = -INFINITY;
        if (p >= k) {
            int64_t n_gt1;
            const uint32_t kx = block_kth_largest([&](int64_t i) { return f2key(s_s[i]); }, p, (int64_t)k, hist, bc, &n_gt1);
            t2 = sub_down(key2f(kx), 0.5f * two_e_q[q]);
        }
        p = collect(t2, c1);                                // S2 behind S1 (n_p goes on counting)
    }
    if (threadIdx.x == 0) atomicAdd(&ctr->rescored, (unsigned long long)p);
    if (p > REFINE_PMAX) {
        // More rows inside the 2E band than the ranking arrays hold: near-duplicate rows stored together (a document's chunks: their
        // scores lie closer together than the coarse pass can tell apart, so the band holds hundreds to thousands of them). Until
        // round 4 such a query paid the exact full scan of the WHOLE corpus (7 ms per 4 queries at 10 M rows: an embedding-like corpus
        // ran at 2 % of the N(0,1) corpus' speed). The band is small next to the corpus: its members are compacted to the front of the
        // list (every thread reads 7 entries, then — behind a barrier — writes the members back), re-scored exactly in place
        // (exact score over coarse score), the k-th largest exact score is found by the radix select, and only what reaches it is ranked.
        // The list is compacted in rounds of 7 entries per thread (the LDS list is one round; a spill list takes up to
        // spill_cap / 7168): a round's members are written behind the earlier rounds' — at or below the round's own first entry, and
        // every entry up to the round's end was read before the barrier, so nothing unread is overwritten.
        int base_out = 0;
        for (uint32_t r0 = 0; r0 < m; r0 += 7u * blockDim.x) {
            uint2 mine[7];
            bool keep[7];
            int cnt = 0;
#pragma unroll
            for (int j = 0; j < 7; ++j) {
                const uint32_t i = r0 + threadIdx.x * 7 + j;
                keep[j] = false;
                if (i < m) {
                    mine[j] = list[i];
                    const float cs = __uint_as_float(mine[j].x);
                    keep[j] = cs >= t2 && cs < c1;
                }
                cnt += keep[j] ? 1 : 0;
            }
            int incl = cnt;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int t = __shfl_up(incl, off, 64);
                if (lane >= off) incl += t;
            }
            if (lane == 63) wtot[wave] = incl;
            __syncthreads();                                          // (also: every thread has read its entries of this round)
            int pos = base_out + incl - cnt;
            for (int w = 0; w < wave; ++w) pos += wtot[w];
            for (int w = 0; w < nw; ++w) base_out += wtot[w];
#pragma unroll
            for (int j = 0; j < 7; ++j)
                if (keep[j]) list[pos++] = mine[j];
            __syncthreads();
        }
        // (two rounds: the p - done rows of S2 were compacted; S1, already exact in the ranking arrays, goes behind them — S1 and
        //  S2 are disjoint subsets of the m hits, so p <= m slots)
        for (int i = threadIdx.x; i < done; i += blockDim.x) list[p - done + i] = make_uint2(__float_as_uint(s_s[i]), (uint32_t)s_r[i]);
        rescore(p - done, [&](int i) { return (int64_t)list[i].y; }, [&](int i, float sx) { list[i].x = __float_as_uint(sx); });
        __syncthreads();
        const int64_t kk2 = k < p ? k : p;
        int64_t n_gt2;
        // (selection keys, k_rows.hpp: +0.0 and -0.0 are one score — with f2key a k-th key of +0.0 left the -0.0 rows out of the ties)
        const uint32_t kth2 = block_kth_largest([&](int64_t i) { return f2key_sel(__uint_as_float(list[i].x)); }, p, kk2, hist, bc, &n_gt2);
        if (!verify_exact(kth2)) return;
        // everything above the k-th key and the entries equal to it whose row key reaches `rkey`: first EVERY tie (rkey = 0; the
        // ranking below orders them by row id), which is all there is to do unless identical rows fill the ranking arrays
        auto take = [&](uint32_t rkey) __attribute__((always_inline)) {
            if (threadIdx.x == 0) n_p = 0;
            __syncthreads();
            for (int i = threadIdx.x; i < p; i += blockDim.x) {
                const uint2 e = list[i];
                const uint32_t key = f2key_sel(__uint_as_float(e.x));
                if (key > kth2 || (key == kth2 && ~e.y >= rkey)) {
                    const int at = atomicAdd(&n_p, 1);
                    if (at < REFINE_PMAX) {
                        s_s[at] = __uint_as_float(e.x);
                        s_r[at] = (int64_t)e.y;
                    }
                }
            }
            __syncthreads();
            return n_p;
        };
        int p2 = take(0u);
        if (p2 > REFINE_PMAX) {
            // > 1024 - k rows tie at the k-th score (identical rows; zeros of both signs): of the ties the kk2 - n_gt2 with the LOWEST
            // rows belong to the answer. The hits' rows are distinct 32-bit local rows (returned ids grow with them: row_base, or the
            // strictly increasing row id map), so that many lowest rows are the keys ~row down to their (kk2 - n_gt2)-th largest —
            // one more radix select (non-ties count as key 0, below every ~row), then kk2 <= k entries are ranked.
            int64_t n_gt_r;
            const uint32_t rkey = block_kth_largest(
                [&](int64_t i) {
                    const uint2 e = list[i];
                    return f2key_sel(__uint_as_float(e.x)) == kth2 ? ~e.y : 0u;
                },
                p, kk2 - n_gt2, hist, bc, &n_gt_r);
            p2 = take(rkey);
        }
        for (int i = threadIdx.x; i < p2; i += blockDim.x) s_r[i] = row_map ? row_map[s_r[i]] : s_r[i] + row_base;
        __syncthreads();
        rank_and_write(s_s, s_r, p2, k, o_s, o_r, out_count + q);
        return;
    }
    RDX_RSTAMP(4);
    rescore(p - done, [&](int i) { return s_r[done + i]; }, [&](int i, float sx) { s_s[done + i] = sx; });
    __syncthreads();
    if (late) {
        int64_t n_gt3;
        const uint32_t kth3 = block_kth_largest([&](int64_t i) { return f2key(s_s[i]); }, p, (int64_t)(k < p ? k : p), hist, bc, &n_gt3);
        if (!verify_exact(kth3)) return;
    }
    RDX_RSTAMP(5);
    // local -> returned row id: + row_base, or through the shard's (strictly increasing) row id map
    for (int i = threadIdx.x; i < p; i += blockDim.x) s_r[i] = row_map ? row_map[s_r[i]] : s_r[i] + row_base;
    __syncthreads();
    rank_and_write(s_s, s_r, p, k, o_s, o_r, out_count + q);
    RDX_RSTAMP(6);
}

// K4, one block per query: the hits are counted (segment sizes -> exclusive prefix), and the query takes one of three routes.
//   m <= list_cap, no segment overflowed: the list in LDS (refine_list<false>);
//   MAY_SPILL (the plan spills: SearchPlan::spill), m <= spill_cap, no segment overflowed: the block goes on IN THIS LAUNCH with its
//     row of the spill buffer as the list (refine_list<true>). Until the one-launch form a second kernel, launched behind this one
//     with a block per possible query, answered the queued queries: 0.22 ms at c4 for 134 of 1 024 blocks with work;
//   otherwise: the exact full scan (exact_list).
template <bool MAY_SPILL>
__device__ __forceinline__ void refine_block(const int q, uint2* __restrict__ spill, uint32_t spill_cap,
                                             const uint2* __restrict__ cand, const uint32_t* __restrict__ cntw,
                                             int n_streams, uint32_t capw, uint32_t list_cap, int k, float two_e,
                                             const float* __restrict__ two_e_q, const float* __restrict__ qhat, MasterView master, int dim,
                                             int64_t row_base, const int64_t* __restrict__ row_map,
                                             float* __restrict__ out_score, int64_t* __restrict__ out_row,
                                             int32_t* __restrict__ out_count, int32_t* __restrict__ exact_list,
                                             RefineCounters* __restrict__ ctr, const float* __restrict__ tau, float inv_scale2,
                                             int pilot) {
    extern __shared__ __attribute__((aligned(16))) char smem[];   // [list_cap] hits (the LDS list)
    __shared__ RefineLds L;
    uint32_t* const seg_off = L.seg_off;
    if (threadIdx.x == 0) L.overflow = 0;
    __syncthreads();
    RDX_RSTAMP(0);
    // segment sizes -> exclusive prefix. Wave 0 scans them 64 at a time with shuffles (n_streams <= 512: at most 8 rounds; the
    // serial loop this replaces was 3-5 us of the kernel at 256 streams)
    for (int w = threadIdx.x; w < n_streams; w += blockDim.x) {
        const uint32_t c = cntw[(int64_t)q * n_streams + w];
        if (c > capw) L.overflow = 1;
        seg_off[w + 1] = c > capw ? capw : c;
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        const int l = threadIdx.x;
        uint32_t carry = 0;
        for (int base = 0; base < n_streams; base += 64) {
            const int w = base + l;
            uint32_t v = w < n_streams ? seg_off[w + 1] : 0u;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const uint32_t t = __shfl_up(v, off, 64);
                if (l >= off) v += t;
            }
            if (w < n_streams) seg_off[w + 1] = carry + v;      // inclusive prefix -> offset of segment w + 1
            carry += __shfl(v, 63, 64);
        }
        if (l == 0) seg_off[0] = 0;
    }
    __syncthreads();
    const uint32_t m = seg_off[n_streams];
    const bool overflow = L.overflow != 0;
    RDX_RSTAMP(1);
    if (threadIdx.x == 0) {
        atomicAdd(&ctr->emitted, (unsigned long long)m);
        atomicMax(&ctr->max_hits, (int)m);
    }
    bool to_spill = false;
    if (overflow || m > list_cap) {
        to_spill = MAY_SPILL && !overflow && m <= spill_cap;
        if (threadIdx.x == 0) {
            if (to_spill) atomicAdd(&ctr->n_spill, 1);
            else exact_list[atomicAdd(&ctr->n_exact, 1)] = q;
        }
        if (!to_spill) return;
    }
    if (m == 0 || k == 0) {
        rank_and_write(L.s_s, L.s_r, 0, k, out_score + (int64_t)q * k, out_row + (int64_t)q * k, out_count + q);
        return;
    }
    if constexpr (MAY_SPILL) {
        if (to_spill) {
            refine_list<true>(L, spill + (int64_t)q * spill_cap, m, q, cand, n_streams, capw, k, two_e, two_e_q, qhat, master, dim, row_base,
                              row_map, out_score, out_row, out_count, exact_list, ctr, tau, inv_scale2, pilot);
            return;
        }
    }
    refine_list<false>(L, reinterpret_cast<uint2*>(smem), m, q, cand, n_streams, capw, k, two_e, two_e_q, qhat, master, dim, row_base,
                       row_map, out_score, out_row, out_count, exact_list, ctr, tau, inv_scale2, pilot);
}

// MAY_SPILL = false: the kernel of every plan that does not spill, the LDS route alone (what k_refine was before the spill list).
// MAY_SPILL = true: both routes; `spill` is [nq_pad][spill_cap] in HBM. The search's last kernel on the MFMA path for every plan.
template <bool MAY_SPILL>
__global__ __launch_bounds__(1024) void k_refine(const uint2* __restrict__ cand, const uint32_t* __restrict__ cntw,
                                                int n_streams, uint32_t capw, uint32_t list_cap, int k, float two_e,
                                                const float* __restrict__ two_e_q, const float* __restrict__ qhat, MasterView master, int dim,
                                                int64_t row_base, const int64_t* __restrict__ row_map,
                                                float* __restrict__ out_score, int64_t* __restrict__ out_row,
                                                int32_t* __restrict__ out_count, int32_t* __restrict__ exact_list,
                                                RefineCounters* __restrict__ ctr, const float* __restrict__ tau, float inv_scale2,
                                                int pilot, uint32_t spill_cap, uint2* __restrict__ spill, const FinishArgs fin) {
    refine_block<MAY_SPILL>((int)blockIdx.x, spill, spill_cap, cand, cntw, n_streams, capw, list_cap, k, two_e, two_e_q, qhat, master, dim,
                            row_base, row_map, out_score, out_row, out_count, exact_list, ctr, tau, inv_scale2, pilot);
    finish_if_last(fin);
}

// K5b as a kernel (the per-query work is select_dense_query, k_rows.hpp): the last launch of an exact-path search ends it
__global__ __launch_bounds__(1024) void k_select_dense(const float* __restrict__ scores, int64_t rows,
                                                       const int32_t* __restrict__ q_list, int k, int64_t row_base,
                                                       const int64_t* __restrict__ row_map,
                                                       float* __restrict__ out_score, int64_t* __restrict__ out_row,
                                                       int32_t* __restrict__ out_count, unsigned long long* __restrict__ t_last,
                                                       const FinishArgs fin) {
    select_dense_query(scores, rows, q_list, k, row_base, row_map, out_score, out_row, out_count, t_last);
    finish_if_last(fin);
}

// Second chance for queries whose candidate segments overflowed: their raw vectors are gathered into a small batch
// (one wave per query) ...
__global__ __launch_bounds__(256) void k_gather_queries(const float* __restrict__ queries, const int32_t* __restrict__ list, int m,
                                                        int dim, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (i >= m) return;
    const float4* src = reinterpret_cast<const float4*>(queries + (int64_t)list[i] * dim);
    float4* dst = reinterpret_cast<float4*>(out + (int64_t)i * dim);
    for (int g = lane; g < (dim >> 2); g += 64) dst[g] = src[g];
}
// ... and the batch's answers are put back where those queries belong
__global__ __launch_bounds__(256) void k_scatter_topk(const float* __restrict__ s, const int64_t* __restrict__ r,
                                                      const int32_t* __restrict__ c, const int32_t* __restrict__ list, int m, int k,
                                                      float* __restrict__ out_score, int64_t* __restrict__ out_row,
                                                      int32_t* __restrict__ out_count) {
    const int i = blockIdx.x;
    if (i >= m) return;
    const int64_t q = list[i];
    for (int j = threadIdx.x; j < k; j += blockDim.x) {
        out_score[q * k + j] = s[(int64_t)i * k + j];
        out_row[q * k + j] = r[(int64_t)i * k + j];
    }
    if (threadIdx.x == 0) out_count[q] = c[i];
}

// C1. merge n_parts partial top-k lists per query. One block per query; n_parts*k <= MERGE_MAX.
// part p of each array starts stride_* ELEMENTS after part p-1 (contiguous [n_parts][nq][k] arrays, or the
// packed all-gather receive buffer).
constexpr int MERGE_MAX = 4096;
__global__ __launch_bounds__(256) void k_merge(const float* __restrict__ part_score, const int64_t* __restrict__ part_row,
                                               const int32_t* __restrict__ part_count, int64_t stride_s, int64_t stride_r,
                                               int64_t stride_c, int n_parts, int64_t nq, int k,
                                               float* __restrict__ out_score, int64_t* __restrict__ out_row,
                                               int32_t* __restrict__ out_count, const int32_t* __restrict__ part_flags = nullptr,
                                               int64_t stride_f = 0, unsigned long long* __restrict__ sig_word = nullptr,
                                               unsigned long long sig_seq = 0) {
    // rdx_signal: the first block tells the host, before it merges anything, whether some rank's partial carried the
    // "incomplete" flag (one 64-bit word, sequence number and value together: nothing to order)
    if (sig_word && blockIdx.x == 0 && threadIdx.x == 0) {
        int any = 0;
        for (int p = 0; p < n_parts; ++p) any |= part_flags[(int64_t)p * stride_f] != 0;
        __hip_atomic_store(sig_word, (sig_seq << 1) | (unsigned long long)any, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    __shared__ float s_s[MERGE_MAX];
    __shared__ int64_t s_r[MERGE_MAX];
    __shared__ int base[65];
    const int64_t q = blockIdx.x;
    if (threadIdx.x == 0) {
        int acc = 0;
        for (int p = 0; p < n_parts; ++p) {
            base[p] = acc;
            int c = part_count[(int64_t)p * stride_c + q];
            acc += c < 0 ? 0 : (c > k ? k : c);
        }
        base[n_parts] = acc;
    }
    __syncthreads();
    // one thread per (part, slot): every load of the gather in flight at once (part after part, k threads at a time, it was
    // n_parts dependent round trips)
    for (int t = threadIdx.x; t < n_parts * k; t += blockDim.x) {
        const int p = t / k, i = t - p * k;
        if (i < base[p + 1] - base[p]) {
            s_s[base[p] + i] = part_score[(int64_t)p * stride_s + q * k + i];
            s_r[base[p] + i] = part_row[(int64_t)p * stride_r + q * k + i];
        }
    }
    __syncthreads();
    rank_and_write(s_s, s_r, base[n_parts], k, out_score + q * k, out_row + q * k, out_count + q);
}

// C1b. merge of TWO partial lists per query when n_parts * k exceeds what k_merge ranks in LDS (k > 2048 with two parts, ...):
// both lists are sorted (score desc, row asc) and no row occurs twice (row ids are global), so an element's place in the merged
// list is its index in its own list plus the number of elements of the other list that come before it — one binary search per
// element, no LDS. rdx_merge_topk folds the parts through this kernel one after the other. out must not alias a or b.
__global__ __launch_bounds__(256) void k_merge_pair(const float* __restrict__ a_s, const int64_t* __restrict__ a_r,
                                                    const int32_t* __restrict__ a_c, const float* __restrict__ b_s,
                                                    const int64_t* __restrict__ b_r, const int32_t* __restrict__ b_c, int k,
                                                    float* __restrict__ out_score, int64_t* __restrict__ out_row,
                                                    int32_t* __restrict__ out_count) {
    const int64_t q = blockIdx.x;
    const int na = min(max(a_c[q], 0), k), nb = min(max(b_c[q], 0), k);
    const float* as = a_s + q * k;
    const float* bs = b_s + q * k;
    const int64_t* ar = a_r + q * k;
    const int64_t* br = b_r + q * k;
    float* os = out_score + q * k;
    int64_t* orow = out_row + q * k;
    for (int t = threadIdx.x; t < na + nb; t += blockDim.x) {
        const bool from_a = t < na;
        const int i = from_a ? t : t - na;
        const float s = from_a ? as[i] : bs[i];
        const int64_t r = from_a ? ar[i] : br[i];
        const float* xs = from_a ? bs : as;
        const int64_t* xr = from_a ? br : ar;
        int lo = 0, hi = from_a ? nb : na;   // first element of the other list that does NOT come before (s, r)
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            const float ms = xs[mid];
            const bool before = ms > s || (ms == s && xr[mid] < r);
            if (before) lo = mid + 1;
            else hi = mid;
        }
        const int pos = i + lo;
        if (pos < k) {
            os[pos] = s;
            orow[pos] = r;
        }
    }
    const int c = na + nb < k ? na + nb : k;
    for (int i = c + threadIdx.x; i < k; i += blockDim.x) {
        os[i] = -INFINITY;
        orow[i] = -1;
    }
    if (threadIdx.x == 0) out_count[q] = c;
}

}  // namespace rdx
