// refine_kernel.hpp — K4: exact re-score + final ordering of the scan's candidates. k_refine (RefineParams) and k_select_dense
// (SelectParams, k_rows.hpp) each end a search. (C1's merge of per-shard partial results is merge_kernel.hpp.)
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

// Everything k_refine is told (FinishArgs apart), grouped by what reads it; refine_params (rdx_index.hip) fills it by name.
struct RefineParams {
    const uint2* cand; const uint32_t* cntw; int n_streams; uint32_t capw, list_cap;   // the scan's hit segments; entries of the LDS list
    // thresholds and bands: 2E of the fp16 pass, or [nq] 2 E_q of the int8 pass (else NULL); tau[q] * inv_scale2 = the scan's threshold
    // in score units (int8: tau_s and 1); option "refine_pilot"
    int k; float two_e; const float* two_e_q; const float* tau; float inv_scale2; int pilot;
    const float* qhat; MasterView master; int dim;   // the exact re-score: the normalised queries [nq][dim] against the master rows
    RowIds ids; TopkOut out;
    int32_t* exact_list; RefineCounters* ctr;        // queries handed to the fallback passes (RefineCounters::n_exact of them)
    uint32_t spill_cap; uint2* spill;                // MAY_SPILL: [nq_pad][spill_cap] in HBM
};

// One block's query: its m > 0 hits (counted and prefixed in L.seg_off by refine_block) live in `list`, in LDS or in its spill row.
struct RefineQuery { RefineLds& L; uint2* list; uint32_t m; int q; };

// The stages of refine_list, in the order it calls them (DESIGN.md §5 has the table and the measurements behind each).
// gather: one thread per ENTRY — its segment is the last w with seg_off[w] <= i (binary search of the prefix in LDS), so every
// thread has loads in flight and none depends on another. The entries keep their order: segment after segment.
__device__ __forceinline__ void gather_hits(const RefineParams& p, const RefineQuery& c) {
    const uint32_t* const seg_off = c.L.seg_off;
    for (uint32_t i = threadIdx.x; i < c.m; i += blockDim.x) {
        int lo = 0, hi = p.n_streams;                       // seg_off[lo] <= i < seg_off[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (seg_off[mid] <= i) lo = mid;
            else hi = mid;
        }
        c.list[i] = p.cand[((int64_t)c.q * p.n_streams + lo) * p.capw + (i - seg_off[lo])];
    }
    __syncthreads();
}

// threshold: the rank-th largest coarse score of the hits; a query whose threshold cannot be verified goes to the fallback passes
__device__ __forceinline__ float coarse_kth(const RefineQuery& c, int64_t rank) {
    const uint2* const list = c.list;
    int64_t n_gt;
    return key2f(block_kth_largest([&](int64_t i) { return f2key(__uint_as_float(list[i].x)); }, c.m, rank, c.L.hist, c.L.bc, &n_gt));
}
__device__ __forceinline__ void to_fallback(const RefineParams& p, int q) {
    if (threadIdx.x == 0) {
        atomicAdd(&p.ctr->spec_fail, 1);
        p.exact_list[atomicAdd(&p.ctr->n_exact, 1)] = q;
    }
}
// The int8 pass is verified AFTER the exact re-score, against the exact k-th score X of the hits: complete iff X - E_q >= tau
// (with E_q ~14x the fp16 E, c_k - 2E >= tau would reject most speculative thresholds). False: left for the fallback.
__device__ __forceinline__ bool verify_exact(const RefineParams& p, int q, float tq, uint32_t kth_key) {
    if (!p.two_e_q || !(tq > -INFINITY) || key2f(kth_key) - 0.5f * p.two_e_q[q] >= tq) return true;
    to_fallback(p, q);
    return false;
}

// collect: rows of the hits with lo <= coarse < hi are appended to s_r (n_p counts them all, the arrays take the first REFINE_PMAX)
__device__ __forceinline__ void reset_count(RefineLds& L) {
    if (threadIdx.x == 0) L.n_p = 0;
    __syncthreads();
}
__device__ __forceinline__ int collect_band(const RefineQuery& c, float lo, float hi) {
    for (uint32_t i = threadIdx.x; i < c.m; i += blockDim.x) {
        const uint2 e = c.list[i];
        const float cs = __uint_as_float(e.x);
        if (cs >= lo && cs < hi) {
            const int pos = atomicAdd(&c.L.n_p, 1);
            if (pos < REFINE_PMAX) c.L.s_r[pos] = (int64_t)e.y;
        }
    }
    __syncthreads();
    return c.L.n_p;
}

// re-score: one wave per candidate row, row_at(i) = its row, put(i, s) takes its exact score (the oracle's bits: exact_dot4)
template <class RowAt, class Put>
__device__ __forceinline__ void rescore_rows(const RefineParams& p, int q, int cnt, RowAt row_at, Put put) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (int)(blockDim.x >> 6);
    const int dim = p.dim, n4 = dim >> 2;
    const float4* q4 = reinterpret_cast<const float4*>(p.qhat + (int64_t)q * dim);
    if (n4 <= 256) {
        // dim <= 1024: the query sits in registers (converted once per block, not once per candidate), a row's four 1 KiB pieces
        // are requested together and the NEXT candidate's pieces before this one is summed.
        const lane_groups<4> grp(lane, n4);
        float4 qf[4];                                       // (kept as floats, widened at use: 16 registers instead of 32)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float4 qq = q4[grp.gi[u]];
            qf[u] = grp.gv[u] ? qq : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        float4 cur[4], nxt[4];
        if (wave < cnt) grp.load(master_row(p.master, row_at(wave), dim), cur);
        for (int i = wave; i < cnt; i += nw) {
            grp.load(master_row(p.master, row_at(i + nw < cnt ? i + nw : i), dim), nxt);   // (the last one re-reads its own row: no branch around loads)
            double acc = 0.0;
#pragma unroll
            for (int u = 0; u < 4; ++u) exact_dot4(acc, qf[u], cur[u]);
            const float sx = (float)wave_sum(acc);
            if (lane == 0) put(i, sx);
#pragma unroll
            for (int u = 0; u < 4; ++u) cur[u] = nxt[u];
        }
        // (a third row in flight per wave — the loop is 9 dependent ~2 us round trips at c3 — needs 16 more registers than the
        //  1024-thread block has: 17 spilled. Measured instead: profiles/r04/refine_stamps.txt)
    } else {
        for (int i = wave; i < cnt; i += nw) {
            const float sx = exact_score(master_row(p.master, row_at(i), dim), q4, n4, lane);
            if (lane == 0) put(i, sx);
        }
    }
}

// rank: local -> returned row id (RowIds, rows_core.hpp), then the best k of the n entries of the ranking arrays (score desc, row asc)
__device__ __forceinline__ void rank_rows(const RefineParams& p, const RefineQuery& c, int n) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) c.L.s_r[i] = p.ids.of(c.L.s_r[i]);
    __syncthreads();
    rank_and_write(c.L.s_s, c.L.s_r, n, p.k, p.out.score + (int64_t)c.q * p.k, p.out.row + (int64_t)c.q * p.k, p.out.count + c.q);
}

// crowded band, the ranking arrays refilled: of the list's first n (exact score, row) what lies above the k-th key or ties with ~row >= rkey
__device__ __forceinline__ int take_reaching(const RefineQuery& c, int n, uint32_t kth, uint32_t rkey) {
    reset_count(c.L);
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const uint2 e = c.list[i];
        const uint32_t key = f2key_sel(__uint_as_float(e.x));
        if (key > kth || (key == kth && ~e.y >= rkey)) {
            const int at = atomicAdd(&c.L.n_p, 1);
            if (at < REFINE_PMAX) {
                c.L.s_s[at] = __uint_as_float(e.x);
                c.L.s_r[at] = (int64_t)e.y;
            }
        }
    }
    __syncthreads();
    return c.L.n_p;
}

// crowded band: n > REFINE_PMAX rows inside the band [lo, hi), more than the ranking arrays hold (near-duplicate rows stored together:
// a document's chunks). Its members are compacted to the front of the list, re-scored exactly in place (exact score over coarse
// score), the k-th largest exact score is found by the radix select, and only what reaches it is ranked. `done` entries of the
// ranking arrays (the pilot's S1, coarse >= hi) already hold their exact scores.
__device__ __forceinline__ void crowded_band(const RefineParams& p, const RefineQuery& c, float lo, float hi, int n, int done, float tq) {
    RefineLds& L = c.L;
    uint2* const list = c.list;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (int)(blockDim.x >> 6);
    // The list is compacted in rounds of 7 entries per thread (the LDS list is one round; a spill list takes up to
    // spill_cap / 7168): a round's members are written behind the earlier rounds' — at or below the round's own first entry, and
    // every entry up to the round's end was read before the barrier, so nothing unread is overwritten.
    int base_out = 0;
    for (uint32_t r0 = 0; r0 < c.m; r0 += 7u * blockDim.x) {
        uint2 mine[7];
        bool keep[7];
        int cnt = 0;
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            const uint32_t i = r0 + threadIdx.x * 7 + j;
            keep[j] = false;
            if (i < c.m) {
                mine[j] = list[i];
                const float cs = __uint_as_float(mine[j].x);
                keep[j] = cs >= lo && cs < hi;
            }
            cnt += keep[j] ? 1 : 0;
        }
        int incl = cnt;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int t = __shfl_up(incl, off, 64);
            if (lane >= off) incl += t;
        }
        if (lane == 63) L.wtot[wave] = incl;
        __syncthreads();                                          // (also: every thread has read its entries of this round)
        int pos = base_out + incl - cnt;
        for (int w = 0; w < wave; ++w) pos += L.wtot[w];
        for (int w = 0; w < nw; ++w) base_out += L.wtot[w];
#pragma unroll
        for (int j = 0; j < 7; ++j)
            if (keep[j]) list[pos++] = mine[j];
        __syncthreads();
    }
    // (two rounds: the n - done rows of S2 were compacted; S1, already exact in the ranking arrays, goes behind them — S1 and
    //  S2 are disjoint subsets of the m hits, so n <= m slots)
    for (int i = threadIdx.x; i < done; i += blockDim.x) list[n - done + i] = make_uint2(__float_as_uint(L.s_s[i]), (uint32_t)L.s_r[i]);
    rescore_rows(p, c.q, n - done, [&](int i) { return (int64_t)list[i].y; }, [&](int i, float sx) { list[i].x = __float_as_uint(sx); });
    __syncthreads();
    const int64_t kk2 = p.k < n ? p.k : n;
    int64_t n_gt2;
    // (selection keys, rows_core.hpp: +0.0 and -0.0 are one score — with f2key a k-th key of +0.0 left the -0.0 rows out of the ties)
    const uint32_t kth2 = block_kth_largest([&](int64_t i) { return f2key_sel(__uint_as_float(list[i].x)); }, n, kk2, L.hist, L.bc, &n_gt2);
    if (!verify_exact(p, c.q, tq, kth2)) return;
    // first EVERY tie (rkey = 0; the ranking orders them by row id): all there is to do unless identical rows fill the ranking arrays
    int n2 = take_reaching(c, n, kth2, 0u);
    if (n2 > REFINE_PMAX) {
        // > 1024 - k rows tie at the k-th score (identical rows; zeros of both signs): of the ties the kk2 - n_gt2 with the LOWEST
        // rows belong to the answer. The hits' rows are distinct 32-bit local rows (returned ids grow with them: RowIds), so that
        // many lowest rows are the keys ~row down to their (kk2 - n_gt2)-th largest — one more radix select (non-ties count as
        // key 0, below every ~row), then kk2 <= k entries are ranked.
        int64_t n_gt_r;
        const uint32_t rkey = block_kth_largest(
            [&](int64_t i) {
                const uint2 e = list[i];
                return f2key_sel(__uint_as_float(e.x)) == kth2 ? ~e.y : 0u;
            },
            n, kk2 - n_gt2, L.hist, L.bc, &n_gt_r);
        n2 = take_reaching(c, n, kth2, rkey);
    }
    rank_rows(p, c, n2);
}

// A query's hits are gathered into `list` and answered: the stages above, and the control flow of the two rounds. The list lives in
// LDS (SPILL = false) or in HBM (SPILL = true): the same statements, so which rows are re-scored does not depend on where it lives.
template <bool SPILL>
__device__ __forceinline__ void refine_list(const RefineParams& p, RefineLds& L, uint2* const list, const uint32_t m, const int q) {
    const RefineQuery c = {L, list, m, q};
    const int k = p.k;
    gather_hits(p, c);
    RDX_RSTAMP(2);
    const int64_t kk = (uint32_t)k < m ? k : m;
    const bool late = p.two_e_q != nullptr;                 // int8 coarse pass: verified after the re-score (verify_exact)
    bool two = late && p.pilot > 0;                         // two rounds: pilot S1, then the band below X1
    const int64_t k1 = (int64_t)p.pilot * k < (int64_t)m ? (int64_t)p.pilot * k : (int64_t)m;
    // lower edge of the first collection: c_k - 2E (one band), or c_k1 itself (S1)
    // (int8 coarse pass: the bound is the query's own, two_e_q[q] = 2 E_q, and tau is already in score units — DESIGN.md §5)
    float t2 = two ? coarse_kth(c, k1) : coarse_kth(c, kk) - (late ? p.two_e_q[q] : p.two_e);
    RDX_RSTAMP(3);
    // Verification of the scan's threshold T (score units). The hits are exactly the allowed rows with coarse >= T. The k best of
    // them have exact >= c_k - E, so the exact k-th best of the corpus is >= c_k - E and every true top-k row has coarse >=
    // c_k - 2E: all of those were emitted iff c_k - 2E >= T (and k hits exist at all). A threshold taken from k sampled rows
    // (k_tau with rank k) passes by construction; a SPECULATIVE one (rank < k: an estimate of where the corpus' k-th score
    // lies) passes unless the estimate was too high — then the query goes to the fallback passes, which use
    // the provable threshold. T = -inf (fewer than k sets sampled): every allowed row was emitted, nothing to verify.
    const float tq = p.tau[q] * p.inv_scale2;
    if (tq > -INFINITY && ((int64_t)m < (int64_t)k || (!late && t2 < tq))) {
        to_fallback(p, q);
        return;
    }
    reset_count(L);
    int n = collect_band(c, t2, INFINITY);
    if (two && n > REFINE_PMAX) {
        // more than the ranking arrays hold tie at the k1-th coarse score (identical rows): the single band, as without a pilot
        two = false;
        t2 = coarse_kth(c, kk) - p.two_e_q[q];
        reset_count(L);
        n = collect_band(c, t2, INFINITY);
    }
    int done = 0;                                           // entries of s_r / s_s that already hold their exact score (S1)
    float c1 = INFINITY;                                    // the band's upper edge: S1 (coarse >= c1) is not collected twice
    if (two) {
        rescore_rows(p, q, n, [&](int i) { return L.s_r[i]; }, [&](int i, float sx) { L.s_s[i] = sx; });
        __syncthreads();
        done = n;
        c1 = t2;
        // X1 = k-th largest exact score of S1; fewer than k rows in S1 (then S1 is every hit): no bound, the band is empty anyway.
        // t3 = X1 - E_q rounded DOWN (E_q = two_e_q / 2 is exact): every hit with coarse >= X1 - E_q is inside whatever the rounding
        t2 = -INFINITY;
        if (n >= k) {
            int64_t n_gt1;
            const uint32_t kx = block_kth_largest([&](int64_t i) { return f2key(L.s_s[i]); }, n, (int64_t)k, L.hist, L.bc, &n_gt1);
            t2 = sub_down(key2f(kx), 0.5f * p.two_e_q[q]);
        }
        n = collect_band(c, t2, c1);                        // S2 behind S1 (n_p goes on counting)
    }
    if (threadIdx.x == 0) atomicAdd(&p.ctr->rescored, (unsigned long long)n);
    if (n > REFINE_PMAX) {
        crowded_band(p, c, t2, c1, n, done, tq);
        return;
    }
    RDX_RSTAMP(4);
    rescore_rows(p, q, n - done, [&](int i) { return L.s_r[done + i]; }, [&](int i, float sx) { L.s_s[done + i] = sx; });
    __syncthreads();
    if (late) {
        int64_t n_gt3;
        const uint32_t kth3 = block_kth_largest([&](int64_t i) { return f2key(L.s_s[i]); }, n, (int64_t)(k < n ? k : n), L.hist, L.bc, &n_gt3);
        if (!verify_exact(p, q, tq, kth3)) return;
    }
    RDX_RSTAMP(5);
    rank_rows(p, c, n);
    RDX_RSTAMP(6);
}

// K4, one block per query: the hits are counted (segment sizes -> exclusive prefix), and the query takes one of three routes.
//   m <= list_cap, no segment overflowed: the list in LDS (refine_list<false>);
//   MAY_SPILL (the plan spills: SearchPlan::spill), m <= spill_cap, no segment overflowed: the block goes on IN THIS LAUNCH with its
//     row of the spill buffer as the list (refine_list<true>);
//   otherwise: the exact full scan (exact_list).
template <bool MAY_SPILL>
__device__ __forceinline__ void refine_block(const RefineParams& p, const int q) {
    extern __shared__ __attribute__((aligned(16))) char smem[];   // [list_cap] hits (the LDS list)
    __shared__ RefineLds L;
    uint32_t* const seg_off = L.seg_off;
    const int n_streams = p.n_streams;
    if (threadIdx.x == 0) L.overflow = 0;
    __syncthreads();
    RDX_RSTAMP(0);
    // segment sizes -> exclusive prefix. Wave 0 scans them 64 at a time with shuffles (n_streams <= 512: at most 8 rounds; the
    // serial loop this replaces was 3-5 us of the kernel at 256 streams)
    for (int w = threadIdx.x; w < n_streams; w += blockDim.x) {
        const uint32_t cw = p.cntw[(int64_t)q * n_streams + w];
        if (cw > p.capw) L.overflow = 1;
        seg_off[w + 1] = cw > p.capw ? p.capw : cw;
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
        atomicAdd(&p.ctr->emitted, (unsigned long long)m);
        atomicMax(&p.ctr->max_hits, (int)m);
    }
    bool to_spill = false;
    if (overflow || m > p.list_cap) {
        to_spill = MAY_SPILL && !overflow && m <= p.spill_cap;
        if (threadIdx.x == 0) {
            if (to_spill) atomicAdd(&p.ctr->n_spill, 1);
            else p.exact_list[atomicAdd(&p.ctr->n_exact, 1)] = q;
        }
        if (!to_spill) return;
    }
    if (m == 0 || p.k == 0) {
        rank_and_write(L.s_s, L.s_r, 0, p.k, p.out.score + (int64_t)q * p.k, p.out.row + (int64_t)q * p.k, p.out.count + q);
        return;
    }
    if constexpr (MAY_SPILL) {
        if (to_spill) {
            refine_list<true>(p, L, p.spill + (int64_t)q * p.spill_cap, m, q);
            return;
        }
    }
    refine_list<false>(p, L, reinterpret_cast<uint2*>(smem), m, q);
}

// A pointer into global memory, or NULL, as a value the compiler keeps (in SGPRs, or parked in a VGPR lane) instead of one it may
// load again from the kernel arguments wherever it is used. NULL stays NULL: both address spaces write it as 0, the casts change no bit.
template <class T>
__device__ __forceinline__ T* held_in_sgprs(T* ptr) {
    auto g = (__attribute__((address_space(1))) T*)ptr;
    asm volatile("" : "+s"(g));
    return (T*)g;
}
__device__ __forceinline__ int held_in_sgprs(int v) {
    asm volatile("" : "+s"(v));
    return v;
}

// MAY_SPILL = false: the kernel of every plan that does not spill, the LDS route alone (what k_refine was before the spill list).
// MAY_SPILL = true: both routes. The search's last kernel on the MFMA path for every plan.
template <bool MAY_SPILL>
__global__ __launch_bounds__(1024) void k_refine(const RefineParams args, const FinishArgs fin) {
    // The master view and dim are read from the kernel arguments ONCE, here: read through the struct at their uses, they were loaded
    // again (a scalar load and its wait) for every candidate row of the re-score loop: +1.7 % on k_refine at c4, profiles/refine_params.
    RefineParams p = args;
    p.master = MasterView{held_in_sgprs(args.master.f32), held_in_sgprs(args.master.raw16), held_in_sgprs(args.master.den)};
    p.dim = held_in_sgprs(args.dim);
    refine_block<MAY_SPILL>(p, (int)blockIdx.x);
    finish_if_last(fin);
}

// K5b as a kernel (the per-query work is select_dense_query, k_rows.hpp): the last launch of an exact-path search ends it
__global__ __launch_bounds__(1024) void k_select_dense(const SelectParams p, const FinishArgs fin) {
    select_dense_query(p);
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
// ... with their filter indices, when the search has a filter per query (padding entries: -1, no filter) ...
__global__ __launch_bounds__(256) void k_gather_filters(const int32_t* __restrict__ qf, const int32_t* __restrict__ list, int m, int m_pad,
                                                        int32_t* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m_pad) out[i] = i < m ? qf[list[i]] : -1;
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

}  // namespace rdx
