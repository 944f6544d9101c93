// search_plan.hpp — what a dense search launches, decided from explicit inputs: the user's search options (SearchOptions and their
// table, set_search_option), what finished searches fed back (SearchAdapt), and the index's shape (PlanShape) give a SearchPlan.
// No HIP include and no handle: a plain C++ compiler builds it, tests/c_abi/plan_dump.cpp prints its plans on the CPU, and
// tests/golden/search_plans.txt records them (DESIGN.md §4 "The search plan"). rdx_index.hip enqueues and completes what the plan says and reads
// options nowhere else.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/rdx.h"
#include "rdx_limits.hpp"

namespace rdx {

// the search options of rdx_index_set_option (include/rdx.h)
struct SearchOptions {
    int force_exact = 0, force_fast = 0, profile = 0, retry = 1, xcd_balance = 1, fuse_epilogue = 1, force_bn = 0;
    int half_boot = 1;       // 129..256 queries take their threshold sample as two 128-query tiles per sampled corpus tile
    int small_scan = 1;      // k_scan_small (split-K over all rows) as the main scan of small launches
    int split_boot = 1;      // k_boot (K loop split over the waves) for the threshold bootstrap of small launches
    int fuse_finish = 1;     // the end-of-search work runs in the last block of the search's last kernel (0: its own launch k_finish)
    int spec_tau = 1;        // speculative scan threshold (rank < k of the sample, verified by k_refine)
    int spread_boot = 1;     // a tile bootstrap (any not taken by k_boot) samples every div-th 32-row block instead of every div-th 256-row tile
    int coarse_i8 = 2;       // main scan on int8 MFMA — 0 never, 1 whenever the shape allows, 2 (default) large batches on large shards
    int refine_pilot = 4;    // int8 searches find their re-score band in two rounds — the pilot*k best coarse hits first, then what lies
                             // within E_q of their exact k-th score (refine_kernel.hpp); 0 = one band of 2E_q below c_k
    int i8_sample_mul = 0;   // how many times denser than the fp16 pass's an int8 search samples its threshold — 1, 2, 4, 8, or 0 (default):
                             // I8_AUTO_SAMPLE_MUL where int8 was chosen automatically (those searches spill), 8 where it was forced
    int i8_eps_classes = 0;  // classes of block error the int8 scan's emit threshold tells apart (k_eps_edges) — 1, 2, 4, 8, or 0 (default):
                             // I8_AUTO_EPS_CLASSES where int8 was chosen automatically, 1 where it was forced
    int refine_spill = 2;    // spill list (k_refine<true>) for queries with more hits than the LDS list — 0 never, 1 always, 2 (default) where int8
                             // was chosen automatically
    int refine_list = 0;     // developer option: upper bound on the LDS list's entries (>= 32), 0 = automatic
    int spill_cap = 0;       // developer option: upper bound on the spill list's entries per query (>= 32), 0 = SPILL_CAP
    int sample_div = 64;
    int64_t cand_cap = 0;    // 0 = automatic
};

// what finished searches feed back to the next plans (rdx_index.hip adapt_sampling, reweight_xcds, enqueue_scan)
struct SearchAdapt {
    int dense_sample = 0;    // searches left with a threshold sample twice as dense (set when a search emitted 3x a random corpus' candidates)
    int spec_backoff = 0;    // searches left during which the provable threshold is used (set when a speculation failed)
    int i8_backoff = 0;      // searches left during which automatic choice (coarse_i8 = 2) keeps the fp16 pass (set when an int8 search
                             // sent more than 1 in 64 of its queries to the fallback passes: rows too crowded for its band, see adapt_sampling)
    double xw[8] = {1, 1, 1, 1, 1, 1, 1, 1};   // relative speed of the XCDs as the last main scans showed it (sum 8)
};

// what the plan needs to know of the index
struct PlanShape {
    int64_t rows = 0;
    int dim_pad = 0, ksteps = 0;   // ksteps = dim_pad / 64
    int n_cu = 256;
    float two_e = 0.f;             // 2E, the coarse pass's error band (DESIGN.md "error bound")
};

// What a search of (rows, nq, k, options) launches: every choice, made by plan_search before anything is enqueued
struct SearchPlan {
    int64_t nq = 0;
    int k = 0, depth = 0, nq_pad = 0;  // depth 0 = the caller's batch; 1 = the second-chance batch of overflowed queries
    int prof = 0;                      // option "profile" (depth 0 only)
    bool retry = false;                // option "retry": overflowed queries of the caller's batch get a second MFMA pass before the exact scan
    bool fuse_finish = false;          // option "fuse_finish": K6 rides in the last block of the search's last kernel
    bool exact_only = false;           // the exact full scan alone; the fields down to `stamps` are the MFMA path's
    int bn = 0, nqt = 0, grid = 0, G = 0, n_streams = 0, n_sets = 0;   // G workgroups per XCD and query tile, 8 G streams
    bool res = false;                  // the 64-query tile stays resident in LDS
    bool fused = false;                // option "fuse_epilogue" with an even number of k-steps: the fused k_scan<EPI_EMIT> variants, where the build has them
    int64_t n_tiles = 0, n_blocks32 = 0;
    bool use_boot = false;             // bootstrap: k_boot over boot_units 32-row blocks, or k_scan<EPI_SETMAX> (the rest)
    int64_t boot_units = 0;
    int boot_sets = 0, bn_b = 0, nqt_b = 0, n_sets_b = 0, div = 1, n_sets_used = 0;
    int64_t boot_tiles = 0, boot_wave_off = 0;   // the tile bootstrap's ScanParams n_tiles, wave_off, row_off, span
    int boot_row_off = 0, boot_span = 0;
    bool use_small = false;            // k_scan_small as the main scan
    bool i8 = false;                   // the main scan runs on the int8 copies (k_scan<..., I8>; DESIGN.md §5 "int8 coarse pass")
    bool i8_auto = false;              // ... chosen automatically (coarse_i8 = 2): the search adapt_sampling's int8 back-off judges
    int eps_classes = 1;               // ... with its emit thresholds in this many classes of block error (1: every block is charged eps_max)
    int64_t sample_rows = 0;
    double expected_per_query = 0.0;   // candidates per query a random corpus would emit with this sample
    uint32_t capw = 0, list_cap = 0;
    bool spill = false;                // queries with more than list_cap hits are answered from a list in HBM (k_refine<true>), not by the fallback
    uint32_t spill_cap = 0;            // entries of that list per query
    int pilot = 0;                     // option "refine_pilot" (k_refine)
    int k_sel = 0;                     // rank of the sampled score the threshold is taken from (< k: speculative)
    float slack = 0.f;
    bool balance = false;              // XCD-weighted split of the main scan's tiles
    int bulk_it = 0, xlo[9] = {};
    bool stamps = false;               // the main scan's workgroups stamp their times
    bool ride = false, big_copy = false;   // host results: with k_finish into pinned staging, or D2H copies
    size_t b_s = 0, b_r = 0, b_c = 0;  // result bytes: scores, rows, counts
};

constexpr int K_FAST_MAX = 256;   // larger k goes through the exact full scan

// Host callers (rdx_host.hpp HostOut): small results travel with the end-of-search kernel into pinned staging and are copied to the
// caller's buffers by the CPU once the mailbox says the search is complete; large ones use D2H copies.
constexpr size_t PIN_MAX = 256 * 1024;   // results up to this size ride with k_finish (one block writing over PCIe)

// Speculative threshold. The provable threshold is the k-th largest sampled score: k/S of the sample's
// quantile scale where the corpus' k-th score sits at k/N — with a 1.6 % sample and k = 10 that is 60x the hits one
// needs. The corpus' k-th score is ESTIMATED by the sample's j-th largest with j ~ k*S/N; taking the smallest j for
// which fewer than k rows of the corpus lie above it (with a factor 2 for the 2E band the verification needs) with
// probability <= 1e-7 per query (the count above the sample's j-th largest is N/S * Gamma(j)) cuts the hits 2-6x
// (c4: 890 -> ~430 per query, c3: 4500 -> ~700). k_refine verifies every query (c_k - 2E >= T); a failed one takes the
// fallback passes, which use rank k, and switches speculation off for the next searches (structured corpora, where
// "every div-th tile" is not a random sample; SearchAdapt::spec_backoff counts them down in enqueue_scan, after this read).
constexpr int I8_AUTO_SAMPLE_MUL = 2;   // (plan_search: the int8 sample where int8 is chosen automatically)
constexpr int I8_AUTO_EPS_CLASSES = EPS_CLASSES;   // (plan_search: classes of block error where int8 is chosen automatically)

inline int speculative_rank(const SearchOptions& o, const SearchAdapt& a, int64_t rows, int k, int depth, int64_t sample_rows) {
    if (!o.spec_tau || depth != 0 || a.spec_backoff != 0 || k <= 1) return k;
    const double lam = 2.0 * (double)k * (double)sample_rows / (double)std::max<int64_t>(rows, 1);
    double term = std::exp(-lam), cdf = term;   // P(Poisson(lam) <= j - 1)
    int j = 1;
    while (1.0 - cdf > 1e-7 && j < k) {
        term *= lam / j;
        cdf += term;
        ++j;
    }
    return std::min(k, j);
}

// bulk: what the slowest XCD should get, dealt interleaved to everybody (whole iterations of all streams);
// tail: the rest, one contiguous range per XCD holding what that XCD should get beyond the bulk
inline void plan_xcd_split(const SearchAdapt& a, SearchPlan* p) {
    const double wmin = *std::min_element(a.xw, a.xw + 8);
    p->bulk_it = (int)std::max<int64_t>(0, (int64_t)std::floor((double)p->n_tiles * wmin / 8.0 / p->G) - 1);
    const int64_t t0 = (int64_t)p->bulk_it * p->n_streams, tail = p->n_tiles - t0;
    double want[8], sum = 0;
    for (int x = 0; x < 8; ++x) sum += (want[x] = std::max(0.0, (double)p->n_tiles * a.xw[x] / 8.0 - (double)p->bulk_it * p->G));
    double acc = 0;
    for (int x = 0; x <= 8; ++x) {
        p->xlo[x] = (int)(t0 + std::llround((double)tail * (sum > 0 ? acc / sum : x / 8.0)));
        if (x < 8) acc += want[x];
    }
    p->xlo[8] = (int)p->n_tiles;
}

// Every decision of a search of nq (<= one launch) queries at `depth`, from the index's shape, the options and the feedback state
// alone: nothing else read, nothing written but *out and, with a code other than RDX_OK, *err. The internal checks fail here, before
// anything is enqueued.
inline int plan_search(const PlanShape& h, const SearchOptions& o, const SearchAdapt& a, int64_t nq, int k, int depth, bool host_out,
                       SearchPlan* out, std::string* err) {
    const auto fail = [err](int code, const char* msg) {
        *err = msg;
        return code;
    };
    SearchPlan& p = *out = SearchPlan{};
    p.nq = nq;
    p.k = k;
    p.depth = depth;
    p.nq_pad = (int)((nq + 255) / 256 * 256);
    p.prof = depth == 0 ? o.profile : 0;
    p.retry = o.retry != 0;
    p.fuse_finish = o.fuse_finish != 0;
    p.pilot = o.refine_pilot;
    // option fuse_epilogue (default on: +1 % at B = 1024 since the static wave priority went in): with an even
    // number of k-steps per tile the emit check of a tile rides with the first k-step of the next one
    p.fused = (h.ksteps & 1) == 0 && o.fuse_epilogue;
    p.b_s = (size_t)nq * k * 4;
    p.b_r = (size_t)nq * k * 8;
    p.b_c = (size_t)nq * 4;
    p.ride = host_out && p.b_s + p.b_r + p.b_c <= PIN_MAX;
    p.big_copy = host_out && !p.ride;

    // small problems and huge k are served by the exact full scan alone (one fp32 read of the corpus)
    // Round 2 re-measured the crossover (B = 4: exact path 0.060 / 0.099 / 0.129 ms at 24 k / 40 k / 60 k rows, MFMA path 0.081 / 0.085 /
    // 0.087): the exact path costs ceil(nq / 4) passes of (1.28 us per 1000 rows + 10 us) on top of what both paths share, the
    // MFMA path ~60 us more than that share whatever the size — and beyond 32 Ki rows the select no longer holds a score row in
    // registers. (The rule it replaces, nq * rows <= 4 M below 64 Ki rows, sent 64 queries x 60 k rows through 16 exact passes.)
    const int64_t exact_passes = (nq + 3) / 4;
    const bool small = h.rows <= 32768 && (double)exact_passes * ((double)h.rows * 1.28e-3 + 10.0) <= 60.0;   // (any size: 600 queries on 1000 rows are 150 passes)
    p.exact_only = o.force_exact || k > K_FAST_MAX || k == 0 || h.rows < 1 || (small && !o.force_fast);
    if (p.exact_only) return RDX_OK;

    // The main scan on int8 MFMA (twice the dot products per clock of fp16, half the bytes; DESIGN.md §5 "int8 coarse pass"): the
    // caller's batch only (not the second pass), in 256-query tiles, at most 8 k-steps of 128 dimensions (|D| < 2^24: exact in fp32).
    // Automatic (option 2): more than one query tile on a shard of at least 2^20 rows, where the MFMA rate decides the scan's time;
    // the bootstrap, the second pass and the exact scan stay fp16 / fp32.
    const bool i8_shape = depth == 0 && nq > 128 && h.dim_pad % 128 == 0 && h.dim_pad <= 1024 && o.force_bn == 0;
    p.i8_auto = i8_shape && o.coarse_i8 == 2 && a.i8_backoff == 0 && nq > 256 && h.rows >= ((int64_t)1 << 20);
    p.i8 = i8_shape && (o.coarse_i8 == 1 || p.i8_auto);
    // Queries with more hits than the LDS list are answered from a list in HBM (k_refine<true>) instead of the fallback passes: where
    // int8 was chosen automatically (option refine_spill = 2), or on every MFMA-path search (1). Everywhere else the plan is what it
    // was before the spill list existed, to the counter.
    p.spill = o.refine_spill == 1 || (o.refine_spill == 2 && p.i8_auto);
    // The int8 scan's emit threshold in classes of block error (DESIGN.md §5 "classes of eps_b"): by the same rule, where int8 was
    // chosen automatically at depth 0; a forced int8 search keeps the one threshold with eps_max unless option i8_eps_classes says
    // otherwise. Only the scan's hits change: segments, lists and the sample stay sized for one class.
    p.eps_classes = !p.i8 ? 1 : (o.i8_eps_classes ? o.i8_eps_classes : (p.i8_auto ? I8_AUTO_EPS_CLASSES : 1));
    p.spill_cap = p.spill ? (uint32_t)(o.spill_cap ? std::min(o.spill_cap, SPILL_CAP) : SPILL_CAP) : 0u;

    // queries per workgroup: 64 (tile resident in LDS), 128, 256. 257..384 queries run as three 128-query tiles rather than
    // one full and one half-empty 256-query tile (measured at 1M x 1024, B = 384: 0.78 vs 0.84 ms; tools/bn_sweep.py)
    p.bn = nq <= 64 ? 64 : (nq <= 128 ? 128 : ((nq > 256 && nq <= 384 && !p.i8) ? 128 : 256));
    if (o.force_bn && (nq + o.force_bn - 1) / o.force_bn <= 32) p.bn = o.force_bn;   // developer option: queries per workgroup
    p.nqt = (int)((nq + p.bn - 1) / p.bn);
    p.grid = std::max(8, h.n_cu / 8 * 8);
    const int wpx = p.grid / 8;
    if (p.nqt > wpx) return fail(RDX_ERR_STATE, "internal: query chunk larger than one scan launch");
    p.G = wpx / p.nqt;
    p.n_streams = 8 * p.G;
    if (p.n_streams > REFINE_STREAMS) return fail(RDX_ERR_STATE, "internal: more streams than the refine kernel gathers");
    p.n_sets = p.n_streams * SETS_PER_STREAM;
    p.n_tiles = (h.rows + 255) / 256;
    if (p.n_tiles * h.ksteps >= ((int64_t)1 << 31)) return fail(RDX_ERR_STATE, "shard too large for one scan launch");
    // the 64-query tile stays resident in LDS when all its k-step images fit (no DMA, no barrier in the main loop)
    p.res = p.bn == 64 && (size_t)h.ksteps * 8192 + 512 <= 160 * 1024 - 1024;
    // bootstrap sample: every div-th tile. More rows sampled = tighter tau = fewer hits; keep the expected hits
    // per query (~1.3 k rows/sample_rows) around 4000/... of the refine list and the sample >= max(64k, 8192) rows
    // Bootstrap geometry. 129..256 queries run their main scan as ONE 256-query tile per workgroup, but their bootstrap samples
    // ~130 tiles: as one tile per workgroup that is half the CUs working through 16 dependent k-steps of 64 KB each (36 us at
    // c3). As TWO 128-query tiles per sampled tile every CU works, a k-step moves 48 KB and takes 1.4 instead of 2.25 us
    // (DESIGN.md §10's table): option "half_boot" (default 1).
    p.bn_b = p.bn;
    p.nqt_b = p.nqt;
    int ns_b = p.n_streams;
    if (o.half_boot && p.bn == 256 && p.nqt == 1) {
        p.bn_b = 128;
        p.nqt_b = 2;
        ns_b = 8 * (wpx / 2);
    }
    p.n_sets_b = ns_b * SETS_PER_STREAM;
    const int64_t want_rows = std::max<int64_t>(64 * (int64_t)k, 8192);
    int div = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(o.sample_div, h.rows / want_rows), 3000 / std::max(k, 1)));
    if (depth > 0) div = std::max(1, div / 8);   // second chance: 8x denser sample -> a threshold that sees the cluster
    // A corpus whose last searches emitted far more candidates than a random corpus would (clustered rows: a query's neighbours are
    // one document's chunks, and a thin sample holds too few of them to place the threshold among them) gets twice the sample for a
    // while: +0.25 ms of bootstrap on a 10 M-row scan, against thousands of surplus candidates per query to gather and re-score
    // (measured, embedding-like corpus at c4: 19.6 -> 16.2 ms per batch; N(0,1) corpus: +1 %, which is why it is not the default).
    else if (a.dense_sample > 0 && div > 1) div = std::max(1, div / 2);
    // The int8 pass emits every row whose coarse score is within E_q (~0.6 sigma of a random corpus' scores at d = 1024) of the
    // threshold: a threshold closer to the corpus' k-th score pays for its sample many times over. Measured on c4 (the refine list
    // holds 7 168 hits): every 64th block 7 900 hits per query, 573 of 1 024 queries re-run; every 32nd 5 400 / 134; every 16th 2 600 /
    // 0; every 8th, 2 640 hits, 11.8 ms per batch (iid) and 5 000 hits, 12.4 ms (embedding-like). The factor is measured at d = 1024 only; E_q relative to the score spread depends on d (both
    // quantisation errors grow like the element spacing, the spread like 1/sqrt(d)), so at other widths it is a choice, not a derivation:
    // what protects those shapes is the fallback, and automatic choice backs off from int8 when it overflows (adapt_sampling).
    // With the spill list a long list costs a longer gather, not a second pass, and the pilot re-scores a few hundred rows whatever the
    // hit count: where int8 is chosen automatically (the searches that spill) the sample is I8_AUTO_SAMPLE_MUL times the fp16 pass's
    // instead of 8 (measured, profiles/i8_sample/ab_c4.txt). Option i8_sample_mul sets the factor for every int8 search.
    if (p.i8 && depth == 0) div = std::max(1, div / (o.i8_sample_mul ? o.i8_sample_mul : (p.i8_auto && p.spill ? I8_AUTO_SAMPLE_MUL : 8)));
    int64_t n_sched = (p.n_tiles + div - 1) / div;
    // whole rounds only: the bootstrap takes as long as its busiest stream, so 77 tiles on 64 streams cost two tiles' time for
    // 1.2 tiles' worth of threshold (a 1.25 M-row shard at B = 1024: 53 -> 27 us of a 2.26 ms search); thin the sample to the
    // last full round instead, as long as it keeps the rows asked for above
    if (n_sched > ns_b && n_sched % ns_b != 0) {
        const int64_t full = n_sched / ns_b * ns_b;
        const int div2 = (int)((p.n_tiles + full - 1) / full);
        if ((p.n_tiles + div2 - 1) / div2 * 256 >= want_rows) {
            div = div2;
            n_sched = (p.n_tiles + div - 1) / div;
        }
    }
    p.div = div;
    // The sample as every div-th 32-ROW BLOCK (option "spread_boot", default 1) instead of every div-th 256-row tile: the same number
    // of rows, eight times finer. Wave w of virtual tile j takes block (8 j + w) * div; the last virtual tile ends inside the corpus.
    // It replaces the whole-rounds schedule above (n_sched becomes the number of virtual tiles) and applies to every bootstrap that
    // k_boot does not take, whatever the batch size.
    p.n_blocks32 = (h.rows + 31) / 32;
    const int64_t n_virtual = ((p.n_blocks32 - 1) / div + 1) / 8;
    p.boot_tiles = p.n_tiles;
    p.boot_span = TILE_ROWS;
    if (o.spread_boot && n_virtual >= 1) {   // wave w of sampled entry j: block (8 j + w) * div (scan_kernel.hpp ScanParams::wave_off)
        n_sched = n_virtual;
        p.boot_wave_off = (int64_t)(div - 1) * h.ksteps * 4096;
        p.boot_row_off = (div - 1) * 32;
        p.boot_span = (7 * div + 1) * 32;
        p.boot_tiles = (n_virtual - 1) * (int64_t)div + 1;   // ceil(n_tiles / div) = n_virtual entries: the last block lies inside the corpus
    }
    p.sample_rows = n_sched * 256;
    p.n_sets_used = (int)std::min<int64_t>(ns_b, n_sched) * SETS_PER_STREAM;
    // Small launches (<= 64 queries and a sample of at most four 32-row blocks per CU): the split-K bootstrap k_boot — one
    // 32-row block per workgroup, the k-steps dealt to the waves — instead of a few whole tiles of 16 dependent k-steps on
    // a few CUs (scan_kernel.hpp K2b). Whole rounds of the CUs when more than one.
    p.boot_units = std::min<int64_t>(p.n_blocks32, n_sched * 8);
    if (p.boot_units > h.n_cu) p.boot_units = p.boot_units / h.n_cu * h.n_cu;
    p.use_boot = o.split_boot && p.bn == BOOT_BN && p.nqt == 1 && p.boot_units <= 4 * (int64_t)h.n_cu;
    // ... and the split-K main scan k_scan_small when the whole corpus is at most 32 such blocks per CU (scan_kernel.hpp K2c)
    p.use_small = o.small_scan && p.bn == BOOT_BN && p.nqt == 1 && h.ksteps <= 16 && p.n_streams == p.grid &&
                  p.n_blocks32 <= 32 * (int64_t)h.n_cu && p.n_blocks32 >= p.grid;
    if (p.use_boot) {
        p.sample_rows = p.boot_units * 32;
        p.boot_sets = (int)p.boot_units * 4;
        p.n_sets_used = p.boot_sets;
    }
    // slots per (query, stream) segment: 8x the expected hits, power of two, [32, 4096]
    double exp_hits = (1.5 * k * (double)h.rows / (double)std::max<int64_t>(p.sample_rows, 1) + k) / p.n_streams;
    // int8: the scan emits coarse + E_q >= T, E_q ~ 0.6 sigma of a random corpus' scores at d = 1024 — about 16x what the fp16 pass
    // would emit from the same sample (measured at 10 M x 1024 with the 8x denser sample above: 2 640 hits per query against 146;
    // DESIGN.md §5; a measured factor at d = 1024, not derived for other widths). The ratio falls as the sample thins — the E_q
    // band is a fixed width, the fp16 count grows with rows / sample_rows: 7 900 hits against 970 at every 64th block, a factor 8 —
    // so at the thinner samples x16 over-estimates: segments up to twice as long as needed (address space only), and the
    // dense_sample trigger below fires at up to 6x instead of 3x a random corpus' hits (profiles/i8_sample/ab_c4.txt).
    if (p.i8) exp_hits *= 16.0;
    p.expected_per_query = exp_hits * p.n_streams;
    // (slots cost address space, not bandwidth: only occupied slots are ever touched)
    // (nq_pad * n_streams is 65,536 whatever the batch: 1024 slots = 512 MiB, 4096 = 2 GiB of the 288)
    uint32_t capw = depth > 0 ? 4096 : 1024;
    while (capw < 4096 && capw < 8.0 * exp_hits) capw *= 2;
    if (o.cand_cap && depth == 0) capw = (uint32_t)std::min<int64_t>(o.cand_cap, 8191);
    // the scan addresses candidate slots with 32-bit indices (scan_kernel.hpp emit_block)
    if ((uint64_t)p.nq_pad * (uint64_t)p.n_streams * capw >= (1ull << 29)) return fail(RDX_ERR_STATE, "internal: candidate segments exceed the 32-bit slot index");
    p.capw = capw;
    p.k_sel = speculative_rank(o, a, h.rows, k, depth, p.sample_rows);
    // proven threshold: 2E below the k-th sampled score — plus, when the sample was summed in another order than the main scan
    // sums (k_boot), twice the fp32 accumulation bound, so that the verification (c_k - 2E >= T, with c_k from the main
    // scan's sums) cannot fail on a rounding difference between the two orders
    p.slack = h.two_e + ((p.use_boot != p.use_small) ? 2.0f * (float)h.dim_pad * 1.1920929e-7f : 0.0f);
    // The eight XCDs do not finish equal shares at the same time (measured on c4: the last XCD 1.1-1.7 ms after the
    // first of 16.5, always the same ones). Each XCD therefore gets a contiguous range of the tile schedule sized by
    // its speed in the previous main scans (from the workgroups' own time stamps, damped) — no coordination
    // inside the kernel, just a different static split. Large launches only.
    p.balance = o.xcd_balance && depth == 0 && p.n_tiles >= 1024 && p.grid <= 512;
    if (p.balance) plan_xcd_split(a, &p);
    p.stamps = (p.balance || p.prof == 3) && p.grid <= 512;   // (Mailbox::wg_times holds 1024 stamps)
    // LDS list of the gathered hits: 16x the expected count (heavy-tailed score distributions of structured corpora; a list overflow costs a second pass), at most REFINE_LIST
    uint32_t list_cap = 1024;
    while (list_cap < (uint32_t)REFINE_LIST && list_cap < 16.0 * exp_hits * p.n_streams) list_cap *= 2;
    p.list_cap = std::min<uint32_t>(list_cap, REFINE_LIST);
    if (o.refine_list) p.list_cap = std::min<uint32_t>(p.list_cap, (uint32_t)o.refine_list);
    return RDX_OK;
}

// What a threshold search (rdx_index_range) of nq queries with lists of max_results launches: the MAIN-SCAN half of what
// plan_search decides for (nq, k = max_results, depth 0), from the shape and the options alone — no feedback state is read, none is
// written. The user supplies the threshold, so nothing of a bootstrap is planned; the scan is the fp16 one (never int8), hit lists
// live in LDS (never spill), every tile is dealt with stride 1, no XCD split and no stamps. Filled: exact_only (the small /
// force_exact / force_fast rule), bn, nqt, grid, G, n_streams, res, fused, use_small, n_tiles, n_blocks32, capw, list_cap; the options
// force_exact, force_fast, force_bn, small_scan, fuse_epilogue, cand_cap and refine_list steer it as they steer a search.
// max_results only SIZES the segments: above K_FAST_MAX (where plan_search leaves the MFMA path) they are those of K_FAST_MAX times
// ceil(max_results / K_FAST_MAX), at most 4096 slots. The hit list is always the largest one, REFINE_LIST entries (option refine_list
// lowers it): plan_search sizes its list by the hits a SAMPLED threshold is expected to leave, which says nothing about a threshold the
// user chose, and a shorter list would only send queries to the exact scan that the kernel could have answered.
inline int plan_range(const PlanShape& h, const SearchOptions& o, int64_t nq, int max_results, SearchPlan* out, std::string* err) {
    SearchOptions oo = o;
    oo.coarse_i8 = 0;
    oo.refine_spill = 0;
    oo.profile = 0;
    oo.xcd_balance = 0;
    const int k_plan = std::min(max_results, K_FAST_MAX);
    SearchPlan s;
    const int rc = plan_search(h, oo, SearchAdapt{}, nq, k_plan, 0, false, &s, err);
    if (rc != RDX_OK) return rc;
    SearchPlan& p = *out = SearchPlan{};
    p.nq = nq;
    p.k = max_results;
    p.nq_pad = s.nq_pad;
    p.exact_only = s.exact_only;
    if (p.exact_only) return RDX_OK;
    p.bn = s.bn;
    p.nqt = s.nqt;
    p.grid = s.grid;
    p.G = s.G;
    p.n_streams = s.n_streams;
    p.res = s.res;
    p.fused = s.fused;
    p.use_small = s.use_small;
    p.n_tiles = s.n_tiles;
    p.n_blocks32 = s.n_blocks32;
    p.capw = s.capw;
    p.list_cap = o.refine_list ? std::min<uint32_t>(REFINE_LIST, (uint32_t)o.refine_list) : (uint32_t)REFINE_LIST;
    const int mul = (max_results + K_FAST_MAX - 1) / K_FAST_MAX;
    if (mul > 1 && !o.cand_cap) p.capw = (uint32_t)std::min<int64_t>((int64_t)s.capw * mul, 4096);
    return RDX_OK;
}

// ------------------------------------------------------------------------------------------------
// the option table
// ------------------------------------------------------------------------------------------------
// how a row takes its value
enum OptionKind {
    OPT_SWITCH,         // any value: stored as value != 0
    OPT_RANGE,          // lo .. hi
    OPT_ZERO_OR_RANGE,  // 0 or lo .. hi; the message ends with hi
    OPT_ZERO_OR_POW2,   // 0 or a power of two in lo .. hi
    OPT_CLAMP,          // a row with a message refuses what lies below lo; everything else is brought into lo .. hi
};

struct OptionRow {
    const char* name;
    int SearchOptions::*member;         // ... or, for the one 64-bit option,
    int64_t SearchOptions::*member64;
    OptionKind kind;
    int64_t lo, hi;
    const char* message;                // of RDX_ERR_INVALID
};

inline constexpr int64_t OPT_NO_LIMIT = INT64_MAX;

inline const OptionRow SEARCH_OPTIONS[] = {
    {"force_exact", &SearchOptions::force_exact, nullptr, OPT_SWITCH, 0, 1, nullptr},
    {"force_fast", &SearchOptions::force_fast, nullptr, OPT_SWITCH, 0, 1, nullptr},
    {"retry", &SearchOptions::retry, nullptr, OPT_SWITCH, 0, 1, nullptr},
    {"fuse_epilogue", &SearchOptions::fuse_epilogue, nullptr, OPT_SWITCH, 0, 1, nullptr},
    {"fuse_finish", &SearchOptions::fuse_finish, nullptr, OPT_SWITCH, 0, 1, nullptr},
    {"split_boot", &SearchOptions::split_boot, nullptr, OPT_SWITCH, 0, 1, nullptr},
    {"small_scan", &SearchOptions::small_scan, nullptr, OPT_SWITCH, 0, 1, nullptr},
    {"half_boot", &SearchOptions::half_boot, nullptr, OPT_SWITCH, 0, 1, nullptr},
    {"spread_boot", &SearchOptions::spread_boot, nullptr, OPT_SWITCH, 0, 1, nullptr},
    {"spec_tau", &SearchOptions::spec_tau, nullptr, OPT_SWITCH, 0, 1, nullptr},         // clears SearchAdapt::spec_backoff
    {"xcd_balance", &SearchOptions::xcd_balance, nullptr, OPT_SWITCH, 0, 1, nullptr},   // resets SearchAdapt::xw
    {"coarse_i8", &SearchOptions::coarse_i8, nullptr, OPT_RANGE, 0, 2,                  // clears SearchAdapt::i8_backoff
     "coarse_i8 must be 0 (never), 1 (whenever the shape allows) or 2 (automatic)"},
    {"refine_pilot", &SearchOptions::refine_pilot, nullptr, OPT_RANGE, 0, 64,
     "refine_pilot must be 0 (one band) or 1..64 (pilot of that many times k hits)"},
    {"i8_sample_mul", &SearchOptions::i8_sample_mul, nullptr, OPT_ZERO_OR_POW2, 1, 8, "i8_sample_mul must be 0 (automatic), 1, 2, 4 or 8"},
    {"i8_eps_classes", &SearchOptions::i8_eps_classes, nullptr, OPT_ZERO_OR_POW2, 1, EPS_CLASSES, "i8_eps_classes must be 0 (automatic), 1, 2, 4 or 8"},
    {"refine_spill", &SearchOptions::refine_spill, nullptr, OPT_RANGE, 0, 2, "refine_spill must be 0 (never), 1 (always) or 2 (automatic)"},
    {"refine_list", &SearchOptions::refine_list, nullptr, OPT_ZERO_OR_RANGE, 32, REFINE_LIST, "refine_list must be 0 (automatic) or 32.."},
    {"spill_cap", &SearchOptions::spill_cap, nullptr, OPT_ZERO_OR_RANGE, 32, SPILL_CAP, "spill_cap must be 0 (automatic) or 32.."},
    {"force_bn", &SearchOptions::force_bn, nullptr, OPT_ZERO_OR_POW2, 64, 256, "force_bn must be 0 (automatic), 64, 128 or 256"},
    {"profile", &SearchOptions::profile, nullptr, OPT_CLAMP, 0, 3, nullptr},
    {"sample_div", &SearchOptions::sample_div, nullptr, OPT_CLAMP, 1, 1 << 20, "sample_div must be >= 1"},
    {"cand_cap", nullptr, &SearchOptions::cand_cap, OPT_CLAMP, 0, OPT_NO_LIMIT,
     "cand_cap must be 0 (auto) or a positive slot count per (query, stream) segment"},
};

// rdx_index_set_option for every option of a search: RDX_OK, or RDX_ERR_INVALID with *err set and nothing changed
inline int set_search_option(SearchOptions& o, SearchAdapt& a, const char* name, int64_t value, std::string* err) {
    const std::string n(name);
    for (const OptionRow& r : SEARCH_OPTIONS) {
        if (n != r.name) continue;
        bool ok = true;
        switch (r.kind) {
        case OPT_SWITCH: value = value != 0; break;
        case OPT_RANGE: ok = value >= r.lo && value <= r.hi; break;
        case OPT_ZERO_OR_RANGE: ok = value == 0 || (value >= r.lo && value <= r.hi); break;
        case OPT_ZERO_OR_POW2: ok = value == 0 || (value >= r.lo && value <= r.hi && (value & (value - 1)) == 0); break;
        case OPT_CLAMP:
            ok = !r.message || value >= r.lo;
            value = std::min(std::max(value, r.lo), r.hi);
            break;
        }
        if (!ok) {
            *err = r.message + (r.kind == OPT_ZERO_OR_RANGE ? std::to_string(r.hi) : std::string());
            return RDX_ERR_INVALID;
        }
        if (r.member64) o.*r.member64 = value;
        else o.*r.member = (int)value;
        if (r.member == &SearchOptions::coarse_i8) a.i8_backoff = 0;
        if (r.member == &SearchOptions::spec_tau) a.spec_backoff = 0;
        if (r.member == &SearchOptions::xcd_balance)
            for (double& w : a.xw) w = 1.0;
        return RDX_OK;
    }
    *err = "unknown option '" + n + "'";
    return RDX_ERR_INVALID;
}

}   // namespace rdx
