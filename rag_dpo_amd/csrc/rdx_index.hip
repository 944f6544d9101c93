// rdx_index.hip — the core unit of the dense index (struct rdx_index: rdx_index.hpp): its lifecycle, options and write path, rdx_l2_normalize,
// the search pipeline and its entry points, masks, the debug and statistics getters, and the threshold search, which is a variant of the
// pipeline (the main scan, then the k_range_* kernels built on k_refine's device code), and the grouped fill, which shares exact_score's long-row
// form with k_refine (rdx_index.hpp says why that keeps it here). The only unit that holds a k_scan kernel (rag_dpo_amd/build.py checks that).
// What is built ON an index and a search — MMR, clustering, k-means, value counts — is rdx_derived.hip; it reaches this unit through the host
// functions rdx_index.hpp declares: set_device, finish_pending, check_mask, check_own_rows, normalize_queries, gather_rows, exact_groups and
// range_chunk. The merge and the signal are rdx_merge.hip.
// The scans and the tail of a search are launched from parameter structs filled by name, each in one place whoever searches: main_scan_params fills
// ScanParams, refine_lists / refine_params k_refine's RefineParams, exact_params / select_params the exact path's, which for_exact_groups drives.
#include "rdx_index.hpp"

#include <cstddef>
#include <cstdio>
#include <memory>

#include "group_fill_kernel.hpp"
#include "k_rows.hpp"
#include "range_kernel.hpp"
#include "refine_kernel.hpp"
#include "scan_kernel.hpp"

int rdx::set_device(const rdx_index* h) {
    HIP_TRY(hipSetDevice(h->device));
    return RDX_OK;
}

static int grow(rdx_index* h, int64_t need_rows) {
    const RowStore& old = h->store;
    const GrowCaps caps = grow_caps(old.cap, need_rows);
    if (caps.roomy == old.cap) return RDX_OK;
    RowStore ns;
    ns.compact = old.compact;
    int64_t ncap = caps.roomy;
    hipError_t e = ns.alloc_rows(ncap, h->dim, h->dim_pad);
    if (e != hipSuccess && caps.tight < caps.roomy) e = ns.alloc_rows(ncap = caps.tight, h->dim, h->dim_pad);   // retry without head-room
    if (e != hipSuccess) return fail(RDX_ERR_NOMEM, std::string("growing index to ") + std::to_string(ncap) + " rows: " + hipGetErrorString(e));
    hipStream_t st = h->own_stream;
    if (old.row_map.p) {   // the id map grows with the rows: old entries kept, new ones start as local + row_base
        e = ns.alloc_ids();
        if (e != hipSuccess) return fail(RDX_ERR_NOMEM, std::string("growing the row id map: ") + hipGetErrorString(e));
        if (h->rows > 0) HIP_TRY(hipMemcpyAsync(ns.row_map.p, old.row_map.p, (size_t)h->rows * 8, hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL(k_iota64, dim3((unsigned)((ncap - h->rows + 255) / 256)), dim3(256), 0, st, ns.row_map.as<int64_t>(), h->rows, ncap - h->rows, h->row_base);
    }
    HIP_TRY(hipMemsetAsync(ns.shadow.p, 0, ns.shadow.bytes, st));
    if (h->rows > 0) {
        if (old.compact) {
            HIP_TRY(hipMemcpyAsync(ns.raw16.p, old.raw16.p, (size_t)h->rows * h->dim * 2, hipMemcpyDeviceToDevice, st));
            HIP_TRY(hipMemcpyAsync(ns.den.p, old.den.p, (size_t)h->rows * 8, hipMemcpyDeviceToDevice, st));
        } else {
            HIP_TRY(hipMemcpyAsync(ns.master.p, old.master.p, (size_t)h->rows * h->dim * 4, hipMemcpyDeviceToDevice, st));
        }
        HIP_TRY(hipMemcpyAsync(ns.shadow.p, old.shadow.p, old.shadow.bytes, hipMemcpyDeviceToDevice, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    h->store = std::move(ns);   // (ns leaves with the old arrays)
    return RDX_OK;
}

// ------------------------------------------------------------------------------------------------
// search: plan, enqueue, complete — ahead of the lifecycle because every call that writes to the index runs finish_pending first
// ------------------------------------------------------------------------------------------------
template <int BN, int EPI, bool RES, bool NTT = false, bool FUSED = false, bool I8 = false>
static int launch_scan(rdx_index* h, const ScanParams& p, int grid, hipStream_t st) {
    // LDS: query-image ring (or the whole resident query tile) + BN hit counters + BN thresholds
    const size_t lds = (size_t)(RES ? p.ksteps : RING_SLOTS) * BN * BK * 2 + BN * (I8 ? 8 + 4 * p.ncls : 8);   // (I8: BN query scales, a table per class)
    void (*kern)(const ScanParams) = p.allow ? k_scan<BN, EPI, true, RES, NTT, FUSED, I8> : k_scan<BN, EPI, false, RES, NTT, FUSED, I8>;
    RDX_TRY(dynamic_lds(h->device, (const void*)kern, lds));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), lds, st, p);
    HIP_TRY(hipGetLastError());
    return RDX_OK;
}

// ... with a filter per query (p.qf): BN bitmap pointers behind the thresholds. These kernels have no non-temporal and no fused variants
// (both are speed only): whatever the plan chose there, a filtered search takes the plain unfused kernel of its tile width.
template <int BN, int EPI, bool RES>
static int launch_scan_q(rdx_index* h, const ScanParams& p, int grid, hipStream_t st) {
    const size_t lds = (size_t)(RES ? p.ksteps : RING_SLOTS) * BN * BK * 2 + BN * 8 + BN * sizeof(const uint32_t*);
    void (*kern)(const ScanParams) = k_scan<BN, EPI, false, RES, false, false, false, true>;
    RDX_TRY(dynamic_lds(h->device, (const void*)kern, lds));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), lds, st, p);
    HIP_TRY(hipGetLastError());
    return RDX_OK;
}

template <int EPI>
static int launch_scan_bn(rdx_index* h, int bn, bool res, bool fused, const ScanParams& p, int grid, hipStream_t st) {
    if (p.qf) {
        if (bn == 64) return res ? launch_scan_q<64, EPI, true>(h, p, grid, st) : launch_scan_q<64, EPI, false>(h, p, grid, st);
        if (bn == 128) return launch_scan_q<128, EPI, false>(h, p, grid, st);
        return launch_scan_q<256, EPI, false>(h, p, grid, st);
    }
    // NTT (4th template argument): one query tile -> every corpus byte is read by exactly one workgroup -> non-temporal loads
    if (bn == 64) {
        if (p.nqt == 1) return res ? launch_scan<64, EPI, true, true>(h, p, grid, st) : launch_scan<64, EPI, false, true>(h, p, grid, st);
        return res ? launch_scan<64, EPI, true>(h, p, grid, st) : launch_scan<64, EPI, false>(h, p, grid, st);
    }
    if (bn == 128) return p.nqt == 1 ? launch_scan<128, EPI, false, true>(h, p, grid, st) : launch_scan<128, EPI, false>(h, p, grid, st);
    if constexpr (EPI == EPI_EMIT) {
#ifdef RDX_CHECK_BOUNDS
        constexpr bool HAVE_FUSED = false;   // the address-checking test build carries one more live value: no fused variants
#else
        constexpr bool HAVE_FUSED = true;
#endif
        // SearchPlan::fused: the emit check of a tile rides with the first k-step of the next one
        if constexpr (HAVE_FUSED) {
            if (fused) {
                if (p.nqt == 1) return launch_scan<256, EPI, false, true, true>(h, p, grid, st);
                return launch_scan<256, EPI, false, false, true>(h, p, grid, st);
            }
        }
    }
    if (p.nqt == 1) return launch_scan<256, EPI, false, true>(h, p, grid, st);   // one query tile: corpus read once -> nt loads
    return launch_scan<256, EPI, false>(h, p, grid, st);
}

// K5a for one group of ep.nq <= QX queries. Up to dim 1024 the register kernel with U = float4 groups per lane: queries in registers,
// two rows in flight per wave, 2 blocks per CU (all resident at once); the LDS kernel beyond
static int launch_exact_scores(const rdx_index* h, const ExactParams& ep, int grid_rows, hipStream_t st) {
    if (h->rows <= 0) return RDX_OK;
    const dim3 g_reg((unsigned)std::max<int64_t>(1, std::min<int64_t>((h->rows + 3) / 4, (int64_t)h->n_cu * 2)));
    dispatch_u(h->dim, [&](auto u) {
        constexpr int U = decltype(u)::value;
        void (*kern)(const ExactParams) = ep.qf ? k_exact_scores<true> : k_exact_scores<false>;   // (qf: a filter per query)
        if constexpr (U > 0) kern = ep.qf ? k_exact_scores_reg<U, true> : k_exact_scores_reg<U, false>;
        if constexpr (U > 0) hipLaunchKernelGGL(kern, g_reg, dim3(256), 0, st, ep);
        else hipLaunchKernelGGL(kern, dim3(std::max(grid_rows, 1)), dim3(256), (size_t)ep.nq * h->dim * 4, st, ep);
    });
    HIP_TRY(hipGetLastError());
    return RDX_OK;
}

// K5a's parameters for this index and the queries in qhat (q_list and nq: per group of QX queries, for_exact_groups)
static ExactParams exact_params(const rdx_index* h, const RowFilter& allow) {
    ExactParams ep = {};
    ep.master = h->mv();
    ep.rows = h->rows;
    ep.dim = h->dim;
    ep.qhat = h->qhat.as<float>();
    ep.allow = allow.allow;
    ep.ftab = allow.ftab;
    ep.qf = allow.qf;
    ep.out = h->dense.as<float>();
    return ep;
}

// K5b's parameters: the best k of each dense score row into `out` (q_list: per group)
static SelectParams select_params(const rdx_index* h, int k, const TopkOut& out) {
    SelectParams sel = {};
    sel.scores = h->dense.as<float>();
    sel.rows = h->rows;
    sel.k = k;
    sel.ids = RowIds{h->row_base, h->store.ids()};
    sel.out = out;
    return sel;
}

// The exact full scan for the queries listed in d_list[0..n_list), QX at a time: K5a leaves a group's scores in `dense`, then
// after(q_list, nq, last) launches what consumes them. t_first_inv: see run_exact.
template <class After>
static int for_exact_groups(rdx_index* h, const int32_t* d_list, int n_list, const RowFilter& allow, unsigned long long* t_first_inv, hipStream_t st, After after) {
    RDX_TRY(h->dense.ensure((size_t)QX * std::max<int64_t>(h->rows, 1) * 4));
    ExactParams ep = exact_params(h, allow);
    ep.t_first_inv = t_first_inv;
    const int grid_rows = (int)std::min<int64_t>((h->rows + 3) / 4, (int64_t)h->n_cu * 16);   // one row per wave up to 16 Ki rows
    for (int j0 = 0; j0 < n_list; j0 += QX) {
        ep.q_list = d_list + j0;
        ep.nq = std::min(QX, n_list - j0);
        RDX_TRY(launch_exact_scores(h, ep, grid_rows, st));
        after(ep.q_list, ep.nq, j0 + QX >= n_list);
        HIP_TRY(hipGetLastError());
    }
    return RDX_OK;
}

int rdx::exact_groups(rdx_index* h, const int32_t* d_list, int n_list, const RowFilter& allow, hipStream_t st,
                      const std::function<void(const int32_t*, int, bool)>& after) {
    return for_exact_groups(h, d_list, n_list, allow, nullptr, st, after);
}

// exact full scan for the queries listed in d_list[0..n_list)
static int run_exact(rdx_index* h, const int32_t* d_list, int n_list, int k, const RowFilter& d_allow, const TopkOut& out, hipStream_t st,
                     bool stamps = false, const FinishArgs* fin = nullptr) {
    const FinishArgs no_fin = {};   // (ctr == NULL: the launch does not end a search)
    // profile = 3: the scoring kernel's first block and the select kernel's last block leave their times in the counter block
    char* const ctr = stamps ? h->ctr.as<char>() : nullptr;
    const auto stamp = [&](size_t off) { return ctr ? reinterpret_cast<unsigned long long*>(ctr + off) : nullptr; };
    return for_exact_groups(h, d_list, n_list, d_allow, stamp(offsetof(RefineCounters, t_first_inv)), st, [&](const int32_t* q_list, int nq, bool last) {
        SelectParams sel = select_params(h, k, out);
        sel.q_list = q_list;
        sel.t_last = stamp(offsetof(RefineCounters, t_last));
        hipLaunchKernelGGL(k_select_dense, dim3(nq), dim3(1024), 0, st, sel, (fin && last) ? *fin : no_fin);
    });
}

// the wait policy of wait_word (rdx_host.hpp)
extern "C" int rdx_set_wait_policy(int spin_us, int sleep_us) {
    if (spin_us < 0 || sleep_us < 0 || sleep_us > 1000000) return fail(RDX_ERR_INVALID, "rdx_set_wait_policy: spin_us >= 0, 0 <= sleep_us <= 1000000");
    g_wait_spin_us.store(spin_us);
    g_wait_sleep_us.store(sleep_us);
    return RDX_OK;
}

// profile 1: an event behind every kernel; profile 2: events 3 and 4 only, around the dominant kernel(s)
static void mark(rdx_index* h, const SearchPlan& p, hipStream_t st, int i) {
    if (p.prof == 1 || (p.prof == 2 && (i == 3 || i == 4))) (void)hipEventRecord(h->ev[i], st);
}

// K6 (end of search): results of small host calls -> pinned staging, counters (+ workgroup stamps) -> mailbox, counter block
// re-zeroed, sequence number published. Runs in the last block of the search's last kernel (option fuse_finish, default) or
// as its own launch behind it.
static FinishArgs finish_args(const rdx_index* h, const SearchPlan& p, const SearchIO& io, unsigned long long seq) {
    FinishArgs f = {};
    f.ctr = h->ctr.as<RefineCounters>();
    f.mb = h->mbox.dev;
    f.seq = seq;
    f.wgt = p.stamps ? h->wgt.as<unsigned long long>() : nullptr;
    f.n_wgt = p.stamps ? 2 * p.grid : 0;
    f.s0 = reinterpret_cast<const uint32_t*>(io.row);
    f.d0 = reinterpret_cast<uint32_t*>(h->pin_out.dev);
    f.w0 = (int64_t)(p.ride ? p.b_r / 4 : 0);
    f.s1 = reinterpret_cast<const uint32_t*>(io.score);
    f.d1 = reinterpret_cast<uint32_t*>(h->pin_out.dev + p.b_r);
    f.w1 = (int64_t)(p.ride ? p.b_s / 4 : 0);
    f.s2 = reinterpret_cast<const uint32_t*>(io.count);
    f.d2 = reinterpret_cast<uint32_t*>(h->pin_out.dev + p.b_r + p.b_s);
    f.w2 = (int64_t)(p.ride ? p.b_c / 4 : 0);
    f.out_flags = io.flags;
    f.may_redo = (!p.exact_only && p.depth == 0) ? 1 : 0;
    return f;
}

// What k_refine and k_range_refine (RangeParams::r) are told alike: the plan's hit segments and list, the k best into `out`, and what the
// exact re-score reads. The fields of a top-k search's thresholds and bands stay zero: refine_params adds them.
static RefineParams refine_lists(const rdx_index* h, const SearchPlan& p, int k, const TopkOut& out) {
    RefineParams r = {};
    r.cand = h->cand.as<uint2>();
    r.cntw = h->cntw.as<uint32_t>();
    r.n_streams = p.n_streams;
    r.capw = p.capw;
    r.list_cap = p.list_cap;
    r.k = k;
    r.qhat = h->qhat.as<float>();
    r.master = h->mv();
    r.dim = h->dim;
    r.ids = RowIds{h->row_base, h->store.ids()};
    r.out = out;
    return r;
}

// what k_refine is told about a plan's search (refine_kernel.hpp RefineParams). An int8 search (p.i8) is refined against the
// bounds and thresholds k_tau8 left: 2 E_q per query, and tau_s, which is in score units already.
static RefineParams refine_params(const rdx_index* h, const SearchPlan& p, const SearchIO& io) {
    RefineParams r = refine_lists(h, p, p.k, TopkOut{io.score, io.row, io.count});
    r.two_e = h->two_e();
    r.pilot = p.pilot;
    r.two_e_q = p.i8 ? h->twoe8.as<float>() : nullptr;
    r.tau = p.i8 ? h->taus8.as<float>() : h->tau.as<float>();
    r.inv_scale2 = p.i8 ? 1.0f : std::ldexp(1.0f, -2 * h->scale_log2);
    r.exact_list = h->exact_list.as<int32_t>();
    r.ctr = h->ctr.as<RefineCounters>();
    r.spill_cap = p.spill_cap;
    r.spill = p.spill ? h->spill.as<uint2>() : nullptr;
    return r;
}

// The ScanParams of a plan's main scan. What its callers set differently are inputs: the `oob` word of the caller's counter block
// (RefineCounters, RangeCounters); the sets of a search's bootstrap and how many per query (a range search has none); xcd_ranges: the
// plan's use_xlo, bulk_it and xlo (a search: without them every stream is interleaved to its end); the workgroups' time stamps or NULL
static ScanParams main_scan_params(const rdx_index* h, const SearchPlan& p, const RowFilter& allow, int* oob, float* setmax, int n_sets,
                                   bool xcd_ranges, unsigned long long* wgt) {
    ScanParams sp = {};
    sp.shadow = h->store.shadow.as<_Float16>();
    sp.qshadow = h->qshadow.as<_Float16>();
    sp.ksteps = h->ksteps;
    sp.rows = h->rows;
    sp.n_tiles = p.n_tiles;
    sp.tile_stride = 1;
    sp.nqt = p.nqt;
    sp.nq_pad = p.nq_pad;
    sp.allow = allow.allow;
    sp.ftab = allow.ftab;
    sp.qf = allow.qf;
    sp.setmax = setmax;
    sp.n_sets = n_sets;
    sp.tau = h->tau.as<float>();
    sp.cntw = h->cntw.as<uint32_t>();
    sp.cand = h->cand.as<uint2>();
    sp.capw = p.capw;
    sp.inv_scale2 = std::ldexp(1.0f, -2 * h->scale_log2);
    if (xcd_ranges) {
        sp.use_xlo = p.balance ? 1 : 0;
        sp.bulk_it = p.bulk_it;
        std::copy(p.xlo, p.xlo + 9, sp.xlo);
    }
    sp.wgt = wgt;
    sp.shadow_bytes = (int64_t)h->store.shadow.bytes;
    sp.oob = oob;
    return sp;
}

// k_boot's and k_scan_small's share of a scan's parameters
static SplitKParams split_k_params(const ScanParams& sp, const SearchPlan& p) { return {sp.shadow, sp.qshadow, sp.ksteps, sp.rows, p.n_blocks32, sp.allow}; }

// The main scan of a plan: k_scan_small, or k_scan<EPI_EMIT> on the fp16 copies or (i8: a search whose plan chose them and prepare_i8 made
// them) on the int8 ones: 256-query tiles, several of them, so never the one-tile nt variants. The int8 k-steps are 128 dimensions wide, half
// as many as the plan counted: the fused variant needs THEIR number even (dim_pad a multiple of 256).
static int launch_main_scan(rdx_index* h, const SearchPlan& p, const ScanParams& sp, bool i8, hipStream_t st) {
    if (p.use_small) {
        const SmallScanParams ss = {split_k_params(sp, p), sp.tau, sp.cntw, sp.cand, sp.capw, sp.inv_scale2, sp.wgt, {sp.ftab, sp.qf}};
        hipLaunchKernelGGL(sp.qf ? k_scan_small<true> : k_scan_small<false>, dim3((unsigned)p.grid), dim3(512), 0, st, ss);
        HIP_TRY(hipGetLastError());
        return RDX_OK;
    }
    if (!i8) return launch_scan_bn<EPI_EMIT>(h, p.bn, p.res, p.fused, sp, p.grid, st);
    ScanParams s8 = sp;
    s8.shadow = reinterpret_cast<const _Float16*>(h->i8.c8.p);
    s8.qshadow = reinterpret_cast<const _Float16*>(h->qshadow8.p);
    s8.ksteps = h->dim_pad / 128;
    s8.tau = h->thr8.as<float>();
    s8.sblk = h->i8.sblk.as<float>();
    s8.qscale = h->tq8.as<float>();
    s8.cls = h->i8.cls8.as<uint32_t>();
    s8.ncls = p.eps_classes;
    s8.shadow_bytes = (int64_t)h->store.cap * h->dim_pad;
#ifndef RDX_CHECK_BOUNDS
    if (p.fused && (s8.ksteps & 1) == 0) return launch_scan<256, EPI_EMIT, false, false, true, true>(h, s8, p.grid, st);
#endif
    return launch_scan<256, EPI_EMIT, false, false, false, true>(h, s8, p.grid, st);
}

// the MFMA path of a plan: bootstrap (k_boot or k_scan<EPI_SETMAX>), k_tau, main scan (k_scan_small or k_scan<EPI_EMIT>), k_refine
static int enqueue_scan(rdx_index* h, const SearchPlan& p, const SearchIO& io, hipStream_t st, const FinishArgs& fin) {
    int* const oob = reinterpret_cast<int*>(h->ctr.as<char>() + offsetof(RefineCounters, oob));
    const ScanParams sp = main_scan_params(h, p, io.allow, oob, h->setmax.as<float>(), p.n_sets, true, p.stamps ? h->wgt.as<unsigned long long>() : nullptr);
    if (p.use_boot) {
        const BootParams bp = {split_k_params(sp, p), (int)p.boot_units, sp.setmax, p.boot_sets, {sp.ftab, sp.qf}};
        hipLaunchKernelGGL(sp.qf ? k_boot<true> : k_boot<false>, dim3((unsigned)p.boot_units), dim3(512), 0, st, bp);
        HIP_TRY(hipGetLastError());
    } else {   // the sample: the scan's parameters without XCD ranges and stamps, over the sampled tiles
        ScanParams pb = main_scan_params(h, p, io.allow, oob, sp.setmax, p.n_sets_b, false, nullptr);
        pb.tile_stride = p.div;
        pb.wave_off = p.boot_wave_off;
        pb.row_off = p.boot_row_off;
        pb.span = p.boot_span;
        pb.n_tiles = p.boot_tiles;
        pb.nqt = p.nqt_b;
        RDX_TRY(launch_scan_bn<EPI_SETMAX>(h, p.bn_b, p.bn_b == p.bn ? p.res : false, false, pb, p.grid, st));
    }
    mark(h, p, st, 2);
    if (p.depth == 0 && h->adapt.spec_backoff > 0) --h->adapt.spec_backoff;
    hipLaunchKernelGGL(k_tau, dim3(p.nq_pad), dim3(256), 0, st, h->setmax.as<float>(), p.use_boot ? p.boot_sets : p.n_sets_b, p.n_sets_used,
                       p.k_sel, p.k_sel == p.k ? p.slack * std::ldexp(1.0f, 2 * h->scale_log2) : 0.0f, (int)p.nq, h->tau.as<float>());
    HIP_TRY(hipGetLastError());
    if (p.i8) {
        hipLaunchKernelGGL(k_tau8, dim3((p.nq_pad + 255) / 256), dim3(256), 0, st, h->tau.as<float>(), std::ldexp(1.0f, -2 * h->scale_log2),
                           h->tq8.as<float>(), h->eq8.as<float>(), h->nq8.as<float>(), h->i8.eps8.as<unsigned int>(), (int)p.nq, p.nq_pad,
                           h->thr8.as<float>(), h->taus8.as<float>(), h->twoe8.as<float>(), h->i8.edge8.as<float>(), p.eps_classes);
        HIP_TRY(hipGetLastError());
    }
    mark(h, p, st, 3);
    RDX_TRY(launch_main_scan(h, p, sp, p.i8, st));
    mark(h, p, st, 4);
    // ONE launch, the search's last kernel on this path: a query with more hits than the LDS list holds goes on in its own block,
    // on its row of the spill buffer (plans that spill run the instantiation that holds both routes)
    const size_t lds = (size_t)p.list_cap * 8;
    const auto refine = p.spill ? k_refine<true> : k_refine<false>;
    RDX_TRY(dynamic_lds(h->device, (const void*)refine, lds));
    hipLaunchKernelGGL(refine, dim3((int)p.nq), dim3(1024), lds, st, refine_params(h, p, io), fin);
    HIP_TRY(hipGetLastError());
    mark(h, p, st, 5);
    return RDX_OK;
}

// int8 pass: bring the corpus copy up to date (blocks from the watermark on; the whole copy after an update, a compaction or a
// reallocation) and quantise the queries (from qhat, which k_refine re-scores with)
static int prepare_i8(rdx_index* h, const SearchPlan& p, hipStream_t st) {
    const int ks8 = h->dim_pad / 128;
    I8Copy& c = h->i8;
    RDX_TRY(c.ensure(h->store.cap, h->dim_pad));
    const I8Work w = c.mark.work(h->rows);
    if (w.nb > 0) {
        if (w.full) HIP_TRY(hipMemsetAsync(c.eps8.p, 0, 4, st));
        hipLaunchKernelGGL(k_quant8_corpus, dim3((unsigned)((w.nb + 3) / 4)), dim3(256), 0, st, h->mv(), h->dim, h->rows, w.b0, w.nb,
                           c.c8.as<int8_t>(), ks8, c.sblk.as<float>(), c.eps8.as<unsigned int>(), c.epsb.as<float>());
        HIP_TRY(hipGetLastError());
        // classes of block error: the edges from the eps_b of a full quantisation (on the stream: no host round trip); what an append
        // quantises is classified against the edges that stand (a block above the last stored edge lands in the top class, whose
        // edge is the running eps_max)
        if (w.full) {
            hipLaunchKernelGGL(k_eps_edges, dim3(EPS_CLASSES - 1), dim3(1024), 0, st, c.epsb.as<float>(), w.nb, c.edge8.as<float>());
            HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(k_eps_classify, dim3((unsigned)((w.nb + 255) / 256)), dim3(256), 0, st, c.epsb.as<float>(), w.b0, w.nb,
                           c.edge8.as<float>(), c.cls8.as<uint8_t>());
        HIP_TRY(hipGetLastError());
        c.mark.quantised(h->rows);
    }
    RDX_TRY(h->qshadow8.ensure((size_t)p.nq_pad * h->dim_pad));
    for (DevBuf* b : {&h->tq8, &h->eq8, &h->nq8, &h->taus8, &h->twoe8}) RDX_TRY(b->ensure((size_t)p.nq_pad * 4));
    RDX_TRY(h->thr8.ensure((size_t)p.eps_classes * p.nq_pad * 4));
    hipLaunchKernelGGL(k_quant8_query, dim3((p.nq_pad + 3) / 4), dim3(256), 0, st, h->qhat.as<float>(), p.nq, (int64_t)p.nq_pad, h->dim,
                       h->qshadow8.as<int8_t>(), ks8, h->tq8.as<float>(), h->eq8.as<float>(), h->nq8.as<float>());
    HIP_TRY(hipGetLastError());
    return RDX_OK;
}

// K1 on nq caller queries (rdx_index.hpp); the query form is instantiated here for rdx_derived.hip as well
template <bool QUERY>
int rdx::normalize_queries(rdx_index* h, const float* queries, int64_t nq, int64_t nq_pad, _Float16* qshadow, int* d_bad, int verbatim, hipStream_t st,
                           float* out) {
    hipLaunchKernelGGL(k_normalize<QUERY>, dim3((int)((std::max(nq, nq_pad) + 3) / 4)), dim3(256), 0, st, queries, (const uint16_t*)nullptr, nq,
                       h->dim, (const int64_t*)nullptr, (int64_t)0, MasterView{out ? out : h->qhat.as<float>(), nullptr, nullptr}, qshadow,
                       QUERY ? h->ksteps : 0, QUERY ? h->scale() : 1.0f, d_bad, nq_pad, verbatim);
    HIP_TRY(hipGetLastError());
    return RDX_OK;
}
template int rdx::normalize_queries<true>(rdx_index*, const float*, int64_t, int64_t, _Float16*, int*, int, hipStream_t, float*);

// the identity query list of an exact-only search, uploaded once (grow-only), not per search
static int ensure_iota(rdx_index* h, int nq_pad, hipStream_t st) {
    if ((size_t)nq_pad * 4 <= h->iota.bytes) return RDX_OK;
    RDX_TRY(h->iota.ensure((size_t)nq_pad * 4));
    const size_t cnt = h->iota.bytes / 4;
    std::vector<int32_t> io_list(cnt);
    for (size_t i = 0; i < cnt; ++i) io_list[i] = (int32_t)i;
    HIP_TRY(hipMemcpyAsync(h->iota.p, io_list.data(), cnt * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    return RDX_OK;
}

// Grow the scratch the plan needs and enqueue it, up to k_finish and the D2H copies of large host results; *seq: the search's number
static int enqueue_search(rdx_index* h, const SearchPlan& p, const SearchIO& io, const HostOut* ho, hipStream_t st,
                          unsigned long long* seq) {
    // K1 on the queries: qhat (fp32, exact re-score) + tiled fp16 copy (scan)
    RDX_TRY(h->qhat.ensure((size_t)p.nq_pad * h->dim * 4));
    RDX_TRY(h->qshadow.ensure((size_t)p.nq_pad * h->dim_pad * 2));
    static_assert(sizeof(RefineCounters) <= 64, "counter block layout: one 64-byte line");
    RDX_TRY(h->ctr.ensure(sizeof(RefineCounters)));
    RDX_TRY(h->exact_list.ensure((size_t)p.nq_pad * 4));
    if (!h->mbox.host) RDX_TRY(h->mbox.map(sizeof(Mailbox)));
    if (p.ride && !h->pin_out.host) RDX_TRY(h->pin_out.map(PIN_MAX));
    if (!p.exact_only) {
        RDX_TRY(h->tau.ensure((size_t)p.nq_pad * 4));
        RDX_TRY(h->cntw.ensure((size_t)p.nq_pad * p.n_streams * 4));
        RDX_TRY(h->cand.ensure((size_t)p.nq_pad * p.n_streams * p.capw * 8));
        RDX_TRY(h->setmax.ensure((size_t)p.nq_pad * std::max(std::max(p.n_sets, p.n_sets_b), p.boot_sets) * 4));
        if (p.stamps) RDX_TRY(h->wgt.ensure((size_t)p.grid * 16));
        if (p.spill) {
            RDX_TRY(h->spill.ensure((size_t)p.nq_pad * p.spill_cap * 8));
        }
    }
    if (!h->ctr_ready) {   // zeroed once; afterwards the k_finish of every search leaves it zeroed for the next one
        HIP_TRY(hipMemsetAsync(h->ctr.p, 0, sizeof(RefineCounters), st));
        h->ctr_ready = true;
    }
    int* d_bad = reinterpret_cast<int*>(h->ctr.as<char>() + offsetof(RefineCounters, bad));
    *seq = ++h->seq;
    mark(h, p, st, 0);
    // depth 1: the rows ARE normalised queries (gathered from qhat): kept bit for bit
    RDX_TRY(normalize_queries<true>(h, io.queries, p.nq, p.nq_pad, h->qshadow.as<_Float16>(), d_bad, p.depth > 0 ? 1 : 0, st));
    if (p.i8) RDX_TRY(prepare_i8(h, p, st));
    mark(h, p, st, 1);

    const FinishArgs fin = finish_args(h, p, io, *seq);
    if (p.exact_only) {
        for (int i = 2; i <= 3; ++i) mark(h, p, st, i);   // events 3..4 bracket the dominant kernels of this path too (K5a + K5b)
        RDX_TRY(ensure_iota(h, p.nq_pad, st));
        RDX_TRY(run_exact(h, h->iota.as<int32_t>(), (int)p.nq, p.k, io.allow, TopkOut{io.score, io.row, io.count}, st, p.prof == 3,
                          p.fuse_finish ? &fin : nullptr));
        for (int i = 4; i <= 5; ++i) mark(h, p, st, i);
    } else {
        RDX_TRY(enqueue_scan(h, p, io, st, p.fuse_finish ? fin : FinishArgs{}));
    }
    if (!p.fuse_finish) {
        hipLaunchKernelGGL(k_finish, dim3(1), dim3(1024), 0, st, fin);
        HIP_TRY(hipGetLastError());
    }
    // large host results: plain copies behind the last kernel (read_mailbox synchronises the stream for them)
    if (p.big_copy) RDX_TRY(copy_results_to_host(*ho, io.score, io.row, io.count, p.nq, p.k, st));
    return RDX_OK;
}

// what the host half keeps of the mailbox: a second-chance pass runs a nested search whose k_finish overwrites it
struct SearchCounts {
    unsigned long long emitted = 0, rescored = 0;
    int bad = 0, n_exact = 0;   // n_exact: queries left to the fallback passes (exact path: all of them)
    float stamp_ms = 0.f;       // profile = 3: first workgroup start -> last workgroup end of the dominant kernel(s)
};

// f(b) for every workgroup of the main scan that stamped its times (idle ones, wpx % nqt != 0, return before they stamp)
template <class F>
static void for_stamped(const SearchPlan& p, F f) {
    for (int b = 0; b < p.grid; ++b)
        if ((b >> 3) < p.G * p.nqt) f(b);
}

static int read_mailbox(rdx_index* h, const PendingSearch& ps, SearchCounts* c) {
    const SearchPlan& p = ps.plan;
    if (p.big_copy) HIP_TRY(hipStreamSynchronize(ps.st));   // pageable D2H copies: complete only after a stream synchronise
    const int rc = wait_word([&] { return __atomic_load_n(&h->mbox.host->seq, __ATOMIC_ACQUIRE) == ps.seq; }, ps.st);   // the ONE host wait of a search
    if (rc == 1) return fail(RDX_ERR_HIP, "internal: the search completed without publishing its mailbox");
    RDX_TRY(rc);
    const Mailbox& mb = *h->mbox.host;
    *c = {mb.emitted, mb.rescored, mb.bad, p.exact_only ? (int)p.nq : mb.n_exact};
    if (p.prof == 3) {
        if (p.exact_only) {
            if (mb.t_last > mb.t_first) c->stamp_ms = (float)((double)(mb.t_last - mb.t_first) * 1e-5);
        } else if (p.grid <= 512) {
            unsigned long long t0 = ~0ull, t1 = 0;
            for_stamped(p, [&](int b) {
                t0 = std::min(t0, mb.wg_times[2 * b]);
                t1 = std::max(t1, mb.wg_times[2 * b + 1]);
            });
            if (t1 > t0) c->stamp_ms = (float)((double)(t1 - t0) * 1e-5);
        }
    }
    return RDX_OK;
}

// the sampling state the next searches start from
static void adapt_sampling(rdx_index* h, const SearchPlan& p, const SearchCounts& c) {
    if (p.depth != 0) return;
    SearchAdapt& a = h->adapt;
    // Automatic int8 pass: its band is E_q wide (~0.6 sigma of a random corpus' scores at d = 1024). On rows that crowd around a
    // query's neighbours (a document's chunks) the hits can overflow the refine list and every such query pays the
    // fp16 second pass on top; when more than 1 in 64 queries of an int8 search did, the next 256 searches take the fp16 pass, after
    // which int8 is tried again. (Measured on the embedding-like c4 corpus: 5 000 hits per query, none re-run, int8 12.4 ms against
    // fp16 16.0 ms per batch — the safeguard is for corpora more crowded than that.)
    if (p.i8_auto && !p.exact_only) {
        if ((int64_t)c.n_exact * 64 > p.nq) a.i8_backoff = 256;
    } else if (a.i8_backoff > 0 && p.nq > 256) {
        --a.i8_backoff;
    }
    if (std::getenv("RDX_DEBUG_HITS"))   // developer (tools/ab_i8_sample.py): the longest hit list of the search and how many queries spilled
        std::fprintf(stderr, "hits max %d spilled %d\n", h->mbox.host->max_hits, h->mbox.host->n_spill);
    if (h->mbox.host->spec_fail > 0) a.spec_backoff = 64;   // a speculative threshold was too high: provable thresholds for a while
    // three times the candidates a random corpus would emit: the corpus is clustered — a denser threshold sample for the next searches
    // (plan_search; re-examined every 256 searches: the denser sample's own emission is what then keeps it on)
    if (!p.exact_only && p.expected_per_query > 0.0) {
        const double per_q = (double)c.emitted / (double)std::max<int64_t>(p.nq, 1);
        if (per_q > (a.dense_sample > 0 ? 1.5 : 3.0) * p.expected_per_query) a.dense_sample = 256;
        else if (a.dense_sample > 0) --a.dense_sample;
    }
}

// the stamps arrived with the counters: re-weight the XCD shares for the next search
static void reweight_xcds(rdx_index* h, const SearchPlan& p, rdx_search_stats* acc) {
    const unsigned long long* wt = h->mbox.host->wg_times;
    double* const xw = h->adapt.xw;
    unsigned long long t0 = ~0ull, tx[8] = {}, lo[8];
    std::fill(lo, lo + 8, ~0ull);
    for_stamped(p, [&](int b) {
        t0 = std::min(t0, wt[2 * b]);
        tx[b & 7] = std::max(tx[b & 7], wt[2 * b + 1]);
        lo[b & 7] = std::min(lo[b & 7], wt[2 * b + 1]);
    });
    double dur[8], mean = 0;
    for (int x = 0; x < 8; ++x) mean += (dur[x] = (double)(tx[x] - t0)) / 8.0;
    if (std::getenv("RDX_DEBUG_XCD")) {   // developer (tools/xcd_spread.py): when each XCD's last (first) workgroup ended, ms after the first start
        std::fprintf(stderr, "xcd end ms:");
        for (int x = 0; x < 8; ++x) std::fprintf(stderr, " %.3f(%.3f)", dur[x] * 1e-5, (double)(lo[x] - t0) * 1e-5);
        std::fprintf(stderr, "\n");
    }
    acc->xcd_finish_spread_ms = (float)((*std::max_element(dur, dur + 8) - *std::min_element(dur, dur + 8)) * 1e-5);   // 100 MHz ticks
    acc->xcd_share_min = (float)*std::min_element(xw, xw + 8);
    acc->xcd_share_max = (float)*std::max_element(xw, xw + 8);
    if (mean > 0) {
        double sum = 0;
        for (int x = 0; x < 8; ++x) {
            xw[x] *= std::sqrt(mean / std::max(dur[x], 1.0));   // damped: half the correction per search
            xw[x] = std::min(1.5, std::max(0.6, xw[x]));
            sum += xw[x];
        }
        for (int x = 0; x < 8; ++x) xw[x] *= 8.0 / sum;
    }
}

static int search_chunk(rdx_index* h, const SearchIO& io, int64_t nq, int k, hipStream_t st, rdx_search_stats* acc, int depth,
                        HostOut* ho, bool defer);

// The *n_exact queries whose candidate segments overflowed (listed in exact_list) get their results rewritten: by a second-chance
// search (caller's batch, option retry) or the exact full scan. *n_exact = the queries the exact scan served in the end.
static int redo_overflowed(rdx_index* h, const PendingSearch& ps, int* n_exact, rdx_search_stats* acc) {
    const SearchPlan& p = ps.plan;
    const hipStream_t st = ps.st;
    if (p.depth == 0 && p.retry) {
        // Overflow means "far more rows above the sampled threshold than expected": similar rows stored together
        // (chunks of one document) that the sparse sample missed. Before paying the exact full scan (one fp32 pass over
        // the corpus per 4 queries), give exactly these queries one more MFMA pass as a small, HBM-bound batch with a
        // denser sample and larger segments; what overflows again goes to the exact scan inside that call.
        const int m = *n_exact, kk = std::max(p.k, 1);
        RDX_TRY(h->r_list.ensure((size_t)m * 4));
        RDX_TRY(h->r_q.ensure((size_t)m * h->dim * 4));
        RDX_TRY(h->r_s.ensure((size_t)m * kk * 4));
        RDX_TRY(h->r_r.ensure((size_t)m * kk * 8));
        RDX_TRY(h->r_c.ensure((size_t)m * 4));
        HIP_TRY(hipMemcpyAsync(h->r_list.p, h->exact_list.p, (size_t)m * 4, hipMemcpyDeviceToDevice, st));
        // from the index's own normalised copy (qhat), not from the caller's buffer: an asynchronous caller may have reused
        // that since (include/rdx.h "Lifetimes"); the nested search stores these rows verbatim, so its scores have the same bits
        hipLaunchKernelGGL(k_gather_queries, dim3((m + 3) / 4), dim3(256), 0, st, h->qhat.as<float>(), h->r_list.as<int32_t>(), m, h->dim,
                           h->r_q.as<float>());
        HIP_TRY(hipGetLastError());
        RowFilter sub_allow = ps.io.allow;
        if (ps.io.allow.qf) {   // a filter per query: the batch's queries bring theirs along (padded to the nested search's 256)
            const int m_pad = (m + 255) / 256 * 256;
            RDX_TRY(h->r_qf.ensure((size_t)m_pad * 4));
            hipLaunchKernelGGL(k_gather_filters, dim3(m_pad / 256), dim3(256), 0, st, ps.io.allow.qf, h->r_list.as<int32_t>(), m, m_pad, h->r_qf.as<int32_t>());
            HIP_TRY(hipGetLastError());
            sub_allow = RowFilter(ps.io.allow.ftab, h->r_qf.as<int32_t>());
        }
        rdx_search_stats sub = {};
        const SearchIO sub_io = {h->r_q.as<float>(), sub_allow, h->r_s.as<float>(), h->r_r.as<int64_t>(), h->r_c.as<int32_t>(), nullptr};
        RDX_TRY(search_chunk(h, sub_io, m, p.k, st, &sub, 1, nullptr, false));
        hipLaunchKernelGGL(k_scatter_topk, dim3(m), dim3(64), 0, st, h->r_s.as<float>(), h->r_r.as<int64_t>(), h->r_c.as<int32_t>(),
                           h->r_list.as<int32_t>(), m, p.k, ps.io.score, ps.io.row, ps.io.count);
        HIP_TRY(hipGetLastError());
        acc->retried_queries += m;
        acc->emitted += sub.emitted;
        acc->rescored += sub.rescored;
        *n_exact = (int)sub.exact_queries;
    } else {
        RDX_TRY(run_exact(h, h->exact_list.as<int32_t>(), *n_exact, p.k, ps.io.allow, TopkOut{ps.io.score, ps.io.row, ps.io.count}, st));
    }
    if (ps.io.flags) HIP_TRY(hipMemsetAsync(ps.io.flags, 0, 16, st));   // the partial is complete now
    HIP_TRY(hipStreamSynchronize(st));   // rdx_search returns with the stream drained
    return RDX_OK;
}

// the search's counters and, with option "profile", its times into the caller's statistics
static int accumulate_stats(rdx_index* h, const SearchPlan& p, const SearchCounts& c, int n_exact, rdx_search_stats* acc) {
    if (p.prof == 1) HIP_TRY(hipEventSynchronize(h->ev[6]));
    acc->sample_rows += p.sample_rows;
    acc->emitted += (int64_t)c.emitted;
    acc->rescored += (int64_t)c.rescored;
    acc->exact_queries += n_exact;
    acc->path = p.exact_only ? 1 : 0;
    if (p.prof == 1) {
        float* const dst[6] = {&acc->ms_normalize, &acc->ms_scan_sample, &acc->ms_tau, &acc->ms_scan_main, &acc->ms_refine, &acc->ms_exact};
        for (int i = 0; i < 6; ++i) {
            float ms = 0;
            (void)hipEventElapsedTime(&ms, h->ev[i], h->ev[i + 1]);
            *dst[i] += ms;
        }
        acc->profiled = 1;
        float tot = 0;
        (void)hipEventElapsedTime(&tot, h->ev[0], h->ev[6]);
        acc->ms_total += tot;
    } else if (p.prof == 2) {
        float ms = 0;
        // non-exact path: both completed (the mailbox came after them in the stream). Exact path: ev[4] sits right behind the
        // kernel whose last block published the mailbox: wait for it (microseconds)
        if (p.exact_only) (void)hipEventSynchronize(h->ev[4]);
        (void)hipEventElapsedTime(&ms, h->ev[3], h->ev[4]);
        acc->profiled = 2;
        if (p.exact_only) acc->ms_exact += ms;   // exact path: K5a + K5b
        else acc->ms_scan_main += ms;
    } else if (p.prof == 3) {
        acc->profiled = 3;
        if (p.exact_only) acc->ms_exact += c.stamp_ms;
        else acc->ms_scan_main += c.stamp_ms;
    }
    return RDX_OK;
}

// the host half of a search (see PendingSearch). *redone (if given) = a fallback pass rewrote results after k_finish.
static int complete_search(rdx_index* h, const PendingSearch& ps, rdx_search_stats* acc, HostOut* ho, bool* redone) {
    const SearchPlan& p = ps.plan;
    if (redone) *redone = false;
    SearchCounts c;
    RDX_TRY(read_mailbox(h, ps, &c));
    adapt_sampling(h, p, c);
    if (h->mbox.host->oob) return fail(RDX_ERR_STATE, "internal: the scan computed a corpus address outside the scan copy (RDX_CHECK_BOUNDS build)");
    if (p.ride) {
        if (p.k > 0) {
            std::memcpy(ho->row, h->pin_out.host, p.b_r);
            std::memcpy(ho->score, h->pin_out.host + p.b_r, p.b_s);
        }
        std::memcpy(ho->count, h->pin_out.host + p.b_r + p.b_s, p.b_c);
    }
    int n_exact = c.n_exact;
    if (!p.exact_only) {
        const bool redo = n_exact > 0 && !c.bad;
        if (redo && redone) *redone = true;
        if (n_exact > 0 && ho) ho->stale = true;   // a fallback pass rewrites some of the rows copied above
        if (p.balance) reweight_xcds(h, p, acc);
        if (redo) RDX_TRY(redo_overflowed(h, ps, &n_exact, acc));
        acc->scan_main_launch_rows = h->rows;
        acc->scan_main_launch_queries = p.nq;
    }
    mark(h, p, ps.st, 6);
    if (c.bad) return fail(RDX_ERR_INVALID, "query embeddings contain NaN or Inf");
    return accumulate_stats(h, p, c, n_exact, acc);
}

// One launch of a search (nq <= 4096) at `depth`: plan, enqueue, and complete it unless `defer` (rdx_search_async: left in h->pending).
// The counter block is zeroed once and afterwards by the k_finish of every search. A search that leaves early (an internal
// check, allocation failure, launch error) may have skipped its k_finish: the next search zeroes the block itself again.
static int search_chunk(rdx_index* h, const SearchIO& io, int64_t nq, int k, hipStream_t st, rdx_search_stats* acc, int depth,
                        HostOut* ho, bool defer) {
    SearchPlan plan;
    unsigned long long seq = 0;
    std::string err;
    SearchOptions opt = h->opt;
    if (io.allow.qf) opt.coarse_i8 = 0;   // a filter per query: the int8 coarse pass knows one bitmap only (include/rdx.h rdx_search_filtered)
    int rc = plan_search(h->shape(), opt, h->adapt, nq, k, depth, ho != nullptr, &plan, &err);
    if (rc != RDX_OK) (void)fail(rc, err);
    if (rc == RDX_OK && depth == 0) h->coarse_bits = plan.exact_only ? 0 : (plan.i8 ? 8 : 16);
    if (rc == RDX_OK) rc = enqueue_search(h, plan, io, ho, st, &seq);
    if (rc == RDX_OK) {
        if (!plan.exact_only) acc->tau_rank = (float)plan.k_sel;
        const PendingSearch ps = {true, plan, io, st, seq, defer ? *acc : rdx_search_stats{}};
        if (defer) h->pending = ps;
        else rc = complete_search(h, ps, acc, ho, nullptr);
    }
    if (rc != RDX_OK) h->ctr_ready = false;
    return rc;
}

// run the host half of a search left pending by rdx_search_async (call with h->mu held)
int rdx::finish_pending(rdx_index* h, bool* redone) {
    if (redone) *redone = false;
    if (!h->pending.active) return RDX_OK;
    PendingSearch ps = h->pending;
    h->pending.active = false;
    RDX_TRY(set_device(h));
    h->stats = ps.stats;
    const int rc = complete_search(h, ps, &h->stats, nullptr, redone);
    if (rc != RDX_OK) h->ctr_ready = false;   // (see search_chunk)
    return rc;
}

// ------------------------------------------------------------------------------------------------
// library / lifecycle
// ------------------------------------------------------------------------------------------------
extern "C" int rdx_version(void) { return RDX_ABI_VERSION; }
extern "C" const char* rdx_last_error(void) { return g_err.c_str(); }

extern "C" int rdx_device_count(int* n) {
    if (!n) return fail(RDX_ERR_INVALID, "rdx_device_count: null pointer");
    HIP_TRY(hipGetDeviceCount(n));
    return RDX_OK;
}

static int check_dim(int dim) {
    if (dim <= 0 || dim % 4 != 0 || dim > MAX_DIM)
        return fail(RDX_ERR_INVALID, "dim must be a positive multiple of 4, at most " + std::to_string(MAX_DIM) + " (got " +
                                         std::to_string(dim) + ")");
    return RDX_OK;
}

extern "C" int rdx_index_create(int device, int dim, rdx_index** out) {
    if (!out) return fail(RDX_ERR_INVALID, "rdx_index_create: null out pointer");
    RDX_TRY(check_dim(dim));
    RDX_TRY(check_device("", device));
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
        return fail(RDX_ERR_STATE, std::string("librdx is built for gfx950 (MI355X) only; device reports ") + prop.gcnArchName);
    auto h = std::make_unique<rdx_index>();
    h->device = device;
    h->dim = dim;
    h->dim_pad = (dim + 63) / 64 * 64;
    h->ksteps = h->dim_pad / 64;
    h->scale_log2 = (int)std::lround(std::log2(std::sqrt((double)dim)));
    h->n_cu = prop.multiProcessorCount;
    const hipError_t e = hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking);
    if (e != hipSuccess) return fail(RDX_ERR_HIP, std::string("hipStreamCreate: ") + hipGetErrorString(e));
    *out = h.release();
    return RDX_OK;
}

// Both streams that may still hold work on the index's memory are drained; then the members free what they own.
extern "C" int rdx_index_destroy(rdx_index* h) {
    if (!h) return RDX_OK;
    const std::unique_ptr<rdx_index> owner(h);
    (void)hipSetDevice(h->device);
    if (h->pending.active) (void)hipStreamSynchronize(h->pending.st);   // an abandoned asynchronous search: let its kernels finish
    (void)hipStreamSynchronize(h->own_stream);
    if (h->ev_ok)
        for (auto& e : h->ev) (void)hipEventDestroy(e);
    (void)hipStreamDestroy(h->own_stream);
    return RDX_OK;
}

extern "C" int rdx_index_dim(const rdx_index* h, int* dim) {
    if (!h || !dim) return fail(RDX_ERR_INVALID, "rdx_index_dim: null pointer");
    *dim = h->dim;
    return RDX_OK;
}

extern "C" int rdx_index_count(const rdx_index* h, int64_t* rows) {
    if (!h || !rows) return fail(RDX_ERR_INVALID, "rdx_index_count: null pointer");
    *rows = h->rows;
    return RDX_OK;
}

extern "C" int rdx_index_reserve(rdx_index* h, int64_t rows) {
    if (!h || rows < 0) return fail(RDX_ERR_INVALID, "rdx_index_reserve: bad argument");
    std::lock_guard<std::mutex> lk(h->mu);
    RDX_TRY(set_device(h));
    return grow(h, rows);
}

extern "C" int rdx_index_set_option(rdx_index* h, const char* name, int64_t value) {
    if (!h || !name) return fail(RDX_ERR_INVALID, "rdx_index_set_option: null pointer");
    std::lock_guard<std::mutex> lk(h->mu);
    RDX_TRY(finish_pending(h, nullptr));   // the host half of an asynchronous search reads the options it was enqueued under
    const std::string n(name);
    if (n == "compact_master") {
        if (h->rows > 0 || h->store.cap > 0) return fail(RDX_ERR_STATE, "compact_master can only be chosen while the index is empty");
        h->store.compact = value != 0;
        return RDX_OK;
    }
    if (n == "row_base") {
        if (value < 0) return fail(RDX_ERR_INVALID, "row_base must be >= 0");
        h->row_base = value;
        return RDX_OK;
    }
    if (n == "dup_batch") {
        if (value < 0 || value > RANGE_CHUNK) return fail(RDX_ERR_INVALID, "dup_batch must be 0 (the range chunk) or 1.." + std::to_string(RANGE_CHUNK));
        h->dup_batch = (int)value;
        return RDX_OK;
    }
    if (n == "facet_table_kb") {
        if (value < 0 || value > ((int64_t)1 << 22)) return fail(RDX_ERR_INVALID, "facet_table_kb must be 0 (automatic) or 1..4194304");
        h->facet_table_kb = value;
        return RDX_OK;
    }
    if (n == "km_tiles") {
        if (value < 0 || value > 4096) return fail(RDX_ERR_INVALID, "km_tiles must be 0 (automatic) or 1..4096");
        h->km_tiles = (int)value;
        return RDX_OK;
    }
    std::string err;   // every other option is a search's (search_plan.hpp)
    const int rc = set_search_option(h->opt, h->adapt, name, value, &err);
    return rc == RDX_OK ? rc : fail(rc, err);
}

extern "C" int rdx_index_xcd_shares(rdx_index* h, double* out8, const double* in8) {
    if (!h) return fail(RDX_ERR_INVALID, "rdx_index_xcd_shares: null index");
    std::lock_guard<std::mutex> lk(h->mu);
    RDX_TRY(finish_pending(h, nullptr));
    if (in8) {
        double w[8], sum = 0;
        for (int x = 0; x < 8; ++x) {
            if (!(in8[x] > 0.0) || !(in8[x] < 100.0)) return fail(RDX_ERR_INVALID, "rdx_index_xcd_shares: shares must be positive finite numbers");
            sum += (w[x] = std::min(1.5, std::max(0.6, in8[x])));
        }
        for (int x = 0; x < 8; ++x) h->adapt.xw[x] = w[x] * 8.0 / sum;
    }
    if (out8)
        for (int x = 0; x < 8; ++x) out8[x] = h->adapt.xw[x];
    return RDX_OK;
}

// ------------------------------------------------------------------------------------------------
// ingest
// ------------------------------------------------------------------------------------------------
static const int64_t STAGE_ROWS = 32768;

// One pass of K1 over the call's n rows in chunks of STAGE_ROWS (host rows through the staging buffer). write: into master/shadow at
// the dst rows; otherwise only the verdict — K1 with no master and no scan copy stores nothing but the `bad` flag.
// *bad = a row of the call holds a NaN or an Inf.
static int normalize_pass(rdx_index* h, const void* rows, bool is_bf16, int64_t n, int space, int64_t row0, const int64_t* d_dst_ids,
                          bool verbatim, bool write, int* bad) {
    hipStream_t st = h->own_stream;
    const size_t esz = is_bf16 ? 2 : 4;
    const MasterView mv = write ? h->mv() : MasterView{nullptr, nullptr, nullptr};
    _Float16* const shadow = write ? h->store.shadow.as<_Float16>() : nullptr;
    RDX_TRY(h->bad.ensure(sizeof(int)));
    HIP_TRY(hipMemsetAsync(h->bad.p, 0, sizeof(int), st));
    for (int64_t off = 0; off < n; off += STAGE_ROWS) {
        const int64_t m = std::min(STAGE_ROWS, n - off);
        const char* src = reinterpret_cast<const char*>(rows) + (size_t)off * h->dim * esz;
        if (space == RDX_HOST) {
            RDX_TRY(h->staging.ensure((size_t)STAGE_ROWS * h->dim * 4));
            HIP_TRY(hipMemcpyAsync(h->staging.p, src, (size_t)m * h->dim * esz, hipMemcpyHostToDevice, st));
            HIP_TRY(hipStreamSynchronize(st));   // pageable source: keep the copy ordered with the caller's buffer
            src = h->staging.as<char>();
        }
        const int grid = (int)((m + 3) / 4);
        hipLaunchKernelGGL(k_normalize<false>, dim3(grid), dim3(256), 0, st, is_bf16 ? nullptr : (const float*)src,
                           is_bf16 ? (const uint16_t*)src : nullptr, m, h->dim, d_dst_ids ? d_dst_ids + off : nullptr,
                           row0 + off, mv, shadow, h->ksteps, h->scale(), h->bad.as<int>(), (int64_t)0, verbatim ? 1 : 0);
        HIP_TRY(hipGetLastError());
        if (space == RDX_HOST) HIP_TRY(hipStreamSynchronize(st));   // staging is reused by the next chunk
    }
    HIP_TRY(hipMemcpyAsync(bad, h->bad.p, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return RDX_OK;
}

// normalise n rows (host or device, fp32 or bf16) into master/shadow at dst rows (row0.. or dst_ids)
static int ingest(rdx_index* h, const void* rows, bool is_bf16, int64_t n, int space, int64_t row0, const int64_t* d_dst_ids,
                  bool verbatim = false) {
    // the int8 copy: an update may touch any block, an append the last partial one and the new ones
    if (d_dst_ids) h->i8.mark.rewritten();
    else h->i8.mark.appended(row0);
    if (space == RDX_DEVICE) HIP_TRY(hipDeviceSynchronize());   // the caller's producers of `rows` (any stream) are done
    int bad = 0;
    // An update writes over rows the index holds, and K1 stops only the wave of the bad row: the call's rows are judged first, so that
    // a refused update has written nothing (include/rdx.h). A refused append leaves its rows beyond the count, where no call reads.
    if (d_dst_ids) RDX_TRY(normalize_pass(h, rows, is_bf16, n, space, row0, d_dst_ids, verbatim, false, &bad));
    if (!bad) RDX_TRY(normalize_pass(h, rows, is_bf16, n, space, row0, d_dst_ids, verbatim, true, &bad));
    if (bad) return fail(RDX_ERR_INVALID, "embeddings contain NaN or Inf");
    return RDX_OK;
}

static int add_impl(rdx_index* h, const void* rows, bool is_bf16, int64_t n, int space, bool verbatim = false) {
    if (!h || (n > 0 && !rows) || n < 0) return fail(RDX_ERR_INVALID, "rdx_index_add: bad argument");
    RDX_TRY(check_space(space));
    if (n == 0) return RDX_OK;
    std::lock_guard<std::mutex> lk(h->mu);
    RDX_TRY(finish_pending(h, nullptr));
    if (h->store.compact && (!is_bf16 || verbatim))
        return fail(RDX_ERR_STATE, "this index keeps a compact master (raw bf16 rows + divisors): rows must arrive through rdx_index_add_bf16");
    RDX_TRY(set_device(h));
    RDX_TRY(grow(h, h->rows + n));
    RDX_TRY(ingest(h, rows, is_bf16, n, space, h->rows, nullptr, verbatim));
    h->rows += n;
    return RDX_OK;
}

extern "C" int rdx_index_add(rdx_index* h, const float* rows, int64_t n, int space) { return add_impl(h, rows, false, n, space); }
extern "C" int rdx_index_add_bf16(rdx_index* h, const uint16_t* rows, int64_t n, int space) {
    return add_impl(h, rows, true, n, space);
}
extern "C" int rdx_index_add_stored(rdx_index* h, const float* rows, int64_t n, int space) {
    return add_impl(h, rows, false, n, space, true);
}

// What a list of row ids must satisfy: every id in [0, limit) and, with `increasing`, above the one before it.
struct IdRule {
    int64_t limit;
    bool increasing;
};
enum class IdFault { none, range, order };

// the first fault of a host id list, *at = its position
static IdFault check_ids(const int64_t* ids, int64_t n, IdRule rule, int64_t* at) {
    for (int64_t i = 0; i < n; ++i) {
        *at = i;
        if (ids[i] < 0 || ids[i] >= rule.limit) return IdFault::range;
        if (rule.increasing && i > 0 && ids[i] <= ids[i - 1]) return IdFault::order;
    }
    return IdFault::none;
}

// the ids of rdx_index_update and rdx_index_get: rows the index holds
static int check_row_ids(const rdx_index* h, const int64_t* ids, int64_t n) {
    int64_t at = 0;
    if (check_ids(ids, n, IdRule{h->rows, false}, &at) != IdFault::none)
        return fail(RDX_ERR_INVALID, "row id " + std::to_string(ids[at]) + " out of range [0, " + std::to_string(h->rows) + ")");
    return RDX_OK;
}

// the ids of rdx_index_update*: each row at most once — two rows of one call for the same destination would be written by two waves
// at once, and the row could end up holding float4 groups of both
static int check_distinct_ids(const int64_t* ids, int64_t n) {
    std::vector<int64_t> s(ids, ids + n);
    std::sort(s.begin(), s.end());
    const auto dup = std::adjacent_find(s.begin(), s.end());
    if (dup != s.end()) return fail(RDX_ERR_INVALID, "row id " + std::to_string(*dup) + " is given more than once");
    return RDX_OK;
}

// A host or device int64 id list: checked on the host by check(host copy) — a device list is brought over for that — and made
// available on the device: a device list as it is, a host list through the scratch `ids`.
template <class Check>
static int stage_ids(rdx_index* h, const int64_t* ids, int64_t n, int space, Check check, const int64_t** d_ids) {
    hipStream_t st = h->own_stream;
    std::vector<int64_t> tmp;
    const int64_t* host_ids = ids;
    if (space == RDX_DEVICE) {
        HIP_TRY(hipDeviceSynchronize());   // the caller's producers of `ids` (any stream) are done
        tmp.resize((size_t)n);
        HIP_TRY(hipMemcpy(tmp.data(), ids, (size_t)n * 8, hipMemcpyDeviceToHost));
        host_ids = tmp.data();
    }
    RDX_TRY(check(host_ids));
    if (space == RDX_DEVICE) {
        *d_ids = ids;
        return RDX_OK;
    }
    RDX_TRY(h->ids.ensure((size_t)n * 8));
    HIP_TRY(hipMemcpyAsync(h->ids.p, ids, (size_t)n * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    *d_ids = h->ids.as<int64_t>();
    return RDX_OK;
}

static int update_impl(const char* fn, rdx_index* h, const int64_t* row_ids, const float* rows, int64_t n, int space, bool verbatim) {
    if (!h || n < 0 || (n > 0 && (!row_ids || !rows))) return fail(RDX_ERR_INVALID, std::string(fn) + ": bad argument");
    RDX_TRY(check_space(space));
    if (n == 0) return RDX_OK;
    std::lock_guard<std::mutex> lk(h->mu);
    RDX_TRY(finish_pending(h, nullptr));
    if (h->store.compact) return fail(RDX_ERR_STATE, std::string(fn) + " takes fp32 rows: not available on an index with a compact (bf16) master");
    RDX_TRY(set_device(h));
    const int64_t* d_ids = nullptr;
    const auto held_once = [&](const int64_t* v) {
        RDX_TRY(check_row_ids(h, v, n));
        return check_distinct_ids(v, n);
    };
    RDX_TRY(stage_ids(h, row_ids, n, space, held_once, &d_ids));
    return ingest(h, rows, false, n, space, 0, d_ids, verbatim);
}

extern "C" int rdx_index_update(rdx_index* h, const int64_t* row_ids, const float* rows, int64_t n, int space) {
    return update_impl("rdx_index_update", h, row_ids, rows, n, space, false);
}
extern "C" int rdx_index_update_stored(rdx_index* h, const int64_t* row_ids, const float* rows, int64_t n, int space) {
    return update_impl("rdx_index_update_stored", h, row_ids, rows, n, space, true);
}

int rdx::gather_rows(const rdx_index* h, const int64_t* d_ids, int64_t n, float* out, hipStream_t st) {
    hipLaunchKernelGGL(k_gather_rows, dim3((int)((n + 3) / 4)), dim3(256), 0, st, h->mv(), d_ids, n, h->dim, out);
    HIP_TRY(hipGetLastError());
    return RDX_OK;
}

extern "C" int rdx_index_get(rdx_index* h, const int64_t* row_ids, int64_t n, float* out, int space) {
    if (!h || n < 0 || (n > 0 && (!row_ids || !out))) return fail(RDX_ERR_INVALID, "rdx_index_get: bad argument");
    RDX_TRY(check_space(space));
    if (n == 0) return RDX_OK;
    std::lock_guard<std::mutex> lk(h->mu);
    RDX_TRY(finish_pending(h, nullptr));
    RDX_TRY(set_device(h));
    hipStream_t st = h->own_stream;
    const int64_t* d_ids = nullptr;
    RDX_TRY(stage_ids(h, row_ids, n, space, [&](const int64_t* v) { return check_row_ids(h, v, n); }, &d_ids));
    for (int64_t off = 0; off < n; off += STAGE_ROWS) {
        const int64_t m = std::min(STAGE_ROWS, n - off);
        float* dst = out + (size_t)off * h->dim;
        if (space == RDX_HOST) {
            RDX_TRY(h->staging.ensure((size_t)STAGE_ROWS * h->dim * 4));
            dst = h->staging.as<float>();
        }
        RDX_TRY(gather_rows(h, d_ids + off, m, dst, st));
        if (space == RDX_HOST) {
            HIP_TRY(hipMemcpyAsync(out + (size_t)off * h->dim, dst, (size_t)m * h->dim * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
    }
    HIP_TRY(hipStreamSynchronize(st));
    return RDX_OK;
}

extern "C" int rdx_index_compact(rdx_index* h, const int64_t* keep, int64_t n_keep) {
    if (!h || n_keep < 0 || (n_keep > 0 && !keep)) return fail(RDX_ERR_INVALID, "rdx_index_compact: bad argument");
    std::lock_guard<std::mutex> lk(h->mu);
    RDX_TRY(finish_pending(h, nullptr));
    RDX_TRY(set_device(h));
    int64_t at = 0;
    const IdFault bad = check_ids(keep, n_keep, IdRule{h->rows, true}, &at);
    if (bad == IdFault::range) return fail(RDX_ERR_INVALID, "compact: row id out of range");
    if (bad == IdFault::order) return fail(RDX_ERR_INVALID, "compact: keep list must be strictly ascending");
    hipStream_t st = h->own_stream;
    RowStore ns;   // (without an id map: the rows are renumbered, the caller sets a new map or none)
    ns.compact = h->store.compact;
    const hipError_t e = ns.alloc_rows(compact_cap(n_keep), h->dim, h->dim_pad);
    if (e != hipSuccess) return fail(RDX_ERR_NOMEM, std::string("compact: ") + hipGetErrorString(e));
    HIP_TRY(hipMemsetAsync(ns.shadow.p, 0, ns.shadow.bytes, st));
    if (n_keep > 0) {
        RDX_TRY(h->ids.ensure((size_t)n_keep * 8));
        HIP_TRY(hipMemcpyAsync(h->ids.p, keep, (size_t)n_keep * 8, hipMemcpyHostToDevice, st));
        const MasterView nv = ns.mv();
        if (ns.compact)
            hipLaunchKernelGGL(k_gather_raw, dim3((int)((n_keep + 3) / 4)), dim3(256), 0, st, h->mv(), h->ids.as<int64_t>(), n_keep, h->dim, nv);
        else
            hipLaunchKernelGGL(k_gather_rows, dim3((int)((n_keep + 3) / 4)), dim3(256), 0, st, h->mv(), h->ids.as<int64_t>(), n_keep, h->dim, nv.f32);
        hipLaunchKernelGGL(k_reshadow, dim3((int)((n_keep + 3) / 4)), dim3(256), 0, st, nv, (int64_t)0, n_keep, h->dim, ns.shadow.as<_Float16>(),
                           h->ksteps, h->scale());
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(st));
    h->store = std::move(ns);   // (ns leaves with the old arrays and the old id map)
    h->rows = n_keep;
    h->i8.mark.renumbered();
    return RDX_OK;
}

extern "C" int rdx_index_set_row_ids(rdx_index* h, int64_t first_row, const int64_t* ids, int64_t n, int space) {
    if (!h || first_row < 0 || n < 0 || (n > 0 && !ids)) return fail(RDX_ERR_INVALID, "rdx_index_set_row_ids: bad argument");
    RDX_TRY(check_space(space));
    std::lock_guard<std::mutex> lk(h->mu);
    if (first_row + n > h->rows) return fail(RDX_ERR_INVALID, "rdx_index_set_row_ids: rows [first_row, first_row + n) must exist");
    if (n == 0) return RDX_OK;
    RDX_TRY(finish_pending(h, nullptr));   // k_refine / k_select_dense of an asynchronous search may still be reading the map
    RDX_TRY(set_device(h));
    hipStream_t st = h->own_stream;
    // the merge's tie order rests on the map being increasing: checked for device ids too
    const auto increasing = [&](const int64_t* v) {
        int64_t at = 0;
        if (check_ids(v, n, IdRule{INT64_MAX, true}, &at) != IdFault::none)
            return fail(RDX_ERR_INVALID, "rdx_index_set_row_ids: ids must be non-negative and strictly increasing");
        return (int)RDX_OK;
    };
    const int64_t* d_ids = nullptr;
    RDX_TRY(stage_ids(h, ids, n, space, increasing, &d_ids));
    RowStore& rs = h->store;
    if (!rs.row_map.p) {
        HIP_TRY(rs.alloc_ids());
        hipLaunchKernelGGL(k_iota64, dim3((unsigned)((rs.cap + 255) / 256)), dim3(256), 0, st, rs.row_map.as<int64_t>(), (int64_t)0, rs.cap, h->row_base);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(rs.row_map.as<int64_t>() + first_row, d_ids, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    return RDX_OK;
}

// scratch of rdx_l2_normalize, kept per device (the call sits on the embed() path of every query: no hipMalloc/hipFree per call)
struct NormScratch {
    std::mutex mu;
    DevBuf in, out, bad;
};
// (never destroyed: a static destructor would call hipFree at process exit, possibly after the HIP runtime is gone)
static NormScratch* const g_norm = new NormScratch[MAX_DEVICES];

extern "C" int rdx_l2_normalize(int device, const float* in, int64_t n, int dim, float* out, int space, void* stream) {
    if (n < 0 || (n > 0 && (!in || !out))) return fail(RDX_ERR_INVALID, "rdx_l2_normalize: bad argument");
    RDX_TRY(check_dim(dim));
    RDX_TRY(check_space(space));
    RDX_TRY(check_device_index("rdx_l2_normalize", device));
    if (n == 0) return RDX_OK;
    HIP_TRY(hipSetDevice(device));
    NormScratch& sc = g_norm[device];
    std::lock_guard<std::mutex> lk(sc.mu);
    hipStream_t st = (hipStream_t)stream;
    const float* d_in = in;
    float* d_out = out;
    RDX_TRY(sc.bad.ensure(sizeof(int)));
    if (space == RDX_HOST) {
        RDX_TRY(sc.in.ensure((size_t)n * dim * 4));
        RDX_TRY(sc.out.ensure((size_t)n * dim * 4));
        HIP_TRY(hipMemcpyAsync(sc.in.p, in, (size_t)n * dim * 4, hipMemcpyHostToDevice, st));
        d_in = sc.in.as<float>();
        d_out = sc.out.as<float>();
    }
    HIP_TRY(hipMemsetAsync(sc.bad.p, 0, sizeof(int), st));
    hipLaunchKernelGGL(k_normalize<false>, dim3((int)((n + 3) / 4)), dim3(256), 0, st, d_in, (const uint16_t*)nullptr, n, dim,
                       (const int64_t*)nullptr, (int64_t)0, MasterView{d_out, nullptr, nullptr}, (_Float16*)nullptr, 0, 1.0f, sc.bad.as<int>());
    HIP_TRY(hipGetLastError());
    int b = 0;
    if (space == RDX_HOST) HIP_TRY(hipMemcpyAsync(out, d_out, (size_t)n * dim * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&b, sc.bad.p, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));   // the NaN/Inf verdict is part of the return value
    if (b) return fail(RDX_ERR_INVALID, "embeddings contain NaN or Inf");
    return RDX_OK;
}

// ------------------------------------------------------------------------------------------------
// search: the entry points and masks
// ------------------------------------------------------------------------------------------------
// what rdx_search and rdx_search_async do first (h->mu held): the pending search completes (scratch buffers are shared), the
// device is selected, the profiling events exist, and the statistics start from the call's shape
static int begin_search(rdx_index* h, int64_t nq, int k, rdx_search_stats* s) {
    RDX_TRY(finish_pending(h, nullptr));
    RDX_TRY(set_device(h));
    if (h->opt.profile && !h->ev_ok) {
        for (auto& e : h->ev) HIP_TRY(hipEventCreate(&e));
        h->ev_ok = true;
    }
    *s = {};
    s->nq = nq;
    s->k = k;
    s->rows = h->rows;
    return RDX_OK;
}

// a resident mask is the index's, as it stands; code: RDX_ERR_STATE, or RDX_ERR_INVALID from the threshold search and the clustering (include/rdx.h)
int rdx::check_mask(const rdx_index* h, const rdx_mask* mask, const char* who, int code) {
    if (mask && (mask->device != h->device || mask->rows != h->rows))
        return fail(code, std::string(who) + ": the mask was made for " + std::to_string(mask->rows) + " rows on device " +
                              std::to_string(mask->device) + ", the index now holds " + std::to_string(h->rows) +
                              " (a mask does not outlive a write to the index)");
    return RDX_OK;
}

// calls that take or return the index's own rows are not a shard's; tail: what the caller is told instead
int rdx::check_own_rows(const rdx_index* h, const char* who, const char* tail) {
    if (h->store.row_map.p || h->row_base != 0)
        return fail(RDX_ERR_STATE, std::string(who) + ": the index returns mapped row ids (a shard): " + tail);
    return RDX_OK;
}

// a checked rdx_search_filtered call that names more than one filter (host arrays)
struct FilterCall {
    const rdx_mask* const* filters;
    int32_t n_filters;
    const int32_t* query_filter;
};

// The call's filter table and indices into the index's scratch, on the search's stream: n_filters device pointers, then the nq indices
// padded with -1 to whole 256-query tiles (every chunk of a search reads its slice up to its own nq_pad).
static int upload_filters(rdx_index* h, const FilterCall& fc, int64_t nq, hipStream_t st, RowFilter* out) {
    const size_t b_tab = ((size_t)fc.n_filters * sizeof(const uint32_t*) + 15) & ~(size_t)15;
    const size_t n_qf = (size_t)((nq + 255) / 256 * 256);
    h->fq_host.assign(b_tab + n_qf * 4, (char)0xff);   // (every index -1)
    const uint32_t** tab = reinterpret_cast<const uint32_t**>(h->fq_host.data());
    for (int32_t f = 0; f < fc.n_filters; ++f) tab[f] = fc.filters[f]->words.as<uint32_t>();
    std::memcpy(h->fq_host.data() + b_tab, fc.query_filter, (size_t)nq * 4);
    RDX_TRY(h->fq.ensure(h->fq_host.size()));
    HIP_TRY(hipMemcpyAsync(h->fq.p, h->fq_host.data(), h->fq_host.size(), hipMemcpyHostToDevice, st));
    *out = RowFilter(reinterpret_cast<const uint32_t* const*>(h->fq.p), reinterpret_cast<const int32_t*>(h->fq.as<char>() + b_tab));
    return RDX_OK;
}

// allow_resident: allow_bits is already device memory whatever `space` says (a resident rdx_mask). fc: a filter per query instead
// (allow_bits NULL).
static int search_impl(rdx_index* h, const float* queries, int64_t nq, int k, const uint32_t* allow_bits, bool allow_resident,
                       float* out_score, int64_t* out_row, int32_t* out_count, int space, void* stream, const FilterCall* fc = nullptr) {
    if (nq < 0 || k < 0) return fail(RDX_ERR_INVALID, "rdx_search: nq and k must be >= 0");
    if (k > SELECT_MAX_K) return fail(RDX_ERR_INVALID, "rdx_search: k larger than " + std::to_string(SELECT_MAX_K) + " is not supported");
    RDX_TRY(check_space(space));
    if (nq == 0) return RDX_OK;
    if (!queries || !out_count || (k > 0 && (!out_score || !out_row))) return fail(RDX_ERR_INVALID, "rdx_search: null pointer");
    rdx_search_stats s;
    RDX_TRY(begin_search(h, nq, k, &s));
    // device pointers: the caller's stream as given (NULL = the default stream the caller produced its inputs on)
    hipStream_t st = (space == RDX_DEVICE || stream) ? (hipStream_t)stream : h->own_stream;

    const uint32_t* d_allow = allow_bits;
    const size_t mask_words = (size_t)((h->rows + 31) / 32);
    if (allow_bits && space == RDX_HOST && !allow_resident && mask_words > 0) {
        // pad to whole 256-row tiles so the scan may read the word of any block it touches
        const size_t pad_words = (size_t)((h->rows + 255) / 256 * 8);
        RDX_TRY(h->mask.ensure(pad_words * 4));
        HIP_TRY(hipMemsetAsync(h->mask.p, 0, pad_words * 4, st));
        HIP_TRY(hipMemcpyAsync(h->mask.p, allow_bits, mask_words * 4, hipMemcpyHostToDevice, st));
        d_allow = h->mask.as<uint32_t>();
    }
    RowFilter per_query;
    if (fc) RDX_TRY(upload_filters(h, *fc, nq, st, &per_query));
    const int64_t CHUNK = 4096;   // queries per pipeline pass (<= 256 * WGs per XCD)
    const int kk = std::max(k, 1);
    for (int64_t q0 = 0; q0 < nq; q0 += CHUNK) {
        const int64_t m = std::min(CHUNK, nq - q0);
        SearchIO io = {queries + (size_t)q0 * h->dim, fc ? RowFilter(per_query.ftab, per_query.qf + q0) : RowFilter(d_allow), out_score ? out_score + (size_t)q0 * k : nullptr,
                       out_row ? out_row + (size_t)q0 * k : nullptr, out_count + q0, nullptr};
        HostOut ho = {io.score, io.row, io.count, false};
        if (space == RDX_HOST) {
            RDX_TRY(h->qraw.ensure((size_t)m * h->dim * 4));
            RDX_TRY(h->o_score.ensure((size_t)m * kk * 4));
            RDX_TRY(h->o_row.ensure((size_t)m * kk * 8));
            RDX_TRY(h->o_count.ensure((size_t)m * 4));
            HIP_TRY(hipMemcpyAsync(h->qraw.p, io.queries, (size_t)m * h->dim * 4, hipMemcpyHostToDevice, st));
            io.queries = h->qraw.as<float>();
            io.score = h->o_score.as<float>();
            io.row = h->o_row.as<int64_t>();
            io.count = h->o_count.as<int32_t>();
        }
        RDX_TRY(search_chunk(h, io, m, k, st, &s, 0, space == RDX_HOST ? &ho : nullptr, false));
        if (space == RDX_HOST && ho.stale) {
            RDX_TRY(copy_results_to_host(ho, io.score, io.row, io.count, m, k, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
    }
    h->stats = s;
    return RDX_OK;
}

extern "C" int rdx_search(rdx_index* h, const float* queries, int64_t nq, int k, const uint32_t* allow_bits, float* out_score,
                          int64_t* out_row, int32_t* out_count, int space, void* stream) {
    if (!h) return fail(RDX_ERR_INVALID, "rdx_search: null index");
    std::lock_guard<std::mutex> lk(h->mu);
    return search_impl(h, queries, nq, k, allow_bits, false, out_score, out_row, out_count, space, stream);
}

extern "C" int rdx_search_async(rdx_index* h, const float* queries, int64_t nq, int k, const rdx_mask* mask, float* out_score,
                                int64_t* out_row, int32_t* out_count, int32_t* out_flags, void* stream) {
    if (!h) return fail(RDX_ERR_INVALID, "rdx_search_async: null index");
    if (nq < 1 || nq > 4096 || k < 0 || k > SELECT_MAX_K) return fail(RDX_ERR_INVALID, "rdx_search_async: 1 <= nq <= 4096, 0 <= k <= " + std::to_string(SELECT_MAX_K));
    if (!queries || !out_count || (k > 0 && (!out_score || !out_row))) return fail(RDX_ERR_INVALID, "rdx_search_async: null pointer");
    std::lock_guard<std::mutex> lk(h->mu);
    RDX_TRY(check_mask(h, mask, "rdx_search_async", RDX_ERR_STATE));
    rdx_search_stats s;
    RDX_TRY(begin_search(h, nq, k, &s));
    const SearchIO io = {queries, mask ? mask->words.as<uint32_t>() : nullptr, out_score, out_row, out_count, out_flags};
    return search_chunk(h, io, nq, k, (hipStream_t)stream, &s, 0, nullptr, true);
}

extern "C" int rdx_search_wait(rdx_index* h, int* redone) {
    if (!h) return fail(RDX_ERR_INVALID, "rdx_search_wait: null index");
    std::lock_guard<std::mutex> lk(h->mu);
    bool r = false;
    const int rc = finish_pending(h, &r);
    if (redone) *redone = r ? 1 : 0;
    return rc;
}

extern "C" int rdx_mask_create(rdx_index* h, const uint32_t* allow_bits, int space, rdx_mask** out) {
    if (!h || !allow_bits || !out) return fail(RDX_ERR_INVALID, "rdx_mask_create: null pointer");
    RDX_TRY(check_space(space));
    std::lock_guard<std::mutex> lk(h->mu);
    RDX_TRY(finish_pending(h, nullptr));
    RDX_TRY(set_device(h));
    auto m = std::make_unique<rdx_mask>();
    m->device = h->device;
    m->rows = h->rows;
    const size_t words = (size_t)((h->rows + 31) / 32), pad_words = (size_t)((h->rows + 255) / 256 * 8);
    RDX_TRY(m->words.ensure(std::max<size_t>(pad_words, 8) * 4));
    hipStream_t st = h->own_stream;
    hipError_t e = hipMemsetAsync(m->words.p, 0, std::max<size_t>(pad_words, 8) * 4, st);
    if (e == hipSuccess && words > 0) {
        if (space == RDX_DEVICE) e = hipDeviceSynchronize();   // the caller's producer of the bits (any stream) is done
        if (e == hipSuccess)
            e = hipMemcpyAsync(m->words.p, allow_bits, words * 4, space == RDX_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(RDX_ERR_HIP, std::string("rdx_mask_create: ") + hipGetErrorString(e));
    *out = m.release();
    return RDX_OK;
}

extern "C" int rdx_mask_destroy(rdx_mask* m) {
    if (!m) return RDX_OK;
    (void)hipSetDevice(m->device);
    const std::unique_ptr<rdx_mask> owner(m);
    return RDX_OK;
}

extern "C" int rdx_search_masked(rdx_index* h, const float* queries, int64_t nq, int k, const rdx_mask* mask, float* out_score,
                                 int64_t* out_row, int32_t* out_count, int space, void* stream) {
    if (!h) return fail(RDX_ERR_INVALID, "rdx_search_masked: null index");
    std::lock_guard<std::mutex> lk(h->mu);
    RDX_TRY(check_mask(h, mask, "rdx_search_masked", RDX_ERR_STATE));
    return search_impl(h, queries, nq, k, mask ? mask->words.as<uint32_t>() : nullptr, true, out_score, out_row, out_count, space, stream);
}

// A filter per query. Everything the header refuses is refused here, before anything is enqueued; a call whose queries
// all name one filter (or none) is the existing search.
extern "C" int rdx_search_filtered(rdx_index* h, const float* queries, int64_t nq, int k, const rdx_mask* const* filters, int32_t n_filters,
                                   const int32_t* query_filter, float* out_score, int64_t* out_row, int32_t* out_count, int space, void* stream) {
    if (!h) return fail(RDX_ERR_INVALID, "rdx_search_filtered: null index");
    if (n_filters < 0 || n_filters > 65535)
        return fail(RDX_ERR_INVALID, "rdx_search_filtered: n_filters must be in [0, 65535] (got " + std::to_string(n_filters) + ")");
    if (n_filters > 0 && !filters) return fail(RDX_ERR_INVALID, "rdx_search_filtered: filters is NULL with n_filters = " + std::to_string(n_filters));
    for (int32_t f = 0; f < n_filters; ++f)
        if (!filters[f]) return fail(RDX_ERR_INVALID, "rdx_search_filtered: filters[" + std::to_string(f) + "] is a NULL handle");
    if (nq > 0 && !query_filter) return fail(RDX_ERR_INVALID, "rdx_search_filtered: query_filter is NULL with nq = " + std::to_string(nq));
    bool one = true;   // every query names query_filter[0]
    for (int64_t q = 0; q < nq; ++q) {
        if (query_filter[q] < -1 || query_filter[q] >= n_filters)
            return fail(RDX_ERR_INVALID, "rdx_search_filtered: query " + std::to_string(q) + " names filter " + std::to_string(query_filter[q]) +
                                             ", outside [-1, " + std::to_string(n_filters) + ")");
        one = one && query_filter[q] == query_filter[0];
    }
    std::lock_guard<std::mutex> lk(h->mu);
    for (int32_t f = 0; f < n_filters; ++f) RDX_TRY(check_mask(h, filters[f], "rdx_search_filtered", RDX_ERR_STATE));
    if (nq <= 0 || one) {
        const rdx_mask* mask = (nq > 0 && query_filter[0] >= 0) ? filters[query_filter[0]] : nullptr;
        return search_impl(h, queries, nq, k, mask ? mask->words.as<uint32_t>() : nullptr, true, out_score, out_row, out_count, space, stream);
    }
    const FilterCall fc = {filters, n_filters, query_filter};
    return search_impl(h, queries, nq, k, nullptr, true, out_score, out_row, out_count, space, stream, &fc);
}

// ---- grouped search: the fill ---------------------------------------------------------------------------------
static_assert(GROUP_FILL_SPAN == RDX_GROUP_FILL_SPAN && GROUP_FILL_MAX_M == RDX_GROUP_MAX_SIZE, "group_fill_kernel.hpp and include/rdx.h disagree");

extern "C" int rdx_index_group_fill(rdx_index* h, const float* queries, int64_t nq, const rdx_mask* mask, const int32_t* job_query,
                                    const int64_t* job_begin, const int64_t* job_end, int64_t n_jobs, const int64_t* group_rows,
                                    int64_t n_group_rows, int m, float* out_score, int64_t* out_row, int32_t* out_count, void* stream) {
    if (!h) return fail(RDX_ERR_INVALID, "rdx_index_group_fill: null index");
    if (nq < 1 || nq > 65535) return fail(RDX_ERR_INVALID, "rdx_index_group_fill: nq must be in [1, 65535]");
    if (n_jobs < 0 || n_jobs > (int64_t)1 << 22) return fail(RDX_ERR_INVALID, "rdx_index_group_fill: n_jobs must be in [0, 2^22]");
    if (m < 1 || m > GROUP_FILL_MAX_M) return fail(RDX_ERR_INVALID, "rdx_index_group_fill: m must be in [1, 16]");
    if (n_group_rows < 0) return fail(RDX_ERR_INVALID, "rdx_index_group_fill: n_group_rows must be >= 0");
    if (n_jobs == 0) return RDX_OK;
    if (!queries || !job_query || !job_begin || !job_end || !out_score || !out_row || !out_count || (n_group_rows > 0 && !group_rows))
        return fail(RDX_ERR_INVALID, "rdx_index_group_fill: null pointer");
    if (((uintptr_t)queries & 15) || (((uintptr_t)group_rows | (uintptr_t)out_row) & 7) || (((uintptr_t)out_score | (uintptr_t)out_count) & 3))
        return fail(RDX_ERR_INVALID, "rdx_index_group_fill: misaligned pointer");
    for (int64_t j = 0; j < n_jobs; ++j) {   // the jobs are host memory: held to the header's words before anything is enqueued
        if (job_query[j] < 0 || job_query[j] >= nq)
            return fail(RDX_ERR_INVALID, "rdx_index_group_fill: job " + std::to_string(j) + " names query " + std::to_string(job_query[j]) +
                                             " of " + std::to_string(nq));
        if (job_begin[j] < 0 || job_end[j] < job_begin[j] || job_end[j] > n_group_rows || job_end[j] - job_begin[j] > GROUP_FILL_SPAN)
            return fail(RDX_ERR_INVALID, "rdx_index_group_fill: job " + std::to_string(j) + " must span 0 <= begin <= end <= n_group_rows, at most " +
                                             std::to_string(GROUP_FILL_SPAN) + " rows");
    }
    std::lock_guard<std::mutex> lk(h->mu);
    RDX_TRY(check_mask(h, mask, "rdx_index_group_fill", RDX_ERR_STATE));
    RDX_TRY(check_own_rows(h, "rdx_index_group_fill", "group_rows must be the index's own rows"));
    RDX_TRY(finish_pending(h, nullptr));
    RDX_TRY(set_device(h));
    hipStream_t st = (hipStream_t)stream;
    RDX_TRY(h->qhat.ensure((size_t)nq * h->dim * 4));
    RDX_TRY(h->bad.ensure(sizeof(int)));
    const size_t jq = ((size_t)n_jobs * 4 + 7) & ~(size_t)7, jb = (size_t)n_jobs * 8;
    RDX_TRY(h->gjobs.ensure(jq + 2 * jb));
    char* const dj = h->gjobs.as<char>();
    HIP_TRY(hipMemcpyAsync(dj, job_query, (size_t)n_jobs * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dj + jq, job_begin, jb, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dj + jq + jb, job_end, jb, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(h->bad.p, 0, sizeof(int), st));
    // K1 on the queries, the call rdx_search makes: the same qhat bits
    RDX_TRY(normalize_queries<false>(h, queries, nq, 0, nullptr, h->bad.as<int>(), 0, st));
    GroupFillParams gp = {};
    gp.master = h->mv();
    gp.rows = h->rows;
    gp.dim = h->dim;
    gp.qhat = h->qhat.as<float>();
    gp.allow = mask ? mask->words.as<uint32_t>() : nullptr;
    gp.job_query = reinterpret_cast<const int32_t*>(dj);
    gp.job_begin = reinterpret_cast<const int64_t*>(dj + jq);
    gp.job_end = reinterpret_cast<const int64_t*>(dj + jq + jb);
    gp.n_jobs = n_jobs;
    gp.group_rows = group_rows;
    gp.m = m;
    gp.out_score = out_score;
    gp.out_row = out_row;
    gp.out_count = out_count;
    dispatch_u(h->dim, [&](auto u) {   // one workgroup per job
        hipLaunchKernelGGL(k_group_fill<decltype(u)::value>, dim3((unsigned)gp.n_jobs), dim3(64 * GROUP_FILL_WAVES), 0, st, gp);
    });
    HIP_TRY(hipGetLastError());
    int b = 0;
    HIP_TRY(hipMemcpyAsync(&b, h->bad.p, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));   // the jobs' host arrays are the caller's again, and the NaN/Inf verdict is part of the return value
    if (b) return fail(RDX_ERR_INVALID, "embeddings contain NaN or Inf");
    return RDX_OK;
}

// ---- threshold search ------------------------------------------------------------------------------------------
static_assert(RDX_RANGE_MAX_RESULTS <= REFINE_PMAX && RDX_RANGE_MAX_RESULTS <= SELECT_MAX_K, "range_kernel.hpp ranks max_results entries in k_refine's arrays");

// the exact path of a range search for the queries listed in d_list[0..n_list): K5a per group of QX queries, then k_range_select_dense
// (fc: the counting variant, for rdx_index_range_facets)
static int run_range_exact(rdx_index* h, const int32_t* d_list, int n_list, int k, const RangeIO& io, hipStream_t st, const FacetIO* fc) {
    return for_exact_groups(h, d_list, n_list, io.allow, nullptr, st, [&](const int32_t* q_list, int nq, bool) {
        SelectParams sel = select_params(h, k, TopkOut{io.score, io.row, io.count});
        sel.q_list = q_list;
        if (fc) hipLaunchKernelGGL(k_range_select_dense<true>, dim3(nq), dim3(1024), 0, st, sel, io.thr, io.total, *fc);
        else hipLaunchKernelGGL(k_range_select_dense<false>, dim3(nq), dim3(1024), 0, st, sel, io.thr, io.total, FacetIO{});
    });
}

// One chunk (nq <= 4096) of a range search: plan_range, K1, k_range_tau, then the exact path for everybody, or the main scan,
// k_range_refine and the exact path for the queries it listed. Returns with the stream drained; paths[0] / [1] take the chunk's queries
// by path. fc: the counting variants of the two last stages instead (rdx_index_range_facets): io's lists are not written, k is 1.
int rdx::range_chunk(rdx_index* h, const RangeIO& io, int64_t nq, int k, hipStream_t st, int32_t* paths, const FacetIO* fc) {
    SearchPlan p;
    std::string err;
    const int prc = plan_range(h->shape(), h->opt, nq, k, &p, &err);
    if (prc != RDX_OK) return fail(prc, err);
    RDX_TRY(h->qhat.ensure((size_t)p.nq_pad * h->dim * 4));
    RDX_TRY(h->tau.ensure((size_t)p.nq_pad * 4));
    RDX_TRY(h->exact_list.ensure((size_t)p.nq_pad * 4));
    RDX_TRY(h->rng_ctr.ensure(sizeof(RangeCounters)));
    if (!p.exact_only) {
        RDX_TRY(h->qshadow.ensure((size_t)p.nq_pad * h->dim_pad * 2));
        RDX_TRY(h->cntw.ensure((size_t)p.nq_pad * p.n_streams * 4));
        RDX_TRY(h->cand.ensure((size_t)p.nq_pad * p.n_streams * p.capw * 8));
    }
    RangeCounters* const ctr = h->rng_ctr.as<RangeCounters>();
    int* const d_bad = reinterpret_cast<int*>(h->rng_ctr.as<char>() + offsetof(RangeCounters, bad));
    HIP_TRY(hipMemsetAsync(h->rng_ctr.p, 0, sizeof(RangeCounters), st));
    // K1 on the queries, the call a search makes: the same qhat bits (and, for the scan, the same tiled fp16 copy)
    RDX_TRY(normalize_queries<true>(h, io.queries, nq, p.nq_pad, p.exact_only ? nullptr : h->qshadow.as<_Float16>(), d_bad, 0, st));
    // (on the exact path too: it is also what refuses a NaN threshold)
    hipLaunchKernelGGL(k_range_tau, dim3((p.nq_pad + 255) / 256), dim3(256), 0, st, io.thr, (int)nq, p.nq_pad, 0.5f * h->two_e(),
                       std::ldexp(1.0f, 2 * h->scale_log2), h->tau.as<float>(), d_bad);
    HIP_TRY(hipGetLastError());
    if (p.exact_only) {
        RDX_TRY(ensure_iota(h, p.nq_pad, st));
        RDX_TRY(run_range_exact(h, h->iota.as<int32_t>(), (int)nq, k, io, st, fc));
    } else {
        // the fp16 scan always, with neither bootstrap sets, XCD ranges nor stamps, and its bounds flag in this call's own counter block
        int* const oob = reinterpret_cast<int*>(h->rng_ctr.as<char>() + offsetof(RangeCounters, oob));
        RDX_TRY(launch_main_scan(h, p, main_scan_params(h, p, io.allow, oob, nullptr, 0, false, nullptr), false, st));
        RangeParams rp = {};
        rp.r = refine_lists(h, p, k, TopkOut{io.score, io.row, io.count});
        rp.thr = io.thr;
        rp.total = io.total;
        rp.fallback_list = h->exact_list.as<int32_t>();
        rp.ctr = ctr;
        const size_t lds = (size_t)p.list_cap * 8;
        if (fc) {
            RDX_TRY(dynamic_lds(h->device, (const void*)k_range_refine<true>, lds));
            hipLaunchKernelGGL(k_range_refine<true>, dim3((unsigned)nq), dim3(1024), lds, st, rp, *fc);
        } else {
            RDX_TRY(dynamic_lds(h->device, (const void*)k_range_refine<false>, lds));
            hipLaunchKernelGGL(k_range_refine<false>, dim3((unsigned)nq), dim3(1024), lds, st, rp, FacetIO{});
        }
        HIP_TRY(hipGetLastError());
    }
    RangeCounters c = {};
    HIP_TRY(hipMemcpyAsync(&c, h->rng_ctr.p, sizeof(c), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (c.oob) return fail(RDX_ERR_STATE, "internal: the scan computed a corpus address outside the scan copy (RDX_CHECK_BOUNDS build)");
    if (c.bad) return fail(RDX_ERR_INVALID, "query embeddings contain NaN or Inf, or a threshold is NaN");
    int n_fb = p.exact_only ? (int)nq : c.n_fallback;
    if (!p.exact_only && n_fb > 0) {
        if (n_fb > nq) return fail(RDX_ERR_STATE, "internal: more fallback queries than queries");
        RDX_TRY(run_range_exact(h, h->exact_list.as<int32_t>(), n_fb, k, io, st, fc));
        HIP_TRY(hipStreamSynchronize(st));
    }
    paths[0] += (int32_t)(nq - n_fb);
    paths[1] += n_fb;
    return RDX_OK;
}

extern "C" int rdx_index_range(rdx_index* h, const float* queries, int64_t nq, const float* thresholds, int max_results, const rdx_mask* mask,
                               float* out_score, int64_t* out_row, int32_t* out_count, int64_t* out_total, int32_t* out_paths, void* stream) {
    if (!h) return fail(RDX_ERR_INVALID, "rdx_index_range: null index");
    if (max_results < 1 || max_results > RDX_RANGE_MAX_RESULTS)
        return fail(RDX_ERR_INVALID, "rdx_index_range: max_results must be in [1, " + std::to_string(RDX_RANGE_MAX_RESULTS) + "]");
    if (nq < 0 || nq > 65535) return fail(RDX_ERR_INVALID, "rdx_index_range: nq must be in [0, 65535]");
    int32_t paths[2] = {0, 0};
    if (out_paths) out_paths[0] = out_paths[1] = 0;
    if (nq == 0) return RDX_OK;
    if (!queries || !thresholds || !out_score || !out_row || !out_count || !out_total) return fail(RDX_ERR_INVALID, "rdx_index_range: null pointer");
    if (((uintptr_t)queries & 15) || (((uintptr_t)out_row | (uintptr_t)out_total) & 7) ||
        (((uintptr_t)thresholds | (uintptr_t)out_score | (uintptr_t)out_count) & 3))
        return fail(RDX_ERR_INVALID, "rdx_index_range: misaligned pointer");
    std::lock_guard<std::mutex> lk(h->mu);
    RDX_TRY(check_mask(h, mask, "rdx_index_range", RDX_ERR_INVALID));
    RDX_TRY(check_own_rows(h, "rdx_index_range", "not available"));
    RDX_TRY(finish_pending(h, nullptr));
    RDX_TRY(set_device(h));
    hipStream_t st = (hipStream_t)stream;
    for (int64_t q0 = 0; q0 < nq; q0 += RANGE_CHUNK) {
        const int64_t m = std::min(RANGE_CHUNK, nq - q0);
        const RangeIO io = {queries + (size_t)q0 * h->dim, thresholds + q0, mask ? mask->words.as<uint32_t>() : nullptr,
                            out_score + (size_t)q0 * max_results, out_row + (size_t)q0 * max_results, out_count + q0, out_total + q0};
        RDX_TRY(range_chunk(h, io, m, max_results, st, paths));
    }
    if (out_paths) {
        out_paths[0] = paths[0];
        out_paths[1] = paths[1];
    }
    return RDX_OK;
}

#ifdef RDX_REFINE_STAMPS
extern "C" int rdx_debug_refine_stamps(unsigned long long* out16) {
    return hipMemcpyFromSymbol(out16, HIP_SYMBOL(rdx::g_refine_stamps), 16 * sizeof(unsigned long long)) == hipSuccess ? 0 : 2;
}
#endif
#ifdef RDX_SELECT_STAMPS
extern "C" int rdx_debug_select_stamps(unsigned long long* out16) {
    return hipMemcpyFromSymbol(out16, HIP_SYMBOL(rdx::g_select_stamps), 16 * sizeof(unsigned long long)) == hipSuccess ? 0 : 2;
}
#endif

extern "C" int rdx_search_last_coarse_bits(rdx_index* h, int32_t* bits) {
    if (!h || !bits) return fail(RDX_ERR_INVALID, "rdx_search_last_coarse_bits: null pointer");
    std::lock_guard<std::mutex> lk(h->mu);
    *bits = h->coarse_bits;
    return RDX_OK;
}

extern "C" int rdx_search_last_stats(rdx_index* h, rdx_search_stats* out) {
    if (!h || !out) return fail(RDX_ERR_INVALID, "rdx_search_last_stats: null pointer");
    std::lock_guard<std::mutex> lk(h->mu);
    *out = h->stats;
    return RDX_OK;
}
