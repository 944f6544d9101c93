// rdx_limits.hpp — the compile-time limits that both the kernels (rdx_common.hpp, scan_kernel.hpp, refine_kernel.hpp) and the search
// plan (search_plan.hpp) use, and the one limit every host unit shares. No HIP include: a plain C++ compiler builds it.
#pragma once

namespace rdx {

constexpr int TILE_ROWS = 256;                    // corpus rows per scan tile / shadow block
constexpr int BK = 64;                            // k elements per k-step image

constexpr int SETS_PER_STREAM = 32;   // bootstrap sets per (stream, query): 8 waves x 2 lane halves x 2 register classes
constexpr int BOOT_BN = 64;           // queries of a k_boot / k_scan_small launch (scan_kernel.hpp K2b, K2c)

constexpr int REFINE_PMAX = 1024;    // most candidates re-scored exactly per query; more -> exact full scan
constexpr int REFINE_LIST = 7168;    // most scan hits gathered per query (56 KiB of LDS: with the 22 KiB of static LDS TWO blocks fit a CU's 160 KiB —
                                     // at B = 1024 the kernel runs in two rounds instead of four); more -> second pass / exact full scan
constexpr int REFINE_STREAMS = 512;  // most (query, stream) segments
constexpr int SPILL_CAP = 40960;     // most hits of a query whose list lives in HBM instead (k_refine<true>; plan_search SearchPlan::spill): 2.4x the
                                     // longest list seen at c4 with the thinnest sample (17 264 hits, every 64th block; 13 358 at the default's
                                     // every 32nd; DESIGN.md §5 "Spill list"), 320 MB for 1 024 queries; more -> second pass
constexpr int EPS_CLASSES = 8;       // most classes of block error the int8 scan tells apart (k_eps_edges, SearchPlan::eps_classes): edges at the
                                     // 50 / 75 / 87.5 ... % quantiles of eps_b, the top class's edge eps_max

constexpr int MAX_DEVICES = 64;      // device indices the per-device host state is sized for (rdx_host.hpp check_device_index)

}   // namespace rdx
