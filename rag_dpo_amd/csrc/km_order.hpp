// km_order.hpp — the ordering core of rdx_index_kmeans, HIP-free: the stable order of rows by label and the segment
// table of the ordered per-cluster sum, as plain functions over arrays. kmeans_kernel.hpp calls them from its kernels;
// tests/c_abi/km_order_host.cpp rehearses them on the CPU, block by block and tile by tile, against a stable sort.
//
// Rows are cut into blocks of `span` consecutive rows (a multiple of KM_TILE), a block into tiles of KM_TILE rows. The position of
// an allowed row r with label c in the order is
//     offset[c][b]  +  members of c in the earlier tiles of block b  +  km_tile_rank(r's tile, r)
// where offset is the exclusive prefix sum of the per-block histograms in (cluster, block) order: index km_hist_index(c, b, nb).
// Every term is a count; no atomic decides a position. offset[c][0] = where cluster c begins: the cluster offsets.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define KM_HD __host__ __device__ inline
#else
#define KM_HD inline
#endif

namespace rdx {

constexpr int KM_TILE = 256;                          // rows per tile: one thread per row
constexpr int KM_SEGMENT = 256;                       // members per segment of the per-cluster sum: part of the definition
constexpr int64_t KM_MAX_HIST = (int64_t)1 << 22;     // upper bound on the histogram's entries, clusters x blocks

// rows per block: the smallest multiple of KM_TILE that keeps clusters x blocks within KM_MAX_HIST (n_clusters <= 4096 <= KM_MAX_HIST)
KM_HD int64_t km_block_span(int64_t rows, int n_clusters) {
    const int64_t max_blocks = KM_MAX_HIST / n_clusters;
    const int64_t tiles = (rows + KM_TILE - 1) / KM_TILE;
    const int64_t tiles_per_block = (tiles + max_blocks - 1) / max_blocks;
    return (tiles_per_block > 0 ? tiles_per_block : 1) * KM_TILE;
}

KM_HD int64_t km_hist_index(int cluster, int64_t block, int64_t n_blocks) { return (int64_t)cluster * n_blocks + block; }

// Entry t of a tile of n <= KM_TILE labels (-1: not a member of anything): how many earlier entries of the tile carry its label;
// *last = no later entry does (that entry alone moves the cluster's running count on, by rank + 1).
KM_HD int km_tile_rank(const int32_t* tile_label, int t, int n, bool* last) {
    const int32_t mine = tile_label[t];
    int rank = 0;
    bool later = false;
    for (int i = 0; i < n; ++i) {
        const bool same = tile_label[i] == mine;
        rank += (same && i < t) ? 1 : 0;
        later = later || (same && i > t);
    }
    *last = !later;
    return rank;
}

// segments a cluster of `count` members is cut into
KM_HD int32_t km_segments_of(int32_t count) { return (count + KM_SEGMENT - 1) / KM_SEGMENT; }

// The segment table. seg_off[c] = segments of the clusters before c (seg_off[K] = all), cluster_off[c] = where c's members begin in the
// order. Segment s < seg_off[K] belongs to the cluster c with seg_off[c] <= s < seg_off[c + 1] (found by bisection; empty clusters
// own no segment), is its (s - seg_off[c])-th, begins at member `first` of the order and holds `length` in [1, KM_SEGMENT] members.
struct KmSegment {
    int32_t cluster, first, length;
};
KM_HD KmSegment km_segment(const int32_t* seg_off, const int32_t* cluster_off, int n_clusters, int32_t s) {
    int lo = 0, hi = n_clusters - 1;   // the largest c with seg_off[c] <= s and seg_off[c + 1] > s
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (seg_off[mid + 1] > s) hi = mid;
        else lo = mid + 1;
    }
    const int32_t k = s - seg_off[lo];
    const int32_t count = cluster_off[lo + 1] - cluster_off[lo];
    const int32_t left = count - k * KM_SEGMENT;
    return KmSegment{lo, cluster_off[lo] + k * KM_SEGMENT, left < KM_SEGMENT ? left : KM_SEGMENT};
}

// an upper bound on the segments of any labelling of `allowed` <= rows rows into n_clusters clusters: every cluster has at most one
// segment that is not full
KM_HD int64_t km_max_segments(int64_t rows, int n_clusters) { return rows / KM_SEGMENT + n_clusters; }

}  // namespace rdx
