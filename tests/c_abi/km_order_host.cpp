// km_order_host.cpp — the ordering core of rdx_index_kmeans (rag_dpo_amd/csrc/km_order.hpp) rehearsed on the host: the kernels' steps
// (a histogram per block, the scan in (cluster, block) order, placement tile by tile with a running position per cluster, the
// segment table) over several labellings and block spans, against a stable sort by label and a direct cut into segments.
// tests/test_kmeans.py builds it with the address and undefined-behaviour sanitizers. Prints one line per case and "ok"; exit status 1
// on the first difference.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <random>
#include <vector>

#include "../../rag_dpo_amd/csrc/km_order.hpp"

using namespace rdx;

namespace {

struct Order {
    std::vector<int32_t> order, cluster_off, seg_off;
};

// what k_km_hist, k_km_scan, k_km_place and k_km_seg_table do, block by block and tile by tile
Order rehearse(const std::vector<int32_t>& label, int K, int64_t span) {
    const int64_t rows = (int64_t)label.size();
    const int64_t nb = std::max<int64_t>(1, (rows + span - 1) / span);
    std::vector<int32_t> hist((size_t)K * nb + 1, 0);
    for (int64_t b = 0; b < nb; ++b)
        for (int64_t r = b * span; r < std::min(rows, (b + 1) * span); ++r)
            if (label[r] >= 0) ++hist[km_hist_index(label[r], b, nb)];
    int32_t carry = 0;
    for (size_t i = 0; i < (size_t)K * nb; ++i) {
        const int32_t v = hist[i];
        hist[i] = carry;
        carry += v;
    }
    hist[(size_t)K * nb] = carry;
    Order o;
    o.order.assign((size_t)carry, -1);
    for (int64_t b = 0; b < nb; ++b) {
        std::vector<int32_t> run(K);
        for (int c = 0; c < K; ++c) run[c] = hist[km_hist_index(c, b, nb)];
        const int64_t end = std::min(rows, (b + 1) * span);
        for (int64_t t0 = b * span; t0 < end; t0 += KM_TILE) {
            const int n = (int)std::min<int64_t>(KM_TILE, end - t0);
            std::vector<int32_t> tile(label.begin() + t0, label.begin() + t0 + n);   // exactly n entries: a read past the tile is an error
            std::vector<int32_t> moved(run);
            for (int t = 0; t < n; ++t) {
                if (tile[t] < 0) continue;
                bool last = false;
                const int rank = km_tile_rank(tile.data(), t, n, &last);
                o.order.at((size_t)(run[tile[t]] + rank)) = (int32_t)(t0 + t);
                if (last) moved[tile[t]] = run[tile[t]] + rank + 1;
            }
            run = moved;
        }
    }
    o.cluster_off.resize(K + 1);
    o.seg_off.resize(K + 1);
    for (int c = 0; c < K; ++c) o.cluster_off[c] = hist[km_hist_index(c, 0, nb)];
    o.cluster_off[K] = carry;
    int32_t segs = 0;
    for (int c = 0; c < K; ++c) {
        o.seg_off[c] = segs;
        segs += km_segments_of(o.cluster_off[c + 1] - o.cluster_off[c]);
    }
    o.seg_off[K] = segs;
    return o;
}

bool check(const char* name, const std::vector<int32_t>& label, int K, int64_t span) {
    const Order o = rehearse(label, K, span);
    std::vector<int32_t> want;
    for (int32_t r = 0; r < (int32_t)label.size(); ++r)
        if (label[r] >= 0) want.push_back(r);
    std::stable_sort(want.begin(), want.end(), [&](int32_t a, int32_t b) { return label[a] < label[b]; });
    if (o.order != want) {
        std::printf("%s: span %lld: the order differs from a stable sort\n", name, (long long)span);
        return false;
    }
    // the segment table against a direct cut of every cluster
    int32_t s = 0;
    for (int c = 0; c < K; ++c) {
        const int32_t begin = o.cluster_off[c], count = o.cluster_off[c + 1] - begin;
        for (int32_t first = 0; first < count; first += KM_SEGMENT, ++s) {
            const KmSegment seg = km_segment(o.seg_off.data(), o.cluster_off.data(), K, s);
            if (seg.cluster != c || seg.first != begin + first || seg.length != std::min<int32_t>(KM_SEGMENT, count - first)) {
                std::printf("%s: segment %d is (%d, %d, %d)\n", name, s, seg.cluster, seg.first, seg.length);
                return false;
            }
        }
    }
    if (s != o.seg_off[K] || (int64_t)s > km_max_segments((int64_t)label.size(), K)) {
        std::printf("%s: %d segments, table says %d, bound %lld\n", name, s, o.seg_off[K], (long long)km_max_segments((int64_t)label.size(), K));
        return false;
    }
    return true;
}

bool run(const char* name, const std::vector<int32_t>& label, int K) {
    for (int64_t span : {256, 512, 768, 4096, 1 << 20})
        if (!check(name, label, K, span)) return false;
    std::printf("%s: %zu rows, %d clusters\n", name, label.size(), K);
    return true;
}

}  // namespace

int main() {
    std::mt19937 rng(12345);
    bool ok = true;
    for (int rows : {1, 63, 257, 4097, 8229}) {
        std::vector<int32_t> l(rows);
        for (int r = 0; r < rows; ++r) l[r] = r % 5;
        ok = ok && run("interleaved", l, 5);
    }
    {
        std::vector<int32_t> l(8229);
        for (auto& v : l) v = (int32_t)(rng() % 70) - 5;   // -5..-1: not allowed (the kernels map them to -1)
        for (auto& v : l) v = v < 0 ? -1 : v;
        ok = ok && run("random with gaps", l, 65);
    }
    {
        std::vector<int32_t> l;   // clusters of exactly 0, 1, 255, 256, 257, 512, 513 members, shuffled
        const int sizes[7] = {0, 1, 255, 256, 257, 512, 513};
        for (int c = 0; c < 7; ++c) l.insert(l.end(), sizes[c], c);
        std::shuffle(l.begin(), l.end(), rng);
        ok = ok && run("segment borders", l, 7);
    }
    {
        std::vector<int32_t> l(5000, 4095);   // one cluster, the last of 4 096
        ok = ok && run("one cluster", l, 4096);
        std::fill(l.begin(), l.end(), -1);
        ok = ok && run("no row allowed", l, 3);
        for (int r = 0; r < 5000; ++r) l[r] = r % 4096;
        ok = ok && run("more clusters than a tile", l, 4096);
    }
    // the block span: a multiple of the tile that keeps clusters x blocks within KM_MAX_HIST
    for (int64_t rows : {(int64_t)1, (int64_t)256, (int64_t)257, (int64_t)1 << 20, ((int64_t)1 << 31) - 1})
        for (int K : {1, 2, 256, 4096}) {
            const int64_t span = km_block_span(rows, K), nb = (rows + span - 1) / span;
            if (span < KM_TILE || span % KM_TILE || nb * K > KM_MAX_HIST || (span > KM_TILE && ((rows + span - KM_TILE - 1) / (span - KM_TILE)) * K <= KM_MAX_HIST)) {
                std::printf("km_block_span(%lld, %d) = %lld\n", (long long)rows, K, (long long)span);
                ok = false;
            }
        }
    if (!ok) return 1;
    std::printf("ok\n");
    return 0;
}
