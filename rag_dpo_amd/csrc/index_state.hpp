// index_state.hpp — the two rules of the dense index's state that are arithmetic and nothing else: how many rows the row storage
// is allocated for, and which part of the int8 copy a search has to quantise. No HIP include: a plain C++ compiler builds it
// (tests/c_abi/index_state_dump.cpp pins both against tests/i8_model.py::Copy8 and a restatement of the capacity policy).
#pragma once
#include <algorithm>
#include <cstdint>

namespace rdx {

// ---- capacity: always a multiple of 256 rows (a scan tile) ----------------------------------------------------------------------
constexpr int64_t round256(int64_t n) { return (n + 255) / 256 * 256; }

// what grow() allocates so that `need` rows fit: half as much again as it has, or exactly the need when memory is short. tight == roomy:
// there is nothing to retry with. need <= cap: both are cap, there is nothing to do
struct GrowCaps {
    int64_t roomy, tight;
};
inline GrowCaps grow_caps(int64_t cap, int64_t need) {
    if (need <= cap) return {cap, cap};
    return {round256(std::max(need, cap + cap / 2)), round256(need)};
}

// what a compaction to n_keep rows allocates: no head-room, never nothing
inline int64_t compact_cap(int64_t n_keep) { return std::max<int64_t>(256, round256(n_keep)); }

// ---- the int8 copy: rows [0, valid) are current ----------------------------------------------------------------------------------
// what a search has to quantise before it scans: the 32-row blocks [b0, b0 + nb), nb == 0: nothing. full: the copy is built anew,
// which resets the running eps_max and takes the class edges again
struct I8Work {
    int64_t b0, nb;
    bool full;
};

class I8Watermark {
    int64_t valid_ = 0;

public:
    int64_t valid() const { return valid_; }
    // the writes: an append re-opens the last partial block, everything else may have touched any block
    void appended(int64_t row0) { valid_ = std::min(valid_, row0 / 32 * 32); }
    void rewritten() { valid_ = 0; }     // rows updated in place
    void renumbered() { valid_ = 0; }    // compaction
    void reallocated() { valid_ = 0; }   // the copy's buffers were allocated anew: their contents are gone
    I8Work work(int64_t rows) const {
        if (valid_ >= rows) return {0, 0, false};
        return {valid_ / 32, (rows + 31) / 32 - valid_ / 32, valid_ == 0};
    }
    void quantised(int64_t rows) { valid_ = rows; }   // the work for `rows` rows is enqueued
};

}   // namespace rdx
