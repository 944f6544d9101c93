// lex_find.hpp — the posting lookup of rdx_lex_score_pairs, HIP-free: where a key lies in a strictly ascending int32
// span. lex_pairs_kernel.hpp calls it from its kernel, over a term's tile directory and over its postings;
// tests/c_abi/lex_find_host.cpp rehearses it on the CPU under the address and undefined-behaviour sanitizers.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define LEX_HD __host__ __device__ inline
#else
#define LEX_HD inline
#endif

namespace rdx {

// the position of `key` in a[0 .. n), strictly ascending, or -1 when it is not there. Reads a[0 .. n) only; n = 0 reads nothing.
LEX_HD int64_t lex_find(const int32_t* a, int64_t n, int32_t key) {
    int64_t lo = 0, hi = n;   // the first position whose value is >= key lies in [lo, hi]
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && a[lo] == key ? lo : -1;
}

}  // namespace rdx
