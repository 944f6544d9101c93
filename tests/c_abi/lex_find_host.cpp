// lex_find_host.cpp — the posting lookup of rdx_lex_score_pairs (rag_dpo_amd/csrc/lex_find.hpp) rehearsed on the host: every span length
// 0 .. 9, 64 and 4 097, with the first key, the last, every key in between, a key below the span, every absent key between two
// neighbours and a key above it, against a linear scan. Each span is a heap block of exactly its length, so a read outside it is an
// error under the address sanitizer. tests/test_m3.py builds it with the address and undefined-behaviour sanitizers. Prints one line
// per length and "ok"; exit status 1 on the first difference.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../rag_dpo_amd/csrc/lex_find.hpp"

using namespace rdx;

namespace {

int64_t linear(const std::vector<int32_t>& a, int32_t key) {
    for (size_t i = 0; i < a.size(); ++i)
        if (a[i] == key) return (int64_t)i;
    return -1;
}

bool check(const std::vector<int32_t>& a, int32_t key) {
    // a copy of exactly n entries on the heap (n = 0: a block of no bytes)
    int32_t* span = new int32_t[a.size()];
    for (size_t i = 0; i < a.size(); ++i) span[i] = a[i];
    const int64_t got = lex_find(span, (int64_t)a.size(), key), want = linear(a, key);
    delete[] span;
    if (got != want) std::printf("length %zu: key %d found at %lld, a scan says %lld\n", a.size(), key, (long long)got, (long long)want);
    return got == want;
}

bool run(size_t n, std::mt19937& rng) {
    // strictly ascending with gaps of 2 .. 5, so that there is an absent key between any two neighbours; the first value is 10
    std::vector<int32_t> a(n);
    int32_t v = 10;
    for (size_t i = 0; i < n; ++i) {
        a[i] = v;
        v += 2 + (int32_t)(rng() % 4);
    }
    long keys = 0;
    bool ok = check(a, 9) && check(a, 0) && check(a, -5) && check(a, INT32_MIN);   // absent below
    ok = ok && check(a, v) && check(a, INT32_MAX);                                  // absent above
    keys += 6;
    for (size_t i = 0; i < n && ok; ++i) {
        ok = check(a, a[i]) && check(a, a[i] + 1);                                  // present (the first and the last among them); absent between
        keys += 2;
    }
    if (ok) std::printf("length %zu: %ld keys\n", n, keys);
    return ok;
}

}  // namespace

int main() {
    std::mt19937 rng(4097);
    bool ok = true;
    for (size_t n = 0; n <= 9 && ok; ++n) ok = run(n, rng);
    ok = ok && run(64, rng) && run(4097, rng);
    // the extremes of the key range as values
    ok = ok && check({INT32_MIN, -1, 0, INT32_MAX}, INT32_MIN) && check({INT32_MIN, -1, 0, INT32_MAX}, INT32_MAX) && check({INT32_MIN, -1, 0, INT32_MAX}, 1);
    if (!ok) return 1;
    std::printf("ok\n");
    return 0;
}
