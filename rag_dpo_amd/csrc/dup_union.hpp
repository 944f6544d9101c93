// dup_union.hpp — the union core of near-duplicate clustering (rdx_index_near_dup): a lock-free union-find over an
// int32 parent array. No HIP include: a plain C++ compiler builds it with the host policy (tests/c_abi/dup_union_host.cpp rehearses it
// with threads under the sanitizers), hipcc builds the same text for the device with dup_kernel.hpp's policy.
//
// State. parent[x] is -1 for a row outside the problem (never read past, never written) and otherwise a row in [0, x]:
//   INVARIANT  0 <= parent[x] <= x  for every row inside, at every moment.
// A row with parent[x] == x is a root. The words change in two ways only, both by compare-and-swap, both to a SMALLER value:
//   link     parent[hi]: hi -> lo  with lo < hi a root when it was read (dup_unite). A root becomes a non-root, for good: nothing ever
//            writes x into parent[x] again.
//   halving  parent[x]: p -> parent[p]  with p != x (dup_find, optional). x is a non-root before and after; parent[p] <= p < x.
// So every word is non-increasing over time, a word below its index stays below it, and the set of a row's ancestors only ever
// merges with other sets: rows that were connected stay connected, and rows are connected only by links, each of which joins the
// sets of the two rows some dup_unite was called with.
//
// Termination — there is no wait on another thread anywhere; every loop iteration either ends the call or has seen a parent word that
// strictly decreased:
//   dup_find   steps from x to p = parent[x] only when p != x, hence p < x by the invariant: the walk strictly descends and ends after
//              at most x steps whatever other threads do meanwhile. A failed halving compare-and-swap is not retried.
//   dup_unite  an iteration ends the call (equal roots, or its compare-and-swap succeeded) or its compare-and-swap on parent[hi]
//              failed. dup_find had just read parent[hi] == hi; the failure returned a smaller value: somebody else's LINK of hi (a
//              halving never touches a root). The loop continues from the value the compare-and-swap returned. Each failure is thus
//              paid for by a distinct successful link, every successful link turns a root into a non-root for good, so there are at
//              most rows - 1 successful compare-and-swap links in all, and at most that many failures per call.
//
// Result. After every dup_unite of a set of edges has returned (in any order, from any number of threads), two rows have the same
// root iff they are connected by the edges, and the root is the smallest row of the component (a link only ever puts the larger
// root under the smaller): dup_find(r) == the label of the definition (rag_dpo_amd/dedup.py).
//
// Memory. The policy P supplies the word type and two operations, and is the only thing that touches the array:
//   P::word                      the array's element (std::atomic<int32_t> on the host, int32_t on the device)
//   P::load(const word* p)       an atomic load
//   P::cas(word* p, e, d)        atomic compare-and-swap of *p from e to d; returns the value it found (== e: it succeeded)
// Relaxed order suffices: no other memory is published through these words, and the arguments above use only the per-word
// modification order. On the device both are agent-scope operations (dup_kernel.hpp says why plain accesses would be wrong).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define RDX_DUP_FN __host__ __device__ __forceinline__
#else
#define RDX_DUP_FN inline
#endif

namespace rdx {

// the root of x, or -1 for a row outside the problem. HALVE: shorten the path on the way (compare-and-swap writes that keep the
// invariant); false = read-only.
template <class P, bool HALVE>
RDX_DUP_FN int32_t dup_find(typename P::word* parent, int32_t x) {
    int32_t p = P::load(parent + x);
    if (p < 0) return -1;
    while (p != x) {                              // p < x
        const int32_t gp = P::load(parent + p);   // gp <= p
        if (HALVE && gp != p) (void)P::cas(parent + x, p, gp);   // gp < p < x; lost to another write: that one lowered it too
        x = p;
        p = gp;
    }
    return x;
}

// whether a and b have the same root right now, without a write (dense clusters ask this far more often than they link)
template <class P>
RDX_DUP_FN bool dup_same(typename P::word* parent, int32_t a, int32_t b) {
    return dup_find<P, false>(parent, a) == dup_find<P, false>(parent, b);
}

// join the sets of a and b; true = this call made the link. Rows outside the problem join nothing.
template <class P>
RDX_DUP_FN bool dup_unite(typename P::word* parent, int32_t a, int32_t b) {
    for (;;) {
        a = dup_find<P, true>(parent, a);
        b = dup_find<P, true>(parent, b);
        if (a < 0 || b < 0 || a == b) return false;
        const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const int32_t was = P::cas(parent + hi, hi, lo);
        if (was == hi) return true;
        a = was;                                  // hi was linked under `was` < hi by somebody else: go on from there
        b = lo;
    }
}

}   // namespace rdx

#if !defined(__HIP_DEVICE_COMPILE__)
#include <atomic>
namespace rdx {
struct DupHostPolicy {
    using word = std::atomic<int32_t>;
    static int32_t load(const word* p) { return p->load(std::memory_order_relaxed); }
    static int32_t cas(word* p, int32_t expected, int32_t desired) {
        p->compare_exchange_strong(expected, desired, std::memory_order_relaxed, std::memory_order_relaxed);
        return expected;
    }
};
}   // namespace rdx
#endif
