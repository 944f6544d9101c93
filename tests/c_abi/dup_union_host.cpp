// dup_union_host.cpp — the union core (rag_dpo_amd/csrc/dup_union.hpp) rehearsed on the host: eight threads unite the edges of
// several graphs in shuffled orders through the std::atomic policy, and the labels must equal those of a plain sequential
// union-find. tests/test_dedup.py builds it twice (address + undefined-behaviour sanitizers; thread sanitizer) and runs it under a
// time limit: a loop that can spin shows up here. Prints one line per graph and "ok"; exit status 1 on the first difference.
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <random>
#include <thread>
#include <utility>
#include <vector>

#include "../../rag_dpo_amd/csrc/dup_union.hpp"

using Edge = std::pair<int32_t, int32_t>;
using rdx::DupHostPolicy;

namespace {

// the definition: sequential union-find, label = smallest row of the component, -1 outside
std::vector<int32_t> sequential_labels(int32_t n, const std::vector<char>& inside, const std::vector<Edge>& edges) {
    std::vector<int32_t> p(n);
    for (int32_t i = 0; i < n; ++i) p[i] = i;
    auto find = [&](int32_t x) {
        while (p[x] != x) x = p[x] = p[p[x]];
        return x;
    };
    for (const Edge& e : edges) {
        if (!inside[e.first] || !inside[e.second]) continue;
        const int32_t a = find(e.first), b = find(e.second);
        if (a != b) p[std::max(a, b)] = std::min(a, b);
    }
    std::vector<int32_t> out(n);
    for (int32_t i = 0; i < n; ++i) out[i] = inside[i] ? find(i) : -1;
    return out;
}

bool run(const char* name, int32_t n, const std::vector<char>& inside, std::vector<Edge> edges, unsigned seed, int n_threads = 8) {
    const std::vector<int32_t> want = sequential_labels(n, inside, edges);
    std::mt19937 rng(seed);
    std::shuffle(edges.begin(), edges.end(), rng);
    for (Edge& e : edges)
        if (rng() & 1) std::swap(e.first, e.second);
    std::unique_ptr<std::atomic<int32_t>[]> parent(new std::atomic<int32_t>[n]);
    for (int32_t i = 0; i < n; ++i) parent[i].store(inside[i] ? i : -1, std::memory_order_relaxed);
    std::atomic<long> links{0};
    std::vector<std::thread> pool;
    for (int t = 0; t < n_threads; ++t) {
        pool.emplace_back([&, t] {
            long mine = 0;
            // interleaved shares: neighbouring edges go to different threads, and every other thread walks its share backwards
            const size_t m = edges.size();
            const size_t share = m > (size_t)t ? (m - t + n_threads - 1) / n_threads : 0;
            for (size_t i = 0; i < share; ++i) {
                const Edge& e = edges[t + ((t & 1) ? share - 1 - i : i) * n_threads];
                if (e.first != e.second && !rdx::dup_same<DupHostPolicy>(parent.get(), e.first, e.second))
                    mine += rdx::dup_unite<DupHostPolicy>(parent.get(), e.first, e.second) ? 1 : 0;
            }
            links.fetch_add(mine, std::memory_order_relaxed);
        });
    }
    for (std::thread& th : pool) th.join();
    int32_t n_inside = 0, n_comp = 0;
    for (int32_t i = 0; i < n; ++i) {
        const int32_t p = parent[i].load(std::memory_order_relaxed);
        if (inside[i] ? (p < 0 || p > i) : p != -1) {
            std::printf("%s: the invariant parent[x] <= x is broken at %d (%d)\n", name, i, p);
            return false;
        }
        const int32_t got = inside[i] ? rdx::dup_find<DupHostPolicy, false>(parent.get(), i) : -1;
        if (got != want[i]) {
            std::printf("%s: label[%d] = %d, the sequential union-find says %d\n", name, i, got, want[i]);
            return false;
        }
        n_inside += inside[i] ? 1 : 0;
        n_comp += inside[i] && want[i] == i ? 1 : 0;
    }
    // every successful link removed exactly one root
    if (links.load() != (long)n_inside - n_comp) {
        std::printf("%s: %ld successful links for %d rows in %d components\n", name, links.load(), n_inside, n_comp);
        return false;
    }
    std::printf("%s: %d rows, %zu edges, %d components, %ld links\n", name, n, edges.size(), n_comp, links.load());
    return true;
}

}   // namespace

int main() {
    bool ok = true;
    std::mt19937 rng(12345);
    {   // a chain of 50 000
        const int32_t n = 50000;
        std::vector<Edge> e;
        for (int32_t i = 0; i + 1 < n; ++i) e.push_back({i, i + 1});
        ok = ok && run("chain", n, std::vector<char>(n, 1), e, 1);
    }
    {   // a star of 50 000, its centre not the smallest row
        const int32_t n = 50000, c = 31337;
        std::vector<Edge> e;
        for (int32_t i = 0; i < n; ++i)
            if (i != c) e.push_back({c, i});
        ok = ok && run("star", n, std::vector<char>(n, 1), e, 2);
    }
    {   // 200 cliques of 50 joined by single bridges: every thread hammers the same few roots
        const int32_t n = 200 * 50;
        std::vector<Edge> e;
        for (int32_t c = 0; c < 200; ++c) {
            for (int32_t a = 0; a < 50; ++a)
                for (int32_t b = a + 1; b < 50; ++b) e.push_back({c * 50 + a, c * 50 + b});
            if (c + 1 < 200) e.push_back({c * 50 + 49, (c + 1) * 50 + 17});
        }
        ok = ok && run("cliques", n, std::vector<char>(n, 1), e, 3);
    }
    {   // a random sparse graph: about 0.6 edges per row, many components of every size
        const int32_t n = 60000;
        std::vector<Edge> e;
        for (int32_t i = 0; i < 36000; ++i) e.push_back({(int32_t)(rng() % n), (int32_t)(rng() % n)});
        ok = ok && run("sparse", n, std::vector<char>(n, 1), e, 4);
    }
    {   // excluded rows: a chain with every seventh row outside (it splits there), and a random graph with a third outside
        const int32_t n = 20000;
        std::vector<char> in(n, 1);
        for (int32_t i = 3; i < n; i += 7) in[i] = 0;
        std::vector<Edge> e;
        for (int32_t i = 0; i + 1 < n; ++i) e.push_back({i, i + 1});
        ok = ok && run("chain with gaps", n, in, e, 5);
        std::vector<char> in2(n, 1);
        for (int32_t i = 0; i < n; ++i) in2[i] = rng() % 3 != 0;
        std::vector<Edge> e2;
        for (int32_t i = 0; i < 30000; ++i) e2.push_back({(int32_t)(rng() % n), (int32_t)(rng() % n)});
        ok = ok && run("sparse with gaps", n, in2, e2, 6);
    }
    {   // everything at once on one root: a clique of 400 given to the threads twice over
        const int32_t n = 400;
        std::vector<Edge> e;
        for (int rep = 0; rep < 2; ++rep)
            for (int32_t a = 0; a < n; ++a)
                for (int32_t b = a + 1; b < n; ++b) e.push_back({a, b});
        ok = ok && run("clique", n, std::vector<char>(n, 1), e, 7);
    }
    std::printf(ok ? "ok\n" : "FAILED\n");
    return ok ? 0 : 1;
}
