// index_state_dump.cpp — the two rules of rag_dpo_amd/csrc/index_state.hpp as a program: event scripts on stdin, one result line per
// line on stdout. No GPU, no HIP: tests/test_index_state.py builds it with g++ under ASan and UBSan and compares its output with
// tests/i8_model.py::Copy8 and with a restatement of the capacity policy.
//
//   w EVENT...     one fresh watermark; events: a<row0> append from row0, u update in place, c compaction, r reallocation,
//                  p<rows> a search of `rows` rows: prints "valid b0 nb full" as they stand BEFORE the work is marked as enqueued
//   g CAP NEED     grow_caps: prints "roomy tight"
//   k N_KEEP       compact_cap: prints the capacity
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "../../rag_dpo_amd/csrc/index_state.hpp"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string kind, ev;
        in >> kind;
        if (kind == "g") {
            long long cap = 0, need = 0;
            in >> cap >> need;
            const rdx::GrowCaps c = rdx::grow_caps(cap, need);
            std::printf("%lld %lld\n", (long long)c.roomy, (long long)c.tight);
        } else if (kind == "k") {
            long long n = 0;
            in >> n;
            std::printf("%lld\n", (long long)rdx::compact_cap(n));
        } else if (kind == "w") {
            rdx::I8Watermark m;
            std::string out;
            while (in >> ev) {
                const long long arg = ev.size() > 1 ? std::stoll(ev.substr(1)) : 0;
                if (ev[0] == 'a') m.appended(arg);
                else if (ev[0] == 'u') m.rewritten();
                else if (ev[0] == 'c') m.renumbered();
                else if (ev[0] == 'r') m.reallocated();
                else if (ev[0] == 'p') {
                    const rdx::I8Work w = m.work(arg);
                    char buf[128];
                    std::snprintf(buf, sizeof buf, "%s%lld %lld %lld %d", out.empty() ? "" : " | ", (long long)m.valid(), (long long)w.b0,
                                  (long long)w.nb, w.full ? 1 : 0);
                    out += buf;
                    if (w.nb > 0) m.quantised(arg);
                } else {
                    std::fprintf(stderr, "unknown event %s\n", ev.c_str());
                    return 2;
                }
            }
            std::printf("%s\n", out.c_str());
        } else {
            std::fprintf(stderr, "unknown line %s\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
