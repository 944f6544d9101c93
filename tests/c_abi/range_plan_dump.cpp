// range_plan_dump.cpp — plan_range (rag_dpo_amd/csrc/search_plan.hpp) beside plan_search for the same shape, as a program: cases on
// stdin ("rows nq k dim_pad n_cu [option=value ...]"), one line per case on stdout. No GPU, no HIP: tests/test_range.py builds it with
// g++ under ASan and UBSan and checks the rules the threshold search's plan is held to.
//   R: rc exact_only i8 spill use_boot balance stamps bn nqt grid n_streams res fused use_small capw list_cap n_blocks32 n_tiles k
//   S: the same fields of plan_search(nq, k, depth 0) with the options as given
#include <cstdio>
#include <iostream>
#include <sstream>

#include "../../rag_dpo_amd/csrc/search_plan.hpp"

static void print_plan(const char* tag, int rc, const rdx::SearchPlan& p) {
    std::printf("%s %d %d %d %d %d %d %d %d %d %d %d %d %d %d %u %u %lld %lld %d", tag, rc, (int)p.exact_only, (int)p.i8, (int)p.spill, (int)p.use_boot,
                (int)p.balance, (int)p.stamps, p.bn, p.nqt, p.grid, p.n_streams, (int)p.res, (int)p.fused, (int)p.use_small, p.capw, p.list_cap,
                (long long)p.n_blocks32, (long long)p.n_tiles, p.k);
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        long long rows, nq;
        int k, dim_pad, n_cu;
        if (!(in >> rows >> nq >> k >> dim_pad >> n_cu)) continue;
        rdx::SearchOptions o;
        rdx::SearchAdapt a;
        std::string err, tok;
        int rc = RDX_OK;
        while (rc == RDX_OK && in >> tok) {
            const size_t eq = tok.find('=');
            if (eq == std::string::npos) continue;
            rc = rdx::set_search_option(o, a, tok.substr(0, eq).c_str(), std::stoll(tok.substr(eq + 1)), &err);
        }
        rdx::PlanShape s;
        s.rows = rows;
        s.dim_pad = dim_pad;
        s.ksteps = dim_pad / 64;
        s.n_cu = n_cu;
        s.two_e = 2.0f * (1.0e-3f + 2.5e-7f * (float)dim_pad);
        rdx::SearchPlan r, p;
        const int rr = rc ? rc : rdx::plan_range(s, o, nq, k, &r, &err);
        const int rs = rc ? rc : rdx::plan_search(s, o, a, nq, k, 0, false, &p, &err);
        std::printf("%s => ", line.c_str());
        print_plan("R", rr, r);
        std::printf(" | ");
        print_plan("S", rs, p);
        std::printf("\n");
    }
    return 0;
}
