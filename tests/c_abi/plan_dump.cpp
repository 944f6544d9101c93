// plan_dump.cpp — the search plan and the option table of rag_dpo_amd/csrc/search_plan.hpp as a program: cases on stdin, one result
// line per case on stdout (format: plan_lines.hpp). No GPU, no HIP: tests/test_search_plan.py builds it with g++ under ASan and UBSan
// and compares its output with the record tests/golden/search_plans.txt.
//
// After " || " a plan line carries what the record does not hold, for the test to check by rule: the plan's fused, fuse_finish,
// pilot, retry, i8_auto and (once more) i8, then the case's ksteps and its options fuse_epilogue, fuse_finish, refine_pilot, retry.
#include <iostream>

#include "../../rag_dpo_amd/csrc/search_plan.hpp"
#include "plan_lines.hpp"

int main() {
    using namespace plan_lines;
    std::string line, err;
    Case c;
    while (std::getline(std::cin, line)) {
        if (!parse_case(line, &c)) continue;
        rdx::SearchOptions o;
        rdx::SearchAdapt a;
        std::string res;
        if (c.probe) {
            a.dense_sample = a.spec_backoff = a.i8_backoff = 5;
            std::copy(PROBE_XW, PROBE_XW + 8, a.xw);
            const int rc = rdx::set_search_option(o, a, c.name.c_str(), c.value, &err);
            res = probe_line(rc, err, o, a);
        } else {
            rdx::PlanShape s;
            s.rows = c.rows;
            s.dim_pad = c.dim_pad;
            s.ksteps = c.dim_pad / 64;
            s.n_cu = c.n_cu;
            s.two_e = 2.0f * (1.0e-3f + 2.5e-7f * (float)c.dim_pad);   // rdx_index::two_e()
            int rc = RDX_OK;
            for (const auto& kv : c.opts)
                if ((rc = rdx::set_search_option(o, a, kv.first.c_str(), kv.second, &err)) != RDX_OK) break;
            a.dense_sample = c.dense_sample;
            a.spec_backoff = c.spec_backoff;
            a.i8_backoff = c.i8_backoff;
            std::copy(c.xw, c.xw + 8, a.xw);
            rdx::SearchPlan p;
            if (rc == RDX_OK) rc = rdx::plan_search(s, o, a, c.nq, c.k, c.depth, c.host_out != 0, &p, &err);
            res = rc ? failed_line(rc, err)
                     : plan_line(p) + " ||" + num(p.fused) + num(p.fuse_finish) + num(p.pilot) + num(p.retry) + num(p.i8_auto) + num(p.i8) + num(s.ksteps) +
                           num(o.fuse_epilogue) + num(o.fuse_finish) + num(o.refine_pilot) + num(o.retry);
        }
        std::printf("%s => %s\n", line.c_str(), res.c_str());
    }
    return 0;
}
