// plan_classes.cpp — SearchPlan::eps_classes and option "i8_eps_classes" of rag_dpo_amd/csrc/search_plan.hpp as a stand-alone
// program (no GPU, no HIP): tests/test_plan_classes.py builds it with g++ under ASan and UBSan and expects its last line.
//
// The rule (DESIGN.md §5 "classes of eps_b"): the int8 scan's emit threshold comes in EPS_CLASSES classes of block error exactly on
// the plans where coarse_i8 = 2 chose the int8 pass at depth 0 (i8_auto), and in one class on every other plan — forced int8, the
// second-chance batch, fp16, small launches, the exact path; option i8_eps_classes = 1, 2, 4, 8 sets it for every int8 search.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "../../rag_dpo_amd/csrc/search_plan.hpp"

static int failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                     \
        }                                                                   \
    } while (0)

static rdx::PlanShape shape(int64_t rows, int dim_pad) {
    rdx::PlanShape s;
    s.rows = rows;
    s.dim_pad = dim_pad;
    s.ksteps = dim_pad / 64;
    s.n_cu = 256;
    s.two_e = 2.0f * (1.0e-3f + 2.5e-7f * (float)dim_pad);
    return s;
}

static rdx::SearchPlan plan(const rdx::PlanShape& s, const rdx::SearchOptions& o, const rdx::SearchAdapt& a, int64_t nq, int k, int depth) {
    rdx::SearchPlan p;
    std::string err;
    const int rc = rdx::plan_search(s, o, a, nq, k, depth, false, &p, &err);
    if (rc != RDX_OK) {
        std::printf("plan_search failed (%d): %s\n", rc, err.c_str());
        ++failures;
    }
    return p;
}

int main() {
    using namespace rdx;
    const SearchOptions dflt;
    const SearchAdapt calm;
    std::string err;
    CHECK(dflt.i8_eps_classes == 0);
    CHECK(SearchPlan{}.eps_classes == 1);
    CHECK(I8_AUTO_EPS_CLASSES == 8 && EPS_CLASSES == 8);

    // automatic int8 at depth 0: more than 256 queries on at least 2^20 rows, dim_pad a multiple of 128 up to 1024
    int n_auto = 0;
    for (int64_t rows : {(int64_t)1 << 20, (int64_t)1250000, (int64_t)10000000})
        for (int dim_pad : {128, 512, 896, 1024})
            for (int64_t nq : {257, 512, 1024, 1030}) {
                const SearchPlan p = plan(shape(rows, dim_pad), dflt, calm, nq, 10, 0);
                CHECK(p.i8 && p.i8_auto && p.eps_classes == 8);
                ++n_auto;
                const SearchPlan d1 = plan(shape(rows, dim_pad), dflt, calm, nq, 10, 1);   // the second-chance batch: fp16
                CHECK(!d1.i8 && !d1.i8_auto && d1.eps_classes == 1);
                SearchOptions forced = dflt;   // forced int8: one class, as i8_sample_mul and refine_spill have it
                SearchAdapt a = calm;
                CHECK(set_search_option(forced, a, "coarse_i8", 1, &err) == RDX_OK);
                const SearchPlan f = plan(shape(rows, dim_pad), forced, calm, nq, 10, 0);
                CHECK(f.i8 && !f.i8_auto && f.eps_classes == 1);
                SearchOptions never = dflt;
                CHECK(set_search_option(never, a, "coarse_i8", 0, &err) == RDX_OK);
                const SearchPlan h = plan(shape(rows, dim_pad), never, calm, nq, 10, 0);
                CHECK(!h.i8 && h.eps_classes == 1);
            }
    CHECK(n_auto == 48);

    // every plan that is not automatic int8 keeps one class: below the row gate, at most 256 queries, a width int8 does not take,
    // small launches (k_boot / k_scan_small), the exact path, the int8 back-off
    {
        CHECK(plan(shape(((int64_t)1 << 20) - 1, 1024), dflt, calm, 1024, 10, 0).eps_classes == 1);
        CHECK(plan(shape(10000000, 1024), dflt, calm, 256, 10, 0).eps_classes == 1);
        CHECK(plan(shape(10000000, 1024), dflt, calm, 64, 10, 0).eps_classes == 1);
        CHECK(plan(shape(10000000, 2048), dflt, calm, 1024, 10, 0).eps_classes == 1);
        CHECK(plan(shape(10000000, 1088), dflt, calm, 1024, 10, 0).eps_classes == 1);
        const SearchPlan small = plan(shape(100000, 1024), dflt, calm, 4, 10, 0);
        CHECK(small.use_small && small.eps_classes == 1);
        const SearchPlan exact = plan(shape(16919, 1024), dflt, calm, 1, 50, 0);
        CHECK(exact.exact_only && exact.eps_classes == 1);
        const SearchPlan bigk = plan(shape(10000000, 1024), dflt, calm, 1024, 300, 0);
        CHECK(bigk.exact_only && bigk.eps_classes == 1);
        SearchAdapt backed = calm;
        backed.i8_backoff = 3;
        const SearchPlan b = plan(shape(10000000, 1024), dflt, backed, 1024, 10, 0);
        CHECK(!b.i8 && !b.i8_auto && b.eps_classes == 1);
    }

    // the option: 0 (automatic), 1, 2, 4, 8 are taken and rule every int8 plan, forced or automatic; fp16 plans stay at one class
    for (int v : {0, 1, 2, 4, 8}) {
        SearchOptions o = dflt;
        SearchAdapt a = calm;
        CHECK(set_search_option(o, a, "i8_eps_classes", v, &err) == RDX_OK);
        CHECK(o.i8_eps_classes == v);
        CHECK(plan(shape(10000000, 1024), o, a, 1024, 10, 0).eps_classes == (v ? v : 8));
        CHECK(plan(shape(10000000, 1024), o, a, 1024, 10, 1).eps_classes == 1);
        CHECK(plan(shape(10000000, 1024), o, a, 64, 10, 0).eps_classes == 1);
        CHECK(set_search_option(o, a, "coarse_i8", 1, &err) == RDX_OK);
        const SearchPlan f = plan(shape(60000, 1024), o, a, 300, 10, 0);
        CHECK(f.i8 && !f.i8_auto && f.eps_classes == (v ? v : 1));
    }
    for (int v : {3, 16, -1, 5, 6, 7, 9, 32}) {
        SearchOptions o = dflt;
        SearchAdapt a = calm;
        CHECK(set_search_option(o, a, "i8_eps_classes", 4, &err) == RDX_OK);
        err.clear();
        CHECK(set_search_option(o, a, "i8_eps_classes", v, &err) == RDX_ERR_INVALID);
        CHECK(err == "i8_eps_classes must be 0 (automatic), 1, 2, 4 or 8");
        CHECK(o.i8_eps_classes == 4);   // refused: nothing changed
    }

    // the classes change nothing else of a plan: the automatic plan with 8 classes and with 1 agree on every sized field
    {
        SearchOptions one = dflt;
        SearchAdapt a = calm;
        CHECK(set_search_option(one, a, "i8_eps_classes", 1, &err) == RDX_OK);
        const SearchPlan p8 = plan(shape(10000000, 1024), dflt, calm, 1024, 10, 0), p1 = plan(shape(10000000, 1024), one, calm, 1024, 10, 0);
        CHECK(p8.eps_classes == 8 && p1.eps_classes == 1);
        CHECK(p8.capw == p1.capw && p8.list_cap == p1.list_cap && p8.expected_per_query == p1.expected_per_query && p8.div == p1.div &&
              p8.sample_rows == p1.sample_rows && p8.spill == p1.spill && p8.spill_cap == p1.spill_cap && p8.k_sel == p1.k_sel &&
              p8.n_streams == p1.n_streams && p8.grid == p1.grid && p8.bn == p1.bn);
    }

    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("plan classes ok\n");
    return 0;
}
