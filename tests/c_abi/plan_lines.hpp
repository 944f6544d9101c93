// plan_lines.hpp — the case reader and the line printer of tests/c_abi/plan_dump.cpp, kept apart from it so that the record
// tests/golden/search_plans.txt can be taken from any commit's plan code with the very same reader and printer (they are templates
// over the plan / option types: whatever has the fields by these names prints).
//
// A case is one line of blank-separated words, the first of which says its form:
//   p r=<rows> q=<nq> k=<k> [d=<dim_pad>] [c=<n_cu>] [depth=1] [host=1] [<option>=<value> ...] [dense_sample=N] [spec_backoff=N]
//     [i8_backoff=N] [xw=<w0>,..,<w7>]                                        a plan case (dim_pad defaults to 1024, n_cu to 256)
//   o <option> <value>                                                        an option probe
// and its result line is "<case> => <result>":
//   plan, failed:   E<code> <message>
//   plan:           0| nq k depth nq_pad prof exact_only| bn nqt grid G n_streams n_sets res n_tiles n_blocks32| use_boot boot_units
//                   boot_sets bn_b nqt_b n_sets_b div n_sets_used boot_tiles boot_wave_off boot_row_off boot_span| use_small i8 sample_rows
//                   expected_per_query capw list_cap spill spill_cap k_sel slack| balance bulk_it xlo[0..8] stamps| ride big_copy b_s b_r b_c
//                   ("=" for a group: every field of it as in a default-constructed plan)
//   probe:          <code> [<message>]| force_exact force_fast profile retry xcd_balance fuse_epilogue force_bn half_boot small_scan
//                   split_boot fuse_finish spec_tau spread_boot coarse_i8 refine_pilot i8_sample_mul refine_spill refine_list spill_cap
//                   sample_div cand_cap| dense_sample spec_backoff i8_backoff xw[0..7]
// A probe starts from the defaults with dense_sample = spec_backoff = i8_backoff = 5 and xw = PROBE_XW, so that the resets show.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

namespace plan_lines {

static const double PROBE_XW[8] = {0.5, 0.75, 1, 1, 1, 1.25, 1.25, 1.25};

struct Case {
    bool probe = false;
    std::string name;   // probe: the option and its value
    int64_t value = 0;
    int64_t rows = 0, nq = 0;   // plan case
    int dim_pad = 1024, n_cu = 256, k = 0, depth = 0, host_out = 0;
    std::vector<std::pair<std::string, int64_t>> opts;
    int dense_sample = 0, spec_backoff = 0, i8_backoff = 0;
    double xw[8] = {1, 1, 1, 1, 1, 1, 1, 1};
};

// false: an empty line or a comment
inline bool parse_case(const std::string& line, Case* c) {
    *c = Case{};
    std::istringstream in(line);
    std::string form, w;
    if (!(in >> form) || form[0] == '#') return false;
    if (form == "o") {
        c->probe = true;
        in >> c->name >> c->value;
        return true;
    }
    while (in >> w) {
        const size_t eq = w.find('=');
        const std::string key = w.substr(0, eq), val = w.substr(eq + 1);
        const int64_t v = std::strtoll(val.c_str(), nullptr, 10);
        if (key == "r") c->rows = v;
        else if (key == "d") c->dim_pad = (int)v;
        else if (key == "q") c->nq = v;
        else if (key == "k") c->k = (int)v;
        else if (key == "c") c->n_cu = (int)v;
        else if (key == "depth") c->depth = (int)v;
        else if (key == "host") c->host_out = (int)v;
        else if (key == "dense_sample") c->dense_sample = (int)v;
        else if (key == "spec_backoff") c->spec_backoff = (int)v;
        else if (key == "i8_backoff") c->i8_backoff = (int)v;
        else if (key == "xw") {
            const char* s = val.c_str();
            for (int x = 0; x < 8; ++x) {
                char* end;
                c->xw[x] = std::strtod(s, &end);
                s = *end ? end + 1 : end;
            }
        } else
            c->opts.emplace_back(key, v);
    }
    return true;
}

inline std::string num(long long v) { return " " + std::to_string(v); }
inline std::string flt(const char* fmt, double v) {
    char b[40];
    std::snprintf(b, sizeof b, fmt, v);
    return std::string(" ") + b;
}

inline std::string failed_line(int rc, const std::string& msg) { return "E" + std::to_string(rc) + " " + msg; }

// the six groups of a plan's fields
template <class Plan>
std::vector<std::string> plan_groups(const Plan& p) {
    std::vector<std::string> g(6);
    g[0] = num(p.nq) + num(p.k) + num(p.depth) + num(p.nq_pad) + num(p.prof) + num(p.exact_only);
    g[1] = num(p.bn) + num(p.nqt) + num(p.grid) + num(p.G) + num(p.n_streams) + num(p.n_sets) + num(p.res) + num(p.n_tiles) + num(p.n_blocks32);
    g[2] = num(p.use_boot) + num(p.boot_units) + num(p.boot_sets) + num(p.bn_b) + num(p.nqt_b) + num(p.n_sets_b) + num(p.div) + num(p.n_sets_used) +
           num(p.boot_tiles) + num(p.boot_wave_off) + num(p.boot_row_off) + num(p.boot_span);
    g[3] = num(p.use_small) + num(p.i8) + num(p.sample_rows) + flt("%.17g", p.expected_per_query) + num(p.capw) + num(p.list_cap) + num(p.spill) +
           num(p.spill_cap) + num(p.k_sel) + flt("%.9g", p.slack);
    g[4] = num(p.balance) + num(p.bulk_it);
    for (int x = 0; x < 9; ++x) g[4] += num(p.xlo[x]);
    g[4] += num(p.stamps);
    g[5] = num(p.ride) + num(p.big_copy) + num((long long)p.b_s) + num((long long)p.b_r) + num((long long)p.b_c);
    return g;
}

template <class Plan>
std::string plan_line(const Plan& p) {
    const std::vector<std::string> g = plan_groups(p), g0 = plan_groups(Plan{});
    std::string s = "0";
    for (size_t i = 0; i < g.size(); ++i) s += "|" + (g[i] == g0[i] ? std::string(" =") : g[i]);
    return s;
}

template <class Opt, class Adapt>
std::string probe_line(int rc, const std::string& msg, const Opt& o, const Adapt& a) {
    std::string s = std::to_string(rc) + (rc ? " " + msg : "") + "|";
    s += num(o.force_exact) + num(o.force_fast) + num(o.profile) + num(o.retry) + num(o.xcd_balance) + num(o.fuse_epilogue) + num(o.force_bn) +
         num(o.half_boot) + num(o.small_scan) + num(o.split_boot) + num(o.fuse_finish) + num(o.spec_tau) + num(o.spread_boot) + num(o.coarse_i8) +
         num(o.refine_pilot) + num(o.i8_sample_mul) + num(o.refine_spill) + num(o.refine_list) + num(o.spill_cap) + num(o.sample_div) +
         num(o.cand_cap) + "|";
    s += num(a.dense_sample) + num(a.spec_backoff) + num(a.i8_backoff);
    for (int x = 0; x < 8; ++x) s += flt("%.17g", a.xw[x]);
    return s;
}

}   // namespace plan_lines
