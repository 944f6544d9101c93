"""The case list of tests/golden/search_plans.txt, and the record itself from a plan_dump binary.

    python tests/golden/make_search_plans.py PLAN_DUMP "COMMIT (how it was recorded)"

feeds the cases to PLAN_DUMP (tests/c_abi/plan_dump.cpp built against the tree's search_plan.hpp, see tests/test_search_plan.py;
or any program that reads and prints with tests/c_abi/plan_lines.hpp) and writes the record. Re-record after a change to the
heuristics: the file's diff is then the list of plans that moved. The record keeps only what precedes " || " on a result line, i.e.
the fields the plan had when the format was fixed; the fields behind it are checked by rule in the test."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
RECORD = os.path.join(HERE, "search_plans.txt")

# (rows, dim_pad, nq, k): c1 (exact path), a k_boot + k_scan_small launch, one 64-query tile, the half_boot batch, an automatic int8
# search with the XCD split, c4
SIX = [(16919, 1024, 1, 50), (65536, 1024, 4, 10), (1048576, 1024, 64, 10), (1048576, 1024, 256, 10), (1250000, 1024, 1024, 10),
       (10000000, 1024, 1024, 10)]
BOOLS = ["force_exact", "force_fast", "retry", "xcd_balance", "fuse_epilogue", "half_boot", "small_scan", "split_boot", "fuse_finish",
         "spec_tau", "spread_boot"]
DEFAULT_ON = {"retry", "xcd_balance", "fuse_epilogue", "half_boot", "small_scan", "split_boot", "fuse_finish", "spec_tau", "spread_boot"}
# non-default values, one at a time (ranges: their ends, or an end and a middle)
VALUES = {"profile": [1, 2, 3], "force_bn": [64, 128, 256], "coarse_i8": [0, 1], "refine_pilot": [0, 64], "i8_sample_mul": [1, 2, 4, 8],
          "refine_spill": [0, 1], "refine_list": [32, 1024], "spill_cap": [32, 4096], "sample_div": [1, 1 << 20], "cand_cap": [1, 100000]}
# option probes: accepted values, then one rejected value where the option rejects any (the switches and `profile` take every value)
PROBES = {"profile": [-1, 0, 1, 2, 3, 7], "force_bn": [0, 64, 128, 256, 96], "coarse_i8": [0, 1, 2, 3], "refine_pilot": [0, 1, 4, 64, 65],
          "i8_sample_mul": [0, 1, 2, 4, 8, 3], "refine_spill": [0, 1, 2, -1], "refine_list": [0, 32, 1024, 7168, 7169],
          "spill_cap": [0, 32, 4096, 40960, 31], "sample_div": [1, 64, 1 << 20, 1 << 30, 0], "cand_cap": [0, 1, 8191, 1 << 40, -1]}


def shape(s, **kw):
    r, d, q, k = s
    return f"p r={r} q={kw.pop('q', q)} k={k}" + (f" d={d}" if d != 1024 else "") + "".join(f" {a}={b}" for a, b in kw.items())


def cases():
    out = []
    # the main cross at dim_pad 1024 (the default of a case)
    for r in (0, 1, 1000, 16919, 32768, 32769, 65536, 262144, 1048576, 1250000, 10000000):
        for q in (1, 4, 64, 65, 128, 129, 256, 257, 384, 385, 1024, 4096):
            out += [f"p r={r} q={q} k={k}" for k in (1, 10, 50)]
    # other widths
    out += [f"p r={r} q={q} k=10 d={d}" for d in (64, 448, 4096) for r in (16919, 1048576, 10000000) for q in (1, 64, 256, 1024)]
    # k edges
    out += [f"p r={r} q={q} k={k}" for (r, q) in ((16919, 1), (1048576, 64), (10000000, 1024)) for k in (0, 256, 257)]
    # every option at each non-default value, one at a time
    for s in SIX:
        out += [shape(s, **{n: 0 if n in DEFAULT_ON else 1}) for n in BOOLS]
        out += [shape(s, **{n: v}) for n, vs in VALUES.items() for v in vs]
    # adapt states
    for s in SIX:
        out += [shape(s, dense_sample=200), shape(s, spec_backoff=3), shape(s, i8_backoff=17), shape(s, xw="0.7,0.8,0.9,1,1,1.1,1.2,1.3")]
    # the second pass
    out += [shape(s, q=q, depth=1) for s in SIX for q in (1, 37, 300)]
    # host results on either side of PIN_MAX
    out += [shape(s, q=q, host=1) for s in (SIX[0], SIX[5]) for q in (1024, 4096)]
    # CU counts beside the default 256 (8: a 1024-query batch is more tiles than one launch takes). No 129..256-query shape here: with
    # fewer than 16 CUs its half_boot bootstrap has no streams and the plan divides by zero (no gfx950 part has so few)
    out += [shape(s, c=c) for s in (SIX[1], SIX[2], SIX[4], SIX[5]) for c in (8, 64, 304)]
    # the plan's internal checks: more than 512 streams needs more than 520 CUs; 1024 queries x 72 streams x 8191 slots pass 2^29
    out += ["p r=1048576 q=64 k=10 c=1024", "p r=10000000 q=1024 k=10 c=304 cand_cap=8191", "p r=100000000000 q=64 k=10"]
    # option probes
    for n in BOOLS:
        out += [f"o {n} {v}" for v in (0, 1, -7)]
    out += [f"o {n} {v}" for n, vs in PROBES.items() for v in vs]
    out += ["o no_such_option 1"]
    return out


def run(plan_dump: str) -> list:
    """the result lines of the case list"""
    r = subprocess.run([plan_dump], input="\n".join(cases()) + "\n", capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise RuntimeError(f"{plan_dump} failed ({r.returncode}):\n{r.stdout[-2000:]}{r.stderr[-4000:]}")
    return r.stdout.splitlines()


def recorded(line: str) -> str:
    return line.split(" || ")[0]


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    lines = [recorded(l) for l in run(sys.argv[1])]
    with open(RECORD, "w") as f:
        f.write(f"# search plans and option probes recorded from {sys.argv[2]}; cases and format: tests/c_abi/plan_lines.hpp,\n"
                "# tests/golden/make_search_plans.py\n" + "\n".join(lines) + "\n")
    print(f"{len(lines)} lines, {os.path.getsize(RECORD)} bytes")
