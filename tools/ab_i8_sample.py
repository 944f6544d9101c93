"""A/B of the int8 pass's threshold-sample density (option i8_sample_mul) against another library, on the contract bench:

    python tools/ab_i8_sample.py --base tools/librdx_parent.so [--shape iid|embed] [--rounds 3] [--muls 8,4,2,1] [--out DIR]

The arms alternate for `rounds` rounds, each in a process of its own: the base library (built from the parent commit by
tools/ab_lib.py or rag_dpo_amd.build.build_lib(out=...); option defaults), the product library with i8_sample_mul set to every value
of --muls and, with --pilot0, the base library with refine_pilot = 0. Every arm runs
    bench.py --steps 50 --warmup 10 --no-cpu --no-others --profile-all [--corpus-shape embed]
with RDX_DEBUG_HITS = 1 (the library's developer line: the longest hit list of a search and how many queries took the spill list).
Round 0 also writes --dump-outputs of every arm, and the tool compares them byte for byte with the base's. One line per run, then
per arm the mean queries/s and its spread (max - min over mean). A run that fails ends the tool."""
import argparse
import filecmp
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(lib, shape, sets, dump, steps, warmup, workload=None):
    """workload: another workload of bench.py than c4, with the timer bench.py uses by itself (events around every kernel would
    sit on the host path that is most of a small workload's step)"""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", str(steps), "--warmup", str(warmup), "--no-cpu", "--no-others"]
    cmd += ["--workload", workload] if workload else ["--profile-all"]
    if shape != "iid":
        cmd += ["--corpus-shape", shape]
    for s in sets:
        cmd += ["--set", s]
    if dump:
        cmd += ["--dump-outputs", dump]
    env = dict(os.environ, RDX_DEBUG_HITS="1")
    if lib:
        env["RDX_LIB_PATH"] = os.path.abspath(lib)
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=600)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-3000:])
        raise SystemExit(f"bench.py failed with {r.returncode}: {' '.join(cmd)}")
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    hits = re.findall(r"hits max (\d+) spilled (\d+)", r.stderr)
    d = json.loads(line)
    ps = d["path_stats"]
    return {"qps": d["value"], "ms_step": d["ms_per_step"], "ms_sample": ps["ms"]["ms_scan_sample"], "ms_main": ps["ms"]["ms_scan_main"],
            "ms_refine": ps["ms"]["ms_refine"], "emitted": ps["emitted_per_query"], "rescored": ps["rescored_per_query"],
            "retried": ps["retried_queries"], "exact": ps["exact_fallback_queries"], "sample_rows": ps["sample_rows"],
            "max_hits": max((int(a) for a, _ in hits), default=-1), "max_spilled": max((int(b) for _, b in hits), default=-1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", required=True)
    ap.add_argument("--shape", default="iid", choices=["iid", "embed"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--muls", default="8,4,2,1")
    ap.add_argument("--pilot0", action="store_true", help="one more arm: the base library with refine_pilot = 0 (round 0 only)")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "ab_i8_sample"), help="where the dumped outputs go (build/ is git-ignored)")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    arms = [("base", a.base, [])] + [(f"mul{m}", None, [f"i8_sample_mul={m}"]) for m in a.muls.split(",") if m]
    os.makedirs(a.out, exist_ok=True)
    got = {name: [] for name, _, _ in arms}
    for rnd in range(a.rounds):
        todo = arms + ([("base_pilot0", a.base, ["refine_pilot=0"])] if a.pilot0 and rnd == 0 else [])
        for name, lib, sets in todo:
            dump = os.path.join(a.out, f"dump_{a.shape}_{name}") if rnd == 0 else None
            res = run(lib, a.shape, sets, dump, a.steps, a.warmup)
            got.setdefault(name, []).append(res)
            print(a.shape, rnd, name, json.dumps(res), flush=True)
    for name, rs in got.items():
        q = [r["qps"] for r in rs]
        mean = sum(q) / len(q)
        print(f"{a.shape} {name}: queries/s mean {mean:.1f} spread {(max(q) - min(q)) / mean * 100:.2f} % of {len(q)} run(s)", flush=True)
    for name in got:
        if name != "base":
            same = all(filecmp.cmp(os.path.join(a.out, f"dump_{a.shape}_base", f), os.path.join(a.out, f"dump_{a.shape}_{name}", f), shallow=False)
                       for f in ("scores.npy", "rows.npy", "counts.npy"))
            print(f"{a.shape} {name}: dumped outputs byte-identical to base: {same}", flush=True)


if __name__ == "__main__":
    main()
