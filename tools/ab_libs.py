"""A/B of whole libraries on the contract bench, a sibling of ab_i8_sample.py (whose run() it uses: same command, same record):

    python tools/ab_libs.py --arm parent=tools/librdx_parent.so --arm part1=tools/librdx_p1.so --arm new= --arm new_mul1=:i8_sample_mul=1 \\
                            [--shape iid|embed] [--workload c1|c2|...] [--rounds 3] [--out DIR]

An arm is NAME=LIBRARY[:OPTION=VALUE,...]; an empty LIBRARY is the product library. The FIRST arm is the base. The arms alternate for
`rounds` rounds, each run a process of its own; round 0 also writes --dump-outputs of every arm, compared byte for byte with the
base's. One line per run, then per arm the mean queries/s, its spread (max - min over mean) and its gain on the base, and the
mean, lowest and highest ms per step. --workload is passed through to bench.py, which then runs that workload's own number of
steps unless --steps / --warmup say otherwise."""
import argparse
import filecmp
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ab_i8_sample import ROOT, run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", action="append", required=True)
    ap.add_argument("--shape", default="iid", choices=["iid", "embed"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "ab_libs"), help="where the dumped outputs go (build/ is git-ignored)")
    ap.add_argument("--workload", default=None, help="bench.py --workload (default: bench.py's own, c4)")
    ap.add_argument("--steps", type=int, default=None, help="default: 50, with --workload the workload's own")
    ap.add_argument("--warmup", type=int, default=None, help="default: 10, with --workload the workload's own")
    a = ap.parse_args()
    steps = a.steps if a.steps is not None else (0 if a.workload else 50)
    warmup = a.warmup if a.warmup is not None else (-1 if a.workload else 10)
    tag = a.workload or a.shape
    arms = []
    for spec in a.arm:
        name, _, rest = spec.partition("=")
        lib, _, sets = rest.partition(":")
        arms.append((name, lib or None, [s for s in sets.split(",") if s]))
    os.makedirs(a.out, exist_ok=True)
    got = {name: [] for name, _, _ in arms}
    for rnd in range(a.rounds):
        for name, lib, sets in arms:
            dump = os.path.join(a.out, f"dump_{tag}_{name}") if rnd == 0 else None
            res = run(lib, a.shape, sets, dump, steps, warmup, a.workload)
            got[name].append(res)
            print(tag, rnd, name, json.dumps(res), flush=True)
    base = arms[0][0]
    mean = {n: sum(r["qps"] for r in rs) / len(rs) for n, rs in got.items()}
    for name, rs in got.items():
        q = [r["qps"] for r in rs]
        ms = [r["ms_step"] for r in rs]
        print(f"{tag} {name}: queries/s mean {mean[name]:.1f} spread {(max(q) - min(q)) / mean[name] * 100:.2f} % of {len(q)} run(s), "
              f"{(mean[name] / mean[base] - 1) * 100:+.2f} % on {base}; ms_per_step mean {sum(ms) / len(ms):.4f} min {min(ms):.4f} max {max(ms):.4f}",
              flush=True)
    for name in got:
        if name != base:
            same = all(filecmp.cmp(os.path.join(a.out, f"dump_{tag}_{base}", f), os.path.join(a.out, f"dump_{tag}_{name}", f), shallow=False)
                       for f in ("scores.npy", "rows.npy", "counts.npy"))
            print(f"{tag} {name}: dumped outputs byte-identical to {base}: {same}", flush=True)


if __name__ == "__main__":
    main()
