"""The search plan and the option table (rag_dpo_amd/csrc/search_plan.hpp) on the CPU: tests/c_abi/plan_dump.cpp, built by g++ under
ASan and UBSan as a stand-alone program, against

  * the record tests/golden/search_plans.txt (the plans and option results of the commit named in its first line), line for line.
    A change to the heuristics re-records it (tests/golden/make_search_plans.py); the file's diff is then the list of plans that moved;
  * the rules for the fields the plan took over from the handle: fused, fuse_finish, pilot, retry, i8_auto;
  * test_gpu_coarse_bound._plan, the restatement the GPU tests place their anchors by.
"""
import os
import subprocess
import sys

import pytest

import test_gpu_coarse_bound as CB
from test_sanitizers import ENV, ROOT, SAN

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_search_plans as MK  # noqa: E402

N_CU = 256
# what _plan is compared on: 6 x 4 x 9 x 2 x 9 = 3 888 cases, all with force_fast = 1, sample_div = 1, spec_tau = 0 (_plan's premises)
GRID_ROWS = (2048, 16919, 32769, 65536, 262144, 1000003)
GRID_DIM = (128, 1000, 1024, 4096)
GRID_B = (1, 4, 64, 65, 128, 129, 256, 300, 1100)
GRID_K = (1, 10)
GRID_OPTS = ({}, {"split_boot": 0}, {"small_scan": 0}, {"split_boot": 0, "small_scan": 0}, {"half_boot": 0}, {"spread_boot": 0},
             {"force_bn": 64}, {"force_bn": 128}, {"force_bn": 256})


@pytest.fixture(scope="module")
def plan_dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan_dump") / "plan_dump")
    subprocess.check_call(["g++", "-std=c++17", *SAN, "-ffp-contract=off", "-Wall", "-Wextra",
                           os.path.join(ROOT, "tests", "c_abi", "plan_dump.cpp"), "-o", exe])
    return exe


def _dump(exe, cases):
    r = subprocess.run([exe], input="\n".join(cases) + "\n", capture_output=True, text=True, timeout=300, env=ENV)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases)
    return lines


@pytest.fixture(scope="module")
def recorded_run(plan_dump):
    return _dump(plan_dump, MK.cases())


def _grid():
    return [(r, d, b, k, o) for r in GRID_ROWS for d in GRID_DIM for b in GRID_B for k in GRID_K for o in GRID_OPTS]


@pytest.fixture(scope="module")
def grid_run(plan_dump):
    fixed = {"force_fast": 1, "sample_div": 1, "spec_tau": 0}
    return _dump(plan_dump, [f"p r={r} q={b} k={k} d={CB.M.dim_pad(d)} c={N_CU}" + "".join(f" {n}={v}" for n, v in {**fixed, **o}.items())
                             for r, d, b, k, o in _grid()])


def test_record(recorded_run):
    with open(MK.RECORD) as f:
        want = [l for l in f.read().splitlines() if not l.startswith("#")]
    got = [MK.recorded(l) for l in recorded_run]
    assert len(want) == len(got) and os.path.getsize(MK.RECORD) <= 160 * 1000
    moved = [f"recorded: {w}\n     now: {g}" for w, g in zip(want, got) if w != g]
    assert not moved, f"{len(moved)} of {len(want)} lines differ from the record, the first:\n" + "\n".join(moved[:5])


def test_fields_taken_over_from_the_handle(recorded_run, grid_run):
    n = 0
    for line in recorded_run + grid_run:
        if " || " not in line:   # an option probe or a plan that failed
            continue
        fused, fuse_finish, pilot, retry, i8_auto, i8, ksteps, o_fuse_epilogue, o_fuse_finish, o_pilot, o_retry = map(int, line.split(" || ")[1].split())
        assert fused == int(ksteps % 2 == 0 and o_fuse_epilogue != 0), line
        assert (fuse_finish, pilot, retry) == (o_fuse_finish, o_pilot, o_retry), line
        assert not i8_auto or i8, line
        n += 1
    assert n > 3888 + 600
    # every value of the four options was seen, and both parities of ksteps (dim_pad 448: 7 k-steps)
    seen = {tuple(map(int, l.split(" || ")[1].split()))[6:] for l in recorded_run if " || " in l}
    assert {s[1] for s in seen} == {0, 1} and {s[2] for s in seen} == {0, 1} and {s[3] for s in seen} >= {0, 4, 64} and {s[4] for s in seen} == {0, 1}
    assert {s[0] % 2 for s in seen} == {0, 1}


def test_plan_restated_in_test_gpu_coarse_bound(grid_run):
    short = 0
    for (r, d, b, k, o), line in zip(_grid(), grid_run):
        groups = line.split(" => ")[1].split(" || ")[0].split("|")
        assert groups[0] == "0" and groups[1].split()[5] == "0", line   # planned, and on the MFMA path
        use_boot = int(groups[3].split()[0])
        use_small, _, sample_rows = map(int, groups[4].split()[:3])
        rb, rs, sampled = CB._plan(r, d, b, k, o, N_CU)
        assert (rb, rs) == (bool(use_boot), bool(use_small)), line
        assert 0 <= sample_rows - 32 * len(sampled) < 256, (line, len(sampled))   # (short of it: the corpus' partial last tile)
        short += sample_rows != 32 * len(sampled)
    assert 0 < short < len(grid_run) // 4
