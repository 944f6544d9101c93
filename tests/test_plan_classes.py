"""SearchPlan::eps_classes and option i8_eps_classes (rag_dpo_amd/csrc/search_plan.hpp, DESIGN.md §5 "classes of eps_b") on the CPU:
tests/c_abi/plan_classes.cpp, a stand-alone program built by g++ under ASan and UBSan with the flags tests/test_search_plan.py uses.
It checks that a plan has 8 classes exactly where coarse_i8 = 2 chose the int8 pass at depth 0, one class on forced int8, depth 1,
fp16, small and exact plans, that the option takes 0 / 1 / 2 / 4 / 8 and refuses 3, 16 and -1, and that nothing else of a plan moves."""
import os
import subprocess

from test_sanitizers import ENV, ROOT, SAN


def test_eps_classes_rule_and_option(tmp_path):
    exe = str(tmp_path / "plan_classes")
    subprocess.check_call(["g++", "-std=c++17", *SAN, "-ffp-contract=off", "-Wall", "-Wextra",
                           os.path.join(ROOT, "tests", "c_abi", "plan_classes.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=ENV)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.splitlines()[-1] == "plan classes ok", r.stdout[-2000:]
