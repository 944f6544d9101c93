"""The two rules of the dense index's state (rag_dpo_amd/csrc/index_state.hpp) on the CPU: tests/c_abi/index_state_dump.cpp, built by
g++ under ASan and UBSan as a stand-alone program, against

  * tests/i8_model.py::Copy8, the model of what prepare_i8 keeps between searches, on scripted writes and searches at the edges of
    the 32-row blocks: the watermark before every search, the first block to quantise, how many, and whether it is a full rebuild;
  * a restatement of the capacity policy of grow() and rdx_index_compact().
"""
import os
import subprocess

import numpy as np
import pytest

import i8_model as M
from test_sanitizers import ENV, ROOT, SAN

EDGES = (0, 1, 31, 32, 33, 64, 77, 255, 256, 257)


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("index_state") / "index_state_dump")
    subprocess.check_call(["g++", "-std=c++17", *SAN, "-Wall", "-Wextra", os.path.join(ROOT, "tests", "c_abi", "index_state_dump.cpp"), "-o", exe])

    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300, env=ENV)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
        out = r.stdout.splitlines()
        assert len(out) == len(lines)
        return out
    return run


# ---- the watermark ---------------------------------------------------------------------------------------------------------------
# a script: ("add", rows after it) | ("update",) | ("compact", rows kept) | ("realloc",) | ("search",)
def _scripts():
    out = {}
    for n in EDGES:
        # "nothing written: nothing to do": the second and third search
        out[f"fresh {n}"] = [("add", n), ("search",), ("search",), ("search",)]
    for i, n0 in enumerate(EDGES):
        for n1 in EDGES[i + 1:]:
            # (n0 % 32 != 0: the append starts inside a partial block)
            out[f"append {n0} {n1}"] = [("add", n0), ("search",), ("add", n1), ("search",), ("search",)]
            out[f"append unsearched {n0} {n1}"] = [("add", n0), ("add", n1), ("search",)]
            out[f"update after append {n0} {n1}"] = [("add", n0), ("search",), ("add", n1), ("update",), ("search",), ("search",)]
            out[f"append after update {n0} {n1}"] = [("add", n0), ("search",), ("update",), ("search",), ("add", n1), ("search",)]
            out[f"compact {n1} {n0}"] = [("add", n1), ("search",), ("compact", n0), ("search",), ("search",), ("add", n1), ("search",)]
            out[f"realloc at the search {n0} {n1}"] = [("add", n0), ("search",), ("add", n1), ("realloc",), ("search",)]
            for n2 in EDGES[EDGES.index(n1) + 1:]:
                out[f"realloc between appends {n0} {n1} {n2}"] = [("add", n0), ("search",), ("add", n1), ("realloc",), ("add", n2), ("search",),
                                                                 ("search",)]
    return out


def _model(script):
    """what Copy8 says of every search of the script: (valid before it, first block, blocks, full rebuild)"""
    c, rows, said = M.Copy8(), 0, []
    for op in script:
        if op[0] == "add":
            if op[1] > rows:                                  # (an append of no rows never reaches ingest)
                c.appended(rows)
                rows = op[1]
        elif op[0] in ("update", "compact", "realloc"):       # (Copy8: "a reallocation would be a full rebuild")
            c.rewritten()
            rows = op[1] if op[0] == "compact" else rows
        else:
            before = c.valid
            c.prepare(np.zeros((rows, 1), M.F32))
            if before < rows:
                assert c.valid == rows and len(c.s) == (rows + 31) // 32
                said.append((before, before // 32, len(c.s) - before // 32, int(before == 0)))
            else:
                assert c.valid == before
                said.append((before, 0, 0, 0))
    return said


def _events(script):
    rows, ev = 0, []
    for op in script:
        if op[0] == "add":
            if op[1] > rows:
                ev.append(f"a{rows}")
                rows = op[1]
        elif op[0] == "compact":
            ev.append("c")
            rows = op[1]
        else:
            ev.append({"update": "u", "realloc": "r", "search": f"p{rows}"}[op[0]])
    return "w " + " ".join(ev)


def test_watermark_agrees_with_copy8(dump):
    scripts = _scripts()
    got = dump([_events(s) for s in scripts.values()])
    seen = set()
    for (name, script), line in zip(scripts.items(), got):
        said = [tuple(map(int, part.split())) for part in line.split(" | ")]
        assert said == _model(script), (name, line)
        seen.update((nb > 0, bool(full), b0 > 0) for _, b0, nb, full in said)
    # (work?, full rebuild?, from a later block?): nothing to do, a full rebuild, an append from a later block
    assert seen >= {(False, False, False), (True, True, False), (True, False, True)}


def test_watermark_cases_by_hand(dump):
    got = dump(["w p0", "w a0 p33 a33 p77 p77", "w a0 p64 a64 p77 u p77", "w a0 p257 c p77", "w a0 p33 a33 r a64 p77"])
    assert got == ["0 0 0 0",
                   "0 0 2 1 | 32 1 2 0 | 77 0 0 0",      # the append re-opens block 1, which held one row
                   "0 0 2 1 | 64 2 1 0 | 0 0 3 1",       # a full block stays; the update rebuilds everything
                   "0 0 9 1 | 0 0 3 1",
                   "0 0 2 1 | 0 0 3 1"]


# ---- the capacity policy -----------------------------------------------------------------------------------------------------------
def _round256(n):
    return (n + 255) // 256 * 256


def _grow_caps(cap, need):
    if need <= cap:
        return cap, cap
    return _round256(max(need, cap + cap // 2)), _round256(need)


def _compact_cap(n):
    return max(256, _round256(n))


def test_capacity_policy(dump):
    caps = sorted({256 * c for c in (0, 1, 2, 3, 4, 5, 8, 100, 4097)})
    grow = [(c, n) for c in caps for n in sorted({0, 1, 255, 256, 257, c - 1, c, c + 1, c + c // 2, c + c // 2 + 1, 2 * c + 300}) if n >= 0]
    keep = [0, 1, 255, 256, 257, 512, 513, 1000003]
    got = dump([f"g {c} {n}" for c, n in grow] + [f"k {n}" for n in keep])
    for (c, n), line in zip(grow, got):
        roomy, tight = map(int, line.split())
        assert (roomy, tight) == _grow_caps(c, n), (c, n, line)
        if n > c:
            assert roomy % 256 == 0 and roomy >= tight >= n > tight - 256 and roomy > c, (c, n, line)
    assert [int(l) for l in got[len(grow):]] == [_compact_cap(n) for n in keep]
    by_hand = dump(["g 512 300", "g 512 512", "g 0 1", "g 256 257", "g 1024 1025", "k 0", "k 257"])
    assert by_hand == ["512 512", "512 512",      # need <= cap: no growth
                       "256 256",
                       "512 512",                  # roomy equals tight: no retry
                       "1536 1280",
                       "256", "512"]
