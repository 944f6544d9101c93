"""Builds librdx.so (HIP, gfx950) in-tree. hipcc cross-compiles without a GPU.

The scan kernel issues its corpus loads as inline asm with hand-counted waits (scan_kernel.hpp): a register such a load
is still in flight to must never be spilled or copied by the compiler, which it would do silently under register
pressure (seen once: 2 % wrong ids in one variant, caught by the parity tests). The build therefore reads the
compiler's own resource remarks and REFUSES a library whose scan kernels spill; the figures are kept next to the
library (librdx.resources.json) and checked again by tests/test_abi.py.

"No spills" is one way of breaking that property, not the property. Since round 3 the build also reads the ISA it is about to
ship (-save-temps: the very listing that is assembled into the library) and refuses a library in which, on any path through a
k_scan kernel, (A) anything but the source's own MFMA reads and asm loads touches the destination registers of an asm load
that may still be in flight, (B) a fragment is used before its load can have retired on any path, or (C) an inline-asm memory
instruction reads an SGPR fewer than 5 wait states after a VALU instruction wrote it (the hazard the compiler cannot see
through inline asm; it is what made the first RDX_CHECK_BOUNDS build fault) — rag_dpo_amd/isa_check.py."""
from __future__ import annotations

import glob
import json
import os
import re
import shutil
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor
from typing import NamedTuple

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "librdx.so")
RESOURCES = os.path.join(HERE, "librdx.resources.json")
# one translation unit per subsystem (the dense index: its core, what is derived from it, the merge), each compiled as a job of its own;
# whatever lies in csrc/ is a source and is hashed. No kernel is defined in two units (csrc/rdx_index.hpp "ONE DEFINITION")
SOURCES = sorted(os.path.basename(f) for f in glob.glob(os.path.join(CSRC, "*.hip")))
HEADERS = sorted(os.path.basename(f) for f in glob.glob(os.path.join(CSRC, "*.hpp"))) + ["../../include/rdx.h"]
CORE = "rdx_index.hip"        # the dense index's core (lifecycle, writes, the search pipeline, the threshold search, the grouped fill): the only
                              # unit that may hold a k_scan kernel; rdx_derived.hip and rdx_merge.hip are built on it and beside it
CHECKERS = ["isa_check.py"]   # part of the recorded hash: a library is only "fresh" if it passed THIS version of the ISA check


def _hipcc() -> str:
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: librdx needs the ROCm toolchain (/opt/rocm/bin/hipcc)")


def source_hash() -> str:
    import hashlib
    h = hashlib.sha256()
    for f in SOURCES + HEADERS:
        h.update(f.encode())
        with open(os.path.join(CSRC, f), "rb") as fh:
            h.update(fh.read())
    for f in CHECKERS:
        with open(os.path.join(HERE, f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()


def is_fresh() -> bool:
    """the library was built from exactly the sources in the tree (content hash recorded next to it; mtimes alone
    would accept a variant library copied over the product file)"""
    if not os.path.exists(LIB) or not os.path.exists(RESOURCES):
        return False
    try:
        with open(RESOURCES) as f:
            rec = json.load(f).get("_build", {})
    except (OSError, ValueError):
        return False
    return rec.get("source_sha256") == source_hash() and rec.get("lib_size") == os.path.getsize(LIB)


def parse_resources(remarks: str) -> dict:
    """{kernel symbol: {"vgprs", "agprs", "spill_vgprs", "spill_sgprs", "scratch_bytes", "lds_bytes"}} from
    -Rpass-analysis=kernel-resource-usage output"""
    out, cur = {}, None
    keys = {"VGPRs": "vgprs", "AGPRs": "agprs", "VGPRs Spill": "spill_vgprs", "SGPRs Spill": "spill_sgprs",
            "ScratchSize [bytes/lane]": "scratch_bytes", "LDS Size [bytes/block]": "lds_bytes"}
    for line in remarks.splitlines():
        if "remark" not in line:
            continue
        # two layouts: "<file>:<line>:<col>: remark: Function Name: X" and, with -save-temps, "remark: <file>:<line>:<col>: Function Name: X"
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r":\s+([A-Za-z][A-Za-z \[\]/]*): (\d+)(?: \[-Rpass|$)", line)
        if m and cur is not None and m.group(1).strip() in keys:
            cur[keys[m.group(1).strip()]] = int(m.group(2))
    return out


def _listing(unit_dir: str) -> str:
    """the device listing -save-temps=obj left beside a unit's object file: the very text that was assembled into it"""
    lst = glob.glob(os.path.join(unit_dir, "*gfx950*.s"))
    if len(lst) != 1:
        raise RuntimeError(f"expected one gfx950 listing from -save-temps in {unit_dir}, found {lst}")
    with open(lst[0]) as f:
        return f.read()


def check_isa(work: str) -> dict:
    """run rag_dpo_amd/isa_check.py over the core unit's device listing (each unit was compiled in work/<unit>); raises on any
    hazard, and on a k_scan kernel in any other unit, where nothing would check it"""
    from . import isa_check
    for s in SOURCES:
        if s != CORE and re.search(r"^\S*k_scan\S*:", _listing(os.path.join(work, s)), re.M):
            raise RuntimeError(f"{s} holds a k_scan kernel — refused: the ISA check reads {CORE} only")
    found = isa_check.check_listing(_listing(os.path.join(work, CORE)))
    if len(found) < 16:
        raise RuntimeError(f"ISA check: only {len(found)} k_scan kernels in the listing — the parser no longer matches the compiler's output")
    bad = {k: hz for k, (hz, st) in found.items() if hz}
    if bad:
        lines = []
        for k, hz in bad.items():
            lines.append(f"  {k}: {len(hz)} hazard(s)")
            lines += [f"    [{h['kind']}] line {h['line']}: {h['text']}  <->  line {h['load_line']}: {h['load_text']}" for h in hz[:6]]
        raise RuntimeError("scan kernels fail the ISA check — refused (rag_dpo_amd/isa_check.py):\n" + "\n".join(lines))
    return {"kernels": len(found), "asm_loads": sum(st["asm_loads"] for _, st in found.values()),
            "asm_vmem": sum(st["asm_vmem"] for _, st in found.values()), "hazards": 0,
            "checks": ["A: no foreign instruction touches an in-flight fragment", "B: no fragment used before its load can have retired",
                       "C: 5 wait states between a VALU SGPR write and an asm VMEM read of it"]}


class SpillCheck(NamedTuple):
    """one condition under which build_lib refuses a library, read from the compiler's resource remarks"""
    fragments: tuple      # a kernel belongs to the check when its symbol holds one of these
    least: int            # kernels there must be (0: however many there are)
    remarks: str          # kernels whose remarks lack the spill or scratch figure: "counted" out of `least`, "required" (one refuses), "ignored"
    spill: bool           # refuse a kernel that spills or uses scratch
    variant: bool         # checked in a variant build (extra_flags) too: a variant may spill where that only costs speed, it is nobody's product
    message: str          # {n}: kernels found; behind a spill check the kernels follow (the offenders alone when least is 0)


SPILL_CHECKS = (
    SpillCheck(("k_scan",), 16, "counted", False, True,
               "the compiler's resource remarks could not be read for the scan kernels — refused (the spill check would be blind)"),
    SpillCheck(("k_scan",), 0, "ignored", True, True,
               "scan kernels spill registers — refused (inline-asm loads may be in flight to a spilled register):"),
    SpillCheck(("k_docs",), 4, "ignored", True, True, "the where_document kernels (doc_kernel.hpp) spill or were not found — refused:"),
    SpillCheck(("k_meta",), 2, "required", True, True, "the `where` predicate kernels (meta_kernel.hpp) spill or were not found — refused:"),
    SpillCheck(("k_topic",), 2, "required", True, True, "the topic boost kernels (topic_kernel.hpp) spill or were not found — refused:"),
    SpillCheck(("k_rerank_select_batch", "k_topic_sims_batch", "k_topic_replay_batch"), 5, "required", True, True,
               "the batched reranker kernels (rerank_batch_kernel.hpp) spill or were not found — refused:"),
    SpillCheck(("k_space",), 5, "required", True, True, "the ip / l2 space kernels (space_kernel.hpp) spill or were not found — refused:"),
    SpillCheck(("k_fuse",), 1, "required", True, True, "the rank fusion kernel (fuse_kernel.hpp) spills or was not found — refused:"),
    SpillCheck(("k_group",), 0, "ignored", True, True, "the grouped search's kernels (group_kernel.hpp, group_fill_kernel.hpp) spill — refused:"),
    SpillCheck(("k_mmr",), 0, "ignored", True, True, "the diversity-aware selection kernel (mmr_kernel.hpp) spills — refused:"),
    SpillCheck(("k_range",), 0, "ignored", True, True, "the threshold search's kernels (range_kernel.hpp) spill — refused:"),
    SpillCheck(("k_dup",), 0, "ignored", True, True, "the near-duplicate clustering kernels (dup_kernel.hpp) spill — refused:"),
    SpillCheck(("k_km_",), 0, "ignored", True, True, "the k-means kernels (kmeans_kernel.hpp) spill — refused:"),
    SpillCheck(("k_facet",), 0, "ignored", True, True, "the value counts' kernels (facet_kernel.hpp) spill — refused:"),
    SpillCheck(("k_maxsim",), 0, "ignored", True, True, "the late-interaction scoring kernel (maxsim_kernel.hpp) spills — refused:"),
    SpillCheck(("k_lex",), 0, "ignored", True, True, "the lexical-weight kernels (lex_kernel.hpp k_lex_reduce, bm25_kernel.hpp k_lex_score, lex_pairs_kernel.hpp k_lex_score_pairs) spill — refused:"),
    SpillCheck(("k_score_pairs", "k_m3_combine"), 0, "ignored", True, True, "the combined score's kernels (m3_kernel.hpp) spill — refused:"),
    # k_refine<false> / k_refine<true> (the plans that spill to the HBM list) run 1024 threads at the 128-register limit (refine_kernel.hpp): a spill would be paid on every search
    SpillCheck(("k_refine",), 2, "required", True, False, "the refine kernels (refine_kernel.hpp) spill or were not found — refused:"),
    # kernels that are given an occupancy target (amdgpu_waves_per_eu: the latency-bound attention kernel E12) pay for a miss
    # silently, in scratch traffic
    SpillCheck(("k_enc_attention_mfma",), 0, "ignored", True, False,
               "k_enc_attention_mfma no longer fits its occupancy target without spilling — refused:"),
    # the batch GEMM (E14, enc_gemm.hpp) is sized for two or three workgroups per CU; scratch traffic in its k-loop would cost that silently
    SpillCheck(("k_enc_gemm",), 6, "required", False, True,
               "the compiler's resource remarks could not be read for the k_enc_gemm kernels ({n} found) — refused"),
    SpillCheck(("k_enc_gemm",), 0, "ignored", True, False, "k_enc_gemm kernels spill or use scratch — refused:"),
)


def refusals(res: dict, variant: bool = False) -> list:
    """the messages of the SPILL_CHECKS that the resource record `res` (parse_resources) fails, in the table's order; a variant
    build is asked only the checks marked for it. build_lib raises on the first."""
    out = []
    for c in SPILL_CHECKS:
        if variant and not c.variant:
            continue
        found = {k: v for k, v in res.items() if any(f in k for f in c.fragments)}
        readable = [k for k, v in found.items() if "spill_vgprs" in v and "scratch_bytes" in v]
        spilling = {k: v for k, v in found.items() if v.get("spill_vgprs", 0) or v.get("scratch_bytes", 0)}
        if (len(readable) if c.remarks == "counted" else len(found)) < c.least or (c.remarks == "required" and len(readable) < len(found)) \
                or (c.spill and spilling):
            listed = found if c.least else spilling
            out.append(c.message.format(n=len(found)) + ("\n" + "\n".join(f"  {k}: {v}" for k, v in listed.items()) if c.spill else ""))
    return out


def build_lib(force: bool = False, verbose: bool = False, extra_flags=(), out: str = None) -> str:
    """out: build a VARIANT (extra_flags) to this path; the product library and its resource record are left alone"""
    if out is None and not force and is_fresh() and not extra_flags:
        return LIB
    # compiled in a scratch directory, one sub-directory and one job per unit, with -save-temps=obj: a unit's device listing
    # (…gfx950.s) lands beside its object file and is the very text that gets assembled into the library
    work = tempfile.mkdtemp(prefix="librdx_build_", dir=os.environ.get("TMPDIR") or None)
    try:
        tmp = os.path.join(work, "librdx.so")
        flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-save-temps=obj", "-Wall", "-Wno-unused-function",
                 "-Rpass-analysis=kernel-resource-usage", *extra_flags]

        def compile_unit(s):
            os.mkdir(os.path.join(work, s))
            cmd = [_hipcc(), *flags, "-c", os.path.join(CSRC, s), "-o", os.path.join(work, s, "unit.o")]
            if verbose:
                print(" ".join(cmd))
            return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=os.path.join(work, s))

        with ThreadPoolExecutor(max_workers=min(16, len(SOURCES))) as pool:
            jobs = list(pool.map(compile_unit, SOURCES))
        remarks = "\n".join(j.stderr for j in jobs)
        noise = ("-Rpass-analysis=kernel-resource-usage", "remark:")
        diag = "\n".join(l for l in remarks.splitlines() if not any(n in l for n in noise))
        if any(j.returncode != 0 for j in jobs):
            raise RuntimeError(f"hipcc failed ({[j.returncode for j in jobs]}):\n{diag[-4000:]}")
        cmd = [_hipcc(), "-shared", "-fPIC", *[os.path.join(work, s, "unit.o") for s in SOURCES], "-o", tmp]
        if verbose:
            print(" ".join(cmd))
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=work)
        if r.returncode != 0:
            raise RuntimeError(f"linking librdx failed ({r.returncode}):\n{r.stderr[-4000:]}")
        res = parse_resources(remarks)
        refused = refusals(res, variant=bool(extra_flags))
        if refused:
            raise RuntimeError(refused[0])
        isa = check_isa(work)
        final_tmp = (out or LIB) + ".tmp"
        shutil.move(tmp, final_tmp)
        tmp = final_tmp
    finally:
        shutil.rmtree(work, ignore_errors=True)
    if out is not None:
        os.replace(tmp, out)
        return out
    os.replace(tmp, LIB)
    res["_build"] = {"source_sha256": source_hash(), "lib_size": os.path.getsize(LIB), "flags": list(extra_flags)}
    res["_isa_check"] = isa
    with open(RESOURCES, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    if verbose and diag.strip():
        print(diag)
    return LIB


if __name__ == "__main__":
    print(build_lib(force=True, verbose=True))
