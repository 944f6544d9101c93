"""Compare two gfx950 device listings kernel by kernel: did a source change alter the code of any kernel both builds share?

Make a listing and its resource remarks for every translation unit U of rag_dpo_amd/csrc/*.hip with
    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S rag_dpo_amd/csrc/U.hip -o U.s \\
          -Rpass-analysis=kernel-resource-usage 2> U.remarks
concatenate the units' listings into X.s and their remarks into X.remarks (no kernel is in two units), then run  python tools/compare_listings.py OLD.s OLD.remarks NEW.s NEW.remarks

Kernels are matched by symbol. A k_scan instantiation of the OLD listing that the NEW one does not have, with the seven template
arguments <BN, EPI, MASK, RES, SIBT, NTT, FUSED> of the scan before the sibling lock-step was removed, is matched through
SIBT = false to the six-argument symbol; SIBT = true instantiations have no counterpart and are listed as removed. k_refine,
k_select_dense, k_exact_scores and k_exact_scores_reg with their loose arguments are matched to the symbols that take
RefineParams / SelectParams / ExactParams. A k_scan with seven template arguments and a k_exact_scores_reg<U> are matched to the
symbols with the trailing argument PERQ = false (a filter per query), k_exact_scores, k_boot and k_scan_small to their
<false> instantiations.

For every matched pair it compares
  * the compiler's resource remarks (SGPRs, VGPRs, AGPRs, scratch, occupancy, LDS, spills) and the .amdhsa_* descriptor
    fields apart from .amdhsa_kernarg_size;
  * the sequence of instruction mnemonics;
  * the instruction text with label numbers normalised, and once more with the immediate offsets of scalar loads
    (kernel-argument loads) masked out.
Exit status 0 when resources, descriptors and mnemonic sequences all match and the text differs at most in masked offsets."""
import re
import sys

_SCAN7 = re.compile(r"^(_ZN3rdx6k_scanI(?:Li\d+E){2})((?:Lb[01]E){5})(EEvNS_10ScanParamsE)$")
# the scan before it had a filter per query: seven template arguments; the eighth, PERQ, is false for every kernel that existed then
_SCAN_NO_PERQ = re.compile(r"^(_ZN3rdx6k_scanI(?:Li\d+E){2}(?:Lb[01]E){5})(EEvNS_10ScanParamsE)$")
_EXACT_REG_NO_PERQ = re.compile(r"^(_ZN3rdx18k_exact_scores_regILi\dE)(EEvNS_11ExactParamsE)$")
# ... and k_exact_scores, k_boot and k_scan_small, plain kernels then, are the <false> instantiations of templates on PERQ
_PLAIN_NO_PERQ = re.compile(r"^(_ZN3rdx(?:14k_exact_scores|6k_boot|12k_scan_small))E(NS_\d+\w+ParamsE)$")
_REMARK_KEYS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill",
                "VGPRs Spill", "LDS Size [bytes/block]")


# kernels whose loose arguments became one parameter struct (k_refine and k_select_dense keep FinishArgs as their second argument)
_STRUCT_ARGS = (
    (re.compile(r"^(_ZN3rdx8k_refineILb[01]EEEv)PK15HIP_vector_typeIjLj2EE\S*(NS_10FinishArgsE)$"), r"\1NS_12RefineParamsE\2"),
    (re.compile(r"^(_ZN3rdx14k_select_denseE)PKfl\S*(NS_10FinishArgsE)$"), r"\1NS_12SelectParamsE\2"),
    (re.compile(r"^(_ZN3rdx14k_exact_scoresE)NS_10MasterViewEli\S*$"), r"\1NS_11ExactParamsE"),
    (re.compile(r"^(_ZN3rdx18k_exact_scores_regILi\dEEEv)NS_10MasterViewEli\S*$"), r"\1NS_11ExactParamsE"),
)


def new_name(sym: str):
    """the symbol a kernel of the OLD listing has in the NEW one, or None if it was removed"""
    for pat, repl in _STRUCT_ARGS:
        if pat.match(sym):
            return pat.sub(repl, sym)
    if _PLAIN_NO_PERQ.match(sym):
        return _PLAIN_NO_PERQ.sub(r"\1ILb0EEEv\2", sym)
    for pat in (_SCAN_NO_PERQ, _EXACT_REG_NO_PERQ):
        if pat.match(sym):
            return pat.sub(r"\1Lb0E\2", sym)
    m = _SCAN7.match(sym)
    if not m:
        return sym
    flags = re.findall(r"Lb([01])E", m.group(2))
    if flags[2] == "1":   # SIBT
        return None
    return m.group(1) + "".join(f"Lb{f}E" for i, f in enumerate(flags) if i != 2) + m.group(3)


def parse_listing(text: str) -> dict:
    """{kernel: {"insts": [text], "desc": {field: value}, "code_len": int}}"""
    out, cur, lines = {}, None, text.splitlines()
    for i, line in enumerate(lines):
        m = re.match(r"^(\S+):\s+; @(\S+)$", line)
        if m and m.group(1) == m.group(2):
            cur = out.setdefault(m.group(1), {"insts": [], "desc": {}, "code_len": None})
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        s = line.split(";", 1)[0].strip()
        if s and not s.startswith(".") and not s.endswith(":"):
            cur["insts"].append(s)
    # descriptors and code sizes (after the function bodies)
    kern = None
    for line in lines:
        m = re.match(r"^\s*\.amdhsa_kernel (\S+)", line)
        if m:
            kern = m.group(1)
            continue
        m = re.match(r"^\s*(\.amdhsa_\S+)\s+(\S+)", line)
        if m and kern in out and m.group(1) != ".amdhsa_code_object_version":   # (a directive of the file, at the head of every unit's listing)
            out[kern]["desc"][m.group(1)] = m.group(2)
            continue
        if line.strip() == ".end_amdhsa_kernel":
            continue
        m = re.match(r"^; codeLenInByte = (\d+)", line)
        if m and kern in out and out[kern]["code_len"] is None:
            out[kern]["code_len"] = int(m.group(1))
    return out


def parse_remarks(text: str) -> dict:
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][A-Za-z \[\]/]*): (\S+) \[-Rpass", line)
        if m and cur is not None and m.group(1).strip() in _REMARK_KEYS:
            cur[m.group(1).strip()] = m.group(2)
    return out


def _norm(inst: str, mask_offsets: bool) -> str:
    inst = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", inst)
    if mask_offsets and inst.startswith("s_load_"):
        inst = re.sub(r"(,\s*|offset:)(0x[0-9a-f]+|\d+)$", r"\1<off>", inst)
    return inst


def main(old_s, old_r, new_s, new_r) -> int:
    old, new = parse_listing(open(old_s).read()), parse_listing(open(new_s).read())
    rem_old, rem_new = parse_remarks(open(old_r).read()), parse_remarks(open(new_r).read())
    ok = True
    matched, removed = [], []
    for sym in old:
        n = sym if sym in new else new_name(sym)
        if n is None or n not in new:
            removed.append(sym)
        else:
            matched.append((sym, n))
    added = sorted(set(new) - {n for _, n in matched})
    identical = offsets_only = 0
    for o, n in matched:
        a, b = old[o], new[n]
        problems = []
        if rem_old.get(o) != rem_new.get(n):
            problems.append(f"resources {rem_old.get(o)} -> {rem_new.get(n)}")
        da = {k: v for k, v in a["desc"].items() if k != ".amdhsa_kernarg_size"}
        db = {k: v for k, v in b["desc"].items() if k != ".amdhsa_kernarg_size"}
        if da != db:
            problems.append(f"descriptor {[(k, da.get(k), db.get(k)) for k in sorted(set(da) | set(db)) if da.get(k) != db.get(k)]}")
        if a["code_len"] != b["code_len"]:
            problems.append(f"code length {a['code_len']} -> {b['code_len']}")
        if [i.split()[0] for i in a["insts"]] != [i.split()[0] for i in b["insts"]]:
            problems.append(f"mnemonic sequence differs ({len(a['insts'])} -> {len(b['insts'])} instructions)")
        elif [_norm(i, True) for i in a["insts"]] != [_norm(i, True) for i in b["insts"]]:
            diff = [(x, y) for x, y in zip(a["insts"], b["insts"]) if _norm(x, True) != _norm(y, True)]
            problems.append(f"{len(diff)} instructions differ beyond kernel-argument offsets, first: {diff[:3]}")
        if problems:
            ok = False
            print(f"DIFFERENT {n}:\n    " + "\n    ".join(problems))
            continue
        if [_norm(i, False) for i in a["insts"]] == [_norm(i, False) for i in b["insts"]]:
            identical += 1
        else:
            offsets_only += 1
            nd = sum(1 for x, y in zip(a["insts"], b["insts"]) if _norm(x, False) != _norm(y, False))
            print(f"kernarg offsets only ({nd} s_load lines, kernarg size {a['desc'].get('.amdhsa_kernarg_size')} -> "
                  f"{b['desc'].get('.amdhsa_kernarg_size')}): {n}")
    print(f"\n{len(matched)} kernels in both listings: {identical} identical, {offsets_only} differ only in kernel-argument offsets, "
          f"{len(matched) - identical - offsets_only} different")
    print(f"removed ({len(removed)}):" + "".join(f"\n    {s}" for s in removed))
    print(f"added ({len(added)}):" + "".join(f"\n    {s}" for s in added))
    return 0 if ok else 1


if __name__ == "__main__":
    if len(sys.argv) != 5:
        sys.exit(__doc__)
    sys.exit(main(*sys.argv[1:]))
