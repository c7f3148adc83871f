#!/usr/bin/env python3
"""Are the gfx950 kernels of two builds the same code?  No GPU needed.

    python tools/compare_kernels.py OLD NEW [--map FILE] [--quiet]

OLD / NEW: libpercnn_pi.so (or any host object / library with HIP offload bundles, or a bare code object).  Per kernel of OLD
it prints whether NEW holds a kernel of the same demangled name<template arguments> -- after the renames of FILE, lines
`regex => replacement` applied to OLD's names -- with the same instruction stream (llvm-objdump -d; addresses, encodings and
the symbol names in comments dropped) and the same resource metadata (register counts, spills, LDS, scratch, kernarg size).
Exit status 0 only if every kernel pairs up one to one and every pair is equal.  The argument list is not part of a name: it
repeats the template arguments for every kernel here, and a rename need not spell it."""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
META = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".group_segment_fixed_size",
        ".private_segment_fixed_size", ".kernarg_segment_size", ".max_flat_workgroup_size", ".wavefront_size")


def run(*cmd):
    return subprocess.run([os.path.join(LLVM, cmd[0]), *cmd[1:]], check=True, capture_output=True, text=True).stdout


def code_objects(path, tmp):
    """the gfx950 code objects bundled in `path` (llvm-objdump --offloading writes them next to its input: work on a copy)"""
    copy = shutil.copy(path, tmp)
    run("llvm-objdump", "--offloading", copy)
    found = sorted(os.path.join(tmp, f) for f in os.listdir(tmp) if "amdgcn" in f)
    return found or [copy]


def short(demangled):
    """`void pi::k<float, 2>(float*, int)` -> `pi::k<float, 2>`"""
    s, depth = demangled.removeprefix("void "), 0
    for i, c in enumerate(s):
        depth += (c == "<") - (c == ">")
        if c == "(" and depth == 0:
            return s[:i]
    return s


def kernels(path):
    """{short name: (instruction lines, metadata)} over every code object of a build"""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in code_objects(path, tmp):
            meta = {}
            for block in run("llvm-readelf", "--notes", co).split("amdhsa.kernels:")[-1].split("\n  - ")[1:]:
                fields = dict(re.findall(r"^(?:    )?(\.\w+): +(\S+)$", block, re.M))     # the kernel's own keys, not its .args'
                if ".name" in fields:                                                    # (amdhsa.version's items follow)
                    meta[fields[".name"]] = tuple(fields.get(k) for k in META)
            text, cur = {}, None
            for line in run("llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co).splitlines():
                m = re.match(r"^[0-9a-f]* ?<(.+)>:$", line)
                if m:
                    cur = text.setdefault(m.group(1), [])
                elif cur is not None and line.strip():
                    ins = line.split("//")[0].strip()
                    if cur and cur[-1].startswith("s_getpc_b64"):            # pc-relative address of a global: layout, not code
                        ins = re.sub(r"0x[0-9a-f]+$", "<pcrel>", ins)
                    cur.append(ins)
            for lines in text.values():                                      # alignment padding behind the last instruction
                while lines and lines[-1].split()[0] in ("s_nop", "s_code_end", "..."):
                    lines.pop()
            names = sorted(meta)
            demangled = subprocess.run(["c++filt"], input="\n".join(names), check=True, capture_output=True, text=True).stdout
            for sym, dem in zip(names, demangled.splitlines()):
                assert short(dem) not in out, f"two kernels named {short(dem)}"
                out[short(dem)] = (text[sym], meta[sym])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--map", help="file of `regex => replacement` renames, old name -> new name")
    ap.add_argument("--quiet", action="store_true", help="list only the kernels that differ")
    a = ap.parse_args()
    rules = []
    for line in open(a.map) if a.map else []:
        if "=>" in line and not line.startswith("#"):
            pat, rep = (s.strip() for s in line.split("=>"))
            rules.append((re.compile(pat), rep))
    old, new = kernels(a.old), kernels(a.new)
    left, equal, renamed, bad = set(new), 0, 0, []
    for name in sorted(old):
        target = name
        for pat, rep in rules:
            if pat.fullmatch(name):
                target = pat.sub(rep, name)
                break
        renamed += target != name
        if target not in left:
            verdict = "MISSING in new (or taken twice)"
        else:
            left.discard(target)
            (t0, m0), (t1, m1) = old[name], new[target]
            verdict = "equal" if (t0, m0) == (t1, m1) else "DIFFERENT:" + (
                f" instructions ({len(t0)} -> {len(t1)})" if t0 != t1 else "") + (
                " metadata " + ", ".join(f"{k} {x} -> {y}" for k, x, y in zip(META, m0, m1) if x != y) if m0 != m1 else "")
        equal += verdict == "equal"
        if verdict != "equal":
            bad.append(name)
        if verdict != "equal" or not a.quiet:
            print(f"{verdict:8s} {name}" + (f"  ->  {target}" if target != name else ""))
    for name in sorted(left):
        print(f"ONLY in new: {name}")
    print(f"kernels: {len(old)} old, {len(new)} new; compared {len(old)} ({renamed} under a rename): {equal} equal, "
          f"{len(bad)} different or missing, {len(left)} only in new")
    return 0 if not bad and not left else 1


if __name__ == "__main__":
    sys.exit(main())
