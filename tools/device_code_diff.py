#!/usr/bin/env python3
"""Is the device code of the working tree the device code of another commit?  No GPU needed.
    python tools/device_code_diff.py [REV] [-j JOBS]          (REV defaults to HEAD)
Compiles every device unit of polydeal_amd/csrc to gfx950 assembly with the Makefile's flags plus --cuda-device-only -S, at REV
(extracted with git archive into a temporary directory) and in the working tree, and compares per unit the set of function symbols
and, per symbol, a hash of its text: instructions, .amdhsa_* block, .set lines and its entry of the metadata.  The order of the
functions in a file may differ (block labels carry the function's index: taken out, as are the comments), lines naming the
compilation-unit id __hip_cuid_* are ignored (the id follows the output path).  Exit status 1 if anything differs.
A refactor of the launchers or the driver that claims unchanged kernel time proves it with this."""
import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("polydeal_amd", "csrc")
# (name, source, extra flags) of every device unit.  This list must match the .hip units of polydeal_amd/csrc/Makefile (pdh_inst.hip once per
# PDH_GROUP): a unit that is missing here is a unit whose kernels the comparison does not see.
UNITS = [("inst_g%d" % g, "pdh_inst.hip", ["-DPDH_GROUP=%d" % g]) for g in range(8)] + [
    (u, "pdh_%s.hip" % u, []) for u in ("rhs", "eval", "exchange", "moment", "terms", "matfree", "cartgen", "tiled", "solve", "shadow", "transfer")]


def makefile_flags(csrc):
    text = open(os.path.join(csrc, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS\s*=\s*(.*)$", text, re.M).group(1)
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    return flags.replace("$(ARCH)", arch).replace("$(DEFS)", "").split()


def compile_unit(csrc, out_dir, unit):
    name, src, defs = unit
    if not os.path.exists(os.path.join(csrc, src)):  # a unit the other side does not have yet
        return name, None
    out = os.path.join(out_dir, name + ".s")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc] + makefile_flags(csrc) + defs + ["--cuda-device-only", "-S", src, "-o", out], cwd=csrc, check=True,
                   stderr=subprocess.DEVNULL)
    return name, out


LABEL = re.compile(r"(\.LBB|\.LJTI|\.Lfunc_begin|\.Lfunc_end)\d+")  # (.LBB<function>_<block>)
COMMENT = re.compile(r"\s*;.*$")  # (loop notes naming blocks, aligned by the width of the function's index)


def functions(path):
    """{symbol: hash of its text and metadata entry}; '<rest>' is what follows the last function (data objects)"""
    text, _, meta = open(path).read().partition("\t.amdgpu_metadata\n")
    lines = [LABEL.sub(r"\1", COMMENT.sub("", l)) for l in text.split("\n") if "__hip_cuid_" not in l]
    starts = []  # (first line, symbol): a function's .type line and the section / linkage directives in front of it
    for i, l in enumerate(lines):
        m = re.match(r"\t\.type\t(\S+),@function", l)
        if m:
            k = i
            while k > 0 and lines[k - 1].startswith(("\t.text", "\t.section\t.text", "\t.protected", "\t.globl", "\t.weak", "\t.hidden", "\t.p2align")):
                k -= 1
            starts.append((k, m.group(1)))
    end = next((i for i, l in enumerate(lines) if l.startswith("\t.section\t.AMDGPU.gpr_maximums")), len(lines))
    while end > 0 and lines[end - 1].startswith(("\t.text", "\t.p2alignl", "\t.fill")):  # (the padding behind the last function)
        end -= 1
    parts = {"<rest>": "\n".join(lines[end:])}
    for (b, sym), (e, _) in zip(starts, starts[1:] + [(end, None)]):
        parts[sym] = "\n".join(lines[b:e])
    for entry in re.split(r"^  - ", meta.partition("amdhsa.kernels:\n")[2].partition("amdhsa.target:")[0], flags=re.M)[1:]:
        parts[re.search(r"^    \.name:\s+(\S+)", entry, re.M).group(1)] += "\n<metadata>\n" + entry
    return {sym: hashlib.sha256(t.encode()).hexdigest() for sym, t in parts.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("rev", nargs="?", default="HEAD")
    ap.add_argument("-j", "--jobs", type=int, default=min(8, os.cpu_count() or 1))
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(["git", "-C", ROOT, "archive", a.rev, CSRC], check=True, stdout=subprocess.PIPE).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
        sides = {"rev": (os.path.join(tmp, CSRC), os.path.join(tmp, "s_rev")), "tree": (os.path.join(ROOT, CSRC), os.path.join(tmp, "s_tree"))}
        with ThreadPoolExecutor(a.jobs) as pool:
            jobs = {}
            for side, (csrc, out_dir) in sides.items():
                os.makedirs(out_dir)
                jobs[side] = [pool.submit(compile_unit, csrc, out_dir, u) for u in UNITS]
            asm = {side: dict(j.result() for j in js) for side, js in jobs.items()}
        bad = 0
        for name, _, _ in UNITS:
            if asm["rev"][name] is None or asm["tree"][name] is None:
                print("%-9s %s" % (name, "not at %s: a new unit" % a.rev if asm["rev"][name] is None else "not in the tree: DIFFERENT"))
                bad += asm["tree"][name] is None
                continue
            fa, fb = functions(asm["rev"][name]), functions(asm["tree"][name])
            diff = (["only at %s: %s" % (a.rev, s) for s in sorted(set(fa) - set(fb))] + ["only in the tree: %s" % s for s in sorted(set(fb) - set(fa))] +
                    ["differs: %s" % s for s in sorted(set(fa) & set(fb)) if fa[s] != fb[s]])
            print("%-9s %3d functions  %s" % (name, len(fb) - 1, "identical" if not diff else "DIFFERENT"))
            for d in diff:
                print("    " + d)
            bad += len(diff)
        print("device code of the working tree %s that of %s" % ("DIFFERS from" if bad else "is", a.rev))
        return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
