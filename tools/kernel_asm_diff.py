#!/usr/bin/env python3
"""Per-kernel gfx950 assembly of the implicit-GEMM translation units of two source trees, compared body by body.  No GPU.

    tools/kernel_asm_diff.py OLD_TREE NEW_TREE [--files-a a.hip,b.hip] [--files-b ...] [--rename 'REGEX=REPL' ...] [--keep DIR]

Each tree's GEMM files (default: every csrc/igemm_*.hip and csrc/conv_igemm_glds.hip it has) are compiled with the flags of that
tree's build.sh plus `--cuda-device-only -S`.  The output is cut into kernel bodies - from the `name:` label of every
.amdhsa_kernel to its `.Lfunc_end`, a range that holds the kernel's descriptor block - and the bodies are compared after
these normalisations, and no others:
  * `;` comments dropped
  * `.LBB<n>_` -> `.LBB_`, `.Ltmp<n>` -> `.Ltmp`, `.Lfunc_end<n>` -> `.Lfunc_end` (the function index changes with the file)
  * the zero page's symbol (external or internal linkage) -> one name
  * every --rename applied to symbol names (for a kernel whose template parameters changed on purpose)
Exit status 0: the same kernels on both sides and every body equal.  A kernel that differs is printed with its first differing lines.
"""
import argparse
import concurrent.futures
import difflib
import glob
import os
import re
import subprocess
import sys
import tempfile

ZERO_PAGE = re.compile(r"_ZN4rgbmL?11g_zero_pageE")


def build_flags(csrc):
    """FLAGS of build.sh: every FLAGS="..." line, with $FLAGS expanded."""
    flags = ""
    for line in open(os.path.join(csrc, "build.sh")):
        m = re.match(r'\s*FLAGS="(.*)"\s*$', line)
        if m:
            flags = m.group(1).replace("$FLAGS", flags)
    return flags.split()


def compile_asm(tree, files, outdir):
    csrc = os.path.join(tree, "rgbmanip_amd", "csrc")
    if not files:
        files = sorted(os.path.basename(f) for f in glob.glob(os.path.join(csrc, "igemm_*.hip")) + glob.glob(os.path.join(csrc, "conv_igemm_glds.hip")))
    if not files:
        sys.exit(f"{csrc}: no implicit-GEMM translation unit found")
    flags = build_flags(csrc)
    os.makedirs(outdir, exist_ok=True)

    def one(f):
        out = os.path.join(outdir, os.path.splitext(f)[0] + ".s")
        subprocess.run(["hipcc"] + flags + ["--cuda-device-only", "-S", f, "-o", out], cwd=csrc, check=True)
        return out

    with concurrent.futures.ThreadPoolExecutor(max_workers=min(len(files), os.cpu_count() or 1, 8)) as ex:
        return list(ex.map(one, files))


def kernel_bodies(asm_files, renames):
    """name -> normalised lines of the function body + its .amdhsa_kernel block"""
    def norm(line):
        line = line.split(";", 1)[0].rstrip()
        line = re.sub(r"\.LBB\d+_", ".LBB_", line)
        line = re.sub(r"\.Ltmp\d+", ".Ltmp", line)
        line = re.sub(r"\.Lfunc_end\d+", ".Lfunc_end", line)
        line = ZERO_PAGE.sub("g_zero_page", line)
        for pat, repl in renames:
            line = pat.sub(repl, line)
        return line

    bodies = {}
    for path in asm_files:
        lines = [norm(l) for l in open(path)]
        kernels = [m.group(1) for l in lines if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l))]
        for name in kernels:
            start = lines.index(name + ":")
            end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
            if name in bodies:
                sys.exit(f"kernel {name} is defined twice")
            bodies[name] = [l for l in lines[start:end + 1] if l.strip()]
            if not any(l.strip() == ".end_amdhsa_kernel" for l in bodies[name]):
                sys.exit(f"kernel {name}: no descriptor block inside its body")
    return bodies


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old_tree")
    ap.add_argument("new_tree")
    ap.add_argument("--files-a", default="")
    ap.add_argument("--files-b", default="")
    ap.add_argument("--rename", action="append", default=[], help="REGEX=REPL applied to both sides")
    ap.add_argument("--keep", default=None, help="directory to keep the .s files in")
    a = ap.parse_args()
    renames = [(re.compile(r.split("=", 1)[0]), r.split("=", 1)[1]) for r in a.rename]
    with tempfile.TemporaryDirectory() as tmp:
        root = a.keep or tmp
        with concurrent.futures.ThreadPoolExecutor(max_workers=2) as ex:      # both trees at once
            asm = list(ex.map(lambda t: compile_asm(t[1], [f for f in t[2].split(",") if f], os.path.join(root, t[0])),
                              (("a", a.old_tree, a.files_a), ("b", a.new_tree, a.files_b))))
        old, new = (kernel_bodies(files, renames) for files in asm)
    bad = 0
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            print(f"ONLY IN {'old' if name in old else 'new'}: {name}")
            bad += 1
        elif old[name] != new[name]:
            bad += 1
            print(f"DIFFERS: {name} ({len(old[name])} / {len(new[name])} lines)")
            for l in list(difflib.unified_diff(old[name], new[name], "old", "new", lineterm="", n=1))[:24]:
                print("    " + l)
    print(f"{len(old)} kernels old, {len(new)} new, {len(set(old) & set(new)) - sum(1 for n in set(old) & set(new) if old[n] != new[n])} equal bodies, {bad} problems")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
