"""Compare the gfx950 ISA of kernels in two builds of librgbm_hip.so, kernel by kernel.

usage: diff_kernel_isa.py <old.so> <new.so> <substring of the demangled kernel name> [more substrings ...]

Extracts the device code objects of both libraries (llvm-objdump --offloading), disassembles them (llvm-objdump -d) and compares the
instruction text of every kernel whose demangled name contains one of the substrings.  Kernels are paired by their demangled name with
defaulted template arguments the new build may have added stripped (a trailing ", 0" / "<0>"), so that an instantiation that gained a
template parameter with its old meaning as the default is compared with what it was.  Addresses and encodings are not compared, only the
instructions and their operands in order.  Prints one line per kernel and exits 1 if one differs or has no partner."""
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


def kernels(so, work):
    dst = os.path.join(work, os.path.basename(so))
    shutil.copy(so, dst)
    subprocess.run([OBJDUMP, "--offloading", dst], check=True, capture_output=True)
    out = {}
    for obj in sorted(glob.glob(dst + ".*gfx950")):
        dis = subprocess.run([OBJDUMP, "-d", "--demangle", obj], check=True, capture_output=True, text=True).stdout
        name = None
        for line in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
            if m:
                name = m.group(1)
                out[name] = []
            elif name and line.startswith("\t"):
                out[name].append(re.sub(r"\s*//.*$", "", line).strip())
    return out


def key(name):
    name = name.replace("(anonymous namespace)", "{anonymous}")      # its parentheses are no argument list
    name = re.sub(r"\(.*$", "", name)                       # drop the argument list
    name = re.sub(r"^void ", "", name)
    name = name.replace("<0>", "")                           # a kernel that became a template with its old meaning as <0>
    return name


def main():
    old_so, new_so, subs = sys.argv[1], sys.argv[2], sys.argv[3:]
    with tempfile.TemporaryDirectory() as a, tempfile.TemporaryDirectory() as b:
        old, new = kernels(old_so, a), kernels(new_so, b)
    bad = 0
    for name in sorted(old):
        if not any(s in name for s in subs):
            continue
        k = key(name)
        partner = [n for n in new if key(n) == k or key(n) == k[:-1] + ", 0>"]
        if len(partner) != 1:
            print(f"NO PARTNER  {k}  ({len(partner)} candidates)")
            bad += 1
            continue
        same = old[name] == new[partner[0]]
        print(f"{'identical ' if same else 'DIFFERENT '} {len(old[name]):6d} instructions  {k}")
        bad += not same
    extra = [n for n in sorted(new) if any(s in n for s in subs) and not any(key(n) in (key(o), key(o)[:-1] + ", 0>") for o in old)]
    for n in extra:
        print(f"new         {len(new[n]):6d} instructions  {key(n)}")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
