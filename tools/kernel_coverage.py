#!/usr/bin/env python3
"""tools/kernel_coverage.py [stats.csv ...] [--list] -- which compiled kernels did a traced run never launch?

Three dispatchers of the engine pick a template instantiation from a count the caller controls (ngd_launch_contract:
k_contract_mfma<RT, PT>; the shape table of accum_em_table.hip; ngd_reduce_chunk: k_reduce_band_w<RB, CNT>), and a test
that compares an output with the oracle says nothing about WHICH compiled form produced it.  This tool answers that from
names alone, on the host (no GPU use):

  * it compiles every ngsdist_amd/csrc/*.hip to gfx950 assembly the way tools/check_asm_loads.py does (hipcc -S
    --cuda-device-only, the Makefile's flags) and collects the kernel entry names (.amdhsa_kernel), demangled;
  * it reads the kernel names of one or more kernel-trace statistics files (`rocprofv3 --kernel-trace --stats`:
    *_kernel_stats.csv, column "Name"; or any text file with one name per line, mangled or demangled);
  * it prints the instantiations that were never launched, file by file, and a count.

Names are compared as `kernel<template arguments>` -- the return type, `(anonymous namespace)::` and the parameter list
are dropped, so the two demanglers need not agree on how they spell a parameter.

    rocprofv3 --kernel-trace --stats -d trace -- python -m pytest -m gpu --deselect tests/test_gpu_fullsize.py
    tools/kernel_coverage.py trace/*/*_kernel_stats.csv > profiles/kernel_coverage/after.txt

--list: print the static list alone (every kernel the library holds).  Exit 0 always: the list is a report, not a check."""
import concurrent.futures
import csv
import glob
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ngsdist_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-ffp-contract=off", "-std=c++17"]


def demangle(names):
    names = list(names)
    if not names:
        return []
    for tool in (os.path.join(os.path.dirname(HIPCC), "..", "llvm", "bin", "llvm-cxxfilt"), "llvm-cxxfilt", "c++filt"):
        try:
            r = subprocess.run([tool], input="\n".join(names) + "\n", capture_output=True, text=True)
        except OSError:
            continue
        if r.returncode == 0:
            out = r.stdout.splitlines()
            if len(out) == len(names):
                return out
    raise SystemExit("no demangler found (llvm-cxxfilt, c++filt)")


def short_name(name):
    """`void (anonymous namespace)::k<1, 4>(double const*, ...) [clone .kd]` -> `k<1, 4>`"""
    s = name.strip().strip('"')
    s = re.sub(r"\s*\[clone [^\]]*\]$", "", s)
    s = re.sub(r"\.kd$", "", s)
    s = s.replace("(anonymous namespace)::", "")
    depth, cut = 0, len(s)
    for k, ch in enumerate(s):
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            cut = k
            break
    s = s[:cut].strip()
    # a return type stands before the name, separated by a blank outside any <...>
    depth, last = 0, 0
    for k, ch in enumerate(s):
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == " " and depth == 0:
            last = k + 1
    s = s[last:]
    return re.sub(r"\s+", " ", re.sub(r"\s*,\s*", ", ", s))


def kernels_of_file(src):
    asm = subprocess.run([HIPCC, *FLAGS, "-S", "--cuda-device-only", src, "-o", "-"], capture_output=True, text=True)
    if asm.returncode != 0:
        raise SystemExit("hipcc failed on %s:\n%s" % (src, asm.stderr[-2000:]))
    return sorted(set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm.stdout, flags=re.M)))


def static_list():
    """-> {file name: [kernel<args>, ...]} of every .hip file that holds a kernel"""
    files = sorted(glob.glob(os.path.join(CSRC, "*.hip")))
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        mangled = list(pool.map(kernels_of_file, files))
    out = {}
    for f, names in zip(files, mangled):
        if names:
            out[os.path.basename(f)] = sorted(set(short_name(n) for n in demangle(names)))
    return out


def traced_names(path):
    """kernel names of a statistics file: the "Name" column of a csv, else one name per line"""
    with open(path, newline="") as fh:
        text = fh.read()
    rows = list(csv.reader(text.splitlines()))
    names = []
    if rows and "Name" in rows[0]:
        k = rows[0].index("Name")
        names = [r[k] for r in rows[1:] if len(r) > k]
    else:
        names = [l for l in text.splitlines() if l.strip() and not l.startswith("#")]
    mangled = [n for n in names if n.strip().strip('"').startswith("_Z")]
    plain = [n for n in names if not n.strip().strip('"').startswith("_Z")]
    return set(short_name(n) for n in plain + demangle([re.sub(r"\.kd$", "", n.strip().strip('"')) for n in mangled]))


def main():
    args = [a for a in sys.argv[1:] if a != "--list"]
    have = static_list()
    total = sum(len(v) for v in have.values())
    if "--list" in sys.argv[1:] or not args:
        print("# %d kernels in %d files" % (total, len(have)))
        for f, names in have.items():
            print("%s (%d)" % (f, len(names)))
            for n in names:
                print("  " + n)
        return
    seen = set()
    for path in args:
        seen |= traced_names(path)
    ours = set(n for names in have.values() for n in names)
    missing = total - len(ours & seen)
    print("# %d kernels in %d files, %d launched, %d never launched (%d statistics file(s))"
          % (total, len(have), total - missing, missing, len(args)))
    for f, names in have.items():
        never = [n for n in names if n not in seen]
        print("%s: %d of %d never launched" % (f, len(never), len(names)))
        for n in never:
            print("  " + n)


if __name__ == "__main__":
    main()
