#!/usr/bin/env python
"""Two builds of the command-line host over one table of command lines: --nj, --mds K, --mds K --mds_align, --boot_stats with
and without --groups, and --win_cmp --win_cmp_mds 2 -- whole genome and windows (in sites, in sites shorter than a block, in
base pairs with one window shorter than a block), without replicates where the mode allows it and with 3, NGSDIST_WIN_GROUP_MAX
unset and 3, --verbose 0 / 1 / 2, and each mode's refusal of replicates on fewer sites than one block.  Compared per run: the
exit status, every output file byte for byte, and stderr without the lines that carry seconds.  Prints one line: runs and
differences.

  python tools/host_sets_compare.py --old BIN --new BIN [--n_ind 9 --n_sites 120] [--geno FILE.bin]

Without --geno a file of random genotype posteriors is written.  The window sizes scale with --n_sites / 120."""
import argparse
import glob
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

SECONDS = re.compile(r"\d\.\d+ m?s\b|^> phases")


def table(n_sites, pos, groups):
    u = n_sites // 120
    rep = ["--boot_block_size", 7 * u]
    genome = [[]] + [["--n_boot_rep", 3] + rep]
    windows = [["--win_size", 30 * u, "--win_step", 15 * u], ["--win_size", 5 * u, "--win_step", 19 * u],
               ["--pos", pos, "--win_bp", 200 * u]]
    modes = [(["--nj"], True), (["--mds", 4], True), (["--mds", 4, "--mds_align"], False), (["--boot_stats"], False),
             (["--boot_stats", "--groups", groups], False)]
    runs = []
    for mode, plain_ok in modes:
        for g in genome:
            if g or plain_ok:
                runs += [(mode + g, 0, v) for v in (0, 1, 2)]
        for w in windows:
            for r in ([], ["--win_boot_rep", 3] + rep):
                if r or plain_ok:
                    runs += [(mode + w + r, gm, v) for gm in (0, 3) for v in (0, 1, 2)]
        runs.append((mode + ["--n_boot_rep", 2, "--boot_block_size", 500 * n_sites], 0, 1))  # refused: no whole block
    for w in windows:
        runs += [(["--win_cmp", "--win_cmp_mds", 2] + w, gm, v) for gm in (0, 3) for v in (0, 1, 2)]
    return runs


def run(binary, base, args, group_max, verbose, d):
    out = os.path.join(d, "o.dist")
    for f in glob.glob(out + "*"):
        os.remove(f)
    env = dict(os.environ)
    env.pop("NGSDIST_WIN_GROUP_MAX", None)
    if group_max:
        env["NGSDIST_WIN_GROUP_MAX"] = str(group_max)
    r = subprocess.run([binary] + [str(a) for a in base + args] + ["--out", out, "--verbose", str(verbose)], capture_output=True, env=env,
                       timeout=300)
    err = [l for l in r.stderr.decode(errors="replace").split("\n") if not SECONDS.search(l)]
    return r.returncode, err, {os.path.basename(f): open(f, "rb").read() for f in sorted(glob.glob(out + "*"))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", required=True)
    ap.add_argument("--new", required=True)
    ap.add_argument("--n_ind", type=int, default=9)
    ap.add_argument("--n_sites", type=int, default=120)
    ap.add_argument("--geno")
    a = ap.parse_args()
    n, u = a.n_sites, a.n_sites // 120
    with tempfile.TemporaryDirectory() as d:
        geno = a.geno or os.path.join(d, "g.bin")
        if not a.geno:
            np.random.default_rng(1).dirichlet([0.5, 0.5, 0.5], size=(n, a.n_ind)).tofile(geno)
        # positions for --win_bp: a chromosome whose last two windows hold 3 u and 17 u sites
        first = n - 20 * u
        coords = [10 * s + 1 for s in range(first)] + [10 * first + 1 + 10 * k for k in range(3 * u)] + \
                 [10 * first + 200 * u + 1 + 10 * k for k in range(17 * u)]
        pos = os.path.join(d, "pos.tsv")
        open(pos, "w").write("".join("chr1\t%d\n" % x for x in coords))
        groups = os.path.join(d, "groups.txt")
        open(groups, "w").write("\n".join(("north", "south", "NA", "north", "south", "solo")[k % 6] for k in range(a.n_ind)) + "\n")
        # (--seed on every line: without it the echo of the arguments prints the clock's)
        base = ["--geno", geno, "--probs", "--n_ind", a.n_ind, "--n_sites", n, "--seed", 3]
        runs = table(n, pos, groups)
        n_diff = n_ok = n_files = 0
        for args, gm, v in runs:
            old, new = (run(b, base, args, gm, v, d) for b in (a.old, a.new))
            if any(s[0] not in (0, 255) for s in (old, new)):  # (killed, or no refusal of the host's: nothing more is started)
                print("STOPPED at %s: status %d / %d\n%s" % (args, old[0], new[0], "\n".join((old[1] + new[1])[-20:])), file=sys.stderr)
                return 2
            n_ok += old[0] == 0
            n_files += len(old[2])
            if old != new:
                n_diff += 1
                print("DIFFERENT: %s NGSDIST_WIN_GROUP_MAX=%d --verbose %d: status %d / %d, files %s" % (
                    " ".join(str(x) for x in args), gm, v, old[0], new[0],
                    [k for k in set(old[2]) | set(new[2]) if old[2].get(k) != new[2].get(k)]), file=sys.stderr)
                print("\n".join(sorted(set(old[1]) ^ set(new[1]))[:10]), file=sys.stderr)
    print("%d x %d: %d command lines with either binary (%d exit 0, %d refused; %d output files), %d differences"
          % (a.n_ind, n, len(runs), n_ok, len(runs) - n_ok, n_files, n_diff))
    return 1 if n_diff else 0


if __name__ == "__main__":
    sys.exit(main())
