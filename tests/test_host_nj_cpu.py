"""The host's --nj path under AddressSanitizer + UBSan on the CPU: the stand-alone binary of test_host_sanitize_cpu.py,
linked against the stub engine plus tests/host_sanitize/stub_nj.cpp -- the trees' entry points with no device behind them
(their records are ngd_nj_host's on made-up distances).  Checked: no sanitizer report, the files of each run form and their
line counts -- also where NGSDIST_WIN_GROUP_MAX cuts 7 windows of unequal length into engine calls of 3, 3 and 1 --, and every
refusal by its message and exit status 255.  (What the trees are is the GPU suite's business: tests/test_gpu_cli_nj.py.)"""
import os
import subprocess

import numpy as np
import pytest

import nj_expect as X
from test_host_groups_cpu import build

EXTS = ("", ".nwk", ".support.nwk", ".windows")
GROUP_MAX = 3  # NGSDIST_WIN_GROUP_MAX of the grouped runs: the 7 windows of seven_windows() in engine calls of 3, 3 and 1


def seven_windows(d):
    """the arguments of 7 windows in base pairs over 120 sites, after writing their positions file into d: 20, 20, 20, 20, 20,
    3 and 17 sites -- the sixth shorter than a bootstrap block of 7"""
    pos = [10 * s + 1 for s in range(100)] + [1001 + 10 * k for k in range(3)] + [1201 + 10 * k for k in range(17)]
    path = str(d / "pos.tsv")
    open(path, "w").write("".join("chr1\t%d\n" % x for x in pos))
    return ["--pos", path, "--win_bp", 200]


def same_shapes(files, other):
    """the files of a run cut into groups of windows against the ungrouped run's: the same files with the same numbers of lines
    and fields (the stubs' made-up numbers follow a window's index within its call), <out>.windows byte for byte"""
    assert files.keys() == other.keys() and files.get(".windows") == other.get(".windows")
    assert files[""] != other[""]  # (those numbers: the run did go to the engine in several calls)
    for ext in files:
        assert (files[ext] is None) == (other[ext] is None), ext
        if files[ext] is not None:
            assert [l.count("\t") for l in files[ext].split("\n")] == [l.count("\t") for l in other[ext].split("\n")], ext


@pytest.fixture(scope="module")
def san_bin(tmp_path_factory):
    return build(str(tmp_path_factory.mktemp("san") / "ngsDist_nj"), ["stub_engine.cpp", "stub_nj.cpp"])


@pytest.fixture(scope="module")
def san_bin_plain(tmp_path_factory):
    """the stub engine alone: the new entry points are weak references, the build links without them"""
    return build(str(tmp_path_factory.mktemp("san0") / "ngsDist_plain"), ["stub_engine.cpp"])


def run(binary, tmp_path, args, ok=True, verbose=1, group_max=0):
    out = str(tmp_path / "o.dist")
    for ext in EXTS:
        if os.path.exists(out + ext):
            os.remove(out + ext)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1",
               NGSDIST_WIN_GROUP_MAX=str(group_max))
    r = subprocess.run([binary] + [str(a) for a in args] + ["--out", out, "--verbose", str(verbose)], capture_output=True, env=env,
                       timeout=300)
    err = r.stderr.decode(errors="replace")
    assert "Sanitizer" not in err and "runtime error" not in err, err[-3000:]
    assert (r.returncode == 0) == ok, err[-1500:]
    if not ok:
        assert r.returncode == 255
        return err
    return {ext: open(out + ext).read() if os.path.exists(out + ext) else None for ext in EXTS}, err


def n_blocks_of(text, n):
    lines = text.split("\n")
    assert lines[-1] == "" and (len(lines) - 1) % (n + 2) == 0, len(lines)
    return (len(lines) - 1) // (n + 2)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = tmp_path_factory.mktemp("data")
    n_ind, n_sites = 9, 120
    gl = str(d / "g.bin")
    np.random.default_rng(1).dirichlet([0.5, 0.5, 0.5], size=(n_sites, n_ind)).tofile(gl)
    labels = str(d / "labels.txt")
    open(labels, "w").write("".join("name%d\n" % k for k in range(n_ind)))
    return gl, labels, n_ind, n_sites


def test_the_files_of_each_run_form(san_bin, tmp_path, data):
    gl, labels, n_ind, n_sites = data
    base = ["--geno", gl, "--probs", "--n_ind", n_ind, "--n_sites", n_sites, "--nj"]
    bp = seven_windows(tmp_path)
    ungrouped = None
    # (arguments, sets, replicates, windows shorter than a block, windows per engine call at the most: 0 = all)
    for extra, n_set, R, short, group_max in (([], 1, 0, 0, 0),
                                              (["--labels", labels], 1, 0, 0, 0),
                                              (["--n_boot_rep", 3, "--boot_block_size", 10, "--seed", 5], 1, 3, 0, 0),
                                              (["--n_boot_rep", 40, "--boot_block_size", 7, "--indep_geno"], 1, 40, 0, 0),
                                              (["--win_size", 40, "--win_step", 20], 5, 0, 0, 0),
                                              (["--win_size", 40, "--win_step", 20, "--win_boot_rep", 2, "--boot_block_size", 7, "--seed", 3], 5, 2, 0, 0),
                                              (["--win_size", 5, "--win_step", 50, "--win_boot_rep", 2, "--boot_block_size", 7], 3, 2, 3, 0),
                                              (bp, 7, 0, 0, 0),
                                              (bp, 7, 0, 0, GROUP_MAX),
                                              (bp + ["--win_boot_rep", 2, "--boot_block_size", 7, "--seed", 3], 7, 2, 1, 0),
                                              (bp + ["--win_boot_rep", 2, "--boot_block_size", 7, "--seed", 3], 7, 2, 1, GROUP_MAX)):
        files, err = run(san_bin, tmp_path, base + extra, group_max=group_max)
        if group_max:
            same_shapes(files, ungrouped)
        ungrouped = files
        assert n_blocks_of(files[""], n_ind) == n_set, extra
        trees = files[".nwk"].split("\n")
        assert trees[-1] == "" and len(trees) - 1 == n_set * (R + 1), extra
        no_tree = [t for t in trees[:-1] if t == ";"]
        assert len(no_tree) == short * R
        for t in trees[:-1]:
            assert t == ";" or (t.startswith("(") and t.endswith(");") and t.count("(") == n_ind - 2 and t.count(":") == 2 * n_ind - 3)
        name = "name%d:" if "--labels" in extra else "Ind_%d:"
        assert all((name % k) in trees[0] for k in range(n_ind))
        if R:
            sup = files[".support.nwk"].split("\n")
            assert sup[-1] == "" and len(sup) - 1 == n_set
            for w, t in enumerate(sup[:-1]):
                _, nodes = X.parse_newick(t)
                inner = [int(nm) for nm, _ in nodes if not nm.startswith(("Ind_", "name"))]
                in_short = trees[w * (R + 1) + 1] == ";"  # (a window shorter than a block: no replicate has a tree)
                assert in_short == (short == n_set or (short == 1 and w == 5))
                assert len(inner) == n_ind - 3 and all(0 <= s <= (0 if in_short else R) for s in inner)
        else:
            assert files[".support.nwk"] is None
        assert (files[".windows"] is not None) == ("--win_size" in extra or "--win_bp" in extra)
        assert "\tnj: true\n" in err
        assert ("WARNING: %d of the run's matrices" % (short * R) in err) == (short > 0)
    # the echo of the arguments has the line only with the flag
    out = str(tmp_path / "plain.dist")
    r = subprocess.run([san_bin, "--geno", gl, "--probs", "--n_ind", str(n_ind), "--n_sites", str(n_sites), "--out", out, "--verbose", "1"],
                       capture_output=True, timeout=300)
    assert r.returncode == 0 and "nj:" not in r.stderr.decode() and not os.path.exists(out + ".nwk")


def test_refusals_by_message_and_exit_status(san_bin, san_bin_plain, tmp_path, data):
    gl, labels, n_ind, n_sites = data
    base = ["--geno", gl, "--probs", "--n_ind", n_ind, "--n_sites", n_sites]
    boot = ["--n_boot_rep", 3, "--boot_block_size", 10]
    groups = str(tmp_path / "groups.txt")
    open(groups, "w").write("\n".join(["a", "b", "a"] * 3))
    err = run(san_bin, tmp_path, base + ["--nj", "--groups", groups], ok=False)
    assert "ERROR: [" in err and "--nj" in err and "--groups" in err
    err = run(san_bin, tmp_path, base + boot + ["--nj", "--boot_stats"], ok=False)
    assert "--nj" in err and "--boot_stats" in err
    err = run(san_bin, tmp_path, base + ["--nj", "--n_gpus", 2], ok=False)
    assert "--nj" in err and "--n_gpus 1" in err
    # fewer than three individuals
    gl2 = str(tmp_path / "g2.bin")
    np.random.default_rng(2).dirichlet([0.5, 0.5, 0.5], size=(n_sites, 2)).tofile(gl2)
    err = run(san_bin, tmp_path, ["--geno", gl2, "--probs", "--n_ind", 2, "--n_sites", n_sites, "--nj"], ok=False)
    assert "--nj" in err and "three individuals" in err
    # a data set that goes through the device in ranges of sites (the budget of test_host_groups_cpu.py: 40 of the 120 sites)
    budget = 256 * 128 * 128 * 8 + 36 * 64 + (512 << 20) + (24 * 128 + 40) * 40
    err = run(san_bin, tmp_path, base + ["--nj", "--max_device_bytes", budget], ok=False)
    assert "--nj" in err and "one GPU" in err
    # fewer sites than one block: no replicate visits a site
    err = run(san_bin, tmp_path, base + ["--n_boot_rep", 2, "--boot_block_size", 500, "--nj"], ok=False)
    assert "at least one bootstrap block" in err
    # an engine without the entry points
    assert "no neighbour-joining trees (--nj)" in run(san_bin_plain, tmp_path, base + ["--nj"], ok=False)
