"""The host's --mds_align path under AddressSanitizer + UBSan on the CPU: the stand-alone binary of
test_host_sanitize_cpu.py, linked against the stub engine plus tests/host_sanitize/stub_mds.cpp, stub_boot_stats.cpp and
stub_mds_align.cpp -- the aligned entry points with no device behind them (their outputs are the host twins' on made-up
distances, so ngd_mds_align_host runs under the sanitizers too).  Checked: no sanitizer report, the files of each run form
and the shape of their blocks -- also where NGSDIST_WIN_GROUP_MAX cuts 7 windows of unequal length into engine calls of 3, 3
and 1 --, that <out> and matrix 0's blocks are the bytes of the run without the flag, and every refusal by its message and exit status 255.  (What the numbers are is the GPU suite's business:
tests/test_gpu_cli_mds_align.py.)"""
import os
import subprocess

import numpy as np
import pytest

from test_host_groups_cpu import build
from test_host_mds_cpu import mds_blocks, n_blocks_of
from test_host_nj_cpu import GROUP_MAX, same_shapes, seven_windows

EXTS = ("", ".mds", ".mds_mean", ".mds_sd", ".mds_lo", ".mds_hi", ".mds_fit", ".windows")
STATS = (".mds_mean", ".mds_sd", ".mds_lo", ".mds_hi")


@pytest.fixture(scope="module")
def san_bin(tmp_path_factory):
    return build(str(tmp_path_factory.mktemp("san") / "ngsDist_mds_align"),
                 ["stub_engine.cpp", "stub_mds.cpp", "stub_boot_stats.cpp", "stub_mds_align.cpp"])


@pytest.fixture(scope="module")
def san_bin_mds(tmp_path_factory):
    """without the aligned entry points: they are weak references, the build links without them"""
    return build(str(tmp_path_factory.mktemp("san0") / "ngsDist_mds"), ["stub_engine.cpp", "stub_mds.cpp", "stub_boot_stats.cpp"])


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


def stat_blocks(text, n, K):
    """the blocks of <out>.mds_mean and its kin: [(eig [K], labels, coordinates [n][K])] -- no "total" line"""
    assert text.endswith("\n\n")
    out = []
    for b in text[:-2].split("\n\n"):
        lines = [l.split("\t") for l in b.split("\n")]
        assert len(lines) == n + 1 and lines[0][0] == "eig" and len(lines[0]) == K + 1
        assert all(len(l) == K + 1 for l in lines[1:])
        for l in lines:
            for x in l[1:]:
                assert x == "nan" or (len(x.split("e")[0].lstrip("-")) == 12 and "e" in x), x  # "%.10e"
        out.append((np.array(lines[0][1:], dtype=float), [l[0] for l in lines[1:]], np.array([l[1:] for l in lines[1:]], dtype=float)))
    return out


def fit_lines(text, R):
    """<out>.mds_fit: [(used, fit [R])]"""
    assert text.endswith("\n")
    out = []
    for l in text[:-1].split("\n"):
        f = l.split("\t")
        assert len(f) == R + 1 and f[0].isdigit()
        out.append((int(f[0]), np.array(f[1:], dtype=float)))
    return out


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
    K = 3
    base = ["--geno", gl, "--probs", "--n_ind", n_ind, "--n_sites", n_sites, "--mds", K]
    bp = seven_windows(tmp_path) + ["--win_boot_rep", 2, "--boot_block_size", 7, "--seed", 3]
    ungrouped = None
    # (arguments, sets, replicates, windows shorter than a block, windows per engine call at the most: 0 = all)
    for extra, n_set, R, short, group_max in ((["--n_boot_rep", 3, "--boot_block_size", 10, "--seed", 5], 1, 3, 0, 0),
                                              (["--n_boot_rep", 40, "--boot_block_size", 7, "--indep_geno", "--labels", labels, "--seed", 9], 1, 40, 0, 0),
                                              (["--win_size", 40, "--win_step", 20, "--win_boot_rep", 2, "--boot_block_size", 7, "--seed", 3], 5, 2, 0, 0),
                                              (["--win_size", 5, "--win_step", 50, "--win_boot_rep", 2, "--boot_block_size", 7, "--seed", 4], 3, 2, 3, 0),
                                              (bp, 7, 2, 1, 0),
                                              (bp, 7, 2, 1, GROUP_MAX)):
        plain, _ = run(san_bin, tmp_path, base + extra, group_max=group_max)  # (the stubs' numbers follow the grouping)
        ci = ["--mds_ci", 0.8] if R == 40 else []
        files, err = run(san_bin, tmp_path, base + extra + ["--mds_align"] + ci, group_max=group_max)
        if group_max:
            same_shapes(files, ungrouped)
        ungrouped = files
        # <out>, and matrix 0 of every set in <out>.mds, are the bytes of the run without the flag
        assert files[""] == plain[""] and n_blocks_of(files[""], n_ind) == n_set
        assert files[".windows"] == plain[".windows"]
        theirs = plain[".mds"][:-2].split("\n\n")
        assert files[".mds"] == "".join(b + "\n\n" for b in theirs[::R + 1])
        assert len(mds_blocks(files[".mds"], n_ind, K)) == n_set
        names = [("name%d" if "--labels" in extra else "Ind_%d") % k for k in range(n_ind)]
        st = {ext: stat_blocks(files[ext], n_ind, K) for ext in STATS}
        fits = fit_lines(files[".mds_fit"], R)
        assert len(fits) == n_set and all(len(st[ext]) == n_set for ext in STATS)
        n_short = 0
        for w in range(n_set):
            used, fit = fits[w]
            assert used == int(np.isfinite(fit).sum()) and used in (0, R)
            n_short += used == 0
            for ext in STATS:
                eig, lab, xy = st[ext][w]
                assert lab == names
                finite = used >= (2 if ext == ".mds_sd" else 1)
                assert np.all(np.isfinite(eig)) == finite and np.all(np.isfinite(xy)) == finite
                assert finite or (np.all(np.isnan(eig)) and np.all(np.isnan(xy)))
            if used:
                assert np.all(fit >= 0)
                assert np.all(st[".mds_lo"][w][2] <= st[".mds_mean"][w][2] + 1e-9) and np.all(st[".mds_mean"][w][2] <= st[".mds_hi"][w][2] + 1e-9)
                assert np.all(st[".mds_sd"][w][2] >= 0) and np.all(st[".mds_lo"][w][0] <= st[".mds_hi"][w][0])
        assert n_short == short
        assert "\tmds_align: true\n\tmds_ci: %f\n" % (0.8 if ci else 0.95) in err
        assert ("WARNING: %d of the run's matrices" % (short * R) in err) == (short > 0)
    # without the flag: no line in the echo of the arguments, none of the files
    files, err = run(san_bin, tmp_path, base + ["--n_boot_rep", 3, "--boot_block_size", 10])
    assert "mds_align" not in err and all(files[ext] is None for ext in STATS + (".mds_fit",))


def test_refusals_by_message_and_exit_status(san_bin, san_bin_mds, tmp_path, data):
    gl, labels, n_ind, n_sites = data
    base = ["--geno", gl, "--probs", "--n_ind", n_ind, "--n_sites", n_sites]
    boot = ["--n_boot_rep", 3, "--boot_block_size", 10]
    err = run(san_bin, tmp_path, base + boot + ["--mds_align"], ok=False)
    assert "ERROR: [" in err and "--mds_align" in err and "--mds K" in err
    err = run(san_bin, tmp_path, base + ["--mds", 2, "--mds_align"], ok=False)
    assert "--mds_align" in err and "--n_boot_rep or --win_boot_rep" in err
    err = run(san_bin, tmp_path, base + ["--mds", 2, "--mds_align", "--win_size", 40], ok=False)
    assert "--mds_align" in err and "--n_boot_rep or --win_boot_rep" in err
    err = run(san_bin, tmp_path, base + boot + ["--mds", 2, "--mds_ci", 0.9], ok=False)
    assert "--mds_ci" in err and "requires" in err and "--mds_align" in err
    for ci in (0, 1, 1.5, -0.2, "x"):
        err = run(san_bin, tmp_path, base + boot + ["--mds", 2, "--mds_align", "--mds_ci", ci], ok=False)
        assert "--mds_ci" in err and "between 0 and 1" in err, ci
    # whatever --mds refuses
    err = run(san_bin, tmp_path, base + boot + ["--mds", n_ind, "--mds_align"], ok=False)
    assert "--mds K" in err and "between 1 and" in err
    err = run(san_bin, tmp_path, base + boot + ["--mds", 2, "--mds_align", "--nj"], ok=False)
    assert "--mds" in err and "--nj" in err
    err = run(san_bin, tmp_path, base + boot + ["--mds", 2, "--mds_align", "--boot_stats"], ok=False)
    assert "--mds" in err and "--boot_stats" in err
    # --boot_ci keeps its own refusal
    err = run(san_bin, tmp_path, base + boot + ["--mds", 2, "--mds_align", "--boot_ci", 0.9], ok=False)
    assert "--boot_ci" in err and "--boot_stats" in err
    # more replicates than the summaries serve; fewer sites than one block
    err = run(san_bin, tmp_path, base + ["--n_boot_rep", 1280, "--boot_block_size", 10, "--mds", 2, "--mds_align"], ok=False)
    assert "too many bootstrap replicates" in err and "--mds_align" in err
    err = run(san_bin, tmp_path, base + ["--n_boot_rep", 2, "--boot_block_size", 500, "--mds", 2, "--mds_align"], ok=False)
    assert "at least one bootstrap block" in err
    # an engine without the entry points
    assert "no aligned replicates (--mds_align)" in run(san_bin_mds, tmp_path, base + boot + ["--mds", 2, "--mds_align"], ok=False)
