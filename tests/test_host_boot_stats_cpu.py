"""The host's --boot_stats path under AddressSanitizer + UBSan on the CPU: the stand-alone binary of
test_host_sanitize_cpu.py, linked against the stub engine plus tests/host_sanitize/stub_boot_stats.cpp (and stub_groups.cpp)
-- the summaries' entry points with no compute behind them.  Checked: no sanitizer report, the files of a run and the
shapes of their blocks -- also where NGSDIST_WIN_GROUP_MAX cuts 7 windows of unequal length into engine calls of 3, 3 and 1 --,
and every refusal by its message and exit status 255.  (What the numbers are is the GPU suite's
business: tests/test_gpu_cli_boot_stats.py.)"""
import os
import subprocess

import numpy as np
import pytest

from test_host_groups_cpu import build
from test_host_nj_cpu import GROUP_MAX, same_shapes, seven_windows

EXTS = ("", ".boot_mean", ".boot_sd", ".boot_lo", ".boot_hi", ".boot_used")


@pytest.fixture(scope="module")
def san_bin(tmp_path_factory):
    return build(str(tmp_path_factory.mktemp("san") / "ngsDist_stats"), ["stub_engine.cpp", "stub_groups.cpp", "stub_boot_stats.cpp"])


@pytest.fixture(scope="module")
def san_bin_plain(tmp_path_factory):
    """the stub engine alone: the new entry points are weak references, the build links without them"""
    return build(str(tmp_path_factory.mktemp("san0") / "ngsDist_plain"), ["stub_engine.cpp"])


def run(binary, tmp_path, args, ok=True, verbose=1, group_max=0):
    out = str(tmp_path / "o.dist")
    for ext in EXTS + (".windows", ".used"):
        if os.path.exists(out + ext):
            os.remove(out + ext)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1",
               NGD_STUB_GROUP_PAIRS="6", NGSDIST_WIN_GROUP_MAX=str(group_max))
    r = subprocess.run([binary] + [str(a) for a in args] + ["--out", out, "--verbose", str(verbose)], capture_output=True, env=env,
                       timeout=300)
    err = r.stderr.decode(errors="replace")
    assert "Sanitizer" not in err and "runtime error" not in err, err[-3000:]
    assert (r.returncode == 0) == ok, err[-1500:]
    if not ok:
        assert r.returncode == 255
        return err
    return {ext: open(out + ext).read() for ext in EXTS}, err


def n_blocks_of(text, n):
    lines = text.split("\n")
    assert lines[-1] == "" and (len(lines) - 1) % (n + 2) == 0, len(lines)
    for k in range(0, len(lines) - 1, n + 2):
        assert lines[k] == "" and lines[k + 1] == str(n)
        assert all(len(l.split("\t")) == n + 1 for l in lines[k + 2:k + n + 2])
    return (len(lines) - 1) // (n + 2)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = tmp_path_factory.mktemp("data")
    n_ind, n_sites = 9, 120
    gl = str(d / "g.bin")
    np.random.default_rng(1).dirichlet([0.5, 0.5, 0.5], size=(n_sites, n_ind)).tofile(gl)
    groups = str(d / "groups.txt")
    open(groups, "w").write("\n".join(["north", "south", "NA", "north", "", "solo", "-", "south", "north"]))
    return gl, groups, n_ind, n_sites


def test_the_six_files_of_a_run(san_bin, tmp_path, data):
    gl, groups, n_ind, n_sites = data
    base = ["--geno", gl, "--probs", "--n_ind", n_ind, "--n_sites", n_sites, "--boot_stats"]
    bp = seven_windows(tmp_path)  # (7 windows, the sixth shorter than a block)
    ungrouped = {}
    # (arguments, sets, windows per engine call at the most: 0 = all)
    for extra, n_set, group_max in ((["--n_boot_rep", 3, "--boot_block_size", 10, "--seed", 5], 1, 0),
                                    (["--n_boot_rep", 70, "--boot_block_size", 7, "--indep_geno", "--boot_ci", 0.5], 1, 0),
                                    (["--win_size", 40, "--win_step", 20, "--win_boot_rep", 2, "--boot_block_size", 7, "--seed", 3], 5, 0),
                                    (["--win_size", 5, "--win_step", 50, "--win_boot_rep", 2, "--boot_block_size", 7], 3, 0),
                                    (["--win_boot_rep", 2, "--boot_block_size", 7, "--seed", 3] + bp, 7, 0),
                                    (["--win_boot_rep", 2, "--boot_block_size", 7, "--seed", 3] + bp, 7, GROUP_MAX)):
        for grp in (False, True):
            files, err = run(san_bin, tmp_path, base + extra + (["--groups", groups] if grp else []), group_max=group_max)
            windows = open(str(tmp_path / "o.dist.windows")).read() if os.path.exists(str(tmp_path / "o.dist.windows")) else None
            if group_max:
                same_shapes(files, ungrouped[grp][0])
                assert windows == ungrouped[grp][1]
            ungrouped[grp] = files, windows
            n = 3 if grp else n_ind
            assert [n_blocks_of(files[ext], n) for ext in EXTS] == [n_set] * 6, (extra, grp)
            R = extra[extra.index("--n_boot_rep" if "--n_boot_rep" in extra else "--win_boot_rep") + 1]
            cells = [c for l in files[".boot_used"].split("\n") if "\t" in l for c in l.split("\t")[1:]]
            assert set(cells) <= {"0", str(R)} and str(R) in cells
            assert (windows is not None) == ("--win_size" in extra or "--win_bp" in extra)
            assert windows is None or len(windows.split("\n")) == n_set + 2
            assert "\tboot_stats: true\n\tboot_ci: %f\n" % (0.5 if "--boot_ci" in extra else 0.95) in err
    # the echo of the arguments has the two lines only with the flag
    out = str(tmp_path / "plain.dist")
    r = subprocess.run([san_bin, "--geno", gl, "--probs", "--n_ind", str(n_ind), "--n_sites", str(n_sites), "--out", out, "--verbose", "1"],
                       capture_output=True, timeout=300)
    assert r.returncode == 0 and "boot_stats" not in r.stderr.decode() and "boot_ci" not in r.stderr.decode()


def test_refusals_by_message_and_exit_status(san_bin, san_bin_plain, tmp_path, data):
    gl, groups, n_ind, n_sites = data
    base = ["--geno", gl, "--probs", "--n_ind", n_ind, "--n_sites", n_sites]
    boot = ["--n_boot_rep", 3, "--boot_block_size", 10]
    err = run(san_bin, tmp_path, base + boot + ["--boot_stats", "--n_gpus", 2], ok=False)
    assert "ERROR: [" in err and "--boot_stats" in err and "--n_gpus 1" in err
    err = run(san_bin, tmp_path, base + ["--boot_stats"], ok=False)
    assert "--boot_stats" in err and "require bootstrap replicates" in err
    err = run(san_bin, tmp_path, base + ["--boot_stats", "--win_size", 40], ok=False)
    assert "require bootstrap replicates" in err
    for ci in ("0", "1", "-0.2", "1.5", "nan"):
        err = run(san_bin, tmp_path, base + boot + ["--boot_stats", "--boot_ci", ci], ok=False)
        assert "--boot_ci" in err and "between 0 and 1" in err, ci
    assert "requires bootstrap summaries" in run(san_bin, tmp_path, base + boot + ["--boot_ci", 0.9], ok=False)
    # R above the cap
    err = run(san_bin, tmp_path, base + ["--n_boot_rep", 1280, "--boot_block_size", 10, "--boot_stats"], ok=False)
    assert "too many bootstrap replicates" in err and "--boot_stats" in err
    err = run(san_bin, tmp_path, base + ["--win_size", 40, "--win_boot_rep", 1280, "--boot_stats"], ok=False)
    assert "too many bootstrap replicates" in err
    # a data set that goes through the device in ranges of sites (the budget of test_host_groups_cpu.py: 40 of the 120 sites)
    budget = 256 * 128 * 128 * 8 + 36 * 64 + (512 << 20) + (24 * 128 + 40) * 40
    err = run(san_bin, tmp_path, base + boot + ["--boot_stats", "--max_device_bytes", budget], ok=False)
    assert "--boot_stats" in err and "one GPU" in err
    # fewer sites than one block: no replicate visits a site
    err = run(san_bin, tmp_path, base + ["--n_boot_rep", 2, "--boot_block_size", 500, "--boot_stats"], ok=False)
    assert "at least one bootstrap block" in err
    # an engine without the entry points
    assert "no bootstrap summaries (--boot_stats)" in run(san_bin_plain, tmp_path, base + boot + ["--boot_stats"], ok=False)
