"""The host's --mds path under AddressSanitizer + UBSan on the CPU: the stand-alone binary of test_host_sanitize_cpu.py,
linked against the stub engine plus tests/host_sanitize/stub_mds.cpp -- the MDS entry points with no device behind them
(their outputs are ngd_mds_host's on made-up distances, so the host twin runs under the sanitizers too).  Checked: no
sanitizer report, the files of each run form and the shape of their blocks -- also where NGSDIST_WIN_GROUP_MAX cuts 7 windows
of unequal length into engine calls of 3, 3 and 1 --, and every refusal by its message and exit status 255.  (What the coordinates are is the GPU suite's business: tests/test_gpu_cli_mds.py.)"""
import os
import subprocess

import numpy as np
import pytest

from test_host_groups_cpu import build
from test_host_nj_cpu import GROUP_MAX, same_shapes, seven_windows

EXTS = ("", ".mds", ".windows")


@pytest.fixture(scope="module")
def san_bin(tmp_path_factory):
    return build(str(tmp_path_factory.mktemp("san") / "ngsDist_mds"), ["stub_engine.cpp", "stub_mds.cpp"])


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


def mds_blocks(text, n, K):
    """the blocks of <out>.mds: [(eig [K], total [2], labels, coordinates [n][K])]"""
    assert text.endswith("\n\n")
    out = []
    for b in text[:-2].split("\n\n"):
        lines = [l.split("\t") for l in b.split("\n")]
        assert len(lines) == n + 2 and lines[0][0] == "eig" and len(lines[0]) == K + 1 and lines[1][0] == "total" and len(lines[1]) == 3
        assert all(len(l) == K + 1 for l in lines[2:])
        out.append((np.array(lines[0][1:], dtype=float), np.array(lines[1][1:], dtype=float), [l[0] for l in lines[2:]],
                    np.array([l[1:] for l in lines[2:]], dtype=float)))
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
        blocks = mds_blocks(files[".mds"], n_ind, K)
        assert len(blocks) == n_set * (R + 1), extra
        bad = [b for b in blocks if np.isnan(b[0]).any()]
        assert len(bad) == short * R
        for eig, tot, names, xy in blocks:
            assert names == [("name%d" if "--labels" in extra else "Ind_%d") % k for k in range(n_ind)]
            if np.isnan(eig).any():
                assert np.isnan(eig).all() and np.isnan(tot).all() and np.isnan(xy).all()
                continue
            assert np.all(np.diff(eig) <= 0) and tot[1] >= tot[0] and tot[1] >= eig[eig > 0].sum() * (1 - 1e-9)
            # the coordinates' squared lengths are the positive eigenvalues (unit vectors, at the printed precision)
            assert np.allclose((xy ** 2).sum(axis=0), np.maximum(eig, 0), rtol=1e-8, atol=1e-12)
        assert (files[".windows"] is not None) == ("--win_size" in extra or "--win_bp" in extra)
        assert "\tmds: 3\n" in err
        assert ("WARNING: %d of the run's matrices" % (short * R) in err) == (short > 0)
    # the echo of the arguments has the line only with the flag
    out = str(tmp_path / "plain.dist")
    r = subprocess.run([san_bin, "--geno", gl, "--probs", "--n_ind", str(n_ind), "--n_sites", str(n_sites), "--out", out, "--verbose", "1"],
                       capture_output=True, timeout=300)
    assert r.returncode == 0 and "mds:" not in r.stderr.decode() and not os.path.exists(out + ".mds")


def test_refusals_by_message_and_exit_status(san_bin, san_bin_plain, tmp_path, data):
    gl, labels, n_ind, n_sites = data
    base = ["--geno", gl, "--probs", "--n_ind", n_ind, "--n_sites", n_sites]
    boot = ["--n_boot_rep", 3, "--boot_block_size", 10]
    groups = str(tmp_path / "groups.txt")
    open(groups, "w").write("\n".join(["a", "b", "a"] * 3))
    err = run(san_bin, tmp_path, base + ["--mds", 2, "--groups", groups], ok=False)
    assert "ERROR: [" in err and "--mds" in err and "--groups" in err
    err = run(san_bin, tmp_path, base + boot + ["--mds", 2, "--boot_stats"], ok=False)
    assert "--mds" in err and "--boot_stats" in err
    err = run(san_bin, tmp_path, base + ["--mds", 2, "--nj"], ok=False)
    assert "--mds" in err and "--nj" in err
    err = run(san_bin, tmp_path, base + ["--mds", 2, "--n_gpus", 2], ok=False)
    assert "--mds" in err and "--n_gpus 1" in err
    for K in (0, n_ind, 17):
        err = run(san_bin, tmp_path, base + ["--mds", K], ok=False)
        assert "--mds K" in err and "between 1 and" in err
    for K in ("3x", "x", "-2", ""):
        err = run(san_bin, tmp_path, base + ["--mds", K], ok=False)
        assert "--mds K" in err and "whole number" in err, K
    # fewer than three individuals
    gl2 = str(tmp_path / "g2.bin")
    np.random.default_rng(2).dirichlet([0.5, 0.5, 0.5], size=(n_sites, 2)).tofile(gl2)
    err = run(san_bin, tmp_path, ["--geno", gl2, "--probs", "--n_ind", 2, "--n_sites", n_sites, "--mds", 1], ok=False)
    assert "--mds" in err and "three individuals" in err
    # a data set that goes through the device in ranges of sites (the budget of test_host_groups_cpu.py: 40 of the 120 sites)
    budget = 256 * 128 * 128 * 8 + 36 * 64 + (512 << 20) + (24 * 128 + 40) * 40
    err = run(san_bin, tmp_path, base + ["--mds", 2, "--max_device_bytes", budget], ok=False)
    assert "--mds" in err and "one GPU" in err
    # fewer sites than one block: no replicate visits a site
    err = run(san_bin, tmp_path, base + ["--n_boot_rep", 2, "--boot_block_size", 500, "--mds", 2], ok=False)
    assert "at least one bootstrap block" in err
    # an engine without the entry points
    assert "no classical MDS (--mds)" in run(san_bin_plain, tmp_path, base + ["--mds", 2], ok=False)
