"""The host's --win_cmp path under AddressSanitizer + UBSan on the CPU: the stand-alone binary of test_host_sanitize_cpu.py,
linked against the stub engine plus tests/host_sanitize/stub_win_cmp.cpp -- ngd_run_windows_cmp with no device behind it (its
outputs are ngd_win_cmp_host's on made-up distances, so the host twin and ngd_win_cmp_finish run under the sanitizers too).
Checked: no sanitizer report, the files and their shapes, every refusal by its message and exit status 255, and that the
plain stub alone links and refuses the flag.  (What the numbers are is the GPU suite's business: tests/test_gpu_cli_win_cmp.py.)"""
import os
import subprocess

import numpy as np
import pytest

from test_host_groups_cpu import build

EXTS = ("", ".windows", ".win_cor", ".win_rms", ".win_cmp", ".win_mds")


@pytest.fixture(scope="module")
def san_bin(tmp_path_factory):
    return build(str(tmp_path_factory.mktemp("san") / "ngsDist_win_cmp"), ["stub_engine.cpp", "stub_windows.cpp", "stub_win_cmp.cpp"])


@pytest.fixture(scope="module")
def san_bin_plain(tmp_path_factory):
    """the stub engine and its windows alone: the new entry point is a weak reference, the build links without it"""
    return build(str(tmp_path_factory.mktemp("san0") / "ngsDist_plain"), ["stub_engine.cpp", "stub_windows.cpp"])


def run(binary, tmp_path, args, ok=True, verbose=1):
    out = str(tmp_path / "o.dist")
    for ext in EXTS:
        if os.path.exists(out + ext):
            os.remove(out + ext)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([binary] + [str(a) for a in args] + ["--out", out, "--verbose", str(verbose)], capture_output=True, env=env,
                       timeout=300)
    err = r.stderr.decode(errors="replace")
    assert "Sanitizer" not in err and "runtime error" not in err, err[-3000:]
    assert (r.returncode == 0) == ok, err[-1500:]
    if not ok:
        assert r.returncode == 255
        return err
    return {ext: open(out + ext).read() if os.path.exists(out + ext) else None for ext in EXTS}, err


def table(text, W):
    lines = text.split("\n")
    assert lines[-1] == "" and len(lines) == W + 1
    t = np.array([l.split("\t") for l in lines[:-1]], dtype=float)
    assert t.shape == (W, W)
    return t


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = tmp_path_factory.mktemp("data")
    n_ind, n_sites = 9, 120
    gl = str(d / "g.bin")
    np.random.default_rng(1).dirichlet([0.5, 0.5, 0.5], size=(n_sites, n_ind)).tofile(gl)
    return gl, n_ind, n_sites


def test_the_files_and_their_shapes(san_bin, tmp_path, data):
    gl, n_ind, n_sites = data
    base = ["--geno", gl, "--probs", "--n_ind", n_ind, "--n_sites", n_sites]
    # (window arguments, windows, the windows left out)
    for win, W, bad in ((["--win_size", 40, "--win_step", 10], 9, [2]), (["--win_size", 30, "--win_step", 30], 4, []),
                        (["--win_size", 2, "--win_step", 50], 3, [0, 1, 2])):
        for K in (0, 2):
            if K and W - len(bad) < 3:
                continue
            files, err = run(san_bin, tmp_path, base + win + ["--win_cmp"] + (["--win_cmp_mds", K] if K else []))
            lines = files[""].split("\n")  # a block per window: an empty line, the number of individuals, a line each
            assert lines[-1] == "" and len(lines) - 1 == W * (n_ind + 2) and len(files[".windows"].strip().split("\n")) >= W
            cor, rms = table(files[".win_cor"], W), table(files[".win_rms"], W)
            keep = np.array([w not in bad for w in range(W)])
            assert np.all(np.isnan(cor[~keep])) and np.all(np.isnan(cor[:, ~keep])) and np.all(np.isnan(rms[~keep]))
            assert np.all(np.isfinite(rms[np.ix_(keep, keep)])) and np.all(np.diag(rms)[keep] == 0)
            assert np.allclose(np.diag(cor)[keep], 1.0) and np.array_equal(cor[np.ix_(keep, keep)], cor[np.ix_(keep, keep)].T)
            lines = files[".win_cmp"].split("\n")
            assert lines[0] == "window\tmean\tsd\tstatus" and lines[-1] == "" and len(lines) == W + 2
            for w, l in enumerate(lines[1:-1]):
                f = l.split("\t")
                assert len(f) == 4 and int(f[0]) == w and int(f[3]) == int(keep[w])
                assert np.isnan(float(f[1])) == (not keep[w]) and np.isnan(float(f[2])) == (not keep[w])
            assert ("WARNING: %d of the run's windows" % len(bad) in err) == bool(bad)
            assert "\twin_cmp: true\n" in err
            if not K:
                assert files[".win_mds"] is None
                continue
            text = files[".win_mds"]
            assert text.endswith("\n\n")
            rows = [l.split("\t") for l in text[:-2].split("\n")]
            assert len(rows) == W + 2 and rows[0][0] == "eig" and len(rows[0]) == K + 1 and rows[1][0] == "total" and len(rows[1]) == 3
            assert [r[0] for r in rows[2:]] == [str(w) for w in range(W)] and all(len(r) == K + 1 for r in rows[2:])
            xy = np.array([r[1:] for r in rows[2:]], dtype=float)
            eig = np.array(rows[0][1:], dtype=float)
            assert np.all(np.isnan(xy[~keep])) and np.all(np.isfinite(xy[keep])) and np.all(np.diff(eig) <= 0)
            assert np.allclose((xy[keep] ** 2).sum(axis=0), np.maximum(eig, 0), rtol=1e-8, atol=1e-12)
    # the echo of the arguments has the line only with the flag
    out = str(tmp_path / "plain.dist")
    r = subprocess.run([san_bin] + [str(a) for a in base] + ["--out", out, "--verbose", "1"], capture_output=True, timeout=300)
    assert r.returncode == 0 and "win_cmp" not in r.stderr.decode() and not os.path.exists(out + ".win_cmp")


def test_refusals_by_message_and_exit_status(san_bin, san_bin_plain, tmp_path, data):
    gl, n_ind, n_sites = data
    base = ["--geno", gl, "--probs", "--n_ind", n_ind, "--n_sites", n_sites]
    win = ["--win_size", 40, "--win_step", 10]
    groups = str(tmp_path / "groups.txt")
    open(groups, "w").write("\n".join(["a", "b", "a"] * 3))
    err = run(san_bin, tmp_path, base + ["--win_cmp"], ok=False)
    assert "ERROR: [" in err and "--win_cmp" in err and "requires windows" in err
    err = run(san_bin, tmp_path, base + win + ["--win_cmp", "--win_boot_rep", 2, "--boot_block_size", 7], ok=False)
    assert "--win_cmp" in err and "--win_boot_rep" in err
    err = run(san_bin, tmp_path, base + win + ["--win_cmp", "--groups", groups], ok=False)
    assert "--win_cmp" in err and "--groups" in err
    err = run(san_bin, tmp_path, base + win + ["--win_cmp", "--win_boot_rep", 2, "--boot_block_size", 7, "--boot_stats"], ok=False)
    assert "--win_cmp" in err
    err = run(san_bin, tmp_path, base + win + ["--win_cmp", "--boot_stats"], ok=False)
    assert "--boot_stats" in err
    err = run(san_bin, tmp_path, base + win + ["--win_cmp", "--nj"], ok=False)
    assert "--win_cmp" in err and "--nj" in err
    err = run(san_bin, tmp_path, base + win + ["--win_cmp", "--mds", 2], ok=False)
    assert "--win_cmp" in err and "--mds" in err
    err = run(san_bin, tmp_path, base + win + ["--win_cmp", "--n_gpus", 2], ok=False)
    assert "--n_gpus 1" in err
    err = run(san_bin, tmp_path, base + win + ["--win_cmp_mds", 2], ok=False)
    assert "--win_cmp_mds" in err and "requires their comparison (--win_cmp)" in err
    for K in (0, 17):
        err = run(san_bin, tmp_path, base + win + ["--win_cmp", "--win_cmp_mds", K], ok=False)
        assert "--win_cmp_mds K" in err and "between 1 and" in err
    err = run(san_bin, tmp_path, base + win + ["--win_cmp", "--win_cmp_mds", 8], ok=False)  # 8 windows kept: K <= 7
    assert "--win_cmp_mds K" in err and "between 1 and" in err
    for K in ("3x", "x", "-2", ""):
        err = run(san_bin, tmp_path, base + win + ["--win_cmp", "--win_cmp_mds", K], ok=False)
        assert "--win_cmp_mds K" in err and "whole number" in err, K
    # fewer than three windows kept
    err = run(san_bin, tmp_path, base + ["--win_size", 2, "--win_step", 50, "--win_cmp", "--win_cmp_mds", 1], ok=False)
    assert "three windows or more" in err
    # a data set that goes through the device in ranges of sites (the budget of test_host_groups_cpu.py: 40 of the 120 sites)
    budget = 256 * 128 * 128 * 8 + 36 * 64 + (512 << 20) + (24 * 128 + 40) * 40
    err = run(san_bin, tmp_path, base + win + ["--win_cmp", "--max_device_bytes", budget], ok=False)
    assert "one GPU" in err
    # an engine without the entry point
    assert "no comparison of windows (--win_cmp): not linked" in run(san_bin_plain, tmp_path, base + win + ["--win_cmp"], ok=False)
