"""Bootstrap replicates inside windows (--win_boot_rep) on the CPU: the host's argument checks, and the host's path under
AddressSanitizer + UBSan built against the stub engine (tests/host_sanitize) -- with the stub of the new entry point and
without it."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "ngsdist_amd", "bin", "ngsDist")
HOST = os.path.join(ROOT, "ngsdist_amd", "csrc", "host", "ngsdist_host.cpp")
SAN = os.path.join(ROOT, "tests", "host_sanitize")
T_GL = os.path.join(ROOT, "tests", "golden", "survey_probe", "t_gl.bin")


def test_the_package_exports_the_job_entry_points():
    from ngsdist_amd import _lib
    import ngsdist_amd as N
    L = _lib.load()
    for name in ("ngd_run_windows_job", "ngd_run_windows_job_device", "ngd_run_windows_job_dist"):
        assert hasattr(L, name)
    assert hasattr(N.Engine, "run_windows_job") and hasattr(N.Engine, "run_windows_job_dist")
    assert L.ngd_abi_version() == 6  # (added under 6, like the windowed calls)


@pytest.mark.parametrize("extra,msg", [
    (["--win_boot_rep", "3"], "bootstrap replicates inside windows (--win_boot_rep) require a window size (--win_size)!"),
    (["--win_size", "10", "--win_boot_rep", "3", "--n_boot_rep", "2"],
     "(--win_boot_rep) cannot be combined with bootstrap replicates of the whole data set (--n_boot_rep)!"),
    (["--win_boot_rep", "3", "--n_boot_rep", "2"], "(--win_boot_rep) require a window size (--win_size)!"),
    (["--win_size", "10", "--win_boot_rep", "3", "--boot_block_size", "0"], "bootstrap block size cannot be less than 1!"),
])
def test_host_argument_checks(tmp_path, extra, msg):
    assert os.path.exists(BIN), "host binary not built"
    r = subprocess.run([BIN, "--geno", T_GL, "--probs", "--n_ind", "6", "--n_sites", "200", "--out", str(tmp_path / "o"),
                        "--verbose", "0"] + extra, capture_output=True, text=True)
    assert r.returncode == 255 and msg in r.stderr, r.stderr


def build(tmp_path, name, extra_sources):
    out = str(tmp_path / name)
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-pthread", "-o", out, HOST, os.path.join(SAN, "stub_engine.cpp")] + extra_sources + \
          [os.path.join(ROOT, "ngsdist_amd", "csrc", "host_util.cpp"), "-I" + os.path.join(ROOT, "ngsdist_amd", "csrc"), "-lz"]
    r = subprocess.run(cmd, capture_output=True)
    if r.returncode != 0:
        err = r.stderr.decode()
        if "libasan" in err or "libubsan" in err or "unrecognized" in err and "fsanitize" in err:
            pytest.skip("no sanitizer runtime here: " + err[-300:])
        pytest.fail("the host does not build against the stub engine:\n" + err[-2000:])
    return out


def run_san(binary, args, ok=True):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([binary] + [str(a) for a in args], capture_output=True, env=env, timeout=300)
    err = r.stderr.decode(errors="replace")
    assert "Sanitizer" not in err and "runtime error" not in err, err[-3000:]
    assert (r.returncode == 0) == ok, err[-1500:]
    return err


def windows(n_sites, size, step, chrom=None):
    ids = [0] * n_sites if chrom is None else list(chrom)
    out, c0 = [], 0
    while c0 < n_sites:
        c1 = c0
        while c1 < n_sites and ids[c1] == ids[c0]:
            c1 += 1
        out += [(s, s + size) for s in range(c0, c1 - size + 1, step)]
        c0 = c1
    return out


def data(tmp_path, n_ind, n_sites, seed):
    gl = tmp_path / "g.bin"
    np.random.default_rng(seed).dirichlet([0.5, 0.5, 0.5], size=(n_sites, n_ind)).tofile(str(gl))
    return gl


def test_host_window_replicates_under_sanitizers(tmp_path):
    san = build(tmp_path, "ngsDist_wboot", [os.path.join(SAN, "stub_windows.cpp"), os.path.join(SAN, "stub_windows_job.cpp")])
    n_ind, n_sites, R = 5, 120, 3
    gl = data(tmp_path, n_ind, n_sites, 2)
    chrom = ["chr1"] * 50 + ["chr2"] * 45 + ["chr3"] * 25
    pos = tmp_path / "p.tsv"
    pos.write_text("chr\tpos\n" + "".join("%s\t%d\n" % (chrom[s], 10 * s + 5) for s in range(n_sites)))
    out = tmp_path / "w.dist"
    base = ["--geno", gl, "--probs", "--n_ind", n_ind, "--n_sites", n_sites, "--out", out, "--verbose", 1, "--seed", 5]
    for with_pos in (False, True):
        for q in (1, 7, 30):  # the default block size; blocks that leave a tail; one block per window
            err = run_san(san, base + ["--win_size", 30, "--win_step", 20, "--win_boot_rep", R, "--boot_block_size", q]
                          + (["--posH", pos] if with_pos else []))
            assert "win_boot_rep: %d" % R in err
            want = windows(n_sites, 30, 20, chrom if with_pos else None)
            text = out.read_text()
            assert text.startswith("\n")
            blocks = text[1:].split("\n\n")  # window-major: a window's R + 1 blocks, then the next window's
            assert len(blocks) == len(want) * (R + 1)
            for k, b in enumerate(blocks):
                lines = b.strip("\n").split("\n")
                assert lines[0] == str(n_ind) and len(lines) == n_ind + 1
                assert lines[1].split("\t")[2] == "%.10f" % (k // (R + 1) + (k % (R + 1)) / 100.0)  # (from the stub)
            rows = (tmp_path / "w.dist.windows").read_text().strip("\n").split("\n")
            assert rows[0] == "window\tchr\tstart\tend\tfirst_site\tn_sites" and len(rows) == len(want) + 1
    # a window shorter than one block: the replicates visit no site (ngsDist.cpp:236) and print 0 / 0, matrix 0 as ever
    run_san(san, base + ["--win_size", 30, "--win_step", 20, "--win_boot_rep", 2, "--boot_block_size", 31, "--evol_model", 0])
    blocks = out.read_text()[1:].split("\n\n")
    want = windows(n_sites, 30, 20)
    assert len(blocks) == len(want) * 3
    for k, b in enumerate(blocks):
        cell = b.strip("\n").split("\n")[1].split("\t")[2]
        assert (cell == "%.10f" % (k // 3)) if k % 3 == 0 else cell in ("nan", "-nan")
    # --win_boot_rep 0: the windows alone, nothing asked of the new entry point
    run_san(san, base + ["--win_size", 30, "--win_step", 20, "--win_boot_rep", 0])
    assert len(out.read_text()[1:].split("\n\n")) == len(want)


def test_host_without_the_new_entry_point_fails_cleanly(tmp_path):
    san = build(tmp_path, "ngsDist_nowboot", [os.path.join(SAN, "stub_windows.cpp")])
    gl = data(tmp_path, 3, 40, 3)
    base = ["--geno", gl, "--probs", "--n_ind", 3, "--n_sites", 40, "--out", tmp_path / "o.dist", "--verbose", 0]
    err = run_san(san, base + ["--win_size", 10, "--win_boot_rep", 2], ok=False)
    assert "this build of the engine has no bootstrap replicates inside windows (--win_boot_rep)!" in err
    run_san(san, base + ["--win_size", 10])
