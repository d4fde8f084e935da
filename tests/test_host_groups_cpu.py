"""The host's --groups path under AddressSanitizer + UBSan on the CPU: the stand-alone binary of test_host_sanitize_cpu.py,
linked against the stub engine plus tests/host_sanitize/stub_groups.cpp -- the group-mean entry points with no compute behind
them.  Checked: no sanitizer report, the shapes of the blocks of <out> and <out>.used, the error exits.  (What the numbers
are is the GPU suite's business: tests/test_gpu_cli_groups.py.)"""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ngsdist_amd", "csrc", "host", "ngsdist_host.cpp")
STUBS = os.path.join(ROOT, "tests", "host_sanitize")


def build(out, stubs):
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-pthread", "-o", out, HOST] + [os.path.join(STUBS, s) for s in stubs] + [
           os.path.join(ROOT, "ngsdist_amd", "csrc", "host_util.cpp"), "-I" + os.path.join(ROOT, "ngsdist_amd", "csrc"), "-lz"]
    r = subprocess.run(cmd, capture_output=True)
    if r.returncode != 0:
        err = r.stderr.decode()
        if "libasan" in err or "libubsan" in err or "unrecognized" in err and "fsanitize" in err:
            pytest.skip("no sanitizer runtime here: " + err[-300:])
        pytest.fail("the host does not build against the stub engine:\n" + err[-2000:])
    return out


@pytest.fixture(scope="module")
def san_bin(tmp_path_factory):
    return build(str(tmp_path_factory.mktemp("san") / "ngsDist_groups"), ["stub_engine.cpp", "stub_groups.cpp"])


@pytest.fixture(scope="module")
def san_bin_plain(tmp_path_factory):
    """the stub engine alone: the new entry points are weak references, the build links without them"""
    return build(str(tmp_path_factory.mktemp("san0") / "ngsDist_plain"), ["stub_engine.cpp"])


def run(binary, tmp_path, args, ok=True):
    out = str(tmp_path / "o.dist")
    for ext in ("", ".used", ".windows"):
        if os.path.exists(out + ext):
            os.remove(out + ext)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([binary] + [str(a) for a in args] + ["--out", out, "--verbose", "1"], capture_output=True, env=env, timeout=300)
    err = r.stderr.decode(errors="replace")
    assert "Sanitizer" not in err and "runtime error" not in err, err[-3000:]
    assert (r.returncode == 0) == ok, err[-1500:]
    if not ok:
        assert r.returncode == 255
        return err
    return open(out).read(), open(out + ".used").read()


def blocks(text, names):
    """the blocks of a file: each '' / 'G' / G rows of a name and G cells -> list of [G][G] cell strings"""
    lines = text.split("\n")
    G, per = len(names), len(names) + 2
    assert lines[-1] == "" and (len(lines) - 1) % per == 0, len(lines)
    out = []
    for k in range(0, len(lines) - 1, per):
        assert lines[k] == "" and lines[k + 1] == str(G)
        rows = [l.split("\t") for l in lines[k + 2:k + per]]
        assert [r[0] for r in rows] == names and all(len(r) == G + 1 for r in rows)
        out.append([r[1:] for r in rows])
    return out


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = tmp_path_factory.mktemp("data")
    n_ind, n_sites = 9, 120
    gl = str(d / "g.bin")
    np.random.default_rng(1).dirichlet([0.5, 0.5, 0.5], size=(n_sites, n_ind)).tofile(gl)
    groups = str(d / "groups.txt")
    # NA, - and an empty line: in no group; "solo" is a group of one; "north" comes back after "south"; a last line without '\n'
    lines = ["north\tx", "south", "NA", "north extra", "", "solo", "-", "south\ty", "north"]
    open(groups, "w").write("\n".join(lines))
    return gl, groups, n_ind, n_sites, ["north", "south", "solo"]


def test_groups_through_the_plain_run_the_bootstrap_and_the_windows(san_bin, tmp_path, data):
    gl, groups, n_ind, n_sites, names = data
    base = ["--geno", gl, "--probs", "--n_ind", n_ind, "--n_sites", n_sites, "--groups", groups]
    for extra, n_mat in (([], 1), (["--indep_geno", "--evol_model", 0, "--tot_sites", 500], 1),
                         (["--n_boot_rep", 3, "--boot_block_size", 10, "--seed", 5], 4),
                         (["--n_boot_rep", 70, "--boot_block_size", 7, "--indep_geno"], 71),  # (three engine calls)
                         (["--n_boot_rep", 2, "--boot_block_size", 500], 3),                  # (no block: nan / 0)
                         (["--win_size", 40, "--win_step", 20, "--pairwise_del"], 5),
                         (["--win_size", 40, "--win_step", 20, "--win_boot_rep", 2, "--boot_block_size", 7, "--seed", 3], 15),
                         (["--win_size", 5, "--win_step", 50, "--win_boot_rep", 2, "--boot_block_size", 7], 9)):
        txt, used = run(san_bin, tmp_path, base + extra)
        bm, bu = blocks(txt, names), blocks(used, names)
        assert len(bm) == len(bu) == n_mat, (extra, len(bm))
        for m, u in zip(bm, bu):
            for a in range(3):
                for b in range(3):
                    assert m[a][b] == m[b][a] and u[a][b] == u[b][a]  # symmetric
                    if u[a][b] == "0":
                        assert m[a][b] == "nan"
                    else:
                        assert int(u[a][b]) > 0 and len(m[a][b].split(".")[1]) == 10  # "%.10f"
            assert m[2][2] == "nan" and u[2][2] == "0"  # the group of one: no cell on its diagonal
        if "--boot_block_size" in extra and 500 in extra:
            assert all(c == "nan" for m in bm[1:] for r in m for c in r) and all(c == "0" for u in bu[1:] for r in u for c in r)
        wpath = str(tmp_path / "o.dist.windows")
        assert os.path.exists(wpath) == ("--win_size" in extra)
        if "--win_size" in extra:
            n_win = len(open(wpath).read().strip().split("\n")) - 1
            assert n_mat == n_win * (1 + (extra[extra.index("--win_boot_rep") + 1] if "--win_boot_rep" in extra else 0))


def test_groups_error_exits(san_bin, san_bin_plain, tmp_path, data):
    gl, groups, n_ind, n_sites, names = data
    base = ["--geno", gl, "--probs", "--n_ind", n_ind, "--n_sites", n_sites]
    short = str(tmp_path / "short.txt")
    open(short, "w").write("a\nb\n")
    assert "invalid GROUPS file!" in run(san_bin, tmp_path, base + ["--groups", short], ok=False)
    long_ = str(tmp_path / "long.txt")
    open(long_, "w").write("a\n" * (n_ind + 1))
    assert "invalid GROUPS file!" in run(san_bin, tmp_path, base + ["--groups", long_], ok=False)
    none = str(tmp_path / "none.txt")
    open(none, "w").write("NA\n" * n_ind)
    assert "invalid GROUPS file!" in run(san_bin, tmp_path, base + ["--groups", none], ok=False)
    assert "--n_gpus 1" in run(san_bin, tmp_path, base + ["--groups", groups, "--n_gpus", 2], ok=False)
    # a data set that goes through the device in ranges of sites
    # (the host's own estimate for 9 individuals on the EM path: 256 slab planes of 128 x 128 doubles + 64 bytes per pair +
    # 512 MiB fixed, 24 x 128 + 40 bytes per site -- a budget that holds 40 of the 120 sites)
    budget = 256 * 128 * 128 * 8 + 36 * 64 + (512 << 20) + (24 * 128 + 40) * 40
    err = run(san_bin, tmp_path, base + ["--groups", groups, "--max_device_bytes", budget], ok=False)
    assert "--groups" in err and "one GPU" in err
    assert "no group means (--groups)" in run(san_bin_plain, tmp_path, base + ["--groups", groups], ok=False)
    # ... and the plain stub still serves a run without the option
    out = str(tmp_path / "o.dist")
    r = subprocess.run([san_bin_plain] + [str(a) for a in base] + ["--out", out, "--verbose", "0"], capture_output=True, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr.decode(errors="replace")
