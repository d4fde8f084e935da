"""Windows along the genome on the CPU: the window list (ngd_window_ranges, host_util.cpp) against the rule it implements,
the host's argument checks for --win_size / --win_step, and the host's windowed path under AddressSanitizer + UBSan built
against the stub engine (tests/host_sanitize) -- with the stub of the windowed entry point and without it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "ngsdist_amd", "bin", "ngsDist")
HOST = os.path.join(ROOT, "ngsdist_amd", "csrc", "host", "ngsdist_host.cpp")
SAN = os.path.join(ROOT, "tests", "host_sanitize")
T_GL = os.path.join(ROOT, "tests", "golden", "survey_probe", "t_gl.bin")
NGD_E_INVALID = -1


def lib():
    from ngsdist_amd import _lib
    return _lib.load()


def rule(n_sites, size, step, chrom=None):
    """the definition: per chromosome (a maximal run of equal ids) [c0 + k step, c0 + k step + size) inside it"""
    ids = [0] * n_sites if chrom is None else list(chrom)
    out, c0 = [], 0
    while c0 < n_sites:
        c1 = c0
        while c1 < n_sites and ids[c1] == ids[c0]:
            c1 += 1
        out += [(s, s + size) for s in range(c0, c1 - size + 1, step)]
        c0 = c1
    return out


def ranges(n_sites, size, step, chrom=None):
    L = lib()
    ids = None if chrom is None else np.ascontiguousarray(chrom, dtype=np.uint32)
    idp = None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_uint32))
    n = L.ngd_window_ranges(idp, n_sites, size, step, None, None, 0)
    if n < 0:
        return n
    lo, hi = np.zeros(n + 3, dtype=np.uint64), np.zeros(n + 3, dtype=np.uint64)
    m = L.ngd_window_ranges(idp, n_sites, size, step, lo.ctypes.data_as(C.POINTER(C.c_uint64)),
                            hi.ctypes.data_as(C.POINTER(C.c_uint64)), n)
    assert m == n and not lo[n:].any() and not hi[n:].any()  # (nothing written past the cap)
    return list(zip(lo[:n].tolist(), hi[:n].tolist()))


@pytest.mark.parametrize("size,step", [(1, 1), (3, 1), (5, 5), (7, 3), (4, 9), (10, 10), (13, 2), (100, 1)])
def test_window_list_follows_the_rule(size, step):
    rng = np.random.default_rng(size * 31 + step)
    lens = [1, 4, 5, 17, 9, 30, 2, 13]  # chromosomes of uneven length, some shorter than a window
    chrom = np.repeat(np.arange(len(lens)) * 7 + 3, lens)
    n = int(chrom.size)
    assert ranges(n, size, step) == rule(n, size, step)
    assert ranges(n, size, step, chrom) == rule(n, size, step, chrom)
    for _ in range(5):
        k = int(rng.integers(1, 6))
        ids = np.repeat(rng.permutation(50)[:k], rng.integers(1, 20, size=k))
        assert ranges(ids.size, size, step, ids) == rule(ids.size, size, step, ids)


def test_window_list_edge_cases():
    assert ranges(10, 11, 1) == [] and ranges(10, 10, 3) == [(0, 10)]
    assert ranges(10, 4, 100) == [(0, 4)]  # a step past the end: one window per chromosome
    assert ranges(6, 3, 3, [1, 1, 1, 2, 2, 2]) == [(0, 3), (3, 6)]
    assert ranges(6, 4, 1, [1, 1, 1, 2, 2, 2]) == []  # no chromosome holds a window
    assert ranges(10, 0, 1) == NGD_E_INVALID and ranges(10, 1, 0) == NGD_E_INVALID
    assert ranges(5, 1, 1, [1, 1, 2, 2, 1]) == NGD_E_INVALID  # a chromosome that comes back
    assert ranges(5, 1, 1, [1, 1, 2, 2, 3]) == [(k, k + 1) for k in range(5)]


def test_python_window_ranges_uses_the_same_list():
    import ngsdist_amd as N
    chrom = ["c1"] * 7 + ["c2"] * 12 + ["c10"] * 3
    lo, hi = N.window_ranges(len(chrom), 4, 3, chrom=chrom)
    assert list(zip(lo.tolist(), hi.tolist())) == rule(len(chrom), 4, 3, [c for c in chrom])
    lo, hi = N.window_ranges(10, 4)
    assert lo.tolist() == [0, 4] and hi.tolist() == [4, 8]
    with pytest.raises(N.NgdError):
        N.window_ranges(4, 1, 1, chrom=["a", "b", "a", "a"])
    with pytest.raises(N.NgdError):
        N.window_ranges(4, 0)


@pytest.mark.skipif(not os.path.exists(BIN), reason="host binary not built")
@pytest.mark.parametrize("extra,msg", [
    (["--win_size", "0"], "window size (--win_size) cannot be less than 1!"),
    (["--win_size", "10", "--win_step", "0"], "window step (--win_step) cannot be less than 1!"),
    (["--win_step", "10"], "window step (--win_step) requires a window size (--win_size)!"),
    (["--win_size", "10", "--n_boot_rep", "3"], "windows (--win_size) cannot be combined with bootstrap replicates"),
    (["--win_size", "10", "--n_gpus", "2"], "windows (--win_size) are computed on one GPU (--n_gpus 1)!"),
    (["--win_size", "201"], "no window fits the data set"),
])
def test_host_argument_checks(tmp_path, extra, msg):
    r = subprocess.run([BIN, "--geno", T_GL, "--probs", "--n_ind", "6", "--n_sites", "200", "--out", str(tmp_path / "o"),
                        "--verbose", "0"] + extra, capture_output=True, text=True)
    assert r.returncode == 255 and msg in r.stderr, r.stderr


@pytest.mark.skipif(not os.path.exists(BIN), reason="host binary not built")
def test_host_refuses_a_positions_file_not_grouped_by_chromosome(tmp_path):
    pos = tmp_path / "p.tsv"
    pos.write_text("".join("%s\t%d\n" % ("ab"[(s // 50) % 2], s) for s in range(200)))
    r = subprocess.run([BIN, "--geno", T_GL, "--probs", "--n_ind", "6", "--n_sites", "200", "--out", str(tmp_path / "o"),
                        "--verbose", "0", "--pos", str(pos), "--win_size", "10"], capture_output=True, text=True)
    assert r.returncode == 255 and "positions file not grouped by chromosome!" in r.stderr


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


def test_host_windows_under_sanitizers(tmp_path):
    san = build(tmp_path, "ngsDist_win", [os.path.join(SAN, "stub_windows.cpp")])
    n_ind, n_sites = 5, 120
    rng = np.random.default_rng(2)
    gl = tmp_path / "g.bin"
    rng.dirichlet([0.5, 0.5, 0.5], size=(n_sites, n_ind)).tofile(str(gl))
    chrom = ["chr1"] * 50 + ["chr2"] * 45 + ["chr3"] * 25
    pos = tmp_path / "p.tsv"
    pos.write_text("chr\tpos\n" + "".join("%s\t%d\n" % (chrom[s], 10 * s + 5) for s in range(n_sites)))
    out = tmp_path / "w.dist"
    base = ["--geno", gl, "--probs", "--n_ind", n_ind, "--n_sites", n_sites, "--out", out, "--verbose", 1]
    for with_pos in (False, True):
        run_san(san, base + ["--win_size", 30, "--win_step", 20] + (["--posH", pos] if with_pos else []))
        want = rule(n_sites, 30, 20, chrom if with_pos else None)
        text = out.read_text()
        assert text.startswith("\n")
        blocks = text[1:].split("\n\n")  # ("\n<n_ind>\n" + rows, window after window)
        assert len(blocks) == len(want)
        for w, b in enumerate(blocks):
            lines = b.strip("\n").split("\n")
            assert lines[0] == str(n_ind) and len(lines) == n_ind + 1
            assert all(len(l.split("\t")) == n_ind + 1 for l in lines[1:])
            assert lines[1].split("\t")[2] == "%.10f" % (w + 0.0)  # (window w's first pair, from the stub)
        rows = (tmp_path / "w.dist.windows").read_text().strip("\n").split("\n")
        assert rows[0] == "window\tchr\tstart\tend\tfirst_site\tn_sites" and len(rows) == len(want) + 1
        for w, ((a, b), row) in enumerate(zip(want, rows[1:])):
            if with_pos:
                assert row == "%d\t%s\t%d\t%d\t%d\t30" % (w, chrom[a], 10 * a + 5, 10 * (b - 1) + 5, a)
            else:
                assert row == "%d\t.\t%d\t%d\t%d\t30" % (w, a + 1, b, a)
    # without the flags: no .windows file, nothing about windows in the argument echo
    (tmp_path / "w.dist.windows").unlink()
    err = run_san(san, base)
    assert not (tmp_path / "w.dist.windows").exists() and "win_" not in err


def test_host_without_the_windowed_entry_point_fails_cleanly(tmp_path):
    san = build(tmp_path, "ngsDist_nowin", [])
    gl = tmp_path / "g.bin"
    np.random.default_rng(3).dirichlet([0.5, 0.5, 0.5], size=(40, 3)).tofile(str(gl))
    base = ["--geno", gl, "--probs", "--n_ind", 3, "--n_sites", 40, "--out", tmp_path / "o.dist", "--verbose", 0]
    err = run_san(san, base + ["--win_size", 10], ok=False)
    assert "this build of the engine has no windows along the genome (--win_size)!" in err
    run_san(san, base)
