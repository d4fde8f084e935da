"""Windows in base pairs on the CPU: the window list in coordinates (ngd_window_ranges_bp, host_util.cpp) against a
brute-force restatement of its definition, the per-window block maps (ngd_window_boot_maps) against the oracle's generator
seeded anew per window, the host's argument checks for --win_bp / --win_bp_step / --win_min_sites, and the host's --win_bp
path under AddressSanitizer + UBSan built against the stub engine (tests/host_sanitize)."""
import ctypes as C
import os
import subprocess
import time

import numpy as np
import pytest

from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "ngsdist_amd", "bin", "ngsDist")
HOST = os.path.join(ROOT, "ngsdist_amd", "csrc", "host", "ngsdist_host.cpp")
SAN = os.path.join(ROOT, "tests", "host_sanitize")
T_GL = os.path.join(ROOT, "tests", "golden", "survey_probe", "t_gl.bin")
NGD_E_INVALID = -1
U64P = C.POINTER(C.c_uint64)


def lib():
    from ngsdist_amd import _lib
    return _lib.load()


def rule(pos, size, step, chrom=None, min_sites=1):
    """the definition, every window searched, no jumps: per chromosome window k covers [1 + k step, 1 + k step + size) for
    every k with 1 + k step <= the last position; kept with max(1, min_sites) sites or more -> (lo, hi, bp_start)"""
    n = len(pos)
    ids = [0] * n if chrom is None else list(chrom)
    out, c0 = [], 0
    while c0 < n:
        c1 = c0
        while c1 < n and ids[c1] == ids[c0]:
            c1 += 1
        k = 0
        while 1 + k * step <= pos[c1 - 1]:
            start = 1 + k * step
            inside = [s for s in range(c0, c1) if start <= pos[s] < start + size]
            if len(inside) >= max(1, min_sites):
                assert inside == list(range(inside[0], inside[-1] + 1))
                out.append((inside[0], inside[-1] + 1, start))
            k += 1
        c0 = c1
    return out


def ranges_bp(pos, size, step, chrom=None, min_sites=1, cap=None, null_pos=False):
    L = lib()
    p = np.ascontiguousarray(pos, dtype=np.uint64)
    ids = None if chrom is None else np.ascontiguousarray(chrom, dtype=np.uint32)
    idp = None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_uint32))
    pp = None if null_pos else p.ctypes.data_as(U64P)
    n = L.ngd_window_ranges_bp(idp, pp, p.size, size, step, min_sites, None, None, None, 0)
    if n < 0:
        return n
    cap = n if cap is None else cap
    lo, hi, st = (np.zeros(n + 3, dtype=np.uint64) for _ in range(3))
    m = L.ngd_window_ranges_bp(idp, pp, p.size, size, step, min_sites, lo.ctypes.data_as(U64P), hi.ctypes.data_as(U64P),
                               st.ctypes.data_as(U64P), cap)
    k = min(n, cap)
    assert m == n and not lo[k:].any() and not hi[k:].any() and not st[k:].any()  # (nothing written past the cap)
    # bp_start may be NULL
    lo2, hi2 = np.zeros(k, dtype=np.uint64), np.zeros(k, dtype=np.uint64)
    assert L.ngd_window_ranges_bp(idp, pp, p.size, size, step, min_sites, lo2.ctypes.data_as(U64P), hi2.ctypes.data_as(U64P), None, k) == n
    assert np.array_equal(lo2, lo[:k]) and np.array_equal(hi2, hi[:k])
    return list(zip(lo[:k].tolist(), hi[:k].tolist(), st[:k].tolist()))


@pytest.mark.parametrize("size,step", [(1, 1), (10, 3), (50, 50), (100, 30), (40, 90), (500, 7), (2000, 700)])
def test_window_list_follows_the_definition(size, step):
    rng = np.random.default_rng(size * 31 + step)
    for trial in range(6):
        lens = rng.integers(1, 40, size=int(rng.integers(1, 5)))
        chrom = np.repeat(rng.permutation(50)[:len(lens)], lens)
        # gaps of 0 give duplicate positions; a few large gaps give runs of empty windows
        pos = np.concatenate([np.cumsum(rng.integers(0, 25, n) * rng.choice([1, 1, 1, 20], n)) + 1 for n in lens])
        for min_sites in (0, 1, 2, 5):
            want = rule(pos.tolist(), size, step, chrom.tolist(), min_sites)
            assert ranges_bp(pos, size, step, chrom, min_sites) == want, (trial, min_sites)
            if trial == 0:
                assert ranges_bp(pos[:lens[0]], size, step, None, min_sites) == rule(pos[:lens[0]].tolist(), size, step, None, min_sites)
        got = ranges_bp(pos, size, step, chrom)
        assert all(l < h for l, h, _ in got) and all(a[0] <= b[0] for a, b in zip(got, got[1:]))  # what ngd_run_windows* wants


def test_window_list_edge_cases():
    assert ranges_bp([5], 10, 10) == [(0, 1, 1)]  # one site
    assert ranges_bp([5], 2, 2) == [(0, 1, 5)]
    assert ranges_bp([7, 7, 7], 3, 3) == [(0, 3, 7)]  # duplicate positions stay together
    # a site exactly on 1 + k T and on 1 + k T + B - 1: B = 10, T = 4 -- position 9 starts window 2 and ends window 0's reach at 10
    assert ranges_bp([9, 10], 10, 4) == rule([9, 10], 10, 4) == [(0, 2, 1), (0, 2, 5), (0, 2, 9)]
    assert ranges_bp([10, 11], 10, 10) == [(0, 1, 1), (1, 2, 11)]  # 10 is window 0's last coordinate, 11 window 1's first
    assert ranges_bp([1, 2, 3, 50], 10, 5, min_sites=2) == [(0, 3, 1)]  # min_sites filters, the kept ones are renumbered
    assert ranges_bp([1, 2, 3, 50], 10, 5, min_sites=0) == ranges_bp([1, 2, 3, 50], 10, 5, min_sites=1)
    full = ranges_bp([3, 9, 14, 30, 31], 10, 3)
    assert len(full) > 4 and ranges_bp([3, 9, 14, 30, 31], 10, 3, cap=4) == full[:4]  # cap smaller than the count
    assert ranges_bp([3, 9, 14, 30, 31], 10, 3, cap=0) == []
    # trailing partial windows are kept: the last window starts at or before the last position
    assert ranges_bp([1, 25], 10, 10)[-1] == (1, 2, 21)
    # chromosomes are counted apart, each from coordinate 1
    assert ranges_bp([5, 15, 5, 15], 10, 10, chrom=[1, 1, 2, 2]) == [(0, 1, 1), (1, 2, 11), (2, 3, 1), (3, 4, 11)]


def test_window_list_refusals():
    ok = [3, 9, 14]
    assert ranges_bp(ok, 0, 1) == NGD_E_INVALID and ranges_bp(ok, 1, 0) == NGD_E_INVALID
    assert ranges_bp(ok, 10, 10, null_pos=True) == NGD_E_INVALID
    assert ranges_bp([0, 9, 14], 10, 10) == NGD_E_INVALID  # a position of 0
    assert ranges_bp([3, 9, 1 << 62], 10, 10) == NGD_E_INVALID and ranges_bp(ok, 1 << 62, 10) == NGD_E_INVALID
    assert ranges_bp([3, 9, (1 << 62) - 1], (1 << 62) - 1, 1 << 63) == [(0, 3, 1)]  # ... the largest of both are served
    assert ranges_bp([3, 9, 8], 10, 10) == NGD_E_INVALID  # positions descend inside a chromosome
    assert ranges_bp([3, 9, 8], 10, 10, chrom=[1, 1, 2]) == [(0, 2, 1), (2, 3, 1)]  # ... not across two
    assert ranges_bp([3, 9, 9], 10, 10) == [(0, 3, 1)]  # equal positions are allowed
    assert ranges_bp([1, 2, 3, 4, 5], 1, 1, chrom=[1, 1, 2, 2, 1]) == NGD_E_INVALID  # a chromosome that comes back


def test_runs_of_empty_windows_are_jumped_over():
    """Two sites 10^15 apart, windows of 10 every 1: position 1 lies in window 0 alone (windows start at coordinate 1), position
    10^15 in the ten windows that start at 10^15 - 9 .. 10^15 -- 11 kept windows out of 10^15, at once.  (With the first site
    at 10 its ten windows 0 .. 9 are all there: 20.)"""
    t0 = time.time()
    got = ranges_bp([1, 10 ** 15], 10, 1)
    assert got == [(0, 1, 1)] + [(1, 2, 10 ** 15 - 9 + k) for k in range(10)]
    got = ranges_bp([10, 10 ** 15], 10, 1)
    assert got == [(0, 1, 1 + k) for k in range(10)] + [(1, 2, 10 ** 15 - 9 + k) for k in range(10)] and len(got) == 20
    # ... and windows that hold a site but too few are jumped over like empty ones
    assert ranges_bp([1, 10 ** 15, 10 ** 15 + 3], 10 ** 15 + 3, 1, min_sites=3) == [(0, 3, 1)]
    assert ranges_bp([1, 10 ** 15], 10 ** 15 - 5, 1, min_sites=2) == []  # 10^15 - 5 windows hold the last site alone
    ks = [k for k in range((10 ** 15 - 10) // 7, 10 ** 15 // 7 + 1) if 10 ** 15 - 9 <= 1 + 7 * k <= 10 ** 15]
    assert len(ks) >= 1 and ranges_bp([5, 10 ** 15, 10 ** 15], 10, 7, min_sites=2) == [(1, 3, 1 + 7 * k) for k in ks]
    assert time.time() - t0 < 1.0


def test_python_window_ranges_bp_uses_the_same_list():
    import ngsdist_amd as N
    pos = [3, 9, 14, 30, 31, 2, 8]
    chrom = ["c1"] * 5 + ["c2"] * 2
    lo, hi, st = N.window_ranges_bp(pos, 10, 3, chrom=chrom, min_sites=2)
    assert list(zip(lo.tolist(), hi.tolist(), st.tolist())) == rule(pos, 10, 3, chrom, 2)
    lo, hi, st = N.window_ranges_bp([5, 15], 10)  # step defaults to the size
    assert (lo.tolist(), hi.tolist(), st.tolist()) == ([0, 1], [1, 2], [1, 11])
    for bad in (dict(pos=[3, 2], size=10), dict(pos=[0, 2], size=10), dict(pos=[1, 2], size=0),
                dict(pos=[1, 2, 3], size=1, chrom=["a", "b", "a"])):
        with pytest.raises(N.NgdError):
            N.window_ranges_bp(**bad)


def boot_maps(seed, lo, hi, n_rep, q, cap=None):
    L = lib()
    lo, hi = np.ascontiguousarray(lo, dtype=np.uint64), np.ascontiguousarray(hi, dtype=np.uint64)
    off = np.full(lo.size, 77, dtype=np.uint64)
    n = L.ngd_window_boot_maps(seed, lo.ctypes.data_as(U64P), hi.ctypes.data_as(U64P), lo.size, n_rep, q, None, 0, off.ctypes.data_as(U64P))
    if n < 0:
        return n
    cap = n if cap is None else cap
    maps = np.full(n + 5, 12345, dtype=np.uint64)
    off2 = np.zeros(lo.size, dtype=np.uint64)
    assert L.ngd_window_boot_maps(seed, lo.ctypes.data_as(U64P), hi.ctypes.data_as(U64P), lo.size, n_rep, q, maps.ctypes.data_as(U64P),
                                  cap, off2.ctypes.data_as(U64P)) == n
    assert np.array_equal(off, off2) and np.all(maps[min(n, cap):] == 12345)  # (nothing is written beyond cap)
    return maps[:min(n, cap)], off, n


@pytest.mark.parametrize("q", [1, 7, 20])
@pytest.mark.parametrize("n_rep", [1, 5, 40])
def test_block_maps_are_those_of_the_cut_down_runs(q, n_rep):
    rng = np.random.default_rng(q * 100 + n_rep)
    lens = rng.integers(1, 110, 30)
    lens[[3, 9, 21]] = lens[0]  # windows of one length
    lens[5] = max(1, q - 1)     # shorter than one block (q > 1)
    lo = np.sort(rng.integers(0, 500, 30))
    hi = lo + lens
    maps, off, n = boot_maps(5, lo, hi, n_rep, q)
    nb = lens // q
    assert n == n_rep * sum(set(nb.tolist())) == len(maps)  # windows with one n_blocks share their maps
    for w in range(30):
        t = O.Taus(5)  # every cut-down run seeds its generator anew
        want = np.stack([t.block_map(int(nb[w])) for _ in range(n_rep)]) if nb[w] else np.zeros((n_rep, 0), dtype=np.uint64)
        assert np.array_equal(maps[int(off[w]):int(off[w]) + n_rep * int(nb[w])].reshape(n_rep, int(nb[w])), want), w
        if nb[w] == 0:
            assert off[w] == 0  # no entries
    assert off[3] == off[9] == off[21] == off[0]  # equal lengths share an offset
    # the classes lie one after the other in the order their first windows come, without gaps
    firsts = sorted({int(off[w]): int(nb[w]) for w in range(30) if nb[w]}.items())
    at = 0
    for o, b in firsts:
        assert o == at
        at += n_rep * b
    assert at == n
    # cap is honoured: a prefix, nothing beyond it
    for cap in (0, 1, n // 2, n - 1):
        part, off_c, n_c = boot_maps(5, lo, hi, n_rep, q, cap=cap)
        assert n_c == n and np.array_equal(part, maps[:cap]) and np.array_equal(off_c, off)


def test_block_maps_edge_cases():
    maps, off, n = boot_maps(1, [0, 10], [3, 12], 4, 5)  # every window shorter than a block
    assert n == 0 and len(maps) == 0 and not off.any()
    maps, off, n = boot_maps(1, [0, 10], [30, 42], 0, 5)  # no replicate
    assert n == 0 and not off.any()
    assert boot_maps(1, [0], [30], 3, 0) == NGD_E_INVALID  # block size 0
    assert boot_maps(1, [5], [4], 3, 2) == NGD_E_INVALID  # a window that ends before it starts
    # the same sequence ngd_boot_block_map gives for equal-length windows today
    import ngsdist_amd as N
    m, o = N.window_boot_maps(9, [0, 60, 120], [200, 260, 320], 6, 7)
    t = N.Taus(9)
    assert not o.any() and np.array_equal(m.reshape(6, 28), np.stack([t.block_map(28) for _ in range(6)]))


# ---- the host ----
def pos_file(path, pos, chrom, header=False):
    path.write_text(("chr\tpos\n" if header else "") + "".join("%s\t%s\n" % (c, p) for c, p in zip(chrom, pos)))
    return path


@pytest.mark.skipif(not os.path.exists(BIN), reason="host binary not built")
@pytest.mark.parametrize("extra,msg", [
    (["--win_bp", "100", "--win_size", "10"], "windows in base pairs (--win_bp) cannot be combined with windows in sites (--win_size)!"),
    (["--win_bp_step", "10"], "window step in base pairs (--win_bp_step) requires a window size in base pairs (--win_bp)!"),
    (["--win_min_sites", "2"], "minimum number of sites per window (--win_min_sites) requires a window size in base pairs (--win_bp)!"),
    (["--win_size", "10", "--win_bp_step", "10"], "(--win_bp_step) requires a window size in base pairs (--win_bp)!"),
    (["--win_bp", "100", "--NOPOS"], "windows in base pairs (--win_bp) require a positions file (--pos / --posH)!"),
    (["--win_bp", "0"], "window size in base pairs (--win_bp) cannot be less than 1!"),
    (["--win_bp", "-5"], "window size in base pairs (--win_bp) cannot be less than 1!"),
    (["--win_bp", "100", "--win_bp_step", "0"], "window step in base pairs (--win_bp_step) cannot be less than 1!"),
    (["--win_bp", "100", "--win_min_sites", "0"], "minimum number of sites per window (--win_min_sites) cannot be less than 1!"),
    (["--win_bp", "100", "--win_step", "5"], "window step (--win_step) requires a window size (--win_size)!"),
    # the windowed flow's own refusals, word for word
    (["--win_bp", "100", "--n_boot_rep", "3"], "windows (--win_size) cannot be combined with bootstrap replicates (--n_boot_rep)!"),
    (["--win_bp", "100", "--n_gpus", "2"], "windows (--win_size) are computed on one GPU (--n_gpus 1)!"),
    (["--win_bp", "100", "--win_boot_rep", "2", "--n_boot_rep", "3"],
     "bootstrap replicates inside windows (--win_boot_rep) cannot be combined with bootstrap replicates of the whole data set (--n_boot_rep)!"),
    (["--win_bp", "100", "--em_exact"], "the reference's EM stopping step (--em_exact) cannot be combined with windows (--win_size)!"),
    (["--win_bp", "100", "--em_exact_boot"], "the reference's EM stopping step (--em_exact_boot) cannot be combined with windows (--win_size)!"),
    (["--win_bp", "100", "--em_exact_win", "--win_boot_rep", "3"],
     "(--em_exact_win) serves plain windows in base pairs (--win_bp) only: not with --win_boot_rep!"),
    (["--win_bp", "100", "--win_min_sites", "500"], "no window is kept"),
    (["--win_bp", "100", "--max_device_bytes", "1000"], "windows (--win_size) need the whole data set on one GPU; it does not fit the device budget!"),
])
def test_host_argument_checks(tmp_path, extra, msg):
    pos = pos_file(tmp_path / "p.tsv", [3 * s + 1 for s in range(200)], ["c"] * 200)
    with_pos = ["--pos", str(pos)]
    if "--NOPOS" in extra:
        extra, with_pos = [x for x in extra if x != "--NOPOS"], []
    r = subprocess.run([BIN, "--geno", T_GL, "--probs", "--n_ind", "6", "--n_sites", "200", "--out", str(tmp_path / "o"),
                        "--verbose", "0"] + with_pos + extra, capture_output=True, text=True)
    if "device budget" in msg and "no HIP device" in r.stderr:
        return  # (that refusal needs a device to size the budget against: the GPU suite has it)
    assert r.returncode == 255 and msg in r.stderr, r.stderr


@pytest.mark.skipif(not os.path.exists(BIN), reason="host binary not built")
@pytest.mark.parametrize("bad,msg", [
    ("0", "need whole numbers from 1"), ("-4", "need whole numbers from 1"), ("12.5", "need whole numbers from 1"),
    ("1e3", "need whole numbers from 1"), (" 7", "need whole numbers from 1"), ("9999999999999999999", "need whole numbers from 1"),
    ("descend", "positions descend inside a chromosome"), ("ungrouped", "positions file not grouped by chromosome!"),
])
def test_host_refuses_positions_it_cannot_window(tmp_path, bad, msg):
    pos = [str(3 * s + 1) for s in range(200)]
    chrom = ["c"] * 200
    if bad == "descend":
        pos[100] = "5"
    elif bad == "ungrouped":
        chrom = ["ab"[(s // 50) % 2] for s in range(200)]
        pos = [str(3 * (s % 50) + 1) for s in range(200)]
    else:
        pos[100] = bad
    pf = pos_file(tmp_path / "p.tsv", pos, chrom)
    r = subprocess.run([BIN, "--geno", T_GL, "--probs", "--n_ind", "6", "--n_sites", "200", "--out", str(tmp_path / "o"),
                        "--verbose", "0", "--pos", str(pf), "--win_bp", "100"], capture_output=True, text=True)
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


def blocks_of(text, n_ind):
    assert text.startswith("\n")
    out = []
    for b in text[1:].split("\n\n"):
        lines = b.strip("\n").split("\n")
        assert lines[0] == str(n_ind) and len(lines) == n_ind + 1 and all(len(l.split("\t")) == n_ind + 1 for l in lines[1:])
        out.append(lines[1].split("\t")[2])  # the matrix's first pair
    return out


def test_host_windows_in_base_pairs_under_sanitizers(tmp_path):
    san = build(tmp_path, "ngsDist_bp", [os.path.join(SAN, x) for x in ("stub_windows.cpp", "stub_windows_job.cpp", "stub_windows_job_var.cpp")])
    n_ind, n_sites = 5, 120
    rng = np.random.default_rng(2)
    gl = tmp_path / "g.bin"
    rng.dirichlet([0.5, 0.5, 0.5], size=(n_sites, n_ind)).tofile(str(gl))
    chrom = ["chr1"] * 50 + ["chr2"] * 45 + ["chr3"] * 25
    gaps = rng.integers(1, 30, n_sites) * rng.choice([1, 1, 9], n_sites)
    pos = np.concatenate([np.cumsum(gaps[:50]), np.cumsum(gaps[50:95]), np.cumsum(gaps[95:])]).tolist()
    pf = pos_file(tmp_path / "p.tsv", pos, chrom, header=True)
    out = tmp_path / "w.dist"
    base = ["--geno", gl, "--probs", "--n_ind", n_ind, "--n_sites", n_sites, "--out", out, "--verbose", 1, "--posH", pf]
    B, T = 300, 110
    for min_sites in (1, 4):
        want = rule(pos, B, T, chrom, min_sites)
        assert len(set(b - a for a, b, _ in want)) > 3
        for R, q in ((0, 1), (3, 4)):
            err = run_san(san, base + ["--win_bp", B, "--win_bp_step", T, "--win_min_sites", min_sites] +
                          (["--win_boot_rep", R, "--boot_block_size", q, "--seed", 5] if R else []))
            assert "win_bp: 300" in err and "win_bp_step: 110" in err and "%d windows of 300 bp every 110 bp" % len(want) in err
            first = blocks_of(out.read_text(), n_ind)
            assert len(first) == len(want) * (R + 1)
            for w, (a, b, _) in enumerate(want):
                assert first[w * (R + 1)] == "%.10f" % w  # (window w's matrix 0, from the stub)
                for m in range(1, R + 1):  # its replicates follow it; 0 / 0 where the window has no block
                    assert first[w * (R + 1) + m] == ("%.10f" % (w + m / 100.0) if (b - a) // q else "nan"), (w, m)
            if R and min_sites == 1:
                assert any((b - a) // q == 0 for a, b, _ in want)
            rows = (tmp_path / "w.dist.windows").read_text().strip("\n").split("\n")
            assert rows[0] == "window\tchr\tstart\tend\tfirst_site\tn_sites\twin_start\twin_end" and len(rows) == len(want) + 1
            for w, ((a, b, st), row) in enumerate(zip(want, rows[1:])):
                assert row == "%d\t%s\t%d\t%d\t%d\t%d\t%d\t%d" % (w, chrom[a], pos[a], pos[b - 1], a, b - a, st, st + B - 1)
                assert st <= pos[a] and pos[b - 1] <= st + B - 1
    # --win_bp_step defaults to the size
    err = run_san(san, base + ["--win_bp", B])
    assert "%d windows of 300 bp every 300 bp" % len(rule(pos, B, B, chrom)) in err
    # the same positions file under --win_size: the .windows file is what it was, six columns
    run_san(san, base + ["--win_size", 30, "--win_step", 20])
    rows = (tmp_path / "w.dist.windows").read_text().strip("\n").split("\n")
    assert rows[0] == "window\tchr\tstart\tend\tfirst_site\tn_sites"
    k = 0
    for c0, c1 in ((0, 50), (50, 95), (95, 120)):
        for a in range(c0, c1 - 30 + 1, 20):
            k += 1
            assert rows[k] == "%d\t%s\t%d\t%d\t%d\t30" % (k - 1, chrom[a], pos[a], pos[a + 29], a)
    assert k == len(rows) - 1
    # ... and with --win_boot_rep there: the equal-length call, as before
    run_san(san, base + ["--win_size", 30, "--win_step", 20, "--win_boot_rep", 2, "--boot_block_size", 7, "--seed", 5])
    assert len(blocks_of(out.read_text(), n_ind)) == 3 * k


def test_host_without_the_unequal_length_entry_point_fails_cleanly(tmp_path):
    san = build(tmp_path, "ngsDist_novar", [os.path.join(SAN, x) for x in ("stub_windows.cpp", "stub_windows_job.cpp")])
    gl = tmp_path / "g.bin"
    np.random.default_rng(3).dirichlet([0.5, 0.5, 0.5], size=(40, 3)).tofile(str(gl))
    pf = pos_file(tmp_path / "p.tsv", [7 * s + 1 for s in range(40)], ["c"] * 40)
    base = ["--geno", gl, "--probs", "--n_ind", 3, "--n_sites", 40, "--out", tmp_path / "o.dist", "--verbose", 0, "--pos", pf]
    err = run_san(san, base + ["--win_bp", 70, "--win_boot_rep", 2], ok=False)
    assert "this build of the engine has no bootstrap replicates inside windows of unequal length (--win_bp with --win_boot_rep)!" in err
    run_san(san, base + ["--win_bp", 70])  # plain windows need ngd_run_windows_dist alone
