"""The k-group range walk of the single-image passes (ngsdist_amd/csrc/kg_ranges.h: the one-image engine's accumulation and the
two by-pass routes of the fix-up go through it) under AddressSanitizer + UBSan on the CPU, from a stand-alone program:
the ranges of whole slices and of a whole pass for a few thousand seeded cases, checked for what the launches rely on
and against a restatement of the loops the engine had before the walk was shared."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def walk_bin(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("kg") / "kg_ranges_san")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-o", out, os.path.join(ROOT, "tests", "kg_ranges", "kg_ranges_main.cpp"),
           "-I" + os.path.join(ROOT, "ngsdist_amd", "csrc")]
    r = subprocess.run(cmd, capture_output=True)
    if r.returncode != 0:
        err = r.stderr.decode()
        # only a missing sanitizer runtime is a reason to skip
        if "libasan" in err or "libubsan" in err or "unrecognized" in err and "fsanitize" in err:
            pytest.skip("no sanitizer runtime here: " + err[-300:])
        pytest.fail("the range walk does not build on its own:\n" + err[-2000:])
    return out


def cases(n, seed):
    """n_ks a multiple of 8 with fewer than 8 slices of padding; whole k-groups per slice (per_slice) or slices of k_per_slice
    contraction indices (a multiple of 3 that is no multiple of 4: the k-groups shared with a neighbour are masked)"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        n_real = int(rng.integers(1, 200))
        n_ks = (n_real + 7) // 8 * 8
        if rng.integers(2):
            per_slice, k_per = int(rng.choice([1, 3, 6, 24, 75, 750, 3000])), 0
            kg_lim = n_real * per_slice
        else:
            per_slice, k_per = 0, 3 * int(rng.choice([1, 2, 3, 6, 10, 25, 101, 1001]))
            kg_lim = (n_real * k_per + 3) // 4
        span = int(rng.choice([1, 7, 64, 300, 5000]))
        res = int(rng.choice([0, 0, rng.integers(1, kg_lim + 2)]))
        rest0 = int(rng.choice([0, rng.integers(0, kg_lim + 3)]))
        out.append((n_ks, per_slice, k_per, kg_lim, span, res, rest0))
    return out


def parent_walk(n_ks, per_slice, k_per, kg_lim, span, res, rest0):
    """the loops that the one-image pass (and, with res = 0 and rest0 = 0, each by-pass route of the fix-up) had of its own
    before kg_ranges.h, in the engine's unsigned 64-bit arithmetic"""
    kg0 = lambda ks: (ks * k_per) >> 2 if k_per else ks * per_slice
    kg1 = lambda ks: min(kg_lim, ((ks + 1) * k_per + 3) >> 2 if k_per else (ks + 1) * per_slice)
    first = 0
    if res:
        while first + 8 <= n_ks and kg1(first + 7) <= res and kg0(first + 7) < kg_lim:
            first += 8
    groups, ks0 = [], first
    while ks0 < n_ks:
        n = 8
        while ks0 + n < n_ks and ((kg1(ks0 + n + 7) - kg0(ks0)) & M64) <= span and kg0(ks0 + n) < kg_lim:
            n += 8
        n = min(n, n_ks - ks0)
        lo = min(kg0(ks0), kg_lim)
        groups.append((ks0, n, lo, max(lo, kg1(ks0 + n - 1))))
        ks0 += n
    ranges = []
    if kg_lim > rest0:
        L = kg_lim - rest0
        r = max(1, (L + span - 1) // span)
        piece = max(64, ((L + r * n_ks - 1) // (r * n_ks) + 3) // 4 * 4)
        for k in range(max(1, (L + piece * n_ks - 1) // (piece * n_ks))):
            lo = min(rest0 + k * piece * n_ks, kg_lim)
            ranges.append((lo, min(lo + piece * n_ks, kg_lim), piece))
    return first, groups, ranges


def test_ranges_of_whole_slices_and_of_a_whole_pass(walk_bin):
    cs = cases(4000, 20241018)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([walk_bin], input="".join(" ".join(map(str, c)) + "\n" for c in cs).encode(), capture_output=True, env=env,
                       timeout=300)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, err[-3000:]
    blocks = r.stdout.decode().split("E\n")
    assert len(blocks) == len(cs) + 1 and blocks[-1] == ""
    merged = 0
    for c, text in zip(cs, blocks):
        n_ks, per_slice, k_per, kg_lim, span, res, rest0 = c
        rows = [l.split() for l in text.splitlines()]
        first = [int(x[1]) for x in rows if x[0] == "F"]
        groups = [tuple(int(v) for v in x[1:]) for x in rows if x[0] == "G"]
        moved = [x[1:] for x in rows if x[0] == "M"]
        ranges = [tuple(int(v) for v in x[1:]) for x in rows if x[0] == "P"]
        assert len(first) == 1 and (first[0], groups, ranges) == parent_walk(*c), c
        first = first[0]
        kg0 = lambda ks: (ks * k_per) >> 2 if k_per else ks * per_slice
        kg1 = lambda ks: min(kg_lim, ((ks + 1) * k_per + 3) >> 2 if k_per else (ks + 1) * per_slice)
        # the slices in order, in eights: [0, first) read from the resident head, the rest range by range
        assert first % 8 == 0 and all(kg1(ks) <= res for ks in range(first)), c
        at = first
        for ks0, n, lo, hi in groups:
            assert ks0 == at and n > 0 and n % 8 == 0 and lo <= hi <= kg_lim, c
            for ks in range(ks0, ks0 + n):
                if kg0(ks) < kg_lim:
                    assert lo <= kg0(ks) and kg1(ks) <= hi, (c, ks)
            if n > 8:
                merged += 1
                assert hi - lo <= span, c
            at += n
        assert at == n_ks, c
        assert moved == [["1", "1"]] * len(groups), c
        # a whole pass: contiguous from rest0 to kg_lim, pieces of whole pipeline trips
        if kg_lim <= rest0:
            assert not ranges, c
        else:
            assert ranges[0][0] == rest0 and ranges[-1][1] == kg_lim, c
            for k, (lo, hi, piece) in enumerate(ranges):
                assert lo < hi <= lo + piece * n_ks and piece % 4 == 0 and piece >= 64, c
                assert k == 0 or lo == ranges[k - 1][1], c
    assert merged > 100  # (the cases do merge eights into longer ranges)
