"""ngd_em2_site (host_util.cpp): the host's restatement of the reference's single-site em2() that the engine's
NGD_OPT_EM_EXACT recheck decides stopping steps with -- iteration count and every bit of sfs equal to the reference's own
compiled em2() (oracle.ref_em2, where oracle/_ref is built; the recorded results of tests/golden/ref_em2 and the oracle's
restatement, which test_oracle_golden.py pins to the same bits, everywhere).  No GPU involved."""
import ctypes as C
import hashlib
import json
import os
import re

import numpy as np
import pytest

from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_EM2 = os.path.join(os.path.dirname(__file__), "golden", "ref_em2")


@pytest.fixture(scope="module")
def N():
    os.environ.setdefault("NGD_NO_TORCH", "1")
    import ngsdist_amd
    return ngsdist_amd


def same_bits(x, y):
    return x.tobytes() == y.tobytes() or (np.isnan(x).all() and np.isnan(y).all())  # (0 / 0: NaN in every cell)


def check(N, g1, g2):
    """em2_site against the reference's em2 on one pair of likelihood triples; returns the step count"""
    sfs, n = N.em2_site(g1, g2)
    port, n_or = O.em2(g1, g2)
    if O.ref_lib() is not None:
        assert same_bits(sfs, O.ref_em2(g1, g2)), (g1, g2, sfs)
    assert same_bits(sfs, port), (g1, g2, sfs, port)
    assert n == n_or, (g1, g2, n, n_or)
    return n


def test_em2_site_on_20000_random_pairs(N):
    # the inputs tests/golden/ref_em2/em2_batch.json records the reference's results on
    rng = np.random.default_rng(7)
    n = 20000
    a = rng.dirichlet([0.5] * 3, size=n)
    b = rng.dirichlet([0.3] * 3, size=n)
    a[:4] = [[1, 0, 0], [1 / 3, 1 / 3, 1 / 3], [0, 0, 1], [1e-300, 1 - 1e-12, 1e-12]]
    b[:4] = [[0, 0, 1], [1 / 3, 1 / 3, 1 / 3], [0, 0, 1], [0.5, 0.5, 0]]
    rec = json.load(open(os.path.join(REF_EM2, "em2_batch.json")))
    assert rec["n"] == n and hashlib.sha256(a.tobytes() + b.tobytes()).hexdigest() == rec["inputs_sha256"]
    got = np.empty((n, 9))
    iters = np.empty(n, dtype=np.int64)
    for k in range(n):
        got[k], iters[k] = N.em2_site(a[k], b[k])
    assert hashlib.sha256(got.tobytes()).hexdigest() == rec["reference_output_sha256"]  # every bit of 20 000 x 9
    if O.ref_lib() is not None:  # ... and live, the reference's own compiled em2()
        ref = np.empty((n, 9))
        dp = C.POINTER(C.c_double)
        O.ref_lib().ref_em2_batch(n, a.ctypes.data_as(dp), b.ctypes.data_as(dp), ref.ctypes.data_as(dp))
        assert got.tobytes() == ref.tobytes()
    n_or = np.array([O.em2(a[k], b[k])[1] for k in range(n)])
    assert np.array_equal(iters, n_or)
    assert iters.min() >= 1 and iters.max() <= 50 and len(set(iters.tolist())) > 20  # (many different step counts)


def norm(v):
    v = np.asarray(v, dtype=np.float64)
    return v / v.sum()


def find_boundary(g1, g2_of, lo, hi):
    """adjacent doubles a < b with different oracle iteration counts (as tests/test_gpu_em_boundary.py)"""
    a, b = lo, hi
    na, nb = O.em2(g1, g2_of(a))[1], O.em2(g1, g2_of(b))[1]
    assert na != nb
    while np.nextafter(a, b) < b:
        m = 0.5 * (a + b)
        if O.em2(g1, g2_of(m))[1] == na:
            a = m
        else:
            b, nb = m, O.em2(g1, g2_of(m))[1]
    return a, b, na, nb


CASES = [  # stopping steps around 3, 18 and 34: the first, second and third table round of the device kernel
    (norm([0.90, 0.08, 0.02]), lambda x: norm([x, 0.10, 0.05]), (0.5, 3.0)),
    (norm([0.6, 0.3, 0.1]), lambda x: norm([x, 0.25, 0.15]), (0.30, 0.60)),
    (norm([0.3503, 0.3315, 0.3182]), lambda x: norm([x, 0.3305, 0.3124]), (0.352, 0.40)),
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_em2_site_at_the_stopping_rules_boundary(N, case):
    g1, g2_of, (lo, hi) = CASES[case]
    a, b, na, nb = find_boundary(g1, g2_of, lo, hi)
    ulp = np.spacing(a)
    steps = {check(N, g1, g2_of(a + k * ulp)) for k in range(-64, 65)}
    assert steps == {na, nb}  # both sides of the boundary were visited


def test_em2_site_on_degenerate_inputs(N):
    third = [1 / 3, 1 / 3, 1 / 3]
    rows = [
        ([0.0, 0.5, 0.5], [0.2, 0.3, 0.5]),          # a zero likelihood
        ([0.0, 0.0, 1.0], [0.0, 1.0, 0.0]),          # called genotypes that disagree
        ([1.0, 0.0, 0.0], [1.0, 0.0, 0.0]),
        (third, third),                              # all three equal
        (third, [0.7, 0.2, 0.1]),
        ([0.25, 0.25, 0.25], [0.25, 0.25, 0.25]),
        ([1e-300, 1e-300, 1e-300], [0.3, 0.3, 0.4]),  # values of 1e-300
        ([1e-300, 1.0, 1e-300], [1e-300, 1e-300, 1.0]),
        ([0.0, 0.0, 0.0], [0.3, 0.3, 0.4]),          # an all-zero individual: 0 / 0 in normalize(), NaN as on the CPU
    ]
    with np.errstate(all="ignore"):
        for g1, g2 in rows:
            check(N, np.array(g1), np.array(g2))
    sfs, n = N.em2_site(third, third)
    assert n == 1 and np.allclose(sfs, 1 / 9)


def test_options_and_prototypes_are_present(N):
    from ngsdist_amd import _lib, engine
    txt = open(os.path.join(ROOT, "include", "ngsdist_amd.h")).read()
    assert re.search(r"#define NGD_OPT_EM_EXACT 15\b", txt) and re.search(r"#define NGD_OPT_EM_EXACT_CAP 16\b", txt)
    assert engine.OPTIONS["em_exact"] == 15 and engine.OPTIONS["em_exact_cap"] == 16
    decl = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    L = _lib.load()
    for name in ("ngd_last_em_exact", "ngd_em_exact_entries", "ngd_em2_site"):
        assert re.search(r"\b%s\s*\(" % name, decl), name
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert "ngd_em_exact_info" in decl and "ngd_em_exact_entry" in decl
    assert C.sizeof(_lib.NgdEmExactInfo) == 32 and C.sizeof(_lib.NgdEmExactEntry) == 40
    assert engine.EM_EXACT_ENTRY.itemsize == 40
    assert L.ngd_abi_version() == 6
    for m in ("last_em_exact", "em_exact_entries"):
        assert hasattr(N.Engine, m)
