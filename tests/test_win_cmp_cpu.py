"""Comparison of windows on the host (ngd_win_cmp_host, ngd_win_cmp_finish, ngd_win_cmp_slice): the device form's twin and
the derived tables against the extended-precision expectation of win_cmp_expect.py on the shapes the GPU tests use, the
status rule, the NaN cases of cor, the power-of-two scaling bit for bit, symmetry by bits, and the exact zero of a
duplicate's rms.  No device is needed."""
import numpy as np
import pytest

import win_cmp_expect as X


def N():
    import ngsdist_amd
    return ngsdist_amd


@pytest.mark.parametrize("W", X.WS)
def test_host_twin_against_the_expectation(W):
    for P in X.P_of(W, N().win_cmp_slice):
        v, at = X.vectors(W, P)
        mean, gram, status = N().win_cmp_host(v)
        X.check_all(v, mean, gram, status, N().win_cmp_finish, "host")
        if "dup" in at:  # the same cells: the same bits, and an RMS difference of exactly 0
            _, rms = N().win_cmp_finish(mean, gram, status, P)
            assert rms[0, 1] == 0.0 and rms[1, 0] == 0.0
            assert X.bits(mean[:1])[0] == X.bits(mean[1:2])[0]
            assert gram[0, 0] == gram[0, 1] == gram[1, 1]


def test_the_slice_rule():
    sl = N().win_cmp_slice
    assert sl(0, 10) == 0 and sl(10, 0) == 0 and sl(N().win_cmp_max_vec() + 1, 10) == 0
    for W in (1, 16, 17, 64, 65, 397, 1000, 4000, N().win_cmp_max_vec()):
        for P in (1, 255, 256, 257, 4950, 499500, 10 ** 7):
            s = sl(W, P)
            assert s >= 256 and s % 4 == 0
            # (tile block, slice) jobs: enough of them for the device while the cell axis allows, and bounded partials
            n_g = (W + 15) // 16
            T = min(4, n_g)
            n_br = (n_g + T - 1) // T
            n_blk = n_br * (n_br + 1) // 2
            n_slices = (P + s - 1) // s
            assert n_slices * n_blk <= 4096 + n_blk
            if P >= 256 * 1024:
                assert n_slices * n_blk >= 1024
    assert sl(37, 499500) == 256 and sl(397, 499500) == 3424


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("where", [0, -1])
def test_a_cell_that_is_not_finite_leaves_its_vector_out_and_no_other(bad, where):
    W, P = 6, 301
    v, _ = X.vectors(W, P)
    v[W - 1] = v[0] + 0.5  # (the maker's own bad vector: finite here)
    clean = N().win_cmp_host(v)
    assert clean[2].tolist() == [1] * W
    w = v.copy()
    w[2, where] = bad
    mean, gram, status = N().win_cmp_host(w)
    assert status.tolist() == [1, 1, 0, 1, 1, 1]
    X.check_all(w, mean, gram, status, N().win_cmp_finish, "host, bad cell")
    keep = [0, 1, 3, 4, 5]
    assert np.array_equal(X.bits(gram[np.ix_(keep, keep)]), X.bits(clean[1][np.ix_(keep, keep)]))
    assert np.array_equal(X.bits(mean[keep]), X.bits(clean[0][keep]))


def test_the_nan_cases_of_cor():
    P = 100
    r = np.random.default_rng(3)
    v = np.stack([r.random(P), np.zeros(P), np.full(P, 0.125), np.full(P, -4.0), r.random(P)])
    mean, gram, status = N().win_cmp_host(v)
    assert status.tolist() == [1] * 5
    assert mean[1] == 0.0 and mean[2] == 0.125 and mean[3] == -4.0
    for k in (1, 2, 3):  # exact zeros: the whole row, the diagonal included
        assert np.all(gram[k] == 0.0) and np.all(gram[:, k] == 0.0)
    cor, rms = N().win_cmp_finish(mean, gram, status, P)
    for k in (1, 2, 3):
        assert np.all(np.isnan(cor[k])) and np.all(np.isnan(cor[:, k]))
    assert cor[0, 0] == 1.0 and cor[4, 4] == 1.0 and np.isfinite(cor[0, 4]) and cor[0, 4] == cor[4, 0]
    assert rms[1, 2] == 0.125 and rms[2, 3] == 4.125 and np.all(np.diag(rms) == 0.0)


@pytest.mark.parametrize("k", [-500, 300])
def test_cor_where_the_product_of_two_diagonals_leaves_the_normal_range(k):
    # cells near 2^k: each diagonal is near 4^k and finite, their product is not -- cor is the quotient all the same
    W, P = 9, 301
    v, _ = X.vectors(W, P)
    v[5], v[6] = np.ldexp(v[5], k), np.ldexp(v[6], k)
    mean, gram, status = N().win_cmp_host(v)
    assert np.all(np.isfinite(gram[:W - 1, :W - 1])) and gram[5, 5] > 0 and float(gram[5, 5]) * float(gram[6, 6]) in (0.0, np.inf)
    X.check_all(v, mean, gram, status, N().win_cmp_finish, "host, cells near 2^%d" % k)
    cor, _ = N().win_cmp_finish(mean, gram, status, P)
    assert abs(cor[5, 5] - 1.0) <= 4 * 2.0 ** -53 and abs(cor[5, 6]) < 1.0 and cor[5, 6] == cor[6, 5]


def test_scaling_by_a_power_of_two_is_exact():
    W, P = 9, 1031  # several slices of 256 cells
    v, _ = X.vectors(W, P)
    mean, gram, status = N().win_cmp_host(v)
    ok = status == 1
    for k in range(-40, 41):
        m2, g2, s2 = N().win_cmp_host(np.ldexp(v, k))
        assert np.array_equal(s2, status)
        assert np.array_equal(X.bits(m2[ok]), X.bits(np.ldexp(mean[ok], k))), k
        assert np.array_equal(X.bits(g2[np.ix_(ok, ok)]), X.bits(np.ldexp(gram[np.ix_(ok, ok)], 2 * k))), k


def test_position_and_company_change_no_bit():
    W, P = 12, 777
    v, _ = X.vectors(W, P)
    mean, gram, status = N().win_cmp_host(v)
    perm = np.random.default_rng(5).permutation(W)
    m2, g2, s2 = N().win_cmp_host(v[perm])
    assert np.array_equal(s2, status[perm]) and np.array_equal(X.bits(m2), X.bits(mean[perm]))
    assert np.array_equal(X.bits(g2), X.bits(gram[np.ix_(perm, perm)]))


def test_finish_and_host_refuse_what_the_header_says():
    import ctypes as C
    from ngsdist_amd import _lib
    L = _lib.load()
    dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint32)
    v = np.ones((2, 3))
    m, g, s = np.full(2, -7.0), np.full((2, 2), -7.0), np.full(2, 9, dtype=np.uint32)
    a = (v.ctypes.data_as(dp), m.ctypes.data_as(dp), g.ctypes.data_as(dp), s.ctypes.data_as(up))
    assert L.ngd_win_cmp_host(None, 2, 3, a[1], a[2], a[3]) == -1
    assert L.ngd_win_cmp_host(a[0], 0, 3, a[1], a[2], a[3]) == -1
    assert L.ngd_win_cmp_host(a[0], 2, 0, a[1], a[2], a[3]) == -1
    assert L.ngd_win_cmp_host(a[0], 2, 3, None, a[2], a[3]) == -1
    assert L.ngd_win_cmp_finish(a[1], a[2], a[3], 2, 0, a[2], a[2]) == -1
    assert L.ngd_win_cmp_finish(a[1], a[2], None, 2, 3, a[2], a[2]) == -1
    assert np.all(m == -7.0) and np.all(g == -7.0) and np.all(s == 9)
