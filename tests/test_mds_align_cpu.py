"""Alignment of MDS replicates, the part that needs no device (include/ngsdist_amd.h "Classical MDS", alignment): the new
names in the header, the binding list and the library; ngd_mds_align_host against numpy's SVD (mds_align_expect.py) on
planted sets X_r = X_0 R_r + 1e-2 noise at n = 3, 4, 5, 64, 65, 257, K = 1, 2, min(n - 1, 16), R = 1, 2, 33; without
noise; where M is singular; status 0; scaling by 2^+-40; the refusals.

Bounds: Y within 1e-9 max(|X_0|, |X_r|) of numpy's where sigma_min(M) >= 1e-3 sigma_max(M) (asserted of every planted
replicate); fit within 1e-9 (|X_r|^2 + |X_0|^2) of |X_r|^2 + |X_0|^2 - 2 SUM sigma; |Q Q^T - I| <= 1e-9.  Every case prints
its largest figures in units of the bound; the largest seen over this file: Y 5.3e-15 of max |X|, fit 1.5e-15 of the
squared norms, orthogonality 1.9e-14; without noise |Y - X_0| 7.0e-16 of max |X| and fit 5.1e-31 |X_0|^2.

Between those two extremes, against mpmath at 60 digits (mds_align_expect.procrustes_mp), at (n, K) = (5, 3), (17, 7), (17, 16),
(65, 15), (65, 16) with R = 3: graded sets -- X_0's columns scaled by geomspace(1, g, K), g = 1e-1, 1e-3, 1e-5, replicates
that differ by a generic rotation, by signs, by turns inside pairs of axes -- and clustered ones (equal scales, X_r = X_0 R_r
+ eps Gaussian, eps = 1e-6, 1e-10, 1e-14) by the same three bounds, Y included although sigma_min(M) / sigma_max(M) goes down
to 1e-10 (every replicate's ratio is asserted by mpmath's sigma to lie within a decade of g^2); the floor band g = 1e-6,
1e-7 (ratios about 1e-12 and 1e-14, where a column may or may not be replaced) by fit, orthogonality, finiteness and the
same bits again, Y against nothing.  The largest seen over these cases: graded Y 1.6e-15 of max |X|, fit 2.1e-17 of the
squared norms, orthogonality 9.9e-14; clustered Y 2.0e-15, fit 1.1e-21, orthogonality 1.1e-14; floor band fit 2.0e-12 of
the squared norms, orthogonality 6.5e-16.  Sign flips, by bits, where no column is replaced (planted and graded
sets): the signs of the replicates' columns change nothing, those of X_0's columns D give Y D and the same fit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mds_align_expect as A
import mds_expect as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["ngd_mds_align_host", "ngd_mds_align_values_device", "ngd_run_job_mds_align", "ngd_run_windows_job_var_mds_align",
       "ngd_last_mds_align_ms"]
SIZES = [3, 4, 5, 64, 65, 257]
REPS = [1, 2, 33]


@pytest.fixture(scope="module")
def N():
    os.environ.setdefault("NGD_NO_TORCH", "1")
    import ngsdist_amd
    return ngsdist_amd


def align(N, Xp, status=None):
    """a planted set [n_mat][n][K] through the twin: (the coordinates the library saw [n_mat][n][K], aligned, fit)"""
    eig, vec = A.eigvec_of(Xp)
    aligned, fit = N.mds_align_host(eig, vec, status)
    return N.mds_coords(eig, vec), aligned, fit


def show(who, worst):
    print("%s: largest figures in units of 1e-9: %s" % (who, {k: "%.3g" % x for k, x in worst.items()}))


def test_header_binding_list_and_library_declare_the_new_names(N):
    from ngsdist_amd import _lib
    txt = open(os.path.join(ROOT, "include", "ngsdist_amd.h")).read()
    decl = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    L = _lib.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, decl), name + " is not declared in the header"
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert "No translation step" in txt and "No scaling step" in txt
    assert L.ngd_abi_version() == 6
    assert callable(N.mds_align_host)
    for name in ("mds_align_values", "run_job_mds_align", "run_windows_job_var_mds_align", "last_mds_align_ms"):
        assert callable(getattr(N.Engine, name))


@pytest.mark.parametrize("n", SIZES)
def test_host_twin_on_planted_sets(N, n):
    for K in A.dims(n):
        for R in REPS:
            Xs, aligned, fit = align(N, A.planted(n, K, R, seed=R))
            assert aligned.shape == (R + 1, K, n) and fit.shape == (R + 1,)
            show("host n=%d K=%d R=%d" % (n, K, R), A.check_set(Xs, aligned, fit))


@pytest.mark.parametrize("n", SIZES)
def test_without_noise_the_replicates_land_on_matrix_0(N, n):
    for K in A.dims(n):
        Xs, aligned, fit = align(N, A.planted(n, K, 5, seed=9, noise=0.0))
        A.check_set(Xs, aligned, fit)
        scale = np.abs(Xs).max()
        x = np.abs(A.nk(aligned[1:]) - Xs[0]).max() / (A.TOL * scale)
        f = fit[1:].max() / (1e-18 * (Xs[0] ** 2).sum())
        print("n=%d K=%d: |Y - X_0| %.3g of 1e-9 max|X|, fit %.3g of 1e-18 |X_0|^2" % (n, K, x, f))
        assert x <= 1 and f <= 1


def singular_sets(N, n, K):
    """(name, set [n_mat][n][K]) where M = X_r^T X_0 is singular"""
    base = A.planted(n, K, 3, seed=21)
    a = base.copy()
    a[1:, :, -1] = 0.0
    b = base.copy()
    b[0, :, -1] = 0.0
    c = base.copy()
    c[0] = 0.0
    d = np.zeros_like(base)
    return [("last column of X_r zero", a), ("last column of X_0 zero", b), ("X_0 zero", c), ("everything zero", d)]


@pytest.mark.parametrize("n", [3, 5, 65])
def test_singular_cases_keep_what_the_contract_pins(N, n):
    for K in A.dims(n):
        for name, Xp in singular_sets(N, n, K):
            Xs, aligned, fit = align(N, Xp)
            show("%s, n=%d K=%d" % (name, n, K), A.check_set(Xs, aligned, fit, regular=False))
            again = align(N, Xp)
            assert np.array_equal(A.bits(aligned), A.bits(again[1])) and np.array_equal(A.bits(fit), A.bits(again[2]))
            # a set's bits do not depend on its neighbours in the call
            eig, vec = A.eigvec_of(np.stack([A.planted(n, K, 3, seed=5), Xp]))
            both = N.mds_align_host(eig, vec)
            assert np.array_equal(A.bits(both[0][1]), A.bits(aligned)) and np.array_equal(A.bits(both[1][1]), A.bits(fit))


@pytest.mark.parametrize("n", [3, 4, 5, 64])
def test_all_equal_matrix_at_full_rank_through_mds_host(N, n):
    K = min(n - 1, 16)
    v = np.full((4, n * (n - 1) // 2), 0.25)
    eig, vec, tot, status = N.mds_host(v, n, K)
    aligned, fit = N.mds_align_host(eig, vec, status)
    Xs = N.mds_coords(eig, vec)
    show("all-equal n=%d K=%d" % (n, K), A.check_set(Xs, aligned, fit, regular=False, status=status))
    again = N.mds_align_host(eig, vec, status)
    assert np.array_equal(A.bits(aligned), A.bits(again[0])) and np.array_equal(A.bits(fit), A.bits(again[1]))


def test_status_0_in_a_replicate_and_in_matrix_0(N):
    n, K, R = 65, 4, 5
    Xp = np.stack([A.planted(n, K, R, seed=s) for s in range(3)])
    eig, vec = A.eigvec_of(Xp)
    status = np.ones((3, R + 1), dtype=np.uint32)
    status[0, 2] = 0   # a replicate
    status[1, 0] = 0   # matrix 0: the whole set is left out
    aligned, fit = N.mds_align_host(eig, vec, status)
    Xs = N.mds_coords(eig, vec)
    for s in range(3):
        A.check_set(Xs[s], aligned[s], fit[s], status=status[s])
    # the matrices that stay carry the bits they have without the ones left out
    plain = N.mds_align_host(eig, vec)
    keep = status.astype(bool) & status[:, :1].astype(bool)
    assert np.array_equal(A.bits(aligned[keep]), A.bits(plain[0][keep])) and np.array_equal(A.bits(fit[keep]), A.bits(plain[1][keep]))


@pytest.mark.parametrize("k", [40, -40])
def test_scaling_by_a_power_of_two_scales_the_result_exactly(N, k):
    for n, K in ((5, 4), (65, 16), (64, 2)):
        sets = [A.planted(n, K, 3, seed=2)] + [x for _, x in singular_sets(N, n, K)]
        for Xp in sets:
            eig, vec = A.eigvec_of(Xp)
            aligned, fit = N.mds_align_host(eig, vec)
            big = N.mds_align_host(eig * 4.0 ** k, vec)
            assert np.array_equal(A.bits(big[0]), A.bits(aligned * 2.0 ** k))
            assert np.array_equal(A.bits(big[1]), A.bits(fit * 4.0 ** k))


# ---- between well separated and singular: graded and clustered spectra against mpmath -------------------------------------
CASES = [(5, 3), (17, 7), (17, 16), (65, 15), (65, 16)]
GRADES = [1e-1, 1e-3, 1e-5]   # sigma_min / sigma_max of M about 1e-2, 1e-6, 1e-10
FLOOR = [1e-6, 1e-7]          # ... about 1e-12 and 1e-14: the band where a column is, or is not, replaced
NEAR = [1e-6, 1e-10, 1e-14]
SEED = 3


def show_mp(who, band, worst):
    print("%s, sigma_min/sigma_max in [%.0e, %.0e): largest figures in units of 1e-9 against mpmath: %s" %
          (who, band[0], band[1], {k: "%.3g" % x for k, x in worst.items()}))


@pytest.mark.parametrize("mode", A.MODES)
@pytest.mark.parametrize("n,K", CASES)
def test_host_twin_on_graded_sets_against_mpmath(N, n, K, mode):
    for g in GRADES:
        Xs, aligned, fit = align(N, A.graded(n, K, 3, g, SEED, mode))
        show_mp("host graded %s n=%d K=%d g=%.0e" % (mode, n, K, g), A.band_of(g), A.check_set_mp(Xs, aligned, fit, A.band_of(g)))


@pytest.mark.parametrize("n,K", CASES)
def test_host_twin_on_clustered_sets_against_mpmath(N, n, K):
    for eps in NEAR:
        Xs, aligned, fit = align(N, A.clustered(n, K, 3, eps, SEED))
        show_mp("host clustered n=%d K=%d eps=%.0e" % (n, K, eps), A.CLUSTERED_BAND,
                A.check_set_mp(Xs, aligned, fit, A.CLUSTERED_BAND))


@pytest.mark.parametrize("mode", A.MODES)
@pytest.mark.parametrize("n,K", CASES)
def test_host_twin_in_the_floor_band_keeps_what_the_contract_pins(N, n, K, mode):
    """a column may or may not be replaced here: fit, orthogonality, finiteness and the same bits again -- Y against nothing"""
    for g in FLOOR:
        Xp = A.graded(n, K, 3, g, SEED, mode)
        Xs, aligned, fit = align(N, Xp)
        show_mp("host floor %s n=%d K=%d g=%.0e" % (mode, n, K, g), A.band_of(g),
                A.check_set_mp(Xs, aligned, fit, A.band_of(g), y=False))
        again = align(N, Xp)
        assert np.array_equal(A.bits(aligned), A.bits(again[1])) and np.array_equal(A.bits(fit), A.bits(again[2]))


def flip_cases(n, K):
    """(name, set) where no column is replaced: a planted set and the graded ones down to sigma_min / sigma_max = 1e-10"""
    return [("planted", A.planted(n, K, 3, seed=SEED))] + [("graded %s g=%.0e" % (mode, g), A.graded(n, K, 3, g, SEED, mode))
                                                           for mode in A.MODES for g in GRADES]


def flips(K, seed):
    """K signs, not all equal (K >= 2)"""
    d = np.random.default_rng(400 + seed).choice([-1.0, 1.0], size=K)
    d[0], d[-1] = -1.0, 1.0
    return d


@pytest.mark.parametrize("n,K", CASES)
def test_sign_flips_change_no_bit_but_the_signs(N, n, K):
    """the signs of the replicates' columns do not matter at all; those of X_0's columns come out in Y as they went in"""
    for name, Xp in flip_cases(n, K):
        eig, vec = A.eigvec_of(Xp)
        aligned, fit = N.mds_align_host(eig, vec)
        d = flips(K, K)
        v = vec.copy()
        v[1:] *= d[:, None]
        got = N.mds_align_host(eig, v)
        assert np.array_equal(A.bits(got[0][1:]), A.bits(aligned[1:])) and np.array_equal(A.bits(got[1]), A.bits(fit)), name
        v = vec.copy()
        v[0] *= d[:, None]
        got = N.mds_align_host(eig, v)
        assert np.array_equal(A.bits(got[0]), A.bits(aligned * d[:, None])) and np.array_equal(A.bits(got[1]), A.bits(fit)), name


def test_refusals(N):
    from ngsdist_amd import _lib
    L = _lib.load()
    dp, u32p = C.POINTER(C.c_double), C.POINTER(C.c_uint32)
    n, K, n_mat = 5, 2, 3
    eig, vec = A.eigvec_of(A.planted(n, K, n_mat - 1, seed=1))
    al = np.full((n_mat, K, n), 7.0)
    fit = np.full(n_mat, 7.0)
    p = lambda a: a.ctypes.data_as(dp)
    ok = (p(eig), p(vec), None, 1, n_mat, n, K, p(al), p(fit))

    def call(**kw):
        names = ["eig", "vec", "status", "n_set", "n_mat", "n_ind", "K", "aligned", "fit"]
        args = list(ok)
        for k_, v in kw.items():
            args[names.index(k_)] = v
        return L.ngd_mds_align_host(*args)

    for bad in (dict(eig=None), dict(vec=None), dict(aligned=None), dict(fit=None), dict(n_set=0), dict(n_mat=0), dict(n_ind=2),
                dict(K=0), dict(K=n), dict(n_ind=40, K=17)):
        assert call(**bad) == -1, bad
        assert np.all(al == 7.0) and np.all(fit == 7.0)
    assert call() == 0 and not np.any(al == 7.0)
    with pytest.raises(ValueError):
        N.mds_align_host(eig, vec[:, :1])
    with pytest.raises(ValueError):
        N.mds_align_host(eig, vec, np.ones(n_mat + 1, dtype=np.uint32))
    assert X.TOL == A.TOL
