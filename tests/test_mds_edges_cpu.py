"""Classical MDS on the host twin (ngd_mds_host) where test_mds_cpu.py's matrices do not go: matrices of few distinct rows
(mds_expect.duplicates: a window with one or two variable sites, clones -- B of rank 1 to 3 and the eigenvalue 0 about n
times over), pairs of eigenvalues 1e-4 .. 1e-13 and 0 apart (mds_expect.near_degenerate: the shift rule and Gram-Schmidt
inside a cluster, checked by subspace), cells times a power of two, and the matrix that is tridiagonal as it stands.

Bounds: the project's, 1e-9 relative to S = max |eigenvalue| for eigenvalues, residuals and totals, 1e-9 for orthonormality
and the subspace figure.  Every case prints its largest figures in units of the bound.

The duplicates cases are why this file exists.  Before the reflector's norm was taken from a scaled row, the rounding
residue of such a B -- itself of low rank, so that every Householder step left a trailing block about eps times smaller
again -- reached squares below the normal range after a dozen steps; tau was then no longer 2 / v^T v, H not orthogonal, and
the vectors came back with max |V V^T - I| of (K = 4 / K = 16; K = 1 passed everywhere; contract 1e-9):
    n = 64   all below 1e-9
    n = 96   quarter 3.3e-7 / 1.7e-4, two sites 1.6e-10 / 3.4e-6
    n = 128  halves 5.6e-4 / 1.2e-3, quarter 3.2e-5 / 1.9e-3
    n = 130  quarter 4.3e-3 / 9.3e-2
    n = 256  quarter 6.8e-11 / 1.7e-4, prototypes - / 5.7e-5
    n = 257  halves 4.2e-9 / 1.8e-7, quarter 1.5e-9 / 6.8e-7, one site 3.6e-8 / 1.7e-3, prototypes 2.6e-7 / 4.5e-3
with eigenvalues, residuals and totals within 1.7e-14 S throughout: 9 of the 18 cases of test_duplicates_against_numpy
failed (every n but 64 at K = 16, n = 96, 128, 130, 257 at K = 4).  The cells times 2^k gave other bits in eig, tot and vec
on most duplicates matrices: the residue met the end of the normal range at another step.  Scaling the row alone mended
orthonormality, eig and tot, not the bits of vec; a row tail no larger than eps^2 max|B| is therefore left alone, which ends
the residue's descent at the same step whatever the scale.
Now, over this file, as fractions of S (of 1 for orthonormality and the subspace figure): duplicates -- eigenvalues 1.5e-14,
residuals 1.7e-14, totals 1.5e-14 of the sum of |eigenvalue|, orthonormality 7.3e-15, 1 - |v . numpy's v| 3.6e-15 --;
near-degenerate -- eigenvalues against the planted ones 1.4e-15, against numpy's 1.2e-15, residuals 2.4e-15, totals
1.6e-15, orthonormality 1.9e-15, the subspace figure 6.7e-16 --; scaling changes no bit."""
import os

import numpy as np
import pytest

import mds_expect as X


@pytest.fixture(scope="module")
def N():
    os.environ.setdefault("NGD_NO_TORCH", "1")
    import ngsdist_amd
    return ngsdist_amd


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def check_duplicates(v, n, K, got, who):
    """every matrix of duplicates(n) by check_matrix; prints and returns the largest figure of each kind"""
    eig, vec, tot, status = got
    assert eig.shape == (X.N_DUP, K) and vec.shape == (X.N_DUP, K, n) and tot.shape == (X.N_DUP, 2)
    assert status.tolist() == [1] * X.N_DUP
    worst, failed = {}, []
    for name, m in X.DUP.items():
        try:
            fig = X.check_matrix(v[m], n, K, eig[m], vec[m], tot[m], sign=True)
        except AssertionError as err:
            failed.append("%s: %s" % (name, err))
            continue
        for kind, x in fig.items():
            worst[kind] = max(worst.get(kind, 0.0), x)
    print("%s duplicates n=%d K=%d: largest figures in units of 1e-9%s: %s" %
          (who, n, K, " (of the matrices that pass)" if failed else "", {k: "%.3g" % x for k, x in worst.items()}))
    assert not failed, "; ".join(failed)
    return worst


def check_near_degenerate(v, n, gap, K, got, who):
    """one matrix of near_degenerate(n, gap): check_matrix, the planted eigenvalues, the two pairs as subspaces"""
    eig, vec, tot, status = got
    assert status == 1
    fig = X.check_matrix(v, n, K, eig, vec, tot, sign=True)
    fig["planted"] = X.check_planted_spectrum(v, n, gap, eig)
    fig["subspace"] = max(X.check_subspace(v, n, vec, [0, 1]), X.check_subspace(v, n, vec, [2, 3]))
    print("%s near-degenerate n=%d gap=%g: largest figures in units of 1e-9: %s" % (who, n, gap, {k: "%.3g" % x for k, x in fig.items()}))
    return fig


def check_exact(n, K, got):
    """the points (1, -1, 0, ..): the eigenvalue 2 with the vector (1, -1, 0, ..) / sqrt 2, every other eigenvalue 0"""
    eig, vec, tot, status = got
    assert status == 1
    assert abs(eig[0] - 2.0) <= X.TOL * 2.0 and np.all(np.abs(eig[1:]) <= X.TOL * 2.0)
    want = np.zeros(n)
    want[:2] = np.sqrt(0.5)
    assert np.abs(np.abs(vec[0]) - want).max() <= X.TOL
    assert abs(tot[0] - 2.0) <= X.TOL * 2.0 and abs(tot[1] - 2.0) <= X.TOL * 2.0


def scaled_cases(n):
    """(name, matrices) whose cells test_scaling multiplies by powers of two"""
    return [("random", X.matrices(n)[:3]), ("duplicates", X.duplicates(n)),
            ("near-degenerate", np.stack([X.near_degenerate(n, gap) for gap in X.GAPS]))]


SCALES = [-40, -7, 9, 40]


def check_scaled(base, got, k, what):
    """cells times 2^k: eig and tot times 4^k and the same vec, bit for bit (every operation of the method commutes with a
    power of two while nothing leaves the normal range)"""
    f = 4.0 ** k
    assert np.array_equal(got[3], base[3]), what
    assert np.array_equal(bits(got[0]), bits(base[0] * f)), what + ": eig"
    assert np.array_equal(bits(got[2]), bits(base[2] * f)), what + ": tot"
    assert np.array_equal(bits(got[1]), bits(base[1])), what + ": vec"


@pytest.mark.parametrize("K", [1, 4, 16])
@pytest.mark.parametrize("n", [64, 96, 128, 130, 256, 257])
def test_duplicates_against_numpy(N, n, K):
    v = X.duplicates(n)
    check_duplicates(v, n, K, N.mds_host(v, n, K), "host")


@pytest.mark.parametrize("n", [5, 64, 65, 257])
def test_near_degenerate_pairs_by_planted_eigenvalues_and_subspaces(N, n):
    K = 4  # (n - 1 at n = 5)
    for gap in X.GAPS:
        v = X.near_degenerate(n, gap)
        eig, vec, tot, status = N.mds_host(v, n, K)
        check_near_degenerate(v, n, gap, K, (eig, vec, tot, status), "host")


@pytest.mark.parametrize("n", [5, 64, 130, 257])
def test_cells_times_a_power_of_two_change_no_bit(N, n):
    for name, v in scaled_cases(n):
        for K in sorted({min(4, n - 1), min(16, n - 1)}):
            base = N.mds_host(v, n, K)
            for k in SCALES:
                check_scaled(base, N.mds_host(v * 2.0 ** k, n, K), k, "%s n=%d K=%d k=%d" % (name, n, K, k))


@pytest.mark.parametrize("n", [4, 64, 128])
def test_a_matrix_that_is_tridiagonal_as_it_stands(N, n):
    """n a power of two: every cell of B exact, every step the H = I arm, every reflector skipped on the way back"""
    v = X.duplicates(n)[X.DUP["exact"]]
    B = X.centred(v, n)
    want = np.zeros((n, n))
    want[:2, :2] = [[1.0, -1.0], [-1.0, 1.0]]
    assert np.array_equal(B, want)
    for K in sorted({1, min(4, n - 1), min(16, n - 1)}):
        check_exact(n, K, N.mds_host(v, n, K))
