"""Alignment of MDS replicates by numpy (include/ngsdist_amd.h "Classical MDS", alignment): orthogonal Procrustes by
numpy.linalg.svd, the planted sets the alignment tests share, and the contract's checks as functions.  Coordinates are
[n][K] here (numpy's way round); the library's arrays are [K][n]: kn() and nk() turn one into the other.  Every check
returns its figure in units of its bound, so that the tests can print it before they assert.

Where numpy's SVD is not exact enough to be the reference -- M graded over many orders of magnitude, numpy's own Y up to ten
times further from the exact one than the library's -- procrustes_mp() is: the same steps by mpmath at 60 digits, once per
input (a cache by the inputs' bytes: device, twin and numpy share one reference).  graded() and clustered() make such sets,
check_band() asserts where a case's sigma_min(M) / sigma_max(M) lies, check_y_mp() and check_fit_mp() are check_y() and
check_fit() against procrustes_mp()."""
import mpmath
import numpy as np

NAN_BITS = np.uint64(0x7FF8000000000000)
TOL = 1e-9   # the project's tolerance
SEP = 1e-3   # Y is compared with numpy's where sigma_min(M) >= SEP * sigma_max(M)
NOISE = 1e-2


def nk(a):
    """[..., K, n] -> [..., n, K]"""
    return np.ascontiguousarray(np.swapaxes(a, -1, -2))


kn = nk


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def dims(n):
    """the K of a size: 1, 2, min(n - 1, 16)"""
    return sorted({1, min(2, n - 1), min(n - 1, 16)})


def procrustes(Xr, X0):
    """(Y, fit, sigma) of the rotation of Xr [n][K] onto X0 by numpy's SVD"""
    U, s, Vt = np.linalg.svd(Xr.T @ X0)
    Y = Xr @ (U @ Vt)
    return Y, ((Y - X0) ** 2).sum(), s


def planted(n, K, R, seed, noise=NOISE):
    """a set of R + 1 configurations [R + 1][n][K]: X_0 has orthonormal centred columns scaled by 1 .. 0.25 (eigenvalues 1 ..
    1/16: lambda_K / lambda_1 >= 0.05), X_r = X_0 R_r + noise * Gaussian with R_r the orthogonal factor of a Gaussian K x K
    matrix (QR: reflections come as often as rotations)"""
    rng = np.random.default_rng(7000 + 131 * seed + 17 * n + K)
    G = rng.normal(size=(n, K))
    X0 = np.linalg.qr(G - G.mean(axis=0))[0] * np.linspace(1.0, 0.25, K)
    X = np.empty((R + 1, n, K))
    X[0] = X0
    for r in range(1, R + 1):
        Rr = np.linalg.qr(rng.normal(size=(K, K)))[0]
        X[r] = X0 @ Rr + noise * rng.normal(size=(n, K))
    return X


MP_DIGITS = 60
MODES = ("generic", "signs", "pairs")
_mp_cache = {}


def procrustes_mp(Xr, X0):
    """(Y, fit, sigma) of the rotation of Xr [n][K] onto X0 by mpmath at MP_DIGITS digits: M = Xr^T X0, svd_r, Q = U V^T, Y =
    Xr Q, fit the sum of the squared differences themselves; Y and sigma (descending) rounded to float64 at the end, fit
    too.  Computed once per input"""
    Xr, X0 = np.ascontiguousarray(Xr, dtype=np.float64), np.ascontiguousarray(X0, dtype=np.float64)
    key = (Xr.shape, Xr.tobytes(), X0.tobytes())
    if key not in _mp_cache:
        with mpmath.workdps(MP_DIGITS):
            A, B = mpmath.matrix(Xr.tolist()), mpmath.matrix(X0.tolist())
            U, S, V = mpmath.svd_r(A.T * B)
            Y = A * (U * V)
            D = Y - B
            fit = mpmath.fsum(d * d for d in D)
            out = (np.array(Y.tolist(), dtype=np.float64).reshape(Xr.shape), float(fit),
                   np.sort(np.array([float(x) for x in S]))[::-1])
        for a in (out[0], out[2]):
            a.setflags(write=False)
        _mp_cache[key] = out
    return _mp_cache[key]


def _centred_orthonormal(rng, n, K):
    G = rng.normal(size=(n, K))
    return np.linalg.qr(G - G.mean(axis=0))[0]


def graded(n, K, R, g, seed, mode):
    """a set [R + 1][n][K] whose M has singular values spread over about g^2: X_0 has orthonormal centred columns scaled by
    geomspace(1, g, K) (the coordinates' sqrt(lambda_k)), and X_r is, by `mode`,
      "generic"  X_0 R_r + 1e-2 g Gaussian, R_r the orthogonal factor of a Gaussian K x K matrix (planted()'s, at these scales)
      "signs"    X_0 D_r + noise, D_r random signs; the noise of axis k is 1e-2 of that axis's scale
      "pairs"    X_0 G_r D_r + noise of the same kind, G_r rotations by random angles inside the pairs of axes (0, 1), (2, 3), ..
    -- what replicates of real coordinates differ by: signs and turns inside pairs of close axes"""
    assert mode in MODES
    rng = np.random.default_rng(9000 + 131 * seed + 17 * n + K + 1000 * MODES.index(mode))
    scale = np.geomspace(1.0, g, K)
    X0 = _centred_orthonormal(rng, n, K) * scale
    X = np.empty((R + 1, n, K))
    X[0] = X0
    for r in range(1, R + 1):
        if mode == "generic":
            X[r] = X0 @ np.linalg.qr(rng.normal(size=(K, K)))[0] + NOISE * g * rng.normal(size=(n, K))
            continue
        T = np.eye(K)
        if mode == "pairs":
            for k in range(0, K - 1, 2):
                t = rng.uniform(0.0, 2.0 * np.pi)
                T[k:k + 2, k:k + 2] = [[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]]
        X[r] = X0 @ T * rng.choice([-1.0, 1.0], size=K) + NOISE * scale * rng.normal(size=(n, K))
    return X


def clustered(n, K, R, eps, seed):
    """a set [R + 1][n][K] whose M has its singular values within about eps of one another: X_0 has orthonormal centred
    columns, all of scale 1, X_r = X_0 R_r + eps * Gaussian"""
    rng = np.random.default_rng(11000 + 131 * seed + 17 * n + K)
    X0 = _centred_orthonormal(rng, n, K)
    X = np.empty((R + 1, n, K))
    X[0] = X0
    for r in range(1, R + 1):
        X[r] = X0 @ np.linalg.qr(rng.normal(size=(K, K)))[0] + eps * rng.normal(size=(n, K))
    return X


def eigvec_of(X):
    """(eig [..., K], vec [..., K, n]) whose coordinates are X [..., n, K] up to rounding: a column's squared length and the
    column over its length (a zero column: eigenvalue 0 and a unit vector)"""
    X = np.asarray(X, dtype=np.float64)
    nrm = np.sqrt((X ** 2).sum(axis=-2))
    vec = np.where(nrm[..., None, :] > 0, X / np.where(nrm > 0, nrm, 1.0)[..., None, :], 0.0)
    vec = kn(vec)
    zero = nrm == 0
    if zero.any():
        vec[zero, 0] = 1.0
    return nrm ** 2, vec


def check_separated(Xr, X0):
    """asserts, by numpy's SVD, that M = Xr^T X0 has sigma_min >= SEP * sigma_max; returns sigma_min / sigma_max"""
    s = np.linalg.svd(Xr.T @ X0, compute_uv=False)
    assert s.min() >= SEP * s.max(), "sigma_min = %.3g sigma_max" % (s.min() / s.max())
    return s.min() / s.max()


def check_band(Xr, X0, lo, hi):
    """asserts, by mpmath's sigma, that lo <= sigma_min / sigma_max < hi for M = Xr^T X0; returns the ratio"""
    s = procrustes_mp(Xr, X0)[2]
    x = s[-1] / s[0]
    assert lo <= x < hi, "sigma_min = %.3g sigma_max, outside [%.3g, %.3g)" % (x, lo, hi)
    return x


def check_y_mp(Xr, X0, Y):
    """Y against mpmath's, in units of TOL * max(|X0|, |Xr|)"""
    x = np.abs(Y - procrustes_mp(Xr, X0)[0]).max() / (TOL * max(np.abs(X0).max(), np.abs(Xr).max()))
    assert x <= 1, "Y: %.3g of its bound (mpmath)" % x
    return x


def check_fit_mp(Xr, X0, fit):
    """fit against mpmath's |Y - X0|^2, in units of TOL * (|Xr|^2 + |X0|^2)"""
    scale = (Xr ** 2).sum() + (X0 ** 2).sum()
    x = abs(fit - procrustes_mp(Xr, X0)[1]) / (TOL * scale)
    assert x <= 1, "fit: %.3g of its bound (mpmath)" % x
    return x


def check_y(Xr, X0, Y):
    """Y against numpy's, in units of TOL * max(|X0|, |Xr|) (largest magnitudes of an entry)"""
    x = np.abs(Y - procrustes(Xr, X0)[0]).max() / (TOL * max(np.abs(X0).max(), np.abs(Xr).max()))
    assert x <= 1, "Y: %.3g of its bound" % x
    return x


def check_fit(Xr, X0, fit):
    """fit against |Xr|^2 + |X0|^2 - 2 SUM sigma, in units of TOL * (|Xr|^2 + |X0|^2)"""
    s = np.linalg.svd(Xr.T @ X0, compute_uv=False)
    scale = (Xr ** 2).sum() + (X0 ** 2).sum()
    if scale == 0.0:
        assert fit == 0.0
        return 0.0
    x = abs(fit - (scale - 2.0 * s.sum())) / (TOL * scale)
    assert x <= 1, "fit: %.3g of its bound" % x
    return x


def check_orth(Xr, Y):
    """|Q Q^T - I| in units of TOL, as far as Y = Xr Q shows Q: Y Y^T = Xr Xr^T (in units of TOL |Xr|^2) always, and where
    Xr has full column rank (sigma_min >= SEP sigma_max) Q itself, recovered by least squares.  The limit of this check:
    the interface returns Y, not Q, so where Xr has a zero column the row of Q that multiplies it is never observed and only
    Q's action on Xr's row space is pinned (Y Y^T = Xr Xr^T); the completion of a singular M is seen with Q whole in the
    cases whose Xr has full rank (a zero column of X0, X0 = 0)"""
    scale = (Xr ** 2).sum()
    if scale == 0.0:
        assert not Y.any()
        return 0.0
    x = np.abs(Y @ Y.T - Xr @ Xr.T).max() / (TOL * scale)
    s = np.linalg.svd(Xr, compute_uv=False)
    if s.min() >= SEP * s.max():
        Q = np.linalg.lstsq(Xr, Y, rcond=None)[0]
        x = max(x, np.abs(Q @ Q.T - np.eye(Q.shape[0])).max() / TOL)
    assert x <= 1, "orthogonality: %.3g of its bound" % x
    return x


def check_left_out(Y, fit):
    """a matrix left out: positive quiet NaNs"""
    assert np.all(bits(Y) == NAN_BITS) and np.all(bits(fit) == NAN_BITS)


def check_set(X, aligned, fit, regular=True, status=None):
    """one set: X [n_mat][n][K] as the library saw it, aligned [n_mat][K][n], fit [n_mat]; `regular`: the separation is
    asserted and Y compared with numpy's.  Returns the largest figure of each kind"""
    worst = {"y": 0.0, "fit": 0.0, "orth": 0.0}
    n_mat = len(X)
    ok = np.ones(n_mat, dtype=bool) if status is None else np.asarray(status, dtype=bool)
    for r in range(n_mat):
        if not ok[r] or not ok[0]:
            check_left_out(aligned[r], fit[r])
            continue
        if r == 0:
            assert np.array_equal(bits(aligned[0]), bits(kn(X[0]))) and bits(fit[0]) == 0
            continue
        Y = nk(aligned[r])
        assert np.all(np.isfinite(Y)) and np.isfinite(fit[r])
        if regular:
            check_separated(X[r], X[0])
            worst["y"] = max(worst["y"], check_y(X[r], X[0], Y))
        worst["fit"] = max(worst["fit"], check_fit(X[r], X[0], fit[r]))
        worst["orth"] = max(worst["orth"], check_orth(X[r], Y))
    return worst


def band_of(g):
    """the decade either side of g^2, where graded(.., g, ..) is to put sigma_min(M) / sigma_max(M)"""
    return 0.1 * g * g, 10.0 * g * g


CLUSTERED_BAND = (0.5, 1.0)  # every singular value within a few eps of 1


def check_set_mp(X, aligned, fit, band, y=True):
    """one set against mpmath: X [n_mat][n][K] as the library saw it, aligned [n_mat][K][n], fit [n_mat]; every replicate's
    sigma_min / sigma_max is asserted to lie in `band` = (lo, hi); y=False (the floor band): Y is compared with nothing --
    fit, orthogonality and finiteness alone.  Returns the largest figure of each kind"""
    worst = {"fit": 0.0, "orth": 0.0}
    assert np.array_equal(bits(aligned[0]), bits(kn(X[0]))) and bits(fit[0]) == 0
    for r in range(1, len(X)):
        Y = nk(aligned[r])
        assert np.all(np.isfinite(Y)) and np.isfinite(fit[r])
        check_band(X[r], X[0], *band)
        if y:
            worst["y"] = max(worst.get("y", 0.0), check_y_mp(X[r], X[0], Y))
        worst["fit"] = max(worst["fit"], check_fit_mp(X[r], X[0], fit[r]))
        worst["orth"] = max(worst["orth"], check_orth(X[r], Y))
    return worst
