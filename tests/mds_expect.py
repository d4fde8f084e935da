"""Classical MDS by numpy (include/ngsdist_amd.h "Classical MDS"): the double-centred matrix B of a row of pair values, its
spectrum by numpy.linalg.eigh, the matrices the MDS tests share, and the contract's checks as functions.  Every check
returns its largest figure relative to its bound's scale, so that the tests can print it before they assert."""
import numpy as np

NAN_BITS = np.uint64(0x7FF8000000000000)
TOL = 1e-9       # the project's tolerance, relative to S = max |eigenvalue| of numpy's eigvalsh of the same B
GAP = 1e-3       # a vector is compared with numpy's where its eigenvalue lies GAP * S or more from every other one
SIGN_GAP = 1e-6  # the sign rule is checked where the two largest magnitudes differ by more than this, relatively
SIZES = [3, 4, 5, 63, 64, 65, 130, 257]
N_MAT = 37
# the random matrices' seed is SEED + n: chosen, by numpy alone, so that at every size each of the top four eigenvalues of
# every random matrix lies at least 2.4e-3 S from every other one (the smallest: n = 3) -- a property of the inputs that
# check_matrix(require_gaps=True) asserts again
SEED = 1010
AT = {"equal": 5, "zero": 6, "ints": 7, "planted": 8, "nan": 18, "inf": 19}  # the special matrices among the 37


def dims(n):
    """the K of a size: 1, 4 (n - 1 where smaller), n - 1 at n <= 5 and 16 at n >= 63"""
    return sorted({1, min(4, n - 1), n - 1 if n <= 5 else 16})


def square(v, n):
    D = np.zeros((n, n))
    D[np.triu_indices(n, 1)] = v
    return D + D.T


def centred(v, n):
    A = -0.5 * square(v, n) ** 2
    r = A.mean(axis=0)
    return A - r[None, :] - r[:, None] + r.mean()


def planted_points(n, seed):
    """n points in 4 dimensions, column j scaled by 2^-j"""
    return np.random.default_rng(seed).normal(size=(n, 4)) * 2.0 ** -np.arange(4)


def matrices(n, seed=None):
    """the 37 matrices of a size: random cells uniform in [0.05, 1.5) with an all-equal one (0.25), an all-zero one, one of
    small integers, the Euclidean distances of planted_points(), and a NaN cell and an inf cell in the middle"""
    p = n * (n - 1) // 2
    rng = np.random.default_rng(SEED + n if seed is None else seed)
    v = rng.uniform(0.05, 1.5, size=(N_MAT, p))
    v[AT["equal"]] = 0.25
    v[AT["zero"]] = 0.0
    v[AT["ints"]] = rng.integers(1, 4, size=p)
    P = planted_points(n, 2000 + n)
    v[AT["planted"]] = np.sqrt(((P[:, None, :] - P[None, :, :]) ** 2).sum(-1))[np.triu_indices(n, 1)]
    v[AT["nan"], p // 2] = np.nan
    v[AT["inf"], p // 2] = np.inf
    return v


def few(n):
    """three matrices of a large size, made one at a time: matrices(n)[0] (the first random one), a planted one (the squared
    distances summed a dimension at a time: n x n at once, not n x n x 4) and a random one with a NaN cell"""
    p = n * (n - 1) // 2
    v = np.empty((3, p))
    v[0] = np.random.default_rng(SEED + n).uniform(0.05, 1.5, size=p)
    P = planted_points(n, 2000 + n)
    d2 = np.zeros((n, n))
    for j in range(P.shape[1]):
        d2 += (P[:, j, None] - P[None, :, j]) ** 2
    v[1] = np.sqrt(d2)[np.triu_indices(n, 1)]
    v[2] = np.random.default_rng(3000 + n).uniform(0.05, 1.5, size=p)
    v[2, p // 2] = np.nan
    return v


def pairs_of(P):
    """the Euclidean distances of the rows of P [n][dim], in pair order; a dimension at a time, so that two equal rows are
    exactly 0 apart and, in one dimension, a distance is |x_a - x_b| with no rounding beyond the subtraction's"""
    n = P.shape[0]
    d2 = np.zeros((n, n))
    for j in range(P.shape[1]):
        d2 += (P[:, j, None] - P[None, :, j]) ** 2
    return np.sqrt(d2)[np.triu_indices(n, 1)]


DUP = {"halves": 0, "quarter": 1, "site": 2, "sites": 3, "protos": 4, "exact": 5}  # the matrices of duplicates(n)
N_DUP = len(DUP)


def duplicates(n, seed=0):
    """six matrices of points with few distinct rows (a window with one or two variable sites, clones): B has rank 1 to 3
    and the eigenvalue 0 about n times over.  Two groups n/2 | n/2 at +-0.5; n/4 at 1 and the rest at 0; one site of
    genotypes 0/1/2 at random; two such sites; three prototype points in the plane, individual i taking prototype i mod 3;
    the points (1, -1, 0, ..., 0), whose B is [[1, -1], [-1, 1]] in a corner of zeros -- at n a power of two every cell of
    it is exact, it is tridiagonal as it stands and its spectrum is {2, 0, ...}"""
    rng = np.random.default_rng(4000 + 31 * seed + n)
    x = np.zeros((N_DUP, n, 2))
    x[DUP["halves"], :, 0] = np.where(np.arange(n) < n // 2, 0.5, -0.5)
    x[DUP["quarter"], :n // 4, 0] = 1.0
    x[DUP["site"], :, 0] = rng.integers(0, 3, size=n)
    x[DUP["sites"]] = rng.integers(0, 3, size=(n, 2))
    x[DUP["protos"]] = rng.normal(size=(3, 2))[np.arange(n) % 3]
    x[DUP["exact"], 0, 0], x[DUP["exact"], 1, 0] = 1.0, -1.0
    return np.stack([pairs_of(P) for P in x])


GAPS = [1e-4, 1e-7, 1e-10, 1e-13, 0.0]


def planted_spectrum(gap):
    return np.array([1.0 + gap, 1.0, 0.25, 0.25 * (1.0 - gap)])


def near_degenerate(n, gap, seed=0):
    """the distances of the points Q diag(sqrt(s)): Q four orthonormal columns orthogonal to the ones vector (QR of a
    centred Gaussian n x 4), s = planted_spectrum(gap) -- B = Q diag(s) Q^T, so its eigenvalues are s and n - 4 zeros by
    construction: two pairs `gap` apart, relatively, which the shift rule and Gram-Schmidt have to hold apart"""
    G = np.random.default_rng(5000 + 31 * seed + n).normal(size=(n, 4))
    Q = np.linalg.qr(G - G.mean(axis=0))[0]
    return pairs_of(Q * np.sqrt(planted_spectrum(gap)))


_spectra = {}


def spectrum(v, n):
    """(B, eigenvalues in descending order, their vectors as rows) by numpy, computed once per matrix"""
    key = (n, v.tobytes())
    if key not in _spectra:
        B = centred(v, n)
        lam, U = np.linalg.eigh(B)
        _spectra[key] = (B, lam[::-1].copy(), U[:, ::-1].T.copy())
    return _spectra[key]


def is_random(m):
    return m not in AT.values()


def check_matrix(v, n, K, eig, vec, tot, sign=True, require_gaps=False):
    """the contract's checks of one finite matrix's outputs against numpy; returns a dict of the figures (each <= 1 passes:
    they are divided by their bounds)"""
    B, lam, U = spectrum(v, n)
    S = np.abs(lam).max()
    fig = {}
    assert eig.shape == (K,) and vec.shape == (K, n) and tot.shape == (2,)
    assert np.all(np.isfinite(eig)) and np.all(np.isfinite(vec)) and np.all(np.isfinite(tot))
    if S == 0.0:  # the all-zero matrix
        assert np.all(np.abs(eig) <= 1e-200) and np.all(np.abs(tot) <= 1e-200)
        fig["orth"] = np.abs(vec @ vec.T - np.eye(K)).max() / TOL
        assert fig["orth"] <= 1
        return fig
    fig["eig"] = np.abs(eig - lam[:K]).max() / (TOL * S)
    fig["tot"] = max(abs(tot[0] - lam.sum()), abs(tot[1] - lam[lam > 0].sum())) / (TOL * np.abs(lam).sum())
    fig["res"] = max(np.linalg.norm(B @ vec[k] - eig[k] * vec[k]) for k in range(K)) / (TOL * S)
    fig["orth"] = np.abs(vec @ vec.T - np.eye(K)).max() / TOL
    assert np.all(np.diff(eig) <= 0), "eigenvalues are not in descending order"
    fig["dot"] = 0.0
    for k in range(K):
        a = np.sort(np.abs(vec[k]))[::-1]
        if sign and a[0] - a[1] > SIGN_GAP * a[0]:
            i = int(np.argmax(np.abs(vec[k])))
            assert vec[k][i] > 0, "sign rule: vector %d" % k
        gap = np.abs(np.delete(lam, k) - lam[k]).min()
        if gap >= GAP * S:
            fig["dot"] = max(fig["dot"], (1 - abs(vec[k] @ U[k])) / TOL)
        elif require_gaps and k < 4:
            raise AssertionError("top-4 eigenvalue %d of a random matrix lies %.3g S from another" % (k, gap / S))
    for name, x in fig.items():
        assert x <= 1, "%s: %.3g of its bound" % (name, x)
    return fig


def check_subspace(v, n, vec, idx):
    """the vectors `idx` of a matrix span what numpy's do: 1 - (the smallest singular value of vec[idx] U[idx]^T), in units
    of TOL.  Holds where the eigenvalues `idx` lie, by numpy alone, GAP * S or more from all others (asserted here),
    however close they lie to each other"""
    B, lam, U = spectrum(v, n)
    S = np.abs(lam).max()
    idx = list(idx)
    away = np.abs(np.delete(lam, idx)[None, :] - lam[idx][:, None]).min()
    assert away >= GAP * S, "eigenvalues %s lie %.3g S from the rest" % (idx, away / S)
    x = (1 - np.linalg.svd(vec[idx] @ U[idx].T, compute_uv=False).min()) / TOL
    assert x <= 1, "subspace %s: %.3g of its bound" % (idx, x)
    return x


def check_planted_spectrum(v, n, gap, eig):
    """the top four eigenvalues of near_degenerate(n, gap) against the planted ones, in units of TOL * S"""
    s = planted_spectrum(gap)
    assert len(eig) >= 4
    x = np.abs(eig[:4] - s).max() / (TOL * s[0])
    assert x <= 1, "planted eigenvalues: %.3g of the bound" % x
    return x


def check_bad(eig, vec, tot, status):
    """a matrix with a cell that is not finite: status 0 and positive quiet NaNs"""
    assert status == 0
    for a in (eig, vec, tot):
        assert np.all(np.ascontiguousarray(a, dtype=np.float64).view(np.uint64) == NAN_BITS)


def check_all(v, n, K, eig, vec, tot, status, who):
    """every matrix of matrices(n): prints and returns the largest figure of each kind"""
    worst = {}
    assert status.tolist() == [0 if m in (AT["nan"], AT["inf"]) else 1 for m in range(len(v))]
    for m in range(len(v)):
        if not status[m]:
            check_bad(eig[m], vec[m], tot[m], status[m])
            continue
        fig = check_matrix(v[m], n, K, eig[m], vec[m], tot[m], require_gaps=is_random(m))
        for name, x in fig.items():
            worst[name] = max(worst.get(name, 0.0), x)
    print("%s n=%d K=%d: largest figures in units of 1e-9: %s" % (who, n, K, {k: "%.3g" % x for k, x in worst.items()}))
    return worst


def check_planted(v, n, coords):
    """the planted matrix at K = 4: the coordinates reproduce every d_ab to 1e-9 * max d"""
    d = np.sqrt(((coords[:, None, :] - coords[None, :, :]) ** 2).sum(-1))[np.triu_indices(n, 1)]
    err = np.abs(d - v).max() / (TOL * v.max())
    print("planted n=%d: distances reproduced to %.3g of the bound" % (n, err))
    assert err <= 1
