"""Classical MDS, the part that needs no device (include/ngsdist_amd.h "Classical MDS"): the new names in the header, the
binding list and the library; ngd_mds_host against numpy (mds_expect.py) at n = 3, 4, 5, 63, 64, 65, 130, 257 on 37 matrices
each -- random ones, an all-equal, an all-zero, a small-integer and a planted Euclidean one, a NaN and an inf one beside
intact neighbours --; ngd_mds_coords; the refusals of the host form.

Bounds: 1e-9 relative to S = max |eigenvalue| (numpy's eigvalsh of the same B).  Every case prints its largest figures in
units of the bound; the largest seen over this file, as fractions of S: eigenvalues 6.0e-15, residuals 8.8e-15, totals
2.8e-15 of the sum of |eigenvalue|, orthonormality 8.9e-16, 1 - |v . numpy's v| 1.3e-15, the planted distances 2.3e-15 of the
largest distance."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mds_expect as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["ngd_mds_max_ind", "ngd_mds_max_dim", "ngd_mds_host", "ngd_mds_coords", "ngd_mds_values_device", "ngd_mds_device",
       "ngd_run_job_mds", "ngd_run_windows_mds", "ngd_run_windows_job_var_mds", "ngd_last_mds_ms"]


@pytest.fixture(scope="module")
def N():
    os.environ.setdefault("NGD_NO_TORCH", "1")
    import ngsdist_amd
    return ngsdist_amd


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def test_header_binding_list_and_library_declare_the_new_names(N):
    from ngsdist_amd import _lib
    txt = open(os.path.join(ROOT, "include", "ngsdist_amd.h")).read()
    decl = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    L = _lib.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, decl), name + " is not declared in the header"
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert re.search(r"#define\s+NGD_OPT_MDS_MAX_BYTES\s+20\b", decl)
    assert "Classical MDS" in txt
    assert L.ngd_abi_version() == 6
    assert N.mds_max_ind() == 4096 and N.mds_max_dim() == 16
    for name in ("mds", "mds_values", "run_job_mds", "run_windows_mds", "run_windows_job_var_mds", "last_mds_ms"):
        assert callable(getattr(N.Engine, name))


@pytest.mark.parametrize("n", X.SIZES)
def test_host_twin_against_numpy(N, n):
    v = X.matrices(n)
    for K in X.dims(n):
        eig, vec, tot, status = N.mds_host(v, n, K)
        assert eig.shape == (X.N_MAT, K) and vec.shape == (X.N_MAT, K, n) and tot.shape == (X.N_MAT, 2)
        X.check_all(v, n, K, eig, vec, tot, status, "host")
        # a matrix served alone carries the bits it has among 37: its neighbours -- the NaN one too -- do not disturb it
        for m in (3, X.AT["nan"] - 1, X.AT["nan"], X.AT["inf"] + 1):
            one = N.mds_host(v[m:m + 1], n, K)
            assert all(np.array_equal(bits(a[0]), bits(b[m])) for a, b in zip(one[:3], (eig, vec, tot))) and one[3][0] == status[m]


@pytest.mark.parametrize("n", X.SIZES)
def test_planted_points_come_back_as_coordinates(N, n):
    v = X.matrices(n)
    K = min(4, n - 1)
    m = X.AT["planted"]
    eig, vec, tot, status = N.mds_host(v[m], n, K)
    assert status == 1
    X.check_planted(v[m], n, N.mds_coords(eig, vec))
    # four dimensions hold every bit of variance there is
    if n > 5:
        assert abs(tot[1] - eig.sum()) <= X.TOL * tot[1] and abs(tot[0] - tot[1]) <= X.TOL * tot[1]


def test_all_zero_and_all_equal(N):
    n, K = 65, 16
    v = X.matrices(n)
    eig, vec, tot, status = N.mds_host(v[[X.AT["zero"], X.AT["equal"]]], n, K)
    assert status.tolist() == [1, 1]
    assert np.all(np.abs(eig[0]) <= 1e-200) and np.all(np.isfinite(vec[0]))
    assert np.abs(vec[0] @ vec[0].T - np.eye(K)).max() <= X.TOL
    # all cells c: the eigenvalue c^2 / 2 with multiplicity n - 1, and 0
    c = 0.5 * 0.25 ** 2
    assert np.abs(eig[1] - c).max() <= X.TOL * c
    assert abs(tot[1][0] - (n - 1) * c) <= X.TOL * n * c and abs(tot[1][1] - (n - 1) * c) <= X.TOL * n * c


def test_coords_of_negative_and_nan_eigenvalues(N):
    eig = np.array([[4.0, -1.0], [np.nan, np.nan]])
    vec = np.array([[[0.6, 0.8, 0.0], [1.0, 0.0, 0.0]], [[np.nan] * 3] * 2])
    c = N.mds_coords(eig, vec)
    assert c.shape == (2, 3, 2)
    assert np.array_equal(c[0], np.array([[1.2, 0.0], [1.6, 0.0], [0.0, 0.0]]))
    assert np.all(np.isnan(c[1]))


def test_host_form_refusals(N):
    from ngsdist_amd import _lib
    L = _lib.load()
    n, K = 5, 2
    v = np.ones((1, 10))
    eig, vec, tot, st = np.full((1, K), 7.0), np.full((1, K, n), 7.0), np.full((1, 2), 7.0), np.full(1, 7, dtype=np.uint32)
    dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint32)
    ptr = lambda a: a.ctypes.data_as(dp)
    good = [ptr(v), 1, n, K, ptr(eig), ptr(vec), ptr(tot), st.ctypes.data_as(up)]
    assert L.ngd_mds_host(*good) == 0
    eig[:] = vec[:] = tot[:] = 7.0
    st[:] = 7
    for at, bad in [(0, None), (4, None), (5, None), (6, None), (7, None), (1, 0), (2, 2), (3, 0), (3, n), (3, 17)]:
        args = list(good)
        args[at] = bad
        assert L.ngd_mds_host(*args) == -1, (at, bad)  # NGD_E_INVALID
    big = [ptr(np.ones((1, 20 * 19 // 2))), 1, 20, 17, ptr(np.empty(17)), ptr(np.empty(17 * 20)), ptr(np.empty(2)), st.ctypes.data_as(up)]
    assert L.ngd_mds_host(*big) == -1  # K above ngd_mds_max_dim()
    assert np.all(eig == 7.0) and np.all(vec == 7.0) and np.all(tot == 7.0) and np.all(st == 7)
    assert L.ngd_mds_coords(None, ptr(vec), 1, n, K, ptr(np.empty(n * K))) == -1
    with pytest.raises(ValueError):
        N.mds_host(np.ones((2, 9)), 5, 2)
