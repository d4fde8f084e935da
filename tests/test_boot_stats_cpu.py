"""Bootstrap summaries, the part that needs no device (include/ngsdist_amd.h "Bootstrap summaries"): the new names in the
header, the binding list and the library, and ngd_boot_stats_host against the numpy statement of the contract
(boot_stats_expect.py) on planted values -- NaN, +-inf, -0.0 / 0.0 ties, duplicates, an all-NaN cell, a cell with one
finite replicate, columns already ascending and descending.  est / mean / lo / hi must be equal as values (made NaNs are
positive quiet NaNs, by bits), used equal, sd within 4 ulp (one division and one square root after sums that are equal)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import boot_stats_expect as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["ngd_boot_stats_max_rep", "ngd_boot_stats_host", "ngd_boot_stats_device", "ngd_boot_stats_values_device",
       "ngd_run_job_stats", "ngd_run_windows_job_var_stats", "ngd_run_job_groups_stats",
       "ngd_run_windows_job_var_groups_stats", "ngd_last_boot_stats_ms"]


@pytest.fixture(scope="module")
def N():
    os.environ.setdefault("NGD_NO_TORCH", "1")
    import ngsdist_amd
    return ngsdist_amd


def test_header_binding_list_and_library_declare_the_new_names(N):
    from ngsdist_amd import _lib
    txt = open(os.path.join(ROOT, "include", "ngsdist_amd.h")).read()
    decl = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    L = _lib.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, decl), name + " is not declared in the header"
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert re.search(r"#define\s+NGD_BOOT_NSTAT\s+5\b", decl) and _lib.NSTAT == 5
    # the version script hides the compiler's own markers and nothing of the interface
    vs = open(os.path.join(ROOT, "ngsdist_amd", "csrc", "exports.map")).read()
    assert "ngd_" not in re.sub(r"#.*", "", vs)
    for method in ("boot_stats", "boot_stats_values", "run_job_stats", "run_windows_job_var_stats", "run_job_groups_stats",
                   "run_windows_job_var_groups_stats", "last_boot_stats_ms"):
        assert callable(getattr(N.Engine, method))
    assert L.ngd_abi_version() == 6  # additions under ABI 6
    # refused on their arguments, before HIP is touched
    out, used = (C.c_double * 5)(), (C.c_uint64 * 1)()
    assert L.ngd_run_job_stats(None, None, 1, 1, 1, 0, 0, 0.95, out, used) == -1
    assert L.ngd_last_error().decode() == "ngd_run_job_stats: null engine"
    assert L.ngd_last_boot_stats_ms(None, None) == -1


def test_max_rep_is_the_lds_tile_rule(N):
    """a workgroup's tile is [R + 1][C] doubles, C the widest of 64, 32, 16 that fits 160 KiB: the cap is the narrowest's"""
    lds = 160 * 1024
    assert N.boot_stats_max_rep() == lds // (16 * 8) - 1 == 1279


@pytest.mark.parametrize("n_rep", [1, 2, 3, 100])
@pytest.mark.parametrize("ci", [0.95, 0.5])
def test_host_function_against_numpy(N, n_rep, ci):
    v = X.planted(3, n_rep, 130, seed=n_rep)
    got = N.boot_stats_host(v, ci)
    assert got[0].shape == (3, 5, 130) and got[1].shape == (3, 130) and got[1].dtype == np.uint64
    X.check_exact(got, X.expect(v, ci), "host R = %d ci %g" % (n_rep, ci))
    # what was planted is there
    s, u = got
    assert np.all(u[:, 5] == 0) and np.all(np.isnan(s[:, 1:, 5]))
    assert np.all(u[:, 6] == 1) and np.all(s[:, 1, 6] == 0.125) and np.all(s[:, 3, 6] == 0.125) and np.all(s[:, 4, 6] == 0.125)
    assert np.all(np.isnan(s[:, 0, 10])) and np.all(np.isposinf(s[:, 0, 11]))
    if n_rep >= 3:
        assert np.all(u[:, 0] == n_rep - 1) and np.all(u[:, 1] == n_rep - 1) and np.all(u[:, 2] == n_rep - 1)
    # one set alone carries the bits it has among the three; a leading shape is kept
    one = N.boot_stats_host(v[1], ci)
    assert np.array_equal(one[0].view(np.uint64), s[1].view(np.uint64)) and np.array_equal(one[1], u[1])
    two = N.boot_stats_host(v.reshape(3, 1, n_rep + 1, 130), ci)
    assert two[0].shape == (3, 1, 5, 130) and np.array_equal(two[0].view(np.uint64).ravel(), s.view(np.uint64).ravel())


def test_order_statistics_are_values_of_the_column(N):
    """R = 100 at 95 %: k_lo = floor(0.025 * 99) = 2, k_hi = ceil(0.975 * 99) = 97"""
    rng = np.random.default_rng(0)
    v = rng.random((101, 7))
    s, u = N.boot_stats_host(v, 0.95)
    srt = np.sort(v[1:], axis=0)
    assert np.array_equal(s[3], srt[2]) and np.array_equal(s[4], srt[97]) and np.all(u == 100)
    s, _ = N.boot_stats_host(v, 0.5)
    assert np.array_equal(s[3], srt[24]) and np.array_equal(s[4], srt[75])


def test_host_function_refusals(N):
    v = np.zeros((2, 3))
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(N.NgdError) as ei:
            N.boot_stats_host(v, bad)
        assert ei.value.code == -1
    with pytest.raises(N.NgdError):
        N.boot_stats_host(np.zeros((1, 3)))  # no replicate
    with pytest.raises(N.NgdError):
        N.boot_stats_host(np.zeros((0, 2, 3)))  # no set
