"""The host arithmetic of the group means (include/ngsdist_amd.h "Group-mean distance matrices"): the numbering of group
pairs, the cells of every group pair, the Python helpers, and the new names in the header and the binding list.  No device."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["ngd_n_group_pairs", "ngd_group_pair_index", "ngd_group_cells", "ngd_set_groups", "ngd_group_means_device",
       "ngd_run_job_groups", "ngd_run_windows_groups", "ngd_run_windows_job_var_groups"]


@pytest.fixture(scope="module")
def N():
    os.environ.setdefault("NGD_NO_TORCH", "1")
    import ngsdist_amd
    return ngsdist_amd


def test_group_pair_numbering_is_the_upper_triangle_with_the_diagonal(N):
    for G in range(1, 8):
        a, b = np.triu_indices(G)  # row-major, a <= b
        assert N.n_group_pairs(G) == len(a) == G * (G + 1) // 2
        assert [N.group_pair_index(G, int(x), int(y)) for x, y in zip(a, b)] == list(range(len(a)))
    assert N.n_group_pairs(0) == 0
    assert N.n_group_pairs(2 ** 32 - 1) == (2 ** 32 - 1) * 2 ** 32 // 2  # (no 32-bit overflow)
    with pytest.raises(ValueError):
        N.group_pair_index(3, 2, 1)


def brute_cells(g, G):
    cells = np.zeros(G * (G + 1) // 2, dtype=np.uint64)
    for i1 in range(len(g)):
        for i2 in range(i1 + 1, len(g)):
            if g[i1] >= 0 and g[i2] >= 0:
                a, b = sorted((int(g[i1]), int(g[i2])))
                cells[a * G - a * (a - 1) // 2 + (b - a)] += 1
    return cells


def test_group_cells_against_a_brute_force_count(N):
    rng = np.random.default_rng(11)
    for n, G in ((2, 1), (3, 2), (17, 3), (40, 7), (63, 5), (30, 30)):
        for _ in range(3):
            g = rng.integers(-1, G, n).astype(np.int32)
            g[g == G - 1] = -1 if G > 2 else G - 1  # G > 2: the last group is empty
            assert np.array_equal(N.group_cells(g, G), brute_cells(g, G)), (n, G)
    everyone = np.zeros(9, dtype=np.int32)
    assert N.group_cells(everyone).tolist() == [36]
    assert N.group_cells(np.arange(5)).sum() == 10 and N.group_cells(np.arange(5))[N.group_pair_index(5, 2, 2)] == 0
    for bad in ([0, 3, 1], [0, -2, 1]):
        with pytest.raises(N.NgdError):
            N.group_cells(bad, 3)
    with pytest.raises(N.NgdError):
        N.group_cells([-1, -1], 0)


def test_expand_groups_is_symmetric_with_the_within_group_value_on_the_diagonal(N):
    G = 4
    m = np.arange(2 * 3 * N.n_group_pairs(G), dtype=np.float64).reshape(2, 3, -1)
    full = N.expand_groups(m, G)
    assert full.shape == (2, 3, G, G)
    for a in range(G):
        for b in range(a, G):
            k = N.group_pair_index(G, a, b)
            assert np.array_equal(full[..., a, b], m[..., k]) and np.array_equal(full[..., b, a], m[..., k])
    with pytest.raises(ValueError):
        N.expand_groups(m, G + 1)


def test_header_binding_list_and_library_declare_the_new_names(N):
    from ngsdist_amd import _lib
    txt = open(os.path.join(ROOT, "include", "ngsdist_amd.h")).read()
    decl = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    L = _lib.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, decl), name + " is not declared in the header"
        assert name in _lib.EXPORTS and hasattr(L, name), name
    for method in ("set_groups", "group_means", "run_job_groups", "run_windows_groups", "run_windows_job_var_groups"):
        assert callable(getattr(N.Engine, method))
    assert L.ngd_abi_version() == 6  # additions under ABI 6
    # refused on their arguments, before HIP is touched
    assert L.ngd_set_groups(None, None, 0) == -1 and "ngd_set_groups" in L.ngd_last_error().decode()
    assert L.ngd_run_windows_groups(None, None, None, 0, 0, 0, None, None) == -1
    assert L.ngd_last_error().decode() == "ngd_run_windows_groups: null engine"
