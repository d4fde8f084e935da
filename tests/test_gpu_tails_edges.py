"""The bootstrap summaries and the group means (boot_stats.hip k_boot_stats, group_reduce.hip k_group_means / k_group_finish,
engine_groups.hip groups_reduce) on the paths test_gpu_boot_stats.py and test_gpu_groups.py stop short of.

* k_boot_stats<32, false> and <16, false>: sums and counts at R = 400 and 700 (R above 319 leaves the 64-wide tile), on
  planted tensors.  Expected values and tolerances are test_gpu_boot_stats.check_sums' as they are: ngsdist_amd.finish, then
  numpy (boot_stats_expect.expect); exact under model 0, check_close under models 1 and 2.
* the two heaps' corners: ci near 1 (no pop on either heap), 0.9 (a fractional rank product), near 0 (the ranks next to
  the median: the most pops on both), at R = 1 .. 5, 100, 101 -- the planted columns hold fewer finite replicates, of
  either parity, down to m = 1 (k_lo = k_hi) and 0; check_exact against numpy.
* groups_reduce in more than one chunk of 2^22 / max(n_work, n_gp) matrices: 24 singleton groups make a mean its one cell,
  so matrix m's mean of group pair (a, b) must be S[m, pair(a, b)] / Cn[m, pair(a, b)] bit for bit -- plain arithmetic, no
  tolerance -- and a wrong offset of the second chunk, in or out, cannot pass: cell 0 of matrix m is 1 / (m + 1).
* the kept form (mean == NULL: the means stay on the device for the summaries) across the same chunk boundary, through
  run_windows_job_var_groups_stats on 140 windows x 101 matrices.
Every tolerance-based comparison prints its largest error.  The largest seen on an MI355X over the cases of this file:
relative error of est / mean / lo / hi under models 1 and 2 4.49e-16 (bound 1e-13); sd at 7.0e-5 of its bound; where equality
is asked, sd 0 ulp from numpy's (bound 4) and everything else equal."""
import numpy as np
import pytest

import boot_stats_expect as X
import test_gpu_boot_stats as TB
from test_gpu_boot_stats import N, bits, same_bits

pytestmark = pytest.mark.gpu

N_IND, N_PAIRS, N_GP = 24, 276, 300
QNAN = 0x7FF8000000000000


def upload(S, Cn):
    import torch
    ds = torch.from_numpy(np.ascontiguousarray(S)).to("cuda")
    dc = torch.from_numpy(np.ascontiguousarray(Cn).astype(np.int64)).to("cuda")
    torch.cuda.synchronize()
    return ds, dc


# ---- a. the narrow tiles from sums and counts --------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rep", [400, 700])
def test_narrow_tiles_from_sums_and_counts(n_rep):
    """276 cells: 8 tiles of 32 cells and 20 more, 17 tiles of 16 and 4 more"""
    width = {400: 32, 700: 16}[n_rep]
    assert (n_rep + 1) * width * 8 <= 160 * 1024 < (n_rep + 1) * 2 * width * 8
    rng = np.random.default_rng(n_rep)
    Cn = rng.integers(0, 301, (2, n_rep + 1, N_PAIRS))
    Cn[rng.random(Cn.shape) < 0.02] = 0
    S = rng.uniform(0.0, 0.6, Cn.shape) * Cn
    Cn = Cn.astype(np.uint64)
    assert 0.01 < (Cn == 0).mean() < 0.04
    with N().Engine(N_IND, 16) as e:
        e.synth_fill(1).commit()
        ds, dc = upload(S, Cn)
        for model in (0, 1, 2):
            got = e.boot_stats(ds.data_ptr(), dc.data_ptr(), 2, n_rep + 1, evol_model=model)
            TB.check_sums(got, S, Cn, model, "planted sums R = %d (tile %d) model %d" % (n_rep, width, model))
            # a set served alone carries the bits it has among two
            one = e.boot_stats(ds[1].data_ptr(), dc[1].data_ptr(), 1, n_rep + 1, evol_model=model)
            assert same_bits((one[0][0], one[1][0]), (got[0][1], got[1][1])), model
        if n_rep == 400:  # --tot_sites: d_cnt is not read (a null pointer here)
            got = e.boot_stats(ds.data_ptr(), None, 2, n_rep + 1, evol_model=0, tot_sites=1234)
            X.check_exact(got, TB.from_sums(S, Cn, 0, 1234), "planted sums R = 400 tot_sites")


# ---- b. the heaps' corners ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_engine():
    with N().Engine(3, 16, kernel="mfma") as e:
        e.synth_fill(1).commit()
        yield e


@pytest.mark.parametrize("n_rep", [1, 2, 3, 4, 5, 100, 101])
def test_the_heaps_corners(small_engine, n_rep):
    v = X.planted(2, n_rep, 70, seed=n_rep)
    for ci in (0.999999, 0.9, 1e-9):
        got = TB.values_on_device(small_engine, v, ci)
        X.check_exact(got, X.expect(v, ci), "values R = %d ci %g" % (n_rep, ci))
    # what the three intervals are for, at a cell whose replicates are all finite (column 12 on: random; the planted
    # columns have fewer finite ones, of either parity, down to m = 1 and 0): the ranks by the contract's two formulas
    last = n_rep - 1
    lo_of = lambda ci: int(np.floor((1.0 - ci) / 2.0 * last))  # noqa: E731
    hi_of = lambda ci: int(np.ceil((1.0 - (1.0 - ci) / 2.0) * last))  # noqa: E731
    assert lo_of(0.999999) == 0 and hi_of(0.999999) == last  # no pop on either heap
    if n_rep >= 100:
        assert 0 < lo_of(0.9) < hi_of(0.9) < last
        # the ranks next to the median: the most pops on both heaps (the two are one rank only at m = 1: R = 1, column 6)
        assert hi_of(1e-9) - lo_of(1e-9) == (1 if last % 2 else 2) and lo_of(1e-9) == (last - 1) // 2
    if n_rep == 1:
        assert lo_of(1e-9) == hi_of(1e-9) == 0


# ---- c. group means in more than one chunk ----------------------------------------------------------------------------------
def singleton_index():
    """the group pair of every pair of individuals, in pair order, and the diagonal group pairs: 24 groups of one"""
    i1, i2 = np.triu_indices(N_IND, 1)  # row-major upper triangle: the pair order
    off = np.array([N().group_pair_index(N_IND, a, b) for a, b in zip(i1, i2)])
    diag = np.array([N().group_pair_index(N_IND, a, a) for a in range(N_IND)])
    assert len(set(off) | set(diag)) == N_GP
    return off, diag


def check_singletons(mean, used, d, what):
    """mean, used [n_mat][n_gp] against the cells d [n_mat][n_pairs]: a mean over one cell is the cell"""
    off, diag = singleton_index()
    fin = np.isfinite(d)
    assert np.array_equal(used[:, off], fin.astype(np.uint64)), what
    assert np.array_equal(bits(mean[:, off][fin]), bits(d[fin])), what
    assert np.all(bits(mean[:, off][~fin]) == QNAN), what
    assert np.all(used[:, diag] == 0) and np.all(bits(mean[:, diag]) == QNAN), what


def test_group_means_in_two_chunks():
    per_chunk = (1 << 22) // N_GP
    assert per_chunk == 13981
    n_mat = per_chunk + 37
    rng = np.random.default_rng(13981)
    Cn = rng.integers(1, 400, (n_mat, N_PAIRS))
    S = rng.uniform(0.0, 0.6, Cn.shape) * Cn
    # cells that are not finite: 0 / 0 and x / 0, about 1 % each
    hole = rng.random(Cn.shape)
    Cn[hole < 0.02] = 0
    S[hole < 0.01] = 0.0
    # matrix m says which it is: cell 0 is 1 / (m + 1)
    Cn[:, 0] = 1 + np.arange(n_mat)
    S[:, 0] = 1.0
    Cn = Cn.astype(np.uint64)
    with np.errstate(all="ignore"):
        d = S / Cn.astype(np.float64)
    assert np.isnan(d).any() and np.isinf(d).any() and len(np.unique(d[:, 0])) == n_mat
    with N().Engine(N_IND, 16) as e:
        e.synth_fill(1).commit().set_groups(np.arange(N_IND), N_IND)
        ds, dc = upload(S, Cn)
        mean, used = e.group_means(ds.data_ptr(), dc.data_ptr(), n_mat, evol_model=0)
        assert e.groups_ms() > 0
    assert mean.shape == (n_mat, N_GP)
    check_singletons(mean, used, d, "%d matrices" % n_mat)


# ---- d. the kept form in more than one chunk ---------------------------------------------------------------------------------
def test_kept_group_means_in_two_chunks():
    import torch
    n_sites, n_win, n_rep, q = 700, 140, 100, 5
    w = np.arange(n_win)
    lo = 4 * w
    hi = lo + 1 + (37 * w) % 140  # 1 .. 140 sites: unequal, some shorter than one block
    assert hi.max() <= n_sites and len(set(hi - lo)) > 100
    short = (hi - lo) // q == 0
    assert 0 < short.sum() < 10
    assert n_win * (n_rep + 1) > (1 << 22) // N_GP
    maps, off = N().window_boot_maps(9, lo, hi, n_rep, q)
    p = TB.synth(31, N_IND, n_sites, miss_frac=0.3)
    with N().Engine(N_IND, n_sites, kernel="mfma", pairwise_del=True) as e:
        e.upload_ind_major(p).commit().set_groups(np.arange(N_IND), N_IND)
        S, Cn = e.run_windows_job_var(lo, hi, maps, off, q, n_rep=n_rep)
        mean, used = e.run_windows_job_var_groups(lo, hi, maps, off, q, evol_model=0, n_rep=n_rep)
        gs = e.run_windows_job_var_groups_stats(lo, hi, maps, off, q, evol_model=0, n_rep=n_rep)
        assert e.windows_info()["batches"] >= 1
        up = torch.from_numpy(mean).to("cuda")
        torch.cuda.synchronize()
        again = e.boot_stats_values(up.data_ptr(), n_win, n_rep + 1, N_GP)
    assert gs[0].shape == (n_win, 5, N_GP) and gs[1].shape == (n_win, N_GP)
    assert same_bits(again, gs)
    X.check_exact(gs, X.expect(mean), "kept means of %d matrices" % (n_win * (n_rep + 1)))
    # the sibling's means themselves: the cells, by the division alone
    with np.errstate(all="ignore"):
        d = N().finish(S.reshape(-1), Cn.reshape(-1), 0, 0).reshape(-1, N_PAIRS)
    assert np.isnan(d).any() and np.isfinite(d).any()
    check_singletons(mean.reshape(-1, N_GP), used.reshape(-1, N_GP), d, "the sibling's means")
    # a window shorter than one block has no finite replicate
    off_gp = singleton_index()[0]
    assert np.all(gs[1][short] == 0) and np.all(gs[1][~short][:, off_gp].max(axis=1) == n_rep)
