"""Classical MDS on the device (mds.hip k_mds, engine_mds.hip) where test_gpu_mds.py's matrices and shapes do not go.

a. The matrices of test_mds_edges_cpu.py -- few distinct rows, pairs of eigenvalues 1e-4 .. 0 apart, cells times a power of
   two, the matrix that is tridiagonal as it stands -- through ngd_mds_values_device, by the same checks against numpy
   (bounds: 1e-9 relative to S = max |eigenvalue|; 1e-9 for orthonormality and the subspace figure), and against the host
   twin (statuses equal, eigenvalues within 1e-9 S).
b. The realistic door: an engine whose 130 individuals are bit-identical copies of three, windows of 1, 2 and 64 sites
   through ngd_run_windows_mds, checked against numpy on the _dist sibling's matrix of the same window.
c. Cells that are not finite in the sums-and-counts form (k_mds<false>): a NaN from the logarithm under model 2 alone, under
   models 1 and 2, a count of 0.
d. A call cut into chunks of whole rounds of the CUs (mds_reduce's `chunk -= chunk % n_cu`).
e. Windows in several batches behind the MDS tail, and (f) in several groups of windows, where the tail writes at an offset
   that the group's first window decides (the hook of test_gpu_tail_groups_of_windows.py).
g. The workgroups of 256 and 512 threads (NGD_MDS_WG) at n = 1153, where every thread-strided loop makes 5 and 3 trips;
   no bit equality with the default is asked for: the sums' trees follow the workgroup.
The cap n = 4096 is left out on purpose: k_mds takes several seconds a matrix there (120 ms at n = 1000, growing with n^3),
and numpy's eigh as long again.

Every comparison prints its largest figure in units of its bound.  The largest seen on an MI355X over this file, as fractions
of S (of 1 for orthonormality, the dot product and the subspace figure; bound 1e-9 each): duplicates -- eigenvalues 2.2e-15,
residuals 2.1e-15, totals 4.3e-15 of the sum of |eigenvalue|, orthonormality 7.2e-15, device against host twin 1.5e-14 --;
near-degenerate -- eigenvalues against the planted ones 8.9e-16, against numpy's 1.2e-15, residuals 9.0e-16, orthonormality
6.7e-16, the subspace figure 6.7e-16, against the host twin 1.4e-15 --; the windows of (b) residuals 6.4e-16, orthonormality
2.5e-15; the planted sums of (c) 8.9e-16; n = 1153 with 256 and 512 threads eigenvalues 2.2e-16, residuals 8.0e-16, totals
1.3e-15, orthonormality 8.9e-16, the planted distances 1.4e-15 of the largest.  (e) makes 3 batches against 2.

With the kernel's reflector as it was before its norm was taken from a scaled row (one run of this file against a build
that held that change back) the duplicates cases failed on the device at every size, n = 64 included, where the host twin
still passed -- orthonormality alone, eigenvalues, residuals and totals staying within 5e-15: the largest max |V V^T - I|
3.3e-2 (n = 130, two sites, K = 16), at n = 64 1.3e-3 (K = 4) and 1.2e-2 (K = 16) on the prototypes; K = 1 passed
everywhere -- and the cells times 2^k changed bits on the duplicates matrices at n = 64, 130 and 257.  Everything else in
this file passed on that build too, (b) excepted, which was not run on it."""
import numpy as np
import pytest

import mds_expect as X
from test_gpu_mds import N, bits, check_finished, device_buffers, finish, on_device, same, synth
from test_mds_edges_cpu import SCALES, check_duplicates, check_exact, check_near_degenerate, check_scaled, scaled_cases

pytestmark = pytest.mark.gpu


def engine(n):
    e = N().Engine(n, 16, kernel="mfma")
    e.synth_fill(1).commit()
    return e


def against_host(v, n, K, got, what):
    """statuses equal and eigenvalues within 1e-9 S of the host twin's; -> the largest difference in units of the bound"""
    heig, _, _, hstatus = N().mds_host(v, n, K)
    assert np.array_equal(got[3], hstatus), what
    S = np.array([np.abs(X.spectrum(v[m], n)[1]).max() for m in range(len(v))])
    worst = (np.abs(got[0] - heig).max(axis=1) / np.where(S > 0, S, 1.0)).max() / X.TOL
    print("%s: device against host twin: eigenvalues differ by %.3g of the bound" % (what, worst))
    assert worst <= 1, what
    return worst


def rows(t, m):
    """matrix m of an (eig, vec, tot, status) tuple"""
    return tuple(x[m] for x in t)


# ---- a. the matrices of test_mds_edges_cpu.py ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 96, 128, 130, 256, 257])
def test_duplicates_against_numpy_and_the_host_twin(n):
    v = X.duplicates(n)
    with engine(n) as e:
        got = {K: on_device(e, v, K) for K in (1, 4, 16)}
    failed = []
    for K, g in got.items():
        try:
            check_duplicates(v, n, K, g, "device")
        except AssertionError as err:  # (every K is shown before the test fails)
            failed.append("K=%d: %s" % (K, err))
        against_host(v, n, K, g, "duplicates n=%d K=%d" % (n, K))
    assert not failed, "; ".join(failed)


@pytest.mark.parametrize("n", [5, 64, 65, 257])
def test_near_degenerate_pairs_by_planted_eigenvalues_and_subspaces(n):
    K = 4  # (n - 1 at n = 5)
    v = np.stack([X.near_degenerate(n, gap) for gap in X.GAPS])
    with engine(n) as e:
        got = on_device(e, v, K)
    for m, gap in enumerate(X.GAPS):
        check_near_degenerate(v[m], n, gap, K, rows(got, m), "device")
    against_host(v, n, K, got, "near-degenerate n=%d" % n)


@pytest.mark.parametrize("n", [5, 64, 130, 257])
def test_cells_times_a_power_of_two_change_no_bit(n):
    with engine(n) as e:
        for name, v in scaled_cases(n):
            for K in sorted({min(4, n - 1), min(16, n - 1)}):
                base = on_device(e, v, K)
                for k in SCALES:
                    check_scaled(base, on_device(e, v * 2.0 ** k, K), k, "%s n=%d K=%d k=%d" % (name, n, K, k))


@pytest.mark.parametrize("n", [4, 64, 128])
def test_a_matrix_that_is_tridiagonal_as_it_stands(n):
    """every step the H = I arm, every reflector skipped on the way back"""
    v = X.duplicates(n)[X.DUP["exact"]][None]
    with engine(n) as e:
        for K in sorted({1, min(4, n - 1), min(16, n - 1)}):
            check_exact(n, K, rows(on_device(e, v, K), 0))


# ---- b. the realistic door: clones in the data, windows of one and two sites ------------------------------------------------
@pytest.mark.parametrize("kernel", ["mfma", "em_table"])
def test_windows_of_an_engine_whose_individuals_are_copies_of_three(kernel):
    n_ind, n_sites, K = 130, 64, 4
    p = np.ascontiguousarray(synth(41, 3, n_sites)[np.arange(n_ind) % 3])  # bit-identical rows
    lo, hi = np.array([0, 0, 30]), np.array([1, 64, 32])
    with N().Engine(n_ind, n_sites, kernel=kernel, indep_geno=kernel == "mfma") as e:
        e.upload_ind_major(p).commit()
        eig, vec, tot, status, dist0 = e.run_windows_mds(K, lo, hi, evol_model=0)
        dist = e.run_windows_dist(lo, hi, 0)
    assert np.array_equal(bits(dist0), bits(dist)) and np.all(np.isfinite(dist)) and np.all(status == 1)
    for w in range(len(lo)):
        fig = X.check_matrix(dist[w], n_ind, K, eig[w, 0], vec[w, 0], tot[w, 0], sign=True)
        print("%s window [%d, %d): largest figures in units of 1e-9: %s" % (kernel, lo[w], hi[w], {k: "%.3g" % x for k, x in fig.items()}))


# ---- c. cells that are not finite in the sums-and-counts form ----------------------------------------------------------------
def test_cells_that_are_not_finite_in_sums_and_counts_leave_the_other_matrices_alone():
    import torch
    n, K = 130, 4
    p = n * (n - 1) // 2
    rng = np.random.default_rng(n)
    Cn = rng.integers(50, 400, (4, p)).astype(np.uint64)
    S = rng.uniform(0.05, 0.6, (4, p)) * Cn
    S[2, -1] = 0.8 * Cn[2, -1]   # pair (n - 2, n - 1) of matrix 2: 1 - 0.8 * 4 / 3 < 0 and 1 - 0.8 > 0: model 2 alone
    S[1, 0] = 1.25 * Cn[1, 0]    # pair (0, 1) of matrix 1: 1 - 1.25 < 0 under model 1 as well
    Cn[3, p // 2] = 0            # matrix 3: a pair without a site, under every model
    want = {0: [1, 1, 1, 0], 1: [1, 0, 1, 0], 2: [1, 0, 0, 0]}
    with N().Engine(n, 16) as e:
        e.synth_fill(1).commit()
        ds, dc = device_buffers(S.shape)
        ds.copy_(torch.from_numpy(S))
        dc.copy_(torch.from_numpy(Cn.astype(np.int64)))
        torch.cuda.synchronize()
        for model in (0, 1, 2):
            d = finish(S, Cn, model)
            assert np.isfinite(d).all(axis=1).astype(int).tolist() == want[model]  # (the statuses are ngd_finish's)
            got = e.mds(ds.data_ptr(), dc.data_ptr(), 4, K, evol_model=model)
            assert got[3].tolist() == want[model], model
            for m in range(4):
                alone = e.mds(ds[m].data_ptr(), dc[m].data_ptr(), 1, K, evol_model=model)
                assert same(alone, rows(got, [m])), (model, m)
                if not want[model][m]:
                    X.check_bad(got[0][m], got[1][m], got[2][m], got[3][m])
            good = [m for m in range(4) if want[model][m]]
            check_finished(rows(got, good), d[good], n, K, "planted sums with cells that are not finite, model %d" % model)


# ---- d. chunks of whole rounds of the CUs -----------------------------------------------------------------------------------
def test_chunks_of_whole_cu_rounds_change_no_bit():
    import torch
    n, K = 5, 2
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    n_mat = 2 * n_cu + 200
    v = np.random.default_rng(5).uniform(0.05, 1.5, size=(n_mat, n * (n - 1) // 2))
    with engine(n) as e:
        whole = on_device(e, v, K)
        # a matrix's scratch is (5 + 4 K) rows of 6 doubles: n_cu + 44 matrices fit, rounded down to n_cu -- three launches,
        # the last one of 200 matrices
        e.set_option("mds_max_bytes", (n_cu + 44) * (n + 4 * K) * 6 * 8)
        cut = on_device(e, v, K)
    assert 200 < n_cu + 44 < n_mat
    assert cut[0].shape == (n_mat, K) and np.all(cut[3] == 1) and same(cut, whole)
    # the matrices are random: an output at a wrong offset is another matrix's
    assert len({bits(x).tobytes() for x in cut[0]}) == n_mat
    against_host(v, n, K, cut, "%d matrices in chunks of %d" % (n_mat, n_cu))


# ---- e. windows in several batches behind the tail ---------------------------------------------------------------------------
N_IND, N_SITES, N_REP, Q = 24, 440, 4, 5
LO = 10 * np.arange(40)
HI = LO + 40


def window_job():
    maps, off = N().window_boot_maps(7, LO, HI, N_REP, Q)
    return synth(19, N_IND, N_SITES), maps, off


def test_windows_in_several_batches_behind_the_tail():
    """40 windows x 5 matrices under the segment-slab plan.  The windows' ends cut the sites into 43 segments, the blocks of
    5 sites into 86 slices: a budget of 60 planes (n_pad = 128) leaves the matrices 0 one batch and cuts the replicates'
    slab, whose slices are the same wherever it is cut"""
    K = 4
    p, maps, off = window_job()
    n_pairs, n_win = N().n_pairs(N_IND), len(LO)
    with N().Engine(N_IND, N_SITES, kernel="mfma", indep_geno=True, single_image=3) as e:
        e.upload_ind_major(p).commit()
        e.set_option("win_plan", 2)
        whole = e.run_windows_job_var_mds(K, LO, HI, maps, off, Q, evol_model=0, n_rep=N_REP)
        unbudgeted = e.windows_info()["batches"]
        e.set_option("win_max_bytes", 60 * 128 * 128 * 8 + (1 << 20))
        small = e.run_windows_job_var_mds(K, LO, HI, maps, off, Q, evol_model=0, n_rep=N_REP)
        batches = e.windows_info()["batches"]
        print("%d batches under the small budget, %d without" % (batches, unbudgeted))
        assert batches > unbudgeted
        ds, dc = device_buffers((n_win, N_REP + 1, n_pairs))
        e.run_windows_job_var(LO, HI, maps, off, Q, d_sum_ptr=ds.data_ptr(), d_cnt_ptr=dc.data_ptr(), n_rep=N_REP)
        sibling = e.mds(ds.data_ptr(), dc.data_ptr(), n_win * (N_REP + 1), K, evol_model=0)
    assert small[0].shape == (n_win, N_REP + 1, K) and np.all(small[3] == 1)
    assert same(small[:4], whole[:4]) and np.array_equal(bits(small[4]), bits(whole[4]))
    assert same(small[:4], sibling)


# ---- f. ... and in several groups of windows: the tail's offsets -------------------------------------------------------------
def test_windows_in_several_groups_behind_the_tail(monkeypatch):
    """Under the per-window plan a window's matrices do not depend on the windows beside it; the hook cuts the call into
    groups of 3 windows (14 groups, the last one of 1), and the tail of every group but the first writes at an offset"""
    K, per_group = 4, 3
    p, maps, off = window_job()
    n_pairs = N().n_pairs(N_IND)
    with N().Engine(N_IND, N_SITES, kernel="mfma", indep_geno=True) as e:
        e.upload_ind_major(p).commit()
        e.set_option("win_plan", 1)
        calls = [(1, lambda: e.run_windows_mds(K, LO, HI, evol_model=0)),
                 (N_REP + 1, lambda: e.run_windows_job_var_mds(K, LO, HI, maps, off, Q, evol_model=0, n_rep=N_REP))]
        for n_mat, call in calls:
            monkeypatch.delenv("NGD_ENABLE_TEST_HOOKS", raising=False)
            monkeypatch.delenv("NGD_TEST_WIN_GROUP_BYTES", raising=False)
            whole = call()
            monkeypatch.setenv("NGD_ENABLE_TEST_HOOKS", "1")
            monkeypatch.setenv("NGD_TEST_WIN_GROUP_BYTES", str(per_group * 16 * n_mat * n_pairs))
            cut = call()
            assert np.all(whole[3] == 1)
            assert same(cut[:4], whole[:4]) and np.array_equal(bits(cut[4]), bits(whole[4])), n_mat
            # the windows differ: an output at a wrong offset is another window's
            assert len({bits(x).tobytes() for x in whole[0][:, 0]}) == len(LO)


# ---- g. the small workgroups on long rows --------------------------------------------------------------------------------------
@pytest.mark.parametrize("wg", [256, 512])
def test_the_small_workgroups_on_rows_of_several_trips(wg, monkeypatch):
    n, K = 1153, 4
    v = X.few(n)  # a random matrix, a planted one, one with a NaN cell
    monkeypatch.setenv("NGD_MDS_WG", str(wg))
    with engine(n) as e:
        eig, vec, tot, status = on_device(e, v, K)
    assert status.tolist() == [1, 1, 0]
    X.check_bad(eig[2], vec[2], tot[2], status[2])
    for m in (0, 1):
        fig = X.check_matrix(v[m], n, K, eig[m], vec[m], tot[m])
        print("device, %d threads, n=%d matrix %d: largest figures in units of 1e-9: %s" % (wg, n, m, {k: "%.3g" % x for k, x in fig.items()}))
    X.check_planted(v[1], n, N().mds_coords(eig[1], vec[1]))
