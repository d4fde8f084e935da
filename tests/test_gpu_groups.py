"""Group-mean distance matrices reduced on the device (ngd_set_groups, ngd_group_means_device, ngd_run_*_groups;
group_reduce.hip k_group_means / k_group_finish).

The expected value never comes from the code under test: the call's host-sum sibling (run_windows, run_job, ...) gives sums
and counts, ngsdist_amd.finish (the host's libm) the cells, and math.fsum over the finite cells of a group pair the mean --
so only the new kernel is under test, not the accumulation.  Counts of finite cells must be equal exactly.  The means'
tolerance: a cell differs from the host's by the logs alone (1 ulp each by both libraries' documented accuracy, 2.2e-16
relative each), the blocked summation of non-negative terms adds at most (cells per thread + tree depth) roundings -- at
most 16 + 8 + 32 here -- so 3e-15 relative at most; the tests ask for 1e-13.  Where the division alone makes a cell
(evol_model 0, --tot_sites) a mean over one cell equals sum / cnt bit for bit.
Every comparison prints its largest relative error; the largest seen on an MI355X over every case of this file: 4.1e-16."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL = 1e-13


def N():
    import ngsdist_amd
    return ngsdist_amd


def synth(seed, n_ind, n_sites, miss_frac=0.0):
    from oracle import oracle as O
    return O.synth_indmajor(seed, n_ind, n_sites, miss_frac=miss_frac)


def group_pair_cells(g, G):
    """-> list over gp of the pair indices (the reference's pair order) of the group pair's cells"""
    g = np.asarray(g, dtype=np.int64)
    i1, i2 = np.triu_indices(len(g), 1)  # row-major upper triangle: the pair order
    a, b = np.minimum(g[i1], g[i2]), np.maximum(g[i1], g[i2])
    gp = np.where(a >= 0, a * G - a * (a - 1) // 2 + (b - a), -1)
    return [np.flatnonzero(gp == k) for k in range(G * (G + 1) // 2)]


def expected(S, Cn, g, G, model, tot=0):
    """host sums and counts [..., n_pairs] -> (mean, used) [..., n_gp]: finish() on the host, fsum over the finite cells"""
    S, Cn = np.asarray(S), np.asarray(Cn)
    lead = S.shape[:-1]
    d = N().finish(S.reshape(-1), Cn.reshape(-1), tot, model).reshape(-1, S.shape[-1])
    cells = group_pair_cells(g, G)
    mean = np.full((d.shape[0], len(cells)), np.nan)
    used = np.zeros((d.shape[0], len(cells)), dtype=np.uint64)
    for k, idx in enumerate(cells):
        v = d[:, idx]
        fin = np.isfinite(v)
        used[:, k] = fin.sum(axis=1)
        for m in np.flatnonzero(used[:, k]):
            mean[m, k] = math.fsum(v[m][fin[m]]) / int(used[m, k])
    return mean.reshape(lead + (-1,)), used.reshape(lead + (-1,))


def check(got, want, what=""):
    (gm, gu), (wm, wu) = got, want
    assert gm.shape == wm.shape and gu.shape == wu.shape, what
    assert np.array_equal(gu, wu), what
    nan = wu == 0
    assert np.array_equal(np.isnan(gm), nan), what
    # a positive quiet NaN where no cell is finite
    assert np.all(gm[nan].view(np.uint64) == 0x7FF8000000000000), what
    err = np.abs(gm[~nan] - wm[~nan]) / np.where(wm[~nan] == 0, 1.0, np.abs(wm[~nan]))
    worst = float(err.max()) if err.size else 0.0
    print("group means %s: largest relative error %.3g over %d means" % (what, worst, err.size))
    assert worst <= RTOL, (what, worst)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


# ---- 1. the smallest cases --------------------------------------------------------------------------------------------
def test_two_individuals_and_a_lone_member():
    p = synth(3, 3, 50)
    with N().Engine(2, 50, kernel="mfma") as e:
        e.upload_ind_major(p[:2]).commit().set_groups([0, 0])
        S, Cn = e.run_windows([0], [50])
        check(e.run_windows_groups([0], [50], evol_model=1), expected(S, Cn, [0, 0], 1, 1), "2 x 1 group")
    with N().Engine(3, 50, kernel="mfma") as e:
        e.upload_ind_major(p).commit().set_groups([1, 0, 1])
        S, Cn = e.run_windows([0, 10], [50, 20])
        got = e.run_windows_groups([0, 10], [50, 20], evol_model=2)
        check(got, expected(S, Cn, [1, 0, 1], 2, 2), "3 x 2 groups")
        # the lone member's diagonal: no cell
        assert np.all(np.isnan(got[0][:, 0])) and np.all(got[1][:, 0] == 0) and np.all(got[1][:, 1] == 2) and np.all(got[1][:, 2] == 1)


# ---- 2. nothing left out, some left out, NaN with used = 0: --pairwise_del on sparse data -----------------------------
@pytest.mark.parametrize("model", [0, 1, 2])
def test_pairwise_del_windows_leave_cells_out(model):
    n_ind, n_sites = 24, 200
    p = synth(7, n_ind, n_sites, miss_frac=0.5)
    g = np.arange(n_ind) % 3
    g[[5, 11]] = -1
    lo, hi = [0, 0, 1, 10, 50], [1, 200, 3, 14, 57]  # (window starts must not decrease: the whole data set comes second)
    with N().Engine(n_ind, n_sites, kernel="mfma", pairwise_del=True) as e:
        e.upload_ind_major(p).commit().set_groups(g, 3)
        S, Cn = e.run_windows(lo, hi)
        # what the CPU oracle gives on this data: the windows leave these many of the 276 cells out (no shared valid site)
        assert ((Cn == 0).sum(axis=1)).tolist() == [231, 0, 176, 126, 22]
        got = e.run_windows_groups(lo, hi, evol_model=model)
        want = expected(S, Cn, g, 3, model)
        check(got, want, "24 x 200 pairwise_del model %d" % model)
        gp22 = N().group_pair_index(3, 2, 2)
        assert got[1][0, gp22] == 0 and np.isnan(got[0][0, gp22])  # window [0, 1): group pair (2, 2) has no finite cell
        cells = N().group_cells(g, 3)
        assert np.all(got[1] <= cells)
        if model == 0:  # the division alone: every cell of the whole data set is finite, nothing is left out
            assert np.array_equal(got[1][1], cells)


# ---- 3. 130 individuals (across the 128 tile), the 49 unequal windows of test_gpu_windows_var.py ------------------------
def groupings(n):
    sizes = [7, 40, 1, 52, 30]
    contiguous = np.repeat(np.arange(5), sizes)
    interleaved = np.random.default_rng(2).permutation(contiguous)
    # group 3's members all have higher indices than group 4's: min / max of a cell's two individuals, not (row, column)
    high_low = np.concatenate([np.repeat([0, 1, 2], [7, 40, 1]), np.full(30, 4), np.full(52, 3)])
    return {"contiguous": contiguous, "interleaved": interleaved, "high_low": high_low}


@pytest.mark.parametrize("kernel", ["mfma", "em_table"])
def test_windows_and_window_jobs_against_their_siblings(kernel):
    import torch
    import test_gpu_windows_var as WV
    n_ind, n_rep, q = 130, 8, 7
    lo, hi = WV.bp_windows()
    maps, off = N().window_boot_maps(9, lo, hi, n_rep, q)
    p = synth(21, n_ind, WV.N_SITES)
    n_pairs, n_win = N().n_pairs(n_ind), len(lo)
    with N().Engine(n_ind, WV.N_SITES, kernel=kernel, indep_geno=kernel == "mfma") as e:
        e.upload_ind_major(p).commit()
        S, Cn = e.run_windows(lo, hi)
        SJ, CJ = e.run_windows_job_var(lo, hi, maps, off, q, n_rep=n_rep)
        ds = torch.empty((n_win, n_rep + 1, n_pairs), dtype=torch.float64, device="cuda")
        dc = torch.empty((n_win, n_rep + 1, n_pairs), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        for name, g in groupings(n_ind).items():
            e.set_groups(g, 5)
            got = e.run_windows_groups(lo, hi, evol_model=1)
            check(got, expected(S, Cn, g, 5, 1), "%s windows %s" % (kernel, name))
            gotj = e.run_windows_job_var_groups(lo, hi, maps, off, q, evol_model=1, n_rep=n_rep)
            check(gotj, expected(SJ, CJ, g, 5, 1), "%s window jobs %s" % (kernel, name))
            # the run form is group_means on the _device sibling's output, bit for bit
            e.run_windows_job_var(lo, hi, maps, off, q, d_sum_ptr=ds.data_ptr(), d_cnt_ptr=dc.data_ptr(), n_rep=n_rep)
            m, u = e.group_means(ds.data_ptr(), dc.data_ptr(), n_win * (n_rep + 1), evol_model=1)
            assert np.array_equal(bits(m), bits(gotj[0].reshape(m.shape))) and np.array_equal(u, gotj[1].reshape(u.shape)), name
            e.run_windows(lo, hi, d_sum_ptr=ds.data_ptr(), d_cnt_ptr=dc.data_ptr())
            m, u = e.group_means(ds.data_ptr(), dc.data_ptr(), n_win, evol_model=1)
            assert np.array_equal(bits(m), bits(got[0])) and np.array_equal(u, got[1]), name
        # 7. determinism: two calls give equal bits; one window alone carries the bits it has among the 49 (the reduction
        # alone: group_means on identical device sums, all at once and window 17's matrix by itself)
        again = e.run_windows_groups(lo, hi, evol_model=1)
        assert np.array_equal(bits(again[0]), bits(got[0])) and np.array_equal(again[1], got[1])
        fs, fc = ds.view(-1, n_pairs), dc.view(-1, n_pairs)  # (the windows' matrices lie one after the other from the start)
        one = e.group_means(fs[17].data_ptr(), fc[17].data_ptr(), 1, evol_model=1)
        assert np.array_equal(bits(one[0][0]), bits(m[17])) and np.array_equal(one[1][0], u[17])


# ---- bit-exact: every individual its own group, one cell per mean, no log ----------------------------------------------
@pytest.mark.parametrize("tot_sites,model", [(0, 0), (1234, 0), (1000, 1)])
def test_one_cell_means_are_the_division_bit_for_bit(tot_sites, model):
    n_ind, n_sites = 24, 300
    p = synth(8, n_ind, n_sites, miss_frac=0.1)
    lo, hi = [0, 37, 100], [300, 38, 200]
    with N().Engine(n_ind, n_sites, kernel="mfma", pairwise_del=not tot_sites) as e:
        e.upload_ind_major(p).commit().set_groups(np.arange(n_ind))
        S, Cn = e.run_windows(lo, hi)
        mean, used = e.run_windows_groups(lo, hi, evol_model=model, tot_sites=tot_sites)
        off = np.array([N().group_pair_index(n_ind, a, b) for a in range(n_ind) for b in range(a + 1, n_ind)])
        diag = np.array([N().group_pair_index(n_ind, a, a) for a in range(n_ind)])
        assert np.all(used[:, diag] == 0) and np.all(np.isnan(mean[:, diag]))
        d = N().finish(S.reshape(-1), Cn.reshape(-1), tot_sites, model).reshape(S.shape)
        fin = np.isfinite(d)
        assert np.array_equal(used[:, off], fin.astype(np.uint64))
        if model == 0:  # the division alone: the host's bits
            with np.errstate(all="ignore"):
                want = S / (np.float64(tot_sites) if tot_sites else Cn.astype(np.float64))
            assert np.array_equal(bits(mean[:, off][fin]), bits(want[fin]))
        else:  # one log: the two libraries' 1 ulp each
            assert np.all(np.abs(mean[:, off][fin] - d[fin]) <= 4.5e-16 * np.abs(d[fin]))
        # G = 1, everyone in the group: used = the finite cells
        e.set_groups(np.zeros(n_ind, dtype=np.int32))
        m1, u1 = e.run_windows_groups(lo, hi, evol_model=model, tot_sites=tot_sites)
        assert np.array_equal(u1[:, 0], fin.sum(axis=1).astype(np.uint64))
        check((m1, u1), expected(S, Cn, np.zeros(n_ind, dtype=int), 1, model, tot_sites), "G = 1")


# ---- 4. the replicate loop ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["mfma", "em_table"])
def test_run_job_groups(kernel):
    n_ind, n_sites, n_rep, q = 65, 400, 40, 7
    p = synth(13, n_ind, n_sites)
    t = N().Taus(5)
    maps = np.stack([t.block_map(n_sites // q) for _ in range(n_rep)])
    g = np.arange(n_ind) % 4
    g[3] = -1
    with N().Engine(n_ind, n_sites, kernel=kernel, indep_geno=kernel == "mfma") as e:
        e.upload_ind_major(p).commit().set_groups(g, 4)
        e.set_option("boot_partials", 0)  # (pins the plan: two calls of a job then agree bit for bit, include/ngsdist_amd.h)
        S, Cn = e.run_job(maps, q)
        got = e.run_job_groups(maps, q, evol_model=2)
        assert got[0].shape == (n_rep + 1, 10)
        check(got, expected(S, Cn, g, 4, 2), "%s job" % kernel)
        s0, c0 = e.fetch_matrix(n_rep)  # the matrices stay in the engine
        assert np.array_equal(bits(s0), bits(S[n_rep])) and np.array_equal(c0, Cn[n_rep])
        S0, C0 = e.run()
        check(e.run_job_groups(None, evol_model=2), expected(S0[None], C0[None], g, 4, 2), "%s full data alone" % kernel)


# ---- 5. a group pair larger than a work item, and rows that are split --------------------------------------------------
def test_a_group_pair_split_over_many_workgroups():
    n_ind, n_sites = 700, 64
    g = np.repeat([0, 1], 350)
    with N().Engine(n_ind, n_sites, kernel="mfma") as e:
        e.synth_fill(17).commit().set_groups(g)
        S, Cn = e.run_windows([0, 5], [64, 40])
        check(e.run_windows_groups([0, 5], [64, 40], evol_model=1), expected(S, Cn, g, 2, 1), "700 x 2 groups")
        e.set_groups(np.arange(n_ind) % 2)
        check(e.run_windows_groups([0, 5], [64, 40], evol_model=1), expected(S, Cn, np.arange(n_ind) % 2, 2, 1), "700 interleaved")


# ---- 6. more matrices than a grid dimension holds ------------------------------------------------------------------------
def test_more_matrices_than_grid_y():
    import torch
    n_mat = 70_000
    rng = np.random.default_rng(4)
    S = rng.random((n_mat, 3)) + 0.01
    Cn = rng.integers(0, 4, (n_mat, 3)).astype(np.uint64)
    ds = torch.from_numpy(S).to("cuda")
    dc = torch.from_numpy(Cn.astype(np.int64)).to("cuda")
    torch.cuda.synchronize()
    with N().Engine(3, 16, kernel="mfma") as e:
        e.synth_fill(1).commit().set_groups([0, 1, 1])
        got = e.group_means(ds.data_ptr(), dc.data_ptr(), n_mat, evol_model=0)
        check(got, expected(S, Cn, [0, 1, 1], 2, 0), "70 000 matrices")
        assert got[1][:, 0].max() == 0 and 0 < got[1][:, 1].mean() < 2  # counts of 0: inf or NaN cells, left out


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_engine_usable():
    n_ind, n_sites = 10, 64
    with N().Engine(n_ind, n_sites, kernel="mfma", pairwise_del=True) as e:
        e.synth_fill(2, 0.1).commit()
        with pytest.raises(N().NgdError) as ei:
            e.run_windows_groups([0], [64])
        assert ei.value.code == -1 and "no grouping set" in str(ei.value)
        e.run_windows([0], [64])  # (the batch buffers and the windows' scratch exist from here on)
        base = e.device_bytes()
        for bad, G in (([0] * 9 + [2], 2), ([0] * 9 + [-2], 2), ([0] * 10, 0)):
            with pytest.raises(N().NgdError) as ei:
                e.set_groups(bad, G)
            assert ei.value.code == -1
        e.set_groups(np.arange(n_ind) % 2)
        assert e.device_bytes() > base
        for kw, code in ((dict(evol_model=3), -5), (dict(tot_sites=50), -1)):
            with pytest.raises(N().NgdError) as ei:
                e.run_windows_groups([0], [64], **kw)
            assert ei.value.code == code
            with pytest.raises(N().NgdError) as ei:
                e.run_job_groups(None, **kw)
            assert ei.value.code == code
        with pytest.raises(N().NgdError):
            e.run_windows_groups([5], [5])  # the sibling's refusal: an empty window
        with pytest.raises(N().NgdError):
            e.set_groups([0] * 9 + [7], 2)  # a refused grouping leaves the one before it
        S, Cn = e.run_windows([0], [64])
        check(e.run_windows_groups([0], [64], evol_model=1), expected(S, Cn, np.arange(n_ind) % 2, 2, 1), "after refusals")
        e.set_groups(None)
        assert e.device_bytes() == base
        with pytest.raises(N().NgdError):
            e.run_job_groups(None)
    with N().Engine(n_ind, n_sites, kernel="mfma", shard_rank=0, shard_world=2) as e:
        e.synth_fill(2).commit().set_groups(np.arange(n_ind) % 2)
        with pytest.raises(N().NgdError) as ei:
            e.run_job_groups(None)
        assert ei.value.code == -1 and "share of the pairs" in str(ei.value)
