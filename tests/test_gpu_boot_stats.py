"""Bootstrap summaries per cell reduced on the device (ngd_boot_stats*_device, ngd_run_*_stats; boot_stats.hip k_boot_stats).

The expected value never comes from the code under test, nor from the host function (test_boot_stats_cpu.py checks that one
against the same numpy statement, boot_stats_expect.py): values as they are go through numpy directly; sums and counts come
from the call's host-sum sibling (run_job, run_windows_job_var) or from the tensors a *_device sibling filled, go through
ngsdist_amd.finish (the host's libm) and then through numpy.
Tolerances.  Values as they are, and sums and counts under evol_model 0 (the division carries the host's bits): est, mean,
lo, hi equal as values, used equal, sd within 4 ulp (a division and a square root after equal sums).  Models 1 and 2: a
cell differs from the host's by the logs alone, 1 ulp each by both libraries' documented accuracy, so est, lo, hi (near
ties may swap, the values stay that close) and the mean of such cells get RTOL = 1e-13 as in test_gpu_groups.py, and sd
gets 1e-12 sd + 64 m 2^-53 |mean|: two-pass deviations carry m roundings of the mean's magnitude.  used is exact: a cell is
finite or not by sum / cnt and 1 - d (1 - d 4 / 3), which carry the host's bits; the tests assert that no finite cell is
near overflow.
Every comparison prints its largest error.  The largest seen on an MI355X over every case of this file: relative error of
est / mean / lo / hi under models 1 and 2 5.55e-16 (bound 1e-13); sd at 0.0042 of its bound; where equality is asked, sd
0 ulp from numpy's (bound 4) and everything else equal."""
import ctypes as C

import numpy as np
import pytest

import boot_stats_expect as X

pytestmark = pytest.mark.gpu


def N():
    import ngsdist_amd
    return ngsdist_amd


def synth(seed, n_ind, n_sites, miss_frac=0.0):
    from oracle import oracle as O
    return O.synth_indmajor(seed, n_ind, n_sites, miss_frac=miss_frac)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a[0]).ravel(), bits(b[0]).ravel()) and np.array_equal(a[1].ravel(), b[1].ravel())


def from_sums(S, Cn, model, tot=0, ci=0.95):
    """host sums and counts [..., n_mat, n_cells] -> the expected (stats, used): finish() on the host, then numpy"""
    S, Cn = np.asarray(S), np.asarray(Cn).astype(np.uint64)
    with np.errstate(all="ignore"):
        d = N().finish(S.reshape(-1), Cn.reshape(-1), tot, model).reshape(S.shape)
    assert np.all(np.abs(d[np.isfinite(d)]) < 1e300)  # finiteness hangs on no last ulp
    return X.expect(d, ci)


def check_sums(got, S, Cn, model, what, tot=0, ci=0.95):
    want = from_sums(S, Cn, model, tot, ci)
    if model == 0:
        X.check_exact(got, want, what)
    else:
        X.check_close(got, want, what)


@pytest.fixture(scope="module")
def small_engine():
    with N().Engine(3, 16, kernel="mfma") as e:
        e.synth_fill(1).commit()
        yield e


def values_on_device(e, v, ci=0.95):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(v)).to("cuda")
    torch.cuda.synchronize()
    n_set, n_mat, n_cells = v.shape
    return e.boot_stats_values(t.data_ptr(), n_set, n_mat, n_cells, ci)


# ---- 1. values as they are: the planted arrays of the CPU test, 130 cells = one past two 64-lane tiles --------------------
@pytest.mark.parametrize("n_rep", [1, 2, 3, 100])
def test_values_form_on_planted_arrays(small_engine, n_rep):
    for ci in (0.95, 0.5):
        v = X.planted(3, n_rep, 130, seed=n_rep)
        got = values_on_device(small_engine, v, ci)
        X.check_exact(got, X.expect(v, ci), "values R = %d ci %g" % (n_rep, ci))
    assert small_engine.last_boot_stats_ms() > 0


# ---- 2. one R per tile width: the largest each of C = 64, 32, 16 serves (a tile is [R + 1][C] doubles in 160 KiB) ---------
def tile_arms():
    n_mat16 = N().boot_stats_max_rep() + 1  # the narrowest tile's
    return {64: n_mat16 // 4 - 1, 32: n_mat16 // 2 - 1, 16: n_mat16 - 1}


@pytest.mark.parametrize("width", [64, 32, 16])
def test_the_largest_r_of_every_tile_width(small_engine, width):
    n_rep = tile_arms()[width]
    assert (n_rep + 1) * width * 8 <= 160 * 1024 < (n_rep + 2) * width * 8
    v = X.planted(2, n_rep, 70, seed=width)  # column 9 holds every special value at once
    got = values_on_device(small_engine, v)
    X.check_exact(got, X.expect(v), "tile width %d, R = %d" % (width, n_rep))
    # a set served alone carries the bits it has among two
    one = values_on_device(small_engine, v[1:])
    assert same_bits((one[0][0], one[1][0]), (got[0][1], got[1][1]))


def test_one_replicate_past_the_cap_is_refused(small_engine):
    import torch
    e, L = small_engine, small_engine._L
    n_mat, n_cells = N().boot_stats_max_rep() + 2, 5
    t = torch.zeros((n_mat, n_cells), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    stats, used = np.full((5, n_cells), -7.0), np.full(n_cells, 77, dtype=np.uint64)
    sp, up = stats.ctypes.data_as(C.POINTER(C.c_double)), used.ctypes.data_as(C.POINTER(C.c_uint64))
    assert L.ngd_boot_stats_values_device(e._h, C.c_void_p(t.data_ptr()), 1, n_mat, n_cells, 0.95, sp, up) == -1
    assert "ngd_boot_stats_max_rep" in L.ngd_last_error().decode()
    assert np.all(stats == -7.0) and np.all(used == 77)
    assert L.ngd_boot_stats_values_device(e._h, C.c_void_p(t.data_ptr()), 1, n_mat - 1, n_cells, 0.95, sp, up) == 0
    assert np.all(stats == 0.0) and np.all(used == n_mat - 2)


# ---- 3. sums and counts: --pairwise_del on sparse data, windows of 1 to 200 sites, one shorter than a block ------------
@pytest.mark.parametrize("model", [0, 1, 2])
def test_sums_and_counts_form_pairwise_del(model):
    import torch
    n_ind, n_sites, n_rep, q = 24, 200, 8, 5
    p = synth(7, n_ind, n_sites, miss_frac=0.5)
    lo, hi = np.array([0, 0, 1, 10, 50, 60]), np.array([1, 200, 3, 14, 57, 160])  # [0, 1), [1, 3), [10, 14): shorter than a block
    maps, off = N().window_boot_maps(3, lo, hi, n_rep, q)
    n_pairs, n_win = N().n_pairs(n_ind), len(lo)
    with N().Engine(n_ind, n_sites, kernel="mfma", pairwise_del=True) as e:
        e.upload_ind_major(p).commit()
        ds = torch.empty((n_win, n_rep + 1, n_pairs), dtype=torch.float64, device="cuda")
        dc = torch.empty((n_win, n_rep + 1, n_pairs), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        e.run_windows_job_var(lo, hi, maps, off, q, d_sum_ptr=ds.data_ptr(), d_cnt_ptr=dc.data_ptr(), n_rep=n_rep)
        torch.cuda.synchronize()
        S, Cn = ds.cpu().numpy(), dc.cpu().numpy().astype(np.uint64)
        assert (Cn[:, 0] == 0).any() and (Cn[1, 0] > 0).all()  # some counts are 0
        got = e.boot_stats(ds.data_ptr(), dc.data_ptr(), n_win, n_rep + 1, evol_model=model)
        check_sums(got, S, Cn, model, "24 x 200 pairwise_del model %d" % model)
        assert np.all(got[1][[0, 2, 3]] == 0) and np.all(np.isnan(got[0][[0, 2, 3], 1:]))  # no block: m = 0
        assert got[1][1].max() == n_rep
        # the host-sum sibling gives the same sums, so the same expectation
        SH, CH = e.run_windows_job_var(lo, hi, maps, off, q, n_rep=n_rep)
        check_sums(got, SH, CH, model, "... against the host-sum sibling")
        # the run form is boot_stats on the _device sibling's output, bit for bit
        run = e.run_windows_job_var_stats(lo, hi, maps, off, q, evol_model=model, n_rep=n_rep)
        assert same_bits(run, got)


def test_sums_and_counts_form_tot_sites():
    """--tot_sites: d_cnt is not read (a null pointer here), the division by the total carries the host's bits"""
    import torch
    n_ind, n_sites, n_rep, q = 24, 200, 8, 5
    p = synth(8, n_ind, n_sites)
    t = N().Taus(5)
    maps = np.stack([t.block_map(n_sites // q) for _ in range(n_rep)])
    n_pairs = N().n_pairs(n_ind)
    with N().Engine(n_ind, n_sites, kernel="mfma") as e:
        e.upload_ind_major(p).commit()
        e.set_option("boot_partials", 0)
        ds = torch.empty((n_rep + 1, n_pairs), dtype=torch.float64, device="cuda")
        dc = torch.empty((n_rep + 1, n_pairs), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        e.run_job(maps, q, d_sum_ptr=ds.data_ptr(), d_cnt_ptr=dc.data_ptr())
        torch.cuda.synchronize()
        S, Cn = ds.cpu().numpy(), dc.cpu().numpy().astype(np.uint64)
        got = e.boot_stats(ds.data_ptr(), None, 1, n_rep + 1, evol_model=0, tot_sites=1234)
        X.check_exact(got, from_sums(S[None], Cn[None], 0, 1234), "tot_sites model 0")
        got = e.boot_stats(ds.data_ptr(), None, 1, n_rep + 1, evol_model=2, tot_sites=1234, ci=0.8)
        X.check_close(got, from_sums(S[None], Cn[None], 2, 1234, 0.8), "tot_sites model 2")


# ---- 4. the run forms against their siblings ------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["mfma", "em_table"])
def test_run_job_stats(kernel):
    import torch
    n_ind, n_sites, n_rep, q = 65, 400, 8, 7
    p = synth(13, n_ind, n_sites)
    t = N().Taus(5)
    maps = np.stack([t.block_map(n_sites // q) for _ in range(n_rep)])
    n_pairs = N().n_pairs(n_ind)
    with N().Engine(n_ind, n_sites, kernel=kernel, indep_geno=kernel == "mfma") as e:
        e.upload_ind_major(p).commit()
        e.set_option("boot_partials", 0)  # (pins the plan: two calls of a job then agree bit for bit)
        S, Cn = e.run_job(maps, q)
        got = e.run_job_stats(maps, q, evol_model=1)
        assert got[0].shape == (5, n_pairs) and got[1].shape == (n_pairs,)
        s0, c0 = e.fetch_matrix(n_rep)  # the matrices stay in the engine
        assert np.array_equal(bits(s0), bits(S[n_rep])) and np.array_equal(c0, Cn[n_rep])
        check_sums((got[0][None], got[1][None]), S[None], Cn[None], 1, "%s job" % kernel)
        ds = torch.empty((n_rep + 1, n_pairs), dtype=torch.float64, device="cuda")
        dc = torch.empty((n_rep + 1, n_pairs), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        e.run_job(maps, q, d_sum_ptr=ds.data_ptr(), d_cnt_ptr=dc.data_ptr())
        dev = e.boot_stats(ds.data_ptr(), dc.data_ptr(), 1, n_rep + 1, evol_model=1)
        assert same_bits((dev[0][0], dev[1][0]), got)


@pytest.mark.parametrize("kernel", ["mfma", "em_table"])
def test_window_jobs_groups_and_batches_against_their_siblings(kernel):
    import torch
    import test_gpu_groups as TG
    import test_gpu_windows_var as WV
    n_ind, n_rep, q = 130, 8, 7
    lo, hi = WV.bp_windows()
    maps, off = N().window_boot_maps(9, lo, hi, n_rep, q)
    p = synth(21, n_ind, WV.N_SITES)
    n_pairs, n_win = N().n_pairs(n_ind), len(lo)
    cfg = dict(indep_geno=True, single_image=3) if kernel == "mfma" else dict(indep_geno=False)  # (two operand images: the slab plan applies)
    with N().Engine(n_ind, WV.N_SITES, kernel=kernel, **cfg) as e:
        e.upload_ind_major(p).commit()
        SJ, CJ = e.run_windows_job_var(lo, hi, maps, off, q, n_rep=n_rep)
        got = e.run_windows_job_var_stats(lo, hi, maps, off, q, evol_model=1, n_rep=n_rep)
        bytes0 = e.device_bytes()
        assert got[0].shape == (n_win, 5, n_pairs) and got[1].shape == (n_win, n_pairs)
        check_sums(got, SJ, CJ, 1, "%s window jobs" % kernel)
        short = (hi - lo) // q == 0
        assert short.sum() == 8 and np.all(got[1][short] == 0) and np.all(got[1][~short] == n_rep)
        ds = torch.empty((n_win, n_rep + 1, n_pairs), dtype=torch.float64, device="cuda")
        dc = torch.empty((n_win, n_rep + 1, n_pairs), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        e.run_windows_job_var(lo, hi, maps, off, q, d_sum_ptr=ds.data_ptr(), d_cnt_ptr=dc.data_ptr(), n_rep=n_rep)
        dev = e.boot_stats(ds.data_ptr(), dc.data_ptr(), n_win, n_rep + 1, evol_model=1)
        assert same_bits(dev, got)
        # one window's set alone carries the bits it has among the 49
        one = e.boot_stats(ds[17].data_ptr(), dc[17].data_ptr(), 1, n_rep + 1, evol_model=1)
        assert same_bits((one[0][0], one[1][0]), (got[0][17], got[1][17]))
        # group forms: the summaries of the means, equal to boot_stats_values on the sibling's means uploaded again
        for name, g in TG.groupings(n_ind).items():
            e.set_groups(g, 5)
            mean, _ = e.run_windows_job_var_groups(lo, hi, maps, off, q, evol_model=1, n_rep=n_rep)
            gs = e.run_windows_job_var_groups_stats(lo, hi, maps, off, q, evol_model=1, n_rep=n_rep)
            assert gs[0].shape == (n_win, 5, 15) and gs[1].shape == (n_win, 15)
            up = torch.from_numpy(mean).to("cuda")
            torch.cuda.synchronize()
            assert same_bits(e.boot_stats_values(up.data_ptr(), n_win, n_rep + 1, 15), gs), name
            X.check_exact(gs, X.expect(mean), "%s group means %s" % (kernel, name))
            gp22 = N().group_pair_index(5, 2, 2)  # a group of one: no cell, NaN means in every matrix
            assert np.all(np.isnan(gs[0][:, 0, gp22])) and np.all(gs[1][:, gp22] == 0)
        # the call's buffers are reused, the grouping's go with it
        e.set_groups(None)
        again = e.run_windows_job_var_stats(lo, hi, maps, off, q, evol_model=1, n_rep=n_rep)
        assert same_bits(again, got)
        assert e.device_bytes() == bytes0
        # a whole-genome job's group form, on the same engine
        t = N().Taus(5)
        jm = np.stack([t.block_map(WV.N_SITES // q) for _ in range(n_rep)])
        e.set_groups(TG.groupings(n_ind)["interleaved"], 5).set_option("boot_partials", 0)
        jmean, _ = e.run_job_groups(jm, q, evol_model=1)
        js = e.run_job_groups_stats(jm, q, evol_model=1)
        X.check_exact((js[0][None], js[1][None]), X.expect(jmean[None]), "%s job group means" % kernel)
        e.set_groups(None).set_option("boot_partials", 1)
        # several batches of windows (the segment-slab plan under a small budget): a set's bits do not depend on the batch
        # or the group of windows it falls in
        e.set_option("win_plan", 2)
        whole = e.run_windows_job_var_stats(lo, hi, maps, off, q, evol_model=1, n_rep=n_rep)
        unbudgeted = e.windows_info()["batches"]
        e.set_option("win_max_bytes", 40 * 256 * 256 * 8 + (1 << 20))
        small = e.run_windows_job_var_stats(lo, hi, maps, off, q, evol_model=1, n_rep=n_rep)
        batches = e.windows_info()["batches"]
        print("%s: %d batches under the small budget, %d without" % (kernel, batches, unbudgeted))
        assert batches > unbudgeted
        e.run_windows_job_var(lo, hi, maps, off, q, d_sum_ptr=ds.data_ptr(), d_cnt_ptr=dc.data_ptr(), n_rep=n_rep)
        assert same_bits(small, e.boot_stats(ds.data_ptr(), dc.data_ptr(), n_win, n_rep + 1, evol_model=1))
        assert same_bits(small, whole)
        check_sums(small, SJ, CJ, 1, "%s window jobs in batches" % kernel)


# ---- 5. refusals: by code, before anything is launched; the engine gives the earlier bits after each -------------------
def test_refusals_leave_the_engine_usable():
    import torch
    n_ind, n_sites, n_rep, q = 10, 64, 4, 8
    t = N().Taus(2)
    maps = np.stack([t.block_map(n_sites // q) for _ in range(n_rep)])
    lo, hi = np.array([0, 8]), np.array([64, 40])
    wmaps, off = N().window_boot_maps(3, lo, hi, n_rep, q)
    cap = N().boot_stats_max_rep()
    big = np.zeros((cap + 1, n_sites // q), dtype=np.uint64)
    n_pairs = N().n_pairs(n_ind)
    with N().Engine(n_ind, n_sites, kernel="mfma", pairwise_del=True) as e:
        e.synth_fill(2, 0.1).commit()
        e.set_option("boot_partials", 0)
        first = e.run_job_stats(maps, q)
        firstw = e.run_windows_job_var_stats(lo, hi, wmaps, off, q, n_rep=n_rep)
        ds = torch.ones((2, n_rep + 1, n_pairs), dtype=torch.float64, device="cuda")
        dc = torch.ones((2, n_rep + 1, n_pairs), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        sp, cp = ds.data_ptr(), dc.data_ptr()
        calls = [
            (lambda: e.run_job_stats(None), -1),                                   # n_rep 0
            (lambda: e.run_job_stats(big, q), -1),                                 # R above the cap
            (lambda: e.run_job_stats(maps, q, evol_model=3), -5),
            (lambda: e.run_job_stats(maps, q, tot_sites=50), -1),                  # with --pairwise_del
            (lambda: e.run_job_groups_stats(maps, q), -1),                         # no grouping
            (lambda: e.run_windows_job_var_groups_stats(lo, hi, wmaps, off, q, n_rep=n_rep), -1),
            (lambda: e.run_windows_job_var_stats(lo, hi, None, off, q, n_rep=0), -1),
            (lambda: e.run_windows_job_var_stats(lo, hi, wmaps, off, q, n_rep=n_rep, evol_model=7), -5),
            (lambda: e.boot_stats(sp, cp, 0, n_rep + 1), -1),                      # n_set 0
            (lambda: e.boot_stats(sp, cp, 2, 1), -1),                              # n_mat < 2
            (lambda: e.boot_stats(None, cp, 2, n_rep + 1), -1),                    # a null pointer
            (lambda: e.boot_stats(sp, None, 2, n_rep + 1), -1),
            (lambda: e.boot_stats(sp, cp, 2, n_rep + 1, tot_sites=9), -1),
            (lambda: e.boot_stats(sp, cp, 2, n_rep + 1, evol_model=3), -5),
            (lambda: e.boot_stats_values(sp, 2, cap + 2, 3), -1),
            (lambda: e.boot_stats_values(None, 2, n_rep + 1, 3), -1),
            (lambda: e.boot_stats_values(sp, 2, n_rep + 1, 0), -1),
        ]
        for ci in (0.0, 1.0, -0.5, 1.5, float("nan")):
            calls.append((lambda ci=ci: e.run_job_stats(maps, q, ci=ci), -1))
            calls.append((lambda ci=ci: e.boot_stats_values(sp, 2, n_rep + 1, 3, ci=ci), -1))
        for k, (call, code) in enumerate(calls):
            with pytest.raises(N().NgdError) as ei:
                call()
            assert ei.value.code == code, (k, str(ei.value))
            assert same_bits(e.run_job_stats(maps, q), first), k
        assert same_bits(e.run_windows_job_var_stats(lo, hi, wmaps, off, q, n_rep=n_rep), firstw)
        # null outputs, through the C interface
        L = e._L
        assert L.ngd_run_job_stats(e._h, maps.ctypes.data_as(C.POINTER(C.c_uint64)), n_rep, n_sites // q, q, 0, 1, 0.95, None, None) == -1
        assert same_bits(e.run_job_stats(maps, q), first)
    with N().Engine(n_ind, n_sites, kernel="mfma", shard_rank=0, shard_world=2) as e:
        e.synth_fill(2).commit()
        with pytest.raises(N().NgdError) as ei:
            e.run_job_stats(maps, q)
        assert ei.value.code == -1 and "share of the pairs" in str(ei.value)
