"""Classical MDS on the device (ngd_mds*_device, ngd_run_*_mds; mds.hip k_mds).

The values form against numpy by the checks of mds_expect.py (bounds: 1e-9 relative to S = max |eigenvalue| of numpy's
eigvalsh of the same B) on the matrices test_mds_cpu.py uses, and against the host twin (eigenvalues within 1e-9 S).  Sums
and counts under models 0, 1 and 2 against numpy on host-finished distances.  Determinism by bits: chunks of one matrix
against the default, a matrix repeated at positions 0, 17 and 36.  The run forms equal ngd_mds_device on their _device
sibling's output bit for bit, dist0 the _dist sibling's matrix 0.  Every comparison prints its largest figure in units of
its bound.  The largest seen on an MI355X over the cases of this file, as fractions of S (of 1 for orthonormality and the
dot product; bound 1e-9 each): eigenvalues 2.2e-15, residuals 2.3e-15, totals 1.7e-15 of the sum of |eigenvalue|,
orthonormality 1.1e-15, 1 - |v . numpy's v| 1.3e-15, device against host twin 6.2e-15, the planted distances 2.1e-15 of the
largest distance.

Also here: n = 1153 (a row is more than one batch of 1024 columns) and n = 2050 (more than 64 KB of LDS), the workgroups of
NGD_MDS_WG, the refusals, and free device memory after repeated calls."""
import ctypes as C

import numpy as np
import pytest

import mds_expect as X

pytestmark = pytest.mark.gpu


def N():
    import ngsdist_amd
    return ngsdist_amd


def synth(seed, n_ind, n_sites, miss_frac=0.0):
    from oracle import oracle as O
    return O.synth_indmajor(seed, n_ind, n_sites, miss_frac=miss_frac)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def same(a, b):
    """two (eig, vec, tot, status) tuples, bit for bit"""
    return (all(np.array_equal(bits(x).ravel(), bits(y).ravel()) for x, y in zip(a[:3], b[:3])) and
            np.array_equal(np.asarray(a[3]).ravel(), np.asarray(b[3]).ravel()))


def on_device(e, v, K):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to("cuda")
    torch.cuda.synchronize()
    return e.mds_values(t.data_ptr(), v.shape[0], K)


def device_buffers(shape):
    import torch
    ds = torch.empty(shape, dtype=torch.float64, device="cuda")
    dc = torch.empty(shape, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    return ds, dc


def to_host(ds, dc):
    import torch
    torch.cuda.synchronize()
    return ds.cpu().numpy(), dc.cpu().numpy().astype(np.uint64)


def finish(S, Cn, model, tot=0):
    with np.errstate(all="ignore"):
        return N().finish(S.reshape(-1), Cn.reshape(-1), tot, model).reshape(S.shape)


# ---- 1. values as they are: wave boundaries (63, 64, 65), a workgroup's edges (3, 4, 5), more rows than waves (130, 257) ----
@pytest.mark.parametrize("n", X.SIZES)
def test_values_form_against_numpy_and_the_host_twin(n):
    v = X.matrices(n)
    with N().Engine(n, 16, kernel="mfma") as e:
        e.synth_fill(1).commit()
        got = {K: on_device(e, v, K) for K in X.dims(n)}
        assert e.last_mds_ms() > 0
    for K, (eig, vec, tot, status) in got.items():
        assert eig.shape == (X.N_MAT, K) and vec.shape == (X.N_MAT, K, n) and tot.shape == (X.N_MAT, 2)
        X.check_all(v, n, K, eig, vec, tot, status, "device")
        heig, _, htot, hstatus = N().mds_host(v, n, K)
        ok = status == 1
        S = np.array([np.abs(X.spectrum(v[m], n)[1]).max() if ok[m] else 1.0 for m in range(X.N_MAT)])
        worst = (np.abs(eig[ok] - heig[ok]).max(axis=1) / np.where(S[ok] > 0, S[ok], 1.0)).max() / X.TOL
        print("device against host twin n=%d K=%d: eigenvalues differ by %.3g of the bound" % (n, K, worst))
        assert np.array_equal(status, hstatus) and worst <= 1
        zero = X.AT["zero"]
        assert np.all(np.abs(eig[zero]) <= 1e-200) and np.all(np.isfinite(vec[zero]))
        # a vector's bits do not depend on how many are asked for
        if K > 1:
            assert np.array_equal(bits(eig[:, :1]), bits(got[1][0])) and np.array_equal(bits(vec[:, :1]), bits(got[1][1]))
    K = min(4, n - 1)
    m = X.AT["planted"]
    X.check_planted(v[m], n, N().mds_coords(got[K][0][m], got[K][1][m]))


# ---- 1b. the kernel's other paths: rows past one batch of loads (1024 columns), LDS past 64 KB (n > 2040), smaller workgroups ----
@pytest.mark.parametrize("n", [1153, 2050])
def test_rows_past_one_batch_of_loads_and_lds_past_64_kb(n):
    K = 4
    v = X.few(n)  # a random matrix, a planted one, one with a NaN cell
    with N().Engine(n, 16, kernel="mfma") as e:
        e.synth_fill(1).commit()
        eig, vec, tot, status = on_device(e, v, K)
    assert status.tolist() == [1, 1, 0]
    X.check_bad(eig[2], vec[2], tot[2], status[2])
    for m in (0, 1):
        fig = X.check_matrix(v[m], n, K, eig[m], vec[m], tot[m])  # (vectors are compared where their eigenvalue is 1e-3 S apart)
        print("device n=%d matrix %d: largest figures in units of 1e-9: %s" % (n, m, {k: "%.3g" % x for k, x in fig.items()}))
    X.check_planted(v[1], n, N().mds_coords(eig[1], vec[1]))


@pytest.mark.parametrize("wg", [256, 512])
def test_the_measurement_override_of_the_workgroup_keeps_the_bounds(wg, monkeypatch):
    n, K = 130, 16
    v = X.matrices(n)
    monkeypatch.setenv("NGD_MDS_WG", str(wg))
    with N().Engine(n, 16, kernel="mfma") as e:
        e.synth_fill(1).commit()
        eig, vec, tot, status = on_device(e, v, K)
        again = on_device(e, v, K)
    X.check_all(v, n, K, eig, vec, tot, status, "device, %d threads" % wg)
    assert same((eig, vec, tot, status), again)


def test_chunks_and_positions_change_no_bit():
    n, K = 65, 4
    v = X.matrices(n)
    rep = v.copy()
    rep[17] = rep[36] = rep[0]
    with N().Engine(n, 16, kernel="mfma") as e:
        e.synth_fill(1).commit()
        whole = on_device(e, v, K)
        at3 = on_device(e, rep, K)
        e.set_option("mds_max_bytes", (n + 4 * K) * (n + 1) * 8)  # one matrix's scratch (a row is n doubles rounded up to even)
        one = on_device(e, v, K)
        e.set_option("mds_max_bytes", 1)  # never fewer than one matrix
        least = on_device(e, v, K)
        e.set_option("mds_max_bytes", 3 * (n + 4 * K) * (n + 1) * 8)
        three = on_device(e, v, K)
    assert same(one, whole) and same(least, whole) and same(three, whole)
    for m in (17, 36):
        assert all(np.array_equal(bits(x[m]), bits(x[0])) for x in at3[:3])
    assert all(np.array_equal(bits(x[0]), bits(y[0])) for x, y in zip(at3[:3], whole[:3]))


# ---- 2. sums and counts ----------------------------------------------------------------------------------------------------
def check_finished(got, d, n, K, what):
    worst = {}
    for m in range(d.shape[0]):
        assert got[3][m] == 1
        for name, x in X.check_matrix(d[m], n, K, got[0][m], got[1][m], got[2][m]).items():
            worst[name] = max(worst.get(name, 0.0), x)
    print("%s: largest figures in units of 1e-9: %s" % (what, {k: "%.3g" % x for k, x in worst.items()}))


@pytest.mark.parametrize("model", [0, 1, 2])
def test_sums_and_counts_against_numpy_on_finished_distances(model):
    n_rep, q, K = 5, 5, 4
    for n_ind, n_sites, kernel in ((65, 400, "mfma"), (40, 600, "em_table")):
        n_pairs = N().n_pairs(n_ind)
        t = N().Taus(3)
        maps = np.stack([t.block_map(n_sites // q) for _ in range(n_rep)])
        with N().Engine(n_ind, n_sites, kernel=kernel, indep_geno=kernel == "mfma") as e:
            e.upload_ind_major(synth(11, n_ind, n_sites)).commit()
            e.set_option("boot_partials", 0)
            ds, dc = device_buffers((n_rep + 1, n_pairs))
            e.run_job(maps, q, d_sum_ptr=ds.data_ptr(), d_cnt_ptr=dc.data_ptr())
            S, Cn = to_host(ds, dc)
            got = e.mds(ds.data_ptr(), dc.data_ptr(), n_rep + 1, K, evol_model=model)
            check_finished(got, finish(S, Cn, model), n_ind, K, "%d x %d %s model %d" % (n_ind, n_sites, kernel, model))
            if model == 0:  # --tot_sites: d_cnt is not read (a null pointer here)
                got = e.mds(ds.data_ptr(), None, n_rep + 1, K, evol_model=0, tot_sites=1234)
                check_finished(got, finish(S, Cn, 0, 1234), n_ind, K, "%d x %d %s tot_sites" % (n_ind, n_sites, kernel))


# ---- 3. the run forms against their siblings ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(65, 400, "mfma"), (40, 600, "em_table")])
def test_run_job_mds(shape):
    n_ind, n_sites, kernel = shape
    n_rep, q, K = 5, 4, 3
    n_pairs = N().n_pairs(n_ind)
    t = N().Taus(5)
    maps = np.stack([t.block_map(n_sites // q) for _ in range(n_rep)])
    with N().Engine(n_ind, n_sites, kernel=kernel, indep_geno=kernel == "mfma") as e:
        e.upload_ind_major(synth(13, n_ind, n_sites)).commit()
        e.set_option("boot_partials", 0)  # (pins the plan: two calls of a job then agree bit for bit)
        got = e.run_job_mds(K, maps, q, evol_model=1)
        assert got[0].shape == (n_rep + 1, K) and got[1].shape == (n_rep + 1, K, n_ind) and got[2].shape == (n_rep + 1, 2)
        assert got[3].tolist() == [1] * (n_rep + 1) and got[4].shape == (n_pairs,)
        assert e.last_mds_ms() > 0
        ds, dc = device_buffers((n_rep + 1, n_pairs))
        e.run_job(maps, q, d_sum_ptr=ds.data_ptr(), d_cnt_ptr=dc.data_ptr())
        assert same(got[:4], e.mds(ds.data_ptr(), dc.data_ptr(), n_rep + 1, K, evol_model=1))
        dist = e.run_job_dist(maps, q, 1)
        assert np.array_equal(bits(got[4]), bits(dist[0]))
        # n_rep = 0: a plain run's one matrix
        plain = e.run_job_mds(K, None, evol_model=1)
        e.run_job(None, d_sum_ptr=ds.data_ptr(), d_cnt_ptr=dc.data_ptr())
        assert plain[0].shape == (1, K)
        assert same(plain[:4], e.mds(ds.data_ptr(), dc.data_ptr(), 1, K, evol_model=1))
        assert np.array_equal(bits(plain[4]), bits(e.run_job_dist(None, 1, 1)[0]))
        assert e.run_job_mds(K, maps, q, evol_model=1, dist0=False)[4] is None


@pytest.mark.parametrize("kernel", ["mfma", "em_table"])
def test_window_forms(kernel):
    n_ind, n_sites, n_rep, q, K = 24, 200, 4, 5, 4
    n_pairs = N().n_pairs(n_ind)
    lo, hi = np.array([0, 0, 1, 10, 50, 60]), np.array([1, 200, 3, 14, 57, 160])  # [0, 1), [1, 3), [10, 14): shorter than a block
    maps, off = N().window_boot_maps(3, lo, hi, n_rep, q)
    n_win = len(lo)
    with N().Engine(n_ind, n_sites, kernel=kernel, indep_geno=kernel == "mfma") as e:
        e.upload_ind_major(synth(17, n_ind, n_sites)).commit()
        # plain windows
        got = e.run_windows_mds(K, lo, hi, evol_model=0)
        assert got[0].shape == (n_win, 1, K) and got[1].shape == (n_win, 1, K, n_ind) and got[3].shape == (n_win, 1) and np.all(got[3] == 1)
        ds, dc = device_buffers((n_win, n_pairs))
        e.run_windows(lo, hi, d_sum_ptr=ds.data_ptr(), d_cnt_ptr=dc.data_ptr())
        assert same(got[:4], e.mds(ds.data_ptr(), dc.data_ptr(), n_win, K, evol_model=0))
        assert np.array_equal(bits(got[4]), bits(e.run_windows_dist(lo, hi, 0)))
        # replicates inside windows of unequal length: no block, no finite replicate, status 0; matrix 0 has its coordinates
        got = e.run_windows_job_var_mds(K, lo, hi, maps, off, q, evol_model=0, n_rep=n_rep)
        assert got[0].shape == (n_win, n_rep + 1, K) and got[3].shape == (n_win, n_rep + 1)
        short = (hi - lo) // q == 0
        assert short.sum() == 3 and np.all(got[3][:, 0] == 1)
        assert np.all(got[3][short, 1:] == 0) and np.all(got[3][~short, 1:] == 1)
        for a in got[:3]:
            assert np.all(bits(a[short, 1:]) == X.NAN_BITS)
        ds, dc = device_buffers((n_win, n_rep + 1, n_pairs))
        e.run_windows_job_var(lo, hi, maps, off, q, d_sum_ptr=ds.data_ptr(), d_cnt_ptr=dc.data_ptr(), n_rep=n_rep)
        assert same(got[:4], e.mds(ds.data_ptr(), dc.data_ptr(), n_win * (n_rep + 1), K, evol_model=0))
        dist = e.run_windows_job_var_dist(lo, hi, maps, off, q, 0, n_rep=n_rep)
        assert np.array_equal(bits(got[4]), bits(dist[:, 0]))
        # n_rep = 0 through the job form: the windows alone
        alone = e.run_windows_job_var_mds(K, lo, hi, None, np.zeros(n_win, dtype=np.uint64), q, evol_model=0, n_rep=0)
        assert same(alone[:4], e.run_windows_mds(K, lo, hi, evol_model=0)[:4])


# ---- 4. refusals: by code, before anything is launched; outputs and engine as they were -----------------------------------
def test_refusals_leave_the_engine_usable():
    n_ind, n_sites, n_rep, q, K = 10, 64, 4, 8, 2
    t = N().Taus(2)
    maps = np.stack([t.block_map(n_sites // q) for _ in range(n_rep)])
    lo, hi = np.array([0, 8]), np.array([64, 40])
    wmaps, off = N().window_boot_maps(3, lo, hi, n_rep, q)
    n_pairs = N().n_pairs(n_ind)
    with N().Engine(n_ind, n_sites, kernel="mfma", pairwise_del=True) as e:
        e.synth_fill(2, 0.1).commit()
        e.set_option("boot_partials", 0)
        first = e.run_job_mds(K, maps, q)
        firstw = e.run_windows_job_var_mds(K, lo, hi, wmaps, off, q, n_rep=n_rep)
        ds, dc = device_buffers((n_rep + 1, n_pairs))
        e.run_job(maps, q, d_sum_ptr=ds.data_ptr(), d_cnt_ptr=dc.data_ptr())
        sp, cp = ds.data_ptr(), dc.data_ptr()
        calls = [
            (lambda: e.mds(sp, cp, 0, K), -1),                                       # n_mat 0
            (lambda: e.mds(None, cp, n_rep + 1, K), -1),                             # a null pointer
            (lambda: e.mds(sp, None, n_rep + 1, K), -1),
            (lambda: e.mds(sp, cp, n_rep + 1, K, tot_sites=9), -1),                  # with --pairwise_del
            (lambda: e.mds(sp, cp, n_rep + 1, K, evol_model=3), -5),
            (lambda: e.mds(sp, cp, n_rep + 1, 0), -1),                               # K = 0
            (lambda: e.mds(sp, cp, n_rep + 1, n_ind), -1),                           # K > n - 1
            (lambda: e.mds_values(None, 2, K), -1),
            (lambda: e.mds_values(sp, 0, K), -1),
            (lambda: e.mds_values(sp, 2, n_ind), -1),
            (lambda: e.run_job_mds(K, maps, q, evol_model=3), -5),
            (lambda: e.run_job_mds(K, maps, q, tot_sites=50), -1),
            (lambda: e.run_job_mds(0, maps, q), -1),
            (lambda: e.run_job_mds(n_ind, maps, q), -1),
            (lambda: e.run_windows_mds(K, lo, hi, evol_model=7), -5),
            (lambda: e.run_windows_mds(K, lo, hi, tot_sites=50), -1),
            (lambda: e.run_windows_mds(n_ind, lo, hi), -1),
            (lambda: e.run_windows_job_var_mds(K, lo, hi, wmaps, off, q, n_rep=n_rep, evol_model=7), -5),
            (lambda: e.run_windows_job_var_mds(K, lo, hi, wmaps, off, q, n_rep=n_rep, tot_sites=5), -1),
            (lambda: e.run_windows_job_var_mds(0, lo, hi, wmaps, off, q, n_rep=n_rep), -1),
        ]
        for k, (call, code) in enumerate(calls):
            with pytest.raises(N().NgdError) as ei:
                call()
            assert ei.value.code == code, (k, str(ei.value))
            assert same(e.run_job_mds(K, maps, q)[:4], first[:4]), k
        assert same(e.run_windows_job_var_mds(K, lo, hi, wmaps, off, q, n_rep=n_rep)[:4], firstw[:4])
        # null outputs through the C interface; a refused call writes nothing
        L = e._L
        eig, vec, tot = np.full((n_rep + 1, K), -7.0), np.full((n_rep + 1, K, n_ind), -7.0), np.full((n_rep + 1, 2), -7.0)
        st = np.full(n_rep + 1, 9, dtype=np.uint32)
        dp = C.POINTER(C.c_double)
        ep, vp, tp, stp = eig.ctypes.data_as(dp), vec.ctypes.data_as(dp), tot.ctypes.data_as(dp), st.ctypes.data_as(C.POINTER(C.c_uint32))
        mp = maps.ctypes.data_as(C.POINTER(C.c_uint64))
        nb = n_sites // q
        assert L.ngd_run_job_mds(e._h, mp, n_rep, nb, q, 0, 1, K, None, vp, tp, stp, None) == -1
        assert L.ngd_run_job_mds(e._h, mp, n_rep, nb, q, 0, 1, K, ep, None, tp, stp, None) == -1
        assert L.ngd_run_job_mds(e._h, mp, n_rep, nb, q, 0, 1, K, ep, vp, None, stp, None) == -1
        assert L.ngd_run_job_mds(e._h, mp, n_rep, nb, q, 0, 1, K, ep, vp, tp, None, None) == -1
        assert L.ngd_run_job_mds(e._h, None, n_rep, nb, q, 0, 1, K, ep, vp, tp, stp, None) == -1
        assert L.ngd_run_job_mds(e._h, mp, n_rep, nb, q, 0, 1, 17, ep, vp, tp, stp, None) == -1
        assert L.ngd_mds_device(e._h, C.c_void_p(sp), C.c_void_p(cp), n_rep + 1, 0, 4, K, ep, vp, tp, stp) == -5
        assert L.ngd_mds_values_device(None, C.c_void_p(sp), 1, K, ep, vp, tp, stp) == -1
        assert np.all(eig == -7.0) and np.all(vec == -7.0) and np.all(tot == -7.0) and np.all(st == 9)
        assert same(e.run_job_mds(K, maps, q)[:4], first[:4])
    with N().Engine(n_ind, n_sites, kernel="mfma", shard_rank=0, shard_world=2) as e:
        e.synth_fill(2).commit()
        with pytest.raises(N().NgdError) as ei:
            e.run_job_mds(K, maps, q)
        assert ei.value.code == -1 and "share of the pairs" in str(ei.value)


def test_fewer_than_three_individuals_and_more_than_either_cap_are_refused():
    with N().Engine(2, 64, kernel="mfma") as e:
        e.synth_fill(2).commit()
        with pytest.raises(N().NgdError) as ei:
            e.run_job_mds(1, None)
        assert ei.value.code == -1 and "three individuals" in str(ei.value)
        s, c = e.run()
        assert s.shape == (1,) and np.isfinite(s).all()
    with N().Engine(20, 64, kernel="mfma") as e:  # K above ngd_mds_max_dim() where n - 1 would allow it
        e.synth_fill(2).commit()
        first = e.run_job_mds(16, None)
        with pytest.raises(N().NgdError) as ei:
            e.run_job_mds(17, None)
        assert ei.value.code == -1 and "min(n_ind - 1, 16)" in str(ei.value)
        assert same(e.run_job_mds(16, None)[:4], first[:4])
    with N().Engine(N().mds_max_ind() + 1, 16, kernel="mfma") as e:
        e.synth_fill(2).commit()
        with pytest.raises(N().NgdError) as ei:
            e.run_job_mds(2, None)
        assert ei.value.code == -1 and "ngd_mds_max_ind" in str(ei.value)
        s, c = e.run()
        assert np.isfinite(s).all()


# ---- 5. repeated calls leave free device memory where it was ---------------------------------------------------------------
def test_repeated_calls_do_not_leak():
    import torch
    n, K = 65, 4
    v = X.matrices(n)[:7]
    with N().Engine(n, 64, kernel="mfma") as e:
        e.synth_fill(3).commit()
        t = torch.from_numpy(v).to("cuda")
        torch.cuda.synchronize()
        first = e.mds_values(t.data_ptr(), 7, K)
        firstj = e.run_job_mds(K, None)
        held, free = e.device_bytes(), torch.cuda.mem_get_info()[0]
        for _ in range(5):
            assert same(e.mds_values(t.data_ptr(), 7, K), first)
            assert same(e.run_job_mds(K, None)[:4], firstj[:4])
        assert e.device_bytes() == held and torch.cuda.mem_get_info()[0] == free
