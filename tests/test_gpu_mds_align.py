"""Alignment of MDS replicates on the device (ngd_mds_align_values_device, ngd_run_job_mds_align,
ngd_run_windows_job_var_mds_align; mds_align.hip k_mds_coords, k_mds_align).

The values form against numpy's SVD by the checks of mds_align_expect.py and against the host twin, on planted sets X_r =
X_0 R_r + 1e-2 noise at n = 3, 5, 63, 64, 65, 257, 1153 (a lane's edge, a wave's edge, more rows than threads, more than one
pass over the workgroup), K = 1, 2, min(n - 1, 16), R = 1, 33, n_set = 1, 3; where M is singular (a zero column of X_r or of
X_0, X_0 = 0, everything zero, and K = n - 1 on an all-equal matrix through mds_host); status 0.  Determinism
by bits: a set repeated at positions 0 and 2 of a call, chunks of the MDS kernel that cut a set.  The run forms: matrix 0
is the _mds sibling's, aligned and fit are the values form's on the sibling's coordinates, the statistics are
boot_stats_values' on the aligned cells, all bit for bit, and boot_stats_host's within 1e-9 max |X_0|.

Bounds: Y within 1e-9 max(|X_0|, |X_r|) of numpy's where sigma_min(M) >= 1e-3 sigma_max(M) (asserted of every planted
replicate), fit within 1e-9 (|X_r|^2 + |X_0|^2) of |X_r|^2 + |X_0|^2 - 2 SUM sigma, |Q Q^T - I| <= 1e-9; device against twin
by the same two bounds (orthogonality as far as Y shows Q: mds_align_expect.check_orth says where that stops).  Every comparison prints its largest figure in units of its bound.  The largest seen on an MI355X
over the cases of this file: Y 6.4e-15 of max |X| against numpy and 1.7e-15 against the twin, fit 1.7e-15 of the squared
norms against the formula and 1.2e-15 against the twin, orthogonality 8.4e-15; the statistics of the run forms differ from
boot_stats_host's by 0.

Also here: the refusals, and free device memory after repeated calls."""
import ctypes as C

import numpy as np
import pytest

import mds_align_expect as A

pytestmark = pytest.mark.gpu

SIZES = [3, 5, 63, 64, 65, 257, 1153]


def N():
    import ngsdist_amd
    return ngsdist_amd


def synth(seed, n_ind, n_sites):
    from oracle import oracle as O
    return O.synth_indmajor(seed, n_ind, n_sites)


bits = A.bits


def upload(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda")
    torch.cuda.synchronize()
    return t


def seen(Xp):
    """planted sets [n_set][n_mat][n][K] -> (eig, vec, the coordinates the library forms of them [n_set][n_mat][n][K])"""
    eig, vec = A.eigvec_of(Xp)
    return eig, vec, N().mds_coords(eig, vec)


def on_device(e, Xs, K, status=None):
    """coordinates [n_set][n_mat][n][K] -> (aligned [n_set][n_mat][K][n], fit [n_set][n_mat])"""
    t = upload(A.kn(Xs))
    return e.mds_align_values(t.data_ptr(), Xs.shape[0], Xs.shape[1], K, status)


def against_twin(Xs, aligned, fit, haligned, hfit):
    """device against host twin over the matrices of a call: (Y, fit) in units of their bounds"""
    y = f = 0.0
    for s in range(Xs.shape[0]):
        for r in range(1, Xs.shape[1]):
            if not np.isfinite(hfit[s, r]):
                assert bits(fit[s, r]) == A.NAN_BITS
                continue
            scale = max(np.abs(Xs[s, 0]).max(), np.abs(Xs[s, r]).max())
            norms = (Xs[s, 0] ** 2).sum() + (Xs[s, r] ** 2).sum()
            if scale > 0:
                y = max(y, np.abs(aligned[s, r] - haligned[s, r]).max() / (A.TOL * scale))
                f = max(f, abs(fit[s, r] - hfit[s, r]) / (A.TOL * norms))
    return y, f


def same_outputs(a, b):
    """two aligned calls' dicts, bit for bit"""
    for k, v in a.items():
        assert np.array_equal(np.atleast_1d(v).view(np.uint8), np.atleast_1d(b[k]).view(np.uint8)), k


def cut_budgets(n, K):
    """values of mds_max_bytes under which the MDS kernel's chunks cut a set of 6 matrices: the scratch of 4 matrices as the
    engine counts it today ((n + 4 K) rows of n + 1 doubles each at odd n: chunks of 4 and 2, a cut inside the set), and 1
    byte -- never fewer than one matrix a chunk, whatever a matrix's scratch is: every set is cut even if that count changes"""
    assert n % 2 == 1
    return [4 * (n + 4 * K) * (n + 1) * 8, 1]


def singular_sets(n, K):
    base = A.planted(n, K, 3, seed=21)
    a, b, c = base.copy(), base.copy(), base.copy()
    a[1:, :, -1] = 0.0   # the last column of X_r
    b[0, :, -1] = 0.0    # the last column of X_0
    c[0] = 0.0           # X_0
    return np.stack([a, b, c, np.zeros_like(base)])


# ---- 1. the values form --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_values_form_against_numpy_and_the_host_twin(n):
    with N().Engine(n, 16, kernel="mfma") as e:
        e.synth_fill(1).commit()
        for K in A.dims(n):
            for R in (1, 33):
                for n_set in (1, 3):
                    eig, vec, Xs = seen(np.stack([A.planted(n, K, R, seed=10 * s + R) for s in range(n_set)]))
                    aligned, fit = on_device(e, Xs, K)
                    assert aligned.shape == (n_set, R + 1, K, n) and fit.shape == (n_set, R + 1)
                    assert e.last_mds_align_ms() > 0
                    worst = {}
                    for s in range(n_set):
                        for k, x in A.check_set(Xs[s], aligned[s], fit[s]).items():
                            worst[k] = max(worst.get(k, 0.0), x)
                    worst["twin y"], worst["twin fit"] = against_twin(Xs, aligned, fit, *N().mds_align_host(eig, vec))
                    print("device n=%d K=%d R=%d n_set=%d: largest figures in units of 1e-9: %s" %
                          (n, K, R, n_set, {k: "%.3g" % x for k, x in worst.items()}))
                    assert worst["twin y"] <= 1 and worst["twin fit"] <= 1


@pytest.mark.parametrize("n", [3, 5, 65, 257])
def test_singular_cases_and_status_0(n):
    with N().Engine(n, 16, kernel="mfma") as e:
        e.synth_fill(1).commit()
        for K in A.dims(n):
            eig, vec, Xs = seen(singular_sets(n, K))
            aligned, fit = on_device(e, Xs, K)
            worst = {}
            for s in range(len(Xs)):
                for k, x in A.check_set(Xs[s], aligned[s], fit[s], regular=False).items():
                    worst[k] = max(worst.get(k, 0.0), x)
            print("singular n=%d K=%d: largest figures in units of 1e-9: %s" % (n, K, {k: "%.3g" % x for k, x in worst.items()}))
            again = on_device(e, Xs, K)
            assert np.array_equal(bits(aligned), bits(again[0])) and np.array_equal(bits(fit), bits(again[1]))
            one = on_device(e, Xs[1:2], K)  # a set's bits do not depend on its neighbours
            assert np.array_equal(bits(aligned[1]), bits(one[0][0])) and np.array_equal(bits(fit[1]), bits(one[1][0]))
            # status 0 in a replicate, and in matrix 0
            eig, vec, Xs = seen(np.stack([A.planted(n, K, 5, seed=s) for s in range(3)]))
            status = np.ones((3, 6), dtype=np.uint32)
            status[0, 2] = status[1, 0] = 0
            aligned, fit = on_device(e, Xs, K, status)
            for s in range(3):
                A.check_set(Xs[s], aligned[s], fit[s], status=status[s])
            plain = on_device(e, Xs, K)
            keep = status.astype(bool) & status[:, :1].astype(bool)
            assert np.array_equal(bits(aligned[keep]), bits(plain[0][keep])) and np.array_equal(bits(fit[keep]), bits(plain[1][keep]))


def test_a_set_repeated_in_a_call_has_the_same_bits():
    n, K, R = 65, 16, 5
    a, b = A.planted(n, K, R, seed=1), A.planted(n, K, R, seed=2)
    _, _, Xs = seen(np.stack([a, b, a]))
    with N().Engine(n, 16, kernel="mfma") as e:
        e.synth_fill(1).commit()
        aligned, fit = on_device(e, Xs, K)
        alone = on_device(e, Xs[:1], K)
    assert np.array_equal(bits(aligned[0]), bits(aligned[2])) and np.array_equal(bits(fit[0]), bits(fit[2]))
    assert np.array_equal(bits(aligned[0]), bits(alone[0][0])) and np.array_equal(bits(fit[0]), bits(alone[1][0]))


@pytest.mark.parametrize("n", [3, 4, 5, 64])
def test_all_equal_matrix_at_full_rank_through_mds_host(n):
    """K = n - 1 (16 at n = 64) on all-equal cells: M = c I up to rounding -- every singular value equal, off-diagonals at
    the level of the skip threshold"""
    K = min(n - 1, 16)
    v = np.full((2, 4, n * (n - 1) // 2), 0.25)
    eig, vec, tot, status = N().mds_host(v.reshape(8, -1), n, K)
    eig, vec, status = eig.reshape(2, 4, K), vec.reshape(2, 4, K, n), status.reshape(2, 4)
    assert np.all(status == 1)
    Xs = N().mds_coords(eig, vec)
    with N().Engine(n, 16, kernel="mfma") as e:
        e.synth_fill(1).commit()
        aligned, fit = on_device(e, Xs, K, status)
        again = on_device(e, Xs, K, status)
        one = on_device(e, Xs[1:], K)
    worst = {}
    for s in range(2):
        for k, x in A.check_set(Xs[s], aligned[s], fit[s], regular=False, status=status[s]).items():
            worst[k] = max(worst.get(k, 0.0), x)
    worst["twin y"], worst["twin fit"] = against_twin(Xs, aligned, fit, *N().mds_align_host(eig, vec, status))
    print("all-equal n=%d K=%d: largest figures in units of 1e-9: %s" % (n, K, {k: "%.3g" % x for k, x in worst.items()}))
    assert worst["twin y"] <= 1 and worst["twin fit"] <= 1
    assert np.array_equal(bits(aligned), bits(again[0])) and np.array_equal(bits(fit), bits(again[1]))
    assert np.array_equal(bits(aligned[1]), bits(one[0][0])) and np.array_equal(bits(fit[1]), bits(one[1][0]))


# ---- 2. the run forms ----------------------------------------------------------------------------------------------------
def check_run(e, out, sib, K, ci, who):
    """out: an aligned call's dict with a leading axis of sets; sib: the _mds sibling's (eig, vec, tot, status, dist0) of
    the same sets [n_set][n_mat]"""
    eig, vec, tot, status, dist0 = sib
    n_set, n_mat, n = eig.shape[0], eig.shape[1], vec.shape[-1]
    assert np.array_equal(bits(out["eig0"]), bits(eig[:, 0])) and np.array_equal(bits(out["vec0"]), bits(vec[:, 0]))
    assert np.array_equal(bits(out["tot0"]), bits(tot[:, 0])) and np.array_equal(out["status"], status)
    assert np.array_equal(bits(out["dist0"]), bits(dist0))
    # aligned and fit: the values form on the sibling's coordinates
    Xs = N().mds_coords(eig, vec)
    aligned, fit = on_device(e, Xs, K, status)
    assert np.array_equal(bits(out["aligned"]), bits(aligned)) and np.array_equal(bits(out["fit"]), bits(fit))
    worst = {}
    for s in range(n_set):
        for k, x in A.check_set(Xs[s], aligned[s], fit[s], regular=False, status=status[s]).items():
            worst[k] = max(worst.get(k, 0.0), x)
    # the statistics: of the aligned cells and the eigenvalues of the matrices that went in
    left_out = ~(status.astype(bool) & status[:, :1].astype(bool))
    cells = np.concatenate([aligned.reshape(n_set, n_mat, K * n), np.where(left_out[..., None], np.nan, eig)], axis=2)
    t = upload(cells)
    stats, used = e.boot_stats_values(t.data_ptr(), n_set, n_mat, K * (n + 1), ci)
    assert np.array_equal(bits(out["stats"]), bits(stats))
    assert np.array_equal(used, np.broadcast_to(out["used"][:, None], used.shape))
    assert np.array_equal(out["used"], (~left_out[:, 1:]).sum(axis=1).astype(np.uint64))
    hstats, hused = N().boot_stats_host(cells, ci)
    assert np.array_equal(hused, used) and np.array_equal(np.isnan(hstats), np.isnan(stats))
    scale = np.abs(Xs[:, 0]).max()
    worst["stats"] = np.nanmax(np.abs(hstats - stats), initial=0.0) / (A.TOL * scale)
    print("%s: largest figures in units of 1e-9: %s" % (who, {k: "%.3g" % x for k, x in worst.items()}))
    assert worst["stats"] <= 1


@pytest.mark.parametrize("n_ind", [5, 65])
def test_run_job_mds_align(n_ind):
    n_sites, n_rep, q, ci = 300, 5, 4, 0.9
    K = 2 if n_ind == 5 else 4
    t = N().Taus(5)
    maps = np.stack([t.block_map(n_sites // q) for _ in range(n_rep)])
    with N().Engine(n_ind, n_sites, kernel="mfma") as e:
        e.upload_ind_major(synth(13, n_ind, n_sites)).commit()
        e.set_option("boot_partials", 0)  # (pins the plan: two calls of a job then agree bit for bit)
        out = e.run_job_mds_align(K, maps, q, ci=ci)
        assert out["stats"].shape == (5, K * (n_ind + 1)) and out["aligned"].shape == (n_rep + 1, K, n_ind)
        assert out["fit"].shape == (n_rep + 1,) and int(out["used"]) == n_rep
        assert e.last_mds_align_ms() > 0 and e.last_mds_ms() > 0 and e.last_boot_stats_ms() > 0
        sib = e.run_job_mds(K, maps, q)
        check_run(e, {k: v if v is None else v[None] for k, v in out.items()}, tuple(a[None] for a in sib), K, ci, "job n=%d" % n_ind)
        # chunks of the MDS kernel that cut the set change no bit
        for budget in cut_budgets(n_ind, K):
            e.set_option("mds_max_bytes", budget)
            same_outputs(out, e.run_job_mds_align(K, maps, q, ci=ci))
        e.set_option("mds_max_bytes", 0)
        bare = e.run_job_mds_align(K, maps, q, ci=ci, aligned=False, dist0=False)
        assert bare["aligned"] is None and bare["dist0"] is None and np.array_equal(bits(bare["stats"]), bits(out["stats"]))


@pytest.mark.parametrize("n_ind", [5, 65])
def test_run_windows_job_var_mds_align(n_ind):
    n_sites, n_rep, q, ci = 300, 5, 8, 0.95
    K = 2 if n_ind == 5 else 4
    lo, hi = np.array([0, 100, 104]), np.array([100, 105, 300])  # [100, 105): shorter than a block
    maps, off = N().window_boot_maps(3, lo, hi, n_rep, q)
    with N().Engine(n_ind, n_sites, kernel="mfma") as e:
        e.upload_ind_major(synth(17, n_ind, n_sites)).commit()
        out = e.run_windows_job_var_mds_align(K, lo, hi, maps, off, q, n_rep=n_rep, ci=ci)
        assert out["used"].tolist() == [n_rep, 0, n_rep]
        assert np.all(out["status"][1, 1:] == 0) and out["status"][1, 0] == 1
        assert np.all(bits(out["stats"][1, 1:]) == A.NAN_BITS) and np.all(np.isfinite(out["stats"][1, 0]))
        assert np.all(bits(out["fit"][1, 1:]) == A.NAN_BITS) and out["fit"][1, 0] == 0.0
        sib = e.run_windows_job_var_mds(K, lo, hi, maps, off, q, n_rep=n_rep)
        check_run(e, out, sib, K, ci, "windows n=%d" % n_ind)
        for budget in cut_budgets(n_ind, K):
            e.set_option("mds_max_bytes", budget)
            same_outputs(out, e.run_windows_job_var_mds_align(K, lo, hi, maps, off, q, n_rep=n_rep, ci=ci))
        e.set_option("mds_max_bytes", 0)


# ---- 3. refusals: by code, before anything is launched; outputs and engine as they were ------------------------------------
def test_refusals_leave_outputs_and_engine_as_they_were():
    n_ind, n_sites, n_rep, q, K = 10, 64, 4, 8, 2
    t = N().Taus(2)
    maps = np.stack([t.block_map(n_sites // q) for _ in range(n_rep)])
    lo, hi = np.array([0, 8]), np.array([64, 40])
    wmaps, off = N().window_boot_maps(3, lo, hi, n_rep, q)
    many = np.zeros((N().boot_stats_max_rep() + 1, n_sites // q), dtype=np.uint64)
    with N().Engine(n_ind, n_sites, kernel="mfma", pairwise_del=True) as e:
        e.synth_fill(2, 0.1).commit()
        e.set_option("boot_partials", 0)
        first = e.run_job_mds_align(K, maps, q)
        _, _, Xs = seen(A.planted(n_ind, K, 3, seed=1)[None])
        dev = upload(A.kn(Xs))
        calls = [
            (lambda: e.run_job_mds_align(K, None, q), -1),                    # n_rep 0
            (lambda: e.run_job_mds_align(K, maps, q, ci=0.0), -1),
            (lambda: e.run_job_mds_align(K, maps, q, ci=1.0), -1),
            (lambda: e.run_job_mds_align(K, maps, q, ci=float("nan")), -1),
            (lambda: e.run_job_mds_align(K, many, q), -1),                    # more replicates than the summaries serve
            (lambda: e.run_job_mds_align(0, maps, q), -1),
            (lambda: e.run_job_mds_align(n_ind, maps, q), -1),
            (lambda: e.run_job_mds_align(K, maps, q, evol_model=3), -5),
            (lambda: e.run_job_mds_align(K, maps, q, tot_sites=50), -1),      # with --pairwise_del
            (lambda: e.run_windows_job_var_mds_align(K, lo, hi, wmaps, off, q, n_rep=0), -1),
            (lambda: e.run_windows_job_var_mds_align(K, lo, hi, wmaps, off, q, n_rep=n_rep, ci=2.0), -1),
            (lambda: e.run_windows_job_var_mds_align(0, lo, hi, wmaps, off, q, n_rep=n_rep), -1),
            (lambda: e.run_windows_job_var_mds_align(K, lo, hi, wmaps, off, q, n_rep=n_rep, evol_model=7), -5),
            (lambda: e.mds_align_values(None, 1, 4, K), -1),
            (lambda: e.mds_align_values(dev.data_ptr(), 0, 4, K), -1),
            (lambda: e.mds_align_values(dev.data_ptr(), 1, 0, K), -1),
            (lambda: e.mds_align_values(dev.data_ptr(), 1, 4, 0), -1),
            (lambda: e.mds_align_values(dev.data_ptr(), 1, 4, n_ind), -1),
        ]
        for k, (call, code) in enumerate(calls):
            with pytest.raises(N().NgdError) as ei:
                call()
            assert ei.value.code == code, (k, str(ei.value))
        again = e.run_job_mds_align(K, maps, q)
        same_outputs(first, again)
        # through the C interface: a refused call writes nothing
        L = e._L
        dp, u32p, u64p = C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
        nc = K * (n_ind + 1)
        o = {"eig0": np.full(K, -7.0), "vec0": np.full((K, n_ind), -7.0), "tot0": np.full(2, -7.0),
             "status": np.full(n_rep + 1, 9, dtype=np.uint32), "stats": np.full((5, nc), -7.0), "used": np.full(1, 9, dtype=np.uint64),
             "fit": np.full(n_rep + 1, -7.0), "aligned": np.full((n_rep + 1, K, n_ind), -7.0), "dist0": np.full(N().n_pairs(n_ind), -7.0)}
        ptr = {"status": u32p, "used": u64p}
        p = {k: v.ctypes.data_as(ptr.get(k, dp)) for k, v in o.items()}
        mp = maps.ctypes.data_as(u64p)
        nb = n_sites // q

        def job(K_=K, ci=0.95, n_rep_=n_rep, maps_=mp, **null):
            args = [None if k in null else p[k] for k in o]
            return L.ngd_run_job_mds_align(e._h, maps_, n_rep_, nb, q, 0, 1, K_, ci, *args)

        for name in ("eig0", "vec0", "tot0", "status", "stats", "used", "fit"):
            assert job(**{name: True}) == -1, name
        assert job(K_=17) == -1 and job(ci=1.5) == -1 and job(n_rep_=0) == -1 and job(maps_=None) == -1
        assert L.ngd_run_job_mds_align(None, mp, n_rep, nb, q, 0, 1, K, 0.95, *[p[k] for k in o]) == -1
        assert L.ngd_mds_align_values_device(e._h, C.c_void_p(dev.data_ptr()), None, 1, 4, K, None, p["fit"]) == -1
        assert L.ngd_mds_align_values_device(e._h, C.c_void_p(dev.data_ptr()), None, 1, 4, K, p["aligned"], None) == -1
        assert L.ngd_mds_align_values_device(None, C.c_void_p(dev.data_ptr()), None, 1, 4, K, p["aligned"], p["fit"]) == -1
        for k, v in o.items():
            assert np.all(v == (9 if k in ptr else -7.0)), k
        assert job(aligned=True, dist0=True) == 0 and np.all(o["aligned"] == -7.0) and np.all(o["dist0"] == -7.0)
        assert np.array_equal(bits(o["stats"]), bits(first["stats"])) and np.array_equal(bits(o["fit"]), bits(first["fit"]))
    with N().Engine(n_ind, n_sites, kernel="mfma", shard_rank=0, shard_world=2) as e:
        e.synth_fill(2).commit()
        with pytest.raises(N().NgdError) as ei:
            e.run_job_mds_align(K, maps, q)
        assert ei.value.code == -1 and "share of the pairs" in str(ei.value)


# ---- 4. repeated calls leave free device memory where it was ---------------------------------------------------------------
def test_repeated_calls_do_not_leak():
    import torch
    n, K, n_rep, q = 65, 4, 5, 4
    t = N().Taus(5)
    maps = np.stack([t.block_map(64 // q) for _ in range(n_rep)])
    _, _, Xs = seen(np.stack([A.planted(n, K, n_rep, seed=s) for s in range(2)]))
    with N().Engine(n, 64, kernel="mfma") as e:
        e.synth_fill(3).commit()
        e.set_option("boot_partials", 0)
        dev = upload(A.kn(Xs))
        first = e.mds_align_values(dev.data_ptr(), 2, n_rep + 1, K)
        firstj = e.run_job_mds_align(K, maps, q)
        held, free = e.device_bytes(), torch.cuda.mem_get_info()[0]
        for _ in range(5):
            again = e.mds_align_values(dev.data_ptr(), 2, n_rep + 1, K)
            assert np.array_equal(bits(again[0]), bits(first[0])) and np.array_equal(bits(again[1]), bits(first[1]))
            assert np.array_equal(bits(e.run_job_mds_align(K, maps, q)["stats"]), bits(firstj["stats"]))
        assert e.device_bytes() == held and torch.cuda.mem_get_info()[0] == free
