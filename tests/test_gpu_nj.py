"""Neighbour-joining trees built on the device (ngd_nj*_device, ngd_run_*_nj; nj.hip k_nj).

Values as they are, and sums and counts under evol_model 0 (the division carries the host's bits): the device's records
equal ngd_nj_host's bit for bit (test_nj_cpu.py checks that one against the dictionary statement nj_expect.py).  Models 1
and 2, where log is the device's: against the host twin on host-finished distances, the bipartition sets are equal and, per
bipartition, |len_dev - len_host| <= 1e-9 * max|d| (the project's parity tolerance), given that the host twin's smallest
relative gap between best and second-best Q over the steps with m >= 5 is at least 1e-8 -- asserted of the test's inputs.
The run forms equal ngd_nj_device on their _device sibling's output bit for bit, dist0 the _dist sibling's matrix 0.
Every comparison under models 1 and 2 prints its largest difference.  The largest seen on an MI355X over the cases of this
file: 4.27e-16 (bound 1e-9), with a smallest relative Q gap at m >= 5 of 1.2e-6 (required: 1e-8)."""
import ctypes as C

import numpy as np
import pytest

import nj_expect as X

pytestmark = pytest.mark.gpu

RTOL = 1e-9


def N():
    import ngsdist_amd
    return ngsdist_amd


def synth(seed, n_ind, n_sites, miss_frac=0.0):
    from oracle import oracle as O
    return O.synth_indmajor(seed, n_ind, n_sites, miss_frac=miss_frac)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def same(a, b):
    """two (child, len, status) triples, bit for bit"""
    return (np.array_equal(np.asarray(a[0]).ravel(), np.asarray(b[0]).ravel()) and
            np.array_equal(bits(a[1]).ravel(), bits(b[1]).ravel()) and np.array_equal(np.asarray(a[2]).ravel(), np.asarray(b[2]).ravel()))


def on_device(e, v):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to("cuda")
    torch.cuda.synchronize()
    return e.nj_values(t.data_ptr(), v.shape[0])


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


def planted(n, n_mat, seed):
    """random matrices with an all-equal one, a small-integer one, an additive tree and a NaN one in the middle"""
    p = n * (n - 1) // 2
    rng = np.random.default_rng(seed)
    v = rng.uniform(0.05, 1.5, size=(n_mat, p))
    tree = None
    if n_mat >= 20:
        v[5] = 0.25
        v[6] = rng.integers(1, 4, size=p)
        tree = X.random_tree(n, seed)
        v[7] = tree[0]
        v[n_mat // 2, p // 2] = np.nan
    return v, tree


# ---- 1. values as they are: wave boundaries (63, 64, 65), a workgroup's edges (3, 4, 5), more rows than waves (130, 257) ----
@pytest.mark.parametrize("n", [3, 4, 5, 63, 64, 65, 130, 257])
def test_values_form_equals_the_host_twin(n):
    v, tree = planted(n, 37, n)
    with N().Engine(n, 16, kernel="mfma") as e:
        e.synth_fill(1).commit()
        got = on_device(e, v)
        assert e.last_nj_ms() > 0
        one = on_device(e, v[3:4])
        mid = on_device(e, v[18:19])
    want = N().nj_host(v, n)
    assert same(got, want)
    assert got[0].shape == (37, 2 * n - 3) and got[2].tolist() == [1] * 18 + [0] + [1] * 18
    assert np.all(got[0][18] == -1) and np.all(bits(got[1][18]) == X.NAN_BITS)
    # a matrix served alone carries the bits it has among 37; so does the one without a tree
    assert same(one, tuple(x[3:4] for x in got)) and same(mid, tuple(x[18:19] for x in got))
    # the all-equal matrix: every decision a tie, the first join (0, 1)
    if n > 3:
        assert got[0][5][0] == 0 and got[0][5][1] == 1
    # the additive tree comes back exactly
    assert set(X.record_splits(got[0][7], n)) == tree[1]
    assert np.array_equal(bits(np.sort(got[1][7])), bits(np.array(tree[2])))


def test_chunks_change_no_bit():
    n = 65
    v, _ = planted(n, 7, 99)
    with N().Engine(n, 16, kernel="mfma") as e:
        e.synth_fill(1).commit()
        whole = on_device(e, v)
        e.set_option("nj_max_bytes", 3 * n * (n + 1) * 8)  # 3 + 3 + 1 (a working row is n doubles rounded up to even: 66)
        three = on_device(e, v)
        e.set_option("nj_max_bytes", 1)  # never fewer than one matrix
        seven = on_device(e, v)
    assert same(whole, N().nj_host(v, n)) and same(three, whole) and same(seven, whole)


# ---- 2. sums and counts ----------------------------------------------------------------------------------------------------
def test_model_0_is_the_host_twin_on_finished_distances():
    n_ind, n_sites, n_rep, q = 24, 200, 6, 5
    n_pairs = N().n_pairs(n_ind)
    t = N().Taus(5)
    maps = np.stack([t.block_map(n_sites // q) for _ in range(n_rep)])
    # --pairwise_del on sparse data: the counts differ from pair to pair
    with N().Engine(n_ind, n_sites, kernel="mfma", pairwise_del=True) as e:
        e.upload_ind_major(synth(7, n_ind, n_sites, miss_frac=0.5)).commit()
        e.set_option("boot_partials", 0)
        ds, dc = device_buffers((n_rep + 1, n_pairs))
        e.run_job(maps, q, d_sum_ptr=ds.data_ptr(), d_cnt_ptr=dc.data_ptr())
        S, Cn = to_host(ds, dc)
        assert len(np.unique(Cn[0])) > 1 and Cn.min() > 0
        got = e.nj(ds.data_ptr(), dc.data_ptr(), n_rep + 1, evol_model=0)
        assert same(got, N().nj_host(finish(S, Cn, 0), n_ind)) and np.all(got[2] == 1)
    # --tot_sites: d_cnt is not read (a null pointer here)
    with N().Engine(n_ind, n_sites, kernel="mfma") as e:
        e.upload_ind_major(synth(8, n_ind, n_sites)).commit()
        e.set_option("boot_partials", 0)
        ds, dc = device_buffers((n_rep + 1, n_pairs))
        e.run_job(maps, q, d_sum_ptr=ds.data_ptr(), d_cnt_ptr=dc.data_ptr())
        S, Cn = to_host(ds, dc)
        got = e.nj(ds.data_ptr(), None, n_rep + 1, evol_model=0, tot_sites=1234)
        assert same(got, N().nj_host(finish(S, Cn, 0, 1234), n_ind))


def check_close(got, d, n, what):
    """models 1 and 2: the device's records against the host twin's on the host-finished distances d [n_mat][n_pairs]"""
    want = N().nj_host(d, n)
    assert np.array_equal(got[2], want[2]) and np.all(want[2] == 1)
    gaps = []
    X.nj_many(d, n, gaps)
    min_gap = min(g for m, g in gaps if m >= 5)
    worst = 0.0
    for k in range(d.shape[0]):
        eg, eh = X.record_edges(got[0][k], got[1][k], n), X.record_edges(want[0][k], want[1][k], n)
        assert set(eg) == set(eh), "%s: matrix %d: the bipartitions differ" % (what, k)
        worst = max(worst, max(abs(eg[s] - eh[s]) for s in eh) / np.abs(d[k]).max())
    print("%s: smallest relative Q gap at m >= 5 %.3g; largest |len_dev - len_host| / max|d| %.3g (bound %g)" % (what, min_gap, worst, RTOL))
    assert min_gap >= 1e-8, "the inputs do not meet the test's condition"
    assert worst <= RTOL


@pytest.mark.parametrize("model", [1, 2])
def test_models_1_and_2_against_the_host_twin(model):
    n_rep, q = 5, 5
    for n_ind, n_sites, kernel in ((24, 1000, "mfma"), (40, 600, "em_table")):
        n_pairs = N().n_pairs(n_ind)
        t = N().Taus(3)
        maps = np.stack([t.block_map(n_sites // q) for _ in range(n_rep)])
        with N().Engine(n_ind, n_sites, kernel=kernel, indep_geno=kernel == "mfma") as e:
            e.upload_ind_major(synth(11, n_ind, n_sites)).commit()
            e.set_option("boot_partials", 0)
            ds, dc = device_buffers((n_rep + 1, n_pairs))
            e.run_job(maps, q, d_sum_ptr=ds.data_ptr(), d_cnt_ptr=dc.data_ptr())
            S, Cn = to_host(ds, dc)
            got = e.nj(ds.data_ptr(), dc.data_ptr(), n_rep + 1, evol_model=model)
        check_close(got, finish(S, Cn, model), n_ind, "%d x %d %s model %d" % (n_ind, n_sites, kernel, model))


# ---- 3. the run forms against their siblings ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(24, 1000, "mfma"), (40, 600, "em_table")])
def test_run_job_nj(shape):
    n_ind, n_sites, kernel = shape
    n_rep, q = 5, 4
    n_pairs = N().n_pairs(n_ind)
    t = N().Taus(5)
    maps = np.stack([t.block_map(n_sites // q) for _ in range(n_rep)])
    with N().Engine(n_ind, n_sites, kernel=kernel, indep_geno=kernel == "mfma") as e:
        e.upload_ind_major(synth(13, n_ind, n_sites)).commit()
        e.set_option("boot_partials", 0)  # (pins the plan: two calls of a job then agree bit for bit)
        got = e.run_job_nj(maps, q, evol_model=1)
        assert got[0].shape == (n_rep + 1, 2 * n_ind - 3) and got[2].tolist() == [1] * (n_rep + 1) and got[3].shape == (n_pairs,)
        assert e.last_nj_ms() > 0
        ds, dc = device_buffers((n_rep + 1, n_pairs))
        e.run_job(maps, q, d_sum_ptr=ds.data_ptr(), d_cnt_ptr=dc.data_ptr())
        assert same(got[:3], e.nj(ds.data_ptr(), dc.data_ptr(), n_rep + 1, evol_model=1))
        dist = e.run_job_dist(maps, q, 1)
        assert np.array_equal(bits(got[3]), bits(dist[0]))
        # n_rep = 0: a plain run's one tree
        plain = e.run_job_nj(None, evol_model=1)
        e.run_job(None, d_sum_ptr=ds.data_ptr(), d_cnt_ptr=dc.data_ptr())
        assert plain[0].shape == (1, 2 * n_ind - 3)
        assert same(plain[:3], e.nj(ds.data_ptr(), dc.data_ptr(), 1, evol_model=1))
        assert np.array_equal(bits(plain[3]), bits(e.run_job_dist(None, 1, 1)[0]))
        assert e.run_job_nj(maps, q, evol_model=1, dist0=False)[3] is None


@pytest.mark.parametrize("kernel", ["mfma", "em_table"])
def test_window_forms(kernel):
    n_ind, n_sites, n_rep, q = 24, 200, 4, 5
    n_pairs = N().n_pairs(n_ind)
    lo, hi = np.array([0, 0, 1, 10, 50, 60]), np.array([1, 200, 3, 14, 57, 160])  # [0, 1), [1, 3), [10, 14): shorter than a block
    maps, off = N().window_boot_maps(3, lo, hi, n_rep, q)
    n_win = len(lo)
    with N().Engine(n_ind, n_sites, kernel=kernel, indep_geno=kernel == "mfma") as e:
        e.upload_ind_major(synth(17, n_ind, n_sites)).commit()
        # plain windows
        got = e.run_windows_nj(lo, hi, evol_model=0)
        assert got[0].shape == (n_win, 1, 2 * n_ind - 3) and got[2].shape == (n_win, 1) and np.all(got[2] == 1)
        ds, dc = device_buffers((n_win, n_pairs))
        e.run_windows(lo, hi, d_sum_ptr=ds.data_ptr(), d_cnt_ptr=dc.data_ptr())
        assert same(got[:3], e.nj(ds.data_ptr(), dc.data_ptr(), n_win, evol_model=0))
        assert np.array_equal(bits(got[3]), bits(e.run_windows_dist(lo, hi, 0)))
        # replicates inside windows of unequal length: no block, no finite replicate, no tree; matrix 0 has one
        got = e.run_windows_job_var_nj(lo, hi, maps, off, q, evol_model=0, n_rep=n_rep)
        assert got[0].shape == (n_win, n_rep + 1, 2 * n_ind - 3) and got[2].shape == (n_win, n_rep + 1)
        short = (hi - lo) // q == 0
        assert short.sum() == 3 and np.all(got[2][:, 0] == 1)
        assert np.all(got[2][short, 1:] == 0) and np.all(got[2][~short, 1:] == 1)
        assert np.all(got[0][short, 1:] == -1) and np.all(bits(got[1][short, 1:]) == X.NAN_BITS)
        ds, dc = device_buffers((n_win, n_rep + 1, n_pairs))
        e.run_windows_job_var(lo, hi, maps, off, q, d_sum_ptr=ds.data_ptr(), d_cnt_ptr=dc.data_ptr(), n_rep=n_rep)
        assert same(got[:3], e.nj(ds.data_ptr(), dc.data_ptr(), n_win * (n_rep + 1), evol_model=0))
        dist = e.run_windows_job_var_dist(lo, hi, maps, off, q, 0, n_rep=n_rep)
        assert np.array_equal(bits(got[3]), bits(dist[:, 0]))
        # n_rep = 0 through the job form: the windows alone
        alone = e.run_windows_job_var_nj(lo, hi, None, np.zeros(n_win, dtype=np.uint64), q, evol_model=0, n_rep=0)
        assert same(alone[:3], e.run_windows_nj(lo, hi, evol_model=0)[:3])


# ---- 4. refusals: by code, before anything is launched; outputs and engine as they were -----------------------------------
def test_refusals_leave_the_engine_usable():
    n_ind, n_sites, n_rep, q = 10, 64, 4, 8
    t = N().Taus(2)
    maps = np.stack([t.block_map(n_sites // q) for _ in range(n_rep)])
    lo, hi = np.array([0, 8]), np.array([64, 40])
    wmaps, off = N().window_boot_maps(3, lo, hi, n_rep, q)
    n_pairs, nb = N().n_pairs(n_ind), 2 * n_ind - 3
    with N().Engine(n_ind, n_sites, kernel="mfma", pairwise_del=True) as e:
        e.synth_fill(2, 0.1).commit()
        e.set_option("boot_partials", 0)
        first = e.run_job_nj(maps, q)
        firstw = e.run_windows_job_var_nj(lo, hi, wmaps, off, q, n_rep=n_rep)
        ds, dc = device_buffers((n_rep + 1, n_pairs))
        e.run_job(maps, q, d_sum_ptr=ds.data_ptr(), d_cnt_ptr=dc.data_ptr())
        sp, cp = ds.data_ptr(), dc.data_ptr()
        calls = [
            (lambda: e.nj(sp, cp, 0), -1),                                       # n_mat 0
            (lambda: e.nj(None, cp, n_rep + 1), -1),                             # a null pointer
            (lambda: e.nj(sp, None, n_rep + 1), -1),
            (lambda: e.nj(sp, cp, n_rep + 1, tot_sites=9), -1),                  # with --pairwise_del
            (lambda: e.nj(sp, cp, n_rep + 1, evol_model=3), -5),
            (lambda: e.nj_values(None, 2), -1),
            (lambda: e.nj_values(sp, 0), -1),
            (lambda: e.run_job_nj(maps, q, evol_model=3), -5),
            (lambda: e.run_job_nj(maps, q, tot_sites=50), -1),
            (lambda: e.run_windows_nj(lo, hi, evol_model=7), -5),
            (lambda: e.run_windows_nj(lo, hi, tot_sites=50), -1),
            (lambda: e.run_windows_job_var_nj(lo, hi, wmaps, off, q, n_rep=n_rep, evol_model=7), -5),
            (lambda: e.run_windows_job_var_nj(lo, hi, wmaps, off, q, n_rep=n_rep, tot_sites=5), -1),
        ]
        for k, (call, code) in enumerate(calls):
            with pytest.raises(N().NgdError) as ei:
                call()
            assert ei.value.code == code, (k, str(ei.value))
            assert same(e.run_job_nj(maps, q)[:3], first[:3]), k
        assert same(e.run_windows_job_var_nj(lo, hi, wmaps, off, q, n_rep=n_rep)[:3], firstw[:3])
        # null outputs through the C interface; a refused call writes nothing
        L = e._L
        child, ln, st = np.full((n_rep + 1, nb), 77, dtype=np.int32), np.full((n_rep + 1, nb), -7.0), np.full(n_rep + 1, 9, dtype=np.uint32)
        chp, lnp, stp = (child.ctypes.data_as(C.POINTER(C.c_int32)), ln.ctypes.data_as(C.POINTER(C.c_double)),
                         st.ctypes.data_as(C.POINTER(C.c_uint32)))
        mp = maps.ctypes.data_as(C.POINTER(C.c_uint64))
        assert L.ngd_run_job_nj(e._h, mp, n_rep, n_sites // q, q, 0, 1, None, lnp, stp, None) == -1
        assert L.ngd_run_job_nj(e._h, mp, n_rep, n_sites // q, q, 0, 1, chp, None, stp, None) == -1
        assert L.ngd_run_job_nj(e._h, mp, n_rep, n_sites // q, q, 0, 1, chp, lnp, None, None) == -1
        assert L.ngd_run_job_nj(e._h, None, n_rep, n_sites // q, q, 0, 1, chp, lnp, stp, None) == -1
        assert L.ngd_nj_device(e._h, C.c_void_p(sp), C.c_void_p(cp), n_rep + 1, 0, 4, chp, lnp, stp) == -5
        assert L.ngd_nj_values_device(None, C.c_void_p(sp), 1, chp, lnp, stp) == -1
        assert np.all(child == 77) and np.all(ln == -7.0) and np.all(st == 9)
        assert same(e.run_job_nj(maps, q)[:3], first[:3])
    with N().Engine(n_ind, n_sites, kernel="mfma", shard_rank=0, shard_world=2) as e:
        e.synth_fill(2).commit()
        with pytest.raises(N().NgdError) as ei:
            e.run_job_nj(maps, q)
        assert ei.value.code == -1 and "share of the pairs" in str(ei.value)


def test_fewer_than_three_individuals_are_refused():
    with N().Engine(2, 64, kernel="mfma") as e:
        e.synth_fill(2).commit()
        with pytest.raises(N().NgdError) as ei:
            e.run_job_nj(None)
        assert ei.value.code == -1 and "three individuals" in str(ei.value)
        s, c = e.run()
        assert s.shape == (1,) and np.isfinite(s).all()


def test_more_individuals_than_the_cap_are_refused():
    n = N().nj_max_ind() + 1
    assert n > 1000
    with N().Engine(n, 16, kernel="mfma") as e:
        e.synth_fill(2).commit()
        with pytest.raises(N().NgdError) as ei:
            e.run_job_nj(None)
        assert ei.value.code == -1 and "ngd_nj_max_ind" in str(ei.value)
        s, c = e.run()
        assert np.isfinite(s).all()


# ---- 5. repeated calls leave free device memory where it was ---------------------------------------------------------------
def test_repeated_calls_do_not_leak():
    import torch
    n = 65
    v, _ = planted(n, 7, 5)
    with N().Engine(n, 64, kernel="mfma") as e:
        e.synth_fill(3).commit()
        t = torch.from_numpy(v).to("cuda")
        torch.cuda.synchronize()
        first = e.nj_values(t.data_ptr(), 7)
        firstj = e.run_job_nj(None)
        held, free = e.device_bytes(), torch.cuda.mem_get_info()[0]
        for _ in range(5):
            assert same(e.nj_values(t.data_ptr(), 7), first)
            assert same(e.run_job_nj(None)[:3], firstj[:3])
        assert e.device_bytes() == held and torch.cuda.mem_get_info()[0] == free
