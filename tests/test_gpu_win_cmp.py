"""Comparison of windows on the device (ngd_win_cmp*_device, ngd_run_windows_cmp; win_cmp.hip).

The values form against the extended-precision expectation of win_cmp_expect.py (gram, mean, rms^2 and cor within the
contract's bounds) and against the host twin, at W in {1, 2, 15, 16, 17, 33, 65} -- the MFMA tile's edges and more tile
blocks than one wavefront owns -- and P in {1, 3, 4, 5, s - 1, s, s + 1, 2 s + 3}, s = win_cmp_slice(W, P): the k-group's
edges and a slice's.  Bits: gram symmetric; a permutation of the vectors permutes mean and gram; a status-0 vector replaced
by a finite one changes nothing outside its row and column; a repeated call; scaling by 2^k.  Sums and counts under models
0, 1 and 2 and with missing data under --pairwise_del against the expectation on host-finished distances.  The run form equals
ngd_win_cmp_device on the _device sibling's output bit for bit, dist ngd_run_windows_dist's, in one group of windows and in
several; once on the EM path.  Every refusal by code and message, the budget's included; free device memory after 20 calls.

Every comparison prints its largest figure in units of its bound.  The largest seen on an MI355X over the cases of this
file (bound 1e-9 each, 3e-9 for cor): gram 1.7e-15 of sqrt(exact[a][a] exact[b][b]), mean 3.2e-16 of mean |x|, rms^2 2.6e-15 of
(exact[a][a] + exact[b][b] + P (mean[a] - mean[b])^2) / P, cor 2.4e-15 absolute, device against host twin 1.3e-15."""
import ctypes as C

import numpy as np
import pytest

import win_cmp_expect as X

pytestmark = pytest.mark.gpu


def N():
    import ngsdist_amd
    return ngsdist_amd


def synth(seed, n_ind, n_sites, miss_frac=0.0):
    from oracle import oracle as O
    return O.synth_indmajor(seed, n_ind, n_sites, miss_frac=miss_frac)


def bits(x):
    return X.bits(x)


def same(a, b):
    """two (mean, gram, status) tuples, bit for bit"""
    return (np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1])) and
            np.array_equal(np.asarray(a[2]), np.asarray(b[2])))


def on_device(e, v):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to("cuda")
    torch.cuda.synchronize()
    return e.win_cmp_values(t.data_ptr(), v.shape[0], v.shape[1])


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


@pytest.fixture(scope="module")
def engine():
    with N().Engine(8, 16, kernel="mfma") as e:  # (the values form is not tied to the engine's n_ind)
        e.synth_fill(1).commit()
        yield e


# ---- 1. values as they are --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", X.WS)
def test_values_form_against_the_expectation_and_the_host_twin(engine, W):
    for P in X.P_of(W, N().win_cmp_slice):
        v, at = X.vectors(W, P)
        exp = X.expect(v)
        mean, gram, status = on_device(engine, v)
        X.check_all(v, mean, gram, status, N().win_cmp_finish, "device", exp)
        X.check_twin(mean, gram, status, *N().win_cmp_host(v), exp, "W=%d P=%d" % (W, P))
        if "dup" in at:
            _, rms = N().win_cmp_finish(mean, gram, status, P)
            assert rms[0, 1] == 0.0 and bits(mean[:1])[0] == bits(mean[1:2])[0] and gram[0, 0] == gram[0, 1] == gram[1, 1]
        for k in ("zero", "pow2"):
            if k in at:
                ok = status == 1
                assert np.all(gram[at[k]][ok] == 0.0) and mean[at[k]] == v[at[k], 0]
    ms = engine.last_win_cmp_ms()
    assert set(ms) == {"stats", "pack", "gram", "sum"} and all(x > 0 for x in ms.values())


# ---- 2. bits -----------------------------------------------------------------------------------------------------------------
def test_bits_permutation_company_repetition_and_scaling(engine):
    W = 33
    P = 2 * N().win_cmp_slice(W, 1) + 3
    assert N().win_cmp_slice(W, P) == N().win_cmp_slice(W, 1)
    v, at = X.vectors(W, P)
    first = on_device(engine, v)
    mean, gram, status = first
    assert same(on_device(engine, v), first)  # a repeated call
    # pairs change tile, tile block and side of the diagonal
    perm = np.random.default_rng(7).permutation(W)
    pm, pg, ps = on_device(engine, v[perm])
    assert np.array_equal(ps, status[perm]) and np.array_equal(bits(pm), bits(mean[perm]))
    assert np.array_equal(bits(pg), bits(gram[np.ix_(perm, perm)]))
    rev = on_device(engine, v[::-1])
    assert np.array_equal(bits(rev[1]), bits(gram[::-1, ::-1]))
    # the status-0 vector replaced by a finite one: no bit outside its row and column changes
    w = v.copy()
    w[at["bad"]] = np.random.default_rng(8).random(P)
    fm, fg, fs = on_device(engine, w)
    keep = np.arange(W) != at["bad"]
    assert fs.tolist() == [1] * W
    assert np.array_equal(bits(fg[np.ix_(keep, keep)]), bits(gram[np.ix_(keep, keep)])) and np.array_equal(bits(fm[keep]), bits(mean[keep]))
    # scaling by a power of two is exact
    ok = status == 1
    for k in (-40, -7, 1, 40):
        m2, g2, s2 = on_device(engine, np.ldexp(v, k))
        assert np.array_equal(s2, status)
        assert np.array_equal(bits(m2[ok]), bits(np.ldexp(mean[ok], k))), k
        assert np.array_equal(bits(g2[np.ix_(ok, ok)]), bits(np.ldexp(gram[np.ix_(ok, ok)], 2 * k))), k


# ---- 3. sums and counts ------------------------------------------------------------------------------------------------------
LO, HI = np.array([0, 0, 1, 5, 10, 16, 32, 40, 63]), np.array([64, 32, 64, 6, 12, 48, 64, 64, 64])  # (starts do not decrease)


def check_finished(got, d, what):
    """the device's result on sums and counts against the expectation on host-finished distances `d` (the device's log may
    differ from the host's by an ulp: far inside the contract)"""
    return X.check_all(d, got[0], got[1], got[2], N().win_cmp_finish, what)


@pytest.mark.parametrize("model", [0, 1, 2])
def test_sums_and_counts_against_the_expectation_on_finished_distances(model):
    n_ind, n_sites = 20, 64
    n_pairs, n_win = N().n_pairs(n_ind), len(LO)
    with N().Engine(n_ind, n_sites, kernel="mfma") as e:
        e.synth_fill(11).commit()
        ds, dc = device_buffers((n_win, n_pairs))
        e.run_windows(LO, HI, d_sum_ptr=ds.data_ptr(), d_cnt_ptr=dc.data_ptr())
        S, Cn = to_host(ds, dc)
        got = e.win_cmp(ds.data_ptr(), dc.data_ptr(), n_win, evol_model=model)
        check_finished(got, finish(S, Cn, model), "sums and counts, model %d" % model)
        if model == 0:  # --tot_sites: d_cnt is not read (a null pointer here)
            got = e.win_cmp(ds.data_ptr(), None, n_win, evol_model=0, tot_sites=1234)
            check_finished(got, finish(S, Cn, 0, 1234), "sums and counts, tot_sites")
            assert got[2].tolist() == [1] * n_win


def test_a_pair_without_sites_under_pairwise_deletion_leaves_its_window_out():
    n_ind, n_sites = 20, 64
    n_pairs, n_win = N().n_pairs(n_ind), len(LO)
    with N().Engine(n_ind, n_sites, kernel="mfma", pairwise_del=True) as e:
        e.synth_fill(12, 0.3).commit()
        ds, dc = device_buffers((n_win, n_pairs))
        e.run_windows(LO, HI, d_sum_ptr=ds.data_ptr(), d_cnt_ptr=dc.data_ptr())
        S, Cn = to_host(ds, dc)
        got = e.win_cmp(ds.data_ptr(), dc.data_ptr(), n_win, evol_model=0)
        check_finished(got, finish(S, Cn, 0), "sums and counts, --pairwise_del")
        none = (Cn == 0).any(axis=1)
        assert none.any() and not none.all() and np.array_equal(got[2] == 0, none)
        whole = e.run_windows_cmp(LO, HI, evol_model=0)
        assert same(whole[:3], got) and np.array_equal(bits(whole[3]), bits(e.run_windows_dist(LO, HI, 0)))


# ---- 4. the run form against its siblings ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(20, 64, "mfma", True), (33, 48, "em_table", False)])
def test_run_windows_cmp_equals_its_siblings(shape):
    n_ind, n_sites, kernel, indep = shape
    lo, hi = np.minimum(LO, n_sites - 1), np.minimum(HI, n_sites)
    n_pairs, n_win = N().n_pairs(n_ind), len(lo)
    with N().Engine(n_ind, n_sites, kernel=kernel, indep_geno=indep) as e:
        e.upload_ind_major(synth(17, n_ind, n_sites)).commit()
        mean, gram, status, dist = e.run_windows_cmp(lo, hi, evol_model=1)
        assert mean.shape == (n_win,) and gram.shape == (n_win, n_win) and status.shape == (n_win,) and dist.shape == (n_win, n_pairs)
        ds, dc = device_buffers((n_win, n_pairs))
        e.run_windows(lo, hi, d_sum_ptr=ds.data_ptr(), d_cnt_ptr=dc.data_ptr())
        assert same((mean, gram, status), e.win_cmp(ds.data_ptr(), dc.data_ptr(), n_win, evol_model=1))
        assert np.array_equal(bits(dist), bits(e.run_windows_dist(lo, hi, 1)))
        assert e.run_windows_cmp(lo, hi, evol_model=1, dist=False)[3] is None
        S, Cn = to_host(ds, dc)
        check_finished((mean, gram, status), finish(S, Cn, 1), "run form %s" % kernel)


@pytest.mark.parametrize("per_group", [2, 3])
def test_groups_of_windows_change_no_bit(per_group, monkeypatch):
    # 9 windows in 5 and in 3 groups (the driver's groups hold the same number of windows each, so 9 cannot fall into 4), under
    # the per-window plan: a window's sums do not depend on the windows beside it there (test_gpu_tail_groups_of_windows.py)
    n_ind, n_sites = 20, 64
    n_pairs = N().n_pairs(n_ind)
    with N().Engine(n_ind, n_sites, kernel="mfma") as e:
        e.upload_ind_major(synth(19, n_ind, n_sites)).commit()
        e.set_option("win_plan", 1)
        monkeypatch.delenv("NGD_TEST_WIN_GROUP_BYTES", raising=False)
        one = e.run_windows_cmp(LO, HI, evol_model=2)
        monkeypatch.setenv("NGD_ENABLE_TEST_HOOKS", "1")
        monkeypatch.setenv("NGD_TEST_WIN_GROUP_BYTES", str(per_group * 16 * n_pairs))
        many = e.run_windows_cmp(LO, HI, evol_model=2)
        assert same(one[:3], many[:3]) and np.array_equal(bits(one[3]), bits(many[3]))


# ---- 5. refusals: by code and message, before anything is launched; outputs and engine as they were ------------------------
def test_refusals_leave_outputs_and_engine_as_they_were():
    n_ind, n_sites = 10, 64
    n_pairs = N().n_pairs(n_ind)
    lo, hi = np.array([0, 8, 30]), np.array([64, 40, 64])
    with N().Engine(n_ind, n_sites, kernel="mfma", pairwise_del=True) as e:
        e.synth_fill(2, 0.1).commit()
        first = e.run_windows_cmp(lo, hi)
        ds, dc = device_buffers((3, n_pairs))
        e.run_windows(lo, hi, d_sum_ptr=ds.data_ptr(), d_cnt_ptr=dc.data_ptr())
        sp, cp = ds.data_ptr(), dc.data_ptr()
        calls = [
            (lambda: e.win_cmp(sp, cp, 0), -1, "no vectors"),
            (lambda: e.win_cmp(None, cp, 3), -1, "null matrices"),
            (lambda: e.win_cmp(sp, None, 3), -1, "null matrices"),
            (lambda: e.win_cmp(sp, cp, 3, tot_sites=9), -1, "pairwise deletion"),
            (lambda: e.win_cmp(sp, cp, 3, evol_model=3), -5, "model"),
            (lambda: e.win_cmp(sp, cp, N().win_cmp_max_vec() + 1), -1, "ngd_win_cmp_max_vec"),
            (lambda: e.win_cmp_values(None, 2, 5), -1, "null vectors"),
            (lambda: e.win_cmp_values(sp, 0, 5), -1, "no vectors"),
            (lambda: e.win_cmp_values(sp, 2, 0), -1, "no cells"),
            (lambda: e.win_cmp_values(sp, N().win_cmp_max_vec() + 1, 5), -1, "ngd_win_cmp_max_vec"),
            (lambda: e.run_windows_cmp(lo, hi, evol_model=7), -5, "model"),
            (lambda: e.run_windows_cmp(lo, hi, tot_sites=50), -1, "pairwise deletion"),
            (lambda: e.run_windows_cmp(lo[:0], hi[:0]), -1, ""),
            (lambda: e.run_windows_cmp(lo, hi + 1), -1, ""),  # the windows' own refusal
        ]
        for k, (call, code, words) in enumerate(calls):
            with pytest.raises(N().NgdError) as ei:
                call()
            assert ei.value.code == code and words in str(ei.value), (k, str(ei.value))
            assert same(e.run_windows_cmp(lo, hi)[:3], first[:3]), k
        # the budget: the bytes needed are named, nothing has run
        e.set_option("win_cmp_max_bytes", 1)
        for call in (lambda: e.win_cmp(sp, cp, 3), lambda: e.win_cmp_values(sp, 3, n_pairs), lambda: e.run_windows_cmp(lo, hi)):
            with pytest.raises(N().NgdError) as ei:
                call()
            assert ei.value.code == -1 and "NGD_OPT_WIN_CMP_MAX_BYTES" in str(ei.value) and " bytes " in str(ei.value)
        # null outputs through the C interface; a refused call writes nothing
        L = e._L
        m, g, st = np.full(3, -7.0), np.full((3, 3), -7.0), np.full(3, 9, dtype=np.uint32)
        d = np.full((3, n_pairs), -7.0)
        dp = C.POINTER(C.c_double)
        mp, gp, stp, dd = m.ctypes.data_as(dp), g.ctypes.data_as(dp), st.ctypes.data_as(C.POINTER(C.c_uint32)), d.ctypes.data_as(dp)
        lp, hp = (x.astype(np.uint64) for x in (lo, hi))
        lpp, hpp = lp.ctypes.data_as(C.POINTER(C.c_uint64)), hp.ctypes.data_as(C.POINTER(C.c_uint64))
        assert L.ngd_run_windows_cmp(e._h, lpp, hpp, 3, 0, 1, mp, gp, stp, dd) == -1  # (the budget)
        assert L.ngd_win_cmp_device(e._h, C.c_void_p(sp), C.c_void_p(cp), 3, 0, 1, mp, gp, stp) == -1
        e.set_option("win_cmp_max_bytes", 0)
        assert L.ngd_run_windows_cmp(e._h, lpp, hpp, 3, 0, 1, None, gp, stp, dd) == -1
        assert L.ngd_run_windows_cmp(e._h, lpp, hpp, 3, 0, 1, mp, None, stp, dd) == -1
        assert L.ngd_run_windows_cmp(e._h, lpp, hpp, 3, 0, 1, mp, gp, None, dd) == -1
        assert L.ngd_run_windows_cmp(e._h, None, hpp, 3, 0, 1, mp, gp, stp, dd) == -1
        assert L.ngd_run_windows_cmp(None, lpp, hpp, 3, 0, 1, mp, gp, stp, dd) == -1
        assert L.ngd_win_cmp_device(e._h, C.c_void_p(sp), C.c_void_p(cp), 3, 0, 4, mp, gp, stp) == -5
        assert L.ngd_win_cmp_values_device(None, C.c_void_p(sp), 3, 5, mp, gp, stp) == -1
        assert L.ngd_win_cmp_values_device(e._h, C.c_void_p(sp), 3, 5, mp, None, stp) == -1
        assert L.ngd_last_win_cmp_ms(e._h, None) == -1
        assert np.all(m == -7.0) and np.all(g == -7.0) and np.all(st == 9) and np.all(d == -7.0)
        assert same(e.run_windows_cmp(lo, hi)[:3], first[:3])
    with N().Engine(n_ind, n_sites, kernel="mfma", shard_rank=0, shard_world=2) as e:
        e.synth_fill(2).commit()
        with pytest.raises(N().NgdError) as ei:
            e.run_windows_cmp(lo, hi)
        assert ei.value.code == -1 and "share of the pairs" in str(ei.value)


# ---- 6. repeated calls leave free device memory where it was ---------------------------------------------------------------
def test_repeated_calls_do_not_leak():
    import torch
    v, _ = X.vectors(17, 300)
    with N().Engine(20, 64, kernel="mfma") as e:
        e.synth_fill(3).commit()
        t = torch.from_numpy(v).to("cuda")
        torch.cuda.synchronize()
        first = e.win_cmp_values(t.data_ptr(), 17, 300)
        firstw = e.run_windows_cmp(LO, HI)
        held, free = e.device_bytes(), torch.cuda.mem_get_info()[0]
        for _ in range(20):
            assert same(e.win_cmp_values(t.data_ptr(), 17, 300), first)
            assert same(e.run_windows_cmp(LO, HI)[:3], firstw[:3])
        assert e.device_bytes() == held and torch.cuda.mem_get_info()[0] == free
