"""Neighbour-joining trees on the device (nj.hip k_nj, engine_nj.hip nj_reduce) at the sizes test_gpu_nj.py stops short of.

A lane of the scan walks a row in batches of NJ_LOADS * 128 = 1024 columns, eight 16-byte loads a batch.  Up to n = 257 the
batch loop makes one trip and unroll slots 0 .. 2 alone hold a live column; here n = 1023 .. 1153 and 2049 put the clamp to
the last live pair of columns and the two masks of NJ_CONSIDER where a row ends in the first, second and third batch.  The
yardstick is ngd_nj_host (test_nj_cpu.py holds it to the dictionary statement nj_expect.py), bit for bit; where the two
could be wrong alike, the additive tree's exact recovery and the (0, 1) first join of an all-tie matrix do not go through
it.  Further: a cell that is not finite wherever it sits; sums and counts (k_nj<false>) on planted tensors, where phase
one's lane loop makes a second trip and a NaN comes from the logarithm; the workgroups of 256 and 512 threads (NGD_NJ_WG),
whose bits must be the default's; and a call cut into chunks of whole rounds of the CUs.
The cap n = 4096 is left out on purpose: the host twin needs about half a minute per matrix there.
Models 1 and 2 use test_gpu_nj.check_close as it is (bipartitions equal, |len_dev - len_host| <= 1e-9 max|d|, given a
smallest relative Q gap of 1e-8 at m >= 5).  The largest seen on an MI355X over the cases of this file:
8.11e-16 (bound 1e-9; n = 130, model 2), with a smallest relative Q gap at m >= 5 of 3.04e-6 (required: 1e-8); at n = 3 and 4,
where the lengths alone are compared, 1.59e-16."""
import functools

import numpy as np
import pytest

import nj_expect as X
import test_gpu_nj as TN
from test_gpu_nj import N, bits, check_close, device_buffers, finish, on_device, same

pytestmark = pytest.mark.gpu


def engine(n):
    e = N().Engine(n, 16, kernel="mfma")
    e.synth_fill(1).commit()
    return e


def rows(t, k):
    """matrices k of a (child, len, status) triple"""
    return tuple(x[k] for x in t)


# ---- a. values as they are, past one batch of the scan ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def six(n):
    """-> (values [6][n_pairs], the additive tree, the host twin's records): random, all cells equal, small integers, all
    cells 0, an additive tree, and a random one with NaN in its last pair (n - 2, n - 1)"""
    p = n * (n - 1) // 2
    rng = np.random.default_rng(n)
    v = np.empty((6, p))
    v[0] = rng.uniform(0.05, 1.5, size=p)
    v[1] = 0.25
    v[2] = rng.integers(1, 4, size=p)
    v[3] = 0.0
    tree = X.random_tree(n, n)
    v[4] = tree[0]
    v[5] = rng.uniform(0.05, 1.5, size=p)
    v[5, p - 1] = np.nan
    return v, tree, N().nj_host(v, n)


def check_six(got, n):
    v, tree, want = six(n)
    assert same(got, want)
    assert got[0].shape == (6, 2 * n - 3) and got[2].tolist() == [1, 1, 1, 1, 1, 0]
    assert np.all(got[0][5] == -1) and np.all(bits(got[1][5]) == X.NAN_BITS)
    # every decision a tie: the first join is (0, 1)
    for k in (1, 3):
        assert got[0][k][0] == 0 and got[0][k][1] == 1, k
    # the additive tree comes back exactly (no host twin in this one)
    assert set(X.record_splits(got[0][4], n)) == tree[1]
    assert np.array_equal(bits(np.sort(got[1][4])), bits(np.array(tree[2])))


# 1023: odd, a padded row, one column short of a full batch; 1024: every unroll slot live, one batch; 1025: lane 0 of row 0
# makes the second trip, for the first join only; 1026: even; 1153: two unroll slots of the second trip over 129 joins
@pytest.mark.parametrize("n", [1023, 1024, 1025, 1026, 1153])
def test_values_form_past_one_scan_batch(n):
    with engine(n) as e:
        got = on_device(e, six(n)[0])
    check_six(got, n)


def test_values_form_in_a_third_batch():
    """n = 2049: no tree among the matrices (random_tree alone costs 4 s there)"""
    n = 2049
    p = n * (n - 1) // 2
    v = np.empty((3, p))
    v[0] = np.random.default_rng(n).uniform(0.05, 1.5, size=p)
    v[1] = 0.25
    v[2] = 0.0
    with engine(n) as e:
        got = on_device(e, v)
    assert same(got, N().nj_host(v, n)) and got[2].tolist() == [1, 1, 1]
    for k in (1, 2):
        assert got[0][k][0] == 0 and got[0][k][1] == 1, k


# ---- b. where a cell that is not finite sits ------------------------------------------------------------------------------
def test_one_cell_that_is_not_finite_wherever_it_sits():
    n = 130
    p = n * (n - 1) // 2
    pair = lambda a, b: a * n - a * (a + 1) // 2 + (b - a - 1)  # noqa: E731
    v = np.random.default_rng(130).uniform(0.05, 1.5, size=(9, p))
    assert pair(0, 1) == 0 and pair(n - 2, n - 1) == p - 1
    planted = {1: (0, np.nan), 3: (p - 1, np.nan), 5: (pair(0, n - 1), np.inf), 7: (pair(64, 65), -np.inf)}
    for k, (at, x) in planted.items():
        v[k, at] = x
    with engine(n) as e:
        got = on_device(e, v)
    want = N().nj_host(v, n)
    assert got[2].tolist() == [1, 0, 1, 0, 1, 0, 1, 0, 1] and np.array_equal(want[2], got[2])
    for k in range(9):
        if k in planted:
            assert np.all(got[0][k] == -1) and np.all(bits(got[1][k]) == X.NAN_BITS), k
        else:
            assert same(rows(got, [k]), rows(want, [k])), k


# ---- c. sums and counts (k_nj<false>) on planted tensors ---------------------------------------------------------------------
def sums(n):
    p = n * (n - 1) // 2
    rng = np.random.default_rng(n)
    Cn = rng.integers(50, 400, (4, p))
    S = rng.uniform(0.05, 0.6, (4, p)) * Cn
    return S, Cn.astype(np.uint64)


def upload(S, Cn):
    import torch
    ds, dc = device_buffers(S.shape)
    ds.copy_(torch.from_numpy(S))
    dc.copy_(torch.from_numpy(Cn.astype(np.int64)))
    torch.cuda.synchronize()
    return ds, dc


def check_lengths(got, d, n, what):
    """n = 3, 4: no step has m >= 5, so check_close's condition has nothing to say; the lengths alone, under its bound,
    branch by branch (at n = 4 the pair and its complement tie in exact arithmetic and make one tree; the three pairings' Q
    of these inputs lie 1e-3 relative and more apart)"""
    want = N().nj_host(d, n)
    assert np.array_equal(got[2], want[2]) and np.all(want[2] == 1)
    worst = 0.0
    for k in range(d.shape[0]):
        eg, eh = X.record_edges(got[0][k], got[1][k], n), X.record_edges(want[0][k], want[1][k], n)
        assert set(eg) == set(eh), "%s: matrix %d: the bipartitions differ" % (what, k)
        worst = max(worst, max(abs(eg[s] - eh[s]) for s in eh) / np.abs(d[k]).max())
    print("%s: largest |len_dev - len_host| / max|d| %.3g (bound %g)" % (what, worst, TN.RTOL))
    assert worst <= TN.RTOL


@pytest.mark.parametrize("n", [3, 4, 65, 130])
def test_sums_and_counts_form_on_planted_tensors(n):
    S, Cn = sums(n)
    with N().Engine(n, 16) as e:
        e.synth_fill(1).commit()
        ds, dc = upload(S, Cn)
        got = [e.nj(ds.data_ptr(), dc.data_ptr(), 4, evol_model=m) for m in (0, 1, 2)]
        if n == 130:  # --tot_sites: d_cnt is not read (a null pointer here)
            tot = e.nj(ds.data_ptr(), None, 4, evol_model=0, tot_sites=1234)
    assert same(got[0], N().nj_host(finish(S, Cn, 0), n)) and np.all(got[0][2] == 1)
    for m in (1, 2):
        (check_close if n >= 5 else check_lengths)(got[m], finish(S, Cn, m), n, "planted sums n = %d model %d" % (n, m))
    if n == 130:
        assert same(tot, N().nj_host(finish(S, Cn, 0, 1234), n)) and np.all(tot[2] == 1)


def test_a_nan_from_the_logarithm_leaves_the_other_matrices_alone():
    n = 130
    S, Cn = sums(n)
    S[2, -1] = 0.8 * Cn[2, -1]  # pair (n - 2, n - 1) of matrix 2: 1 - 0.8 * 4 / 3 < 0 ... and 1 - 0.8 > 0: model 2 alone
    S[1, -1] = 1.25 * Cn[1, -1]  # matrix 1: 1 - 1.25 < 0 under model 1 as well
    d1, d2 = finish(S, Cn, 1), finish(S, Cn, 2)
    assert np.isnan(d1[1, -1]) and np.isfinite(d1[2, -1]) and np.isnan(d2[1, -1]) and np.isnan(d2[2, -1])
    assert np.isfinite(np.delete(d1, 1, 0)).all() and np.isfinite(d2[[0, 3]]).all()
    with N().Engine(n, 16) as e:
        e.synth_fill(1).commit()
        ds, dc = upload(S, Cn)
        for m, status in ((1, [1, 0, 1, 1]), (2, [1, 0, 0, 1])):
            got = e.nj(ds.data_ptr(), dc.data_ptr(), 4, evol_model=m)
            assert got[2].tolist() == status, m
            for k in range(4):
                alone = e.nj(ds[k].data_ptr(), dc[k].data_ptr(), 1, evol_model=m)
                assert same(alone, rows(got, [k])), (m, k)
                if not status[k]:
                    assert np.all(got[0][k] == -1) and np.all(bits(got[1][k]) == X.NAN_BITS), (m, k)


# ---- d. the other workgroups: a tree's bits depend on its matrix alone -----------------------------------------------------
@functools.lru_cache(maxsize=None)
def small_set(n):
    v, tree = TN.planted(n, 37, n)
    return v, N().nj_host(v, n)


@pytest.mark.parametrize("wg", ["256", "512", "1024", "300"])
def test_every_workgroup_size_gives_the_host_twins_bits(wg, monkeypatch):
    """NGD_NJ_WG is read on every call; a value outside 256, 512, 1024 is the default"""
    for n in (5, 65, 1153):
        v, want = small_set(n) if n < 1000 else (six(n)[0], six(n)[2])
        with engine(n) as e:
            monkeypatch.setenv("NGD_NJ_WG", wg)
            got = on_device(e, v)
            monkeypatch.delenv("NGD_NJ_WG")
            if wg == "300":
                assert same(got, on_device(e, v)), n
        assert same(got, want), (wg, n)
        if n == 1153:
            check_six(got, n)


# ---- e. chunks of whole rounds of the CUs -----------------------------------------------------------------------------------
def test_chunks_of_whole_cu_rounds_change_no_bit():
    import torch
    n = 5
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    n_mat = 2 * n_cu + 200
    v = np.random.default_rng(5).uniform(0.05, 1.5, size=(n_mat, n * (n - 1) // 2))
    with engine(n) as e:
        whole = on_device(e, v)
        # a working copy is 5 rows of 6 doubles: n_cu + 44 matrices fit, rounded down to n_cu -- three launches, the last partial
        e.set_option("nj_max_bytes", (n_cu + 44) * 5 * 6 * 8)
        cut = on_device(e, v)
    assert 200 < n_cu + 44 < n_mat
    assert same(cut, whole) and same(cut, N().nj_host(v, n)) and np.all(cut[2] == 1)
