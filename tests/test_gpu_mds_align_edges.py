"""Alignment of MDS replicates on the device (mds_align.hip k_mds_align through ngd_mds_align_values_device) where
test_gpu_mds_align.py's sets do not go: between a well separated M = X_r^T X_0 (planted sets: sigma_min / sigma_max >= 1/16 or
so) and an exactly singular one, and at every K.  Coordinates are uploaded as they are to a small engine of the same n_ind;
R = 3 throughout.  The reference is mpmath at 60 digits (mds_align_expect.procrustes_mp), computed once per input and shared
with the host twin's comparison: numpy's SVD is up to ten times further from it than the library is on graded matrices.

a. Every K: planted sets (n_set = 2) at n = 17, K = 1 .. 16, and n = 65, K = 3, 5, 7, 8, 9, 15, 16, by check_set against
   numpy and against the host twin -- the only place where K = 3 and 5 .. 15 run on the device (tid / K, tid % K, Mq[a * K +
   b], the `b < K` arms of the unrolled loops, the `done` mask).
b. Graded and clustered spectra at (n, K) = (5, 3), (17, 7), (17, 16), (65, 15), (65, 16): X_0's columns scaled by
   geomspace(1, g, K), g = 1e-1, 1e-3, 1e-5, replicates that differ from it by a generic rotation, by signs, by turns inside
   pairs of axes (sigma_min / sigma_max of M about 1e-2, 1e-6, 1e-10); equal scales and X_r = X_0 R_r + eps Gaussian, eps =
   1e-6, 1e-10, 1e-14.  Y and fit against mpmath, device against twin, orthogonality.
c. The floor band, g = 1e-6, 1e-7 (ratios about 1e-12, 1e-14: a column may or may not be replaced by the completion) at (17,
   16), (65, 15), (65, 4): fit against mpmath, orthogonality, finiteness, the same bits again and as set 1 of 3, device fit
   against twin fit.  Y is compared with nothing: either side may replace the borderline column, the contract allows both.
d. Bits: coordinates times 2^k give Y times 2^k and fit times 4^k, k = +-40 and +-300 (where only the scaling of M by a
   power of two keeps the Jacobi's squared norms in range), on a planted set, graded sets (g = 1e-5) and the four singular
   sets at (5, 4), (65, 15), (64, 2); the signs of the replicates' columns change no bit and those of X_0's
   columns D give Y D and the same fit, on planted and graded sets (g >= 1e-5: no column replaced) at (17, 7), (65, 16); a
   status-0 replicate and a status-0 matrix 0 among graded sets change no bit of the others.
e. The run form at K = 16: ngd_run_job_mds_align at n_ind = 33, 300 sites, 5 replicates by test_gpu_mds_align.check_run
   (real trailing eigenvalues lie close to one another), and the same bits under chunks of the MDS kernel that cut the set.

Every band case asserts by mpmath's sigma that each replicate's sigma_min / sigma_max lies within a decade of g^2 (clustered:
in [0.5, 1)); a case outside its band fails.

Bounds, all the project's tolerance in the header's own units: Y within 1e-9 max(|X_0|, |X_r|) of mpmath's, fit within 1e-9
(|X_r|^2 + |X_0|^2) of mpmath's |Y - X_0|^2, |Q Q^T - I| <= 1e-9 as far as Y shows Q (mds_align_expect.check_orth).  The
header promises Y only where sigma_min >= 1e-3 sigma_max; that the same bound is asked for down to 1e-10 rests on the host
twin, the same method, which stays more than five orders of magnitude inside it there (test_mds_align_cpu.py).  Device
against twin: one bound where both are pinned to one answer (a, b), two bounds and fit only where each is within one bound
of the exact fit and Y is not pinned (c).  Every comparison prints its largest figure in units of its bound.
The largest seen on an MI355X over the cases of this file: (a) Y 7.4e-15 of max |X| against numpy and 6.3e-16 against the
twin, fit 5.0e-16 of the squared norms against the formula and 1.5e-17 against the twin, orthogonality 1.5e-14; (b) graded Y
1.7e-15 against mpmath and 5.1e-16 against the twin, fit 2.3e-17 and 9.2e-18, orthogonality 8.5e-14; clustered Y 2.2e-15 and
1.8e-15, fit 9.6e-22 and 8.4e-22, orthogonality 1.1e-14; (c) fit 1.7e-12 of the squared norms against mpmath and 4.7e-18
against the twin, orthogonality 6.5e-16; (e) fit 3.9e-16, orthogonality 6.9e-15, the statistics differ from
boot_stats_host's by 0.

Against builds of mds_align.hip with one thing changed (one run of this file each): `tid % K` read as `tid % MAL_K` in the Q
step fails (a), (b), (c) and the three tests by bits; MAL_FLOOR at 1e-6 fails (b)'s graded sets, (c), the sign flips and
status 0; MAL_SWEEPS at 2 fails (a), (b) at K >= 7 (graded: K >= 15) and (e); without the scaling of M by a power of two only k = +-300 of the
scaling test fails -- at k = +-40 the unscaled sums are exact multiples too --; without the fabs in |g| > eps sqrt(ab)
everything but the scaling test fails."""
import numpy as np
import pytest

import mds_align_expect as A
from test_gpu_mds_align import N, against_twin, bits, check_run, cut_budgets, on_device, same_outputs, seen, singular_sets, synth

pytestmark = pytest.mark.gpu

CASES = [(5, 3), (17, 7), (17, 16), (65, 15), (65, 16)]
GRADES = [1e-1, 1e-3, 1e-5]
FLOOR = [1e-6, 1e-7]
NEAR = [1e-6, 1e-10, 1e-14]
SEED = 3


def engine(n):
    e = N().Engine(n, 16, kernel="mfma")
    e.synth_fill(1).commit()
    return e


def show(who, worst):
    print("device %s: largest figures in units of 1e-9: %s" % (who, {k: "%.3g" % x for k, x in worst.items()}))


def same(a, b):
    """two (aligned, fit) pairs, bit for bit"""
    return np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))


# ---- a. every K ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,Ks", [(17, list(range(1, 17))), (65, [3, 5, 7, 8, 9, 15, 16])])
def test_every_K_against_numpy_and_the_host_twin(n, Ks):
    failed = []
    with engine(n) as e:
        for K in Ks:
            eig, vec, Xs = seen(np.stack([A.planted(n, K, 3, seed=10 * s + K) for s in range(2)]))
            aligned, fit = on_device(e, Xs, K)
            assert aligned.shape == (2, 4, K, n) and fit.shape == (2, 4)
            try:  # (every K is shown before the test fails)
                worst = {}
                for s in range(2):
                    for k, x in A.check_set(Xs[s], aligned[s], fit[s]).items():
                        worst[k] = max(worst.get(k, 0.0), x)
                worst["twin y"], worst["twin fit"] = against_twin(Xs, aligned, fit, *N().mds_align_host(eig, vec))
                show("every K n=%d K=%d" % (n, K), worst)
                assert worst["twin y"] <= 1 and worst["twin fit"] <= 1, "twin: %s" % worst
            except AssertionError as err:
                failed.append("K=%d: %s" % (K, err))
    assert not failed, "; ".join(failed)


# ---- b. graded and clustered spectra ------------------------------------------------------------------------------------------
def check_against_mpmath_and_twin(e, Xp, K, band, who):
    eig, vec, Xs = seen(Xp[None])
    aligned, fit = on_device(e, Xs, K)
    worst = A.check_set_mp(Xs[0], aligned[0], fit[0], band)
    worst["twin y"], worst["twin fit"] = against_twin(Xs, aligned, fit, *N().mds_align_host(eig, vec))
    show("%s, sigma_min/sigma_max in [%.0e, %.0e)" % (who, band[0], band[1]), worst)
    assert worst["twin y"] <= 1 and worst["twin fit"] <= 1


@pytest.mark.parametrize("mode", A.MODES)
@pytest.mark.parametrize("n,K", CASES)
def test_graded_sets_against_mpmath_and_the_host_twin(n, K, mode):
    with engine(n) as e:
        for g in GRADES:
            check_against_mpmath_and_twin(e, A.graded(n, K, 3, g, SEED, mode), K, A.band_of(g),
                                          "graded %s n=%d K=%d g=%.0e" % (mode, n, K, g))


@pytest.mark.parametrize("n,K", CASES)
def test_clustered_sets_against_mpmath_and_the_host_twin(n, K):
    with engine(n) as e:
        for eps in NEAR:
            check_against_mpmath_and_twin(e, A.clustered(n, K, 3, eps, SEED), K, A.CLUSTERED_BAND,
                                          "clustered n=%d K=%d eps=%.0e" % (n, K, eps))


# ---- c. the floor band --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", A.MODES)
@pytest.mark.parametrize("n,K", [(17, 16), (65, 15), (65, 4)])
def test_floor_band_keeps_what_the_contract_pins(n, K, mode):
    with engine(n) as e:
        for g in FLOOR:
            eig, vec, Xs = seen(np.stack([A.planted(n, K, 3, seed=1), A.graded(n, K, 3, g, SEED, mode), A.planted(n, K, 3, seed=2)]))
            aligned, fit = on_device(e, Xs, K)
            band = A.band_of(g)
            worst = A.check_set_mp(Xs[1], aligned[1], fit[1], band, y=False)
            assert same((aligned, fit), on_device(e, Xs, K))
            alone = on_device(e, Xs[1:2], K)  # a set's bits do not depend on its neighbours
            assert same((aligned[1], fit[1]), (alone[0][0], alone[1][0]))
            hfit = N().mds_align_host(eig[1], vec[1])[1]
            norms = (Xs[1, 1:] ** 2).sum(axis=(1, 2)) + (Xs[1, 0] ** 2).sum()
            worst["twin fit"] = (np.abs(fit[1, 1:] - hfit[1:]) / (A.TOL * norms)).max()
            show("floor %s n=%d K=%d g=%.0e, sigma_min/sigma_max in [%.0e, %.0e)" % (mode, n, K, g, band[0], band[1]), worst)
            assert worst["twin fit"] <= 2


# ---- d. bits --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [40, -40, 300, -300])
@pytest.mark.parametrize("n,K", [(5, 4), (65, 15), (64, 2)])
def test_scaling_by_a_power_of_two_scales_the_result_exactly(n, K, k):
    """k = +-300: the squared norms of M's columns as the sums give them (4^+-600 of these) leave the range of a double;
    those of M scaled into [1, 2) do not"""
    sets = [A.planted(n, K, 3, seed=2)] + [A.graded(n, K, 3, 1e-5, SEED, mode) for mode in A.MODES] + list(singular_sets(n, K))
    _, _, Xs = seen(np.stack(sets))
    with engine(n) as e:
        aligned, fit = on_device(e, Xs, K)
        big = on_device(e, Xs * 2.0 ** k, K)
    for s in range(len(sets)):
        assert np.array_equal(bits(big[0][s]), bits(aligned[s] * 2.0 ** k)), "set %d: Y" % s
        assert np.array_equal(bits(big[1][s]), bits(fit[s] * 4.0 ** k)), "set %d: fit" % s


def regular_sets(n, K):
    """sets where no column is replaced: a planted one and the graded ones down to sigma_min / sigma_max = 1e-10"""
    return np.stack([A.planted(n, K, 3, seed=SEED)] + [A.graded(n, K, 3, g, SEED, mode) for mode in A.MODES for g in GRADES])


@pytest.mark.parametrize("n,K", [(17, 7), (65, 16)])
def test_sign_flips_change_no_bit_but_the_signs(n, K):
    """the signs of the replicates' columns do not matter at all; those of X_0's columns come out in Y as they went in"""
    _, _, Xs = seen(regular_sets(n, K))
    d = np.random.default_rng(400 + K).choice([-1.0, 1.0], size=K)
    d[0], d[-1] = -1.0, 1.0
    with engine(n) as e:
        aligned, fit = on_device(e, Xs, K)
        Xf = Xs.copy()
        Xf[:, 1:] *= d
        got = on_device(e, Xf, K)
        assert np.array_equal(bits(got[0][:, 1:]), bits(aligned[:, 1:])) and np.array_equal(bits(got[1]), bits(fit))
        Xf = Xs.copy()
        Xf[:, 0] *= d
        got = on_device(e, Xf, K)
        assert np.array_equal(bits(got[0]), bits(aligned * d[:, None])) and np.array_equal(bits(got[1]), bits(fit))


@pytest.mark.parametrize("n,K", [(17, 7), (65, 16)])
def test_status_0_among_graded_sets_changes_no_bit_of_the_others(n, K):
    _, _, Xs = seen(np.stack([A.graded(n, K, 3, 1e-5, SEED, mode) for mode in A.MODES]))
    status = np.ones((3, 4), dtype=np.uint32)
    status[0, 2] = status[1, 0] = 0
    with engine(n) as e:
        aligned, fit = on_device(e, Xs, K, status)
        plain = on_device(e, Xs, K)
    for s in range(3):
        A.check_set(Xs[s], aligned[s], fit[s], regular=False, status=status[s])
    keep = status.astype(bool) & status[:, :1].astype(bool)
    assert not keep.all() and np.array_equal(bits(aligned[keep]), bits(plain[0][keep])) and np.array_equal(bits(fit[keep]), bits(plain[1][keep]))


# ---- e. the run form at a large K ----------------------------------------------------------------------------------------------
def test_run_job_mds_align_at_K_16():
    n_ind, K, n_sites, n_rep, q, ci = 33, 16, 300, 5, 4, 0.9
    t = N().Taus(5)
    maps = np.stack([t.block_map(n_sites // q) for _ in range(n_rep)])
    with N().Engine(n_ind, n_sites, kernel="mfma") as e:
        e.upload_ind_major(synth(13, n_ind, n_sites)).commit()
        e.set_option("boot_partials", 0)  # (pins the plan: two calls of a job then agree bit for bit)
        out = e.run_job_mds_align(K, maps, q, ci=ci)
        assert np.all(out["status"] == 1) and int(out["used"]) == n_rep
        sib = e.run_job_mds(K, maps, q)
        check_run(e, {k: v if v is None else v[None] for k, v in out.items()}, tuple(a[None] for a in sib), K, ci, "run job n=33 K=16")
        for budget in cut_budgets(n_ind, K):
            e.set_option("mds_max_bytes", budget)
            same_outputs(out, e.run_job_mds_align(K, maps, q, ci=ci))
        e.set_option("mds_max_bytes", 0)
