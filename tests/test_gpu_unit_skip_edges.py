"""The plain pass that leaves the unit-sum coordinate out (NGD_OPT_UNIT_SKIP), where it could be wrong with
tests/test_gpu_unit_skip.py green: the correction d_0 2^-53 (E_i + E_j) at a magnitude an assertion can see, the unit mark at
|t0 - 1| = 2^-40 and one ulp past it, the 1e-3-per-site rule at its edge, the same edge with slices of 32 768 sites, and a
staged load whose eager slices are of the other kind of pass or belong to a rejected load.

A. Normalised data has t0 = fl(p0 + p1 + p2) within 3 ulp of 1: the correction is ~1e-16 of a sum, a thousand times below
   ARMS, and k_unit_scan (layout.hip) or the E_i + E_j of k_reduce (reduce.hip) could do anything.  perturbed() scales every
   individual by (1 + f_i), |f_i| in [0.3, 0.9] 2^-40: the set is still *unit*, |E_i| reaches 2e7 units of 2^-53, and a cluster
   of ten nearly identical individuals (sums of 2e-2 per site) makes the correction 2e-11 of its pairs' sums.  sensitivity()
   states, from the oracle's sums, d_0 and E summed on the host, what a dropped correction would move: the tests fail their own
   set-up if that is not far above the bound they then hold between the arms.
B. Values whose t0 is exact in any order of addition, at the bound (the mark stays) and one ulp past it (the pass runs whole,
   the bits of the engine that never skips), at the corners the scan's guards decide.
C, D. Clone pairs of 4 eps per site around NGD_FIX_MEAN_UNIT = 1e-3.
E. The eager pass beside a staged load (NGD_OPT_EAGER_FULL) with the option changed before run() or in the middle of the load.

The bound between the arms, ARMS, is tests/test_gpu_unit_skip.py's: rounding of O(n) terms of magnitude <= 1, ~7e-13
absolute at 3000 sites, against sums of ~0.3 n -- and of 2e-2 n = 60 in the cluster, 1.2e-14."""
import numpy as np
import pytest

from oracle import oracle as O
from test_gpu_parity import _raw_gl
from test_gpu_upload_contract import nan_then_clean, stage

pytestmark = pytest.mark.gpu

RTOL = 1e-9  # tests/test_gpu_parity.py
ARMS = 1e-13  # tests/test_gpu_unit_skip.py
PAIR_TOL = 1e-10  # ngd_internal.h at NGD_FIX_MEAN_UNIT: the skipping pass's worst case for a pair just above the rule


def N():
    import ngsdist_amd
    return ngsdist_amd


def rel_err(a, b):
    a, b = np.asarray(a), np.asarray(b)
    den = np.where(b == 0, 1.0, np.abs(b))
    return float(np.max(np.abs(a - b) / den)) if a.size else 0.0


def n_kg(n_sites):
    return 3 * ((n_sites + 15) // 16 * 16) // 4


def pair_index(n_ind, i, j):
    assert i < j
    return i * n_ind - i * (i + 1) // 2 + j - i - 1


def same(a, b, tag=""):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), ("not the same bits", tag)


def clones(n_ind, n_sites, eps, seed=5, hom_only=False):
    """copies of one individual whose likelihoods are confident to `eps` (tests/test_gpu_parity.py clones()); hom_only: no
    heterozygous sites (under --avg_nuc_dist two copies of a heterozygote are half a difference apart)"""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 2, size=n_sites) * 2 if hom_only else rng.integers(0, 3, size=n_sites)
    p = eps * (1 + rng.random((n_ind, n_sites, 3)))
    p[:, np.arange(n_sites), g] = 0
    p[:, np.arange(n_sites), g] = 1 - p.sum(axis=2)
    return p


def engine(p, unit_skip=1, **kw):
    n_ind, n_sites, _ = p.shape
    kw.setdefault("kernel", "mfma")
    if n_ind < 400:
        kw.setdefault("single_image", 2)
    e = N().Engine(n_ind, n_sites, **kw)
    if n_ind >= 400:
        assert e.image_mode() == (2, True)  # the engine's own choice
    e.set_option("unit_skip", unit_skip)
    e.upload_ind_major(p).commit()
    return e


def site_major(x, a, b):
    return np.ascontiguousarray(x[:, a:b].transpose(1, 0, 2))


# ---- A. unit sums off by up to 2^-40 -----------------------------------------------------------------------------------
def cluster_rows(n_ind):
    """ten rows: 100..109 of 130; the last ten of 600 (second 128-tile onwards, into the last partial group of 16)"""
    c0 = 100 if n_ind == 130 else n_ind - 12 if n_ind < 130 else n_ind - 10
    return c0, c0 + 10


def perturbed(n_ind, n_sites, seed=21, hom_only=False):
    """ordinary individuals and a cluster of ten clones (eps = 5e-3: pair sums of 1.97e-2 per site), every individual scaled by
    (1 + f_i), |f_i| in [0.3, 0.9] 2^-40, negative for i % 3 == 0 -- but one sign in the whole cluster, so that E_i + E_j
    does not cancel there"""
    p = O.synth_indmajor(seed, n_ind, n_sites)
    c0, c1 = cluster_rows(n_ind)
    p[c0:c1] = clones(10, n_sites, 5e-3, hom_only=hom_only)
    f = np.random.default_rng(seed + 1).uniform(0.3, 0.9, n_ind) * 2.0 ** -40
    f[np.arange(n_ind) % 3 == 0] *= -1
    f[c0:c1] = np.abs(f[c0:c1]) * np.sign(f[c0])
    return p * (1 + f)[:, None, None]


def unit_E(p):
    """E_i = SUM_s (t0_i(s) - 1) in units of 2^-53, as int64; t0 = fl(fl(p0 + p1) + p2) is the image's (layout.hip: the first
    row of the congruence is (1, 1, 1), asserted in sensitivity()); fails unless the data set is *unit*"""
    d = ((p[..., 0] + p[..., 1]) + p[..., 2]) - 1.0
    assert np.all(np.abs(d) <= 2.0 ** -40)
    e = d * 2.0 ** 53
    assert np.all(e == np.rint(e))
    return e.astype(np.int64).sum(axis=1)


def dropped_correction(p, so, score, E=None):
    """|d_0 2^-53 (E_i + E_j)| relative to the oracle's sum, per pair: what an engine that lost the correction would be off by"""
    c, d = N().score_congruence(score)
    assert np.array_equal(c[0], [1.0, 1.0, 1.0])
    E = unit_E(p) if E is None else E
    i, j = np.triu_indices(p.shape[0], 1)
    return np.abs(d[0] * (E[i] + E[j]).astype(np.float64) * 2.0 ** -53) / np.abs(so)


def sensitivity(p, so, score):
    """the precondition: a dropped correction exceeds 20 ARMS for every pair inside the cluster and 3 ARMS for at least half
    of all pairs"""
    n_ind = p.shape[0]
    rel = dropped_correction(p, so, score)
    c0, c1 = cluster_rows(n_ind)
    i, j = np.triu_indices(n_ind, 1)
    inside = (i >= c0) & (i < c1) & (j >= c0) & (j < c1)
    assert inside.sum() == 45
    print("   a dropped correction: cluster %.3g .. %.3g, median of all pairs %.3g, above 3 ARMS %.3f of them"
          % (rel[inside].min(), rel[inside].max(), np.median(rel), np.mean(rel > 3 * ARMS)))
    assert rel[inside].min() > 20 * ARMS
    assert np.mean(rel > 3 * ARMS) >= 0.5
    return inside


def kept(so, n_sites):
    """the skip is kept iff no pair's sum is below 1e-3 per site; no data set of group A comes near"""
    return bool(np.all(so > 2e-3 * n_sites))


def both_arms(p, score, so, co):
    """arm 1 and arm 0 on p: each against the oracle, the k-groups visited, run to run; -> their results"""
    n_ind, n_sites, _ = p.shape
    assert kept(so, n_sites)
    res = {}
    for arm in (1, 0):
        with engine(p, arm, score=score) as e:
            s, c = e.run()
            assert e.plain_pass_kgroups() == (n_kg(n_sites) * 2 // 3 if arm else n_kg(n_sites))
            same(e.run(), (s, c), "run to run")
        print("   unit_skip %d: rel to the oracle %.3g" % (arm, rel_err(s, so)))
        assert np.array_equal(c, co)
        assert rel_err(s, so) < RTOL, arm
        res[arm] = (s, c)
    return res


@pytest.mark.parametrize("avg", [False, True], ids=["default", "avg_nuc_dist"])
@pytest.mark.parametrize("n_ind,n_sites", [(130, 3001), (33, 3), (130, 3003), (600, 3001)])
def test_visible_correction_both_arms_against_the_oracle_and_each_other(n_ind, n_sites, avg):
    """33 x 3: a single period with one site missing from it; 600: the engine's own choice, the cluster in rows 590..599"""
    score = O.score_matrix(avg)
    p = perturbed(n_ind, n_sites, hom_only=avg)
    so, co = O.all_pairs(p, score=score, n_threads=16)
    inside = sensitivity(p, so, score)
    res = both_arms(p, score, so, co)
    d = np.abs(res[1][0] - res[0][0]) / np.abs(res[0][0])
    print("   the arms: rel %.3g (inside the cluster %.3g)" % (d.max(), d[inside].max()))
    assert d.max() < ARMS
    assert np.array_equal(res[1][1], res[0][1])


def test_visible_correction_two_site_shards_add_up_to_the_whole():
    """each shard's E is its own sites': with none, or with the whole set's in both, the total would be off by a correction's
    worth, or two"""
    n_ind, n_sites, cut = 130, 3003, 1504
    score = O.score_matrix(False)
    p = perturbed(n_ind, n_sites)
    so, co = O.all_pairs(p, n_threads=16)
    sensitivity(p, so, score)
    with engine(p, 1) as e:
        whole = e.run()
        assert e.plain_pass_kgroups() == n_kg(n_sites) * 2 // 3
    with engine(p, 0) as e:
        whole0 = e.run()
    tot_s, tot_c = np.zeros_like(whole[0]), np.zeros_like(whole[1])
    for lo, hi in ((0, cut), (cut, n_sites)):
        with engine(p[:, lo:hi], 1) as e:
            s, c = e.run()
            assert e.plain_pass_kgroups() == n_kg(hi - lo) * 2 // 3
        tot_s += s
        tot_c += c
    print("   shards against the whole: rel %.3g, against the whole with unit_skip 0: %.3g"
          % (rel_err(tot_s, whole[0]), rel_err(tot_s, whole0[0])))
    assert np.array_equal(tot_c, whole[1]) and np.array_equal(tot_c, co)
    assert rel_err(tot_s, whole[0]) < ARMS
    assert rel_err(tot_s, whole0[0]) < ARMS  # (the engine that never skips: shards that all lost their E would still add up)
    assert rel_err(whole[0], so) < RTOL


def test_visible_correction_does_not_depend_on_the_upload_order():
    """the pieces of tests/test_gpu_unit_skip.py's cuts in reverse, after a piece of another perturbed data set was sent
    first: the bits of a one-call upload -- the integer sum is order-free and is the committed data's alone"""
    n_ind, n_sites = 130, 3003
    p = perturbed(n_ind, n_sites)
    other = perturbed(n_ind, n_sites, seed=33)
    assert np.all(unit_E(other[:, 1001:1999]) != unit_E(p[:, 1001:1999]))  # (a piece's worth that must not survive)
    cuts = [0, 1, 6, 1001, 1999, 2002, 3003]
    with N().Engine(n_ind, n_sites, kernel="mfma", single_image=2) as e:
        e.upload_sites(site_major(other, 1001, 1999), 1001)
        for a, b in reversed(list(zip(cuts[:-1], cuts[1:]))):
            e.upload_sites(site_major(p, a, b), a)
        got = e.commit().run()
        assert e.plain_pass_kgroups() == n_kg(n_sites) * 2 // 3
    with N().Engine(n_ind, n_sites, kernel="mfma", single_image=2) as e:
        want = e.upload_sites(site_major(p, 0, n_sites), 0).commit().run()
        assert e.plain_pass_kgroups() == n_kg(n_sites) * 2 // 3
    same(got, want)


def test_visible_correction_after_a_load_rejected_for_nan():
    """ngd_upload_sites takes prepared values and checks nothing (a NaN there clears the mark and the sums are NaN where the
    reference's are): NGD_E_NAN comes from the raw path.  So: a raw load with a NaN, commit() raises -6, then the perturbed
    data through upload_sites on the same engine -- the bits of a fresh engine's, with the skip: E, the mark and the NaN
    flag are the second load's alone"""
    n_ind, n_sites = 130, 3003
    p = perturbed(n_ind, n_sites)
    bad, _ = nan_then_clean(n_ind, n_sites)
    with engine(p, 1) as e:
        want = e.run()
        assert e.plain_pass_kgroups() == n_kg(n_sites) * 2 // 3
    with N().Engine(n_ind, n_sites, kernel="mfma", single_image=2) as e:
        e.upload_raw_sites(bad, 0)
        with pytest.raises(N().NgdError) as ei:
            e.commit()
        assert ei.value.code == -6
        got = e.upload_sites(site_major(p, 0, n_sites), 0).commit().run()
        assert e.plain_pass_kgroups() == n_kg(n_sites) * 2 // 3
        same(e.run(), got, "run to run")
    same(got, want)


EAGER_N_IND, EAGER_N_SITES = 392, 11_000  # tests/test_gpu_upload_contract.py's eager shape: n_slices = 64, 1-MiB pieces


def eager_engine(**opt):
    e = N().Engine(EAGER_N_IND, EAGER_N_SITES, kernel="mfma", n_slices=64, single_image=2)
    for k, v in opt.items():
        e.set_option(k, v)
    return e


@pytest.mark.parametrize("eager", [0, 1])
def test_fresh_staged_load_after_nan_on_the_congruent_image(eager):
    """tests/test_gpu_upload_contract.py test_fresh_staged_load_after_nan on ONE image in congruent coordinates: the rejected
    load's eager slices are slices of the list, and nothing of them, of its E or of its mark is kept (a staged load
    normalises: E itself is not visible here)"""
    n_ind, n_sites = EAGER_N_IND, EAGER_N_SITES
    bad, clean = nan_then_clean(n_ind, n_sites)
    with eager_engine() as e:
        want = e.upload_raw_sites(clean, 0).commit().run()
        assert e.plain_pass_kgroups() == n_kg(n_sites) * 2 // 3
    with eager_engine(stage_piece_mib=1, eager_full=eager) as e:
        stage(e, bad, 0)
        with pytest.raises(N().NgdError) as ei:
            e.commit()
        assert ei.value.code == -6
        stage(e, clean, 0)
        got = e.commit().run()
        assert e.plain_pass_kgroups() == n_kg(n_sites) * 2 // 3
        same(e.run(), got, "run to run")
    same(got, want, eager)
    so, co = O.all_pairs(O.prep_binary(clean, n_ind, n_sites), n_threads=16)
    assert np.array_equal(got[1], co) and rel_err(got[0], so) < RTOL


# ---- B. the mark at its bound -------------------------------------------------------------------------------------------
# (p0, p1, p2) whose t0 = (0.5 + 0.25) + p2 is exact in any order of addition; whether the data set stays *unit*
MARK = {"at+": (0.25 + 2.0 ** -40, 1 + 2.0 ** -40, True),
        "at-": (0.25 - 2.0 ** -40, 1 - 2.0 ** -40, True),
        "past+": (0.25 + 2.0 ** -40 + 2.0 ** -52, 1 + 2.0 ** -40 + 2.0 ** -52, False),
        "past-": (0.25 - 2.0 ** -40 - 2.0 ** -53, 1 - 2.0 ** -40 - 2.0 ** -53, False)}
_MARK_REF = {}


def mark_data(n_ind, n_sites):
    """ordinary data, made once per shape and left unchanged: a test copies it and sets its one (individual, site)"""
    if (n_ind, n_sites) not in _MARK_REF:
        _MARK_REF[(n_ind, n_sites)] = O.synth_indmajor(3 + n_ind + n_sites, n_ind, n_sites)
    return _MARK_REF[(n_ind, n_sites)]


@pytest.mark.parametrize("n_ind,n_sites,ind,site,which", [
    (33, 3001, 0, 0, "at+"),            # individual 0, site 0
    (130, 3001, 0, 0, "past-"),
    (33, 3001, 32, 3000, "past+"),      # the last individual of a partial group of 16, the last site, n_sites % 4 = 1
    (130, 3001, 129, 3000, "at-"),
    (130, 3002, 129, 3001, "past-"),    # n_sites % 4 = 2
    (130, 3002, 0, 3001, "at+"),
    (130, 3003, 129, 3002, "past+"),    # n_sites % 4 = 3
    (33, 3003, 32, 3002, "at-"),
    (130, 3008, 129, 3007, "past-"),    # n_sites % 4 = 0
    (33, 3008, 32, 3007, "at+"),
    (130, 3001, 129, 0, "past+"),       # the last individual at site 0
    (130, 3001, 64, 256, "past-"),      # the first site of the scan's second grid.y share (64 periods of four sites each)
    (33, 3001, 32, 1029, "past+"),      # ... and one inside a later share, at residue 1 of its period
    (130, 3003, 77, 2999, "at-"),
])
def test_mark_at_the_bound_and_one_ulp_past_it(n_ind, n_sites, ind, site, which):
    third, t0, unit = MARK[which]
    p = mark_data(n_ind, n_sites).copy()
    p[ind, site] = (0.5, 0.25, third)
    assert (p[ind, site, 0] + p[ind, site, 1]) + p[ind, site, 2] == t0 == (p[ind, site, 2] + p[ind, site, 1]) + p[ind, site, 0]
    assert (abs(t0 - 1) <= 2.0 ** -40) == unit and abs(abs(t0 - 1) - 2.0 ** -40) <= 2.0 ** -52
    so, co = O.all_pairs(p, n_threads=16)
    res = {}
    for arm in (1, 0):
        with engine(p, arm) as e:
            res[arm] = e.run()
            assert e.plain_pass_kgroups() == (n_kg(n_sites) * 2 // 3 if arm and unit else n_kg(n_sites)), (arm, which)
        assert np.array_equal(res[arm][1], co) and rel_err(res[arm][0], so) < RTOL, arm
    if unit:
        assert rel_err(res[1][0], res[0][0]) < ARMS and np.array_equal(res[1][1], res[0][1])
    else:
        same(res[1], res[0], "past the bound: the bits of the engine that never skips")


# ---- C. the 1e-3-per-site rule at its edge --------------------------------------------------------------------------------
def with_clone_pair(n_ind, n_sites, rows, eps, seed=3):
    p = O.synth_indmajor(seed, n_ind, n_sites)
    p[list(rows)] = clones(2, n_sites, eps)
    return p


@pytest.mark.parametrize("n_ind,rows", [(130, (77, 129)), (601, (5, 600))], ids=["130", "601-straddling-tiles"])
def test_one_pair_below_the_rule_among_ordinary_individuals_drops_the_skip(n_ind, rows):
    """eps = 2e-4: 8e-4 per site, below NGD_FIX_MEAN_UNIT and far above NGD_FIX_MEAN.  The skipping pass notes the one pair;
    the rerun notes nothing, and its bits are the never-skipping engine's"""
    n_sites = 3001
    p = with_clone_pair(n_ind, n_sites, rows, 2e-4)
    so, co = O.all_pairs(p, n_threads=16)
    k = pair_index(n_ind, *rows)
    assert 7.9e-4 * n_sites < so[k] < 8.1e-4 * n_sites and np.all(np.delete(so, k) > 0.1 * n_sites)
    with engine(p, 1) as e:
        got = e.run()
        assert e.plain_pass_kgroups() == n_kg(n_sites)
        assert e.fixup()["flagged"] == 0
        same(e.run(), got, "run to run")
        assert e.plain_pass_kgroups() == n_kg(n_sites)
    with engine(p, 0) as e:
        want = e.run()
    same(got, want)
    assert np.array_equal(got[1], co) and rel_err(got[0], so) < RTOL


@pytest.mark.parametrize("n_ind,rows", [(130, (77, 129)), (601, (5, 600))], ids=["130", "601-straddling-tiles"])
def test_one_pair_just_above_the_rule_keeps_the_skip(n_ind, rows):
    """eps = 3e-4: 1.2e-3 per site, where the skipping pass is at its least accurate and still delivers; ngd_internal.h states
    1e-10 relative as its worst case for such a pair (slices of 4000 sites; these are far shorter)"""
    n_sites = 3001
    p = with_clone_pair(n_ind, n_sites, rows, 3e-4)
    so, co = O.all_pairs(p, n_threads=16)
    k = pair_index(n_ind, *rows)
    assert 1.19e-3 * n_sites < so[k] < 1.2e-3 * n_sites and np.all(np.delete(so, k) > 0.1 * n_sites)
    res = {}
    for arm in (1, 0):
        with engine(p, arm) as e:
            res[arm] = e.run()
            assert e.plain_pass_kgroups() == (n_kg(n_sites) * 2 // 3 if arm else n_kg(n_sites))
        assert np.array_equal(res[arm][1], co) and rel_err(res[arm][0], so) < RTOL, arm
    s1, s0 = res[1][0], res[0][0]
    print("   %d x %d, clone pair %s at %.4g per site: unit_skip 1 rel to the oracle %.3g, to unit_skip 0 %.3g; unit_skip 0 to the "
          "oracle %.3g" % (n_ind, n_sites, rows, so[k] / n_sites, abs(s1[k] - so[k]) / so[k], abs(s1[k] - s0[k]) / s0[k],
                           abs(s0[k] - so[k]) / so[k]))
    assert abs(s1[k] - s0[k]) / s0[k] <= PAIR_TOL
    assert rel_err(np.delete(s1, k), np.delete(s0, k)) < ARMS


# ---- D. the same edge with long slices --------------------------------------------------------------------------------------
def test_pairs_just_above_the_rule_with_slices_of_32768_sites():
    """40 x 262 144 in eight slices: 32 768 sites each, eight times the length ngd_internal.h's worst case is written for
    and the accumulators run to -16 384.  Clone pairs at 1.2e-3, 2e-3 and 2e-2 per site: the skip is kept, every sum is the
    oracle's to RTOL and the three pairs' to the 1e-10 the header states.  [measured] 1.6e-13, 3.5e-13, 6.8e-14 -- and 2e-12 for
    the first with slices of 262 144 sites, longer than any the engine plans: profiles/unit_skip/threshold_edges.txt"""
    n_ind, n_sites = 40, 262_144
    p = O.synth_indmajor(17, n_ind, n_sites)
    pairs = {(0, 1): 3e-4, (2, 39): 5e-4, (20, 21): 5e-3}
    for r, (rows, eps) in enumerate(pairs.items()):
        p[list(rows)] = clones(2, n_sites, eps, seed=50 + r)
    so, co = O.all_pairs(p, n_threads=16)
    res = {}
    for arm in (1, 0):
        with engine(p, arm, n_slices=8) as e:
            res[arm] = e.run()
            assert e.plain_pass_kgroups() == (n_kg(n_sites) * 2 // 3 if arm else n_kg(n_sites))
        print("   unit_skip %d: rel to the oracle %.3g" % (arm, rel_err(res[arm][0], so)))
        assert np.array_equal(res[arm][1], co) and rel_err(res[arm][0], so) < RTOL, arm
    s1, s0 = res[1][0], res[0][0]
    for rows, eps in pairs.items():
        k = pair_index(n_ind, *rows)
        assert 3.9 * eps * n_sites < so[k] < 4 * eps * n_sites
        print("   40 x 262144, 8 slices of 32768 sites, clone pair %s at %.4g per site: unit_skip 1 rel to the oracle %.3g, to "
              "unit_skip 0 %.3g; unit_skip 0 to the oracle %.3g" % (rows, so[k] / n_sites, abs(s1[k] - so[k]) / so[k],
                                                                    abs(s1[k] - s0[k]) / s0[k], abs(s0[k] - so[k]) / so[k]))
        assert abs(s1[k] - so[k]) / so[k] <= PAIR_TOL, rows


# ---- E. eager slices of the wrong kind --------------------------------------------------------------------------------------
_EAGER_REF = {}


def eager_ref(arm):
    """(the raw data, the results of an engine that had unit_skip = arm throughout and loaded in one call)"""
    if "raw" not in _EAGER_REF:
        _EAGER_REF["raw"] = _raw_gl(EAGER_N_IND, EAGER_N_SITES, 81)
    if arm not in _EAGER_REF:
        with eager_engine(unit_skip=arm) as e:
            _EAGER_REF[arm] = e.upload_raw_sites(_EAGER_REF["raw"], 0).commit().run()
            assert e.plain_pass_kgroups() == (n_kg(EAGER_N_SITES) * 2 // 3 if arm else n_kg(EAGER_N_SITES))
    return _EAGER_REF["raw"], _EAGER_REF[arm]


@pytest.mark.parametrize("load,flip_at,final", [(1, None, 0), (0, None, 1), (1, 50, 0), (0, 50, 1), (1, 5, 0), (0, 5, 1)])
def test_eager_slices_of_the_other_kind_of_pass_are_dropped(load, flip_at, final):
    """392 x 11 000, 64 slices, pieces of 111 sites staged in ascending order with NGD_OPT_EAGER_FULL.  The image has 8256
    k-groups, 5504 of them on the list: slices of 132 k-groups, or of 88 list entries.  eager_advance launches whole eights of
    slices once they and the NGD_KG_TAIL = 8 groups behind them are below the prefix: the list's 2 (prefix / 4) >= 8 x 88 + 8
    entries, or 3 (prefix / 4) >= 8 x 132 + 8 k-groups -- a prefix of 1424, or 1420, sites: either kind may start after the
    13th piece (prefix 1443), the next eight after the 26th.  Whether they started cannot be observed and is not asserted.

    unit_skip = `load` while the pieces go in, changed to `final` before run() (flip_at None) or before piece flip_at -- before
    any slice can have started (5), or after dozens may have (50): one kind of slices per load, and run() drops those of
    the other kind.  The pass run() makes is `final`'s, and its bits those of a one-call engine that never had another value."""
    n_ind, n_sites = EAGER_N_IND, EAGER_N_SITES
    raw, want = eager_ref(final)
    cap = (1 << 20) // (n_ind * 24)
    with eager_engine(stage_piece_mib=1, eager_full=1) as e:
        if not load:  # (1 is the option's default: left untouched)
            e.set_option("unit_skip", 0)
        for k, a in enumerate(range(0, n_sites, cap)):
            if k == flip_at:
                e.set_option("unit_skip", final)
            stage(e, raw[a:a + cap], a)
        e.commit()
        e.set_option("unit_skip", final)
        got = e.run()
        assert e.plain_pass_kgroups() == (n_kg(n_sites) * 2 // 3 if final else n_kg(n_sites))
        same(e.run(), got, "run to run")
    same(got, want)
