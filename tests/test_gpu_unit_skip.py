"""The congruent one-image engine's layout and the plain pass that leaves the unit-sum coordinate out (NGD_OPT_UNIT_SKIP).

In the ONE image of a congruent engine (ngd_config.single_image = 2) twelve contraction indices are four whole sites, the
four t0 = p0 + p1 + p2 first, in a k-group of their own (ngsdist_amd/csrc/ngd_layout.h).  On the reference's matrices, without
--pairwise_del and on a data set ngd_commit found to be *unit*, the plain pass walks the other k-groups only and the
reduction adds d_0 (n + E_i + E_j).  Checked here: the shapes at which the period of four sites can go wrong, both arms
(unit_skip 1 / 0) against the oracle and against each other, called genotypes bit for bit with the two-image engine, every
other pass on the layout, the mark, the upload contract, a staged load, site shards, the fix-up pass and the engine's memory.

The bound between the two arms, 1e-13 relative, is derived: they differ by the rounding of O(n) terms of magnitude <= 1 --
~sqrt(n) 2^-53 ~ 6e-15 absolute at n = 3008 against sums of ~0.3 n, and the constant's correction is rounded once at the
result's magnitude (2^-53 relative).

The skipping pass delivers its sums only where none is below 1e-3 per site (its accumulators run to -n_slice / 2: 2^-53 of
that per rounding, too much for the tiny sums of nearly identical individuals); a data set with such a pair takes the full
pass from then on -- skip_expected() says which from the oracle's sums."""
import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

RTOL = 1e-9  # tests/test_gpu_parity.py
ARMS = 1e-13


def N():
    import ngsdist_amd
    return ngsdist_amd


def rel_err(a, b):
    a, b = np.asarray(a), np.asarray(b)
    den = np.where(b == 0, 1.0, np.abs(b))
    return float(np.max(np.abs(a - b) / den)) if a.size else 0.0


def n_kg(n_sites):
    return 3 * ((n_sites + 15) // 16 * 16) // 4


def skip_expected(so, n_sites):
    """the pass without the unit-sum coordinate is kept iff no pair's sum is below 1e-3 per site (NGD_FIX_MEAN_UNIT; the
    oracle's sums are within 1e-9 relative of the engine's, and none of these data sets has a sum that close to the bound)"""
    assert not np.any(np.abs(so / (1e-3 * n_sites) - 1) < 1e-6)
    return bool(np.all(so >= 1e-3 * n_sites))


def engine(p, unit_skip=1, **kw):
    n_ind, n_sites, _ = p.shape
    kw.setdefault("kernel", "mfma")
    e = N().Engine(n_ind, n_sites, **kw)
    e.set_option("unit_skip", unit_skip)
    e.upload_ind_major(p).commit()
    return e


def called(seed, n_ind, n_sites):
    g = np.random.default_rng(seed).integers(0, 3, size=(n_ind, n_sites))
    p = np.zeros((n_ind, n_sites, 3))
    np.put_along_axis(p, g[..., None], 1.0, axis=2)
    return p


# ---- shapes where the period of four sites can go wrong ------------------------------------------------------------
@pytest.mark.parametrize("n_sites", [1, 3, 4, 5, 3001, 3002, 3003, 3008])
@pytest.mark.parametrize("n_ind", [33, 130, 400, 600])
def test_plain_pass_both_arms_against_the_oracle(n_ind, n_sites):
    """single_image = 2 for the small engines; 400 and 600 individuals as the engine's own choice"""
    kw = {"single_image": 2} if n_ind < 400 else {}
    p = O.synth_indmajor(7 + n_ind + n_sites, n_ind, n_sites)
    for avg in (False, True):
        score = O.score_matrix(avg)
        so, co = O.all_pairs(p, score=score, n_threads=16)
        res = {}
        for arm in (1, 0):
            with engine(p, arm, score=score, **kw) as e:
                if n_ind >= 400:
                    assert e.image_mode() == (2, True)
                s, c = e.run()
                assert e.plain_pass_kgroups() == (n_kg(n_sites) * 2 // 3 if arm and skip_expected(so, n_sites) else n_kg(n_sites))
                s2, c2 = e.run()
                assert np.array_equal(s, s2) and np.array_equal(c, c2)  # run to run
            print("n_ind %d n_sites %d avg %d unit_skip %d: rel to the oracle %.3g" % (n_ind, n_sites, avg, arm, rel_err(s, so)))
            assert np.array_equal(c, co)
            assert rel_err(s, so) < RTOL, (avg, arm)
            res[arm] = (s, c)
        print("   the arms: rel %.3g" % rel_err(res[1][0], res[0][0]))
        assert rel_err(res[1][0], res[0][0]) < ARMS, avg
        assert np.array_equal(res[1][1], res[0][1])


# ---- called genotypes: every value dyadic, any order and the constant are exact ------------------------------------
@pytest.mark.parametrize("n_ind,n_sites", [(130, 3003), (600, 3001)])
def test_called_genotypes_bit_for_bit_with_the_two_image_engine(n_ind, n_sites):
    p = called(n_ind, n_ind, n_sites)
    out = []
    for single in (3, 2):
        with engine(p, 1, single_image=single) as e:
            r = [e.run()]
            if single == 2:
                assert e.plain_pass_kgroups() == n_kg(n_sites) * 2 // 3
            for B, partials in ((7, 0), (8, 2), (6, 2)):
                e.set_option("boot_partials", partials)
                r.append(e.run(N().Taus(B + n_ind).block_map(n_sites // B), B))
        out.append(r)
    for k, (two, one) in enumerate(zip(*out)):
        assert np.array_equal(two[0], one[0]) and np.array_equal(two[1], one[1]), k


# ---- the other passes on the new layout ----------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[(130, 2000), (600, 3000)], ids=["130x2000", "600x3000"])
def data(request):
    n_ind, n_sites = request.param
    p = O.synth_indmajor(31 + n_ind, n_ind, n_sites, miss_frac=0.1)
    return p


def boot_ref(p, m, B, pdel):
    n_sites = p.shape[1]
    return O.all_pairs(p, pairwise_del=pdel, site_src=O.boot_site_src(m, B), n_sites=len(m) * B, n_threads=16)


@pytest.mark.parametrize("pdel", [False, True])
def test_weighted_pass_and_partials_on_the_layout(data, pdel):
    p = data
    n_ind, n_sites, _ = p.shape
    kw = {"single_image": 2} if n_ind < 400 else {}
    with engine(p, 1, pairwise_del=pdel, **kw) as e:
        assert e.image_mode() == (2, True)
        for B, partials in ((7, 0), (8, 2), (6, 2), (10, 2)):
            m = N().Taus(B + n_ind).block_map(n_sites // B)
            e.set_option("boot_partials", partials)
            s, c = e.run(m, B)
            so, co = boot_ref(p, m, B, pdel)
            print("B %d partials %d pdel %d: rel %.3g" % (B, partials, pdel, rel_err(s, so)))
            assert np.array_equal(c, co) and rel_err(s, so) < RTOL, (B, partials)


@pytest.mark.parametrize("pdel", [False, True])
def test_job_whose_blocks_do_not_cover_the_last_sites(data, pdel):
    """the lead matrix is then the job's own plain pass: the bits of run(), the oracle's values"""
    p = data
    n_ind, n_sites, _ = p.shape
    kw = {"single_image": 2} if n_ind < 400 else {}
    B, n_blocks = 8, n_sites // 8 - 3
    t = N().Taus(5)
    maps = np.stack([t.block_map(n_blocks) for _ in range(3)])
    with engine(p, 1, pairwise_del=pdel, **kw) as e:
        S, Cn = e.run_job(maps, B)
        s, c = e.run()
        assert e.plain_pass_kgroups() == (n_kg(n_sites) if pdel else n_kg(n_sites) * 2 // 3)
    assert np.array_equal(S[0], s) and np.array_equal(Cn[0], c)
    so, co = O.all_pairs(p, pairwise_del=pdel, n_threads=16)
    assert np.array_equal(c, co) and rel_err(s, so) < RTOL
    for r in range(3):
        sb, cb = boot_ref(p, maps[r], B, pdel)
        assert np.array_equal(Cn[r + 1], cb) and rel_err(S[r + 1], sb) < RTOL, r


@pytest.mark.parametrize("size,step", [(10, 3), (64, 16)])
@pytest.mark.parametrize("pdel", [False, True])
def test_windows_on_the_layout(data, pdel, size, step):
    """(600 individuals, windows of 10 sites: every fifth window -- starts at every residue mod 4 -- so that the matrices stay
    within a few hundred MB)"""
    p = data
    n_ind, n_sites, _ = p.shape
    kw = {"single_image": 2} if n_ind < 400 else {}
    lo, hi = N().window_ranges(n_sites, size, step)
    if n_ind >= 400 and size == 10:
        lo, hi = lo[::5], hi[::5]
    with engine(p, 1, pairwise_del=pdel, **kw) as e:
        s, c = e.run_windows(lo, hi)
    worst = 0.0
    for w, (a, b) in enumerate(zip(lo, hi)):
        so, co = O.all_pairs(p, pairwise_del=pdel, site_src=np.arange(int(a), int(b)), n_threads=16)
        assert np.array_equal(c[w], co), w
        worst = max(worst, rel_err(s[w], so))
    print("windows %d / %d pdel %d: worst rel %.3g over %d windows" % (size, step, pdel, worst, len(lo)))
    assert worst < RTOL


# ---- the mark ------------------------------------------------------------------------------------------------------
def test_data_that_does_not_sum_to_one_takes_every_k_group():
    n_ind, n_sites = 130, 3001
    p = O.synth_indmajor(3, n_ind, n_sites)
    p[17, [0, 5, 1234, 3000]] *= 0.5
    so, co = O.all_pairs(p, n_threads=16)
    res = {}
    for arm in (1, 0):
        with engine(p, arm, single_image=2) as e:
            res[arm] = e.run()
            assert e.plain_pass_kgroups() == n_kg(n_sites)
    assert np.array_equal(res[1][0], res[0][0]) and np.array_equal(res[1][1], res[0][1])  # bit for bit
    assert np.array_equal(res[1][1], co) and rel_err(res[1][0], so) < RTOL
    # a value that is not finite clears the mark too (the sums are then NaN where the reference's are)
    q = O.synth_indmajor(3, n_ind, n_sites)
    q[3, 77, 1] = np.inf
    with engine(q, 1, single_image=2) as e:
        e.run()
        assert e.plain_pass_kgroups() == n_kg(n_sites)


def test_sites_uploaded_again_with_normalised_data_bring_the_skip_back():
    n_ind, n_sites = 130, 3001
    p = O.synth_indmajor(3, n_ind, n_sites)
    bad = p.copy()
    bad[17, 1230:1240] *= 0.5
    sm = lambda x, a, b: np.ascontiguousarray(x[:, a:b].transpose(1, 0, 2))
    with N().Engine(n_ind, n_sites, kernel="mfma", single_image=2) as e:
        e.upload_ind_major(bad)
        e.upload_sites(sm(p, 1229, 1241), 1229)
        s, c = e.commit().run()
        assert e.plain_pass_kgroups() == n_kg(n_sites) * 2 // 3
    with engine(p, 1, single_image=2) as e:
        s1, c1 = e.run()
    assert np.array_equal(s, s1) and np.array_equal(c, c1)


# ---- upload contract -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arm", [1, 0])
def test_pieces_off_the_period_in_reverse_order_and_one_sent_twice(arm):
    n_ind, n_sites = 130, 3003
    p = O.synth_indmajor(11, n_ind, n_sites)
    other = O.synth_indmajor(12, n_ind, n_sites)
    sm = lambda x, a, b: np.ascontiguousarray(x[:, a:b].transpose(1, 0, 2))
    cuts = [0, 1, 6, 1001, 1999, 2002, 3003]
    with N().Engine(n_ind, n_sites, kernel="mfma", single_image=2) as e:
        e.set_option("unit_skip", arm)
        e.upload_sites(sm(other, 1001, 1999), 1001)  # sent twice: other data first
        for a, b in reversed(list(zip(cuts[:-1], cuts[1:]))):
            e.upload_sites(sm(p, a, b), a)
        s, c = e.commit().run()
        m = N().Taus(2).block_map(n_sites // 6)
        e.set_option("boot_partials", 2)
        sb, cb = e.run(m, 6)
    with N().Engine(n_ind, n_sites, kernel="mfma", single_image=2) as e:
        e.set_option("unit_skip", arm)
        e.upload_sites(sm(p, 0, n_sites), 0)
        s1, c1 = e.commit().run()
        e.set_option("boot_partials", 2)
        sb1, cb1 = e.run(m, 6)
    assert np.array_equal(s, s1) and np.array_equal(c, c1)
    assert np.array_equal(sb, sb1) and np.array_equal(cb, cb1)


# ---- staged load ---------------------------------------------------------------------------------------------------
def test_staged_load_in_pieces_with_and_without_the_eager_pass():
    """raw likelihoods prepared on the device, in pieces of 1 000 and 1 001 sites: the bits of the same data loaded in one
    call, whether or not the plain pass started beside the load"""
    n_ind, n_sites = 600, 20_000
    raw = np.ascontiguousarray(O.synth_indmajor(41, n_ind, n_sites).transpose(1, 0, 2))
    with N().Engine(n_ind, n_sites, kernel="mfma") as e:
        assert e.image_mode() == (2, True)
        ref = e.upload_raw_sites(raw, 0).commit().run()
        assert e.plain_pass_kgroups() == n_kg(n_sites) * 2 // 3
    for piece in (1000, 1001):
        for eager in (0, 1):
            with N().Engine(n_ind, n_sites, kernel="mfma") as e:
                e.set_option("eager_full", eager)
                for a in range(0, n_sites, piece):
                    e.upload_raw_sites(raw[a:a + piece], a)
                s, c = e.commit().run()
                assert e.plain_pass_kgroups() == n_kg(n_sites) * 2 // 3
                s2, c2 = e.run()
            assert np.array_equal(s, ref[0]) and np.array_equal(c, ref[1]), (piece, eager)
            assert np.array_equal(s2, ref[0]) and np.array_equal(c2, ref[1]), (piece, eager)


# ---- site shards ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["synth", "upload"])
def test_two_site_shards_add_up_to_the_whole(how):
    n_ind, n_sites, cut = 130, 3003, 1504
    p = O.synth_indmajor(9, n_ind, n_sites)
    with N().Engine(n_ind, n_sites, kernel="mfma", single_image=2) as e:
        whole = e.synth_fill(9, 0.0).run() if how == "synth" else e.upload_ind_major(p).commit().run()
    tot_s, tot_c = np.zeros_like(whole[0]), np.zeros_like(whole[1])
    for lo, hi in ((0, cut), (cut, n_sites)):
        with N().Engine(n_ind, hi - lo, kernel="mfma", single_image=2) as e:
            s, c = e.synth_fill(9, 0.0, site0=lo).run() if how == "synth" else e.upload_ind_major(p[:, lo:hi]).commit().run()
            assert e.plain_pass_kgroups() == n_kg(hi - lo) * 2 // 3
        tot_s += s
        tot_c += c
    assert np.array_equal(tot_c, whole[1])
    assert rel_err(tot_s, whole[0]) < ARMS
    so, co = O.all_pairs(p, n_threads=16)
    assert np.array_equal(whole[1], co) and rel_err(whole[0], so) < RTOL


# ---- fix-up --------------------------------------------------------------------------------------------------------
def clones(n_ind, n_sites, eps, seed=5):
    """copies of one individual whose likelihoods are confident to `eps` (tests/test_gpu_parity.py clones())"""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 3, size=n_sites)
    p = eps * (1 + rng.random((n_ind, n_sites, 3)))
    p[:, np.arange(n_sites), g] = 0
    p[:, np.arange(n_sites), g] = 1 - p.sum(axis=2)
    return p


@pytest.mark.parametrize("eps", [1e-9, 1e-13])
def test_clones_are_noted_on_the_finished_value_and_the_pass_runs_whole(eps):
    n_ind, n_sites = 100, 3001
    p = clones(n_ind, n_sites, eps)
    so, co = O.all_pairs(p, n_threads=16)
    with engine(p, 1, single_image=2) as e:
        s, c = e.run()
        f = e.fixup()
        assert e.plain_pass_kgroups() == n_kg(n_sites)  # the pass without the coordinate noted pairs: run whole, and stays so
        s2, c2 = e.run()
        assert np.array_equal(s, s2) and e.plain_pass_kgroups() == n_kg(n_sites)
    with engine(p, 0, single_image=2) as e:
        s0, c0 = e.run()
    assert np.array_equal(s, s0) and np.array_equal(c, c0)  # the bits of the engine that never skips
    assert f["flagged"] == f["recomputed"] == n_ind * (n_ind - 1) // 2 and f["skipped"] == 0
    assert np.array_equal(c, co) and rel_err(s, so) < RTOL


def test_clones_recomputed_by_one_more_pass():
    """so many noted pairs that the engine takes the whole matrix once more in the two-image arithmetic (the shape at which
    tests/test_gpu_parity.py test_congruent_single_image_fixup_by_one_more_pass has it choose that route)"""
    n_ind, n_sites = 500, 20_000
    p = clones(n_ind, n_sites, 1e-9)
    so, co = O.all_pairs(p, n_threads=16)
    with engine(p, 1) as e:
        assert e.image_mode() == (2, True)
        s, c = e.run()
        f = e.fixup()
        assert e.plain_pass_kgroups() == n_kg(n_sites)
    assert f["by_pass"] == 1 and f["flagged"] == f["recomputed"] == n_ind * (n_ind - 1) // 2
    assert np.array_equal(c, co) and rel_err(s, so) < RTOL


# ---- memory --------------------------------------------------------------------------------------------------------
PARENT_BYTES_600x3000 = 117724304  # ngd_device_bytes() of this engine with the library of the commit before this one


def test_device_bytes_grow_by_the_list_and_the_corrections_alone():
    """ngd_device_bytes() of a 600 x 3000 engine of the engine's own choice: the figure of the commit before this one
    (PARENT_BYTES_600x3000, measured with that commit's library on an MI355X) plus the new state exactly -- one int64 per
    individual and one for the scan's flag, and the list of 2/3 of the k-groups with its 16 entries of padding."""
    n_ind, n_sites = 600, 3000
    with N().Engine(n_ind, n_sites, kernel="mfma") as e:
        assert e.image_mode() == (2, True)
        got = e.device_bytes()
    new_state = 8 * (n_ind + 1) + 4 * (n_kg(n_sites) * 2 // 3 + 16)
    print("device_bytes %d, parent %s, new state %d" % (got, PARENT_BYTES_600x3000, new_state))
    assert got == PARENT_BYTES_600x3000 + new_state
