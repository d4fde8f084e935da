"""Every launch arm of the spilled-terms contraction (contract_mfma.hip) against a reference of its own.

ngd_launch_contract picks k_contract_mfma<RT, PT> from the number of matrices of the job: RT = groups of 16 matrices in a
launch (1 to 8), PT = 4 slot groups per wavefront up to RT = 4 and 2 above, launches in batches of 8 groups (a remainder
launch starts at matrix group 8, 16, ...).  The sweeps below reach every RT as a first launch, both PT, remainder
launches of RT = 1, 2 and 5, three launches, and every padding of the slot groups -- and hold EVERY matrix of every job
to tests/site_terms.py: the per-site terms of the oracle combined with the job's weights in extended precision (the sums
of the EM path are linear in them), counts from the same weights in integers.  Each case reads the plan it ran from the
engine's own report (ngd_last_spill_timing), so none can pass by taking another plan; no cell is excluded.

Tolerances are the project's: 1e-9 against the oracle, 1e-12 between the spilled-terms plan and the engine's own
em_spill = 0 passes (include/ngsdist_amd.h), counts exact."""
import functools

import numpy as np
import pytest

import site_terms as ST
from oracle import oracle as O

pytestmark = pytest.mark.gpu

RTOL = 1e-9        # against the oracle
RTOL_SELF = 1e-12  # the spilled-terms plan against the engine's own passes (include/ngsdist_amd.h)
SEED = 77


def N():
    import ngsdist_amd
    return ngsdist_amd


def rel_err(a, b):
    a, b = np.asarray(a), np.asarray(b)
    den = np.where(b == 0, 1.0, np.abs(b))
    return float(np.max(np.abs(a - b) / den)) if a.size else 0.0


def spill_unit(block_size):
    """q: the block size or its largest divisor up to 64 (the sites of a unit leave the EM kernel as one term)"""
    return max(d for d in range(1, min(64, block_size) + 1) if block_size % d == 0)


def live_slot_groups(n_ind):
    """groups of 16 pair slots that hold a pair: per row of a 64 x 64 tile, one per group of 16 columns with a column
    above the diagonal and below n_ind (the spilled-terms plan)"""
    n, nt = 0, (n_ind + 63) // 64
    for ti in range(nt):
        for tj in range(ti, nt):
            for row in range(64):
                i = ti * 64 + row
                first, last = (row + 1 if ti == tj else 0), min(63, n_ind - 1 - tj * 64)
                if i < n_ind and first <= last:
                    n += (last >> 4) - (first >> 4) + 1
    return n


# live slot groups and their padding to a multiple of 4, worked out by hand for the shapes below
SLOT_GROUPS = {9: (8, 0), 10: (9, 3), 11: (10, 2), 12: (11, 1), 70: (225, 3)}


@functools.lru_cache(maxsize=None)
def data(n_ind, n_sites, pdel):
    p = O.synth_indmajor(SEED, n_ind, n_sites, miss_frac=0.15)
    p.setflags(write=False)
    terms, valid = ST.site_terms(p, pdel, False)
    terms.setflags(write=False)
    valid.setflags(write=False)
    return p, terms, valid


def draw_maps(n_rep, n_blocks, seed=3):
    t = N().Taus(seed)
    return np.stack([t.block_map(n_blocks) for _ in range(n_rep)])


def check_plan(t, n_mat, q, chunks, pad):
    groups = (n_mat + 15) // 16
    assert t["matrices"] == n_mat and t["matrix_groups"] == groups, t
    assert t["unit_sites"] == q, t
    assert t["chunks"] == chunks, t
    assert t["contract_launches"] == chunks * ((groups + 7) // 8), t
    assert t["slot_groups"] - t["slot_groups_live"] == pad and t["slot_groups"] % 4 == 0, t


def run_three_ways(p, n_mat, lead, pdel, block_size):
    """the job in one chunk, in chunks of 2 k-groups of terms, and by the engine's own em_spill = 0 passes; the plan of the
    two spilled runs asserted from the engine's report -> ((S, C) one chunk, (S, C) chunked, (S, C) em_spill = 0, W)"""
    n_ind, n_sites, _ = p.shape
    n_rep = n_mat - (1 if lead else 0)
    n_blocks = n_sites // block_size
    maps = draw_maps(n_rep, n_blocks)
    q = spill_unit(block_size)
    s_end = n_sites if lead else n_blocks * block_size
    live, pad = SLOT_GROUPS[n_ind]
    assert (live, pad) == (live_slot_groups(n_ind), -live_slot_groups(n_ind) % 4)
    with N().Engine(n_ind, n_sites, pairwise_del=pdel, indep_geno=False, kernel="em_table") as e:
        e.set_option("boot_partials", 0)
        e.upload_ind_major(p).commit()
        call = (lambda: e.run_job(maps, block_size)) if lead else (lambda: e.run_batch(maps, block_size))
        one = call()
        t = e.spill_timing()
        check_plan(t, n_mat, q, 1, pad)
        assert t["slot_groups_live"] == live
        # scratch for 2 k-groups (8 units) of terms + the tail k-group of the operand run-ahead
        e.set_option("em_spill_bytes", (2 + 1) * int(t["slot_groups"]) * 64 * 8)
        chunked = call()
        check_plan(e.spill_timing(), n_mat, q, -(-s_end // (8 * q)), pad)
        e.set_option("em_spill", 0)
        own = call()
        assert e.spill_timing()["chunks"] == 0
    return one, chunked, own, ST.job_weights(n_sites, block_size, maps, lead)


def check_every_matrix(runs, own, W, terms, valid, pdel, exact=False):
    want_s, want_c = ST.combine(W, terms), ST.combine_counts(W, valid, pdel)
    nan = np.isnan(want_s)
    S0, C0 = own
    assert np.array_equal(C0, want_c)
    for how, (S, Cn) in zip(("one chunk", "chunks of 2 k-groups"), runs):
        assert S.shape == want_s.shape
        assert np.array_equal(Cn, want_c), how
        assert np.array_equal(np.isnan(S), nan) and np.array_equal(np.isnan(S0), nan), how
        worst = 0.0
        for r in range(W.shape[0]):  # every matrix
            ok = ~nan[r]
            assert np.all(np.isfinite(S[r][ok])), (how, r)
            if exact:
                assert np.array_equal(S[r].view(np.uint64), want_s[r].view(np.uint64)), (how, r)
            err = rel_err(S[r][ok], want_s[r][ok])
            assert err < RTOL, (how, r, err)
            assert rel_err(S[r][ok], S0[r][ok]) < RTOL_SELF, (how, r)
            worst = max(worst, err)
        print("%s: %d matrices, max rel err %.3g against the combined site terms" % (how, W.shape[0], worst))


N_MAT_SWEEP = [3, 16, 17, 33, 49, 64, 65, 81, 97, 113, 128, 129, 145, 200, 257]


@pytest.mark.parametrize("k,n_mat", list(enumerate(N_MAT_SWEEP)))
def test_every_matrix_count_arm(k, n_mat):
    """11 k-groups, the last one partial; RT = 1 .. 8 as a first launch, PT = 4 and 2, remainder launches of RT = 1 (129
    matrices), 2 (145) and 5 with PT = 2 (200), three launches (257); jobs with a lead matrix and batches without,
    --pairwise_del off and on, in turn down the list"""
    lead, pdel = k % 2 == 0, (k // 2) % 2 == 1
    p, terms, valid = data(10, 43, pdel)
    one, chunked, own, W = run_three_ways(p, n_mat, lead, pdel, 1)
    assert W.shape[0] == n_mat
    check_every_matrix((one, chunked), own, W, terms, valid, pdel)


GEOMETRY = [(43, 1), (43, 5), (300, 128), (300, 130)]  # q = 1, 5 (n_eff = 40: the lead's last unit holds 3 sites), 64, 26


@pytest.mark.parametrize("n_mat", [17, 129])
@pytest.mark.parametrize("i,n_ind", list(enumerate([9, 10, 11, 12, 70])))
@pytest.mark.parametrize("j,geometry", list(enumerate(GEOMETRY)))
def test_slot_group_padding_and_unit_sizes(n_mat, i, n_ind, j, geometry):
    """8, 9, 10 and 11 live slot groups (padding 0, 3, 2, 1), three 64-tiles of which one has 6 live columns; units of 1, 5,
    64 and 26 sites, a last unit that is short; one group of matrices + one, and a remainder launch"""
    n_sites, block_size = geometry
    assert spill_unit(block_size) == (1, 5, 64, 26)[j]
    pdel = (i + j) % 2 == 1
    p, terms, valid = data(n_ind, n_sites, pdel)
    one, chunked, own, W = run_three_ways(p, n_mat, True, pdel, block_size)
    check_every_matrix((one, chunked), own, W, terms, valid, pdel)


@functools.lru_cache(maxsize=None)
def called(n_ind, n_sites):
    g = np.random.default_rng(1).integers(0, 3, size=(n_ind, n_sites))
    p = np.zeros((n_ind, n_sites, 3))
    np.put_along_axis(p, g[..., None], 1.0, axis=2)
    p.setflags(write=False)
    return p


def test_called_genotypes_plain_pass_bit_exact():
    """the README's claim for called genotypes, on the table-driven EM kernel: one-hot likelihoods make every term 0, 1/2 or
    1 (the oracle's EM-path sums are the --indep_geno sums bit for bit), so the plain pass gives those bits"""
    p = called(10, 43)
    so, co = O.all_pairs(p, indep_geno=True)
    se, ce = O.all_pairs(p, indep_geno=False)
    assert np.array_equal(se.view(np.uint64), so.view(np.uint64)) and np.array_equal(ce, co)
    with N().Engine(10, 43, indep_geno=False, kernel="em_table") as e:
        s, c = e.upload_ind_major(p).commit().run()
    assert np.array_equal(c, co)
    assert np.array_equal(s.view(np.uint64), so.view(np.uint64))


@pytest.mark.parametrize("n_mat,pdel", [(49, False), (81, True), (200, False)])
def test_called_genotypes_every_matrix_bit_exact(n_mat, pdel):
    """weights and terms are small dyadics: any order of FP64 additions is exact, so every matrix of the job equals the
    integer reference bit for bit (RT = 4 / PT = 4, RT = 6 / PT = 2, and a remainder launch of RT = 5)"""
    p = called(10, 43)
    terms, valid = ST.site_terms(p, pdel, True)
    assert np.array_equal(terms, ST.site_terms(p, pdel, False)[0]) and set(np.unique(terms)) <= {0.0, 0.5, 1.0}
    one, chunked, own, W = run_three_ways(p, n_mat, True, pdel, 1)
    assert np.array_equal(ST.combine(W, terms), W.astype(np.float64) @ terms)  # (exact either way)
    check_every_matrix((one, chunked), own, W, terms, valid, pdel, exact=True)


@pytest.mark.parametrize("n_mat", [129, 200])
@pytest.mark.parametrize("block_size,site", [(1, 41), (5, 21)])
def test_terms_that_are_not_finite_reach_exactly_the_matrices_that_draw_them(n_mat, block_size, site):
    """an all-zero individual at one site (0 / 0 in normalize(), as on the CPU) -- in the last, partial k-group of the chunk,
    and as the second site of a unit of 5: k_spill_sanitize writes NaN at D[r >> 4][(r & 15) >> 2][r & 3] of every matrix r
    that weights the site, matrix groups of a remainder launch included; every other cell as without it"""
    n_ind, n_sites, who = 10, 43, 3
    q = spill_unit(block_size)
    assert (site // 4 == (n_sites - 1) // 4 and n_sites % 4 != 0) if q == 1 else (q == 5 and site % q == 1)
    p = np.array(data(n_ind, n_sites, False)[0])
    p[who, site] = 0.0
    terms, valid = ST.site_terms(p, False, False)
    one, chunked, own, W = run_three_ways(p, n_mat, True, False, block_size)
    pairs = np.array([who in (a, b) for a in range(n_ind) for b in range(a + 1, n_ind)])
    want_nan = np.outer(W[:, site] != 0, pairs)
    assert np.array_equal(np.isnan(ST.combine(W, terms)), want_nan)
    drawn = want_nan.any(axis=1)
    assert drawn[0] and drawn[1:128].any() and not drawn[1:128].all()
    if n_mat > 129:  # ... and both kinds among the matrices of the remainder launch
        assert drawn[128:].any() and not drawn[128:].all()
    for S, _ in (one, chunked):
        assert np.array_equal(np.isnan(S), want_nan)
    check_every_matrix((one, chunked), own, W, terms, valid, False)
