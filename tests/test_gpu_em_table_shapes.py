"""Workgroup shapes 1 to 4 of the table-driven EM kernel (ngd_config.variant; the shape table of accum_em_table.hip) in the
forms the rest of the suite reaches only where a random sweep happens to draw them: the weighted pass (a replicate as
run(block_map) without per-block partials: WEIGHTED = true, with and without --pairwise_del), the per-pair batch pass
these shapes borrow for a job (engine_plans.hip em_borrow: k_accum_em_batch<fast, PDEL, RB = 4 / 8 / 16> over slices of
its own rule, n_sites / 256), the plain pass of shape 4 against shape 0's bits, and the slices launcher of the eager
full-data pass.  Every matrix against the CPU oracle: counts exact, sums within 1e-9; the engine's own plans against
each other within 1e-12 (include/ngsdist_amd.h).  The oracle's matrices do not depend on the shape: computed once."""
import functools

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

RTOL = 1e-9
RTOL_SELF = 1e-12
VARIANTS = [1, 2, 3, 4]
N_INDS = [33, 65, 130]   # one 64-tile mostly empty, three tiles with a one-column edge, six with a two-column edge
N_SITES = [5, 257]       # fewer sites than a round of steps has wavefronts; a partial last group of 4
N_REPS = [3, 7, 20]      # with the lead matrix: 4, 8 and 16 + 5 matrices -- RB = 4, 8, and 16 then 8 in a second pass


def N():
    import ngsdist_amd
    return ngsdist_amd


def rel_err(a, b):
    a, b = np.asarray(a), np.asarray(b)
    den = np.where(b == 0, 1.0, np.abs(b))
    return float(np.max(np.abs(a - b) / den)) if a.size else 0.0


def bits(a):
    return np.asarray(a).view(np.uint64)


@functools.lru_cache(maxsize=None)
def data(n_ind, n_sites):
    p = O.synth_indmajor(41, n_ind, n_sites, miss_frac=0.1)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def maps_of(n_sites, B, n_rep):
    t = N().Taus(17 + B)
    m = np.stack([t.block_map(n_sites // B) for _ in range(n_rep)])
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def oracle_matrix(n_ind, n_sites, pdel, B, r):
    """matrix r of the job over maps_of(n_sites, B, 20): r = -1 the full data set, else replicate r (a prefix of the 20 maps
    serves the shorter jobs)"""
    p = data(n_ind, n_sites)
    if r < 0:
        return O.all_pairs(p, pairwise_del=pdel, indep_geno=False, n_threads=8)
    src = O.boot_site_src(maps_of(n_sites, B, 20)[r], B)
    return O.all_pairs(p, pairwise_del=pdel, indep_geno=False, site_src=src, n_sites=n_sites // B * B, n_threads=8)


def engine(n_ind, n_sites, pdel, variant, **options):
    e = N().Engine(n_ind, n_sites, pairwise_del=pdel, indep_geno=False, kernel="em_table", variant=variant)
    for k, v in options.items():
        e.set_option(k, v)
    e.upload_ind_major(data(n_ind, n_sites)).commit()
    return e


def against_oracle(s, c, ref, tag):
    so, co = ref
    assert np.array_equal(c, co), tag
    assert np.all(np.isfinite(s)), tag
    err = rel_err(s, so)
    assert err < RTOL, (tag, err)


@pytest.mark.parametrize("pdel", [False, True])
@pytest.mark.parametrize("n_sites", N_SITES)
@pytest.mark.parametrize("n_ind", N_INDS)
@pytest.mark.parametrize("variant", VARIANTS)
def test_weighted_pass(variant, n_ind, n_sites, pdel):
    """run(block_map, B) without per-block partials: one list-driven weighted pass of the shape's own kernel"""
    with engine(n_ind, n_sites, pdel, variant, boot_partials=0) as e:
        for B in (1, 7):
            if B > n_sites:  # no whole block: refused as everywhere (ngd_run: empty bootstrap geometry)
                with pytest.raises(N().NgdError) as ei:
                    e.run(np.zeros(0, dtype=np.uint64), B)
                assert ei.value.code == -1
                continue
            for r in (0, 1):
                s, c = e.run(maps_of(n_sites, B, 20)[r], B)
                against_oracle(s, c, oracle_matrix(n_ind, n_sites, pdel, B, r), (B, r))
        s, c = e.run()  # ... and the plain pass afterwards
        against_oracle(s, c, oracle_matrix(n_ind, n_sites, pdel, 1, -1), "plain")


def job_both_ways(variant, n_ind, n_sites, pdel, B, n_reps):
    with engine(n_ind, n_sites, pdel, variant, boot_partials=0) as e:
        for n_rep in n_reps:
            maps = maps_of(n_sites, B, 20)[:n_rep]
            e.set_option("em_batch", 1)
            S, Cn = e.run_job(maps, B)
            assert e.spill_timing()["chunks"] == 0  # (the spilled-terms plan is shape 0's)
            launches = e.timing()["launches"]
            e.set_option("em_batch", 0)
            S1, C1 = e.run_job(maps, B)
            assert S.shape == (n_rep + 1, e.n_pairs)
            for m in range(n_rep + 1):  # every matrix
                against_oracle(S[m], Cn[m], oracle_matrix(n_ind, n_sites, pdel, B, m - 1), (n_rep, m))
                assert np.array_equal(Cn[m], C1[m]) and rel_err(S[m], S1[m]) < RTOL_SELF, (n_rep, m)
            # the borrowed batch pass: ceil(n_mat / 16) accumulation launches; one pass per matrix otherwise
            assert launches == (n_rep + 1 + 15) // 16 and e.timing()["launches"] == n_rep + 1, (n_rep, launches)


@pytest.mark.parametrize("pdel", [False, True])
@pytest.mark.parametrize("n_sites", N_SITES)
@pytest.mark.parametrize("n_ind", N_INDS)
@pytest.mark.parametrize("variant", VARIANTS)
def test_job_by_the_borrowed_batch_pass(variant, n_ind, n_sites, pdel):
    """jobs of 3, 7 and 20 replicates with em_batch = 1 (k_accum_em_batch, RB = 4, 8, 16 and a second pass) and with
    em_batch = 0 (one pass of the shape's own kernel per matrix): every matrix against the oracle, the two within 1e-12;
    blocks of 7 at 257 sites (n_eff = 252: the last 5 sites are the lead matrix's alone)"""
    job_both_ways(variant, n_ind, n_sites, pdel, 1 if n_sites < 7 else 7, N_REPS)


def test_job_where_the_borrowed_kernel_takes_two_slices():
    """600 sites: n_sites / 256 = 2 slices of the borrowed per-pair kernel (the shape's own kernel keeps its slices)"""
    job_both_ways(1, 65, 600, True, 1, [20])


@pytest.mark.parametrize("pdel", [False, True])
@pytest.mark.parametrize("n_sites", N_SITES)
@pytest.mark.parametrize("n_ind", N_INDS)
def test_shape_4_gives_the_bits_of_shape_0(n_ind, n_sites, pdel):
    """accum_em_table.hip's shape table: the default form packs a site's later rounds, shape 4 scans every round row by row
    -- the same bits"""
    with engine(n_ind, n_sites, pdel, 0) as e:
        s0, c0 = e.run()
    with engine(n_ind, n_sites, pdel, 4) as e:
        s4, c4 = e.run()
    assert np.array_equal(c0, c4)
    assert np.array_equal(bits(s0), bits(s4))


@pytest.mark.parametrize("variant", VARIANTS)
def test_full_data_pass_started_beside_a_staged_load(variant):
    """NGD_OPT_EAGER_FULL on shapes 1 to 4 (ngd_launch_accum_em_table_slices): the leading slices of the plain pass are
    accumulated while the pieces of a staged load are still arriving -- the bits and counts of the same engine without it,
    as tests/test_gpu_parity.py asserts for shape 0; one shape against the oracle too"""
    n_ind, n_sites, pdel = 90, 30_000, variant % 2 == 0
    raw = np.ascontiguousarray(O.synth_indmajor(77, n_ind, n_sites, miss_frac=0.05 if pdel else 0.0).transpose(1, 0, 2))
    res = {}
    for eager in (0, 1):
        with N().Engine(n_ind, n_sites, pairwise_del=pdel, indep_geno=False, kernel="em_table", variant=variant) as e:
            e.set_option("stage_piece_mib", 1)  # many pieces, so that slices complete while later ones are still in flight
            e.set_option("eager_full", eager)
            e.upload_raw_sites(raw, 0).commit()
            res[eager] = e.run()
            again = e.run()  # nothing eager left
            assert np.array_equal(bits(again[0]), bits(res[eager][0])) and np.array_equal(again[1], res[eager][1])
    assert np.array_equal(bits(res[0][0]), bits(res[1][0])) and np.array_equal(res[0][1], res[1][1])
    if variant == 3:
        so, co = O.all_pairs(np.ascontiguousarray(raw.transpose(1, 0, 2)), pairwise_del=pdel, indep_geno=False, n_threads=16)
        against_oracle(res[1][0], res[1][1], (so, co), "eager")
