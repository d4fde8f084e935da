"""The later table rounds of the EM kernels on planted input (tests/em_rounds_expect.py): every stopping step from 1 to
T_MAX = 40, one to three packed units per wavefront, rows on either side of the dense line, every skip and prefetch pattern
of neighbouring rows, a third round (a fourth of the 12-step shapes) from one pair to a whole tile -- in every form that
shares accum_em_table.hip's round code (weighted, several matrices per pass, spilled terms, the slice table, the three
noting forms) and in the per-pair kernels, whose loops see steps beyond 31 nowhere else in the suite.  Every matrix against
the CPU oracle: counts equal, sums within 1e-9, all finite; the table rounds the engine reports against the count the
stopping steps imply.  tests/test_em_rounds_cpu.py holds what makes that a check of the stopping step: no (pair, site) of
the scenes comes within 1e-9 of the tolerance."""
import functools

import numpy as np
import pytest

import em_rounds_expect as X
from oracle import oracle as O
from test_gpu_em_boundary import CASES, c_at, find_boundary

pytestmark = pytest.mark.gpu

RTOL = 1e-9
N_IND = X.N_IND
# steps per table round of ngd_config.variant 0 ... 4: the CH of with_shape()'s table in accum_em_table.hip (the engine does not
# report it; if a shape's round length changes there, test_plain_pass_and_its_table_rounds fails on the count and this line moves)
CH = {0: 16, 1: 16, 2: 12, 3: 12, 4: 16}
VARIANTS = [0, 1, 2, 3, 4]
# (the scenes with missing data, --pairwise_del): without it the uniform vectors are data, and a pair of them stops at step 1
MODES = [(False, False), (True, True), (True, False)]
N_TILES = 6


def N():
    import ngsdist_amd
    return ngsdist_amd


@functools.lru_cache(maxsize=None)
def data(miss):
    return X.scenes(miss=miss)[0]


def n_sites():
    return data(False).shape[1]


@functools.lru_cache(maxsize=None)
def oracle_plain(miss, pdel):
    return O.all_pairs(data(miss), pairwise_del=pdel, indep_geno=False, n_threads=8)


@functools.lru_cache(maxsize=None)
def maps_of(B, n_rep=7):
    t = N().Taus(23 + B)
    m = np.stack([t.block_map(n_sites() // B) for _ in range(n_rep)])
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def oracle_rep(miss, pdel, B, r):
    """replicate r of maps_of(B); r = -1: the full data set"""
    if r < 0:
        return oracle_plain(miss, pdel)
    src = O.boot_site_src(maps_of(B)[r], B)
    return O.all_pairs(data(miss), pairwise_del=pdel, indep_geno=False, site_src=src, n_sites=n_sites() // B * B, n_threads=8)


@functools.lru_cache(maxsize=None)
def rounds_of(miss, pdel, ch):
    return X.expected_rounds(data(miss), ch, N_IND, pdel)


def rel_err(a, b):
    a, b = np.asarray(a), np.asarray(b)
    den = np.where(b == 0, 1.0, np.abs(b))
    return float(np.max(np.abs(a - b) / den)) if a.size else 0.0


def against_oracle(s, c, ref, tag):
    so, co = ref
    assert np.array_equal(c, co), tag
    assert np.all(np.isfinite(s)), tag
    err = rel_err(s, so)
    assert err < RTOL, (tag, err)


def engine(miss, pdel, kernel="em_table", variant=0, **options):
    e = N().Engine(N_IND, n_sites(), pairwise_del=pdel, indep_geno=False, kernel=kernel, variant=variant)
    e.upload_ind_major(data(miss)).commit()
    for k, v in options.items():
        e.set_option(k, v)
    return e


def O_pair(i1, i2):
    return N_IND * i1 - i1 * (i1 + 1) // 2 + (i2 - i1 - 1)


# ---- the plain pass ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES, ids=lambda m: "miss%d-pdel%d" % m)
@pytest.mark.parametrize("variant", VARIANTS)
def test_plain_pass_and_its_table_rounds(variant, mode):
    miss, pdel = mode
    with engine(miss, pdel, variant=variant) as e:
        s, c = e.run()
        tile_sites, rounds = e.em_work()
        launches = e.timing()["launches"]
    against_oracle(s, c, oracle_plain(miss, pdel), (variant, mode))
    want = rounds_of(miss, pdel, CH[variant])
    print("variant %d %s: %d table rounds over %d (tile, site)s, expected %d" % (variant, mode, rounds, tile_sites, want))
    assert launches == 1 and tile_sites == N_TILES * n_sites()  # one pass of the table kernel over every tile and site
    assert rounds == want


@pytest.mark.parametrize("mode", MODES, ids=lambda m: "miss%d-pdel%d" % m)
def test_shape_4_gives_the_bits_of_shape_0(mode):
    miss, pdel = mode
    with engine(miss, pdel, variant=0) as e:
        s0, c0 = e.run()
        w0 = e.em_work()
    with engine(miss, pdel, variant=4) as e:
        s4, c4 = e.run()
        w4 = e.em_work()
    assert np.array_equal(c0, c4) and w0 == w4
    assert np.array_equal(s0.view(np.uint64), s4.view(np.uint64))


# ---- weighted, several matrices per pass, spilled terms --------------------------------------------------------------------------

@pytest.mark.parametrize("pdel", [False, True])
@pytest.mark.parametrize("variant", VARIANTS)
def test_weighted_pass(variant, pdel):
    """a replicate as run(block_map) without per-block partials: sites that are not drawn are skipped whole"""
    with engine(pdel, pdel, variant=variant, boot_partials=0) as e:
        for B in (1, 7):
            for r in (0, 1):
                s, c = e.run(maps_of(B)[r], B)
                drawn = len(np.unique(maps_of(B)[r])) * B  # sites of weight 0 are skipped whole: no (tile, site) visit
                assert e.timing()["launches"] == 1 and e.em_work()[0] == N_TILES * drawn, (B, r, e.em_work(), drawn)
                against_oracle(s, c, oracle_rep(pdel, pdel, B, r), (B, r))
            assert len(np.unique(maps_of(B)[0])) < n_sites() // B  # (some block is not drawn)


@pytest.mark.parametrize("pdel", [False, True])
def test_four_and_eight_matrices_per_pass(pdel):
    """em_batch = 1 on shape 0: jobs of 3 and 7 replicates are ONE pass of the RB = 4 / RB = 8 form (2 waves per SIMD)"""
    with engine(pdel, pdel, boot_partials=0, em_spill=0, em_batch=1) as e:
        for n_rep, B in ((3, 1), (7, 1), (3, 7), (7, 7)):
            S, Cn = e.run_job(maps_of(B)[:n_rep], B)
            assert e.timing()["launches"] == 1 and e.spill_timing()["chunks"] == 0, (n_rep, B)
            for m in range(n_rep + 1):
                against_oracle(S[m], Cn[m], oracle_rep(pdel, pdel, B, m - 1), (n_rep, B, m))


@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("pdel", [False, True])
def test_spilled_terms(pdel, B):
    with engine(pdel, pdel, boot_partials=0, em_spill=1) as e:
        S, Cn = e.run_job(maps_of(B)[:5], B)
        spill = e.spill_timing()
    assert spill["chunks"] >= 1 and spill["matrices"] == 6, spill
    for m in range(6):
        against_oracle(S[m], Cn[m], oracle_rep(pdel, pdel, B, m - 1), (B, m))


# ---- the slice-table form ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def windows():
    """every site on its own, every group of scenes, everything"""
    info = X.scenes()[1]
    lo, hi = list(range(n_sites())), list(range(1, n_sites() + 1))
    kinds = [x["kind"] for x in info]
    start = 0
    for s in range(1, n_sites() + 1):
        if s == n_sites() or kinds[s] != kinds[start]:
            lo.append(start)
            hi.append(s)
            start = s
    lo.append(0)
    hi.append(n_sites())
    lo, hi = np.array(lo, dtype=np.int64), np.array(hi, dtype=np.int64)
    order = np.lexsort((hi, lo))  # (window starts must not decrease)
    return lo[order], hi[order]


@functools.lru_cache(maxsize=None)
def oracle_windows(miss, pdel):
    lo, hi = windows()
    p = data(miss)
    out = [O.all_pairs(np.ascontiguousarray(p[:, a:b]), pairwise_del=pdel, indep_geno=False, n_threads=8) for a, b in zip(lo, hi)]
    return np.stack([s for s, _ in out]), np.stack([c for _, c in out])


def windows_against_oracle(S, Cn, miss, pdel, tag):
    So, Co = oracle_windows(miss, pdel)
    assert np.array_equal(Cn, Co), tag
    assert np.all(np.isfinite(S)), tag
    assert np.all(np.abs(S - So) <= RTOL * np.abs(So)), (tag, rel_err(S, So))  # (a cell without a valid site is 0)


@pytest.mark.parametrize("pdel", [False, True])
@pytest.mark.parametrize("variant", VARIANTS)
def test_windows_by_the_slice_table(variant, pdel):
    lo, hi = windows()
    with engine(pdel, pdel, variant=variant, win_plan=2) as e:
        S, Cn = e.run_windows(lo, hi)
        info = e.windows_info()
    assert info["windows_by_pass"] == 0 and info["segments"] >= n_sites(), info  # the slab plan: a segment per site at least
    windows_against_oracle(S, Cn, pdel, pdel, variant)


# ---- the per-pair kernels --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pdel", [False, True])
@pytest.mark.parametrize("kernel", ["em_fast", "em_faithful"])
def test_per_pair_kernels_plain_weighted_and_batch(kernel, pdel):
    with engine(pdel, pdel, kernel=kernel, boot_partials=0, em_batch=1) as e:
        s, c = e.run()
        against_oracle(s, c, oracle_plain(pdel, pdel), kernel)
        assert e.em_work()[1] == 0  # (not the table kernel)
        for B in (1, 7):
            s, c = e.run(maps_of(B)[0], B)
            against_oracle(s, c, oracle_rep(pdel, pdel, B, 0), (kernel, B))
            for n_rep in (3, 7):
                S, Cn = e.run_job(maps_of(B)[:n_rep], B)
                for m in range(n_rep + 1):
                    against_oracle(S[m], Cn[m], oracle_rep(pdel, pdel, B, m - 1), (kernel, B, n_rep, m))


# ---- the noting forms: nothing of the scenes is within 2^-36 of the tolerance --------------------------------------------------------

@pytest.mark.parametrize("pdel", [False, True])
@pytest.mark.parametrize("variant", VARIANTS)
def test_noting_plain_pass_notes_nothing(variant, pdel):
    with engine(pdel, pdel, variant=variant, em_exact=1) as e:
        s, c = e.run()
        info, ent, rounds = e.last_em_exact(), e.em_exact_entries(), e.em_work()[1]
    assert info["noted"] == 0 and len(ent) == 0 and info["passes"] == 1, info
    assert rounds == rounds_of(pdel, pdel, CH[variant])
    against_oracle(s, c, oracle_plain(pdel, pdel), variant)


@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("pdel", [False, True])
def test_noting_spilled_terms_note_nothing(pdel, B):
    with engine(pdel, pdel, boot_partials=0, em_spill=2, em_exact=2) as e:
        S, Cn = e.run_job(maps_of(B)[:5], B)
        info, spill = e.last_em_exact(), e.spill_timing()
    assert info["noted"] == 0 and spill["chunks"] >= 1 and spill["matrices"] == 6, (info, spill)
    for m in range(6):
        against_oracle(S[m], Cn[m], oracle_rep(pdel, pdel, B, m - 1), (B, m))


@pytest.mark.parametrize("pdel", [False, True])
@pytest.mark.parametrize("variant", VARIANTS)
def test_noting_windows_note_nothing(variant, pdel):
    lo, hi = windows()
    with engine(pdel, pdel, variant=variant, win_plan=2, em_exact=1, em_exact_win=1) as e:
        S, Cn = e.run_windows(lo, hi)
        info, win = e.last_em_exact(), e.windows_info()
    assert info["noted"] == 0 and win["windows_by_pass"] == 0, (info, win)
    windows_against_oracle(S, Cn, pdel, pdel, variant)


# ---- notes raised in a later round -------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def probes():
    pr = X.boundary_probes(CASES, find_boundary)
    p, planted = X.probe_scenes(pr)
    return pr, p, planted, O.all_pairs(p, indep_geno=False, n_threads=8)


@pytest.mark.parametrize("variant", VARIANTS)
def test_notes_raised_in_rounds_2_and_3_by_packed_units_and_by_the_row_scan(variant):
    """stops within a few ulps of the tolerance near steps 18 and 34 (cases 1 and 2 of tests/test_gpu_em_boundary.py), each
    once as the only column still searching in its round (shape 0: packed_units notes it, row and column from the unit's
    list) and once in a row with 31 pairs still searching (scan_row notes it): the list holds exactly the planted (pair,
    site)s at the oracle's step, and the sums are the oracle's"""
    pr, p, planted, (so, co) = probes()
    with N().Engine(N_IND, p.shape[1], indep_geno=False, kernel="em_table", variant=variant) as e:
        e.upload_ind_major(p).commit()
        e.set_option("em_exact", 1)
        s, c = e.run()
        ent, info = e.em_exact_entries(), e.last_em_exact()
    T_or = {site: O.em2(p[i1, site], p[i2, site])[1] for i1, i2, site, _ in planted}
    got = [(int(x["i1"]), int(x["i2"]), int(x["site"])) for x in ent]
    assert got == sorted((i1, i2, site) for i1, i2, site, _ in planted), (got, planted)
    assert info["noted"] == len(planted) and info["passes"] == 1
    for x in ent:
        assert int(x["t_ref"]) == T_or[int(x["site"])], x
        assert abs(int(x["t_dev"]) - int(x["t_ref"])) <= 1, x
    assert {T_or[site] > 32 for *_, site, _ in planted} == {False, True} and min(T_or.values()) > 16
    against_oracle(s, c, (so, co), variant)
    # the planted pair's sum: its term of every site at the oracle's step
    (i1, i2) = planted[0][:2]
    want = sum(c_at(p[i1, site], p[i2, site], T_or[site]) for *_, site, _ in planted)
    assert abs(s[O_pair(i1, i2)] - want) / want < 1e-12, (s[O_pair(i1, i2)], want)
