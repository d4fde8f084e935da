"""Bootstrap replicates inside windows of UNEQUAL length (ngd_run_windows_job_var*, windows in base pairs): every matrix of
every window against the CPU oracle on the window's sites with the window's own maps, through both plans (the unit slab
with the descriptor form of the banded reduction, one job per window), every kernel and the engine ABI.

The data set: 777 sites on two chromosomes with uneven gaps between positions, windows of 2000 bp every 700 bp -- 49 windows
of 28 distinct lengths from 1 to 107 sites, so that windows shorter than a block, whole numbers of blocks, shared lengths and
two chunks of replicates all occur.  The expected value for (window w, replicate r) is the oracle over
site_src = lo[w] + boot_site_src(map_w[r], q) with map_w drawn from a generator seeded anew for the window's n_blocks.

On the EM path the oracle's per-site terms (tests/site_terms.py: the oracle on one-site slices, a term does not depend on the
window it is added to) are combined with each matrix's weights; the direct oracle on every window there would take minutes
at 130 individuals.  The all-zero-individual test runs the oracle directly on every window, at its small size."""
import functools

import numpy as np
import pytest

import site_terms as ST
from oracle import oracle as O

pytestmark = pytest.mark.gpu

RTOL = 1e-9        # against the oracle: the suite's figure
RTOL_SELF = 1e-12  # between plans of the engine that differ in the order of additions (include/ngsdist_amd.h)
N_SITES, SIZE_BP, STEP_BP = 777, 2000, 700


def N():
    import ngsdist_amd
    return ngsdist_amd


def rel_err(a, b):
    a, b = np.asarray(a), np.asarray(b)
    den = np.where(b == 0, 1.0, np.abs(b))
    return float(np.max(np.abs(a - b) / den)) if a.size else 0.0


def positions():
    rng = np.random.default_rng(3)
    gaps = rng.integers(1, 40, N_SITES)
    g2 = gaps[600:].copy()
    g2[100:] *= 12
    return np.concatenate([np.cumsum(gaps[:600]), np.cumsum(g2)]).astype(np.uint64), [0] * 600 + [1] * 177


@functools.lru_cache(maxsize=None)
def bp_windows():
    pos, chrom = positions()
    lo, hi, start = N().window_ranges_bp(pos, SIZE_BP, STEP_BP, chrom)
    L = (hi - lo).astype(np.int64)
    # what a CPU prototype of the definition gives on this data
    assert len(lo) == 49 and len(set(L)) == 28 and L.min() == 1 and L.max() == 107
    assert (L // 7 == 0).sum() == 8 and ((L % 7 == 0) & (L >= 7)).sum() == 5 and (L // 20 == 0).sum() == 29
    assert len(L) - len(set(L)) >= 5  # several windows share a length
    assert np.all(np.diff(lo.astype(np.int64)) >= 0) and np.all(lo < hi)
    return lo, hi


def oracle_maps(seed, lo, hi, n_rep, q):
    """the maps of every window, drawn on the CPU: a generator seeded anew per n_blocks -> list of [n_rep][n_blocks_w]"""
    by_nb = {}
    out = []
    for a, b in zip(lo, hi):
        nb = int(b - a) // q
        if nb not in by_nb:
            t = O.Taus(seed)
            by_nb[nb] = np.stack([t.block_map(nb) for _ in range(n_rep)]) if nb else np.zeros((n_rep, 0), dtype=np.uint64)
        out.append(by_nb[nb])
    return out


def oracle_job_var(p, lo, hi, wmaps, q, pairwise_del=False, indep_geno=True):
    """-> (sums, counts) [n_win][n_rep + 1][n_pairs], the oracle on every (window, matrix); no block: sum 0, count 0"""
    n_pairs = O.n_pairs(p.shape[0])
    S, Cn = [], []
    for a, b, maps in zip(lo, hi, wmaps):
        srcs = [np.arange(a, b)] + [int(a) + O.boot_site_src(m, q) for m in maps]
        s = np.zeros((len(srcs), n_pairs))
        c = np.zeros((len(srcs), n_pairs), dtype=np.uint64)
        for k, src in enumerate(srcs):
            if len(src):
                s[k], c[k] = O.all_pairs(p, pairwise_del=pairwise_del, indep_geno=indep_geno, site_src=src, n_threads=8)
        S.append(s)
        Cn.append(c)
    return np.stack(S), np.stack(Cn)


@functools.lru_cache(maxsize=None)
def em_terms(seed, n_ind):
    return ST.site_terms(O.synth_indmajor(seed, n_ind, N_SITES), False, False)


def terms_job_var(terms, valid, lo, hi, wmaps, q):
    """the same from per-site terms (EM path): sum_s W[w][r][s] terms[s]"""
    S, Cn = [], []
    for a, b, maps in zip(lo, hi, wmaps):
        W = ST.job_weights(int(b - a), q, maps=maps, lead=True) if maps.shape[1] else \
            np.concatenate([np.ones((1, int(b - a)), np.int64), np.zeros((len(maps), int(b - a)), np.int64)])
        S.append(ST.combine(W, terms[a:b]))
        Cn.append(ST.combine_counts(W, valid[a:b], False))
    return np.stack(S), np.stack(Cn)


N_REP_MAX = 40


@functools.lru_cache(maxsize=None)
def synth_case(seed, n_ind, miss_frac, q, map_seed, pairwise_del, indep_geno):
    """p, the windows, the engine's maps (40 replicates: fewer are a prefix of every class) and the oracle's matrices"""
    lo, hi = bp_windows()
    p = O.synth_indmajor(seed, n_ind, N_SITES, miss_frac=miss_frac)
    wmaps = oracle_maps(map_seed, lo, hi, N_REP_MAX, q)
    if indep_geno:
        ref = oracle_job_var(p, lo, hi, wmaps, q, pairwise_del, True)
    else:
        ref = terms_job_var(*em_terms(seed, n_ind), lo, hi, wmaps, q)
    return p, lo, hi, wmaps, ref


def engine_maps(seed, lo, hi, n_rep, q, wmaps=None):
    """the maps as the engine's door draws them; against the CPU's when given"""
    maps, off = N().window_boot_maps(seed, lo, hi, n_rep, q)
    if wmaps is not None:
        for w in range(len(lo)):
            nb = int(hi[w] - lo[w]) // q
            got = maps[int(off[w]):int(off[w]) + n_rep * nb].reshape(n_rep, nb)
            assert np.array_equal(got, wmaps[w][:n_rep]), "window %d draws other maps than the cut-down run" % w
    return maps, off


def engine(p, kernel, pairwise_del=False, indep_geno=True, **kw):
    n_ind, n_sites, _ = p.shape
    e = N().Engine(n_ind, n_sites, pairwise_del=pairwise_del, indep_geno=indep_geno, kernel=kernel, **kw)
    e.upload_ind_major(p).commit()
    return e


def check(e, lo, hi, maps, off, q, n_rep, ref, plans, exact=False, nan_ok=False):
    so, co = ref[0][:, :n_rep + 1], ref[1][:, :n_rep + 1]
    got = {}
    for plan in plans:
        e.set_option("win_plan", plan)
        s, c = e.run_windows_job_var(lo, hi, maps, off, q, n_rep=n_rep)
        assert s.shape == (len(lo), n_rep + 1, e.n_pairs) and c.shape == s.shape
        assert np.array_equal(c, co), "plan %d: counts" % plan
        if exact:
            assert np.array_equal(s, so), "plan %d: called genotypes must be bit-exact" % plan
        ok = np.isfinite(so) if nan_ok else np.ones(so.shape, dtype=bool)
        if nan_ok:
            assert np.array_equal(np.isnan(s), np.isnan(so)), "plan %d: non-finite terms in the wrong matrices" % plan
        err = rel_err(s[ok], so[ok])
        print("plan %d q %d R %d: max rel err %.3g" % (plan, q, n_rep, err))
        assert err < RTOL, "plan %d" % plan
        info = e.windows_info()
        if plan == 1:
            assert info["windows_by_pass"] == len(lo) and info["segments"] == 0 and info["batches"] == 0
        if plan == 2:
            assert info["windows_by_pass"] == 0 and info["batches"] >= 2 and info["segments"] >= 1
        got[plan] = s[ok]
    if 1 in got and 2 in got:
        err = rel_err(got[2], got[1])
        print("plans 2 / 1: max rel diff %.3g" % err)
        assert err <= RTOL_SELF
    return s, c


MFMA = [("mfma", {"single_image": 3}), ("mfma", {"single_image": 2})]


@pytest.mark.parametrize("kernel,kw,plans", [(k, kw, (0, 1, 2)) for k, kw in MFMA] + [("stream", {}, (0, 1))],
                         ids=["two-images", "congruent", "stream"])
@pytest.mark.parametrize("n_ind", [6, 40, 130])
@pytest.mark.parametrize("q", [1, 7, 20])
@pytest.mark.parametrize("n_rep", [5, 40])
def test_indep_jobs_against_the_oracle(kernel, kw, plans, n_ind, q, n_rep):
    p, lo, hi, wmaps, ref = synth_case(7, n_ind, 0.0, q, 11, False, True)
    maps, off = engine_maps(11, lo, hi, n_rep, q, wmaps)
    with engine(p, kernel, **kw) as e:
        _, c = check(e, lo, hi, maps, off, q, n_rep, ref, plans)
        # a replicate's count is n_blocks_w q, 0 for a window shorter than one block
        assert np.array_equal(c[:, 1:, 0], np.repeat((((hi - lo) // np.uint64(q)) * np.uint64(q))[:, None], n_rep, axis=1))
        if kernel == "stream":
            e.set_option("win_plan", 2)
            with pytest.raises(N().NgdError) as ei:
                e.run_windows_job_var(lo, hi, maps, off, q, n_rep=n_rep)
            assert ei.value.code == -1


@pytest.mark.parametrize("kernel,plans", [("em_table", (0, 1, 2)), ("em_fast", (0, 1))])
@pytest.mark.parametrize("n_ind", [6, 40, 130])
@pytest.mark.parametrize("q", [1, 7, 20])
@pytest.mark.parametrize("n_rep", [5, 40])
def test_em_jobs_against_the_oracle(kernel, plans, n_ind, q, n_rep):
    p, lo, hi, wmaps, ref = synth_case(7, n_ind, 0.0, q, 11, False, False)
    maps, off = engine_maps(11, lo, hi, n_rep, q, wmaps)
    with engine(p, kernel, indep_geno=False) as e:
        check(e, lo, hi, maps, off, q, n_rep, ref, plans)
        if kernel == "em_fast":
            e.set_option("win_plan", 2)
            with pytest.raises(N().NgdError) as ei:
                e.run_windows_job_var(lo, hi, maps, off, q, n_rep=n_rep)
            assert ei.value.code == -1


@pytest.mark.parametrize("kernel,kw,plans", [(k, kw, (0, 1, 2)) for k, kw in MFMA] + [("stream", {}, (0, 1))],
                         ids=["two-images", "congruent", "stream"])
@pytest.mark.parametrize("q", [7, 20])
def test_pairwise_del_jobs(kernel, kw, plans, q):
    p, lo, hi, wmaps, ref = synth_case(5, 40, 0.2, q, 3, True, True)
    n_vis = ((hi - lo) // np.uint64(q)) * np.uint64(q)
    assert (ref[1][:, 1:6] < n_vis[:, None, None]).any()  # some replicate count lies below n_blocks_w q
    maps, off = engine_maps(3, lo, hi, 5, q, wmaps)
    with engine(p, kernel, pairwise_del=True, **kw) as e:
        check(e, lo, hi, maps, off, q, 5, ref, plans)


@pytest.mark.parametrize("single_image", [2, 3])
def test_called_genotypes_bit_exact(single_image):
    rng = np.random.default_rng(1)
    n_ind, n_sites = 24, 900
    g = rng.integers(0, 3, size=(n_ind, n_sites))
    p = np.zeros((n_ind, n_sites, 3))
    np.put_along_axis(p, g[..., None], 1.0, axis=2)
    pos = np.cumsum(rng.integers(1, 40, n_sites))
    lo, hi, _ = N().window_ranges_bp(pos, 3000, 1100)
    assert len(set((hi - lo).tolist())) > 3
    for q in (7, 10):
        wmaps = oracle_maps(2, lo, hi, 6, q)
        ref = oracle_job_var(p, lo, hi, wmaps, q)
        maps, off = engine_maps(2, lo, hi, 6, q, wmaps)
        with engine(p, "mfma", single_image=single_image) as e:
            check(e, lo, hi, maps, off, q, 6, ref, plans=(0, 1, 2), exact=True)
            e.set_option("win_plan", 2)
            assert np.array_equal(e.run_windows_job_var(lo, hi, maps, off, q, n_rep=6)[0][:, 0], e.run_windows(lo, hi)[0])


@pytest.mark.parametrize("kernel,plans", [("em_table", (0, 1, 2)), ("em_fast", (0, 1))])
@pytest.mark.parametrize("q", [1, 7, 20])
def test_em_jobs_with_an_all_zero_individual(kernel, plans, q):
    """An all-zero individual at one site gives 0/0 as on the CPU: NaN for that individual's pairs in exactly the matrices that
    visit the site -- matrix 0 of the windows that hold it, and the replicates that draw its block."""
    n_ind, site = 20, 130
    lo, hi = bp_windows()
    p = O.synth_indmajor(11, n_ind, N_SITES, miss_frac=0.05)
    p[3, site] = 0
    wmaps = oracle_maps(9, lo, hi, 5, q)
    so, co = oracle_job_var(p, lo, hi, wmaps, q, indep_geno=False)
    nans = np.isnan(so).any(axis=2)  # [window][matrix]
    holds = (lo <= site) & (site < hi)
    assert holds.sum() >= 2 and np.array_equal(nans[:, 0], holds) and nans[:, 1:].any() and not nans[holds, 1:].all()
    maps, off = engine_maps(9, lo, hi, 5, q, wmaps)
    with engine(p, kernel, indep_geno=False) as e:
        check(e, lo, hi, maps, off, q, 5, (so, co), plans=plans, nan_ok=True)


@pytest.mark.parametrize("pdel", [False, True])
def test_a_budget_that_forces_several_batches_gives_the_unbatched_bits(pdel):
    """The unit slab's slices are cut by the boundaries of every window of the call, so a block is added up from the same
    slices wherever NGD_OPT_WIN_MAX_BYTES cuts the call into batches: the replicates carry the unbatched call's bits.  Matrix 0
    is ngd_run_windows()'s at the same budget; the budget here leaves that call one batch (98 window ends: at most 97
    segments) and cuts the unit slab (381 slices at q = 7) into several."""
    q, n_rep = 7, 40
    p, lo, hi, wmaps, ref = synth_case(5, 40, 0.2 if pdel else 0.0, q, 3, pdel, True)
    maps, off = engine_maps(3, lo, hi, n_rep, q, wmaps)
    plane = 128 * 128 * (12 if pdel else 8)  # a slice's partial sums (+ counts): n_pad = 128
    budget = 84 * plane + (1 << 20)
    # two windows of one length with more slices from the first to the second than the budget holds: their class is split
    lo_i, hi_i = lo.astype(np.int64).tolist(), hi.astype(np.int64).tolist()
    bnd = sorted({a + k * q for a, b in zip(lo_i, hi_i) for k in range((b - a) // q + 1)} | set(hi_i))
    between = max(len([s for s in bnd if lo_i[i] <= s < max(hi_i[i:j + 1])]) for i in range(len(lo_i)) for j in range(i + 1, len(lo_i))
                  if hi_i[i] - lo_i[i] == hi_i[j] - lo_i[j] >= q)
    assert between * plane > budget and len(set(lo_i) | set(hi_i)) * plane < budget, between
    with engine(p, "mfma", pairwise_del=pdel, single_image=3) as e:
        e.set_option("win_plan", 2)
        s0, c0 = e.run_windows_job_var(lo, hi, maps, off, q, n_rep=n_rep)
        assert e.windows_info()["batches"] == 2  # (without a budget: one batch for the matrices 0, one for the replicates)
        e.set_option("win_max_bytes", budget)
        s, c = check(e, lo, hi, maps, off, q, n_rep, ref, plans=(2,))
        info = e.windows_info()
        print("budgeted: %r" % info)
        assert info["batches"] >= 1 + 3  # matrix 0's one batch + the unit slab's
        diff = rel_err(s, s0)
        print("batched against unbatched: max rel diff %.3g, %d of %d cells differ" % (diff, (s != s0).sum(), s.size))
        assert np.array_equal(c, c0)
        assert np.array_equal(s.view(np.uint64), s0.view(np.uint64)), "the batched call must give the bits of the unbatched call"
        sw, cw = e.run_windows(lo, hi)
        assert e.windows_info()["batches"] == 1 and np.array_equal(s[:, 0].view(np.uint64), sw.view(np.uint64))
        e.set_option("win_max_bytes", 1)  # no window fits: the slab alone cannot run, auto takes the per-window plan
        with pytest.raises(N().NgdError) as ei:
            e.run_windows_job_var(lo, hi, maps, off, q, n_rep=n_rep)
        assert ei.value.code == -4
        check(e, lo, hi, maps, off, q, n_rep, ref, plans=(0,))
        assert e.windows_info()["windows_by_pass"] == len(lo)


@pytest.mark.parametrize("kernel,kw,indep,pdel", [("mfma", {"single_image": 3}, True, False), ("mfma", {"single_image": 3}, True, True),
                                                  ("mfma", {"single_image": 2}, True, False), ("mfma", {"single_image": 2}, True, True),
                                                  ("em_table", {}, False, False), ("stream", {}, True, False)],
                         ids=["two-images", "two-images-pdel", "congruent", "congruent-pdel", "em_table", "stream"])
def test_equal_length_windows_give_run_windows_job_bits(kernel, kw, indep, pdel):
    q, n_rep = 7, 40
    p = O.synth_indmajor(7, 40, N_SITES, miss_frac=0.2 if pdel else 0.0)
    lo, hi = N().window_ranges(N_SITES, 200, 60)
    maps, off = N().window_boot_maps(11, lo, hi, n_rep, q)
    assert len(maps) == n_rep * (200 // q) and not off.any()
    with engine(p, kernel, pairwise_del=pdel, indep_geno=indep, **kw) as e:
        for plan in (1, 2) if kernel != "stream" else (1,):
            e.set_option("win_plan", plan)
            s0, c0 = e.run_windows_job(lo, hi, maps.reshape(n_rep, 200 // q), q)
            i0 = e.windows_info()
            s, c = e.run_windows_job_var(lo, hi, maps, off, q)  # (n_rep read off the layout)
            i1 = e.windows_info()
            assert np.array_equal(s.view(np.uint64), s0.view(np.uint64)) and np.array_equal(c, c0), "plan %d" % plan
            assert {k: v for k, v in i0.items() if k != "ms"} == {k: v for k, v in i1.items() if k != "ms"}


def test_the_launch_is_split_where_grid_y_ends():
    """70 000 windows of one replicate each: more than grid.y holds, so k_reduce_band_wv runs as two launches whose
    descriptors, rows of block starts and outputs continue where the first ended."""
    n_ind, q = 6, 7
    p = O.synth_indmajor(7, n_ind, N_SITES)
    # (lengths 37, 92, 11, 5 -- no block -- and 107; apart from each other, so that a range has the same slices alone)
    ranges = [(3, 40), (50, 142), (150, 161), (200, 205), (400, 507)]
    pick = np.sort(np.random.default_rng(1).integers(0, len(ranges), 70_000))
    assert len(set(pick.tolist())) == 5
    lo = np.array([ranges[k][0] for k in pick], dtype=np.uint64)
    hi = np.array([ranges[k][1] for k in pick], dtype=np.uint64)
    assert np.all(np.diff(lo.astype(np.int64)) >= 0)
    maps, off = N().window_boot_maps(4, lo, hi, 1, q)
    with engine(p, "mfma", single_image=3) as e:
        e.set_option("win_plan", 2)
        s, c = e.run_windows_job_var(lo, hi, maps, off, q, n_rep=1)
        assert e.windows_info()["windows_by_pass"] == 0
        for k, (a, b) in enumerate(ranges):
            l1, h1 = np.array([a], dtype=np.uint64), np.array([b], dtype=np.uint64)
            m1, o1 = N().window_boot_maps(4, l1, h1, 1, q)
            s1, c1 = e.run_windows_job_var(l1, h1, m1, o1, q, n_rep=1)
            sel = pick == k
            assert sel.sum() > 10_000
            assert np.array_equal(c[sel], np.broadcast_to(c1, c[sel].shape)), "range %d" % k
            assert np.array_equal(s[sel].view(np.uint64), np.broadcast_to(s1, s[sel].shape).view(np.uint64)), "range %d" % k


def test_misuse_is_refused_and_the_engine_works_afterwards():
    q, n_rep = 7, 5
    p, lo, hi, wmaps, ref = synth_case(7, 6, 0.0, q, 11, False, True)
    maps, off = engine_maps(11, lo, hi, n_rep, q, wmaps)
    with engine(p, "mfma", single_image=3) as e:
        def refused(lo_=lo, hi_=hi, maps_=maps, off_=off, q_=q, n_rep_=n_rep, code=-1):
            with pytest.raises(N().NgdError) as ei:
                e.run_windows_job_var(lo_, hi_, maps_, off_, q_, n_rep=n_rep_)
            assert ei.value.code == code, str(ei.value)
            return str(ei.value)

        assert "block size 0" in refused(q_=0)
        assert "no windows" in refused(lo_=lo[:0], hi_=hi[:0], off_=off[:0])
        assert "reaches past" in refused(hi_=np.where(np.arange(len(hi)) == 48, N_SITES + 1, hi))
        assert "empty" in refused(hi_=np.where(np.arange(len(hi)) == 4, lo, hi))
        assert "must not decrease" in refused(lo_=lo[::-1].copy(), hi_=hi[::-1].copy(), off_=off[::-1].copy())
        assert "maps_len" in refused(maps_=maps[:-1])  # the last class's maps reach one entry past the table
        big = int(np.argmax(hi - lo))
        assert "maps_len" in refused(off_=np.where(np.arange(len(off)) == big, len(maps), off))
        bad = maps.copy()
        bad[int(off[big]) + 2] = int(hi[big] - lo[big]) // q  # == n_blocks_w: one past the last block
        assert "out of range" in refused(maps_=bad)
        import ctypes as C
        from ngsdist_amd import _lib
        L = _lib.load()
        u64p = C.POINTER(C.c_uint64)
        lp, hp, mp = (x.ctypes.data_as(u64p) for x in (lo, hi, maps))
        out = np.empty((len(lo), n_rep + 1, e.n_pairs))
        outc = np.empty(out.shape, dtype=np.uint64)
        dp, cp = out.ctypes.data_as(C.POINTER(C.c_double)), outc.ctypes.data_as(u64p)
        assert L.ngd_run_windows_job_var(e._h, lp, hp, len(lo), mp, len(maps), None, n_rep, q, dp, cp) == -1   # null offsets
        assert L.ngd_run_windows_job_var(e._h, lp, hp, len(lo), None, 0, off.ctypes.data_as(u64p), n_rep, q, dp, cp) == -1  # null maps
        assert L.ngd_run_windows_job_var(None, lp, hp, len(lo), mp, len(maps), off.ctypes.data_as(u64p), n_rep, q, dp, cp) == -1
        assert L.ngd_run_windows_job_var_dist(e._h, lp, hp, len(lo), mp, len(maps), off.ctypes.data_as(u64p), n_rep, q, 0, 3, dp) == -5
        assert L.ngd_run_windows_job_var_device(e._h, lp, hp, len(lo), mp, len(maps), off.ctypes.data_as(u64p), n_rep, q, None, None) == -1
        # ... and n_rep = 0 is run_windows(), bit for bit; then the job itself
        s0, c0 = e.run_windows_job_var(lo, hi, maps[:0], off, q, n_rep=0)
        sw, cw = e.run_windows(lo, hi)
        assert np.array_equal(s0[:, 0].view(np.uint64), sw.view(np.uint64)) and np.array_equal(c0[:, 0], cw)
        check(e, lo, hi, maps, off, q, n_rep, ref, plans=(0,))
    # NGD_OPT_EM_EXACT: refused in the words of every call the option does not serve, with or without NGD_OPT_EM_EXACT_WIN
    pe = O.synth_indmajor(7, 6, N_SITES)
    with engine(pe, "em_table", indep_geno=False) as e:
        for value, win in ((1, 0), (2, 0), (2, 1), (1, 1)):
            e.set_option("em_exact", 0)
            e.set_option("em_exact_win", 0)
            e.set_option("em_exact", value)
            e.set_option("em_exact_win", win)
            with pytest.raises(N().NgdError) as ei:
                e.run_windows_job_var(lo, hi, maps, off, q, n_rep=n_rep)
            assert ei.value.code == -1 and "NGD_OPT_EM_EXACT is on" in str(ei.value) and "is not served" in str(ei.value)
        e.set_option("em_exact_win", 0)
        e.set_option("em_exact", 0)
        s, _ = e.run_windows_job_var(lo, hi, maps, off, q, n_rep=n_rep)
        assert np.all(np.isfinite(s))


def test_the_dist_form_is_finish_on_every_matrix():
    q, n_rep = 20, 5
    p, lo, hi, wmaps, ref = synth_case(7, 6, 0.0, q, 11, False, True)
    maps, off = engine_maps(11, lo, hi, n_rep, q, wmaps)
    with engine(p, "mfma", single_image=3) as e:
        s, c = e.run_windows_job_var(lo, hi, maps, off, q, n_rep=n_rep)
        with np.errstate(all="ignore"):
            d = e.run_windows_job_var_dist(lo, hi, maps, off, q, evol_model=2, n_rep=n_rep)
            want = N().finish(s.reshape(-1), c.reshape(-1), 0, 2).reshape(s.shape)
        assert np.array_equal(d.view(np.uint64), want.view(np.uint64))
        short = (hi - lo) < q
        assert short.sum() == 29 and np.isnan(d[short, 1:]).all() and np.isfinite(d[short, 0]).all()  # 0 / 0 where no block
