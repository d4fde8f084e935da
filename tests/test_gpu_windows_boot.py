"""Bootstrap replicates inside windows (ngd_run_windows_job*, --win_boot_rep): every matrix of every window against the CPU
oracle run on the window's sites with the window's block map, through both plans (the unit slab, one job per window), every
kernel, the engine ABI and the C++ host.

The expected value for (window w, replicate r) is the oracle over site_src = lo[w] + boot_site_src(map[r], q) with the maps
of a generator seeded once (every run on a cut-down file seeds it anew: windows of one length draw the same maps)."""
import functools
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

RTOL = 1e-9      # against the oracle: the suite's figure
RTOL_SELF = 1e-12  # between plans of the engine that differ in the order of additions (include/ngsdist_amd.h)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "ngsdist_amd", "bin", "ngsDist")


def N():
    import ngsdist_amd
    return ngsdist_amd


def rel_err(a, b):
    a, b = np.asarray(a), np.asarray(b)
    den = np.where(b == 0, 1.0, np.abs(b))
    return float(np.max(np.abs(a - b) / den)) if a.size else 0.0


def draw_maps(seed, n_rep, n_blocks):
    t = O.Taus(seed)
    return np.stack([t.block_map(n_blocks) for _ in range(n_rep)]) if n_rep else np.zeros((0, n_blocks), dtype=np.uint64)


def oracle_job(p, lo, hi, maps, q, pairwise_del=False, indep_geno=True):
    """-> (sums, counts) [n_win][n_rep + 1][n_pairs]"""
    S, Cn = [], []
    for a, b in zip(lo, hi):
        srcs = [np.arange(a, b)] + [int(a) + O.boot_site_src(m, q) for m in maps]
        out = [O.all_pairs(p, pairwise_del=pairwise_del, indep_geno=indep_geno, site_src=src, n_threads=8) for src in srcs]
        S.append(np.stack([s for s, _ in out]))
        Cn.append(np.stack([c for _, c in out]))
    return np.stack(S), np.stack(Cn)


@functools.lru_cache(maxsize=None)
def synth_case(seed, n_ind, n_sites, miss_frac, size, step, q, n_rep, map_seed, pairwise_del, indep_geno):
    p = O.synth_indmajor(seed, n_ind, n_sites, miss_frac=miss_frac)
    lo, hi = N().window_ranges(n_sites, size, step)
    maps = draw_maps(map_seed, n_rep, size // q)
    return p, lo, hi, maps, oracle_job(p, lo, hi, maps, q, pairwise_del, indep_geno)


def engine(p, kernel, pairwise_del=False, indep_geno=True, **kw):
    n_ind, n_sites, _ = p.shape
    e = N().Engine(n_ind, n_sites, pairwise_del=pairwise_del, indep_geno=indep_geno, kernel=kernel, **kw)
    e.upload_ind_major(p).commit()
    return e


def check(e, lo, hi, maps, q, ref, plans, exact=False, nan_ok=False):
    so, co = ref
    for plan in plans:
        e.set_option("win_plan", plan)
        s, c = e.run_windows_job(lo, hi, maps, q)
        assert s.shape == (len(lo), len(maps) + 1, e.n_pairs) and c.shape == s.shape
        assert np.array_equal(c, co), "plan %d: counts" % plan
        if exact:
            assert np.array_equal(s, so), "plan %d: called genotypes must be bit-exact" % plan
        ok = np.isfinite(so) if nan_ok else np.ones(so.shape, dtype=bool)
        if nan_ok:
            assert np.array_equal(np.isnan(s), np.isnan(so)), "plan %d: non-finite terms in the wrong matrices" % plan
        err = rel_err(s[ok], so[ok])
        print("plan %d q %d R %d: max rel err %.3g" % (plan, q, len(maps), err))
        assert err < RTOL, "plan %d" % plan
        info = e.windows_info()
        if plan == 1:
            assert info["windows_by_pass"] == len(lo) and info["segments"] == 0 and info["batches"] == 0
        if plan == 2:
            assert info["windows_by_pass"] == 0 and info["batches"] >= 1 and info["segments"] >= 1


KERNELS = [("mfma", {"single_image": 3}), ("mfma", {"single_image": 2}), ("stream", {})]


@pytest.mark.parametrize("kernel,kw", KERNELS)
@pytest.mark.parametrize("n_ind", [6, 40, 130])
@pytest.mark.parametrize("q", [1, 7, 20, 60])
@pytest.mark.parametrize("n_rep", [5, 40])
def test_indep_jobs_against_the_oracle(kernel, kw, n_ind, q, n_rep):
    p, lo, hi, maps, ref = synth_case(7, n_ind, 777, 0.0, 200, 60, q, n_rep, 11, False, True)
    assert len(lo) == 10 and (200 % q == 4) == (q == 7)
    with engine(p, kernel, **kw) as e:
        check(e, lo, hi, maps, q, ref, plans=(0, 1, 2) if kernel == "mfma" else (0, 1))
        if kernel == "stream":
            e.set_option("win_plan", 2)
            with pytest.raises(N().NgdError) as ei:
                e.run_windows_job(lo, hi, maps, q)
            assert ei.value.code == -1


@pytest.mark.parametrize("kernel,kw", KERNELS)
@pytest.mark.parametrize("q", [7, 20])
def test_pairwise_del_jobs(kernel, kw, q):
    p, lo, hi, maps, ref = synth_case(5, 40, 777, 0.2, 200, 60, q, 5, 3, True, True)
    assert ref[1][:, 1:].min() < (200 // q) * q  # some replicate count is below n_blocks q
    with engine(p, kernel, pairwise_del=True, **kw) as e:
        check(e, lo, hi, maps, q, ref, plans=(0, 1, 2) if kernel == "mfma" else (0, 1))


@pytest.mark.parametrize("single_image", [2, 3])
def test_called_genotypes_bit_exact(single_image):
    rng = np.random.default_rng(1)
    n_ind, n_sites = 24, 900
    g = rng.integers(0, 3, size=(n_ind, n_sites))
    p = np.zeros((n_ind, n_sites, 3))
    np.put_along_axis(p, g[..., None], 1.0, axis=2)
    lo, hi = N().window_ranges(n_sites, 300, 110)
    for q in (7, 10):
        maps = draw_maps(2, 6, 300 // q)
        ref = oracle_job(p, lo, hi, maps, q)
        with engine(p, "mfma", single_image=single_image) as e:
            check(e, lo, hi, maps, q, ref, plans=(0, 1, 2), exact=True)
            # exact arithmetic: matrix 0 carries run_windows()' bits whatever the slices
            e.set_option("win_plan", 2)
            assert np.array_equal(e.run_windows_job(lo, hi, maps, q)[0][:, 0], e.run_windows(lo, hi)[0])


@pytest.mark.parametrize("kernel,plans", [("em_table", (0, 1, 2)), ("em_fast", (0, 1)), ("em_faithful", (0, 1))])
@pytest.mark.parametrize("q", [1, 7, 20])
def test_em_jobs_with_an_all_zero_individual(kernel, plans, q):
    """An all-zero individual at one site gives 0/0 as on the CPU: NaN for that individual's pairs in exactly the matrices that
    visit the site -- matrix 0 of the windows that hold it, and the replicates that draw its block."""
    n_ind, n_sites, size = 20, 300, 100
    p = O.synth_indmajor(11, n_ind, n_sites, miss_frac=0.05)
    p[3, 130] = 0
    lo, hi = N().window_ranges(n_sites, size, 40)
    maps = draw_maps(9, 5, size // q)
    so, co = oracle_job(p, lo, hi, maps, q, indep_geno=False)
    nans = np.isnan(so).any(axis=2)  # [window][matrix]
    holds = (lo <= 130) & (130 < hi)
    assert np.array_equal(nans[:, 0], holds) and nans[:, 1:].any() and not nans[holds, 1:].all()
    with engine(p, kernel, indep_geno=False) as e:
        check(e, lo, hi, maps, q, (so, co), plans=plans, nan_ok=True)


def clones(seed, n_ind, n_sites, members, miss_frac=0.0):
    """clusters of nearly identical individuals (confident, equal genotypes everywhere) among ordinary ones"""
    rng = np.random.default_rng(seed)
    p = O.synth_indmajor(seed, n_ind, n_sites, miss_frac=miss_frac)
    g = rng.integers(0, 3, size=n_sites)
    for k in members:
        x = 1e-12 * (1 + rng.random((n_sites, 3)))
        x[np.arange(n_sites), g] = 0
        x[np.arange(n_sites), g] = 1 - x.sum(axis=1)
        p[k] = x
    return p


@pytest.mark.parametrize("pairwise_del", [False, True])
@pytest.mark.parametrize("q", [20, 7])
@pytest.mark.parametrize("n_ind,kw", [(40, {"single_image": 2, "exact_shapes": 1}), (400, {})])
def test_clones_on_a_one_image_engine_are_fixed_in_every_matrix(pairwise_del, q, n_ind, kw):
    n_sites, size, step = 777, 200, 60
    members = list(range(5, 17)) + [30, 31]
    p = clones(3, n_ind, n_sites, members, miss_frac=0.2 if pairwise_del else 0.0)
    lo, hi = N().window_ranges(n_sites, size, step)
    maps = draw_maps(4, 5, size // q)
    so, co = oracle_job(p, lo, hi, maps, q, pairwise_del=pairwise_del)
    # the oracle itself shows sums below the noting threshold (1e-6 x the sites visited) in every matrix
    assert np.all(((so < 1e-6 * co) & (co > 0)).sum(axis=2) >= 12 * 11 // 2 + 1)
    with engine(p, "mfma", pairwise_del=pairwise_del, **kw) as e:
        assert e.image_mode() == (2, True)
        for plan in (2, 1, 0):
            check(e, lo, hi, maps, q, (so, co), plans=(plan,))
            fx = e.fixup()
            print("plan %d: fixup %r" % (plan, fx))
            assert fx["recomputed"] > 0 and fx["skipped"] == 0, "plan %d recomputed nothing" % plan
            assert e.windows_info()["fixup_pairs"] > 0


@pytest.mark.parametrize("kernel,kw,indep,pdel", [("mfma", {"single_image": 3}, True, False), ("mfma", {"single_image": 3}, True, True),
                                                  ("mfma", {"single_image": 2}, True, False), ("em_table", {}, False, False)])
@pytest.mark.parametrize("q", [7, 20, 300])
def test_jobs_agree_with_run_job_on_an_engine_of_the_window_alone(kernel, kw, indep, pdel, q):
    n_ind, n_sites, size = 40, 600, 200
    p = O.synth_indmajor(13, n_ind, n_sites, miss_frac=0.1 if pdel else 0.0)
    lo, hi = N().window_ranges(n_sites, size, 90)
    maps = draw_maps(6, 5, size // q)
    with engine(p, kernel, pairwise_del=pdel, indep_geno=indep, **kw) as e:
        for w, (a, b) in enumerate(zip(lo, hi)):
            with engine(np.ascontiguousarray(p[:, a:b]), kernel, pairwise_del=pdel, indep_geno=indep, **kw) as ew:
                if q > size:  # W < q: no block -- whatever run_job() does on the window's own engine, here too
                    with pytest.raises(N().NgdError) as e1:
                        ew.run_job(maps, q)
                    with pytest.raises(N().NgdError) as e2:
                        e.run_windows_job(lo, hi, maps, q)
                    assert e1.value.code == e2.value.code == -1
                    continue
                sw, cw = ew.run_job(maps, q)
            for plan in (2, 1):
                e.set_option("win_plan", plan)
                s, c = e.run_windows_job(lo[w:w + 1], hi[w:w + 1], maps, q)
                assert np.array_equal(c[0], cw)
                assert rel_err(s[0], sw) < RTOL_SELF, "plan %d window %d" % (plan, w)
        if q <= size:  # ... and the engine is as usable as before
            e.set_option("win_plan", 0)
            s, _ = e.run_windows_job(lo, hi, maps, q)
            assert np.all(np.isfinite(s))


BAND_ENGINES = [("mfma", {"single_image": 3}, 40, True), ("mfma", {"single_image": 2, "exact_shapes": 1}, 40, True),
                ("em_table", {}, 12, False)]


@pytest.mark.parametrize("kernel,kw,n_ind,indep", BAND_ENGINES, ids=["two-images", "congruent", "em_table"])
@pytest.mark.parametrize("pdel", [False, True])
@pytest.mark.parametrize("q", [4, 7])
@pytest.mark.parametrize("n_rep", [1, 2, 4, 16, 17, 32, 64, 65])
def test_every_group_size_of_the_band_reduction(kernel, kw, n_ind, indep, pdel, q, n_rep):
    """k_reduce_band_w<RB, CNT> (reduce.hip): RB = ngd_reduce_chunk(n_rep) = 1, 4, 16 or 32 replicates per group, with counts
    (--pairwise_del) and without -- one replicate, a full group of 4, 16 and 32, one more than a group (17, 65), two groups
    of 32.  240 sites, windows of 80 every 40; q = 4 divides the step (a block is one slice of the slab), q = 7 does not.
    The slab plan forced and read back; every matrix of every window against the oracle on the window's sites with the
    window's map, counts exact; matrix 0 the bits of run_windows()."""
    p, lo, hi, maps, (so, co) = synth_case(29, n_ind, 240, 0.2 if pdel else 0.0, 80, 40, q, 65, 13, pdel, indep)
    assert len(lo) == 5 and maps.shape == (65, 80 // q)
    maps, so, co = maps[:n_rep], so[:, :n_rep + 1], co[:, :n_rep + 1]  # (a generator draws map after map: a prefix)
    with engine(p, kernel, pairwise_del=pdel, indep_geno=indep, **kw) as e:
        e.set_option("win_plan", 2)
        s, c = e.run_windows_job(lo, hi, maps, q)
        info = e.windows_info()
        assert info["windows_by_pass"] == 0 and info["batches"] >= 1 and info["segments"] >= 1, info
        s0, c0 = e.run_windows(lo, hi)
        assert e.windows_info()["windows_by_pass"] == 0
    assert s.shape == (5, n_rep + 1, e.n_pairs) and c.shape == s.shape
    assert np.array_equal(c, co)
    assert np.all(np.isfinite(s))
    for w in range(5):
        for m in range(n_rep + 1):  # every matrix of every window
            err = rel_err(s[w, m], so[w, m])
            assert err < RTOL, (w, m, err)
    assert np.array_equal(c[:, 0], c0)
    assert np.array_equal(s[:, 0].view(np.uint64), s0.view(np.uint64))


def test_matrix_0_and_no_replicates_are_run_windows_bit_for_bit():
    """Under the slab plan matrix 0 of every window is run_windows()' matrix under the slab plan, bit for bit, whatever the
    block size: it is reduced from the windows' own segments, not from the replicates' finer slices (whose additions come in
    another order).  One-image engines included, clones and their fix-up included.  n_rep = 0 IS run_windows(), any plan."""
    n_ind, n_sites = 40, 777
    lo, hi = N().window_ranges(n_sites, 200, 60)
    cases = (("mfma", {"single_image": 3}, True, False, O.synth_indmajor(7, n_ind, n_sites)),
             ("mfma", {"single_image": 3}, True, True, O.synth_indmajor(7, n_ind, n_sites, miss_frac=0.2)),
             ("mfma", {"single_image": 2, "exact_shapes": 1}, True, False, clones(3, n_ind, n_sites, list(range(5, 17)))),
             ("mfma", {"single_image": 2, "exact_shapes": 1}, True, True, clones(3, n_ind, n_sites, list(range(5, 17)), 0.2)),
             ("em_table", {}, False, False, O.synth_indmajor(7, n_ind, n_sites)))
    for kernel, kw, indep, pdel, p in cases:
        with engine(p, kernel, indep_geno=indep, pairwise_del=pdel, **kw) as e:
            e.set_option("win_plan", 2)
            s0, c0 = e.run_windows(lo, hi)
            for q in (1, 7, 20, 60):
                s, c = e.run_windows_job(lo, hi, draw_maps(1, 5, 200 // q), q)
                assert e.windows_info()["windows_by_pass"] == 0
                assert np.array_equal(c[:, 0], c0), (kernel, kw, q)
                assert np.array_equal(s[:, 0].view(np.uint64), s0.view(np.uint64)), (kernel, kw, pdel, q)
            for plan in (0, 1, 2):  # n_rep = 0 is run_windows(), whatever the plan
                e.set_option("win_plan", plan)
                s0, c0 = e.run_windows(lo, hi)
                for maps in (None, np.zeros((0, 10), dtype=np.uint64)):
                    s, c = e.run_windows_job(lo, hi, maps, 20)
                    assert s.shape == (len(lo), 1, e.n_pairs)
                    assert np.array_equal(s[:, 0], s0) and np.array_equal(c[:, 0], c0)


@pytest.mark.parametrize("pdel", [False, True])
def test_a_budget_that_forces_several_batches(pdel):
    q, n_rep = 7, 40
    p, lo, hi, maps, ref = synth_case(5, 40, 777, 0.2 if pdel else 0.0, 200, 60, q, n_rep, 3, pdel, True)
    with engine(p, "mfma", pairwise_del=pdel, single_image=3) as e:
        e.set_option("win_plan", 2)
        e.run_windows_job(lo, hi, maps, q)
        assert e.windows_info()["batches"] == 2  # (without a budget: one batch for the matrices 0, one for the replicates)
        e.set_option("win_max_bytes", 80 * 128 * 128 * (12 if pdel else 8) + (1 << 20))  # ~ two windows' slices
        check(e, lo, hi, maps, q, ref, plans=(2,))
        info = e.windows_info()
        print("budgeted: %r" % info)
        assert info["batches"] > 2 and info["batches"] > 1
        e.set_option("win_max_bytes", 1)  # no window fits: the slab alone cannot run, auto takes the per-window plan
        with pytest.raises(N().NgdError) as ei:
            e.run_windows_job(lo, hi, maps, q)
        assert ei.value.code == -4
        check(e, lo, hi, maps, q, ref, plans=(0,))
        assert e.windows_info()["windows_by_pass"] == len(lo)


def test_misuse_is_refused_and_holds_no_memory():
    p = O.synth_indmajor(3, 20, 500)
    with engine(p, "mfma") as e:
        lo, hi = np.array([0, 100, 250]), np.array([200, 300, 450])
        maps = draw_maps(1, 3, 10)
        s, c = e.run_windows_job(lo, hi, maps, 20)
        before = e.device_bytes()
        big = maps.copy()
        big[2, 9] = 10
        bad = [
            (lo, np.array([200, 300, 451]), maps, 20),   # windows of unequal length
            (lo, hi, maps, 0),                           # block size 0
            (lo, hi, maps, 21),                          # n_blocks != W / block_size (200 // 21 = 9, the maps have 10)
            (lo, hi, maps[:, :9], 20),
            (lo, hi, big, 20),                           # a map entry >= n_blocks
            (lo, hi, draw_maps(1, 3, 0), 201),           # W < q: no block (run_job's "empty bootstrap geometry")
            ([0], [501], maps, 20), ([5], [5], maps, 20), ([10, 9], [210, 209], maps, 20), ([], [], maps, 20),  # run_windows' refusals
        ]
        for k in range(2 * len(bad)):
            a, b, m, q = bad[k % len(bad)]
            with pytest.raises(N().NgdError) as ei:
                e.run_windows_job(a, b, m, q)
            assert ei.value.code == -1, k
            with pytest.raises(N().NgdError) as ei:
                e.run_windows_job_dist(a, b, m, q)
            assert ei.value.code == -1, k
        L, C = N().engine._lib.load(), N().engine.C
        lp, hp = [x.astype(np.uint64) for x in (lo, hi)]
        u64p = C.POINTER(C.c_uint64)
        out = np.zeros(3 * 4 * e.n_pairs)
        rc = L.ngd_run_windows_job_dist(e._h, lp.ctypes.data_as(u64p), hp.ctypes.data_as(u64p), 3, None, 3, 10, 20, 0, 1,
                                        out.ctypes.data_as(C.POINTER(C.c_double)))
        assert rc == -1  # null maps with n_rep > 0
        with pytest.raises(N().NgdError) as ei:
            e.run_windows_job_dist(lo, hi, maps, 20, evol_model=3)
        assert ei.value.code == -5
        assert e.device_bytes() == before
        s2, c2 = e.run_windows_job(lo, hi, maps, 20)  # ... and the engine is as usable as before
        assert np.array_equal(s2, s) and np.array_equal(c2, c)
    with engine(p, "mfma", pairwise_del=True) as e:
        with pytest.raises(N().NgdError) as ei:
            e.run_windows_job_dist(lo, hi, maps, 20, tot_sites=1000)
        assert ei.value.code == -1
    with N().Engine(20, 500, kernel="mfma", shard_rank=0, shard_world=2) as e:
        e.upload_ind_major(p).commit()
        with pytest.raises(N().NgdError) as ei:
            e.run_windows_job(lo, hi, maps, 20)
        assert ei.value.code == -1


def test_job_dist_is_finish_of_the_job_and_the_device_form_agrees():
    import torch
    p = O.synth_indmajor(21, 30, 900)
    lo, hi = N().window_ranges(900, 300, 150)
    maps = draw_maps(8, 4, 30)
    with engine(p, "mfma") as e:
        s, c = e.run_windows_job(lo, hi, maps, 10)
        for model in (0, 1, 2):
            d = e.run_windows_job_dist(lo, hi, maps, 10, evol_model=model)
            want = N().finish(s.reshape(-1), c.reshape(-1), 0, model).reshape(s.shape)
            assert np.array_equal(d.view(np.uint64), want.view(np.uint64))
        d = e.run_windows_job_dist(lo, hi, maps, 10, evol_model=0, tot_sites=1000)
        assert np.array_equal(d, s / 1000.0)
        ds = torch.zeros(s.shape, dtype=torch.float64, device="cuda")
        dc = torch.zeros(s.shape, dtype=torch.int64, device="cuda")
        assert e.run_windows_job(lo, hi, maps, 10, d_sum_ptr=ds.data_ptr(), d_cnt_ptr=dc.data_ptr()) is None
        torch.cuda.synchronize()
        assert np.array_equal(ds.cpu().numpy(), s) and np.array_equal(dc.cpu().numpy().astype(np.uint64), c)


def test_the_default_engine_at_a_few_hundred_individuals():
    """the host's default engine above 384 padded individuals is one-image: auto plan, whatever it picks, against the oracle"""
    n_ind, n_sites, q = 400, 1200, 25
    p = O.synth_indmajor(19, n_ind, n_sites)
    lo, hi = N().window_ranges(n_sites, 400, 200)
    maps = draw_maps(2, 33, 400 // q)
    ref = oracle_job(p, lo, hi, maps, q)
    with engine(p, "mfma") as e:
        assert e.image_mode()[0] == 2
        check(e, lo, hi, maps, q, ref, plans=(0, 2))


# ---- the C++ host ----

def run_cli(tmp_path, args, name="w.dist", ok=True):
    out = str(tmp_path / name)
    r = subprocess.run([BIN] + [str(a) for a in args] + ["--out", out, "--verbose", "0"], capture_output=True, timeout=600)
    assert (r.returncode == 0) == ok, r.stderr.decode()
    return out, r


def split_blocks(text):
    assert text.startswith("\n")
    return text[1:].split("\n\n")


def cells(block):
    lines = [l for l in block.split("\n") if l]
    return np.array([[float(x) for x in l.split("\t")[1:]] for l in lines[1:]])


@pytest.mark.parametrize("mode", ["call_geno", "gl", "em"])
def test_cli_window_replicates_match_runs_on_the_cut_down_files(tmp_path, mode):
    n_ind, n_sites, R = 12, 600, 3
    rng = np.random.default_rng(8)
    raw = rng.dirichlet([0.6, 0.6, 0.6], size=(n_sites, n_ind))
    raw.tofile(str(tmp_path / "g.bin"))
    chrom = ["chrA"] * 250 + ["chrB"] * 300 + ["chrC"] * 50
    pos = str(tmp_path / "p.tsv")
    with open(pos, "w") as fh:
        fh.write("chr\tpos\n")
        for s in range(n_sites):
            fh.write("%s\t%d\n" % (chrom[s], 1000 + 7 * s))
    flags = {"call_geno": ["--probs", "--call_geno", "--indep_geno"], "gl": ["--probs", "--indep_geno"],
             "em": ["--probs"]}[mode]
    base = ["--n_ind", n_ind] + flags + ["--evol_model", 1]
    boot = ["--boot_block_size", 10, "--seed", 5]
    for with_pos in (False, True):
        extra = ["--posH", pos] if with_pos else []
        out, _ = run_cli(tmp_path, ["--geno", tmp_path / "g.bin", "--n_sites", n_sites, "--win_size", 100, "--win_step", 60,
                                    "--win_boot_rep", R] + boot + extra + base)
        lo, hi = N().window_ranges(n_sites, 100, 60, chrom=chrom if with_pos else None)
        got = split_blocks(open(out).read())
        assert len(got) == len(lo) * (R + 1)
        win = open(out + ".windows").read().strip().split("\n")
        assert win[0] == "window\tchr\tstart\tend\tfirst_site\tn_sites" and len(win) == len(lo) + 1
        for w, line in enumerate(win[1:]):
            f = line.split("\t")
            if with_pos:
                assert f == [str(w), chrom[lo[w]], str(1000 + 7 * lo[w]), str(1000 + 7 * (hi[w] - 1)), str(lo[w]), "100"]
            else:
                assert f == [str(w), ".", str(lo[w] + 1), str(hi[w]), str(lo[w]), "100"]
        for w in range(len(lo)):
            raw[lo[w]:hi[w]].tofile(str(tmp_path / "c.bin"))
            ref, _ = run_cli(tmp_path, ["--geno", tmp_path / "c.bin", "--n_sites", hi[w] - lo[w], "--n_boot_rep", R] + boot + base,
                             name="c.dist")
            want = split_blocks(open(ref).read())
            assert len(want) == R + 1
            for m in range(R + 1):
                a, b = got[w * (R + 1) + m], want[m]
                if mode == "call_geno":
                    assert a.rstrip("\n") == b.rstrip("\n")  # (the last block of a file ends with its newline)
                else:
                    assert np.allclose(cells(a), cells(b), rtol=1e-9, atol=2e-10)
