"""Windows along the genome on the paths and shapes test_gpu_windows.py leaves out: one-image engines with --pairwise_del,
a fix-up list that overflows, results written to a caller's device buffers, output groups, more windows than one banded
reduction launch holds, the MFMA block forms, budget batches with count planes, the per-window plan on the other engines,
windows straight after a staged load and the C++ host on a one-image engine.  Every window against the CPU oracle run on
that window's sites alone: counts exact, sums to 1e-9 relative, called genotypes bit for bit."""
import numpy as np
import pytest

from oracle import oracle as O
from test_gpu_parity import _raw_gl, clones
from test_gpu_windows import RTOL, blocks, check, engine, mixed_windows, N, oracle_windows, rel_err, run_cli, split_blocks

pytestmark = pytest.mark.gpu


def many_windows(n_sites, size, step):
    """mixed_windows plus a sliding run, ordered by start: groups of 16 windows of very different extents"""
    lo, hi = mixed_windows(n_sites)
    slo, shi = N().window_ranges(n_sites, size, step)
    lo, hi = np.concatenate([lo, slo.astype(np.int64)]), np.concatenate([hi, shi.astype(np.int64)])
    order = np.argsort(lo, kind="stable")
    assert len(lo) > 16
    return lo[order], hi[order]


def n_pad(n_ind):
    return (n_ind + 127) // 128 * 128


def pair_index(n_ind, i, j):
    return N().engine._lib.load().ngd_pair_index(n_ind, i, j)


def sampled_rows(seed, n_ind, n_sites, inds):
    """rows of O.synth_indmajor(seed, n_ind, n_sites) (what Engine.synth_fill(seed) holds) for a few individuals"""
    return np.concatenate([O.synth_indmajor(seed, n_ind, n_sites, i0=i, n_sub=1) for i in inds])


def check_sampled(s, c, rows, inds, n_ind, lo, hi, windows):
    """the pairs of the sampled individuals in the given windows against the oracle on those rows"""
    idx = np.array([pair_index(n_ind, inds[a], inds[b]) for a in range(len(inds)) for b in range(a + 1, len(inds))])
    for w in windows:
        so, co = O.all_pairs(rows, site_src=np.arange(lo[w], hi[w]))
        assert np.array_equal(c[w][idx], co), w
        assert rel_err(s[w][idx], so) < RTOL, w


def plant_scattered_clones(p, groups, seed):
    """copies of one individual per group: pairs alone in their 16 x 16 tile and a cluster inside one tile"""
    for g in groups:
        p[g] = clones(len(g), p.shape[1], 1e-11, seed=seed + g[0])
    return p


# ---- A: one-image engines (single_image = 0 above 384 padded individuals) under --pairwise_del ----

@pytest.mark.parametrize("pairwise_del", [False, True])
def test_one_image_engine_windows_with_and_without_pairwise_del(pairwise_del):
    """500 individuals: the default engine holds ONE image in congruent coordinates, and every window's nearly identical
    pairs go through the fix-up (engine_windows.hip windows_fixup), under --pairwise_del noted by k_fix_flag from their counts
    across the batch's windows.  One clone of each group misses sites [1000, 1100): under --pairwise_del its pairs' counts
    are not the window's length there, without it those windows hold no nearly identical pair of it."""
    n_ind, n_sites = 500, 3000
    p = O.synth_indmajor(31, n_ind, n_sites, miss_frac=0.1)
    groups = ([0, 17], [40, 290], [41, 291], [400, 401, 402, 403, 404, 170])
    plant_scattered_clones(p, groups, 31)
    for g in groups:
        p[g[0], 1000:1100] = 1.0 / 3
    lo, hi = many_windows(n_sites, 300, 300)
    ref = oracle_windows(p, lo, hi, pairwise_del)
    with engine(p, "mfma", pairwise_del=pairwise_del) as e:
        assert e.image_mode() == (2, True)
        infos = {}
        for plan in (2, 1):
            check(e, p, lo, hi, plans=(plan,), pairwise_del=pairwise_del, ref=ref, infos=infos)
            assert infos[plan]["fixup_pairs"] > 0 and e.fixup()["skipped"] == 0, plan


# ---- B: more noted pairs than the fix list holds ----

@pytest.mark.parametrize("pairwise_del", [False, True])
def test_windows_with_more_noted_pairs_than_the_list_holds(pairwise_del):
    """1500 copies of one individual (1 124 250 pairs, all noted in every window): the list of noted pairs overflows and
    windows_fixup recomputes every pair of the engine in every window of the batch -- one-site and nested windows"""
    n_ind, n_sites = 1500, 48
    p = clones(n_ind, n_sites, 1e-10)
    if pairwise_del:
        miss = np.random.default_rng(3).random((n_ind, n_sites)) < 0.1
        p[miss] = 1.0 / 3
    lo, hi = np.array([0, 0, 3, 3, 10, 20, 47]), np.array([48, 1, 40, 4, 11, 44, 48])
    so, co = oracle_windows(p, lo, hi, pairwise_del)
    n_pairs = N().n_pairs(n_ind)
    with engine(p, "mfma", pairwise_del=pairwise_del) as e:
        assert e.image_mode() == (2, True)
        for plan in (2, 1):
            e.set_option("win_plan", plan)
            s, c = e.run_windows(lo, hi)
            f, info = e.fixup(), e.windows_info()
            assert f["flagged"] > 2 ** 20 and f["skipped"] == 0, plan
            if plan == 2:
                assert info["batches"] == 1 and f["recomputed"] == n_pairs and info["fixup_pairs"] == n_pairs * len(lo)
            assert np.array_equal(c, co), plan
            for w in range(len(lo)):
                ok = co[w] > 0  # (a pair without a valid site in the window: 0 / 0 on both sides)
                assert rel_err(s[w][ok], so[w][ok]) < RTOL, (plan, w)


# ---- C: results in a caller's device buffers (ngd_run_windows_device) ----

@pytest.mark.parametrize("n_ind", [130, 420])
def test_windows_into_device_buffers(n_ind):
    """Every [window][pair] cell written, nothing in the guard rows before and after, and the bits of the host-memory call
    with the same plan, windows and budget (one output group: the same launches).  A budget of a few segments' planes: the
    slab plan runs in batches, each written at its own offset.  130 individuals: two images; 420: one image + fix-up."""
    import torch

    n_sites = 1500
    p = O.synth_indmajor(43, n_ind, n_sites, miss_frac=0.1)
    if n_ind > 384:
        plant_scattered_clones(p, ([3, 200], [300, 301, 302, 303, 304]), 43)
    lo, hi = many_windows(n_sites, 400, 200)
    n_win, n_pairs = len(lo), N().n_pairs(n_ind)
    dev = torch.device("cuda")
    for pairwise_del in (False, True):
        so, co = oracle_windows(p, lo, hi, pairwise_del)
        with engine(p, "mfma", pairwise_del=pairwise_del) as e:
            assert e.image_mode() == ((2, True) if n_ind > 384 else (3, False))
            e.set_option("win_max_bytes", 12 * n_pad(n_ind) ** 2 * 8 + (1 << 20))
            for plan in (2, 1):
                e.set_option("win_plan", plan)
                s, c = e.run_windows(lo, hi)
                host_info = e.windows_info()
                if plan == 2:
                    assert host_info["batches"] >= 2
                assert np.array_equal(c, co) and rel_err(s, so) < RTOL, (pairwise_del, plan)
                ds = torch.full((n_win + 2, n_pairs), float("nan"), dtype=torch.float64, device=dev)
                dc = torch.full((n_win + 2, n_pairs), -1, dtype=torch.int64, device=dev)
                torch.cuda.synchronize()
                assert e.run_windows(lo, hi, d_sum_ptr=ds.data_ptr() + n_pairs * 8, d_cnt_ptr=dc.data_ptr() + n_pairs * 8) is None
                torch.cuda.synchronize()
                assert e.windows_info()["batches"] == host_info["batches"]
                hs, hc = ds.cpu().numpy(), dc.cpu().numpy()
                assert np.all(np.isnan(hs[0])) and np.all(np.isnan(hs[-1])), (pairwise_del, plan)
                assert np.all(hc[0] == -1) and np.all(hc[-1] == -1), (pairwise_del, plan)
                assert not np.isnan(hs[1:-1]).any() and not (hc[1:-1] == -1).any(), (pairwise_del, plan)
                assert np.array_equal(hs[1:-1].view(np.uint64), s.view(np.uint64)), (pairwise_del, plan)
                assert np.array_equal(hc[1:-1].view(np.uint64), c), (pairwise_del, plan)
                del ds, dc


# ---- D: an output group boundary of the host-memory forms ----

def test_windows_across_an_output_group_boundary():
    """1000 individuals, 299 windows of 40 sites every 20: ngd_run_windows returns results in groups of 2 GiB / (16 n_pairs)
    = 268 windows, so windows 268 .. 298 come from a second group.  Holds ~2.4 GB of host memory at its peak (the sums and
    counts of all windows), 1.2 GB for the distances after them."""
    n_ind, n_sites = 1000, 6000
    lo, hi = N().window_ranges(n_sites, 40, 20)
    n_pairs = N().n_pairs(n_ind)
    per = (2 << 30) // (16 * n_pairs)
    assert per == 268 and len(lo) == 299
    ws = [0, per - 2, per - 1, per, per + 1, len(lo) - 1]
    inds = [0, 1, 127, 128, 500, 999]
    rows = sampled_rows(5, n_ind, n_sites, inds)
    with N().Engine(n_ind, n_sites, kernel="mfma") as e:
        e.synth_fill(5, 0.0)
        e.set_option("win_plan", 2)
        s, c = e.run_windows(lo, hi)
        assert e.windows_info()["windows_by_pass"] == 0
        assert np.all(c == (hi - lo)[:, None])
        check_sampled(s, c, rows, inds, n_ind, lo, hi, ws)
        s_w, c_w = s[ws].copy(), c[ws].copy()
        del s, c
        for k, w in enumerate(ws):  # one window alone: the same segments' sums, grouped otherwise (rounding only)
            s1, c1 = e.run_windows(lo[w:w + 1], hi[w:w + 1])
            assert np.array_equal(c1[0], c_w[k]) and rel_err(s_w[k], s1[0]) < 1e-12, w
        d = e.run_windows_dist(lo, hi, evol_model=1)
        d_w = d[ws].copy()
        del d
    want = N().finish(s_w.reshape(-1), c_w.reshape(-1), 0, 1).reshape(s_w.shape)
    assert np.array_equal(d_w.view(np.uint64), want.view(np.uint64))


# ---- E: more windows than one banded reduction launch holds ----

@pytest.mark.parametrize("pairwise_del", [False, True])
def test_more_windows_than_one_band_launch(pairwise_del):
    """600 000 windows that all start at site 0 and end at 1, 37 or 100 in turn: three segments, one batch, and
    ngd_launch_reduce_band split at 16 x 32 768 windows (grid.y), for the sums and, under --pairwise_del, the counts.  Window
    524 288, the first of the second launch, ends at a different site than window 0."""
    n_ind, n_sites, n_win = 3, 100, 600_000
    ends = np.array([1, 37, 100])
    assert (16 * 32768) % 3 != 0
    p = O.synth_indmajor(61, n_ind, n_sites, miss_frac=0.2 if pairwise_del else 0.0)
    lo, hi = np.zeros(n_win, dtype=np.uint64), np.tile(ends, n_win // 3).astype(np.uint64)
    with engine(p, "mfma", pairwise_del=pairwise_del) as e:
        e.set_option("win_plan", 2)
        s, c = e.run_windows(lo, hi)
        info = e.windows_info()
    assert info["segments"] == 3 and info["batches"] == 1
    for k, end in enumerate(ends):
        so, co = O.all_pairs(p, pairwise_del=pairwise_del, site_src=np.arange(end))
        assert np.array_equal(c[k::3], np.broadcast_to(co, c[k::3].shape)), end
        assert rel_err(s[k::3], np.broadcast_to(so, s[k::3].shape)) < RTOL, end


# ---- F: the MFMA block forms with the slice table ----

@pytest.mark.parametrize("n_ind", [64, 200, 256, 383])
def test_windows_on_every_block_form(n_ind):
    """exact_shapes 0 .. 7 (accum_mfma.hip EXACT; forms 3 and 5 are rewritten when a slice table is given), --pairwise_del with
    10 % missing, both plans.  64 and 256 individuals: the last group of 16 holds no zero padding (tools/fuzz_parity.py case
    40501, test_gpu_parity.py test_mfma_exact_block_forms)."""
    n_sites = 1030
    p = O.synth_indmajor(41 + n_ind, n_ind, n_sites, miss_frac=0.1)
    lo, hi = many_windows(n_sites, 300, 100)
    ref = oracle_windows(p, lo, hi, pairwise_del=True)
    for form in range(8):
        with engine(p, "mfma", pairwise_del=True, exact_shapes=form) as e:
            check(e, p, lo, hi, plans=(2, 1), pairwise_del=True, ref=ref)


def test_called_genotype_windows_on_every_block_form():
    """called genotypes (exact arithmetic): every block form's windows bit for bit, 256 individuals"""
    n_ind, n_sites = 256, 1030
    rng = np.random.default_rng(256)
    p = np.zeros((n_ind, n_sites, 3))
    np.put_along_axis(p, rng.integers(0, 3, size=(n_ind, n_sites))[..., None], 1.0, axis=2)
    lo, hi = many_windows(n_sites, 300, 100)
    ref = oracle_windows(p, lo, hi)
    for form in range(8):
        with engine(p, "mfma", exact_shapes=form) as e:
            check(e, p, lo, hi, plans=(2, 1), exact=True, ref=ref)


# ---- G: budget batches under --pairwise_del ----

def test_budget_batches_with_pairwise_del():
    """200 individuals (two 128-tiles), --pairwise_del: a batch also holds a count plane per segment (cnt_boot).  A budget of a
    few segments' planes: at least three batches, the counts of one batch, sums within 1e-12 of it and 1e-9 of the oracle."""
    n_ind, n_sites = 200, 3000
    p = O.synth_indmajor(19, n_ind, n_sites, miss_frac=0.1)
    rng = np.random.default_rng(6)
    lo = np.sort(rng.integers(0, n_sites - 200, size=40))
    hi = lo + rng.integers(1, 200, size=40)
    with engine(p, "mfma", pairwise_del=True) as e:
        so, co = check(e, p, lo, hi, plans=(2,), pairwise_del=True)
        s1, c1 = e.run_windows(lo, hi)
        assert e.windows_info()["batches"] == 1
        e.set_option("win_max_bytes", 12 * n_pad(n_ind) ** 2 * 8 + (1 << 20))
        s2, c2 = e.run_windows(lo, hi)
        assert e.windows_info()["batches"] >= 3
    assert np.array_equal(c1, c2) and np.array_equal(c2, co)
    assert rel_err(s2, s1) < 1e-12 and rel_err(s2, so) < RTOL


# ---- H: the per-window plan on the other engines ----

@pytest.mark.parametrize("kernel", ["em_table", "em_fast"])
@pytest.mark.parametrize("pairwise_del", [False, True])
def test_em_windows_beyond_one_tile(kernel, pairwise_del):
    """130 individuals: EM kernels over more than one 64-individual tile, with and without --pairwise_del"""
    n_ind, n_sites = 130, 300
    p = O.synth_indmajor(23, n_ind, n_sites, miss_frac=0.05)
    lo, hi = many_windows(n_sites, 100, 50)
    with engine(p, kernel, pairwise_del=pairwise_del, indep_geno=False) as e:
        check(e, p, lo, hi, plans=(0, 1), pairwise_del=pairwise_del, indep_geno=False)
        assert e.windows_info()["windows_by_pass"] == len(lo)


@pytest.mark.parametrize("pairwise_del", [False, True])
def test_windows_on_an_engine_that_forms_q_by_ranges(pairwise_del):
    """single_image = 1: only p resident, q formed a range of k-groups at a time -- the smallest ranges
    (single_image_bytes = 1); the segment-slab plan does not apply"""
    n_ind, n_sites = 130, 1500
    p = O.synth_indmajor(29, n_ind, n_sites, miss_frac=0.1)
    lo, hi = many_windows(n_sites, 400, 200)
    with engine(p, "mfma", pairwise_del=pairwise_del, single_image=1) as e:
        assert e.image_mode()[0] == 1
        e.set_option("single_image_bytes", 1)
        check(e, p, lo, hi, plans=(0, 1), pairwise_del=pairwise_del)
        assert e.windows_info()["windows_by_pass"] == len(lo)
        e.set_option("win_plan", 2)
        with pytest.raises(N().NgdError):
            e.run_windows(lo, hi)


# ---- I: windows straight after a staged load ----

@pytest.mark.parametrize("call_geno", [False, True])
def test_windows_first_after_a_staged_load(call_geno):
    """stage_piece_mib = 1 and eager_full = 1: slices of the full pass accumulated beside the load; a windowed call first
    drops them (windows_impl eager_discard), then run().  Both against the oracle on the host's preparation of the same
    raw likelihoods; called genotypes bit for bit."""
    n_ind, n_sites = 200, 4000
    raw = _raw_gl(n_ind, n_sites, 12)
    p = O.prep_binary(raw, n_ind, n_sites, call_geno=call_geno)
    lo, hi = many_windows(n_sites, 1000, 500)
    so, co = oracle_windows(p, lo, hi, pairwise_del=True)
    fo, fc = O.all_pairs(p, pairwise_del=True, n_threads=8)
    with N().Engine(n_ind, n_sites, pairwise_del=True, kernel="mfma") as e:
        e.set_option("stage_piece_mib", 1)
        e.set_option("eager_full", 1)
        for s0, s1 in ((0, 1500), (1500, 2900), (2900, n_sites)):
            e.upload_raw_sites(np.ascontiguousarray(raw[s0:s1]), s0, call_geno=call_geno)
        e.commit()
        s, c = e.run_windows(lo, hi)
        f, fcnt = e.run()
    assert np.array_equal(c, co) and np.array_equal(fcnt, fc)
    if call_geno:
        assert np.array_equal(s, so) and np.array_equal(f, fo)
    assert rel_err(s, so) < RTOL and rel_err(f, fo) < RTOL


# ---- J: the C++ host on a one-image engine ----

def test_cli_windows_with_pairwise_del_on_a_one_image_engine(tmp_path):
    """--win_size / --win_step with --pairwise_del and --posH over three chromosomes, 400 individuals (the host's default
    engine holds one image; a pair of copies with missing sites goes through the fix-up): the first and last window and
    the first of the second chromosome against runs of the host on files cut down to the window's sites"""
    n_ind, n_sites = 400, 600
    rng = np.random.default_rng(14)
    raw = rng.dirichlet([0.6, 0.6, 0.6], size=(n_sites, n_ind))
    raw[:, [5, 300]] = clones(2, n_sites, 1e-11, seed=14).transpose(1, 0, 2)
    raw[rng.random((n_sites, n_ind)) < 0.1] = 0.25
    raw.tofile(str(tmp_path / "g.bin"))
    chrom = ["chrA"] * 230 + ["chrB"] * 220 + ["chrC"] * 150
    pos = str(tmp_path / "p.tsv")
    with open(pos, "w") as fh:
        fh.write("chr\tpos\n")
        for s in range(n_sites):
            fh.write("%s\t%d\n" % (chrom[s], 1000 + 7 * s))
    base = ["--n_ind", n_ind, "--probs", "--indep_geno", "--pairwise_del", "--evol_model", 1]
    out, _ = run_cli(tmp_path, ["--geno", tmp_path / "g.bin", "--n_sites", n_sites, "--win_size", 100, "--win_step", 60,
                                "--posH", pos] + base)
    lo, hi = N().window_ranges(n_sites, 100, 60, chrom=chrom)
    got = split_blocks(open(out).read())
    assert len(got) == len(lo)
    second = int(np.argmax(lo >= 230))
    assert chrom[lo[second]] == "chrB" and chrom[lo[second - 1]] == "chrA"
    for w in (0, second, len(lo) - 1):
        raw[lo[w]:hi[w]].tofile(str(tmp_path / "c.bin"))
        ref, _ = run_cli(tmp_path, ["--geno", tmp_path / "c.bin", "--n_sites", hi[w] - lo[w]] + base, name="c.dist")
        want = split_blocks(open(ref).read())
        assert len(want) == 1
        a, b = blocks("\n" + got[w])[0], blocks("\n" + want[0])[0]
        assert a.shape == (n_ind, n_ind) and np.allclose(a, b, rtol=1e-9, atol=2e-10), w
