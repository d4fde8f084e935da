"""Windows along the genome on the EM path's table-driven kernel through the segment-slab plan (NGD_OPT_WIN_PLAN = 2 on an
NGD_KERNEL_EM_TABLE engine): one accumulation pass whose slices are the segments between window boundaries (accum_em_table.hip,
the slice-table form) plus the banded reduction.  Every window against the CPU oracle's EM run on that window's sites alone
(counts exact, sums to 1e-9 relative) and against the per-window plan of the same engine (counts exact, sums to 1e-12: the
two plans add the same per-site terms in a different order)."""
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from test_gpu_windows import BIN, RTOL, check, engine, mixed_windows, N, oracle_windows, rel_err, split_blocks

pytestmark = pytest.mark.gpu

PLAN_TOL = 1e-12  # plan 2 against plan 1, a batched call against a one-batch call (the header's bound)


def em_engine(p, pairwise_del=False, kernel="em_table", **kw):
    return engine(p, kernel, pairwise_del=pairwise_del, indep_geno=False, **kw)


def run_plan(e, plan, lo, hi):
    e.set_option("win_plan", plan)
    s, c = e.run_windows(lo, hi)
    return s, c, e.windows_info()


@pytest.mark.parametrize("pairwise_del", [False, True])
def test_plan_2_runs_on_the_table_kernel(pairwise_del):
    """(on an engine without the EM form of the plan the call fails with NGD_E_INVALID, -1)"""
    n_ind, n_sites = 130, 300
    p = O.synth_indmajor(11, n_ind, n_sites, miss_frac=0.05)
    lo, hi = mixed_windows(n_sites)
    infos = {}
    with em_engine(p, pairwise_del) as e:
        _, co = check(e, p, lo, hi, plans=(2,), pairwise_del=pairwise_del, indep_geno=False, infos=infos)
    info = infos[2]
    assert info["windows_by_pass"] == 0 and info["segments"] >= 1 and info["batches"] >= 1
    assert info["band_launches"] == (2 if pairwise_del else 1) * info["batches"]
    n_pad = (n_ind + 127) // 128 * 128
    assert info["slab_bytes"] == info["segments"] * n_pad * n_pad * (12 if pairwise_del else 8)
    if pairwise_del:
        assert co.min() < (hi - lo).max()  # (some pair does miss sites: the counts are not the windows' lengths)


@pytest.mark.parametrize("n_ind", [70, 200])
@pytest.mark.parametrize("pairwise_del", [False, True])
def test_more_tile_rows_and_a_ragged_edge_agree_with_the_per_window_plan(n_ind, pairwise_del):
    n_sites = 500
    p = O.synth_indmajor(23, n_ind, n_sites, miss_frac=0.05)
    lo, hi = mixed_windows(n_sites)
    slo, shi = N().window_ranges(n_sites, 120, 45)
    lo, hi = np.concatenate([lo, slo.astype(np.int64)]), np.concatenate([hi, shi.astype(np.int64)])
    order = np.argsort(lo, kind="stable")
    lo, hi = lo[order], hi[order]
    with em_engine(p, pairwise_del) as e:
        check(e, p, lo, hi, plans=(2,), pairwise_del=pairwise_del, indep_geno=False)
        s2, c2, i2 = run_plan(e, 2, lo, hi)
        s1, c1, i1 = run_plan(e, 1, lo, hi)
        # auto takes the cheaper plan by estimate: here one pass over the covered sites against 24 passes
        s0, c0, i0 = run_plan(e, 0, lo, hi)
    assert i1["windows_by_pass"] == len(lo) and i2["windows_by_pass"] == 0 and i0["windows_by_pass"] == 0
    assert np.array_equal(c1, c2) and np.array_equal(c0, c2)
    d = rel_err(s2, s1)
    print("plan 2 against plan 1, %d individuals, pairwise_del=%d: %.3g relative" % (n_ind, pairwise_del, d))
    assert d < PLAN_TOL
    assert np.array_equal(s0, s2)


@pytest.mark.parametrize("pairwise_del", [False, True])
def test_batches_by_the_memory_budget(pairwise_del):
    n_ind, n_sites = 70, 3000
    p = O.synth_indmajor(13, n_ind, n_sites, miss_frac=0.1 if pairwise_del else 0.0)
    rng = np.random.default_rng(4)
    lo = np.sort(rng.integers(0, n_sites - 200, size=40))
    hi = lo + rng.integers(1, 200, size=40)
    plane = 128 * 128
    with em_engine(p, pairwise_del) as e:
        check(e, p, lo, hi, plans=(2,), pairwise_del=pairwise_del, indep_geno=False)
        s1, c1, one = run_plan(e, 2, lo, hi)
        # a budget of eight segments' planes (sums, and counts under --pairwise_del) + the tables
        e.set_option("win_max_bytes", 8 * plane * (12 if pairwise_del else 8) + 4096)
        s2, c2, info = run_plan(e, 2, lo, hi)
        assert info["batches"] >= 3 and one["batches"] == 1 and info["windows_by_pass"] == 0
        assert info["slab_bytes"] <= 8 * plane * (12 if pairwise_del else 8)
        assert np.array_equal(c1, c2)
        d = rel_err(s2, s1)
        print("batched against one batch, pairwise_del=%d: %.3g relative" % (pairwise_del, d))
        assert d < PLAN_TOL
        # a budget no window fits: the slab plan alone cannot run, auto takes the per-window plan
        e.set_option("win_max_bytes", 1)
        with pytest.raises(N().NgdError) as ei:
            e.run_windows(lo, hi)
        assert ei.value.code == -4
        s3, c3, i3 = run_plan(e, 0, lo, hi)
        assert i3["windows_by_pass"] == len(lo) and i3["segments"] == 0
        assert np.array_equal(c3, c1) and rel_err(s3, s1) < PLAN_TOL


def test_chromosome_windows_give_segments_of_unequal_length():
    n_ind, n_sites = 70, 600
    p = O.synth_indmajor(29, n_ind, n_sites, miss_frac=0.05)
    chrom = ["chrA"] * 251 + ["chrB"] * 298 + ["chrC"] * 51  # chromosomes start at sites 0, 251 and 549
    lo, hi = N().window_ranges(n_sites, 100, 60, chrom=chrom)
    assert 251 in lo and not np.any((lo < 251) & (hi > 251)) and not np.any((lo < 549) & (hi > 549))
    # a long chromosome-wide window on top: intervals longer than a slice, cut into pieces
    lo = np.concatenate([lo, [251]]).astype(np.int64)
    hi = np.concatenate([hi, [549]]).astype(np.int64)
    order = np.argsort(lo, kind="stable")
    for pairwise_del in (False, True):
        with em_engine(p, pairwise_del) as e:
            check(e, p, lo[order], hi[order], plans=(2, 0), pairwise_del=pairwise_del, indep_geno=False)


def test_non_finite_terms_reach_exactly_the_windows_that_hold_their_site():
    """An all-zero individual at one site gives 0/0 in normalize(), as on the CPU: NaN for that individual's pairs in the
    windows that contain the site and nowhere else (the banded reduction selects segments, it never multiplies by 0)."""
    # the oracle's own behaviour, on the case the plan was specified with
    q = O.synth_indmajor(3, 6, 40)
    q[2, 10] = 0
    sa, _ = O.all_pairs(q, indep_geno=False, site_src=np.arange(5, 20))
    sb, _ = O.all_pairs(q, indep_geno=False, site_src=np.arange(20, 40))
    assert int(np.isnan(sa).sum()) == 5 and np.all(np.isfinite(sb))

    n_ind, n_sites = 70, 300
    p = O.synth_indmajor(31, n_ind, n_sites)
    p[2, 10] = 0     # first tile row
    p[66, 250] = 0   # second tile row / column
    lo = np.array([0, 5, 10, 11, 20, 100, 200, 250, 251])
    hi = np.array([10, 20, 11, 300, 40, 260, 250, 251, 300])
    so, co = oracle_windows(p, lo, hi, indep_geno=False)
    holds = [(a <= 10 < b, a <= 250 < b) for a, b in zip(lo, hi)]
    for w, (h2, h66) in enumerate(holds):  # the oracle: NaN in exactly the pairs of the individuals whose site the window holds
        assert int(np.isnan(so[w]).sum()) == (n_ind - 1) * (h2 + h66) - (h2 and h66)
    assert any(not (a or b) for a, b in holds) and any(a and not b for a, b in holds) and any(b and not a for a, b in holds)
    with em_engine(p) as e:
        for plan in (2, 1):
            s, c, info = run_plan(e, plan, lo, hi)
            assert (info["windows_by_pass"] == 0) == (plan == 2)
            assert np.array_equal(c, co)
            assert np.array_equal(np.isnan(s), np.isnan(so)), "plan %d" % plan
            ok = np.isfinite(so)
            assert np.all(np.isfinite(s[ok])) and rel_err(s[ok], so[ok]) < RTOL
        # ... and with the budget of a few planes: a segment two batches share carries its NaN into both
        e.set_option("win_max_bytes", 3 * 128 * 128 * 8 + 4096)
        s, c, info = run_plan(e, 2, lo, hi)
        assert info["batches"] >= 2
        assert np.array_equal(np.isnan(s), np.isnan(so)) and rel_err(s[ok], so[ok]) < RTOL


def test_the_engine_s_other_calls_are_unchanged_by_a_windowed_call():
    """the windowed call takes the scratch of the bootstrap's partial results and drops their cache: run() and a
    two-replicate run_batch give the same bits before and after it"""
    n_ind, n_sites, B = 130, 600, 3
    p = O.synth_indmajor(37, n_ind, n_sites, miss_frac=0.05)
    maps = np.stack([N().Taus(5 + r).block_map(n_sites // B) for r in range(2)])
    lo, hi = N().window_ranges(n_sites, 200, 50)
    for pairwise_del in (False, True):
        with em_engine(p, pairwise_del) as e:
            s_a, c_a = e.run()
            b_a, bc_a = e.run_batch(maps, B)
            sw, cw, info = run_plan(e, 2, lo, hi)
            assert info["windows_by_pass"] == 0 and info["segments"] >= len(lo)
            s_b, c_b = e.run()
            b_b, bc_b = e.run_batch(maps, B)
            sw2, cw2, _ = run_plan(e, 2, lo, hi)
        assert np.array_equal(s_a.view(np.uint64), s_b.view(np.uint64)) and np.array_equal(c_a, c_b)
        assert np.array_equal(b_a.view(np.uint64), b_b.view(np.uint64)) and np.array_equal(bc_a, bc_b)
        assert np.array_equal(sw.view(np.uint64), sw2.view(np.uint64)) and np.array_equal(cw, cw2)
        # the whole data set as one window is run()'s matrix, to rounding
        so, co = O.all_pairs(p, pairwise_del=pairwise_del, indep_geno=False, n_threads=8)
        assert np.array_equal(c_a, co) and rel_err(s_a, so) < RTOL


@pytest.mark.parametrize("kernel,indep", [("em_fast", False), ("em_faithful", False), ("stream", True)])
def test_the_other_kernels_still_refuse_plan_2(kernel, indep):
    p = O.synth_indmajor(11, 20, 300, miss_frac=0.05)
    lo, hi = np.array([0, 30, 101]), np.array([100, 200, 300])
    with engine(p, kernel, indep_geno=indep) as e:
        e.set_option("win_plan", 2)
        with pytest.raises(N().NgdError) as ei:
            e.run_windows(lo, hi)
        assert ei.value.code == -1
        check(e, p, lo, hi, plans=(0, 1), indep_geno=indep)
        assert e.windows_info()["windows_by_pass"] == len(lo)


@pytest.mark.parametrize("variant", [1, 2, 3, 4])
def test_every_workgroup_shape_of_the_table_kernel_has_the_plan(variant):
    """include/ngsdist_amd.h: the segment-slab plan serves NGD_KERNEL_EM_TABLE with any ngd_config.variant"""
    n_ind, n_sites = 70, 300
    p = O.synth_indmajor(41, n_ind, n_sites, miss_frac=0.05)
    lo, hi = mixed_windows(n_sites)
    ref = oracle_windows(p, lo, hi, indep_geno=False)
    with em_engine(p, variant=variant) as e:
        check(e, p, lo, hi, plans=(2, 1), indep_geno=False, ref=ref)
    refd = oracle_windows(p, lo, hi, pairwise_del=True, indep_geno=False)
    with em_engine(p, True, variant=variant) as e:
        check(e, p, lo, hi, plans=(2,), pairwise_del=True, indep_geno=False, ref=refd)


def test_windows_dist_and_the_command_line_reach_the_plan(tmp_path):
    """bin/ngsDist --win_size without --indep_geno above 32 individuals: the engine's auto plan is the segment slab, and the
    file holds the bytes of an engine pinned to the per-window plan (the two plans' sums differ by rounding, ~1e-16
    relative; a cell within that of a rounding edge of "%.10f" would differ in its last digit -- none does here)"""
    n_ind, n_sites = 40, 600
    rng = np.random.default_rng(8)
    raw = rng.dirichlet([0.6, 0.6, 0.6], size=(n_sites, n_ind))
    raw.tofile(str(tmp_path / "g.bin"))
    out = str(tmp_path / "w.dist")
    r = subprocess.run([BIN, "--geno", str(tmp_path / "g.bin"), "--probs", "--n_ind", str(n_ind), "--n_sites", str(n_sites),
                        "--win_size", "100", "--win_step", "50", "--evol_model", "1", "--out", out, "--verbose", "2"],
                       capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    lo, hi = N().window_ranges(n_sites, 100, 50)
    lines = [l for l in r.stderr.decode().split("\n") if l.startswith("> windows ")]
    assert len(lines) == 1 and " 0 windows by a pass of their own" in lines[0], r.stderr.decode()
    assert int(lines[0].split(": ")[1].split(" ")[0]) >= len(lo)  # segments
    labels = ["Ind_%d" % i for i in range(n_ind)]
    with N().Engine(n_ind, n_sites, indep_geno=False, kernel="auto") as e:
        e.upload_raw_sites(raw, 0).commit()
        e.set_option("win_plan", 1)
        d1 = e.run_windows_dist(lo, hi, evol_model=1)
        assert e.windows_info()["windows_by_pass"] == len(lo)
        e.set_option("win_plan", 0)
        d0 = e.run_windows_dist(lo, hi, evol_model=1)
        i0 = e.windows_info()
        s0, c0 = e.run_windows(lo, hi)
    assert i0["windows_by_pass"] == 0 and i0["segments"] >= len(lo)
    assert np.array_equal(d0.view(np.uint64), N().finish(s0.reshape(-1), c0.reshape(-1), 0, 1).reshape(s0.shape).view(np.uint64))
    print("windowed distances, auto against the per-window plan: %.3g relative" % rel_err(d0, d1))
    assert rel_err(d0, d1) < RTOL
    got = open(out, "rb").read()
    assert len(split_blocks(got.decode())) == len(lo)
    assert got == b"".join(N().format_matrix(d1[w], labels) for w in range(len(lo)))
