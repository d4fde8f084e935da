"""Windows along the genome (ngd_run_windows*, --win_size / --win_step): every window's matrix against the CPU oracle run on
the window's sites alone, through both plans (one weighted pass per window, the segment slab), the engine ABI and the C++
host."""
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

RTOL = 1e-9
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "ngsdist_amd", "bin", "ngsDist")


def N():
    import ngsdist_amd
    return ngsdist_amd


def rel_err(a, b):
    a, b = np.asarray(a), np.asarray(b)
    den = np.where(b == 0, 1.0, np.abs(b))
    return float(np.max(np.abs(a - b) / den)) if a.size else 0.0


def oracle_windows(p, lo, hi, pairwise_del=False, indep_geno=True):
    out = [O.all_pairs(p, pairwise_del=pairwise_del, indep_geno=indep_geno, site_src=np.arange(a, b), n_threads=8)
           for a, b in zip(lo, hi)]
    return np.stack([s for s, _ in out]), np.stack([c for _, c in out])


def engine(p, kernel, pairwise_del=False, indep_geno=True, **kw):
    n_ind, n_sites, _ = p.shape
    e = N().Engine(n_ind, n_sites, pairwise_del=pairwise_del, indep_geno=indep_geno, kernel=kernel, **kw)
    e.upload_ind_major(p).commit()
    return e


def check(e, p, lo, hi, plans=(0, 1, 2), pairwise_del=False, indep_geno=True, exact=False, ref=None, infos=None):
    """every plan of `plans` against the oracle on each window's sites (ref: its (sums, counts), computed once by the caller);
    infos: a dict that receives windows_info() per plan"""
    so, co = oracle_windows(p, lo, hi, pairwise_del, indep_geno) if ref is None else ref
    for plan in plans:
        e.set_option("win_plan", plan)
        s, c = e.run_windows(lo, hi)
        assert s.shape == (len(lo), e.n_pairs)
        assert np.array_equal(c, co), "plan %d: counts" % plan
        if exact:
            assert np.array_equal(s, so), "plan %d: called genotypes must be bit-exact" % plan
        assert rel_err(s, so) < RTOL, "plan %d" % plan
        info = e.windows_info()
        if infos is not None:
            infos[plan] = info
        if plan == 1:
            assert info["windows_by_pass"] == len(lo) and info["segments"] == 0
        if plan == 2:
            assert info["windows_by_pass"] == 0 and info["batches"] >= 1 and info["segments"] >= 1
    return so, co


# sliding, nested, gapped and one-site windows; boundaries at every residue mod 4 (the unaligned k-group edges)
def mixed_windows(n_sites):
    lo = [0, 0, 1, 2, 3, 5, 7, 50, 50, 51, 97, 98, 130, n_sites - 1]
    hi = [40, 13, 30, 3, 90, 6, 250, 101, 60, 52, 200, 99, 131, n_sites]
    return np.array(lo), np.array(hi)


@pytest.mark.parametrize("kernel,kw", [("mfma", {"single_image": 3}), ("mfma", {"single_image": 2}), ("stream", {})])
@pytest.mark.parametrize("n_ind", [6, 40, 130])
def test_indep_windows_against_the_oracle(kernel, kw, n_ind):
    n_sites = 777
    p = O.synth_indmajor(7, n_ind, n_sites)
    lo, hi = mixed_windows(n_sites)
    with engine(p, kernel, **kw) as e:
        plans = (0, 1, 2) if kernel == "mfma" else (0, 1)
        check(e, p, lo, hi, plans=plans)
        if kernel == "stream":
            e.set_option("win_plan", 2)
            with pytest.raises(N().NgdError):
                e.run_windows(lo, hi)


@pytest.mark.parametrize("kernel", ["mfma", "stream"])
def test_pairwise_del_windows(kernel):
    p = O.synth_indmajor(5, 40, 3000, miss_frac=0.2)
    lo, hi = N().window_ranges(3000, 700, 300)
    lo, hi = np.concatenate([lo, [5, 1999]]), np.concatenate([hi, [6, 2003]])
    order = np.argsort(lo, kind="stable")
    with engine(p, kernel, pairwise_del=True) as e:
        _, co = check(e, p, lo[order], hi[order], plans=(0, 1, 2) if kernel == "mfma" else (0, 1), pairwise_del=True)
    assert co.min() < 700


@pytest.mark.parametrize("single_image", [2, 3])
def test_called_genotypes_bit_exact(single_image):
    rng = np.random.default_rng(1)
    n_ind, n_sites = 24, 4000
    g = rng.integers(0, 3, size=(n_ind, n_sites))
    p = np.zeros((n_ind, n_sites, 3))
    np.put_along_axis(p, g[..., None], 1.0, axis=2)
    lo, hi = N().window_ranges(n_sites, 1001, 333)
    with engine(p, "mfma", single_image=single_image) as e:
        check(e, p, lo, hi, exact=True)


@pytest.mark.parametrize("kernel", ["em_table", "em_fast", "em_faithful"])
def test_em_windows(kernel):
    p = O.synth_indmajor(11, 20, 300, miss_frac=0.05)
    lo, hi = np.array([0, 1, 30, 30, 101, 299]), np.array([100, 2, 200, 31, 300, 300])
    with engine(p, kernel, indep_geno=False) as e:
        check(e, p, lo, hi, plans=(0, 1), indep_geno=False)
        assert e.windows_info()["windows_by_pass"] == len(lo)


def test_windows_start_at_arbitrary_sites_and_batches_agree():
    n_ind, n_sites = 70, 3000
    p = O.synth_indmajor(13, n_ind, n_sites)
    rng = np.random.default_rng(4)
    lo = np.sort(rng.integers(0, n_sites - 200, size=40))
    hi = lo + rng.integers(1, 200, size=40)
    with engine(p, "mfma", single_image=3) as e:
        check(e, p, lo, hi, plans=(2,))
        s1, c1 = e.run_windows(lo, hi)
        one = e.windows_info()
        # a budget of a few segments' planes: at least three batches, the same results (segments they share recomputed)
        e.set_option("win_max_bytes", 12 * 128 * 128 * 8 + (1 << 20))
        s2, c2 = e.run_windows(lo, hi)
        info = e.windows_info()
        assert info["batches"] >= 3 and one["batches"] == 1
        assert np.array_equal(c1, c2) and rel_err(s2, s1) < 1e-12
        # a budget no window fits: the slab plan alone cannot run, auto takes the per-window plan
        e.set_option("win_max_bytes", 1)
        with pytest.raises(N().NgdError) as ei:
            e.run_windows(lo, hi)
        assert ei.value.code == -4
        e.set_option("win_plan", 0)
        s3, _ = e.run_windows(lo, hi)
        assert e.windows_info()["windows_by_pass"] == len(lo)
        assert rel_err(s3, s1) < RTOL


def test_windows_agree_with_run_mult_batch_on_a_block_grid():
    n_ind, n_sites, B = 50, 4000, 100
    p = O.synth_indmajor(17, n_ind, n_sites, miss_frac=0.1)
    lo, hi = N().window_ranges(n_sites, 4 * B, 2 * B)
    mult = np.zeros((len(lo), n_sites // B), dtype=np.uint32)
    for w, (a, b) in enumerate(zip(lo, hi)):
        mult[w, a // B:b // B] = 1
    for pdel in (False, True):
        with engine(p, "mfma", pairwise_del=pdel, single_image=3) as e:
            e.set_option("win_plan", 2)
            s, c = e.run_windows(lo, hi)
            sm, cm = e.run_batch(mult=mult, block_size=B)
            assert np.array_equal(c, cm) and rel_err(s, sm) < 1e-12


def test_clones_on_a_one_image_engine_are_fixed_in_every_window():
    n_ind, n_sites = 200, 6000
    rng = np.random.default_rng(3)
    p = O.synth_indmajor(9, n_ind, n_sites)
    g = rng.integers(0, 3, size=n_sites)
    for k in list(range(5, 25)) + [150, 151]:  # a cluster of nearly identical individuals, and a pair of them
        q = 1e-12 * (1 + rng.random((n_sites, 3)))
        q[np.arange(n_sites), g] = 0
        q[np.arange(n_sites), g] = 1 - q.sum(axis=1)
        p[k] = q
    lo, hi = N().window_ranges(n_sites, 1000, 500)
    with engine(p, "mfma", single_image=2) as e:
        assert e.image_mode() == (2, True)
        check(e, p, lo, hi, plans=(2, 1))
        e.set_option("win_plan", 2)
        e.run_windows(lo, hi)
        assert e.windows_info()["fixup_pairs"] >= 190 * len(lo)


def test_bad_windows_are_refused_and_hold_no_memory():
    p = O.synth_indmajor(3, 20, 500)
    with engine(p, "mfma") as e:
        s, _ = e.run_windows([0], [500])
        assert rel_err(s[0], O.all_pairs(p)[0]) < RTOL
        before = e.device_bytes()
        bad = [([0], [501]), ([5], [5]), ([7], [3]), ([10, 9], [20, 30]), ([], [])]
        for k in range(20):
            lo, hi = bad[k % len(bad)]
            with pytest.raises(N().NgdError) as ei:
                e.run_windows(lo, hi)
            assert ei.value.code == -1
        assert e.device_bytes() == before
        with pytest.raises(N().NgdError) as ei:
            e.run_windows_dist([0], [10], evol_model=3)
        assert ei.value.code == -5


def test_windows_dist_is_finish_of_the_windows():
    p = O.synth_indmajor(21, 30, 900)
    lo, hi = N().window_ranges(900, 300, 150)
    with engine(p, "mfma") as e:
        s, c = e.run_windows(lo, hi)
        for model in (0, 1, 2):
            d = e.run_windows_dist(lo, hi, evol_model=model)
            want = N().finish(s.reshape(-1), c.reshape(-1), 0, model).reshape(s.shape)
            assert np.array_equal(d.view(np.uint64), want.view(np.uint64))
        d = e.run_windows_dist(lo, hi, evol_model=0, tot_sites=1000)
        assert np.array_equal(d, s / 1000.0)


def test_engine_sharing_pairs_refuses_windows():
    p = O.synth_indmajor(3, 20, 300)
    with N().Engine(20, 300, kernel="mfma", shard_rank=0, shard_world=2) as e:
        e.upload_ind_major(p).commit()
        with pytest.raises(N().NgdError):
            e.run_windows([0], [100])


def test_near_full_size_windows():
    n_ind, n_sites = 1000, 100000
    lo, hi = N().window_ranges(n_sites, 2000, 500)
    with N().Engine(n_ind, n_sites, kernel="mfma") as e:
        e.synth_fill(5, 0.0)
        s, c = e.run_windows(lo, hi)
        info = e.windows_info()
        assert info["windows_by_pass"] == 0 and info["segments"] >= len(lo)
        assert np.all(c == (hi - lo)[:, None])
        inds = [0, 1, 17, 500, 501, 999]
        rows = np.concatenate([O.synth_indmajor(5, n_ind, n_sites, i0=i, n_sub=1) for i in inds])
        for w in (0, len(lo) // 2, len(lo) - 1):
            so, _ = O.all_pairs(rows, site_src=np.arange(lo[w], hi[w]))
            k = 0
            for ia in range(len(inds)):
                for ib in range(ia + 1, len(inds)):
                    got = s[w, N().engine._lib.load().ngd_pair_index(n_ind, inds[ia], inds[ib])]
                    assert abs(got - so[k]) <= RTOL * abs(so[k])
                    k += 1


# ---- the C++ host ----

def run_cli(tmp_path, args, name="w.dist", ok=True):
    out = str(tmp_path / name)
    r = subprocess.run([BIN] + [str(a) for a in args] + ["--out", out, "--verbose", "0"], capture_output=True, timeout=600)
    assert (r.returncode == 0) == ok, r.stderr.decode()
    return out, r


def split_blocks(text):
    """the print blocks of a .dist file ("\n<n_ind>\n" + rows each), without their leading newline"""
    assert text.startswith("\n")
    return text[1:].split("\n\n")


def blocks(text):
    """the matrices of a .dist file: lists of rows of floats"""
    parts = split_blocks(text)
    mats = []
    for part in parts:
        lines = [l for l in part.split("\n") if l]
        mats.append(np.array([[float(x) for x in l.split("\t")[1:]] for l in lines[1:]]))
    return mats


@pytest.mark.parametrize("mode", ["call_geno", "gl", "em"])
def test_cli_windows_match_runs_on_the_cut_down_files(tmp_path, mode):
    n_ind, n_sites = 12, 600
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
    for with_pos in (False, True):
        extra = ["--posH", pos] if with_pos else []
        out, _ = run_cli(tmp_path, ["--geno", tmp_path / "g.bin", "--n_sites", n_sites, "--win_size", 100, "--win_step", 60]
                         + extra + base)
        lo, hi = N().window_ranges(n_sites, 100, 60, chrom=chrom if with_pos else None)
        text = open(out).read()
        got = split_blocks(text)
        assert len(got) == len(lo)
        win = open(out + ".windows").read().strip().split("\n")
        assert win[0] == "window\tchr\tstart\tend\tfirst_site\tn_sites" and len(win) == len(lo) + 1
        for w, line in enumerate(win[1:]):
            f = line.split("\t")
            if with_pos:
                assert f == [str(w), chrom[lo[w]], str(1000 + 7 * lo[w]), str(1000 + 7 * (hi[w] - 1)), str(lo[w]), "100"]
            else:
                assert f == [str(w), ".", str(lo[w] + 1), str(hi[w]), str(lo[w]), "100"]
        for w in (0, 1, len(lo) - 1):
            raw[lo[w]:hi[w]].tofile(str(tmp_path / "c.bin"))
            ref, _ = run_cli(tmp_path, ["--geno", tmp_path / "c.bin", "--n_sites", hi[w] - lo[w]] + base, name="c.dist")
            want = split_blocks(open(ref).read())
            assert len(want) == 1
            if mode == "call_geno":
                assert got[w].rstrip("\n") == want[0].rstrip("\n")  # (the last block of a file ends with its newline)
            else:
                a, b = blocks("\n" + got[w])[0], blocks("\n" + want[0])[0]
                assert np.allclose(a, b, rtol=1e-9, atol=2e-10)


def test_cli_window_errors(tmp_path):
    T_GL = os.path.join(ROOT, "tests", "golden", "survey_probe", "t_gl.bin")
    base = ["--geno", T_GL, "--probs", "--n_ind", 6, "--n_sites", 200, "--indep_geno"]
    for extra, msg in ((["--win_size", 0], "window size"), (["--win_size", 10, "--win_step", 0], "window step"),
                       (["--win_step", 10], "requires a window size"), (["--win_size", 500], "no window"),
                       (["--win_size", 10, "--n_boot_rep", 2], "bootstrap"), (["--win_size", 10, "--n_gpus", 2], "one GPU")):
        _, r = run_cli(tmp_path, base + extra, ok=False)
        assert r.returncode == 255 and msg in r.stderr.decode()
    # without the flags nothing changes: no .windows file
    out, _ = run_cli(tmp_path, base + ["--evol_model", 0], name="plain.dist")
    assert open(out).read() == open(os.path.join(ROOT, "tests", "golden", "survey_probe", "t_gl_I0.dist")).read()
    assert not os.path.exists(out + ".windows")
