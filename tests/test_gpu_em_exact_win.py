"""NGD_OPT_EM_EXACT_WIN / --em_exact_win: the windowed calls -- ngd_run_windows*, ngd_run_windows_job* -- on the EM path stop
every (pair, site) where the reference does.

The list of in-band (pair, site)s depends neither on the window nor on the replicate, so the segment-slab plan's one
accumulation pass per batch notes it (the slice-table form of the noting kernel), the host rechecks it behind the banded
reductions, and every matrix of every window takes its weight of the site times (c_ref - c_dev).  Data: the planted set of
tests/test_gpu_em_exact.py (130 individuals x 64 sites, 100 in-band probes on a diagonal 64-tile, an off-diagonal one and a
ragged third).  Yardstick for a window [lo, hi): the oracle's pair loop on the array cut down to the window -- for a
replicate with the block map's site_src on that array -- on the reference's own compiled em2() where oracle/_ref is built.
Tolerance: 1e-9 relative, the project's bar, on every cell; counts equal.

A window holds few sites: one site stopped a step early is a far larger share of a 16-site window's sum than of the
genome's.  test_windows prints (pytest -s) how many (window, pair) cells the option-off call misses."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from test_gpu_em_exact import BIN, CASES, N, N_IND, N_SITES, O_pair, RTOL, boundaries, entry_keys, oracle_pairs, planted

pytestmark = pytest.mark.gpu

PLANE = 8 * 256 * 256  # bytes of one slice's partial result: n_pad = 130 rounded up to 128s
SEEDS = [211, 212, 213]
STEP = ([0, 8, 16, 24, 32, 40, 48], [16, 24, 32, 40, 48, 56, 64])  # 16 sites every 8: overlapping, their segments shared
WINDOWS = {
    "step": STEP,
    "mixed": ([0, 3, 5], [64, 30, 6]),  # everything; starts and ends off any multiple of 4; a single site
    "gap": ([4, 33], [12, 47]),         # sites 12 .. 32 belong to no window
}
_cache = {}


def win_oracle(pdel, lo, hi):
    """(sums, counts) [n_win][n_pairs] of the windows' cut-down arrays"""
    p = planted(pdel)[0]
    out = []
    for a, b in zip(lo, hi):
        key = (pdel, a, b)
        if key not in _cache:
            _cache[key] = oracle_pairs(np.ascontiguousarray(p[:, a:b]), pairwise_del=pdel)
        out.append(_cache[key])
    return np.stack([s for s, _ in out]), np.stack([c for _, c in out])


def job_maps(B, W=16):
    return np.stack([N().Taus(s).block_map(W // B) for s in SEEDS])


def job_oracle(pdel, lo, hi, B):
    """[n_win][1 + replicates][n_pairs]: matrix 0 the window, matrix r the replicate's sites of the cut-down array"""
    key = ("job", pdel, tuple(lo), tuple(hi), B)
    if key not in _cache:
        p = planted(pdel)[0]
        maps = job_maps(B, hi[0] - lo[0])
        S0, C0 = win_oracle(pdel, lo, hi)
        S, Cn = [], []
        for w, (a, b) in enumerate(zip(lo, hi)):
            cut = np.ascontiguousarray(p[:, a:b])
            rows = [(S0[w], C0[w])] + [oracle_pairs(cut, pairwise_del=pdel, site_src=O.boot_site_src(bm, B), n_sites=len(bm) * B)
                                       for bm in maps]
            S.append(np.stack([s for s, _ in rows]))
            Cn.append(np.stack([c for _, c in rows]))
        _cache[key] = (maps, np.stack(S), np.stack(Cn))
    return _cache[key]


def within(S, So, tol=RTOL):
    """every cell within tol (relative) of the yardstick; a cell whose yardstick is 0 -- no valid site -- must be 0"""
    return bool(np.all(np.abs(S - So) <= tol * np.abs(So)))


def missed(S, So):
    return int(np.sum(np.abs(S - So) > RTOL * np.abs(So)))


def engine(pdel, options=(), **kw):
    e = N().Engine(N_IND, N_SITES, indep_geno=False, pairwise_del=pdel, **kw)
    e.upload_ind_major(planted(pdel)[0]).commit()
    for k, v in dict(options).items():
        e.set_option(k, v)
    return e


def run_windows(pdel, lo, hi, exact, options=(), **kw):
    with engine(pdel, options, **kw) as e:
        if exact:
            e.set_option("em_exact", exact)
            e.set_option("em_exact_win", 1)
        S, Cn = e.run_windows(lo, hi)
        return S, Cn, e.em_exact_entries(), e.last_em_exact(), e.windows_info()


def run_job(pdel, lo, hi, B, exact, options=(), **kw):
    maps = job_oracle(pdel, lo, hi, B)[0]
    with engine(pdel, options, **kw) as e:
        if exact:
            e.set_option("em_exact", 2)
            e.set_option("em_exact_win", 1)
        S, Cn = e.run_windows_job(lo, hi, maps, B)
        return S, Cn, e.em_exact_entries(), e.last_em_exact(), e.windows_info()


def check_list(ent, info):
    order = list(map(tuple, ent[["i1", "i2", "site"]].tolist()))
    assert order == sorted(order) and len(set(order)) == len(order)  # every entry once
    assert info["noted"] == len(ent)


def quiet_cells(ent, lo, hi):
    """[window][pair]: no noted site of the pair lies inside the window"""
    q = np.ones((len(lo), N().n_pairs(N_IND)), dtype=bool)
    for x in ent:
        for w, (a, b) in enumerate(zip(lo, hi)):
            if a <= int(x["site"]) < b:
                q[w, O_pair(int(x["i1"]), int(x["i2"]))] = False
    return q


SLAB = dict(win_plan=2)


@pytest.mark.parametrize("value", [1, 2])
@pytest.mark.parametrize("pdel", [False, True])
def test_windows(pdel, value):
    n_missed = 0
    for name, (lo, hi) in WINDOWS.items():
        So, Co = win_oracle(pdel, lo, hi)
        S0, C0, ent0, info0, _ = run_windows(pdel, lo, hi, 0, SLAB)
        assert len(ent0) == 0 and info0["noted"] == 0
        S, Cn, ent, info, wi = run_windows(pdel, lo, hi, value, SLAB)
        S2, C2, ent2, _, _ = run_windows(pdel, lo, hi, value, SLAB)
        n_missed += missed(S0, So)
        with np.errstate(invalid="ignore"):  # (--pairwise_del: a pair without a valid site in a window is 0 / 0)
            worst_off = np.nanmax(np.abs(S0 - So) / np.abs(So))
        print("pairwise_del=%d value %d %s: noted %d, changed %d; option off misses %d of %d (window, pair) cells, by up to %.3g"
              % (pdel, value, name, info["noted"], info["changed"], missed(S0, So), S0.size,
                 worst_off))
        assert np.array_equal(Cn, Co) and np.array_equal(C0, Co)
        assert within(S, So), (name, missed(S, So))
        assert np.array_equal(S.view(np.uint64), S2.view(np.uint64)) and ent.tobytes() == ent2.tobytes()  # run to run
        check_list(ent, info)
        assert info["passes"] == 1 and wi["windows_by_pass"] == 0 and wi["batches"] == 1
        quiet = quiet_cells(ent, lo, hi)
        assert np.array_equal(S[quiet].view(np.uint64), S0[quiet].view(np.uint64))  # quiet cells: the option-off bits
        covered = {s for a, b in zip(lo, hi) for s in range(a, b)}
        keys = entry_keys(ent)
        assert all(site in covered for _, _, site in keys)
        gone = planted(pdel)[2]
        for i1, i2, site, *_ in planted(pdel)[1]:
            assert ((i1, i2, site) in keys) == ((i1, i2, site) != gone and site in covered), (name, i1, i2, site)
        if name == "mixed" and value == 1:  # the window [0, 64) is the plain pass under value 1
            with engine(pdel) as e:
                e.set_option("em_exact", 1)
                s, c = e.run()
            assert np.array_equal(c, Cn[0]) and within(S[0], s, 1e-12)
    # the planted set guarantees it: at every probe the adjacent iterates differ by more than 1e-6 of the full-data sum
    assert n_missed > 0


@pytest.mark.parametrize("B", [1, 4, 3, 16])
@pytest.mark.parametrize("pdel", [False, True])
def test_jobs(pdel, B):
    """block sizes 1, 4 (divides the step), 3 (does not: blocks of a few slices and a tail of one site that only matrix 0
    sees) and 16 (one block)"""
    lo, hi = STEP
    maps, So, Co = job_oracle(pdel, lo, hi, B)
    S0 = run_job(pdel, lo, hi, B, 0, SLAB)[0]
    S, Cn, ent, info, wi = run_job(pdel, lo, hi, B, 2, SLAB)
    S2, _, ent2, _, _ = run_job(pdel, lo, hi, B, 2, SLAB)
    print("pairwise_del=%d B=%d: noted %d, changed %d; option off misses %d of %d cells"
          % (pdel, B, info["noted"], info["changed"], missed(S0, So), S0.size))
    assert np.array_equal(Cn, Co)
    assert within(S, So), missed(S, So)
    assert np.array_equal(S.view(np.uint64), S2.view(np.uint64)) and ent.tobytes() == ent2.tobytes()
    check_list(ent, info)
    assert wi["windows_by_pass"] == 0
    Sw = run_windows(pdel, lo, hi, 2, SLAB)[0]
    assert np.array_equal(S[:, 0].view(np.uint64), Sw.view(np.uint64))  # matrix 0: run_windows under the same options
    with engine(pdel, SLAB) as e:
        e.set_option("em_exact", 2)
        e.set_option("em_exact_win", 1)
        d = e.run_windows_job_dist(lo, hi, maps, B, 1)
    do = O.finish(So.reshape(-1), Co.reshape(-1), 0, 1).reshape(So.shape)
    fin = np.isfinite(do)
    assert np.array_equal(np.isnan(d), np.isnan(do)) and within(d[fin], do[fin])


@pytest.mark.parametrize("pdel", [False, True])
def test_several_batches(pdel):
    """a budget of a few planes: the windows go batch by batch, each batch noted, rechecked and patched on its own; overlapping
    windows of two batches note their shared sites twice and the call's list holds them once"""
    lo, hi = STEP
    per_plane = PLANE + (PLANE // 2 if pdel else 0)
    for value in (1, 2):
        S, Cn, ent, info, wi = run_windows(pdel, lo, hi, value, SLAB)
        Sb, Cb, entb, infob, wib = run_windows(pdel, lo, hi, value, dict(SLAB, win_max_bytes=3 * per_plane + 65536))
        assert wi["batches"] == 1 and wib["batches"] > 1
        assert np.array_equal(Cn, Cb) and within(Sb, S, 1e-12)
        check_list(entb, infob)
        assert entry_keys(entb) == entry_keys(ent) and infob["passes"] == 1
    B = 4
    S, Cn, ent, info, wi = run_job(pdel, lo, hi, B, 2, SLAB)
    Sb, Cb, entb, infob, wib = run_job(pdel, lo, hi, B, 2, dict(SLAB, win_max_bytes=12 * per_plane + 65536))
    assert wib["batches"] > wi["batches"] and wib["windows_by_pass"] == 0
    assert np.array_equal(Cn, Cb) and within(Sb, S, 1e-12) and within(Sb, job_oracle(pdel, lo, hi, B)[1])
    check_list(entb, infob)
    assert entry_keys(entb) == entry_keys(ent)


def test_a_list_that_overflows_grows_and_the_batch_runs_once_more():
    lo, hi = STEP
    S, Cn, ent, info, _ = run_windows(False, lo, hi, 1, SLAB)
    S8, C8, ent8, info8, _ = run_windows(False, lo, hi, 1, dict(SLAB, em_exact_cap=8))
    assert info["passes"] == 1 and info8["passes"] == 2 and info8["noted"] == info["noted"] > 8
    assert np.array_equal(S.view(np.uint64), S8.view(np.uint64)) and np.array_equal(Cn, C8)
    assert ent.tobytes() == ent8.tobytes()
    S, Cn, ent, info, _ = run_job(False, lo, hi, 4, 2, SLAB)
    S8, C8, ent8, info8, _ = run_job(False, lo, hi, 4, 2, dict(SLAB, em_exact_cap=8))
    assert info["passes"] == 1 and info8["passes"] == 2 and info8["noted"] == info["noted"] > 8
    assert np.array_equal(S.view(np.uint64), S8.view(np.uint64)) and np.array_equal(Cn, C8)
    assert ent.tobytes() == ent8.tobytes()


@pytest.mark.parametrize("pdel", [False, True])
def test_the_per_window_plan(pdel):
    """NGD_OPT_WIN_PLAN = 1: under value 2 every window goes through the noting plans of a multiplicity vector; under value 1
    the call is refused and computes nothing"""
    lo, hi = STEP
    So, Co = win_oracle(pdel, lo, hi)
    S, Cn, _, _, _ = run_windows(pdel, lo, hi, 2, SLAB)
    Sp, Cp, entp, infop, wip = run_windows(pdel, lo, hi, 2, dict(win_plan=1))
    assert wip["windows_by_pass"] == len(lo) and wip["batches"] == 0
    assert np.array_equal(Cp, Co) and within(Sp, So) and within(Sp, S, 1e-12)
    check_list(entp, infop)
    B = 4
    maps, Sjo, Cjo = job_oracle(pdel, lo, hi, B)
    Sj = run_job(pdel, lo, hi, B, 2, SLAB)[0]
    Sjp, Cjp, entj, infoj, wij = run_job(pdel, lo, hi, B, 2, dict(win_plan=1))
    assert wij["windows_by_pass"] == len(lo)
    assert np.array_equal(Cjp, Cjo) and within(Sjp, Sjo) and within(Sjp, Sj, 1e-12)
    check_list(entj, infoj)
    import torch
    n_pairs = N().n_pairs(N_IND)
    ds = torch.full((len(lo), n_pairs), -7.0, dtype=torch.float64, device="cuda")
    dc = torch.full((len(lo), n_pairs), 77, dtype=torch.int64, device="cuda")
    with engine(pdel, dict(win_plan=1)) as e:
        e.set_option("em_exact", 1)
        e.set_option("em_exact_win", 1)
        for call in (lambda: e.run_windows(lo, hi), lambda: e.run_windows(lo, hi, d_sum_ptr=ds.data_ptr(), d_cnt_ptr=dc.data_ptr())):
            with pytest.raises(N().NgdError) as ei:
                call()
            assert ei.value.code == -1 and "NGD_OPT_EM_EXACT_WIN" in str(ei.value) and "nothing was computed" in str(ei.value)
        torch.cuda.synchronize()
        assert bool(torch.all(ds == -7.0)) and bool(torch.all(dc == 77))  # nothing is written
        e.set_option("win_plan", 0)  # ... and the engine serves the call by the slab
        S1, C1 = e.run_windows(lo, hi)
        assert np.array_equal(C1, Co) and within(S1, So)


def test_another_kernel_shape():
    """variant = 1 .. 4 (4 wavefronts x 16 rows, rows only; 12 steps per round; shape 0 scanned row by row): each its own
    instantiation of the noting slice-table form, without and with --pairwise_del"""
    lo, hi = STEP
    for pdel in (False, True):
        So, Co = win_oracle(pdel, lo, hi)
        keys0 = entry_keys(run_windows(pdel, lo, hi, 1, SLAB)[2])
        for variant in (1, 2, 3, 4):
            S0 = run_windows(pdel, lo, hi, 0, SLAB, variant=variant)[0]
            S, Cn, ent, info, _ = run_windows(pdel, lo, hi, 1, SLAB, variant=variant)
            assert np.array_equal(Cn, Co) and within(S, So) and missed(S0, So) > 0, (pdel, variant)
            check_list(ent, info)
            quiet = quiet_cells(ent, lo, hi)
            assert np.array_equal(S[quiet].view(np.uint64), S0[quiet].view(np.uint64)), (pdel, variant)
            assert entry_keys(ent) == keys0, (pdel, variant)  # the list does not depend on the shape


def test_engines_of_32_individuals_or_fewer():
    """kernel = auto resolves to the per-pair kernel there; NGD_OPT_EM_EXACT moves the engine to the table-driven one, and the
    windows follow: one window that holds a probe and one that holds none"""
    g1, g2_of, _ = CASES[1]
    a, b, na, nb = boundaries()[1]
    p = O.synth_indmajor(9, 20, 300)
    p[3, 17], p[11, 17] = g1, g2_of(a)
    p[4, 200], p[5, 200] = g1, g2_of(b)
    lo, hi = [10, 100], [40, 160]
    So = [oracle_pairs(np.ascontiguousarray(p[:, x:y])) for x, y in zip(lo, hi)]
    for order in ((("em_exact", 1), ("em_exact_win", 1)), (("em_exact_win", 1), ("em_exact", 2))):  # (in either order)
        with N().Engine(20, 300, indep_geno=False) as e:
            e.upload_ind_major(p).commit()
            for name, value in order:
                e.set_option(name, value)
            S, Cn = e.run_windows(lo, hi)
            keys = entry_keys(e.em_exact_entries())
        assert (3, 11, 17) in keys and all(10 <= site < 40 for _, _, site in keys)  # (the second window is quiet)
        for w in range(2):
            assert np.array_equal(Cn[w], So[w][1]) and within(S[w], So[w][0])


def test_refusals_lifecycle_and_nothing_leaks():
    Nn = N()
    L = Nn._lib.load()
    lo, hi = STEP
    maps = job_maps(4)
    So, Co = win_oracle(False, lo, hi)

    def refused(fn, *words):
        with pytest.raises(Nn.NgdError) as ei:
            fn()
        assert ei.value.code == -1 and all(w in str(ei.value) for w in words), str(ei.value)

    def free_now():
        f, t = C.c_uint64(), C.c_uint64()
        assert L.ngd_device_memory(-1, C.byref(f), C.byref(t)) == 0
        return f.value

    with Nn.Engine(N_IND, N_SITES, indep_geno=True) as e:  # not an EM engine
        refused(lambda: e.set_option("em_exact_win", 1), "NGD_OPT_EM_EXACT_WIN")
        e.set_option("em_exact_win", 0)
    with Nn.Engine(N_IND, N_SITES, indep_geno=False, kernel="em_fast") as e:
        refused(lambda: e.set_option("em_exact_win", 1), "NGD_OPT_EM_EXACT_WIN")
    S_off, C_off, _, _, _ = run_windows(False, lo, hi, 0)
    Sj_off = run_job(False, lo, hi, 4, 0)[0]
    with engine(False) as e:
        refused(lambda: e.set_option("em_exact_win", 2), "NGD_OPT_EM_EXACT_WIN is 0 or 1")
        e.set_option("em_exact_win", 1)  # on its own: nothing changes
        S, Cn = e.run_windows(lo, hi)
        assert np.array_equal(S.view(np.uint64), S_off.view(np.uint64)) and np.array_equal(Cn, C_off)
        assert len(e.em_exact_entries()) == 0 and e.last_em_exact()["noted"] == 0
        Sj, _ = e.run_windows_job(lo, hi, maps, 4)
        assert np.array_equal(Sj.view(np.uint64), Sj_off.view(np.uint64)) and len(e.em_exact_entries()) == 0
        e.set_option("em_exact", 1)  # value 1: the windows, not the replicates
        S, Cn = e.run_windows(lo, hi)
        assert within(S, So) and len(e.em_exact_entries()) > 0
        refused(lambda: e.run_windows_job(lo, hi, maps, 4), "NGD_OPT_EM_EXACT_WIN", "NGD_OPT_EM_EXACT = 2")
        refused(lambda: e.run_windows_job_dist(lo, hi, maps, 4), "NGD_OPT_EM_EXACT_WIN", "NGD_OPT_EM_EXACT = 2")
        e.set_option("em_exact_win", 0)  # back to 0: the refusal of NGD_OPT_EM_EXACT alone, in its words
        refused(lambda: e.run_windows(lo, hi), "NGD_OPT_EM_EXACT is on", "not served")
        refused(lambda: e.run_windows_job(lo, hi, maps, 4), "NGD_OPT_EM_EXACT is on", "not served")
        e.set_option("em_exact", 2)
        refused(lambda: e.run_windows(lo, hi), "NGD_OPT_EM_EXACT is on", "not served")
        e.set_option("em_exact_win", 1)
        Sj, _ = e.run_windows_job(lo, hi, maps, 4)
        assert within(Sj, job_oracle(False, lo, hi, 4)[1])
    base = None
    for rnd in range(21):
        with engine(False, dict(win_plan=1 + rnd % 2)) as e:
            e.set_option("em_exact", 2)
            e.set_option("em_exact_win", 1)
            S, Cn = e.run_windows_job(lo, hi, maps, 4) if rnd % 3 else e.run_windows(lo, hi)
            assert np.all(np.isfinite(S))
        if rnd == 0:
            base = free_now()  # (after a warm-up round: the runtime's own pools)
    leaked = base - free_now()
    assert leaked < (64 << 20), "device memory not returned: %d MiB" % (leaked >> 20)


def printed_blocks(text, n_ind):
    """the matrices of a .dist file, block by block: [n_blocks][n_pairs]"""
    rows = [ln.split("\t") for ln in text.splitlines()]
    rows = [[float(x) for x in r[1:]] for r in rows if len(r) == n_ind + 1]
    assert rows and len(rows) % n_ind == 0
    iu = np.triu_indices(n_ind, 1)
    return np.stack([np.array(rows[k:k + n_ind])[iu] for k in range(0, len(rows), n_ind)])


@pytest.mark.parametrize("boot", [False, True])
def test_host_flag_prints_the_oracles_cells(tmp_path, boot):
    """ngsDist --em_exact_win --win_size 16 --win_step 8 on the planted set as a binary file, and once more with three
    replicates inside every window: every printed cell within the print's granularity of what the reference's flow gives on
    the file cut down to the window"""
    p = planted(False)[0]
    raw = np.ascontiguousarray(p.transpose(1, 0, 2))  # the file's order: [site][individual][3]
    path = tmp_path / "planted.bin"
    raw.tofile(str(path))
    lo, hi = N().window_ranges(N_SITES, 16, 8)
    assert (list(lo), list(hi)) == STEP
    R = 3 if boot else 0
    want = []
    hooked = O.ref_lib() is not None and O.use_reference_em2(True)
    try:
        for a, b in zip(lo, hi):
            pp = O.prep_binary(raw[a:b].reshape(-1), N_IND, b - a)
            _, raws = O.run_reference_flow(pp, indep_geno=False, n_boot_rep=R, boot_block_size=4, seed=7, raw=True, n_threads=8)
            want += [d for _, _, d in raws]
    finally:
        if hooked:
            O.use_reference_em2(False)
    do = np.stack(want)
    out = str(tmp_path / "o.dist")
    args = [BIN, "--geno", str(path), "--probs", "--n_ind", str(N_IND), "--n_sites", str(N_SITES), "--prep", "host",
            "--em_exact_win", "--win_size", "16", "--win_step", "8", "--out", out, "--verbose", "1"]
    if boot:
        args += ["--win_boot_rep", "3", "--boot_block_size", "4", "--seed", "7"]
    r = subprocess.run(args, capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    assert b"em_exact_win: true" in r.stderr and b"==> em_exact: " in r.stderr
    assert int(r.stderr.split(b"==> em_exact: ")[1].split()[0]) >= 100
    with open(out) as fh:
        d = printed_blocks(fh.read(), N_IND)
    assert d.shape == do.shape
    fin = np.isfinite(do)
    assert np.array_equal(np.isnan(d), np.isnan(do))
    assert np.all(np.abs(d[fin] - do[fin]) <= 1e-9 * np.abs(do[fin]) + 1e-10), np.max(np.abs(d[fin] - do[fin]))
