"""NGD_OPT_EM_EXACT: the plain pass of the table-driven EM kernel stops every (pair, site) where the reference does.

The kernels decide `fabs(lik - oldLik) < 0.001` (emOptim2.cpp:127) from ratios of power sums, and within rounding of the
tolerance may stop one EM step from the reference (tests/test_gpu_em_boundary.py pins that as "one of the two adjacent
iterates").  With the option on, the pass notes every stop within 2^-36 of the threshold, the host reruns those sites the
reference's way and the sums are patched: here every probe, inside the band too, must sit at the ORACLE's step.
Yardstick: the oracle's pair loop on the reference's own compiled em2() (oracle.use_reference_em2) where oracle/_ref is
built, the oracle's restatement (pinned to the same bits by tests/test_oracle_golden.py) otherwise.

test_planted_probes prints (pytest -s) how many of its planted in-band probes the engine with the option OFF decides
differently from the reference: the feature's reason to exist."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SC = O.DEFAULT_SCORE.reshape(3, 3)
RTOL = 1e-9  # the project's bar


def N():
    import ngsdist_amd
    return ngsdist_amd


def norm(v):
    v = np.asarray(v, dtype=np.float64)
    return v / v.sum()


def c_at(g1, g2, T):
    """score-weighted sum of the EM iterate after T steps (closed form of the single-site EM)"""
    f1, f2 = g1 ** T, g2 ** T
    return float((f1 / f1.sum()) @ SC @ (f2 / f2.sum()))


def find_boundary(g1, g2_of, lo, hi):
    """adjacent doubles a < b with different oracle iteration counts"""
    a, b = lo, hi
    na, nb = O.em2(g1, g2_of(a))[1], O.em2(g1, g2_of(b))[1]
    assert na != nb
    while np.nextafter(a, b) < b:
        m = 0.5 * (a + b)
        if O.em2(g1, g2_of(m))[1] == na:
            a = m
        else:
            b, nb = m, O.em2(g1, g2_of(m))[1]
    return a, b, na, nb


CASES = [
    # (g1, second individual as a function of x, bracket): stopping steps around 3, 18 (second table round), 34 (third)
    (norm([0.90, 0.08, 0.02]), lambda x: norm([x, 0.10, 0.05]), (0.5, 3.0)),
    (norm([0.6, 0.3, 0.1]), lambda x: norm([x, 0.25, 0.15]), (0.30, 0.60)),
    (norm([0.3503, 0.3315, 0.3182]), lambda x: norm([x, 0.3305, 0.3124]), (0.352, 0.40)),
]

_cache = {}


def boundaries():
    if "b" not in _cache:
        _cache["b"] = [find_boundary(g1, g2_of, lo, hi) for g1, g2_of, (lo, hi) in CASES]
    return _cache["b"]


def oracle_pairs(p, **kw):
    """the yardstick: the pair loop on the reference's own em2() where it is built"""
    hooked = O.ref_lib() is not None and O.use_reference_em2(True)
    try:
        return O.all_pairs(p, indep_geno=False, n_threads=8, **kw)
    finally:
        if hooked:
            O.use_reference_em2(False)


def entry_keys(ent):
    return {(int(x["i1"]), int(x["i2"]), int(x["site"])) for x in ent}


def test_classification_of_every_probe_at_and_around_the_boundary():
    """one site, individuals (2k, 2k+1) = probe k: per case a + k ulp for k in -64 .. 64 step 4 and the six far probes"""
    pairs, T_or, near, far6 = [], [], [], []
    for (g1, g2_of, _), (a, b, na, nb) in zip(CASES, boundaries()):
        assert abs(na - nb) == 1
        ulp = np.spacing(a)
        xs = [a + k * ulp for k in range(-64, 65, 4)]
        xs += [a - 4096 * ulp, a + 4096 * ulp, a * (1 - 1e-10), a * (1 + 1e-10), a * (1 - 1e-6), a * (1 + 1e-6)]
        for q, x in enumerate(xs):
            near.append(q < 33)
            far6.append(q >= 37)
            pairs.append((g1, g2_of(x)))
            T_or.append(O.em2(g1, g2_of(x))[1])
    assert len(pairs) == 3 * 39
    n_ind = 2 * len(pairs)
    p = np.zeros((n_ind, 1, 3))
    for k, (g1, g2) in enumerate(pairs):
        p[2 * k, 0], p[2 * k + 1, 0] = g1, g2
    so, co = oracle_pairs(p)
    with N().Engine(n_ind, 1, indep_geno=False) as e:
        e.set_option("em_exact", 1)
        s, c = e.upload_ind_major(p).commit().run()
        ent = e.em_exact_entries()
        info = e.last_em_exact()
    assert info["noted"] == len(ent) and info["passes"] == 1
    by_key = {(int(x["i1"]), int(x["i2"]), int(x["site"])): x for x in ent}
    for k, (g1, g2) in enumerate(pairs):
        idx = N().n_pairs(n_ind) - N().n_pairs(n_ind - 2 * k)  # pair (2k, 2k+1)
        want = c_at(g1, g2, T_or[k])
        assert abs(s[idx] - want) / want < 1e-12, (k, s[idx], want, T_or[k])  # the oracle's step, near probes included
        x = by_key.get((2 * k, 2 * k + 1, 0))
        if near[k]:
            assert x is not None and int(x["t_ref"]) == T_or[k], (k, x)
        if far6[k]:
            assert x is None, (k, x)
    # every other pair of the engine is a single site too: all of them at the reference's step
    assert np.array_equal(c, co) and np.max(np.abs(s - so) / np.abs(so)) < RTOL
    for x in ent:  # what the list says it is
        assert abs(x["c_ref"] - c_at(p[x["i1"], 0], p[x["i2"], 0], int(x["t_ref"]))) / x["c_ref"] < 1e-12


# ---- planted data set: 130 individuals (a diagonal and an off-diagonal 64-tile, and a third of two individuals) x 64 sites
N_IND, N_SITES = 130, 64


def planted(pdel):
    key = ("planted", pdel)
    if key in _cache:
        return _cache[key]
    p = O.synth_indmajor(5, N_IND, N_SITES, miss_frac=0.1 if pdel else 0.0)
    offs = [-8, -3, -1, 0, 1, 2, 5, 8]
    probes = []  # (i1, i2, site, case, g1, g2)
    spots = [(i, i + 65, i % N_SITES) for i in range(50)] + [(j, j + 1, (j + 32) % N_SITES) for j in range(0, 100, 2)]
    for q, (i1, i2, site) in enumerate(spots):
        case = q % 3
        g1, g2_of, _ = CASES[case]
        a = boundaries()[case][0]
        g2 = g2_of(a + offs[(q // 3) % len(offs)] * np.spacing(a))
        p[i1, site], p[i2, site] = g1, g2
        probes.append((i1, i2, site, case, g1, g2))
    gone = None
    if pdel:  # a planted site where one of the two is missing: the pair does not visit it
        i1, i2, site = probes[7][:3]
        p[i2, site] = 1.0 / 3
        gone = (i1, i2, site)
    so, co = oracle_pairs(p, pairwise_del=pdel)
    # a wrong step must not hide inside the tolerance: at every planted (pair, site) the two adjacent iterates differ by
    # more than 1e-6 of the pair's reference sum
    for i1, i2, site, case, g1, g2 in probes:
        if gone == (i1, i2, site):
            continue
        na, nb = boundaries()[case][2:]
        d = abs(c_at(g1, g2, na) - c_at(g1, g2, nb))
        assert d > 1e-6 * so[O_pair(i1, i2)], (i1, i2, site, d, so[O_pair(i1, i2)])
    _cache[key] = (p, probes, gone, so, co)
    return _cache[key]


def O_pair(i1, i2):
    return N_IND * i1 - i1 * (i1 + 1) // 2 + (i2 - i1 - 1)


def run_planted(pdel, exact, **kw):
    p = planted(pdel)[0]
    opts = kw.pop("options", {})
    with N().Engine(N_IND, N_SITES, indep_geno=False, pairwise_del=pdel, **kw) as e:
        e.upload_ind_major(p).commit()
        if exact:
            e.set_option("em_exact", 1)
        for k, v in opts.items():
            e.set_option(k, v)
        s, c = e.run()
        return s, c, e.em_exact_entries(), e.last_em_exact()


@pytest.mark.parametrize("pdel", [False, True])
def test_planted_probes(pdel):
    """100 in-band probes planted in a background of synthetic sites: every pair within 1e-9 of the oracle, pairs without a
    noted site bit-equal to the option-off pass, two runs identical.  Prints how many planted probes the option-OFF engine
    decides differently from the reference (sum off by more than 1e-9)."""
    p, probes, gone, so, co = planted(pdel)
    s0, c0, ent0, info0 = run_planted(pdel, False)
    assert len(ent0) == 0 and info0["noted"] == 0 and info0["passes"] == 0
    s, c, ent, info = run_planted(pdel, True)
    s2, c2, ent2, info2 = run_planted(pdel, True)
    assert np.array_equal(c, co) and np.array_equal(c0, co)
    err = np.abs(s - so) / np.abs(so)
    planted_idx = [O_pair(i1, i2) for i1, i2, site, *_ in probes if (i1, i2, site) != gone]
    off_wrong = int(np.sum(np.abs(s0[planted_idx] - so[planted_idx]) / np.abs(so[planted_idx]) > RTOL))
    print("pairwise_del=%d: noted %d, changed %d; worst pair %.3g (option off: %.3g); planted probes decided differently "
          "with the option off: %d of %d" % (pdel, info["noted"], info["changed"], err.max(),
                                             np.max(np.abs(s0 - so) / np.abs(so)), off_wrong, len(planted_idx)))
    assert err.max() < RTOL, (int(np.argmax(err)), err.max())
    keys = entry_keys(ent)
    noted_pairs = {O_pair(i1, i2) for i1, i2, _ in keys}
    quiet = np.array([k not in noted_pairs for k in range(len(s))])
    assert np.array_equal(s[quiet].view(np.uint64), s0[quiet].view(np.uint64))  # no entry: the bits of the option-off pass
    assert np.array_equal(s.view(np.uint64), s2.view(np.uint64)) and ent.tobytes() == ent2.tobytes()  # run to run
    assert info["passes"] == 1 and info["noted"] == len(ent) >= len(planted_idx)
    for i1, i2, site, *_ in probes:
        assert ((i1, i2, site) in keys) == ((i1, i2, site) != gone), (i1, i2, site)
    assert list(map(tuple, ent[["i1", "i2", "site"]].tolist())) == sorted(map(tuple, ent[["i1", "i2", "site"]].tolist()))


@pytest.mark.parametrize("kw", [dict(n_slices=2), dict(n_slices=7), dict(variant=1), dict(variant=2), dict(variant=3),
                                dict(variant=4)], ids=lambda kw: "-".join("%s%d" % kv for kv in kw.items()))
@pytest.mark.parametrize("pdel", [False, True])
def test_planted_probes_in_every_shape_and_slicing(pdel, kw):
    p, probes, gone, so, co = planted(pdel)
    s, c, ent, info = run_planted(pdel, True, **kw)
    s0, c0, _, _ = run_planted(pdel, False, **kw)
    assert np.array_equal(c, co)
    assert np.max(np.abs(s - so) / np.abs(so)) < RTOL
    keys = entry_keys(ent)
    noted_pairs = {O_pair(i1, i2) for i1, i2, _ in keys}
    quiet = np.array([k not in noted_pairs for k in range(len(s))])
    assert np.array_equal(s[quiet].view(np.uint64), s0[quiet].view(np.uint64))
    assert info["passes"] == 1
    for i1, i2, site, *_ in probes:
        assert ((i1, i2, site) in keys) == ((i1, i2, site) != gone)


def test_a_list_that_overflows_grows_and_the_pass_runs_once_more():
    s, c, ent, info = run_planted(False, True)
    s8, c8, ent8, info8 = run_planted(False, True, options=dict(em_exact_cap=8))
    assert info["passes"] == 1 and info8["passes"] == 2 and info8["noted"] == info["noted"] > 8
    assert np.array_equal(s.view(np.uint64), s8.view(np.uint64)) and np.array_equal(c, c8)
    assert ent.tobytes() == ent8.tobytes()


def test_calls_the_option_does_not_serve_are_refused_and_nothing_leaks():
    Nn = N()
    L = Nn._lib.load()
    p, probes, gone, so, co = planted(False)
    maps = np.stack([Nn.Taus(r).block_map(N_SITES // 4) for r in range(3)])

    def refused(fn):
        with pytest.raises(Nn.NgdError) as ei:
            fn()
        assert ei.value.code == -1 and "NGD_OPT_EM_EXACT" in str(ei.value), str(ei.value)

    def free_now():
        f, t = C.c_uint64(), C.c_uint64()
        assert L.ngd_device_memory(-1, C.byref(f), C.byref(t)) == 0
        return f.value

    base = None
    for rnd in range(21):
        with Nn.Engine(N_IND, N_SITES, indep_geno=False) as e:
            e.upload_ind_major(p).commit()
            e.set_option("em_exact", 1)
            if rnd % 5 == 0:
                refused(lambda: e.run(maps[0], 4))
                refused(lambda: e.run_job(maps, 4))
                refused(lambda: e.run_batch(maps, 4))
                refused(lambda: e.run_mult(np.ones(N_SITES // 4, dtype=np.uint32), 4))
                refused(lambda: e.run_windows([0, 16], [32, 64]))
                refused(lambda: e.run_windows_job([0, 32], [32, 64], maps[:, :8], 4))
                refused(lambda: e.run_job_dist(maps, 4))
            s, c = e.run()  # the engine stays usable
            assert np.array_equal(c, co) and np.max(np.abs(s - so) / np.abs(so)) < RTOL
            e.set_option("em_exact", 0)
            S, Cn = e.run_job(maps, 4)  # ... and serves them again with the option off
            assert np.array_equal(Cn[0], co) and np.all(np.isfinite(S))
        if rnd == 0:
            base = free_now()  # (after a warm-up round: the runtime's own pools)
    leaked = base - free_now()
    assert leaked < (64 << 20), "device memory not returned: %d MiB" % (leaked >> 20)
    with Nn.Engine(N_IND, N_SITES, indep_geno=True) as e:  # not an EM engine
        refused(lambda: e.set_option("em_exact", 1))
    for k in ("em_fast", "em_faithful"):
        with Nn.Engine(N_IND, N_SITES, indep_geno=False, kernel=k) as e:
            refused(lambda: e.set_option("em_exact", 1))
    with Nn.Engine(N_IND, N_SITES, indep_geno=False, n_slices=2) as e:  # (two slices: an engine the eager pass serves)
        e.set_option("eager_full", 1)
        refused(lambda: e.set_option("em_exact", 1))
    with Nn.Engine(N_IND, N_SITES, indep_geno=False) as e:
        e.set_option("em_exact", 1)
        refused(lambda: e.set_option("eager_full", 1))


def test_auto_means_the_table_kernel_at_any_number_of_individuals():
    """kernel = auto resolves to the per-pair kernel up to 32 individuals; with the option it is the table-driven one"""
    g1, g2_of, _ = CASES[1]
    a, b, na, nb = boundaries()[1]
    p = O.synth_indmajor(9, 20, 300)
    p[3, 17], p[11, 17] = g1, g2_of(a)
    p[4, 200], p[5, 200] = g1, g2_of(b)
    so, co = oracle_pairs(p)
    with N().Engine(20, 300, indep_geno=False) as e:
        e.upload_ind_major(p).commit()
        e.set_option("em_exact", 1)
        s, c = e.run()
        keys = entry_keys(e.em_exact_entries())
    assert (3, 11, 17) in keys and (4, 5, 200) in keys
    assert np.array_equal(c, co) and np.max(np.abs(s - so) / np.abs(so)) < RTOL


BIN = os.path.join(ROOT, "ngsdist_amd", "bin", "ngsDist")


def test_host_flag_prints_the_oracles_cells_and_refuses_what_it_does_not_serve(tmp_path):
    """ngsDist ... --em_exact on the planted set as a binary file: every printed cell is the oracle's; in site ranges too"""
    p = planted(False)[0]
    raw = np.ascontiguousarray(p.transpose(1, 0, 2))  # the file's order: [site][individual][3]
    path = tmp_path / "planted.bin"
    raw.tofile(str(path))
    pp = O.prep_binary(raw.reshape(-1), N_IND, N_SITES)  # what the host makes of the file (--prep host: the host's libm)
    hooked = O.ref_lib() is not None and O.use_reference_em2(True)
    try:
        exp = O.run_reference_flow(pp, indep_geno=False)
    finally:
        if hooked:
            O.use_reference_em2(False)
    base = [BIN, "--geno", str(path), "--probs", "--n_ind", str(N_IND), "--n_sites", str(N_SITES), "--prep", "host"]
    for extra in ([], ["--n_gpus", "2", "--same_device"]):
        out = str(tmp_path / "o.dist")
        r = subprocess.run(base + ["--em_exact", "--out", out, "--verbose", "1"] + extra, capture_output=True)
        assert r.returncode == 0, r.stderr.decode()
        assert b"em_exact: true" in r.stderr and b"==> em_exact: " in r.stderr
        noted = int(r.stderr.split(b"==> em_exact: ")[1].split()[0])
        assert noted >= 100
        with open(out) as fh:
            assert fh.read() == exp, extra
    for flags, msg in ((["--indep_geno"], b"not with --indep_geno / --call_geno"),
                       (["--call_geno"], b"not with --indep_geno / --call_geno"),
                       (["--n_boot_rep", "2"], b"cannot be combined with bootstrap replicates (--n_boot_rep)"),
                       (["--win_size", "16"], b"cannot be combined with windows (--win_size)")):
        r = subprocess.run(base + ["--em_exact", "--out", str(tmp_path / "x"), "--verbose", "0"] + flags, capture_output=True)
        assert r.returncode == 255 and msg in r.stderr, (flags, r.returncode, r.stderr)
