"""NGD_OPT_EM_EXACT = 2 / --em_exact_boot: bootstrap replicates -- block maps, multiplicities, batches and jobs -- on the EM
path stop every (pair, site) where the reference does.

The list of in-band (pair, site)s does not depend on the replicate, so the plan's one EM launch notes it (per-block
partials: the plain noting form over slices that are blocks; else the spilled-terms pass in its noting form) and matrix r
takes its multiplicity of the site's block times (c_ref - c_dev).  Data: the planted set of tests/test_gpu_em_exact.py
(130 individuals x 64 sites, 100 in-band probes on a diagonal tile, an off-diagonal tile and a third).  Yardstick per
matrix: the oracle's pair loop over the replicate's sites, on the reference's own compiled em2() where oracle/_ref is built.
Tolerance: 1e-9 relative, the project's bar, on every pair of every matrix; counts equal.

Block size 10 leaves 60 of the 64 sites to the replicates (7: 63), so probes planted on later sites weigh 0 in every
replicate and 1 in matrix 0.  With the smallest scratch the spilled-terms plan takes, a chunk is one k-group of four units:
4 x 10 = 40 sites at block size 10, i.e. two chunks for 64 sites; the other block sizes give three chunks or more.  Block
size 10 is therefore run once more on the WIDE set -- 64 synthetic sites in front of the planted 64: 128 sites, 120 of them
the replicates', four chunks, the probes on sites 120 .. 127 beyond the truncation.

A slab of per-block partial sums that the noting form filled is not the option-off cache (the noting form stops in-band
pairs at the widened threshold and only the matrices are patched): test_option_off_after_value_2_on_one_engine."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from test_gpu_em_exact import (BIN, CASES, N, N_IND, N_SITES, O_pair, RTOL, boundaries, c_at, entry_keys, oracle_pairs,
                               planted)

pytestmark = pytest.mark.gpu

N_REP = 5
SEEDS = [101 + r for r in range(N_REP)]  # (the planted-difference assertion of reference() holds for these: checked there)
PARTIALS = dict(boot_partials=2)
SPILL = dict(boot_partials=0, em_spill=2)
_cache = {}


def dataset(pdel, wide=False):
    """(p, probes, gone, n_sites): the planted set, or (wide) the same behind 64 more synthetic sites"""
    p, probes, gone, _, _ = planted(pdel)
    if not wide:
        return p, probes, gone, N_SITES
    key = ("wide", pdel)
    if key not in _cache:
        front = O.synth_indmajor(6, N_IND, N_SITES, miss_frac=0.1 if pdel else 0.0)
        _cache[key] = (np.ascontiguousarray(np.concatenate([front, p], axis=1)),
                       [(i1, i2, site + N_SITES, case, g1, g2) for i1, i2, site, case, g1, g2 in probes],
                       None if gone is None else (gone[0], gone[1], gone[2] + N_SITES), 2 * N_SITES)
    return _cache[key]


def job_maps(B, n_rep=N_REP, n_sites=N_SITES):
    return np.stack([N().Taus(s).block_map(n_sites // B) for s in SEEDS[:n_rep]])


def weights(maps, B, lead=True, n_sites=N_SITES):
    """[matrix][site]: the multiplicity of the site in the matrix (0 beyond the truncation of ngsDist.cpp:236)"""
    nb = maps.shape[1]
    w = np.zeros((len(maps) + (1 if lead else 0), n_sites))
    if lead:
        w[0] = 1
    for r, bm in enumerate(maps):
        m = np.bincount(bm.astype(np.int64), minlength=nb)
        w[r + (1 if lead else 0), :nb * B] = np.repeat(m, B)
    return w


def reference(pdel, B, wide=False):
    """the oracle's (sums, counts) of the full data + the N_REP replicates at block size B -- and, on the CPU, the feature's
    reason: at every planted (pair, site), in every matrix that draws it, the two adjacent iterates differ by more than
    1e-6 of that matrix's reference sum, so a wrong step cannot hide inside the tolerance"""
    key = (pdel, B, wide)
    if key in _cache:
        return _cache[key]
    p, probes, gone, n_sites = dataset(pdel, wide)
    so, co = oracle_pairs(p, pairwise_del=pdel) if wide else planted(pdel)[3:]
    maps = job_maps(B, n_sites=n_sites)
    S, Cn = [so], [co]
    for bm in maps:
        s, c = oracle_pairs(p, pairwise_del=pdel, site_src=O.boot_site_src(bm, B), n_sites=len(bm) * B)
        S.append(s)
        Cn.append(c)
    S, Cn = np.stack(S), np.stack(Cn)
    w = weights(maps, B, n_sites=n_sites)
    for i1, i2, site, case, g1, g2 in probes:
        if gone == (i1, i2, site):
            continue
        na, nb = boundaries()[case][2:]
        d = abs(c_at(g1, g2, na) - c_at(g1, g2, nb))
        for r in range(len(S)):
            if w[r, site]:
                assert d > 1e-6 * S[r, O_pair(i1, i2)], (B, r, i1, i2, site, d, S[r, O_pair(i1, i2)])
    _cache[key] = (maps, S, Cn, w)
    return _cache[key]


def run_job(pdel, B, exact, options, n_ind=N_IND, n_sites=N_SITES, p=None, maps=None, wide=False, **kw):
    if p is None:
        p, _, _, n_sites = dataset(pdel, wide)
    maps = reference(pdel, B, wide)[0] if maps is None else maps
    with N().Engine(n_ind, n_sites, indep_geno=False, pairwise_del=pdel, **kw) as e:
        e.upload_ind_major(p).commit()
        for k, v in options.items():
            e.set_option(k, v)
        if exact:
            e.set_option("em_exact", 2)
        S, Cn = e.run_job(maps, B)
        return S, Cn, e.em_exact_entries(), e.last_em_exact(), e.spill_timing()


def rel_err(S, So):
    return np.abs(S - So) / np.abs(So)


def quiet_mask(ent, w):
    """[matrix][pair]: the pair has no noted site of non-zero weight in the matrix"""
    q = np.ones((len(w), N().n_pairs(N_IND)), dtype=bool)
    for x in ent:
        q[w[:, int(x["site"])] != 0, O_pair(int(x["i1"]), int(x["i2"]))] = False
    return q


def check_job(pdel, B, options, min_chunks=0, wide=False):
    p, probes, gone, _ = dataset(pdel, wide)
    maps, So, Co, w = reference(pdel, B, wide)
    S0, C0, ent0, info0, _ = run_job(pdel, B, False, options, wide=wide)
    assert len(ent0) == 0 and info0["noted"] == 0
    S, Cn, ent, info, spill = run_job(pdel, B, True, options, wide=wide)
    S2, C2, ent2, _, _ = run_job(pdel, B, True, options, wide=wide)
    err = rel_err(S, So)
    print("pairwise_del=%d B=%d %s: noted %d, changed %d, chunks %d; worst cell %.3g (option off: %.3g, %d cells beyond 1e-9)"
          % (pdel, B, options, info["noted"], info["changed"], spill["chunks"], err.max(), rel_err(S0, So).max(),
             int(np.sum(rel_err(S0, So) > RTOL))))
    assert np.array_equal(Cn, Co) and np.array_equal(C0, Co)
    assert err.max() < RTOL, (np.unravel_index(int(np.argmax(err)), err.shape), err.max())
    quiet = quiet_mask(ent, w)
    assert np.array_equal(S[quiet].view(np.uint64), S0[quiet].view(np.uint64))  # quiet cells: the bits of the option-off job
    assert np.array_equal(S.view(np.uint64), S2.view(np.uint64)) and ent.tobytes() == ent2.tobytes()  # run to run
    assert info["passes"] == 1 and info["noted"] == len(ent)
    keys = entry_keys(ent)
    for i1, i2, site, *_ in probes:
        assert ((i1, i2, site) in keys) == ((i1, i2, site) != gone), (i1, i2, site)
    order = list(map(tuple, ent[["i1", "i2", "site"]].tolist()))
    assert order == sorted(order) and len(set(order)) == len(order)
    if "em_spill" in options:
        assert spill["chunks"] >= max(1, min_chunks) and spill["matrices"] == N_REP + 1
    else:
        assert spill["chunks"] == 0  # (per-block partials served it)
    return spill


@pytest.mark.parametrize("B", [1, 4, 7, 10])
@pytest.mark.parametrize("pdel", [False, True])
def test_job_by_per_block_partials(pdel, B):
    check_job(pdel, B, PARTIALS)


@pytest.mark.parametrize("B", [1, 4, 7, 10])
@pytest.mark.parametrize("pdel", [False, True])
def test_job_by_spilled_terms_in_one_chunk_and_in_several(pdel, B):
    spill = check_job(pdel, B, SPILL)
    # the smallest scratch the plan takes: two k-groups of terms (one of them the operand run-ahead's tail), i.e. chunks of
    # one k-group = 4 units of the block size's largest divisor up to 64 -- 4, 16, 28 and 40 sites
    small = dict(SPILL, em_spill_bytes=int(spill["slot_groups"]) * 512 * 5 // 2)
    want = {1: 16, 4: 4, 7: 3, 10: 2}[B]
    got = check_job(pdel, B, small, min_chunks=want)
    assert got["chunks"] == want and (want >= 3 or B == 10)


@pytest.mark.parametrize("pdel", [False, True])
def test_truncating_block_size_in_four_chunks(pdel):
    """block size 10 on the wide set (128 sites, 120 the replicates'): chunks of 40 sites, so the truncation at site 120 and
    the probes beyond it fall in the last of four chunks; by per-block partials too (the lead matrix's own pass there)"""
    spill = check_job(pdel, 10, SPILL, wide=True)
    small = dict(SPILL, em_spill_bytes=int(spill["slot_groups"]) * 512 * 5 // 2)
    assert check_job(pdel, 10, small, min_chunks=3, wide=True)["chunks"] == 4
    check_job(pdel, 10, PARTIALS, wide=True)


@pytest.mark.parametrize("B", [4, 10])
def test_option_off_after_value_2_on_one_engine(B):
    """value 2 makes its per-block partial sums with the noting form; the option-off job that follows on the SAME engine, same
    geometry, must not be reduced from that slab: its bits are a fresh option-off engine's -- and the other way round, a value
    2 job after an option-off one makes its own"""
    p = planted(False)[0]
    maps, So, Co, w = reference(False, B)
    S_off = run_job(False, B, False, PARTIALS)[0]
    S_on = run_job(False, B, True, PARTIALS)[0]
    assert not np.array_equal(S_off.view(np.uint64), S_on.view(np.uint64))
    with N().Engine(N_IND, N_SITES, indep_geno=False) as e:
        e.upload_ind_major(p).commit()
        e.set_option("boot_partials", 2)
        for on in (2, 0, 0, 2, 0):
            e.set_option("em_exact", on)
            S, Cn = e.run_job(maps, B)
            assert np.array_equal(S.view(np.uint64), (S_on if on else S_off).view(np.uint64)), on
            assert (len(e.em_exact_entries()) > 0) == (on != 0)


def test_the_option_off_job_misses_planted_cells():
    """the feature's reason (pytest -s): how many (matrix, pair) cells the option-off job has beyond 1e-9 of the oracle --
    reference() has asserted, with the oracle alone, that a wrong step at a planted site is worth more than 1e-6 there"""
    for B in (1, 10):
        maps, So, Co, w = reference(False, B)
        S0 = run_job(False, B, False, SPILL)[0]
        S = run_job(False, B, True, SPILL)[0]
        print("block size %d: option off, %d of %d (matrix, pair) cells beyond 1e-9 (worst %.3g); option 2: %d (worst %.3g)"
              % (B, int(np.sum(rel_err(S0, So) > RTOL)), S0.size, rel_err(S0, So).max(), int(np.sum(rel_err(S, So) > RTOL)),
                 rel_err(S, So).max()))
        assert rel_err(S, So).max() < RTOL


def test_the_other_calls():
    """run(map), run_mult, run_batch (maps and multiplicities) and run_job_dist under value 2; value 3 is refused"""
    B = 4
    p = planted(False)[0]
    maps, So, Co, w = reference(False, B)
    nb = N_SITES // B
    mult = np.stack([np.bincount(bm.astype(np.int64), minlength=nb) for bm in maps]).astype(np.uint32)
    for options in (PARTIALS, SPILL):
        with N().Engine(N_IND, N_SITES, indep_geno=False) as e:
            e.upload_ind_major(p).commit()
            for k, v in options.items():
                e.set_option(k, v)
            e.set_option("em_exact", 2)
            with pytest.raises(N().NgdError) as ei:
                e.set_option("em_exact", 3)
            assert ei.value.code == -1
            s, c = e.run(maps[0], B)
            assert np.array_equal(c, Co[1]) and rel_err(s, So[1]).max() < RTOL, options
            assert e.last_em_exact()["noted"] == len(e.em_exact_entries()) >= 90
            s, c = e.run_mult(mult[1], B)
            assert np.array_equal(c, Co[2]) and rel_err(s, So[2]).max() < RTOL, options
            S, Cn = e.run_batch(maps, B)
            assert np.array_equal(Cn, Co[1:]) and rel_err(S, So[1:]).max() < RTOL, options
            S, Cn = e.run_batch(mult=mult[:2], block_size=B)
            assert np.array_equal(Cn, Co[1:3]) and rel_err(S, So[1:3]).max() < RTOL, options
            d = e.run_job_dist(maps, B, 1)
            do = np.stack([O.finish(So[r], Co[r], 0, 1) for r in range(len(So))])
            fin = np.isfinite(do)  # (a cell the model cannot correct is the same non-finite value in both)
            assert np.array_equal(np.isnan(d), np.isnan(do)) and rel_err(d[fin], do[fin]).max() < RTOL, options
            assert e.last_em_exact()["noted"] == len(e.em_exact_entries()) >= 99
            s, c = e.run()  # the plain pass, as under value 1
            assert np.array_equal(c, Co[0]) and rel_err(s, So[0]).max() < RTOL


def test_a_list_that_overflows_grows_and_the_plan_runs_once_more():
    for options in (PARTIALS, SPILL):
        S, Cn, ent, info, _ = run_job(False, 4, True, options)
        S8, C8, ent8, info8, _ = run_job(False, 4, True, dict(options, em_exact_cap=8))
        assert info["passes"] == 1 and info8["passes"] == 2 and info8["noted"] == info["noted"] > 8
        assert np.array_equal(S.view(np.uint64), S8.view(np.uint64)) and np.array_equal(Cn, C8)
        assert ent.tobytes() == ent8.tobytes()


def test_engines_of_32_individuals_or_fewer():
    """kernel = auto resolves to the per-pair kernel there; the option moves the engine to the table-driven one and, for
    value 2, deals it the spilled-terms plan's pair slots"""
    g1, g2_of, _ = CASES[1]
    a, b, na, nb = boundaries()[1]
    p = O.synth_indmajor(9, 20, 300)
    p[3, 17], p[11, 17] = g1, g2_of(a)
    p[4, 200], p[5, 200] = g1, g2_of(b)
    B = 5
    maps = np.stack([N().Taus(s).block_map(300 // B) for s in SEEDS[:3]])
    So = [oracle_pairs(p)] + [oracle_pairs(p, site_src=O.boot_site_src(bm, B), n_sites=300) for bm in maps]
    for options in (PARTIALS, SPILL):
        S, Cn, ent, info, spill = run_job(False, B, True, options, n_ind=20, n_sites=300, p=p, maps=maps)
        keys = entry_keys(ent)
        assert (3, 11, 17) in keys and (4, 5, 200) in keys
        for r, (so, co) in enumerate(So):
            assert np.array_equal(Cn[r], co) and rel_err(S[r], so).max() < RTOL, (options, r)
        assert (spill["chunks"] > 0) == ("em_spill" in options)


def test_refusals_and_nothing_leaks():
    Nn = N()
    L = Nn._lib.load()
    p = planted(False)[0]
    maps, So, Co, w = reference(False, 4)

    def refused(fn, word):
        with pytest.raises(Nn.NgdError) as ei:
            fn()
        assert ei.value.code == -1 and "NGD_OPT_EM_EXACT" in str(ei.value) and word in str(ei.value), str(ei.value)

    def free_now():
        f, t = C.c_uint64(), C.c_uint64()
        assert L.ngd_device_memory(-1, C.byref(f), C.byref(t)) == 0
        return f.value

    with Nn.Engine(N_IND, N_SITES, indep_geno=False) as e:
        e.upload_ind_major(p).commit()
        e.set_option("em_exact", 2)
        refused(lambda: e.run_windows([0, 16], [32, 64]), "not served")
        refused(lambda: e.run_windows_job([0, 32], [32, 64], maps[:, :8], 4), "not served")
        S, Cn = e.run_job(maps, 4)
        assert rel_err(S, So).max() < RTOL
    with Nn.Engine(N_IND, N_SITES, indep_geno=False, variant=1) as e:  # another shape: no spilled-terms plan
        e.upload_ind_major(p).commit()
        e.set_option("em_exact", 2)
        e.set_option("boot_partials", 0)
        refused(lambda: e.run_job(maps, 4), "no plan that notes")
        refused(lambda: e.run(maps[0], 4), "no plan that notes")
        e.set_option("boot_partials", 2)  # ... and the engine is usable: per-block partials have the noting form in every shape
        S, Cn = e.run_job(maps, 4)
        assert np.array_equal(Cn, Co) and rel_err(S, So).max() < RTOL
    with Nn.Engine(N_IND, N_SITES, indep_geno=False) as e:
        e.upload_ind_major(p).commit()
        e.set_option("em_exact", 2)
        e.set_option("boot_partials", 0)
        e.set_option("em_spill", 0)
        refused(lambda: e.run_job(maps, 4), "no plan that notes")
        s, c = e.run()
        assert rel_err(s, So[0]).max() < RTOL
    base = None
    for rnd in range(21):
        with Nn.Engine(N_IND, N_SITES, indep_geno=False) as e:
            e.upload_ind_major(p).commit()
            e.set_option("em_exact", 2)
            for k, v in (PARTIALS if rnd % 2 else SPILL).items():
                e.set_option(k, v)
            S, Cn = e.run_job(maps, 4)
            assert np.all(np.isfinite(S))
        if rnd == 0:
            base = free_now()  # (after a warm-up round: the runtime's own pools)
    leaked = base - free_now()
    assert leaked < (64 << 20), "device memory not returned: %d MiB" % (leaked >> 20)


def printed_matrices(text, n_ind):
    rows = [[float(x) for x in ln.split("\t")[1:]] for ln in text.splitlines() if "\t" in ln]
    assert len(rows) % n_ind == 0 and all(len(r) == n_ind for r in rows)
    iu = np.triu_indices(n_ind, 1)
    return np.stack([np.array(rows[k:k + n_ind])[iu] for k in range(0, len(rows), n_ind)])


def test_host_flag_prints_the_oracles_cells(tmp_path):
    """ngsDist --em_exact_boot --n_boot_rep 3 on the planted set as a binary file, on one engine and in two site ranges:
    every printed cell within the print's granularity of the oracle's distance (cells, not bytes: four matrices of GL data
    have enough cells for a reordered sum to cross a %.10f rounding edge)"""
    p = planted(False)[0]
    raw = np.ascontiguousarray(p.transpose(1, 0, 2))  # the file's order: [site][individual][3]
    path = tmp_path / "planted.bin"
    raw.tofile(str(path))
    pp = O.prep_binary(raw.reshape(-1), N_IND, N_SITES)
    hooked = O.ref_lib() is not None and O.use_reference_em2(True)
    try:
        _, raws = O.run_reference_flow(pp, indep_geno=False, n_boot_rep=3, boot_block_size=4, seed=7, raw=True, n_threads=8)
    finally:
        if hooked:
            O.use_reference_em2(False)
    do = np.stack([d for _, _, d in raws])
    base = [BIN, "--geno", str(path), "--probs", "--n_ind", str(N_IND), "--n_sites", str(N_SITES), "--prep", "host",
            "--em_exact_boot", "--n_boot_rep", "3", "--boot_block_size", "4", "--seed", "7", "--verbose", "1"]
    for extra in ([], ["--n_gpus", "2", "--same_device"]):
        out = str(tmp_path / "o.dist")
        r = subprocess.run(base + ["--out", out] + extra, capture_output=True)
        assert r.returncode == 0, r.stderr.decode()
        assert b"em_exact_boot: true" in r.stderr and b"==> em_exact: " in r.stderr
        assert int(r.stderr.split(b"==> em_exact: ")[1].split()[0]) >= 100
        with open(out) as fh:
            d = printed_matrices(fh.read(), N_IND)
        assert d.shape == do.shape
        fin = np.isfinite(do)
        assert np.array_equal(np.isnan(d), np.isnan(do))
        assert np.all(np.abs(d[fin] - do[fin]) <= 1e-9 * np.abs(do[fin]) + 1e-10), (extra, np.max(np.abs(d[fin] - do[fin])))
