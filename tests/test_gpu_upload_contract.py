"""The upload contract of include/ngsdist_amd.h: before a successful ngd_commit, sites may be written any number of times,
by any of the upload paths (ngd_upload_sites, ngd_upload_ind_major, ngd_upload_raw_sites, ngd_stage_acquire / submit), in
any order, and each site holds the last values written to it -- whether it is missing included (the --pairwise_del mask).
After NGD_E_NAN the engine takes a fresh upload, and the full-data pass started beside a staged load (NGD_OPT_EAGER_FULL)
never keeps slices of sites that were written again.

Every test builds the final data set on the host (the raw path's sites prepared by the oracle's prep_binary) and checks the
engine against the oracle on it -- counts exact, sums to 1e-9 relative -- and against the same engine loaded once, in order
(upload_ind_major; one upload_raw_sites where the sites came by the raw path), bit for bit."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from test_gpu_parity import N, _raw_gl, rel_err

pytestmark = pytest.mark.gpu

RTOL = 1e-9
N_IND, N_SITES = 70, 3000  # (two groups of 64 individuals; 47 mask words)
CFG = {"mfma": dict(kernel="mfma", indep_geno=True), "stream": dict(kernel="stream", indep_geno=True),
       "em_fast": dict(kernel="em_fast", indep_geno=False), "em_table": dict(kernel="em_table", indep_geno=False),
       "mfma_single": dict(kernel="mfma", indep_geno=True, single_image=1)}
HOST, RAW = 1, 2  # how a site was last written: prepared on the host / raw, prepared on the device
_ORACLE = {}


def oracle(tag, p, pairwise_del, indep, block=None):
    """O.all_pairs, once per (data set, flags, replicate): `tag` names the data set p"""
    key = (tag, pairwise_del, indep, None if block is None else (block[0].tobytes(), block[1]))
    if key not in _ORACLE:
        kw = {} if block is None else dict(site_src=O.boot_site_src(*block), n_sites=len(block[0]) * block[1])
        _ORACLE[key] = O.all_pairs(p, pairwise_del=pairwise_del, indep_geno=indep, n_threads=16, **kw)
    return _ORACLE[key]


def prep(**kw):
    from ngsdist_amd import _lib
    return _lib.NgdPrep(int(kw.get("in_logscale", False)), int(kw.get("call_geno", False)), float(kw.get("N_thresh", 0.0)),
                        float(kw.get("call_thresh", 0.0)))


def stage(e, raw, s0, **kw):
    """raw sites [s0, s0 + len(raw)) through ngd_stage_acquire / ngd_stage_submit themselves: one piece per buffer"""
    from ngsdist_amd.engine import _check
    pr = prep(**kw)
    n, done = raw.shape[0], 0
    while done < n:
        buf, cap = C.POINTER(C.c_double)(), C.c_uint64()
        _check(e._L.ngd_stage_acquire(e._h, C.byref(buf), C.byref(cap)))
        c = min(int(cap.value), n - done)
        assert c > 0
        np.ctypeslib.as_array(buf, shape=(c * e.n_ind * 3,))[:] = raw[done:done + c].reshape(-1)
        _check(e._L.ngd_stage_submit(e._h, s0 + done, c, C.byref(pr)))
        done += c


def apply(e, ops, **kw):
    """ops: (path, s0, block) in order; block is site-major, prepared for "sites", raw for "raw" / "stage" """
    for path, s0, block in ops:
        block = np.ascontiguousarray(block)
        if path == "sites":
            e.upload_sites(block, s0)
        elif path == "raw":
            e.upload_raw_sites(block, s0, **kw)
        else:
            stage(e, block, s0, **kw)
    return e


def final_of(ops, n_ind, n_sites, **kw):
    """what each site holds after ops: (p [n_ind][n_sites][3] as gen_dist reads it, how each site came, its values)"""
    kind = np.zeros(n_sites, dtype=np.int8)
    val = np.zeros((n_sites, n_ind, 3))
    for path, s0, block in ops:
        kind[s0:s0 + len(block)] = HOST if path == "sites" else RAW
        val[s0:s0 + len(block)] = block
    assert np.all(kind != 0)
    p = val.copy()
    r = np.flatnonzero(kind == RAW)
    if r.size:
        p[r] = O.prep_binary(val[r], n_ind, r.size, **kw).transpose(1, 0, 2)
    return np.ascontiguousarray(p.transpose(1, 0, 2)), kind, val


def load_once(e, p, kind, val, **kw):
    """the same final data set in ONE in-order load: upload_ind_major, one upload_raw_sites, or in-order runs of both"""
    if np.all(kind == HOST):
        return e.upload_ind_major(p)
    if np.all(kind == RAW):
        return e.upload_raw_sites(val, 0, **kw)
    cut = np.flatnonzero(np.diff(kind)) + 1
    for a, b in zip(np.r_[0, cut], np.r_[cut, len(kind)]):
        if kind[a] == HOST:
            e.upload_sites(np.ascontiguousarray(p[:, a:b].transpose(1, 0, 2)), int(a))
        else:
            e.upload_raw_sites(val[a:b], int(a), **kw)
    return e


def check(s, c, so, co, exact=False, tag=""):
    assert np.array_equal(c, co), ("counts", tag)
    if exact:
        assert np.array_equal(s, so), ("sums", tag)
    else:
        assert rel_err(s, so) < RTOL, ("sums", tag, rel_err(s, so))


def same(a, b, tag=""):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), ("not the same bits", tag)


def pieces(rng, n_sites):
    """a partition of [0, n_sites): boundaries at 63, 64 and 65 within mask words, one-site pieces, random lengths up to a
    few hundred sites; in random order but for the piece that ends at n_sites - 1, which comes last"""
    cuts = {n_sites}
    for w in range(64, n_sites, 64 * 5):
        cuts.update({w - 1, w, w + 1})
    for s in rng.choice(n_sites - 2, 12, replace=False) + 1:
        cuts.update({int(s), int(s) + 1})  # a piece of one site
    cuts.update(int(x) for x in rng.integers(1, n_sites, n_sites // 200))
    cuts = sorted(x for x in cuts if 0 < x <= n_sites)
    out = list(zip([0] + cuts[:-1], cuts))
    head = [out[i] for i in rng.permutation(len(out) - 1)]
    return head + [out[-1]]


def engine(cfg, pairwise_del, n_ind=N_IND, n_sites=N_SITES, **opt):
    e = N().Engine(n_ind, n_sites, pairwise_del=pairwise_del, **CFG[cfg])
    for k, v in opt.items():
        e.set_option(k, v)
    return e


def raw_and_prepared(seed, n_ind=N_IND, n_sites=N_SITES):
    raw = _raw_gl(n_ind, n_sites, seed)
    return raw, np.ascontiguousarray(O.prep_binary(raw, n_ind, n_sites).transpose(1, 0, 2))  # both site-major


def is_miss(t):
    return (np.abs(t[..., 0] - t[..., 1]) < 1e-5) & (np.abs(t[..., 1] - t[..., 2]) < 1e-5)


# ---- 1. order and granularity -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", list(CFG))
@pytest.mark.parametrize("pairwise_del", [False, True])
def test_pieces_in_random_order_by_every_path(cfg, pairwise_del):
    """Seeded random pieces in random order: host-prepared (ngd_upload_sites), raw (ngd_upload_raw_sites), raw through the
    staging ring directly, and all three mixed within one load.  One-MiB buffers in a ring of two: it turns many times."""
    raw, pre = raw_and_prepared(31)
    rng = np.random.default_rng(32)
    cut = pieces(rng, N_SITES)
    mix = rng.integers(0, 3, len(cut))
    loads = {path: [(path, a, (pre if path == "sites" else raw)[a:b]) for a, b in cut] for path in ("sites", "raw", "stage")}
    loads["mixed"] = [(("sites", "raw", "stage")[m], a, (pre if m == 0 else raw)[a:b]) for (a, b), m in zip(cut, mix)]
    indep = CFG[cfg]["indep_geno"]
    for name, ops in loads.items():
        p, kind, val = final_of(ops, N_IND, N_SITES)
        with engine(cfg, pairwise_del, stage_piece_mib=1, stage_ring=2) as e:
            got = apply(e, ops).commit().run()
        with engine(cfg, pairwise_del) as e:
            want = load_once(e, p, kind, val).commit().run()
        check(*got, *oracle("pieces", p, pairwise_del, indep), tag=name)  # (the same p for every load)
        same(got, want, name)


@pytest.mark.parametrize("pairwise_del", [False, True])
def test_ind_major_upload_in_staging_chunks_over_an_earlier_load(pairwise_del):
    """ngd_upload_ind_major moves ~256 MiB of the caller's array at a time: here three chunks, whose boundaries fall inside
    mask words, over a data set that was loaded before (other values, other missing sites) -- against the same data set
    in random pieces of ngd_upload_sites"""
    n_ind, n_sites = 40, 600_000
    staging = (256 << 20) // (n_ind * 24)
    assert n_sites > 2 * staging and staging % 64 != 0
    p = O.synth_indmajor(41, n_ind, n_sites, miss_frac=0.08)
    old = O.synth_indmajor(42, n_ind, n_sites, miss_frac=0.3)
    with engine("mfma", pairwise_del, n_ind, n_sites) as e:
        e.upload_ind_major(old)
        got = e.upload_ind_major(p).commit().run()
    del old
    sm = np.ascontiguousarray(p.transpose(1, 0, 2))
    rng = np.random.default_rng(43)
    bounds = np.unique(np.r_[0, rng.integers(1, n_sites, 40), staging - 1, staging, staging + 1, n_sites])
    order = rng.permutation(len(bounds) - 1)
    with engine("mfma", pairwise_del, n_ind, n_sites) as e:
        for k in order:
            e.upload_sites(sm[bounds[k]:bounds[k + 1]], int(bounds[k]))
        want = e.commit().run()
    del sm
    check(*got, *oracle("ind-major", p, pairwise_del, True))
    same(got, want)


# ---- 2. writing sites again ------------------------------------------------------------------------------------------
def rewrites(path, raw, pre, seed):
    """a whole in-order load through `path`, then again: a few ranges with new likelihoods, single sites at word edges,
    and single cells flipped present -> missing, missing -> present and missing -> missing"""
    host = path == "sites"
    cur = (pre if host else raw).copy()
    ops = [(path, 0, cur.copy())]
    new_raw, new_pre = raw_and_prepared(seed)
    new = new_pre if host else new_raw
    rng = np.random.default_rng(seed)
    for a, b in ((5, 300), (1000, 1130), (N_SITES - 77, N_SITES)):
        cur[a:b] = new[a:b]
        ops.append((path, a, cur[a:b].copy()))
    for s in (0, 63, 64, 127, 128, 2047, 2048, N_SITES - 1):
        cur[s] = new[(s + 17) % N_SITES]
        ops.append((path, s, cur[s:s + 1].copy()))
    m = is_miss(cur)  # (raw: the missing cells are the equal triples, as after preparation)
    present, missing = np.argwhere(~m), np.argwhere(m)
    miss = rng.choice(len(missing), 48, replace=False)
    flips = [(present[rng.choice(len(present), 24, replace=False)], np.full(3, 1 / 3 if host else 0.25)),  # -> missing
             (missing[miss[:24]], np.array([0.6, 0.3, 0.1])),                                               # -> present
             (missing[miss[24:]], np.full(3, 0.5 if host else 0.7))]               # missing -> missing, other values
    for cells, t in flips:
        for s, i in cells:
            cur[s, i] = t
    for s in sorted({int(s) for cells, _ in flips for s, _ in cells}):
        ops.append((path, s, cur[s:s + 1].copy()))
    return ops


@pytest.mark.parametrize("cfg", ["mfma", "stream", "em_fast", "em_table"])
@pytest.mark.parametrize("path", ["sites", "raw", "stage"])
@pytest.mark.parametrize("pairwise_del", [False, True])
def test_sites_written_again_hold_their_last_values_and_missingness(cfg, path, pairwise_del):
    """Sites written twice or more hold their last values; under --pairwise_del a site that turns missing clears its bit
    of the mask (emit(), layout.hip), or the valid-site counts of its individual's pairs stay one too high"""
    raw, pre = raw_and_prepared(51)
    ops = rewrites(path, raw, pre, 52)
    p, kind, val = final_of(ops, N_IND, N_SITES)
    flips = is_miss(final_of(ops[:1], N_IND, N_SITES)[0]) != is_miss(p)
    assert flips.sum() >= 40  # (missingness of cells changed both ways)
    with engine(cfg, pairwise_del, stage_piece_mib=1, stage_ring=2) as e:
        got = apply(e, ops).commit().run()
    with engine(cfg, pairwise_del) as e:
        want = load_once(e, p, kind, val).commit().run()
    check(*got, *oracle("rewrite-" + ("sites" if path == "sites" else "raw"), p, pairwise_del, CFG[cfg]["indep_geno"]))
    same(got, want)


# ---- 3. a fresh load after NGD_E_NAN ----------------------------------------------------------------------------------
NAN_SHAPES = {"mfma": (392, 11_000), "em_table": (70, 4000)}


def nan_then_clean(n_ind, n_sites, call_geno=False):
    """data that fails (a NaN cell in a late piece) and the clean data loaded after it: the NaN cell's site and some early
    sites, present before, are missing in it"""
    rng = np.random.default_rng(n_ind)
    if call_geno:
        bad = rng.gamma(0.4, size=(n_sites, n_ind, 3)) + 1e-9  # (no ties: every genotype called, one-hot)
        clean = rng.gamma(0.4, size=(n_sites, n_ind, 3)) + 1e-9
    else:
        bad, clean = _raw_gl(n_ind, n_sites, 61), _raw_gl(n_ind, n_sites, 62)
    s_nan = n_sites - n_sites // 7
    early = np.r_[0, 1, 63, 64, 65, 200:260]
    bad[early] = rng.gamma(0.4, size=(len(early), n_ind, 3)) + 1e-9
    bad[s_nan] = rng.gamma(0.4, size=(n_ind, 3)) + 1e-9
    bad[s_nan, n_ind // 2, 1] = np.nan
    clean[np.r_[early, s_nan]] = 0.25  # missing (call_geno: a tie, left missing)
    return bad, clean


@pytest.mark.parametrize("kernel", list(NAN_SHAPES))
@pytest.mark.parametrize("pairwise_del", [False, True])
def test_fresh_staged_load_after_nan(kernel, pairwise_del):
    """ngd_commit() rejects the load with NGD_E_NAN; the same engine then takes clean data through the staged path: its
    full pass and a bootstrap replicate are the clean one-shot engine's bits -- nothing of the rejected load is kept (its
    missing-site bits, or slices of the full pass started beside it under NGD_OPT_EAGER_FULL)"""
    n_ind, n_sites = NAN_SHAPES[kernel]
    cfg = dict(kernel=kernel, indep_geno=kernel == "mfma", pairwise_del=pairwise_del)
    if kernel == "mfma":
        cfg.update(n_slices=64, single_image=3)  # (slices for the eager pass; two images)
    bad, clean = nan_then_clean(n_ind, n_sites)
    m = N().Taus(5).block_map(n_sites // 50)
    with N().Engine(n_ind, n_sites, **cfg) as e:
        e.upload_raw_sites(clean, 0).commit()
        want = e.run(), e.run(m, 50)
    p = O.prep_binary(clean, n_ind, n_sites)
    so = oracle("nan-" + kernel, p, pairwise_del, cfg["indep_geno"]), \
        oracle("nan-" + kernel, p, pairwise_del, cfg["indep_geno"], (m, 50))
    for eager in (0, 1):
        with N().Engine(n_ind, n_sites, **cfg) as e:
            e.set_option("stage_piece_mib", 1)
            e.set_option("eager_full", eager)
            stage(e, bad, 0)
            with pytest.raises(N().NgdError) as ei:
                e.commit()
            assert ei.value.code == -6
            stage(e, clean, 0)
            e.commit()
            got = e.run(), e.run(m, 50)
        for k in (0, 1):
            check(*got[k], *so[k], tag=(eager, k))
            same(got[k], want[k], (eager, k))


def test_fresh_staged_load_after_nan_called_genotypes_bit_exact():
    """the same with called genotypes (one-hot vectors, ties left missing): the oracle's bits"""
    n_ind, n_sites = 70, 4000
    bad, clean = nan_then_clean(n_ind, n_sites, call_geno=True)
    p = O.prep_binary(clean, n_ind, n_sites, call_geno=True)
    with N().Engine(n_ind, n_sites, kernel="mfma", pairwise_del=True) as e:
        e.set_option("stage_piece_mib", 1)
        stage(e, bad, 0, call_geno=True)
        with pytest.raises(N().NgdError) as ei:
            e.commit()
        assert ei.value.code == -6
        stage(e, clean, 0, call_geno=True)
        got = e.commit().run()
    check(*got, *oracle("nan-call", p, True, True), exact=True)


# ---- 4. eager slices and a piece submitted again ----------------------------------------------------------------------
EAGER_N_IND, EAGER_N_SITES = 392, 11_000


@pytest.mark.parametrize("seq", ["again_at_0", "again_mid_prefix", "jump_ahead_then_below"])
@pytest.mark.parametrize("pairwise_del", [False, True])
def test_eager_slices_and_a_piece_submitted_again(seq, pairwise_del):
    """NGD_OPT_EAGER_FULL, one-MiB pieces loaded in order (slices of the full pass start beside the load), then a piece
    submitted again with other data: at site 0 / inside the prefix the first slices cover / after a jump ahead (which
    leaves the slices valid) a piece below the prefix.  run() and a second run(): the bits of an engine without eager
    slices given the same sequence, and the oracle on the final data."""
    n_ind, n_sites = EAGER_N_IND, EAGER_N_SITES
    raw, new = _raw_gl(n_ind, n_sites, 71), _raw_gl(n_ind, n_sites, 72)
    cap = (1 << 20) // (n_ind * 24)
    again = 0 if seq == "again_at_0" else 700
    if seq == "jump_ahead_then_below":
        mid = n_sites // 2 // cap * cap
        ops = [("stage", a, raw[a:a + cap]) for a in range(0, mid, cap)]
        ops.append(("stage", 8000, new[8000:8000 + cap]))
        ops.append(("stage", again, new[again:again + cap]))
        ops += [("stage", a, raw[a:a + cap]) for a in range(mid, n_sites, cap)]
    else:
        ops = [("stage", a, raw[a:a + cap]) for a in range(0, n_sites, cap)]
        ops.append(("stage", again, new[again:again + cap]))
    p, _, _ = final_of(ops, n_ind, n_sites)
    res = {}
    for eager in (0, 1):
        with N().Engine(n_ind, n_sites, kernel="mfma", pairwise_del=pairwise_del, n_slices=64, single_image=3) as e:
            e.set_option("stage_piece_mib", 1)
            e.set_option("eager_full", eager)
            apply(e, ops).commit()
            res[eager] = e.run(), e.run()
    for k in (0, 1):
        check(*res[1][k], *oracle("eager-%d" % again, p, pairwise_del, True), tag=k)
        same(res[1][k], res[0][k], k)
        same(res[0][k], res[0][0])
