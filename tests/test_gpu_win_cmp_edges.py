"""The comparison of windows (win_cmp.hip, engine_win_cmp.hip, win_cmp_geom.h) where test_gpu_win_cmp.py stops short.

A. three and four block rows of tile blocks (W = 129, 130, 193, 200: k_wincmp_gram's triangular decode with t >= 2, and
   with bi >= 1 and t >= 1) against the extended-precision expectation and the host twin; the older file's bit properties
   at W = 193.  (130 because at 129 the third block row holds nothing but the maker's status-0 vector.)
B. slices longer than 256 cells (W = 2048, P = 1800: 260 cells a slice, 7 slices, the last of 240): every pair screened
   against numpy's FP64 product, a pair inside each of the 528 tile blocks and 4000 random pairs against the
   extended-precision expectation; position and company, and the scaling by 2^-7, bit for bit.
C. one slice over the whole cell axis (W = 5745, P = 300: 4095 tile blocks, 90 block rows), screened and sampled in the
   same way; the rule itself, and its rounding at (5745, 301), without a device.
D. the run form past 16 windows (41 and 70 windows of 20 individuals; groups of 7 and of 11 windows, so that w0 is no
   multiple of 16 and a group straddles a fragment of 16 vectors), against its siblings bit for bit; once on the EM path;
   once under --pairwise_del with windows 5, 16 and 40 without data.
E. cells that are not finite or extreme: +inf and -inf in a vector's first and last cell, a vector of large mean and tiny
   spread, one of cells near 2^-500; sums and counts on planted tensors whose cells are +inf or NaN under models 1 and 2
   (sum / cnt = 1, above 1, 3/4), with and without tot_sites.

Every comparison prints its largest figure in units of its bound.  The largest seen on an MI355X over the cases of this
file (bound 1e-9 each, 3e-9 for cor): gram 2.0e-15 of sqrt(exact[a][a] exact[b][b]), mean 3.1e-16 of mean |x|, rms^2 2.6e-15
of (exact[a][a] + exact[b][b] + P (mean[a] - mean[b])^2) / P, cor 2.9e-15 absolute, device against host twin 1.6e-15, device
against the FP64 screen 1.3e-15 (B) and 1.1e-15 (C).  The vector of large mean and tiny spread and the 2048 x 1800 case
stay at the older file's figures: that vector's cells and its mean lie in one binade, so the centring is exact and the
mean's rounding enters the diagonal squared.  C runs on the device (1.4 s there, most of it the host's passes over the
5745 x 5745 result), so nothing of it is left to the rule's CPU test alone.  The whole file takes 7 s.

The cell near 2^-500 exposed ngd_win_cmp_finish: cor[a][a] of that vector was +inf, because the product of the two
diagonals (2^-1000 each) underflowed before the root was taken (test_extreme_vectors_*; host_util.cpp)."""
import numpy as np
import pytest

import win_cmp_expect as X
from test_gpu_win_cmp import N, bits, check_finished, device_buffers, finish, on_device, same, synth, to_host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    with N().Engine(8, 16, kernel="mfma") as e:  # (the values form is not tied to the engine's n_ind)
        e.synth_fill(1).commit()
        yield e


def geometry(W, P):
    """win_cmp_geom.h's rule for the tiles, and the slice looked up: (n_gz, n_br, tile blocks, cells per slice, slices,
    cells of the last slice)"""
    n_g = (W + 15) // 16
    T = min(4, n_g)
    n_gz = (n_g + T - 1) // T * T
    n_br = n_gz // T
    s = N().win_cmp_slice(W, P)
    n_sl = (P + s - 1) // s
    return n_gz, n_br, n_br * (n_br + 1) // 2, s, n_sl, P - (n_sl - 1) * s


# ---- A. more block rows -----------------------------------------------------------------------------------------------------
# (at W = 129 the third block row holds the maker's status-0 vector alone, whose row is written from the status: 130 puts a
# finite vector there, so that the tile blocks with t = 2 are compared)
@pytest.mark.parametrize("W,n_gz,n_br,n_blk", [(129, 12, 3, 6), (130, 12, 3, 6), (193, 16, 4, 10), (200, 16, 4, 10)])
def test_three_and_four_block_rows_against_the_expectation_and_the_host_twin(engine, W, n_gz, n_br, n_blk):
    for P, n_sl, last in ((257, 2, 1), (515, 3, 3)):
        assert geometry(W, P) == (n_gz, n_br, n_blk, 256, n_sl, last)
        v, _ = X.vectors(W, P)
        exp = X.expect(v)
        mean, gram, status = on_device(engine, v)
        X.check_all(v, mean, gram, status, N().win_cmp_finish, "device", exp)
        X.check_twin(mean, gram, status, *N().win_cmp_host(v), exp, "W=%d P=%d" % (W, P))


def test_bits_across_four_block_rows(engine):
    W, P = 193, 515
    assert geometry(W, P) == (16, 4, 10, 256, 3, 3)
    v, at = X.vectors(W, P)
    first = on_device(engine, v)
    mean, gram, status = first
    assert same(on_device(engine, v), first)  # a repeated call
    # pairs move between tile blocks with t >= 2 and across the diagonal
    perm = np.random.default_rng(7).permutation(W)
    pm, pg, ps = on_device(engine, v[perm])
    assert np.array_equal(ps, status[perm]) and np.array_equal(bits(pm), bits(mean[perm]))
    assert np.array_equal(bits(pg), bits(gram[np.ix_(perm, perm)]))
    rm, rg, rs = on_device(engine, v[::-1])
    assert np.array_equal(rs, status[::-1]) and np.array_equal(bits(rm), bits(mean[::-1]))
    assert np.array_equal(bits(rg), bits(gram[::-1, ::-1]))
    # the status-0 vector replaced by a finite one: no bit outside its row and column changes
    w = v.copy()
    w[at["bad"]] = np.random.default_rng(8).random(P)
    fm, fg, fs = on_device(engine, w)
    keep = np.arange(W) != at["bad"]
    assert fs.tolist() == [1] * W
    assert np.array_equal(bits(fg[np.ix_(keep, keep)]), bits(gram[np.ix_(keep, keep)])) and np.array_equal(bits(fm[keep]), bits(mean[keep]))


# ---- B, C. slices longer than 256 cells; one slice ---------------------------------------------------------------------------
def pairs_in_every_tile_block(W, n_br, n_random, seed):
    """a pair (a, b) inside each tile block of 64 x 64 vectors on or above the diagonal, read as [a][b] and as [b][a], and
    n_random pairs anywhere"""
    r = np.random.default_rng(seed)
    out = []
    for bi in range(n_br):
        for bj in range(bi, n_br):
            a = min(W - 1, 64 * bi + int(r.integers(64)))
            b = min(W - 1, 64 * bj + int(r.integers(64)))
            out += [(a, b), (b, a)]
    return out + [(int(a), int(b)) for a, b in r.integers(0, W, (n_random, 2))]


def test_slices_longer_than_256_cells(engine):
    W, P = 2048, 1800
    assert N().win_cmp_slice(W, P) == 260
    assert geometry(W, P) == (128, 32, 528, 260, 7, 240)
    v, _ = X.vectors(W, P)
    rows = X.expect_rows(v)
    first = on_device(engine, v)
    mean, gram, status = first
    X.screen_all(v, mean, gram, status, "device", rows)
    pairs = pairs_in_every_tile_block(W, 32, 4000, 2048)
    assert len(pairs) == 2 * 528 + 4000
    X.check_pairs(v, mean, gram, status, N().win_cmp_finish, pairs, "device", rows)
    # position and company at fixed (W, P): vectors 0 .. 63 at the far end, the others permuted
    perm = np.concatenate([64 + np.random.default_rng(9).permutation(W - 64), np.arange(64)])
    pm, pg, ps = on_device(engine, v[perm])
    assert np.array_equal(ps, status[perm]) and ps[W - 64:].tolist() == [1] * 64
    assert np.array_equal(bits(pm[W - 64:]), bits(mean[:64])) and np.array_equal(bits(pg[W - 64:, W - 64:]), bits(gram[:64, :64]))
    assert np.array_equal(bits(pg), bits(gram[np.ix_(perm, perm)]))
    # scaling by a power of two is exact
    ok = status == 1
    m2, g2, s2 = on_device(engine, np.ldexp(v, -7))
    assert np.array_equal(s2, status) and np.array_equal(bits(m2[ok]), bits(np.ldexp(mean[ok], -7)))
    assert np.array_equal(bits(g2[:64, :64]), bits(np.ldexp(gram[:64, :64], -14)))
    assert np.array_equal(bits(g2[np.ix_(ok, ok)]), bits(np.ldexp(gram[np.ix_(ok, ok)], -14)))


def test_the_slice_rule_where_one_slice_covers_the_cell_axis():
    sl = N().win_cmp_slice
    assert geometry(5745, 300)[:3] == (360, 90, 4095)  # 4096 / 4095 = 1 wavefront per tile block is wanted: one slice
    assert sl(5745, 300) == 300 and sl(5745, 301) == 304 and sl(5745, 255) == 256
    assert sl(2048, 1800) == 260 and sl(2048, 1792) == 256 and sl(2048, 1793) == 260  # (want = 7: 256 cells up to P = 1792)


def test_one_slice_over_the_whole_cell_axis(engine):
    W, P = 5745, 300
    assert geometry(W, P) == (360, 90, 4095, 300, 1, 300)
    v, _ = X.vectors(W, P)
    rows = X.expect_rows(v)
    mean, gram, status = on_device(engine, v)
    X.screen_all(v, mean, gram, status, "device", rows)
    # a pair in each block of the first and of the last block row and of the diagonal, and 2000 anywhere
    r = np.random.default_rng(5745)
    blocks = [(0, bj) for bj in range(90)] + [(bi, bi) for bi in range(90)] + [(bi, 89) for bi in range(90)]
    pairs = [(min(W - 1, 64 * bi + int(r.integers(64))), min(W - 1, 64 * bj + int(r.integers(64)))) for bi, bj in blocks]
    pairs = pairs + [(b, a) for a, b in pairs] + [(int(a), int(b)) for a, b in r.integers(0, W, (2000, 2))]
    X.check_pairs(v, mean, gram, status, N().win_cmp_finish, pairs, "device", rows)


# ---- D. the run form past 16 windows -----------------------------------------------------------------------------------------
N_IND, SIZE = 20, 8
N_PAIRS = N_IND * (N_IND - 1) // 2


def windows(n_win):
    lo, hi = N().window_ranges(n_win * SIZE, SIZE)
    assert len(lo) == n_win
    return lo, hi


def cut_into_groups(monkeypatch, per_group, n_win):
    """the hook of test_groups_of_windows_change_no_bit; -> the first window of every group by the driver's rule
    (engine_windows.hip windows_chunked: budget / (16 bytes x pairs) windows a group)"""
    budget = per_group * 16 * N_PAIRS
    monkeypatch.setenv("NGD_ENABLE_TEST_HOOKS", "1")
    monkeypatch.setenv("NGD_TEST_WIN_GROUP_BYTES", str(budget))
    per = max(1, min(n_win, budget // (16 * N_PAIRS)))
    assert per == per_group and per % 16 != 0
    w0 = list(range(0, n_win, per))
    # a later group starts inside a fragment of 16 vectors, and a group straddles two fragments
    assert any(w % 16 for w in w0) and any(w // 16 != (min(w + per, n_win) - 1) // 16 for w in w0)
    return w0


def uncut(monkeypatch):
    monkeypatch.delenv("NGD_ENABLE_TEST_HOOKS", raising=False)
    monkeypatch.delenv("NGD_TEST_WIN_GROUP_BYTES", raising=False)


def same_run(a, b):
    """two (mean, gram, status, dist) results bit for bit"""
    return same(a[:3], b[:3]) and np.array_equal(bits(a[3]), bits(b[3]))


@pytest.mark.parametrize("n_win,kernel,n_gz,n_br", [(41, "mfma", 3, 1), (70, "mfma", 8, 2), (41, "em_table", 3, 1)])
def test_run_form_past_16_windows_whole_and_in_groups(n_win, kernel, n_gz, n_br, monkeypatch):
    lo, hi = windows(n_win)
    assert geometry(n_win, N_PAIRS)[:2] == (n_gz, n_br) and N_PAIRS == 190
    with N().Engine(N_IND, n_win * SIZE, kernel=kernel, indep_geno=kernel == "mfma") as e:
        e.upload_ind_major(synth(41, N_IND, n_win * SIZE)).commit()
        e.set_option("win_plan", 1)
        uncut(monkeypatch)
        one = e.run_windows_cmp(lo, hi, evol_model=1)
        assert one[2].tolist() == [1] * n_win
        # the siblings
        ds, dc = device_buffers((n_win, N_PAIRS))
        e.run_windows(lo, hi, d_sum_ptr=ds.data_ptr(), d_cnt_ptr=dc.data_ptr())
        assert same(one[:3], e.win_cmp(ds.data_ptr(), dc.data_ptr(), n_win, evol_model=1))
        assert np.array_equal(bits(one[3]), bits(e.run_windows_dist(lo, hi, 1)))
        S, Cn = to_host(ds, dc)
        d = finish(S, Cn, 1)
        assert np.array_equal(bits(one[3]), bits(d))
        check_finished(one[:3], d, "run form, %d windows, %s" % (n_win, kernel))
        for per_group in (7, 11):
            w0 = cut_into_groups(monkeypatch, per_group, n_win)
            many = e.run_windows_cmp(lo, hi, evol_model=1)
            assert same_run(one, many), per_group
            # the hook did cut: under the segment-slab plan a batch does not span groups
            e.set_option("win_plan", 2)
            e.run_windows_cmp(lo, hi, evol_model=1, dist=False)
            assert e.windows_info()["batches"] >= len(w0)
            e.set_option("win_plan", 1)


def test_run_form_with_windows_without_data_under_pairwise_deletion(monkeypatch):
    n_win, gone = 41, (5, 16, 40)  # status-0 vectors at a fragment's first slot (16), inside a group (5) and last (40)
    lo, hi = windows(n_win)
    p = synth(43, N_IND, n_win * SIZE, miss_frac=0.05)
    for w in gone:
        p[:, int(lo[w]):int(hi[w]), :] = 1.0 / 3.0  # no data at these sites: every pair of the window is without a site
    with N().Engine(N_IND, n_win * SIZE, kernel="mfma", pairwise_del=True) as e:
        e.upload_ind_major(p).commit()
        e.set_option("win_plan", 1)
        uncut(monkeypatch)
        one = e.run_windows_cmp(lo, hi, evol_model=1)
        mean, gram, status, dist = one
        assert np.flatnonzero(status == 0).tolist() == list(gone)
        assert np.array_equal(np.isfinite(dist).all(axis=1), status == 1)
        check_finished(one[:3], dist, "run form, --pairwise_del")  # (status, the NaN rows and columns among it)
        S, Cn = e.run_windows(lo, hi)
        assert np.array_equal((Cn == 0).all(axis=1), status == 0) and np.array_equal(bits(dist), bits(finish(S, Cn, 1)))
        for per_group in (7, 11):
            cut_into_groups(monkeypatch, per_group, n_win)
            assert same_run(one, e.run_windows_cmp(lo, hi, evol_model=1)), per_group
        # the remaining windows alone, as a call of 38 vectors: another (W, P), so within the bound, not by bits -- but
        # the vectors' means are the sums of their own cells alone
        uncut(monkeypatch)
        keep = status == 1
        few = e.run_windows_cmp(lo[keep], hi[keep], evol_model=1)
        assert few[2].tolist() == [1] * 38 and np.array_equal(bits(few[0]), bits(mean[keep]))
        assert np.array_equal(bits(few[3]), bits(dist[keep]))


# ---- E. cells that are not finite, and extreme ones ------------------------------------------------------------------------
@pytest.mark.parametrize("P", [5, 257])
def test_an_infinite_cell_leaves_its_vector_out_and_no_other(engine, P):
    W = 17
    clean, at = X.vectors(W, P, extreme=True)
    clean[at["bad"]] = np.random.default_rng(P).random(P)
    cm, cg, cs = on_device(engine, clean)
    assert cs.tolist() == [1] * W
    keep = np.arange(W) != at["bad"]
    for bad in (np.inf, -np.inf):
        for where in (0, P - 1):
            v, at = X.vectors(W, P, bad=bad, bad_at=where, extreme=True)
            assert v[at["bad"], where] == bad and np.isfinite(v).sum() == W * P - 1 and np.array_equal(v[keep], clean[keep])
            mean, gram, status = on_device(engine, v)
            assert status.tolist() == [1] * (W - 1) + [0]
            X.check_all(v, mean, gram, status, N().win_cmp_finish, "device, %g in cell %d" % (bad, where))
            assert np.array_equal(bits(mean[keep]), bits(cm[keep])) and np.array_equal(bits(gram[np.ix_(keep, keep)]), bits(cg[np.ix_(keep, keep)]))


@pytest.mark.parametrize("W,P", [(17, 5), (17, 257), (65, 515)])
def test_extreme_vectors_large_mean_and_cells_near_2_to_the_minus_500(engine, W, P):
    v, at = X.vectors(W, P, extreme=True)
    assert abs(v[at["big"]] - 1.0).max() < 1e-7 and 0 < v[at["tiny"]].max() < 2.0 ** -499
    exp = X.expect(v)
    mean, gram, status = on_device(engine, v)
    X.check_all(v, mean, gram, status, N().win_cmp_finish, "device, extreme vectors", exp)
    X.check_twin(mean, gram, status, *N().win_cmp_host(v), exp, "extreme vectors W=%d P=%d" % (W, P))
    cor, _ = N().win_cmp_finish(mean, gram, status, P)
    # (the roots one by one: two roundings and the product's)
    assert abs(cor[at["tiny"], at["tiny"]] - 1.0) <= 4 * 2.0 ** -53 and cor[at["big"], at["big"]] == 1.0


TOT = 1 << 22
PLANTED = {"one": (2, 0, 1.0), "above": (5, 189, 1.5), "three_quarters": (8, 77, 0.75), "below": (11, 100, 0.75 - 2.0 ** -20),
           "minus_zero": (14, 3, -0.0)}  # name: (vector, cell, sum / cnt)


def planted(tot):
    """sums and counts of 20 vectors of 190 cells, sum / cnt (or sum / tot_sites) in [0.05, 0.6) but for the planted cells,
    whose counts are 2^22 so that every quotient is exact"""
    r = np.random.default_rng(190)
    Cn = r.integers(200, 400, (20, N_PAIRS)).astype(np.uint64)
    S = r.uniform(0.05, 0.6, Cn.shape) * (float(tot) if tot else Cn.astype(np.float64))
    for w, c, d in PLANTED.values():
        Cn[w, c] = TOT
        S[w, c] = d * TOT
        assert S[w, c] / TOT == d
    assert np.signbit(S[14, 3]) and S[14, 3] == 0.0
    return S, Cn


@pytest.mark.parametrize("model,tot", [(0, 0), (1, 0), (2, 0), (1, TOT), (2, TOT)])
def test_planted_sums_and_counts_whose_cells_are_not_finite(model, tot):
    import torch
    S, Cn = planted(tot)
    d = finish(S, Cn, model, tot)
    fin = np.isfinite(d).all(axis=1)
    # the test's own eyes: which vectors the model takes out, and by which kind of cell
    out = {0: [], 1: [2, 5], 2: [2, 5, 8]}[model]
    assert np.flatnonzero(~fin).tolist() == out
    if model == 1:
        assert d[2, 0] == np.inf and np.isnan(d[5, 189]) and np.isfinite(d[8, 77])
    if model == 2:
        assert np.isnan(d[2, 0]) and np.isnan(d[5, 189]) and d[8, 77] == np.inf and np.isfinite(d[11, 100]) and d[11, 100] > 10
    assert np.signbit(d[14, 3]) and d[14, 3] == 0.0
    with N().Engine(N_IND, 16, kernel="mfma") as e:
        e.synth_fill(1).commit()
        ds = torch.from_numpy(S).to("cuda")
        dc = torch.from_numpy(Cn.astype(np.int64)).to("cuda")
        torch.cuda.synchronize()
        got = e.win_cmp(ds.data_ptr(), None if tot else dc.data_ptr(), 20, evol_model=model, tot_sites=tot)
        assert np.array_equal(got[2] == 1, fin), (model, tot, got[2])
        check_finished(got, d, "planted sums and counts, model %d, tot_sites %d" % (model, tot))
