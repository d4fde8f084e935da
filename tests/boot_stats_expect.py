"""What the bootstrap summaries must give (include/ngsdist_amd.h "Bootstrap summaries"), in numpy, for the tests of the host
function and of the device kernel -- never from either of them.  Per cell the operations run in the order the contract
names: a loop over the replicates in ascending r (elementwise over the cells, so each cell's additions are sequential
float64 additions from 0.0), np.sort of the finite replicates, and the two rank formulas in float64."""
import numpy as np

QNAN = 0x7FF8000000000000


def planted(n_set, n_rep, n_cells, seed):
    """values [n_set][n_rep + 1][n_cells] with every special case in known cells of every set: column 0 a NaN replicate,
    1 +inf, 2 -inf, 3 a -0.0 / 0.0 tie, 4 duplicates, 5 all replicates NaN, 6 one finite replicate, 7 ascending,
    8 descending, 9 every special value at once, 10 a NaN estimate, 11 an inf estimate; the rest random"""
    rng = np.random.default_rng(seed)
    v = rng.random((n_set, n_rep + 1, n_cells)) * rng.choice([1e-3, 1.0, 50.0], size=(n_set, 1, n_cells))
    R = n_rep
    r = lambda k: 1 + (k % R)  # a replicate's row
    v[:, r(0), 0] = np.nan
    v[:, r(1), 1] = np.inf
    v[:, r(2), 2] = -np.inf
    v[:, 1:, 3] = np.where(np.arange(R) % 2 == 0, -0.0, 0.0)[None, :]
    if R > 2:
        v[:, r(2), 3] = 0.25
    v[:, 1:, 4] = np.round(v[:, 1:, 4] * 3 / max(v[:, 1:, 4].max(), 1e-300)) / 3  # four distinct values
    v[:, 1:, 5] = np.nan
    v[:, 1:, 6] = np.nan
    v[:, r(R // 2), 6] = 0.125
    v[:, 1:, 7] = np.sort(v[:, 1:, 7], axis=1)
    v[:, 1:, 8] = -np.sort(-v[:, 1:, 8], axis=1)
    for k, x in enumerate((np.nan, np.inf, -np.inf, -0.0, 0.0, v[0, 1, 9], v[0, 1, 9])):
        v[:, r(3 * k + 1), 9] = x  # (fewer rows than values: the later ones win)
    v[:, 0, 10] = np.nan
    v[:, 0, 11] = np.inf
    return v


def expect(values, ci=0.95):
    """values float64[..., n_mat, n_cells] -> (stats float64[..., 5, n_cells], used uint64[..., n_cells])"""
    v = np.asarray(values, dtype=np.float64)
    n_mat = v.shape[-2]
    rep = np.moveaxis(v, -2, 0)[1:]  # [R][..., n_cells]
    fin = np.isfinite(rep)
    m = fin.sum(axis=0)
    p_lo = (1.0 - float(ci)) / 2.0
    p_hi = 1.0 - p_lo
    with np.errstate(all="ignore"):
        acc = np.zeros(m.shape)
        for r in range(n_mat - 1):
            acc = np.where(fin[r], acc + rep[r], acc)
        mean = acc / m.astype(np.float64)
        ss = np.zeros(m.shape)
        for r in range(n_mat - 1):
            d = rep[r] - mean
            ss = np.where(fin[r], ss + d * d, ss)
        sd = np.sqrt(ss / (m - 1).astype(np.float64))
    nan = np.uint64(QNAN).view(np.float64)
    mean = np.where(m == 0, nan, mean)
    sd = np.where(m < 2, nan, sd)
    s = np.sort(np.where(fin, rep, np.inf), axis=0)  # the finite ones first, ascending
    last = np.maximum(m, 1) - 1
    k_lo = np.floor(p_lo * last.astype(np.float64)).astype(np.int64)
    k_hi = np.ceil(p_hi * last.astype(np.float64)).astype(np.int64)
    lo = np.where(m == 0, nan, np.take_along_axis(s, k_lo[None], axis=0)[0])
    hi = np.where(m == 0, nan, np.take_along_axis(s, k_hi[None], axis=0)[0])
    stats = np.stack([np.moveaxis(v, -2, 0)[0], mean, sd, lo, hi], axis=-2)
    return stats, m.astype(np.uint64)


def sd_tol(m, sd, mean):
    """the bound on sd from sums and counts through the device's log: 1e-12 sd + 64 m 2^-53 |mean| (two-pass deviations carry
    m roundings of the mean's magnitude)"""
    return 1e-12 * np.abs(sd) + 64.0 * m * 2.0 ** -53 * np.abs(mean)


def check_exact(got, want, what):
    """est / mean / lo / hi equal as values, NaNs by bits where the contract makes them, used equal, sd within 4 ulp"""
    (gs, gu), (ws, wu) = got, want
    assert gs.shape == ws.shape and gu.shape == wu.shape, what
    assert np.array_equal(gu, wu), what
    for k, name in ((0, "est"), (1, "mean"), (3, "lo"), (4, "hi")):
        assert np.array_equal(gs[..., k, :], ws[..., k, :], equal_nan=True), (what, name)
    made = np.broadcast_to((wu == 0)[..., None, :], gs[..., [1, 3, 4], :].shape)
    assert np.all(gs[..., [1, 3, 4], :][made].view(np.uint64) == QNAN), what
    few = wu < 2
    g2, w2 = gs[..., 2, :], ws[..., 2, :]
    assert np.all(g2[few].view(np.uint64) == QNAN), what
    ulp = np.abs(g2[~few] - w2[~few]) / np.spacing(np.abs(w2[~few]))
    worst = float(ulp.max()) if ulp.size else 0.0
    print("boot stats %s: sd off by at most %.3g ulp over %d cells, the rest equal" % (what, worst, ulp.size))
    assert worst <= 4, (what, worst)


def check_close(got, want, what, rtol=1e-13, exact_used=True):
    """from sums and counts under models 1 and 2: every statistic but sd within rtol, sd within sd_tol, used equal"""
    (gs, gu), (ws, wu) = got, want
    assert gs.shape == ws.shape and gu.shape == wu.shape, what
    if exact_used:
        assert np.array_equal(gu, wu), what
    worst = 0.0
    for k in (0, 1, 3, 4):
        g, w = gs[..., k, :], ws[..., k, :]
        assert np.array_equal(np.isfinite(g), np.isfinite(w)), (what, k)
        f = np.isfinite(w)
        assert np.array_equal(g[~f], w[~f], equal_nan=True), (what, k)
        err = np.abs(g[f] - w[f]) / np.where(w[f] == 0, 1.0, np.abs(w[f]))
        worst = max(worst, float(err.max()) if err.size else 0.0)
    print("boot stats %s: largest relative error %.3g (est, mean, lo, hi)" % (what, worst))
    assert worst <= rtol, (what, worst)
    g, w = gs[..., 2, :], ws[..., 2, :]
    f = wu >= 2
    assert np.all(np.isnan(g[~f]))
    tol = sd_tol(wu[f].astype(np.float64), w[f], ws[..., 1, :][f])
    err = np.abs(g[f] - w[f])
    ratio = float((err / np.maximum(tol, 1e-300)).max()) if err.size else 0.0
    print("boot stats %s: sd at most %.3g of its bound" % (what, ratio))
    assert np.all(err <= tol), (what, ratio)
