"""What the comparison of windows must give (include/ngsdist_amd.h "Comparison of windows"), computed directly from the
definition in extended precision: numpy's longdouble where that is wider than a double (x86: 64 bits of mantissa), exact
rational arithmetic where it is not.  rms^2 comes from the cell differences themselves, never from the Gram matrix.  Also
the input makers of test_win_cmp_cpu.py and test_gpu_win_cmp.py, and check_all, which prints every comparison's largest figure
in units of its bound.  For W too large for the W^2 loop (test_gpu_win_cmp_edges.py): check_pairs, the same on listed pairs
and every diagonal entry, and screen_all, every pair against numpy's FP64 product.

Bounds.  gram and rms^2 are the contract's: 1e-9 of sqrt(exact[a][a] exact[b][b]), and 1e-9 of (exact[a][a] + exact[b][b] +
P (mean[a] - mean[b])^2) / P.  The header sets none for mean and cor; the ones here follow from those two.  mean: a sum of P
terms in any fixed order is within P 2^-53 of SUM |x|, P below 2^31 here, so 1e-9 of mean |x| holds whatever the tree.
cor = g_ab / sqrt(g_aa g_bb): g_ab off by 1e-9 of the scale and each diagonal by 1e-9 of itself move it by at most
1e-9 + |cor| 1e-9 <= 2e-9, to first order; 3e-9 with the division's and the root's roundings."""
import math
from fractions import Fraction

import numpy as np

TOL = 1e-9
COR_TOL = 3e-9
NAN_BITS = 0x7FF8000000000000
WIDE = np.finfo(np.longdouble).nmant > 52

# the shapes of the tests: the MFMA tile's edges (15, 16, 17), more tiles than one wavefront owns (65: five groups of 16
# vectors, two tile blocks a side), the k-group's edges and a slice's (P_of)
WS = (1, 2, 15, 16, 17, 33, 65)


def P_of(W, slice_of):
    """the cell counts at W vectors: the k-group's edges, and a slice's with s = slice_of(W, P) looked up -- the rule gives
    the same s at every one of them, which is asserted"""
    s = slice_of(W, 1)
    Ps = (1, 3, 4, 5, s - 1, s, s + 1, 2 * s + 3)
    assert all(slice_of(W, P) == s for P in Ps), (W, s)
    return Ps


def vectors(W, P, seed=0, bad=np.nan, bad_at=None, extreme=False):
    """W vectors of P cells: a common random base plus noise of 1e-2 each, as the windows of one genome resemble each other;
    among them, as far as W allows, an exact duplicate of vector 0 (index 1), a copy of it plus noise of 1e-9 (2), an all-zero
    vector (3), a vector of one power-of-two value (4), and with W >= 3 a vector with a cell that is not finite (the last):
    the value `bad` (NaN, +inf or -inf) in cell `bad_at` (7 W mod P when not given).  extreme, with W >= 8: a vector of large
    mean and tiny spread, 1 + 1e-8 noise (5), and one of cells near 2^-500 (6), whose products stay short of underflow.  The
    other vectors are the same with and without the options.
    -> (values float64[W][P], dict of the special indices)"""
    r = np.random.default_rng(1000 * W + P + seed)
    base = r.random(P)
    v = base[None, :] + 1e-2 * r.standard_normal((W, P))
    at = {}
    if W >= 2:
        v[1] = v[0]
        at["dup"] = 1
    if W >= 4:
        v[2] = v[0] + 1e-9 * r.standard_normal(P)
        at["near"] = 2
    if W >= 5:
        v[3] = 0.0
        at["zero"] = 3
    if W >= 6:
        v[4] = 0.25
        at["pow2"] = 4
    if W >= 3:
        v[W - 1, (7 * W) % P if bad_at is None else bad_at] = bad
        at["bad"] = W - 1
    if extreme and W >= 8:  # (drawn last: the vectors above do not depend on the option)
        v[5] = 1.0 + 1e-8 * r.standard_normal(P)
        v[6] = np.ldexp(0.5 + r.random(P), -500)
        at["big"], at["tiny"] = 5, 6
    return np.ascontiguousarray(v), at


def _sum(x):
    return np.sum(x, dtype=np.longdouble) if WIDE else Fraction(0) + sum(Fraction(float(t)) for t in x)


def expect(values):
    """-> dict: status uint32[W]; mean, gram [W][W], rms2 [W][W] (the mean of the squared cell differences), absmean (the
    mean of |x|), as longdouble arrays (or arrays of Fractions); entries of a status-0 vector are None / NaN"""
    v = np.asarray(values, dtype=np.float64)
    W, P = v.shape
    status = np.array([1 if np.all(np.isfinite(v[w])) else 0 for w in range(W)], dtype=np.uint32)
    if WIDE:
        x = np.where(status[:, None] == 1, v, 0.0).astype(np.longdouble)
        mean = x.sum(axis=1) / np.longdouble(P)
        z = x - mean[:, None]
        gram = np.array([[np.sum(z[a] * z[b]) for b in range(W)] for a in range(W)], dtype=np.longdouble)
        rms2 = np.array([[np.sum((x[a] - x[b]) ** 2) / np.longdouble(P) for b in range(W)] for a in range(W)], dtype=np.longdouble)
        absmean = np.abs(x).sum(axis=1) / np.longdouble(P)
    else:
        x = [[Fraction(float(t)) if status[w] else Fraction(0) for t in v[w]] for w in range(W)]
        mean = np.array([sum(r) / P for r in x], dtype=object)
        z = [[t - mean[w] for t in x[w]] for w in range(W)]
        gram = np.array([[sum(p * q for p, q in zip(z[a], z[b])) for b in range(W)] for a in range(W)], dtype=object)
        rms2 = np.array([[sum((p - q) ** 2 for p, q in zip(x[a], x[b])) / P for b in range(W)] for a in range(W)], dtype=object)
        absmean = np.array([sum(abs(t) for t in r) / P for r in x], dtype=object)
    return {"status": status, "mean": mean, "gram": gram, "rms2": rms2, "absmean": absmean, "W": W, "P": P}


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _f(x):
    return float(x)


def _scale(ea, eb):
    """sqrt(exact[a][a] exact[b][b]) as a double: the roots first, so that two diagonals near 2^-1000 do not underflow in the
    product (the vector of cells near 2^-500)"""
    return math.sqrt(_f(ea)) * math.sqrt(_f(eb))


def _check_status(mean, gram, status, cor, rms, exp_status, what):
    """status, the NaNs written from it (a status-0 vector: its mean, row and column the positive quiet NaN, and everything
    derived NaN), finite numbers everywhere else, symmetry by bits"""
    ok = exp_status == 1
    assert np.array_equal(status, exp_status), (what, status)
    for w in np.flatnonzero(~ok):
        assert bits(mean[w:w + 1])[0] == NAN_BITS
        assert np.all(bits(gram[w]) == NAN_BITS) and np.all(bits(gram[:, w]) == NAN_BITS)
        if cor is not None:
            assert np.all(np.isnan(cor[w])) and np.all(np.isnan(cor[:, w])) and np.all(np.isnan(rms[w])) and np.all(np.isnan(rms[:, w]))
    assert np.all(np.isfinite(gram[np.ix_(ok, ok)])) and np.all(np.isfinite(mean[ok]))
    assert np.array_equal(bits(gram), bits(gram.T)), what + ": gram is not symmetric bit for bit"
    if cor is not None:
        assert np.array_equal(bits(rms), bits(rms.T)) and np.array_equal(bits(cor), bits(cor.T))


def _check_mean(fig, what, a, mean_a, e_mean, e_absmean):
    err = abs(_f(mean_a - e_mean) if WIDE else _f(Fraction(float(mean_a)) - e_mean))
    bound = TOL * _f(e_absmean)
    assert err <= bound, (what, "mean", a, err, bound)
    if bound > 0:
        fig["mean"] = max(fig["mean"], err / bound)


def _check_pair(fig, what, a, b, P, got, e_ab, e_aa, e_bb, e_dm, e_rms2):
    """gram, rms^2 and cor of one pair, got = (gram[a][b], rms[a][b], cor[a][b]), against the exact Gram entry, the two exact
    diagonals, the exact difference of the means and the exact mean squared cell difference"""
    g_ab, rms_ab, cor_ab = got
    g = np.longdouble(g_ab) if WIDE else Fraction(float(g_ab))
    scale = _scale(e_aa, e_bb)
    err, bound = abs(_f(g - e_ab)), TOL * scale
    assert err <= bound, (what, "gram", a, b, err, bound)
    if bound > 0:
        fig["gram"] = max(fig["gram"], err / bound)
    bound = TOL * _f((e_aa + e_bb + P * e_dm * e_dm) / P)
    r2 = np.longdouble(rms_ab) ** 2 if WIDE else Fraction(float(rms_ab)) ** 2
    err = abs(_f(r2 - e_rms2))
    assert err <= bound, (what, "rms2", a, b, err, bound)
    if bound > 0:
        fig["rms2"] = max(fig["rms2"], err / bound)
    if e_aa == 0 or e_bb == 0:
        # the exact diagonal is 0 only for the vectors the header pins: all cells zero, or one power of two (and P = 1)
        assert np.isnan(cor_ab), (what, "cor is not NaN", a, b, cor_ab)
        assert g_ab == 0.0
    else:
        err = abs(float(cor_ab) - _f(e_ab) / scale)
        assert err <= COR_TOL, (what, "cor", a, b, err)
        fig["cor"] = max(fig["cor"], err / COR_TOL)


def _say(what, W, P, fig):
    print("%s W=%d P=%d: largest figures in units of their bounds: %s" % (what, W, P, {k: "%.3g" % x for k, x in fig.items()}))
    return fig


def check_all(values, mean, gram, status, finish, what, exp=None):
    """mean / gram / status of `values` (device or host twin) and the cor / rms that finish(mean, gram, status, P) derives
    from them, against the expectation: status, the NaNs written from it, symmetry by bits, then gram, mean, rms^2 and cor
    within their bounds.  Prints the largest figure of each in units of its bound and returns them."""
    exp = exp or expect(values)
    W, P = exp["W"], exp["P"]
    ok = exp["status"] == 1
    assert mean.shape == (W,) and gram.shape == (W, W) and status.shape == (W,)
    cor, rms = finish(mean, gram, status, P)
    _check_status(mean, gram, status, cor, rms, exp["status"], what)
    fig = {"gram": 0.0, "mean": 0.0, "rms2": 0.0, "cor": 0.0}
    E = exp["gram"]
    for a in np.flatnonzero(ok):
        _check_mean(fig, what, a, mean[a], exp["mean"][a], exp["absmean"][a])
        assert rms[a, a] == 0.0
        for b in np.flatnonzero(ok):
            _check_pair(fig, what, a, b, P, (gram[a, b], rms[a, b], cor[a, b]), E[a, b], E[a, a], E[b, b],
                        exp["mean"][a] - exp["mean"][b], exp["rms2"][a, b])
    return _say(what, W, P, fig)


def check_twin(mean, gram, status, hmean, hgram, hstatus, exp, what):
    """device against host twin: both within the contract of the same exact value, so within twice the bound of each other"""
    assert np.array_equal(status, hstatus)
    ok = np.flatnonzero(exp["status"] == 1)
    worst = 0.0
    for a in ok:
        assert abs(mean[a] - hmean[a]) <= 2 * TOL * _f(exp["absmean"][a])
        for b in ok:
            bound = 2 * TOL * _scale(exp["gram"][a, a], exp["gram"][b, b])
            err = abs(gram[a, b] - hgram[a, b])
            assert err <= bound, (what, a, b, err, bound)
            if bound > 0:
                worst = max(worst, err / bound)
    print("%s: device against host twin, gram differs by %.3g of the bound" % (what, worst))
    return worst


def expect_rows(values):
    """the per-vector part of the expectation, for W too large for expect()'s W^2 loop: -> dict of status, mean, absmean, the
    diagonal of gram, and the extended-precision cells x and centred cells z that expect_pair() multiplies"""
    v = np.asarray(values, dtype=np.float64)
    W, P = v.shape
    status = np.all(np.isfinite(v), axis=1).astype(np.uint32)
    if WIDE:
        x = np.where(status[:, None] == 1, v, 0.0).astype(np.longdouble)
        mean = x.sum(axis=1) / np.longdouble(P)
        z = x - mean[:, None]
        diag = (z * z).sum(axis=1)
        absmean = np.abs(x).sum(axis=1) / np.longdouble(P)
    else:
        x = [[Fraction(float(t)) if status[w] else Fraction(0) for t in v[w]] for w in range(W)]
        mean = np.array([sum(r) / P for r in x], dtype=object)
        z = [[t - mean[w] for t in x[w]] for w in range(W)]
        diag = np.array([sum(t * t for t in r) for r in z], dtype=object)
        absmean = np.array([sum(abs(t) for t in r) / P for r in x], dtype=object)
    return {"status": status, "mean": mean, "absmean": absmean, "diag": diag, "x": x, "z": z, "W": W, "P": P}


def expect_pair(rows, a, b):
    """-> (exact gram[a][b], exact mean squared cell difference of a and b)"""
    x, z, P = rows["x"], rows["z"], rows["P"]
    if WIDE:
        return np.sum(z[a] * z[b]), np.sum((x[a] - x[b]) ** 2) / np.longdouble(P)
    return sum(p * q for p, q in zip(z[a], z[b])), sum((p - q) ** 2 for p, q in zip(x[a], x[b])) / P


def check_pairs(values, mean, gram, status, finish, pairs, what, rows=None):
    """check_all on the listed (a, b) pairs and on every diagonal entry only: the same bounds, the same printing.  The mean
    and the diagonal of every vector are formed first, then the listed products.  A listed pair with a status-0 vector is
    covered by the NaN check of its row and column."""
    rows = rows or expect_rows(values)
    W, P = rows["W"], rows["P"]
    assert mean.shape == (W,) and gram.shape == (W, W) and status.shape == (W,)
    cor, rms = finish(mean, gram, status, P)
    _check_status(mean, gram, status, cor, rms, rows["status"], what)
    fig = {"gram": 0.0, "mean": 0.0, "rms2": 0.0, "cor": 0.0}
    ok, d, m = rows["status"] == 1, rows["diag"], rows["mean"]
    for a in np.flatnonzero(ok):
        _check_mean(fig, what, a, mean[a], m[a], rows["absmean"][a])
        assert rms[a, a] == 0.0
        _check_pair(fig, what, a, a, P, (gram[a, a], rms[a, a], cor[a, a]), d[a], d[a], d[a], m[a] - m[a], m[a] - m[a])
    n = 0
    for a, b in pairs:
        if ok[a] and ok[b]:
            e_ab, e_rms2 = expect_pair(rows, a, b)
            _check_pair(fig, what, a, b, P, (gram[a, b], rms[a, b], cor[a, b]), e_ab, d[a], d[b], m[a] - m[b], e_rms2)
            n += 1
    print("%s: %d listed pairs and %d diagonal entries" % (what, n, int(ok.sum())))
    return _say(what, W, P, fig)


def screen_all(values, mean, gram, status, what, rows=None):
    """every pair of status-1 vectors against numpy's FP64 product of the centred cells, within the contract's bound
    1e-9 sqrt(d_a d_b), d the extended-precision diagonal; status, the NaN rows written from it and symmetry by bits.  A
    screen for W too large for the W^2 loop, not the reference (check_pairs is, on the pairs it is given): the cells are
    centred in extended precision and rounded once, and the FP64 product of P terms is within about P 2^-53 of the scale."""
    rows = rows or expect_rows(values)
    W = rows["W"]
    assert mean.shape == (W,) and gram.shape == (W, W) and status.shape == (W,)
    _check_status(mean, gram, status, None, None, rows["status"], what)
    ok = np.flatnonzero(rows["status"] == 1)
    zc = np.array([[_f(t) for t in rows["z"][w]] for w in ok]) if not WIDE else rows["z"][ok].astype(np.float64)
    root = np.array([math.sqrt(_f(t)) for t in rows["diag"][ok]])
    err = np.abs(gram[np.ix_(ok, ok)] - zc @ zc.T)
    bound = TOL * np.outer(root, root)
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    assert np.all(err <= bound), (what, "gram", ok[worst[0]], ok[worst[1]], err[worst], bound[worst])
    with np.errstate(invalid="ignore", divide="ignore"):
        fig = float(np.max(np.where(bound > 0, err / bound, 0.0)))
    print("%s W=%d P=%d: every pair against the FP64 product, largest difference %.3g of the bound" % (what, W, rows["P"], fig))
    return fig
