"""What the comparison of windows must give (include/ngsdist_amd.h "Comparison of windows"), computed directly from the
definition in extended precision: numpy's longdouble where that is wider than a double (x86: 64 bits of mantissa), exact
rational arithmetic where it is not.  rms^2 comes from the cell differences themselves, never from the Gram matrix.  Also
the input makers of test_win_cmp_cpu.py and test_gpu_win_cmp.py, and check_all, which prints every comparison's largest figure
in units of its bound.

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


def vectors(W, P, seed=0):
    """W vectors of P cells: a common random base plus noise of 1e-2 each, as the windows of one genome resemble each other;
    among them, as far as W allows, an exact duplicate of vector 0 (index 1), a copy of it plus noise of 1e-9 (2), an all-zero
    vector (3), a vector of one power-of-two value (4), and with W >= 3 a vector with a cell that is not finite (the last).
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
        v[W - 1, (7 * W) % P] = np.nan
        at["bad"] = W - 1
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


def check_all(values, mean, gram, status, finish, what, exp=None):
    """mean / gram / status of `values` (device or host twin) and the cor / rms that finish(mean, gram, status, P) derives
    from them, against the expectation: status, the NaNs written from it, symmetry by bits, then gram, mean, rms^2 and cor
    within their bounds.  Prints the largest figure of each in units of its bound and returns them."""
    exp = exp or expect(values)
    W, P = exp["W"], exp["P"]
    ok = exp["status"] == 1
    assert mean.shape == (W,) and gram.shape == (W, W) and status.shape == (W,)
    assert np.array_equal(status, exp["status"]), (what, status)
    cor, rms = finish(mean, gram, status, P)
    # a status-0 vector: its mean, row and column the positive quiet NaN, and everything derived NaN
    for w in np.flatnonzero(~ok):
        assert bits(mean[w:w + 1])[0] == NAN_BITS
        assert np.all(bits(gram[w]) == NAN_BITS) and np.all(bits(gram[:, w]) == NAN_BITS)
        assert np.all(np.isnan(cor[w])) and np.all(np.isnan(cor[:, w])) and np.all(np.isnan(rms[w])) and np.all(np.isnan(rms[:, w]))
    assert np.all(np.isfinite(gram[np.ix_(ok, ok)])) and np.all(np.isfinite(mean[ok]))
    assert np.array_equal(bits(gram), bits(gram.T)), what + ": gram is not symmetric bit for bit"
    assert np.array_equal(bits(rms), bits(rms.T)) and np.array_equal(bits(cor), bits(cor.T))
    fig = {"gram": 0.0, "mean": 0.0, "rms2": 0.0, "cor": 0.0}
    E = exp["gram"]
    for a in np.flatnonzero(ok):
        err = abs(_f(mean[a] - exp["mean"][a]) if WIDE else _f(Fraction(float(mean[a])) - exp["mean"][a]))
        bound = TOL * _f(exp["absmean"][a])
        assert err <= bound, (what, "mean", a, err, bound)
        if bound > 0:
            fig["mean"] = max(fig["mean"], err / bound)
        assert rms[a, a] == 0.0
        for b in np.flatnonzero(ok):
            g = np.longdouble(gram[a, b]) if WIDE else Fraction(float(gram[a, b]))
            scale = math.sqrt(_f(E[a, a]) * _f(E[b, b]))
            err, bound = abs(_f(g - E[a, b])), TOL * scale
            assert err <= bound, (what, "gram", a, b, err, bound)
            if bound > 0:
                fig["gram"] = max(fig["gram"], err / bound)
            dm = exp["mean"][a] - exp["mean"][b]
            bound = TOL * _f((E[a, a] + E[b, b] + P * dm * dm) / P)
            r2 = np.longdouble(rms[a, b]) ** 2 if WIDE else Fraction(float(rms[a, b])) ** 2
            err = abs(_f(r2 - exp["rms2"][a, b]))
            assert err <= bound, (what, "rms2", a, b, err, bound)
            if bound > 0:
                fig["rms2"] = max(fig["rms2"], err / bound)
            if E[a, a] == 0 or E[b, b] == 0:
                # the exact diagonal is 0 only for the vectors the header pins: all cells zero, or one power of two (and P = 1)
                assert np.isnan(cor[a, b]), (what, "cor is not NaN", a, b, cor[a, b])
                assert gram[a, b] == 0.0
            else:
                err = abs(float(cor[a, b]) - _f(E[a, b]) / scale)
                assert err <= COR_TOL, (what, "cor", a, b, err)
                fig["cor"] = max(fig["cor"], err / COR_TOL)
    print("%s W=%d P=%d: largest figures in units of their bounds: %s" % (what, W, P, {k: "%.3g" % x for k, x in fig.items()}))
    return fig


def check_twin(mean, gram, status, hmean, hgram, hstatus, exp, what):
    """device against host twin: both within the contract of the same exact value, so within twice the bound of each other"""
    assert np.array_equal(status, hstatus)
    ok = np.flatnonzero(exp["status"] == 1)
    worst = 0.0
    for a in ok:
        assert abs(mean[a] - hmean[a]) <= 2 * TOL * _f(exp["absmean"][a])
        for b in ok:
            bound = 2 * TOL * math.sqrt(_f(exp["gram"][a, a]) * _f(exp["gram"][b, b]))
            err = abs(gram[a, b] - hgram[a, b])
            assert err <= bound, (what, a, b, err, bound)
            if bound > 0:
                worst = max(worst, err / bound)
    print("%s: device against host twin, gram differs by %.3g of the bound" % (what, worst))
    return worst
