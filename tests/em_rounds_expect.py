"""Planted input for the later table rounds of the EM kernels, and what the CPU says about it.

The single-site EM of a pair has a closed form (accum_em_table.hip's header): with A_t(i) = SUM_x GL_i[x]^t the pair
(i, j) stops at the first step t with R_t(i) * R_t(j) < e^tole, R_t = A_{t+1} A_{t-1} / A_t^2, or at step 50.  So the
stopping step of every (pair, site) can be CHOSEN: this module holds a menu of likelihood vectors whose pairs stop at
every step from 1 to T_MAX, builds one-site scenes from it that put a chosen number of pairs into the second and third
table round of a 64 x 64 tile, and states in numpy -- from the power sums, with nothing of the kernels' code -- where
every pair stops, how close it comes to the tolerance on the way, and how many table rounds the kernel must report.

T_MAX = 40 is what a search over likelihoods (1, rho, rho') on a 400 x 400 grid finds as the latest stop short of the
forced one ((1, rho, rho) against itself, rho = 0.933 ... 0.936); tests/test_em_rounds_cpu.py repeats it coarsely.
"""
import functools
import math

import numpy as np

TOLE = 0.001
E_TOLE = math.exp(TOLE)
MAX_ITER = 50
T_MAX = 40          # the latest stop valid input reaches before the forced one (see above)
TS = 64             # the kernel's tile edge
PACK_DENSE = 24     # accum_em_table.hip: rows with fewer pairs still searching go through packed units
N_IND = 130         # six tiles: (0, 1) is full, (0, 2) and (1, 2) have two columns, (2, 2) has one pair
MIN_MARGIN = 1e-9   # every scene keeps |R_i R_j / e^tole - 1| at least this large at every step up to the stop

RHOS = [0.02, 0.08, 0.20, 0.30, 0.55, 0.70, 0.78, 0.82, 0.85, 0.87, 0.885, 0.90, 0.91, 0.92, 0.93, 0.935, 0.94, 0.95, 0.952, 0.96, 0.97, 0.98]
UNIFORM = np.full(3, 1.0 / 3)
# R_1 < e^tole <= R_t for t = 2 ... 27: as a row it can stop in the first block of eight steps of round 1 (at step 1,
# against a uniform column) and in none of the second block's -- the one way a row gets to skip its second block only
DIPPER = np.array([1.0, 0.9414, 0.9314])


def norm(v):
    v = np.asarray(v, dtype=np.float64)
    return v / v.sum()


def fast_vectors():
    """R_t = 1 from step 2 on (the certain genotypes: R_1 = 3) or at every step (uniform)"""
    return [np.array([1.0, 0, 0]), np.array([0, 1.0, 0]), np.array([0, 0, 1.0]), UNIFORM.copy()]


def slow_vectors():
    return ([norm([1, r, r]) for r in RHOS] + [norm([r, 1, 0.999 * r]) for r in RHOS] + [norm([1, r, 0]) for r in RHOS]
            + [norm(DIPPER)])


def menu():
    return np.array(fast_vectors() + slow_vectors())


def factors(g):
    """R_t for t = 1 ... MAX_ITER along a new last axis, of likelihood vectors g[..., 3]"""
    g = np.asarray(g, dtype=np.float64)
    t = np.arange(0, MAX_ITER + 2, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        A = (g[..., None, :] ** t[:, None]).sum(-1)
        return A[..., 2:] * A[..., :-2] / A[..., 1:-1] ** 2


def is_miss(g):
    """miss_data() of the reference: all three likelihoods within 1e-5 of each other"""
    g = np.asarray(g, dtype=np.float64)
    return (np.abs(g[..., 0] - g[..., 1]) < 1e-5) & (np.abs(g[..., 1] - g[..., 2]) < 1e-5)


def _stop_of(prod):
    ok = prod < E_TOLE
    return np.where(ok.any(-1), ok.argmax(-1) + 1, MAX_ITER)


def pair_stop(g1, g2):
    """stopping step of single pairs of vectors (broadcast over the leading axes)"""
    return _stop_of(factors(g1) * factors(g2))


def own_stop(g):
    """where a pair with a certain genotype stops: the individual's own factor decides from step 2 on"""
    return pair_stop(g, np.array([1.0, 0, 0]))


def _walk(p, want_margin):
    p = np.asarray(p, dtype=np.float64)
    n, S, _ = p.shape
    R = factors(p)  # [n][S][50]
    T = np.zeros((n, n, S), dtype=np.uint8)
    M = np.full((n, n, S), np.inf) if want_margin else None
    steps = np.arange(1, MAX_ITER + 1)
    for i in range(n - 1):
        prod = R[i][None] * R[i + 1:]
        Ti = _stop_of(prod)
        T[i, i + 1:] = Ti
        if want_margin:
            d = np.abs(prod / E_TOLE - 1.0)
            d[steps > Ti[..., None]] = np.inf
            M[i, i + 1:] = d.min(-1)
    return T, M


def stop_steps(p, pairwise_del=False):
    """T[i][j][site] for i < j (0 elsewhere) of p[n_ind][n_sites][3]: the first t with R_t(i) R_t(j) < e^0.001, or 50.
    pairwise_del: a pair with a missing individual is not visited by the reference; the table kernel gives it thresholds
    of +inf and it leaves at step 1 with a term of exactly 0 -- it is listed as 1, which is what the rounds count."""
    T, _ = _walk(p, False)
    if pairwise_del:
        miss = is_miss(p)
        gone = miss[:, None, :] | miss[None, :, :]
        T[gone & (T > 0)] = 1
    return T


def margins(p):
    """min over t <= T of |R_t(i) R_t(j) / e^tole - 1| for i < j (+inf elsewhere)"""
    return _walk(p, True)[1]


def expected_rounds(p, CH, n_ind, pairwise_del=False):
    """table rounds of one plain pass of the table kernel over p[:n_ind]: per 64 x 64 tile of the upper triangle and per
    site, the rounds of CH steps until the tile's last pair has stopped (one at least)"""
    T = stop_steps(np.asarray(p)[:n_ind], pairwise_del).astype(np.int64)
    nt = (n_ind + TS - 1) // TS
    total = 0
    for ti in range(nt):
        for tj in range(ti, nt):
            last = T[ti * TS:(ti + 1) * TS, tj * TS:(tj + 1) * TS].max(axis=(0, 1))  # (0 where i >= j: never the largest)
            total += int(np.maximum(1, -(-last // CH)).sum())
    return total


# ---- scenes ---------------------------------------------------------------------------------------------------------------

def _perm(rng, v):
    """the vector with its likelihoods permuted: R_t is symmetric in them, the terms are not"""
    return np.asarray(v)[rng.permutation(3)]


@functools.lru_cache(maxsize=None)
def _classes():
    sv = slow_vectors()[:-1]  # (not the dipper: a class member's factor stays at or above e^tole until its own stop)
    own = [int(own_stop(v)) for v in sv]
    pick = lambda lo, hi: [v for v, o in zip(sv, own) if lo <= o <= hi and not is_miss(v)]
    return {"r1b": pick(9, 16), "r2a": pick(17, 24), "r2b": pick(25, 28), "r2": pick(17, 28)}


def _take(rng, vs, k):
    """k vectors going round the list, each with its likelihoods permuted"""
    return [_perm(rng, vs[q % len(vs)]) for q in range(k)]


def long_vectors(rng, k):
    """k vectors like (1, 0.93, 0.93): every pair among them stops in the third round of 16 steps (37 ... T_MAX), each
    against a certain genotype in the second (21 ... 28).  A draw whose pair comes within 1e-8 of the tolerance at some
    step on its way is drawn again (of 8000 pairs x 40 steps a few would come within 1e-9 by chance)."""
    rho = 0.908 + 0.027 * rng.random(k)
    while True:
        R = factors(np.array([norm([1, r, r]) for r in rho]))
        prod = R[:, None] * R[None]
        d = np.abs(prod / E_TOLE - 1.0)
        d[np.arange(1, MAX_ITER + 1) > _stop_of(prod)[..., None]] = np.inf
        bad = np.unique(np.where(d.min(-1) < 1e-8)[0])
        if not len(bad):
            return [_perm(rng, norm([1, r, r])) for r in rho]
        rho[bad[0]] = 0.908 + 0.027 * rng.random()


SKIP_PATTERNS = ["10101010", "01010101", "11110000", "00001111", "10000001", "11111111"]
SEARCHING_COLUMNS = [1, 7, 8, 9, 16, 17, 23, 24, 25, 63, 64]


@functools.lru_cache(maxsize=None)
def scenes(n_ind=N_IND, miss=False):
    """-> (p[n_ind][n_sites][3], info): one site per scene; info[site] = dict(name, kind, ...) with what the scene is
    meant to hold (tests/test_em_rounds_cpu.py checks it against stop_steps).  Individuals a scene does not name are certain
    genotypes drawn per (individual, site); miss: up to five of those per site are (1/3, 1/3, 1/3) instead -- missing
    data under --pairwise_del.  Rows are individuals 0 ... 63, columns 64 ... 127 (the full tile), 128 and 129 the edge."""
    assert n_ind == N_IND, "the scenes are laid out for 130 individuals"
    rng = np.random.default_rng(20240613)
    cl = _classes()
    cols, info = [], []

    def scene(name, kind, named, **what):
        g = np.zeros((n_ind, 3))
        g[np.arange(n_ind), rng.integers(0, 3, n_ind)] = 1.0
        for i, v in named.items():
            g[i] = v
        if miss:
            free = np.array([i for i in range(n_ind) if i not in named], dtype=np.int64)
            for i in rng.permutation(free)[:5]:
                g[i] = UNIFORM
        info.append(dict(name=name, kind=kind, site=len(cols), named=sorted(named), **what))
        cols.append(g)

    def lanes(k, where):
        if where == "first":
            return list(range(k))
        if where == "last":
            return list(range(TS - k, TS))
        if where == "ends":  # lanes 0 and 63 (63 alone for one column), the rest spread between them
            return [63] if k == 1 else sorted([0, 63] + rng.permutation(np.arange(1, TS - 1))[:k - 2].tolist())
        return sorted(rng.permutation(TS)[:k].tolist())

    # searching columns in round 2: k slow columns of the full tile against fast rows
    for k in SEARCHING_COLUMNS:
        for where in (["first"] if k == TS else ["first", "last", "ends", "scattered"]):
            for c in (["r2"] if k == TS else ["r2a", "r2b"]):
                ls = lanes(k, where)
                scene("cols-%d-%s-%s" % (k, where, c), "cols", dict(zip([TS + x for x in ls], _take(rng, cl[c], k))), k=k, lanes=ls)
    # ... inside the two-column edge tiles and the one-pair diagonal tile
    for who in ([128], [129], [128, 129]):
        scene("edge-" + "-".join(map(str, who)), "edge", dict(zip(who, _take(rng, cl["r2"], len(who)))), who=who)
    scene("edge-long", "edge", dict(zip([128, 129], long_vectors(rng, 2))), who=[128, 129])
    scene("edge-rows", "edge", dict(zip([3, 70, 128, 129], _take(rng, cl["r2"], 2) + long_vectors(rng, 2))), who=[128, 129])
    # slow rows against fast columns: every such row is dense in round 2
    for name, rows in (("1", [5]), ("8", list(range(24, 32))), ("9", list(range(24, 33))), ("64", list(range(TS)))):
        scene("rows-" + name, "rows", dict(zip(rows, _take(rng, cl["r2"], len(rows)))), rows=rows)
    # skip patterns: the 8 rows of wavefront 2 (rows 16 ... 23) follow the pattern, those of wavefront 5 its complement
    forms = {
        # bit 1 / bit 0 of the pattern -> the row's vector class (None: a fast row)
        "r2-first-block": ("r2b", "r2a"),   # dense in round 2 both: cannot / can stop in its first block
        "r2-dense-sparse": ("r2a", None),   # dense rows searching their first block beside rows left to the packed units
        "r2-skip-sparse": ("r2b", None),    # dense rows skipping their first block beside such rows
        "r1-first-block": ("r1b", None),    # round 1: cannot stop in the first block / a fast row
        "r1-second-block": ("dip", None),   # round 1: can stop in the first block only (at step 1)
    }
    for form, (one, zero) in forms.items():
        for pat in SKIP_PATTERNS:
            named = {}
            for w, flip in ((2, False), (5, True)):
                for r in range(8):
                    c = one if (pat[r] == "1") != flip else zero
                    if c == "dip":
                        named[8 * w + r] = _perm(rng, norm(DIPPER))
                    elif c is not None:
                        named[8 * w + r] = _take(rng, cl[c][int(rng.integers(0, len(cl[c]))):] + cl[c], 1)[0]
            if one == "dip":  # columns a dipper row stops against at step 1
                for c in (64, 64 + 31, 127):
                    named[c] = UNIFORM.copy()
            scene("skip-%s-%s" % (form, pat), "skip", named, form=form, pattern=pat)
    # round 3: slow rows x slow columns whose pairs stop in 33 ... T_MAX; slow x fast leaves in round 2
    for name, rows, ls in (("1x1", [13], [40]), ("8x8", list(range(32, 40)), lanes(8, "scattered")),
                           ("8x20", list(range(8, 16)), lanes(20, "ends")), ("3x30", [49, 50, 51], lanes(30, "scattered")),
                           ("64x64", list(range(TS)), list(range(TS)))):
        who = rows + [TS + x for x in ls]
        scene("round3-" + name, "round3", dict(zip(who, long_vectors(rng, len(who)))), rows=rows, lanes=ls)
    # the sweep: rows and columns graded over the menu (its first 64 vectors, its last 64, one against the other, draws)
    m = menu()
    M = len(m)
    head, tail = np.arange(TS), M - TS + np.arange(TS)
    for name, ro, co in (("head", head, head), ("tail", tail, tail), ("head-tail", head, tail), ("tail-head", tail[::-1], head),
                         ("shuffled", rng.permutation(M)[:TS], rng.permutation(M)[:TS]),
                         ("shuffled-2", rng.permutation(M)[:TS], rng.permutation(M)[:TS])):
        named = {}
        for x in range(TS):
            named[x] = _perm(rng, m[ro[x]])
            named[TS + x] = _perm(rng, m[co[x]])
        named[128], named[129] = _perm(rng, m[int(rng.integers(4, len(m)))]), _perm(rng, m[int(rng.integers(4, len(m)))])
        scene("sweep-" + name, "sweep", named)
    # ... and with a few graded columns only: graded rows that are dense in round 2 beside fast rows left to the packed units
    for name, ro, k in (("rows-head", head, 12), ("rows-tail", tail, 20)):
        named = {x: _perm(rng, m[ro[x]]) for x in range(TS)}
        for x in lanes(k, "scattered"):
            named[TS + x] = _perm(rng, m[int(rng.integers(4, M))])
        scene("sweep-" + name, "sweep", named)
    p = np.ascontiguousarray(np.stack(cols, axis=1))
    p.setflags(write=False)
    return p, info


def searching_after(T, n_rounds, CH=16):
    """[row][site]: pairs of the full tile (rows 0 ... 63 x columns 64 ... 127) still searching after n_rounds rounds"""
    return (T[:TS, TS:2 * TS] > n_rounds * CH).sum(axis=1)


def boundary_probes(cases, find_boundary, offsets=(-2, 0, 1, 3)):
    """in-band probes from cases 1 and 2 of tests/test_gpu_em_boundary.py (stops near 18 and 34): the doubles `offsets` ulps
    from the point where the oracle's step count changes -> [(g1, g2, table round of 16 steps)]"""
    out = []
    for case, rnd in ((1, 2), (2, 3)):
        g1, g2_of, (lo, hi) = cases[case]
        a = find_boundary(g1, g2_of, lo, hi)[0]
        out += [(g1, g2_of(a + k * np.spacing(a)), rnd) for k in offsets]
    return out


def probe_scenes(probes, n_ind=N_IND):
    """Sites for stops within rounding of the tolerance (probes: (g1, g2, round) with the pair's stop in table round 2 or 3
    of 16 steps): each probe twice, the pair being row 20 x column 64 + 9 of the full tile --
      packed: nothing else slow at the site, so the pair's column is the only one still searching in its round;
      dense:  30 more columns that keep every row searching in that round, so the pair's row is scanned the plain way.
    -> (p, planted) with planted = [(i1, i2, site, form)]"""
    rng = np.random.default_rng(977)
    cl = _classes()
    cols, planted = [], []
    for g1, g2, rnd in probes:
        for form in ("packed", "dense"):
            g = np.zeros((n_ind, 3))
            g[np.arange(n_ind), rng.integers(0, 3, n_ind)] = 1.0
            g[20], g[TS + 9] = g1, g2
            if form == "dense":
                others = [x for x in rng.permutation(TS) if x != 9][:30]
                vs = _take(rng, cl["r2b"], 30) if rnd == 2 else long_vectors(rng, 30)
                for x, v in zip(others, vs):
                    g[TS + x] = v
            planted.append((20, TS + 9, len(cols), form))
            cols.append(g)
    return np.ascontiguousarray(np.stack(cols, axis=1)), planted
