"""What keeps tests/test_gpu_em_rounds.py honest, checked without a GPU: the numpy statement of the stopping step agrees
with the oracle's EM, the scenes hold every stopping step and the occupancies they are named for, and no (pair, site) of
them comes near enough to the tolerance for any device form to stop elsewhere than the oracle."""
import numpy as np
import pytest

import em_rounds_expect as X
from oracle import oracle as O
from test_gpu_em_boundary import CASES, find_boundary


def data(miss=False):
    p, info = X.scenes(miss=miss)
    return p, info, X.stop_steps(p)


def test_stop_steps_is_the_oracles_step_count_for_every_ordered_pair_of_the_menu():
    m = X.menu()
    p = np.ascontiguousarray(np.concatenate([m, m])[:, None, :])  # individuals k and len(m) + k: menu vector k
    T = X.stop_steps(p)
    for a in range(len(m)):
        for b in range(len(m)):
            want = O.em2(m[a], m[b])[1]
            assert X.pair_stop(m[a], m[b]) == want, (a, b)
            if a != b:
                assert T[min(a, len(m) + b), max(a, len(m) + b), 0] == want, (a, b)
                assert T[min(a, b), max(a, b), 0] == want
    assert np.all(T[np.tril_indices(2 * len(m))] == 0)


def test_the_latest_stop_of_valid_input_is_t_max():
    grid = np.linspace(0.80, 0.99, 96)
    v = np.array([X.norm([1, a, b]) for a in grid for b in grid if b <= a])
    R = X.factors(v)
    own = X._stop_of(R * R)
    assert own.max() == X.T_MAX
    top = np.argsort(-own, kind="stable")[:200]
    assert X._stop_of(R[top][:, None] * R[top][None]).max() == X.T_MAX
    # the menu reaches it, and a vector against a certain genotype gets as far as 28
    m = X.menu()
    Rm = X.factors(m)
    assert X._stop_of(Rm[:, None] * Rm[None]).max() == X.T_MAX
    assert X.own_stop(m).max() == 28


@pytest.mark.parametrize("miss", [False, True])
def test_every_step_up_to_t_max_occurs_in_the_scenes(miss):
    p, info, T = data(miss)
    assert 100 <= p.shape[1] <= 150 and p.shape[0] == X.N_IND == 130 and len(info) == p.shape[1]
    assert np.allclose(p.sum(-1), 1.0, atol=1e-15) and np.all(p >= 0)
    full = T[:X.TS, X.TS:2 * X.TS]
    assert set(np.unique(full)) == set(range(1, X.T_MAX + 1))
    assert set(np.unique(T[np.triu_indices(X.N_IND, 1)])) == set(range(1, X.T_MAX + 1))
    sweep = [x["site"] for x in info if x["kind"] == "sweep"]
    assert set(np.unique(full[:, :, sweep])) == set(range(1, X.T_MAX + 1))  # the sweep alone, both round lengths' edges in it
    if miss:
        gone = X.is_miss(p)
        assert np.all((1 <= gone.sum(0)) | (np.array([len(x["named"]) for x in info]) == X.N_IND))
        assert gone.sum() >= 4 * len(info)


@pytest.mark.parametrize("miss", [False, True])
def test_no_pair_of_the_scenes_comes_near_the_tolerance(miss):
    p, info, T = data(miss)
    M = X.margins(p)
    iu = np.triu_indices(X.N_IND, 1)
    worst = M[iu].min()
    print("smallest margin of the scenes (miss=%d): %.3g over %d (pair, site)s" % (miss, worst, M[iu].size))
    assert worst >= X.MIN_MARGIN
    assert X.MIN_MARGIN > 1000 * 4096 * 2.0 ** -52 and X.MIN_MARGIN > 50 * 2.0 ** -36  # the boundary test's band, the noting band


def test_each_scene_has_the_occupancy_it_is_named_for():
    p, info, T = data()
    after1, after2 = X.searching_after(T, 1), X.searching_after(T, 2)
    full = T[:X.TS, X.TS:2 * X.TS]
    own = X.own_stop(p)  # [individual][site]
    seen = set()
    for x in info:
        s, kind = x["site"], x["kind"]
        seen.add(kind)
        a1, a2 = after1[:, s], after2[:, s]
        if kind == "cols":
            k = x["k"]
            assert np.all(a1 == k) and np.all(a2 == 0), x["name"]  # every row: the k columns, done in round 2
            assert np.array_equal(np.where((full[:, :, s] > 16).any(0))[0], x["lanes"])
            assert (k >= X.PACK_DENSE) == (x["k"] in (24, 25, 63, 64))
            assert full[:, :, s].max() <= 28
        elif kind == "rows":
            rows = x["rows"]
            assert np.all(a1[rows] == X.TS) and np.all(np.delete(a1, rows) == 0) and np.all(a2 == 0), x["name"]
        elif kind == "edge":
            who = x["who"]
            assert np.all(T[:128, who, s].max(0) > 16)  # the edge tiles' columns search in round 2
            assert T[128, 129, s] > (32 if "long" in x["name"] or "rows" in x["name"] else 0)
        elif kind == "round3":
            rows, ls = x["rows"], x["lanes"]
            assert np.all(a2[rows] == len(ls)) and np.all(np.delete(a2, rows) == 0), x["name"]
            assert np.all(a1[rows] == X.TS) and np.all(np.delete(a1, rows) == len(ls))
            assert full[:, :, s].max() <= X.T_MAX and full[np.ix_(rows, ls)][:, :, s].min() >= 33
        elif kind == "skip":
            one, zero = {"r2-first-block": ((25, 28), (17, 24)), "r2-dense-sparse": ((17, 24), None),
                         "r2-skip-sparse": ((25, 28), None), "r1-first-block": ((9, 16), None),
                         "r1-second-block": ("dip", None)}[x["form"]]
            for w, flip in ((2, False), (5, True)):
                for r in range(8):
                    row = 8 * w + r
                    c = one if (x["pattern"][r] == "1") != flip else zero
                    R = X.factors(p[row, s])
                    if c is None:  # a fast row: done with the fast columns in round 1, never dense afterwards
                        assert own[row, s] == 2 and a1[row] < X.PACK_DENSE
                    elif c == "dip":  # can stop at step 1 and at no other step of round 1; dense in round 2
                        assert R[0] < X.E_TOLE and np.all(R[1:16] >= X.E_TOLE * (1 + 1e-6)) and a1[row] >= X.TS - 3
                        assert np.sum(full[row, :, s] == 1) == 3
                    else:
                        assert c[0] <= own[row, s] <= c[1], (x["name"], row, own[row, s])
                        # row_nostop of the blocks before its own stop: the row's factor alone is at or above e^tole there
                        assert np.all(R[:own[row, s] - 1] >= X.E_TOLE * (1 + 1e-9))
                        assert a1[row] == (X.TS if c[0] >= 17 else 0)
        elif kind == "sweep":
            # dense rows beside rows of one, two (three) packed units and rows that are done: in round 2 where only a few columns
            # are graded, in round 3 where all are
            a = a1 if "rows" in x["name"] else a2
            assert a.max() >= X.PACK_DENSE and np.any((a > 0) & (a < X.PACK_DENSE)), x["name"]
            if a is a2:
                assert np.all(a1 >= X.PACK_DENSE) and np.any(a2 == 0) and {1, 2} <= set(-(-a2 // 8)), x["name"]
    assert seen == {"cols", "edge", "rows", "skip", "round3", "sweep"}
    # one, two and three packed units per wavefront in round 2, and the dense line from both sides
    ks = sorted({x["k"] for x in info if x["kind"] == "cols"})
    assert {-(-k // 8) for k in ks if k < X.PACK_DENSE} == {1, 2, 3} and 23 in ks and 24 in ks


def test_expected_rounds_against_a_plain_loop_over_tiles():
    p, info, T = data()
    sub = p[:, ::9]  # a dozen scenes
    n_ind = 70       # three tiles, one of them six columns wide
    Ts = X.stop_steps(sub[:n_ind])
    for CH in (12, 16):
        total = 0
        for s in range(sub.shape[1]):
            for ti in range(2):
                for tj in range(ti, 2):
                    last = 0
                    for i in range(64 * ti, min(n_ind, 64 * ti + 64)):
                        for j in range(max(i + 1, 64 * tj), min(n_ind, 64 * tj + 64)):
                            last = max(last, int(Ts[i, j, s]))
                    r = 1
                    while r * CH < last:
                        r += 1
                    total += r
        assert X.expected_rounds(sub, CH, n_ind) == total
    # pairs with a missing individual leave at step 1
    pm, _ = X.scenes(miss=True)
    Tm, T0 = X.stop_steps(pm, True), X.stop_steps(pm)
    gone = X.is_miss(pm)
    either = (gone[:, None, :] | gone[None, :, :]) & np.triu(np.ones((X.N_IND, X.N_IND), bool), 1)[:, :, None]
    assert either.any() and np.all(Tm[either] == 1) and np.array_equal(Tm[~either], T0[~either]) and np.any(T0[either] > 16)
    assert X.expected_rounds(pm, 16, X.N_IND, True) <= X.expected_rounds(pm, 16, X.N_IND)


def test_the_probes_of_a_later_round_sit_where_they_are_meant_to():
    """the in-band probes of tests/test_gpu_em_rounds.py: stops in rounds 2 and 3, the pair's column alone (packed) or its
    row dense (plain scan) in that round, and no OTHER pair of those sites near the tolerance"""
    probes = X.boundary_probes(CASES, find_boundary)
    p, planted = X.probe_scenes(probes)
    T, M = X.stop_steps(p), X.margins(p)
    for (i1, i2, s, form), (g1, g2, rnd) in zip(planted, [q for q in probes for _ in range(2)]):
        t = int(T[i1, i2, s])
        assert 16 * (rnd - 1) < t <= 16 * rnd and abs(t - O.em2(g1, g2)[1]) <= 1
        assert M[i1, i2, s] < 2.0 ** -40  # inside the noting band
        left = X.searching_after(T, rnd - 1)[:, s]
        cols_left = int((T[:X.TS, X.TS:2 * X.TS, s] > 16 * (rnd - 1)).any(0).sum())
        if form == "packed" and rnd == 3:
            assert left[i1] == 1 and cols_left == 1
        elif form == "packed":
            assert left[i1] < X.PACK_DENSE and cols_left < 8
        else:
            assert left[i1] >= X.PACK_DENSE
        M[i1, i2, s] = np.inf
    assert M[np.triu_indices(X.N_IND, 1)].min() >= X.MIN_MARGIN
