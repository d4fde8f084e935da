"""Neighbour-joining trees, the part that needs no device (include/ngsdist_amd.h "Neighbour-joining trees"): the new names
in the header, the binding list and the library; ngd_nj_host against the dictionary statement of the contract
(nj_expect.py) bit for bit -- n = 3 (no join), 4, 5, random 9 and 33, an all-equal matrix where every decision is a tie, a
small-integer matrix with many ties; additive trees recovered exactly (bipartitions and the multiset of branch lengths, by
bits); NaN / inf matrices without a tree beside intact neighbours; the refusals; ngd_nj_newick and ngd_nj_support."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import nj_expect as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["ngd_nj_max_ind", "ngd_nj_host", "ngd_nj_values_device", "ngd_nj_device", "ngd_run_job_nj", "ngd_run_windows_nj",
       "ngd_run_windows_job_var_nj", "ngd_last_nj_ms", "ngd_nj_support", "ngd_nj_newick"]


@pytest.fixture(scope="module")
def N():
    os.environ.setdefault("NGD_NO_TORCH", "1")
    import ngsdist_amd
    return ngsdist_amd


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.uint64), np.ascontiguousarray(b, dtype=np.float64).view(np.uint64))


def check_against_expect(N, vals, n):
    c, l, s = N.nj_host(vals, n)
    ce, le, se = X.nj_many(vals, n)
    assert np.array_equal(s, se)
    assert np.array_equal(c, ce)
    assert same_bits(l, le)
    return c, l, s


def test_header_binding_list_and_library_declare_the_new_names(N):
    from ngsdist_amd import _lib
    txt = open(os.path.join(ROOT, "include", "ngsdist_amd.h")).read()
    decl = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    L = _lib.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, decl), name + " is not declared in the header"
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert re.search(r"#define\s+NGD_OPT_NJ_MAX_BYTES\s+19\b", decl)
    assert re.search(r"#define\s+NGD_NJ_NBRANCH\(n\)\s+\(2 \* \(n\) - 3\)", decl)
    assert L.ngd_abi_version() == 6
    assert N.nj_max_ind() >= 1000


@pytest.mark.parametrize("n", [3, 4, 5, 9, 33])
def test_host_equals_the_statement_on_random_values(N, n):
    rng = np.random.default_rng(100 + n)
    vals = rng.uniform(0.05, 1.5, size=(6, n * (n - 1) // 2))
    c, l, s = check_against_expect(N, vals, n)
    assert np.all(s == 1) and c.shape == (6, 2 * n - 3)
    for rec in c:  # every node but the three at the centre is a child exactly once
        assert sorted(rec.tolist()) == list(range(2 * n - 3))


@pytest.mark.parametrize("n", [4, 7, 12])
def test_ties_go_to_the_lower_ids(N, n):
    p = n * (n - 1) // 2
    rng = np.random.default_rng(7)
    vals = np.stack([np.full(p, 0.25), np.ones(p), rng.integers(1, 4, size=p).astype(np.float64),
                     rng.integers(0, 2, size=p).astype(np.float64)])
    c, _, _ = check_against_expect(N, vals, n)
    assert c[0][0] == 0 and c[0][1] == 1  # all equal: the first join is (0, 1)


@pytest.mark.parametrize("n", [4, 5, 9, 33, 70])
def test_additive_trees_are_recovered_exactly(N, n):
    for seed in range(3):
        vals, splits, lengths = X.random_tree(n, 1000 * n + seed)
        c, l, s = N.nj_host(vals[None, :], n)
        assert s[0] == 1
        assert set(X.record_splits(c[0], n)) == splits
        assert same_bits(np.sort(l[0]), np.array(lengths))


def test_the_statement_recovers_additive_trees_too():
    vals, splits, lengths = X.random_tree(9, 5)
    c, l, s = X.nj(vals, 9)
    assert s == 1 and set(X.record_splits(c, 9)) == splits and sorted(l) == lengths


def test_a_matrix_that_is_not_finite_has_no_tree_and_leaves_its_neighbours_alone(N):
    n = 9
    rng = np.random.default_rng(3)
    vals = rng.uniform(0.1, 1.0, size=(5, n * (n - 1) // 2))
    clean = vals.copy()
    vals[1, 17] = np.nan
    vals[3, 0] = np.inf
    vals[4, -1] = -np.inf
    c, l, s = check_against_expect(N, vals, n)
    assert s.tolist() == [1, 0, 1, 0, 0]
    for k in (1, 3, 4):
        assert np.all(c[k] == -1) and np.all(l[k].view(np.uint64) == X.NAN_BITS)
    c0, l0, _ = N.nj_host(clean, n)
    for k in (0, 2):
        assert np.array_equal(c[k], c0[k]) and same_bits(l[k], l0[k])


def test_threads_change_no_bit(N):
    n = 12
    vals = np.random.default_rng(9).uniform(0.1, 1.0, size=(70, n * (n - 1) // 2))
    c, l, s = N.nj_host(vals, n)
    for k in (0, 33, 69):
        c1, l1, s1 = N.nj_host(vals[k], n)
        assert np.array_equal(c[k], c1) and same_bits(l[k], l1) and s1 == 1


def test_refusals(N):
    from ngsdist_amd import _lib
    L = _lib.load()
    v = np.ones(3)
    child = np.zeros(3, dtype=np.int32)
    ln = np.zeros(3)
    st = np.zeros(1, dtype=np.uint32)
    vp, cp, lp, sp = (v.ctypes.data_as(C.POINTER(C.c_double)), child.ctypes.data_as(C.POINTER(C.c_int32)),
                      ln.ctypes.data_as(C.POINTER(C.c_double)), st.ctypes.data_as(C.POINTER(C.c_uint32)))
    assert L.ngd_nj_host(vp, 1, 3, cp, lp, sp) == 0
    assert L.ngd_nj_host(None, 1, 3, cp, lp, sp) == -1
    assert L.ngd_nj_host(vp, 1, 3, None, lp, sp) == -1
    assert L.ngd_nj_host(vp, 1, 3, cp, None, sp) == -1
    assert L.ngd_nj_host(vp, 1, 3, cp, lp, None) == -1
    assert L.ngd_nj_host(vp, 0, 3, cp, lp, sp) == -1
    assert L.ngd_nj_host(vp, 1, 2, cp, lp, sp) == -1
    sup = np.zeros(1, dtype=np.uint32)
    used = C.c_uint32(0)
    assert L.ngd_nj_support(None, sp, 1, 3, sup.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(used)) == -1
    assert L.ngd_nj_support(cp, sp, 0, 3, sup.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(used)) == -1
    assert L.ngd_nj_newick(None, lp, 3, None, None, None, 0) == -1
    assert L.ngd_nj_newick(cp, lp, 2, None, None, None, 0) == -1
    # n = 5: the centre names node 7, which no join makes; join 0 names its own node 5 (a walk that would never end)
    for rec in ([0, 1, 5, 2, 3, 4, 7], [5, 1, 2, 3, 5, 6, 4]):
        bad = np.array(rec, dtype=np.int32)
        assert L.ngd_nj_newick(bad.ctypes.data_as(C.POINTER(C.c_int32)), np.zeros(7).ctypes.data_as(C.POINTER(C.c_double)), 5, None,
                               None, None, 0) == -1


def test_newick_parses_back_to_the_record(N):
    n = 9
    vals = np.random.default_rng(21).uniform(0.1, 1.0, size=n * (n - 1) // 2)
    c, l, s = N.nj_host(vals, n)
    labels = ["L%d_x" % k for k in range(n)]
    text = N.nj_newick(c, l, labels).decode()
    assert text.endswith(");\n") and text.count("\n") == 1 and text.count("(") == n - 2
    splits, nodes = X.parse_newick(text)
    want = X.record_splits(c, n)
    norm = [X._normal([labels.index(x) for x in sp], n) for sp in splits]
    assert set(norm) == set(want) and len(norm) == n - 3
    # every branch at %.10f, in the order the walk closes them: each record entry once
    assert sorted(ln for _, ln in nodes) == sorted("%.10f" % x for x in l)
    by_leaf = {name: ln for name, ln in nodes if name in labels}
    for e in range(2 * n - 3):
        if c[e] < n:
            assert by_leaf[labels[c[e]]] == "%.10f" % l[e]
    # children in recorded order: the three at the centre are the last three entries
    assert text.startswith("(" + (labels[c[-3]] + ":" if c[-3] < n else "("))
    # supports follow the closing bracket of their join
    sup = np.arange(100, 100 + n - 3, dtype=np.uint32)
    text2 = N.nj_newick(c, l, labels, sup).decode()
    splits2, nodes2 = X.parse_newick(text2)
    inner = [(name, sp) for (name, _), sp in zip([x for x in nodes2 if x[0] not in labels], splits2)]
    assert len(inner) == n - 3
    for name, sp in inner:
        t = want.index(X._normal([labels.index(x) for x in sp], n))
        assert name == str(100 + t)
    # default labels, and a record without a tree
    assert N.nj_newick(np.array([0, 1, 2], dtype=np.int32), np.array([0.5, 0.25, -0.125]), ["a", "b", "c"]) == \
        b"(a:0.5000000000,b:0.2500000000,c:-0.1250000000);\n"
    assert N.nj_newick(np.full(2 * n - 3, -1, dtype=np.int32), np.full(2 * n - 3, np.nan), labels) == b";\n"


def test_newick_sizes_like_format_matrix(N):
    from ngsdist_amd import _lib
    L = _lib.load()
    c = np.array([0, 1, 2], dtype=np.int32)
    l = np.array([0.5, 0.25, 1.0])
    args = (c.ctypes.data_as(C.POINTER(C.c_int32)), l.ctypes.data_as(C.POINTER(C.c_double)), 3, None, None)
    need = L.ngd_nj_newick(*args, None, 0)
    want = b"(Ind_0:0.5000000000,Ind_1:0.2500000000,Ind_2:1.0000000000);\n"
    assert need == len(want)
    buf = C.create_string_buffer(b"#" * (need + 4), need + 4)
    assert L.ngd_nj_newick(*args, buf, need - 1) == need and buf.raw == b"#" * (need + 4)  # too small: nothing written
    assert L.ngd_nj_newick(*args, buf, need) == need and buf.raw == want + b"####"


def rec4(first, centre):
    """a record of four leaves: one join, three at the centre"""
    return list(first) + list(centre)


def test_support_counts_both_records_of_one_tree_alike(N):
    n = 4
    # tree {0,1}|{2,3}: joined as (0,1) -> centre 2,3,4, or as (2,3) -> centre 0,1,4; tree {0,2}|{1,3} differs
    a = rec4((0, 1), (2, 3, 4))
    b = rec4((2, 3), (0, 1, 4))
    other = rec4((0, 2), (1, 3, 4))
    none = [-1] * 5
    child = np.array([a, b, a, other, none, b], dtype=np.int32)
    status = np.array([1, 1, 1, 1, 0, 1], dtype=np.uint32)
    sup, used = N.nj_support(child, status, n)
    assert sup.tolist() == [3] and used == 4  # the replicate without a tree is left out of n_used
    child[0] = b
    sup, used = N.nj_support(child, status, n)
    assert sup.tolist() == [3] and used == 4
    # matrix 0 without a tree: every support 0, the replicates with a tree still counted
    status0 = status.copy()
    status0[0] = 0
    child[0] = none
    sup, used = N.nj_support(child, status0, n)
    assert sup.tolist() == [0] and used == 4


def test_support_on_real_records(N):
    n = 9
    rng = np.random.default_rng(5)
    base = rng.uniform(0.2, 1.0, size=n * (n - 1) // 2)
    vals = np.stack([base] + [base + rng.normal(0, 0.05, size=base.size) for _ in range(12)])
    vals[4, 3] = np.nan
    c, l, s = N.nj_host(vals, n)
    sup, used = N.nj_support(c, s, n)
    assert used == 11
    ref = X.record_splits(c[0], n)
    want = [sum(1 for r in range(1, 13) if s[r] and ref[t] in set(X.record_splits(c[r], n))) for t in range(n - 3)]
    assert sup.tolist() == want
    sup3, used3 = N.nj_support(np.array([[0, 1, 2]] * 3, dtype=np.int32), np.ones(3, dtype=np.uint32), 3)
    assert sup3.size == 0 and used3 == 2
