"""The per-window forms of the slab planner (ngsdist_amd/csrc/win_plan.h win_each_fits_var / win_plan_batch_var: what
engine_windows.hip windows_slab_var tells the device for a job over windows of UNEQUAL length) under AddressSanitizer +
UBSan on the CPU, from a stand-alone program: batches, slice tables, window tables, descriptors, rows of block starts and
the classes' weight rows of seeded random window lists against a restatement in Python -- EM or MFMA kernel, with and
without --pairwise_del, the congruent image's layout, budgets that force several batches and split a class across them.
Windows of one length must get win_plan_batch's tables."""
import bisect
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
TAIL = 8           # NGD_KG_TAIL
PLANE = 128 * 128  # n_pad * n_pad of the smallest engine
DESC = 4           # NGD_WIN_DESC


@pytest.fixture(scope="module")
def plan_bin(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("wpv") / "win_plan_var_san")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-D_GLIBCXX_ASSERTIONS", "-o", out,
           os.path.join(ROOT, "tests", "win_plan_var", "win_plan_var_main.cpp"), "-I" + os.path.join(ROOT, "ngsdist_amd", "csrc")]
    r = subprocess.run(cmd, capture_output=True)
    if r.returncode != 0:
        err = r.stderr.decode()
        # only a missing sanitizer runtime is a reason to skip
        if "libasan" in err or "libubsan" in err or "unrecognized" in err and "fsanitize" in err:
            pytest.skip("no sanitizer runtime here: " + err[-300:])
        pytest.fail("the planner does not build on its own:\n" + err[-2000:])
    return out


def reduce_chunk(n_rep):
    return 1 if n_rep <= 1 else 4 if n_rep <= 4 else 16 if n_rep <= 16 else 32


def plain_bytes(env, n_seg, span, n_win):
    """win_batch_bytes() without a job"""
    em, pdel, _, _, quad = env
    n_ks = (n_seg + 7) // 8 * 8
    cnt = n_seg * PLANE * 4 if pdel else 0
    if em:
        return n_seg * PLANE * 8 + cnt + n_seg * 5 * 8 + n_win * 16
    wkg = 3 * span // 4 + n_ks * ((7 if quad else 3) + TAIL) + 1 + TAIL
    return n_ks * PLANE * 8 + cnt + wkg * 32 + n_ks * 5 * 8 + n_win * 16


def var_bytes(env, n_seg, span, n_win, blk_entries, wt_rows, n_rep):
    """+ the rows of block starts, four words per window, the weight rows of the classes held"""
    chunk, pdel = env[3], env[1]
    stride = (n_rep + chunk - 1) // chunk * chunk
    return (plain_bytes(env, n_seg, span, n_win) + blk_entries * 4 + n_win * DESC * 8 + wt_rows * stride * (12 if pdel else 8)) & M64


def win_bnd(lo, hi, q):
    wb = [lo + b * q for b in range((hi - lo) // q + 1)]
    if wb[-1] != hi:
        wb.append(hi)
    return wb


def kg_lo(s, quad):
    return 3 * (s >> 2) if quad else (3 * s) >> 2


def kg_hi(s, quad):
    return 3 * ((s + 3) >> 2) if quad else (3 * s + 3) >> 2


def plan(env, lo, hi, cls, budget, n_rep, q):
    """the definition: None where some window alone does not fit, else the batches"""
    em, pdel, n_ks_plain, chunk, quad = env
    stride = (n_rep + chunk - 1) // chunk * chunk
    n_win = len(lo)
    nbk = [(h - l) // q for l, h in zip(lo, hi)]
    for w in range(n_win):
        if var_bytes(env, nbk[w] + 1, hi[w] - lo[w], 1, nbk[w] + 1, nbk[w], n_rep) > budget:
            return None
    # a batch's slices are cut by every boundary of the CALL inside its span: the same slices under any budget
    every = sorted({s for l, h in zip(lo, hi) for s in win_bnd(l, h, q)})
    out, a = [], 0
    while a < n_win:
        x, b, hi_max, blk_entries, wt_rows, rows, order = [], a, 0, 0, 0, {}, []
        while b < n_win:
            hm = max(hi_max, hi[b])
            merged = [s for s in every if lo[a] <= s <= hm]
            n_seg_ub = len(merged) - 1
            fresh = nbk[b] > 0 and cls[b] not in rows
            be, wr = blk_entries + nbk[b] + 1, wt_rows + (nbk[b] if fresh else 0)
            if b > a and (var_bytes(env, n_seg_ub, hm - lo[a], b + 1 - a, be, wr, n_rep) > budget or n_seg_ub >= 1 << 30):
                break
            if fresh:
                rows[cls[b]] = wt_rows
                order.append(cls[b])
            x, hi_max, blk_entries, wt_rows, b = merged, hm, be, wr, b + 1
        nb = b - a
        at = lambda s: bisect.bisect_left(x, s)
        cover = [0] * len(x)
        for w in range(a, b):
            cover[at(lo[w])] += 1
            cover[at(hi[w])] -= 1
        for k in range(1, len(x)):
            cover[k] += cover[k - 1]
        piece = M64
        if em:
            ivs = [(x[k], x[k + 1]) for k in range(len(x) - 1) if cover[k] > 0]
            piece = max(64, (sum(h - l for l, h in ivs) + n_ks_plain - 1) // max(1, n_ks_plain))
            n_cut = sum((h - l - 1) // piece + 1 for l, h in ivs)
            if n_cut > len(ivs) and (var_bytes(env, n_cut, hi_max - lo[a], nb, blk_entries, wt_rows, n_rep) > budget or n_cut >= 1 << 30):
                piece = M64
        seg_of, seg_end, tab = [0] * len(x), [0] * len(x), []
        n_seg = wkg = max_wkg = 0
        for k in range(len(x) - 1):
            seg_of[k] = seg_end[k] = n_seg
            if cover[k] <= 0:
                continue
            if em:
                ln = x[k + 1] - x[k]
                n_p = 1 if ln <= piece else (ln - 1) // piece + 1
                per = (ln + n_p - 1) // n_p
                for s in range(x[k], x[k + 1], per):
                    tab.append((0, 0, 0, s, min(s + per, x[k + 1])))
                    n_seg += 1
            else:
                kg0, kg1 = kg_lo(x[k], quad), kg_hi(x[k + 1], quad)
                tab.append((kg0, kg1, wkg, x[k], x[k + 1]))
                wkg, max_wkg, n_seg = wkg + kg1 - kg0 + 1 + TAIL, max(max_wkg, kg1 - kg0 + 1 + TAIL), n_seg + 1
            seg_end[k] = n_seg
        seg_of[-1] = seg_end[-1] = n_seg
        n_ks = n_seg if em else (n_seg + 7) // 8 * 8
        tab += [(0, 0, wkg, 0, 0)] * (n_ks - n_seg)
        wt = [(seg_of[at(lo[w])], seg_end[at(hi[w]) - 1], hi[w] - lo[w]) for w in range(a, b)]
        desc, blk, off = [], [], 0
        for w in range(a, b):
            desc.append((off, nbk[w], rows[cls[w]] * stride if nbk[w] else 0, nbk[w] * q))
            blk.append([seg_of[at(lo[w] + k * q)] for k in range(nbk[w] + 1)])
            off += nbk[w] + 1
        out.append((a, b, hi_max, n_seg, n_ks, max_wkg, wkg + 1 + TAIL, var_bytes(env, n_seg, hi_max - lo[a], nb, off, wt_rows, n_rep),
                    wt_rows, tab, wt, desc, blk, [(c, rows[c]) for c in order]))
        a = b
    return out


def window_lists(rng):
    """windows of unequal length with starts that never decrease; every fourth list has one length"""
    fam = int(rng.integers(4))
    n = int(rng.integers(1, 30))
    if fam == 0:  # one length: sliding windows
        W, S = int(rng.choice([12, 60, 96, 210])), int(rng.choice([7, 20, 48, 250]))
        first = int(rng.integers(0, 40))
        lo = [first + k * S for k in range(n)]
        hi = [l + W for l in lo]
    elif fam == 1:  # coordinate windows: sites at uneven positions, windows of `size` every `step`
        pos = np.cumsum(rng.integers(1, 40, 400) * rng.choice([1, 1, 1, 12], 400))
        size, step = int(rng.choice([300, 1000, 2500])), int(rng.choice([100, 400, 1000]))
        lo, hi = [], []
        for k in range((int(pos[-1]) - 1) // step + 1):
            l, h = int(np.searchsorted(pos, 1 + k * step)), int(np.searchsorted(pos, 1 + k * step + size))
            if h > l:
                lo.append(l)
                hi.append(h)
        lo, hi = lo[:n], hi[:n]
    else:  # any list: equal starts, nested windows, duplicates, gaps, a few lengths that come back
        lens = [int(v) for v in rng.integers(1, 150, 4)]
        lo, hi, at = [], [], int(rng.integers(0, 50))
        for _ in range(n):
            kind = int(rng.integers(4)) if lo else 0
            if kind == 1:
                lo.append(lo[-1]); hi.append(lo[-1] + int(rng.choice(lens)))
            elif kind == 2:
                lo.append(lo[-1]); hi.append(hi[-1])
            else:
                at = max(at, lo[-1] if lo else 0) + int(rng.integers(0, 120))
                lo.append(at); hi.append(at + int(rng.choice(lens)))
    return fam, lo, hi


def cases(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        fam, lo, hi = window_lists(rng)
        q = int(rng.choice([1, 3, 7, 20, 64, 200]))
        n_rep = int(rng.choice([1, 3, 5, 16, 40]))
        # classes: windows that share n_blocks and an offset -- here one offset per n_blocks, or (a caller's own maps) two
        two = int(rng.integers(3)) == 0
        ids, cls = {}, []
        for w, (l, h) in enumerate(zip(lo, hi)):
            nb = (h - l) // q
            cls.append(ids.setdefault((nb, w % 2 if two else 0), len(ids)) if nb else -1)
        em, pdel = int(rng.integers(2)), int(rng.integers(2))
        env = (em, pdel, int(rng.choice([1, 8, 160])) if em else 0, reduce_chunk(n_rep), 0 if em else int(rng.integers(2)))
        nbk = [(h - l) // q for l, h in zip(lo, hi)]
        single = max(var_bytes(env, k + 1, h - l, 1, k + 1, k, n_rep) for l, h, k in zip(lo, hi, nbk))
        n_bnd = len({s for l, h in zip(lo, hi) for s in win_bnd(l, h, q)})
        whole = max(single, var_bytes(env, 2 * n_bnd, max(hi) - lo[0], len(lo), sum(nbk) + len(lo), sum(nbk), n_rep))
        kind = int(rng.integers(4))  # unbounded; one window per batch; in between; below a single window
        budget = [M64, single, single + int(rng.integers(0, whole - single + 1)), single - 1][kind]
        out.append((env, lo, hi, cls, budget, n_rep, q, kind, fam))
    return out


def test_batches_tables_and_descriptors_of_the_unequal_length_job(plan_bin):
    cs = cases(2500, 20261019)
    lines = []
    for env, lo, hi, cls, budget, n_rep, q, _, _ in cs:
        em, pdel, n_ks_plain, chunk, quad = env
        head = [em, pdel, n_ks_plain, TAIL, chunk, PLANE, quad, budget, n_rep, q, len(lo)]
        lines.append(" ".join(map(str, head + [v for t in zip(lo, hi, cls) for v in t])) + "\n")
    run_env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([plan_bin], input="".join(lines).encode(), capture_output=True, env=run_env, timeout=300)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, err[-3000:]
    blocks = r.stdout.decode().split("E\n")
    assert len(blocks) == len(cs) + 1 and blocks[-1] == ""
    seen = {"multi": 0, "class_split": 0, "class_shared": 0, "no_block": 0, "quad": 0, "em_cut": 0, "one_length": 0, "refused": 0,
            "pdel": 0, "tail": 0}
    for c, text in zip(cs, blocks):
        env, lo, hi, cls, budget, n_rep, q, kind, fam = c
        rows = [l.split() for l in text.splitlines()]
        ints = lambda tag: [[int(v) for v in x[1:]] for x in rows if x[0] == tag]
        nbk = [(h - l) // q for l, h in zip(lo, hi)]
        assert ints("S") == [[var_bytes(env, k + 1, h - l, 1, k + 1, k, n_rep) for l, h, k in zip(lo, hi, nbk)]], c
        want = plan(env, lo, hi, cls, budget, n_rep, q)
        assert ints("F") == [[0 if want is None else 1]] and (want is None) == (kind == 3), c
        if want is None:
            assert not ints("B") and not ints("T") and not ints("D"), c
            seen["refused"] += 1
            continue
        T, Wt, D, K = ints("T"), ints("W"), ints("D"), ints("K")
        Cl = [[tuple(int(v) for v in t.split(":")) for t in x[1:]] for x in rows if x[0] == "C"]
        got, ti, wi = [], 0, 0
        for (a, b, hi_max, n_seg, n_ks, max_wkg, w_total, nbytes, wt_rows), cl in zip(ints("B"), Cl):
            got.append((a, b, hi_max, n_seg, n_ks, max_wkg, w_total, nbytes, wt_rows, [tuple(t) for t in T[ti:ti + n_ks]],
                        [tuple(t) for t in Wt[wi:wi + b - a]], [tuple(t) for t in D[wi:wi + b - a]], K[wi:wi + b - a], cl))
            ti, wi = ti + n_ks, wi + b - a
        assert (ti, wi) == (len(T), len(Wt)) and len(Cl) == len(got) and got == want, c
        # what the kernel relies on, spelled out on the plan itself
        at, held = 0, {}
        stride = (n_rep + env[3] - 1) // env[3] * env[3]
        for a, b, hi_max, n_seg, n_ks, _, _, nbytes, wt_rows, tab, wt, desc, blk, cl in got:
            assert a == at and b > a, c
            at = b
            seen["multi"] += b - a > 1
            if b - a > 1:
                assert nbytes <= budget, c
            real = tab[:n_seg]
            rows_of = dict(cl)
            assert sorted(rows_of) == sorted({cls[w] for w in range(a, b) if nbk[w]}), c  # the batch's own classes only
            assert wt_rows == sum(nbk[[w for w in range(a, b) if cls[w] == k][0]] for k in rows_of), c
            off = 0
            for w, (f, l, _), (boff, nb, woff, vis), row in zip(range(a, b), wt, desc, blk):
                assert (boff, nb, vis) == (off, nbk[w], nbk[w] * q) and len(row) == nb + 1 and row[0] == f and row[-1] <= l, c
                off += nb + 1
                for k in range(nb):  # the slices [row[k], row[k + 1]) tile block k
                    s = real[row[k]:row[k + 1]]
                    assert s and s[0][3] == lo[w] + k * q and s[-1][4] == lo[w] + (k + 1) * q, c
                    assert all(p[4] == t[3] for p, t in zip(s, s[1:])), c
                if nb:
                    assert woff == rows_of[cls[w]] * stride and woff + nb * stride <= wt_rows * stride, c
                    seen["tail"] += row[-1] < l
                else:
                    seen["no_block"] += 1
            for k in rows_of:
                held.setdefault(k, set()).add(a)
            seen["class_shared"] += len([w for w in range(a, b) if nbk[w]]) > len(rows_of)
        assert at == len(lo), c
        seen["class_split"] += any(len(v) > 1 for v in held.values())
        seen["quad"] += env[4]
        seen["pdel"] += env[1]
        bset = {s for l, h in zip(lo, hi) for s in win_bnd(l, h, q)}  # (a slice that starts off every boundary: an EM piece)
        seen["em_cut"] += any(t[3] not in bset for g in got for t in g[9][:g[3]])
        if fam == 0:  # one length: the tables of win_plan_batch
            assert ints("Q") == [[1]], c
            seen["one_length"] += 1
        else:
            assert ints("Q") in ([], [[1]]), c  # (a random list may have one length too)
    assert all(v > 20 for v in seen.values()), seen
