"""The planner of the windowed calls' slab plans (ngsdist_amd/csrc/win_plan.h: engine_windows.hip windows_slab asks it for
every batch, windows_impl for the boundaries of its estimate) under AddressSanitizer + UBSan on the CPU, from a stand-alone
program: the batches, slice tables, window tables and block-start tables of a few thousand seeded cases, checked for what
the launches and kernels rely on and against a restatement of the loops windows_slab had before the planner was split off."""
import bisect
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
TAIL = 8           # NGD_KG_TAIL
PLANE = 128 * 128  # n_pad * n_pad of the smallest engine


@pytest.fixture(scope="module")
def plan_bin(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("wp") / "win_plan_san")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-D_GLIBCXX_ASSERTIONS", "-o", out, os.path.join(ROOT, "tests", "win_plan", "win_plan_main.cpp"),
           "-I" + os.path.join(ROOT, "ngsdist_amd", "csrc")]
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


def parent_bytes(env, n_seg, span, n_win, bt):
    """windows_batch_bytes() as it read its five values off the engine"""
    em, pdel, _, chunk = env
    n_ks = (n_seg + 7) // 8 * 8
    job = 0
    if bt:
        n_rep, n_blocks, _ = bt
        stride = (n_rep + chunk - 1) // chunk * chunk
        job = n_win * (n_blocks + 1) * 4 + n_blocks * stride * (12 if pdel else 8)
    cnt = n_seg * PLANE * 4 if pdel else 0
    if em:
        return (n_seg * PLANE * 8 + cnt + n_seg * 5 * 8 + n_win * 16 + job) & M64
    wkg = 3 * span // 4 + n_ks * (3 + TAIL) + 1 + TAIL
    return (n_ks * PLANE * 8 + cnt + wkg * 32 + n_ks * 5 * 8 + n_win * 16 + job) & M64


def win_bnd(lo, hi, bt):
    wb = [lo] + ([lo + b * bt[2] for b in range(1, bt[1] + 1)] if bt else [])
    if wb[-1] != hi:
        wb.append(hi)
    return wb


def parent_plan(env, lo, hi, budget, bt):
    """the loops of windows_slab() before win_plan.h, in the engine's unsigned 64-bit arithmetic: None where some window
    alone does not fit, else the batches (a, b, hi_max, n_seg, n_ks, max_wkg, w_total, tab, wt, blk)"""
    em, pdel, n_ks_plain, _ = env
    n_win = len(lo)
    for w in range(n_win):
        if parent_bytes(env, bt[1] + 1 if bt else 1, hi[w] - lo[w], 1, bt) > budget:
            return None
    out, a = [], 0
    while a < n_win:
        x, b, hi_max = [], a, 0
        while b < n_win:
            merged = sorted(set(x) | set(win_bnd(lo[b], hi[b], bt)))
            n_seg_ub, hm = (len(merged) - 1) & M64, max(hi_max, hi[b])
            if b > a and (parent_bytes(env, n_seg_ub, hm - lo[a], b + 1 - a, bt) > budget or n_seg_ub >= 1 << 30):
                break
            x, hi_max, b = merged, hm, b + 1
        nb = b - a
        at = lambda s: bisect.bisect_left(x, s)
        cover = [0] * len(x)
        for w in range(a, b):
            cover[at(lo[w])] += 1
            cover[at(hi[w])] -= 1
        piece = M64
        if em:
            covered = n_cov = n_cut = run = 0
            for k in range(len(x) - 1):
                run += cover[k]
                if run > 0:
                    covered += x[k + 1] - x[k]
                    n_cov += 1
            piece = max(64, (covered + n_ks_plain - 1) // max(1, n_ks_plain))
            run = 0
            for k in range(len(x) - 1):
                run += cover[k]
                if run > 0:
                    n_cut += (x[k + 1] - x[k] - 1) // piece + 1
            if n_cut > n_cov and (parent_bytes(env, n_cut, hi_max - lo[a], nb, bt) > budget or n_cut >= 1 << 30):
                piece = M64
        seg_of, seg_end, tab = [0] * len(x), [0] * len(x), []
        n_seg = wkg = max_wkg = run = 0
        for k in range(len(x) - 1):
            run += cover[k]
            seg_of[k] = seg_end[k] = n_seg
            if run <= 0:
                continue
            if em:
                ln = x[k + 1] - x[k]
                n_p = 1 if ln <= piece else (ln - 1) // piece + 1
                per = (ln + n_p - 1) // n_p
                s = x[k]
                while s < x[k + 1]:
                    tab.append((0, 0, 0, s, min(s + per, x[k + 1])))
                    s, n_seg = s + per, n_seg + 1
            else:
                kg0, kg1 = 3 * x[k] // 4, (3 * x[k + 1] + 3) // 4
                n_wkg = kg1 - kg0 + 1 + TAIL
                tab.append((kg0, kg1, wkg, x[k], x[k + 1]))
                wkg, max_wkg, n_seg = wkg + n_wkg, max(max_wkg, n_wkg), n_seg + 1
            seg_end[k] = n_seg
        seg_of[-1] = seg_end[-1] = n_seg
        n_ks = n_seg if em else (n_seg + 7) // 8 * 8
        tab += [(0, 0, wkg, 0, 0)] * (n_ks - n_seg)
        wt = [(seg_of[at(lo[w])], seg_end[at(hi[w]) - 1], hi[w] - lo[w]) for w in range(a, b)]
        blk = []
        for w in range(a, b) if bt else ():
            i, row = at(lo[w]), []
            for k in range(bt[1] + 1):
                while x[i] < lo[w] + k * bt[2]:
                    i += 1
                row.append(seg_of[i])
            blk.append(row)
        out.append((a, b, hi_max, n_seg, n_ks, max_wkg, wkg + 1 + TAIL, tab, wt, blk))
        a = b
    return out


def window_lists(rng):
    """(family, lo, hi, job or None): the shapes callers pass -- starts never decrease"""
    fam = int(rng.integers(8))
    bt = None
    if fam < 3:  # sliding windows: the step divides the length, does not, exceeds it (gaps)
        W = int(rng.choice([12, 64, 100, 600, 2000]))
        S = [W // int(rng.choice([1, 2, 4])), max(1, W // 3 + int(rng.integers(1, 7))), W + int(rng.integers(1, 50))][fam]
        if fam == 1 and W % S == 0:
            S += 1
        n = int(rng.integers(1, 25))
        first = int(rng.integers(0, 40))
        lo = [first + k * S for k in range(n)]
        hi = [l + W for l in lo]
    elif fam == 3:  # chromosome style: windows side by side inside stretches with unequal gaps between them
        lo, hi, at = [], [], int(rng.integers(0, 30))
        for _ in range(int(rng.integers(1, 5))):
            W, S = int(rng.choice([30, 100, 700])), int(rng.choice([10, 30, 100]))
            for k in range(int(rng.integers(1, 7))):
                lo.append(at + k * S)
                hi.append(at + k * S + W)
            at = hi[-1] + int(rng.choice([0, 1, 17, 333]))
    elif fam == 4:  # any list: equal starts, a window nested in the one before it, exact duplicates among them
        lo, hi, at = [], [], int(rng.integers(0, 50))
        for _ in range(int(rng.integers(1, 20))):
            kind = int(rng.integers(5)) if lo else 0
            if kind == 1:  # the same start, another length
                lo.append(lo[-1]); hi.append(lo[-1] + int(rng.integers(1, 300)))
            elif kind == 2 and hi[-1] - lo[-1] >= 3:  # nested: starts later, ends sooner
                lo.append(lo[-1] + 1); hi.append(hi[-1] - 1)
            elif kind == 3:  # a duplicate
                lo.append(lo[-1]); hi.append(hi[-1])
            else:
                at = max(at, lo[-1] if lo else 0) + int(rng.integers(0, 200))
                lo.append(at); hi.append(at + int(rng.integers(1, 400)))
    else:  # jobs: one length W, blocks of q sites
        W = int(rng.choice([24, 60, 96, 210]))
        S = int(rng.choice([W // 2, W // 3, W, W + 5, 7]))
        qs = {5: [1, 1, 2], 6: [d for d in range(2, S + 1) if S % d == 0 and d <= W] or [1], 7: [W // 2 + 1, W // 2 + 3, 5, 9, 11, 13, W]}[fam]
        q = int(rng.choice(qs))
        n = int(rng.integers(1, 9))
        first = int(rng.integers(0, 40))
        lo = [first + k * S for k in range(n)]
        if n > 2 and rng.integers(4) == 0:
            lo[2] = lo[1]  # (two windows of a job may coincide)
            lo.sort()
        hi = [l + W for l in lo]
        bt = (int(rng.choice([1, 3, 5, 16, 40])), W // q, q)
    return fam, lo, hi, bt


def cases(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        fam, lo, hi, bt = window_lists(rng)
        em, pdel = int(rng.integers(2)), int(rng.integers(2))
        env = (em, pdel, int(rng.choice([1, 8, 160])) if em else 0, reduce_chunk(bt[0]) if bt else 1)
        single = max(parent_bytes(env, bt[1] + 1 if bt else 1, h - l, 1, bt) for l, h in zip(lo, hi))
        n_bnd = len({s for l, h in zip(lo, hi) for s in win_bnd(l, h, bt)})
        whole = max(single, parent_bytes(env, 2 * n_bnd, max(hi) - lo[0], len(lo), bt))
        kind = int(rng.integers(4))  # unbounded; one window per batch; in between; below a single window
        budget = [M64, single, single + int(rng.integers(0, whole - single + 1)), single - 1][kind]
        out.append((env, lo, hi, bt, budget, kind, fam))
    return out


def intervals(pairs):
    """the union of [lo, hi) ranges given by ascending lo, as disjoint intervals"""
    out = []
    for l, h in pairs:
        if out and l <= out[-1][1]:
            out[-1][1] = max(out[-1][1], h)
        else:
            out.append([l, h])
    return out


def test_batches_and_tables_of_the_slab_plans(plan_bin):
    cs = cases(3000, 20241101)
    lines = []
    for env, lo, hi, bt, budget, _, _ in cs:
        em, pdel, n_ks_plain, chunk = env
        head = [em, pdel, n_ks_plain, TAIL, chunk, PLANE, budget] + (list(bt) if bt else [0, 0, 0]) + [len(lo)]
        lines.append(" ".join(map(str, head + [v for p in zip(lo, hi) for v in p])) + "\n")
    run_env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([plan_bin], input="".join(lines).encode(), capture_output=True, env=run_env, timeout=300)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, err[-3000:]
    blocks = r.stdout.decode().split("E\n")
    assert len(blocks) == len(cs) + 1 and blocks[-1] == ""
    seen = {"multi": 0, "cut": 0, "uncut_by_budget": 0, "pad": 0, "tail": 0, "split_block": 0, "gap": 0, "refused": 0}
    for c, text in zip(cs, blocks):
        env, lo, hi, bt, budget, kind, fam = c
        em, pdel, n_ks_plain, chunk = env
        n_win = len(lo)
        rows = [l.split() for l in text.splitlines()]
        ints = lambda tag: [[int(v) for v in x[1:]] for x in rows if x[0] == tag]
        # the estimate's distinct boundaries and the fit test, as windows_impl() and windows_slab() had them
        # (N: the former rule of windows_impl() spelled out -- every lo, every hi, every block start; win_bnd() above is the
        # header's rule, which leaves out a hi that equals the last block's end: the distinct values must be the same)
        assert ints("N") == [[len({s for l, h in zip(lo, hi) for s in ([l, h] + ([l + b * bt[2] for b in range(1, bt[1] + 1)] if bt else []))})]], c
        assert ints("S") == [[parent_bytes(env, bt[1] + 1 if bt else 1, h - l, 1, bt) for l, h in zip(lo, hi)]], c
        want = parent_plan(env, lo, hi, budget, bt)
        assert ints("F") == [[0 if want is None else 1]], c
        assert (want is None) == (kind == 3), c
        if want is None:
            assert not ints("B") and not ints("T") and not ints("W") and not ints("K"), c
            seen["refused"] += 1
            continue
        # ... and the whole plan, batch by batch
        got, ti, wi, ki = [], 0, 0, 0
        T, Wt, K = ints("T"), ints("W"), ints("K")
        for a, b, hi_max, n_seg, n_ks, max_wkg, w_total, nbytes in ints("B"):
            assert nbytes == parent_bytes(env, n_seg, hi_max - lo[a], b - a, bt), c
            got.append((a, b, hi_max, n_seg, n_ks, max_wkg, w_total, [tuple(t) for t in T[ti:ti + n_ks]],
                        [tuple(t) for t in Wt[wi:wi + b - a]], K[ki:ki + b - a] if bt else []))
            ti, wi, ki = ti + n_ks, wi + b - a, ki + (b - a if bt else 0)
        assert (ti, wi, ki) == (len(T), len(Wt), len(K)) and got == want, c
        at = 0
        for a, b, hi_max, n_seg, n_ks, max_wkg, w_total, tab, wt, blk in got:
            # batches: consecutive, non-empty; more than one window only within the budget
            assert a == at and b > a and hi_max == max(hi[a:b]), c
            at = b
            if b - a > 1:
                seen["multi"] += 1
                assert parent_bytes(env, n_seg, hi_max - lo[a], b - a, bt) <= budget, c
            if kind == 1 and fam < 3:  # (distinct starts, one length: a second window always adds bytes)
                assert b - a == 1, c
            # real slices: ascending, disjoint, non-empty, and together exactly the windows' sites
            real = tab[:n_seg]
            assert n_seg >= 1 and all(t[3] < t[4] for t in real) and all(p[4] <= t[3] for p, t in zip(real, real[1:])), c
            union = intervals(zip(lo[a:b], hi[a:b]))
            assert intervals((t[3], t[4]) for t in real) == union, c
            seen["gap"] += len(union) > 1
            if not em:
                # k-group ranges, weight regions back to back from 0, the padding to eights
                off = 0
                for kg0, kg1, woff, slo, shi in real:
                    assert (kg0, kg1, woff) == (3 * slo // 4, (3 * shi + 3) // 4, off), c
                    off += kg1 - kg0 + 1 + TAIL
                assert w_total == off + 1 + TAIL and max_wkg == max(t[1] - t[0] + 1 + TAIL for t in real), c
                assert n_ks % 8 == 0 and 0 <= n_ks - n_seg < 8 and tab[n_seg:] == [(0, 0, off, 0, 0)] * (n_ks - n_seg), c
                seen["pad"] += n_ks > n_seg
            else:
                # no padding; the pieces of an interval between two boundaries tile it, none longer than the rule allows
                assert n_ks == n_seg and all(t[:3] == (0, 0, 0) for t in tab), c
                bnd = sorted({s for w in range(a, b) for s in win_bnd(lo[w], hi[w], bt)})
                covered = sum(h - l for l, h in union)
                piece = max(64, (covered + n_ks_plain - 1) // max(1, n_ks_plain))
                n_cov = n_cut = 0
                for l, h in zip(bnd, bnd[1:]):
                    inside = [t for t in real if l <= t[3] and t[4] <= h]
                    if any(u[0] <= l and h <= u[1] for u in union):
                        n_cov, n_cut = n_cov + 1, n_cut + (h - l - 1) // piece + 1
                        assert inside and inside[0][3] == l and inside[-1][4] == h, c
                        assert all(p[4] == t[3] for p, t in zip(inside, inside[1:])), c
                    else:
                        assert not inside, c
                if n_seg == n_cov and n_cut > n_cov:  # uncut: only where the pieces' planes would not fit
                    assert parent_bytes(env, n_cut, hi_max - lo[a], b - a, bt) > budget, c
                    seen["uncut_by_budget"] += 1
                else:
                    assert n_seg == n_cut and all(t[4] - t[3] <= piece for t in real), c
                    seen["cut"] += n_cut > n_cov
            # window table: the slices [f, l) of a window tile exactly [lo, hi)
            for w, (f, l, ln) in zip(range(a, b), wt):
                assert 0 <= f < l <= n_seg and ln == hi[w] - lo[w], c
                assert real[f][3] == lo[w] and real[l - 1][4] == hi[w], c
                assert all(p[4] == t[3] for p, t in zip(real[f:l], real[f + 1:l])), c
            # a job: the slices [blk[k], blk[k + 1]) tile block k; the tail's slices follow the last block
            for w, row, (f, l, _) in zip(range(a, b), blk, wt):
                n_blocks, q = bt[1], bt[2]
                assert len(row) == n_blocks + 1 and row[0] == f and row[-1] <= l, c
                for k in range(n_blocks):
                    s = real[row[k]:row[k + 1]]
                    assert s and s[0][3] == lo[w] + k * q and s[-1][4] == lo[w] + (k + 1) * q, c
                    assert all(p[4] == t[3] for p, t in zip(s, s[1:])), c
                    seen["split_block"] += len(s) > 1
                if n_blocks * q < hi[w] - lo[w]:
                    assert row[-1] < l and real[row[-1]][3] == lo[w] + n_blocks * q, c
                    seen["tail"] += 1
                else:
                    assert row[-1] == l, c
        assert at == n_win, c
    # (the cases do reach every branch the checks above tell apart)
    assert all(v > 20 for v in seen.values()), seen
