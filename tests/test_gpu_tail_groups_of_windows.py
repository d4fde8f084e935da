"""The tails of the windowed calls across groups of windows (engine_windows.hip windows_chunked).

A windowed call with host outputs works its windows in groups whose matrices fit ~2 GB of the engine's batch buffers, and the
tail of every group -- the copy, the distances, the group means, the bootstrap summaries, the trees -- writes at an offset
that the group's first window decides.  At real sizes only a call of a thousand individuals spans two groups, so the test
hook NGD_TEST_WIN_GROUP_BYTES (under NGD_ENABLE_TEST_HOOKS=1) cuts the budget until a group holds 2 of this file's 7
windows: 4 groups, the last one partial.  Under the per-window plan (NGD_OPT_WIN_PLAN = 1) a window's matrices do not depend
on the windows beside it, so every output of the cut call must equal the whole call's bit for bit, NaN cells included.
(The segment-slab plan adds a window up from the segments its batch's boundaries cut, and the automatic choice weighs the
windows of a group: there the last bits of a sum depend on the group, whatever the tail does.  That plan serves here only
to show that the hook cuts: a batch does not span groups, so 4 groups are 4 batches at least.)"""
import numpy as np
import pytest

import test_gpu_boot_stats as TB

pytestmark = pytest.mark.gpu

N_IND, N_SITES, N_REP, Q = 10, 96, 4, 8
N_PAIRS = 45
# 7 windows of unequal length; [10, 15) and [40, 47) are shorter than one block: their replicates are 0 / 0
LO = np.array([0, 0, 10, 24, 40, 41, 60])
HI = np.array([96, 30, 15, 50, 47, 96, 93])
# 5 groups, group 1 of one individual (its diagonal has no cell: NaN, used 0)
GROUPS = np.random.default_rng(2).permutation(np.repeat(np.arange(5), [3, 1, 2, 2, 2]))
PER_GROUP = 2  # windows a group holds under the hook


def N():
    import ngsdist_amd
    return ngsdist_amd


NONE = np.zeros(0, dtype=np.uint64)


def nj_pairs(r):
    child, length, status, dist0 = r
    return [(length, child), (dist0, status)]


def same(a, b):
    """lists of (float64 array, integer array): same shapes, the floats equal by their bits, the integers by value"""
    return len(a) == len(b) and all(x[0].shape == y[0].shape and x[1].shape == y[1].shape and TB.same_bits(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("kernel", ["mfma", "em_table"])
def test_every_tail_across_groups_of_windows(kernel, monkeypatch):
    maps, off = N().window_boot_maps(9, LO, HI, N_REP, Q)
    p = TB.synth(31, N_IND, N_SITES, miss_frac=0.3)
    job = (LO, HI, maps, off, Q)
    with N().Engine(N_IND, N_SITES, kernel=kernel, indep_geno=kernel == "mfma", pairwise_del=True) as e:
        e.upload_ind_major(p).commit().set_groups(GROUPS, 5)
        # (name, matrices per window, the call -> a list of (float64 array, integer array))
        calls = [
            ("run_windows_groups", 1, lambda: [e.run_windows_groups(LO, HI, evol_model=1)]),
            ("run_windows_job_var_groups", N_REP + 1, lambda: [e.run_windows_job_var_groups(*job, evol_model=2, n_rep=N_REP)]),
            ("run_windows_job_var_stats", N_REP + 1, lambda: [e.run_windows_job_var_stats(*job, evol_model=1, n_rep=N_REP)]),
            ("run_windows_job_var_groups_stats", N_REP + 1,
             lambda: [e.run_windows_job_var_groups_stats(*job, evol_model=1, n_rep=N_REP)]),
            ("run_windows_nj", 1, lambda: nj_pairs(e.run_windows_nj(LO, HI, evol_model=0, dist0=True))),
            ("run_windows_job_var_nj", N_REP + 1, lambda: nj_pairs(e.run_windows_job_var_nj(*job, evol_model=0, n_rep=N_REP, dist0=True))),
            ("run_windows_job_var", N_REP + 1, lambda: [e.run_windows_job_var(*job, n_rep=N_REP)]),
            ("run_windows_job_var_dist", N_REP + 1, lambda: [(e.run_windows_job_var_dist(*job, evol_model=1, n_rep=N_REP), NONE)]),
        ]
        # the hook cuts the groups, and only behind its gate
        e.set_option("win_plan", 2)
        for gate, groups in ((None, 1), ("0", 1), ("1", -(-len(LO) // PER_GROUP))):
            monkeypatch.setenv("NGD_TEST_WIN_GROUP_BYTES", str(PER_GROUP * 16 * N_PAIRS))
            if gate is None:
                monkeypatch.delenv("NGD_ENABLE_TEST_HOOKS", raising=False)
            else:
                monkeypatch.setenv("NGD_ENABLE_TEST_HOOKS", gate)
            e.run_windows_groups(LO, HI)
            assert e.windows_info()["batches"] == groups, gate
        e.set_option("win_plan", 1)
        for name, n_mat, call in calls:
            monkeypatch.delenv("NGD_ENABLE_TEST_HOOKS", raising=False)
            monkeypatch.delenv("NGD_TEST_WIN_GROUP_BYTES", raising=False)
            whole = call()
            monkeypatch.setenv("NGD_ENABLE_TEST_HOOKS", "1")
            monkeypatch.setenv("NGD_TEST_WIN_GROUP_BYTES", str(PER_GROUP * 16 * n_mat * N_PAIRS))
            cut = call()
            assert same(whole, cut), name
            # the test's own eyes: NaN cells are among what was compared
            if name.endswith("stats") or name.endswith("_dist"):
                assert np.isnan(whole[0][0]).any() and np.isfinite(whole[0][0]).any(), name
