"""--mds K --mds_align end to end through the C++ host (ngsdist_amd/bin/ngsDist) on a 12 x 400 text file, with --n_boot_rep 5
and with --win_size .. --win_boot_rep 5: <out> and <out>.mds -- matrix 0 of every set -- are byte for byte those of the run
without --mds_align (its matrix 0 blocks); <out>.mds_mean / _sd / _lo / _hi and <out>.mds_fit parse to the values the Python
door gives on the same data, seed and block size, at the printed precision ("%.10e"); the refused flag combinations exit
non-zero with a message.  Under NGSDIST_WIN_GROUP_MAX=3 the host sends the 7 windows to the engine in calls of 3, 3 and 1: the
files are those of the Python calls on the same three groups of windows, one after the other."""
import os

import numpy as np
import pytest

from test_gpu_cli_mds import GROUPS, LABELS, N_IND, N_SITES, Q, SEED, data, read, run_cli, unequal_windows  # noqa: F401 (data: a fixture)

pytestmark = pytest.mark.gpu

K, R, CI = 2, 5, 0.9
STATS = (".mds_mean", ".mds_sd", ".mds_lo", ".mds_hi")


def check_files(out, plain_mds, res, R=R):
    """the files of an aligned run of R replicates against the Python door's dict (a leading axis of sets) and the .mds of the
    run without --mds_align"""
    n_set = res["eig0"].shape[0]
    theirs = read(plain_mds).decode()[:-2].split("\n\n")
    assert len(theirs) == n_set * (R + 1)
    assert read(out + ".mds").decode() == "".join(b + "\n\n" for b in theirs[::R + 1])
    for k, ext in enumerate(STATS, start=1):
        text = open(out + ext).read()
        assert text.endswith("\n\n")
        blocks = text[:-2].split("\n\n")
        assert len(blocks) == n_set
        for w, b in enumerate(blocks):
            lines = [l.split("\t") for l in b.split("\n")]
            assert len(lines) == N_IND + 1 and lines[0][0] == "eig" and [l[0] for l in lines[1:]] == LABELS
            cells = res["stats"][w, k]
            xy, eig = cells[:K * N_IND].reshape(K, N_IND), cells[K * N_IND:]
            assert lines[0][1:] == ["%.10e" % x for x in eig], (ext, w)
            assert [l[1:] for l in lines[1:]] == [["%.10e" % x for x in xy[:, i]] for i in range(N_IND)], (ext, w)
    lines = open(out + ".mds_fit").read().split("\n")
    assert lines[-1] == "" and len(lines) == n_set + 1
    for w in range(n_set):
        assert lines[w].split("\t") == ["%d" % res["used"][w]] + ["nan" if np.isnan(x) else "%.10e" % x for x in res["fit"][w, 1:]]
    print("%s: %d sets, used %s" % (os.path.basename(out), n_set, res["used"].tolist()))


def test_bootstrap_replicates(tmp_path, data):
    import ngsdist_amd as N
    path, pos, p = data
    base = ["--geno", path, "--probs", "--n_ind", N_IND, "--n_sites", N_SITES, "--n_boot_rep", R, "--boot_block_size", Q, "--seed", SEED,
            "--mds", K]
    plain = run_cli(tmp_path, base, "mds.dist")
    out = run_cli(tmp_path, base + ["--mds_align", "--mds_ci", CI], "align.dist")
    assert read(out) == read(plain)
    t = N.Taus(SEED)
    maps = np.stack([t.block_map(N_SITES // Q) for _ in range(R)])
    with N.Engine(N_IND, N_SITES, indep_geno=False) as e:
        e.upload_ind_major(p).commit()
        res = e.run_job_mds_align(K, maps, Q, evol_model=1, ci=CI)
    assert int(res["used"]) == R
    check_files(out, plain + ".mds", {k: None if v is None else v[None] for k, v in res.items()})


def test_replicates_inside_windows(tmp_path, data):
    import ngsdist_amd as N
    path, pos, p = data
    base = ["--geno", path, "--probs", "--n_ind", N_IND, "--n_sites", N_SITES, "--win_size", 100, "--win_step", 50, "--win_boot_rep", R,
            "--boot_block_size", Q, "--seed", SEED, "--mds", K]
    plain = run_cli(tmp_path, base, "mds.dist")
    out = run_cli(tmp_path, base + ["--mds_align"], "align.dist")  # (--mds_ci: 0.95)
    assert read(out) == read(plain) and read(out + ".windows") == read(plain + ".windows")
    lo, hi = N.window_ranges(N_SITES, 100, 50)
    assert len(lo) == 7
    maps, off = N.window_boot_maps(SEED, lo, hi, R, Q)
    with N.Engine(N_IND, N_SITES, indep_geno=False) as e:
        e.upload_ind_major(p).commit()
        res = e.run_windows_job_var_mds_align(K, lo, hi, maps, off, Q, evol_model=1, n_rep=R)
    assert res["used"].tolist() == [R] * 7
    check_files(out, plain + ".mds", res)


def test_replicates_inside_windows_in_several_engine_calls(tmp_path, data):
    """The host's window w0 + k is set k of its call: one Python call per group on that group's windows (the whole table of
    maps, the group's offsets), concatenated; <out> and <out>.mds are the run's without --mds_align in the same groups.  (Not
    the ungrouped run's bytes: a call cuts its slices by the boundaries of its own windows, DESIGN.md "The budget does not
    change the replicates' bits".)"""
    import ngsdist_amd as N
    path, pos, p = data
    R8 = 8
    shape = ["--geno", path, "--probs", "--n_ind", N_IND, "--n_sites", N_SITES, "--win_size", 100, "--win_step", 50]
    base = shape + ["--win_boot_rep", R8, "--boot_block_size", Q, "--seed", SEED, "--mds", K]
    ungrouped = run_cli(tmp_path, shape, "plain.dist")
    plain = run_cli(tmp_path, base, "mds.dist", group_max=3)
    out = run_cli(tmp_path, base + ["--mds_align"], "align.dist", group_max=3)
    assert read(out) == read(plain) and read(out + ".windows") == read(ungrouped + ".windows")
    lo, hi = N.window_ranges(N_SITES, 100, 50)
    assert len(lo) == 7
    maps, off = N.window_boot_maps(SEED, lo, hi, R8, Q)
    with N.Engine(N_IND, N_SITES, indep_geno=False) as e:
        e.upload_ind_major(p).commit()
        parts = [e.run_windows_job_var_mds_align(K, lo[g], hi[g], maps, off[g], Q, evol_model=1, n_rep=R8) for g in GROUPS]
    res = {k: None if parts[0][k] is None else np.concatenate([q[k] for q in parts]) for k in parts[0]}
    assert res["used"].tolist() == [R8] * 7
    assert read(out) == b"".join(N.format_matrix(d, LABELS) for d in res["dist0"])
    check_files(out, plain + ".mds", res, R8)


def test_unequal_windows_in_several_engine_calls(tmp_path, data):
    """the test above where every group has map offsets of its own (windows in base pairs of several lengths)"""
    import ngsdist_amd as N
    path, pos, p = data
    R8 = 8
    shape, lo, hi, groups = unequal_windows(tmp_path)
    shape = ["--geno", path, "--probs", "--n_ind", N_IND, "--n_sites", N_SITES] + shape
    base = shape + ["--win_boot_rep", R8, "--boot_block_size", Q, "--seed", SEED, "--mds", K]
    ungrouped = run_cli(tmp_path, shape, "plain.dist")
    plain = run_cli(tmp_path, base, "mds.dist", group_max=3)
    out = run_cli(tmp_path, base + ["--mds_align"], "align.dist", group_max=3)
    assert read(out) == read(plain) and read(out + ".windows") == read(ungrouped + ".windows")
    maps, off = N.window_boot_maps(SEED, lo, hi, R8, Q)
    assert all(off[g].tolist() != off[groups[0]].tolist() for g in groups[1:])
    with N.Engine(N_IND, N_SITES, indep_geno=False) as e:
        e.upload_ind_major(p).commit()
        parts = [e.run_windows_job_var_mds_align(K, lo[g], hi[g], maps, off[g], Q, evol_model=1, n_rep=R8) for g in groups]
    res = {k: None if parts[0][k] is None else np.concatenate([q[k] for q in parts]) for k in parts[0]}
    assert res["used"].tolist() == [R8] * len(lo)
    assert read(out) == b"".join(N.format_matrix(d, LABELS) for d in res["dist0"])
    check_files(out, plain + ".mds", res, R8)


def test_refused_flag_combinations(tmp_path, data):
    path, pos, p = data
    base = ["--geno", path, "--probs", "--n_ind", N_IND, "--n_sites", N_SITES]
    boot = ["--n_boot_rep", R, "--boot_block_size", Q]
    for extra, words in ((boot + ["--mds_align"], ("--mds_align", "--mds K")),
                         (["--mds", K, "--mds_align"], ("--mds_align", "--n_boot_rep or --win_boot_rep")),
                         (boot + ["--mds", K, "--mds_ci", 0.9], ("--mds_ci", "--mds_align")),
                         (boot + ["--mds", K, "--mds_align", "--mds_ci", 1], ("--mds_ci", "between 0 and 1")),
                         (boot + ["--mds", K, "--mds_align", "--mds_ci", 0], ("--mds_ci", "between 0 and 1")),
                         (boot + ["--mds", N_IND, "--mds_align"], ("--mds K",)),
                         (boot + ["--mds", K, "--mds_align", "--nj"], ("--mds", "--nj"))):
        err = run_cli(tmp_path, base + extra, "no.dist", ok=False)
        assert "ERROR" in err and all(w in err for w in words), (extra, err)
