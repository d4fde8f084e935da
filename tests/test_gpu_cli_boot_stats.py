"""--boot_stats end to end through the C++ host (ngsdist_amd/bin/ngsDist) on a 12 x 400 text file: <out> is, byte for byte,
what the same command prints without the replicates' flags; every <out>.boot_* file is, byte for byte, the print block
(format_matrix, or the G x G layout of --groups) of the statistic the Python call gives on the same data, seed and block
size; --boot_ci changes <out>.boot_lo and <out>.boot_hi and nothing else.  Under NGSDIST_WIN_GROUP_MAX=3 the host sends the 7
windows to the engine in calls of 3, 3 and 1: the files are, byte for byte, those of the Python calls on the same three groups
of windows, one after the other."""
import gzip
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "ngsdist_amd", "bin", "ngsDist")
N_IND, N_SITES, R, Q, SEED = 12, 400, 8, 10, 5  # (evol_model: the host's default, 1)
NAMES = ["popA", "popB", "single"]
STATS = (".boot_mean", ".boot_sd", ".boot_lo", ".boot_hi")
LABELS = ["Ind_%d" % i for i in range(N_IND)]


def run_cli(tmp_path, args, name, group_max=0):
    out = str(tmp_path / name)
    r = subprocess.run([BIN] + [str(a) for a in args] + ["--out", out, "--verbose", "0"], capture_output=True, timeout=600,
                       env=dict(os.environ, NGSDIST_WIN_GROUP_MAX=str(group_max)))
    assert r.returncode == 0, r.stderr.decode()
    return out


def read(path):
    with open(path, "rb") as fh:
        return fh.read()


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    from oracle import oracle as O
    d = tmp_path_factory.mktemp("boot_stats_cli")
    p = O.synth_indmajor(31, N_IND, N_SITES, miss_frac=0.1)
    sm = np.ascontiguousarray(p.transpose(1, 0, 2))  # [site][ind][3], the file order
    path = str(d / "post.txt.gz")  # (the host reads text through zlib)
    with gzip.open(path, "wt") as fh:
        for k in range(N_SITES):
            fh.write("chrSIM\t%d\t" % (k + 1) + "\t".join("%.17g" % x for x in sm[k].reshape(-1)) + "\n")
    g = np.array([0] * 5 + [1] * 4 + [-1] + [2] + [1])
    groups = str(d / "groups.txt")
    open(groups, "w").write("\n".join("NA" if k < 0 else NAMES[k] for k in g) + "\n")
    return path, groups, g, O.load_text(path, N_IND, N_SITES, in_probs=True)  # (prepared as the host prepares it)


def groups_block(cells, fmt):
    """the G x G block of --groups (format_groups of the host): cells [n_gp] -> bytes"""
    import ngsdist_amd as N
    G = len(NAMES)
    txt = "\n%d\n" % G
    for a in range(G):
        txt += NAMES[a] + "".join("\t" + fmt(cells[N.group_pair_index(G, min(a, b), max(a, b))]) for b in range(G)) + "\n"
    return txt.encode()


def c_float(x):
    return "nan" if np.isnan(x) and not np.signbit(x) else "-nan" if np.isnan(x) else "%.10f" % x


def pairs_used_block(u):
    m = np.zeros((N_IND, N_IND), dtype=np.uint64)
    m[np.triu_indices(N_IND, 1)] = u
    m = m + m.T
    return ("\n%d\n" % N_IND + "".join(LABELS[i] + "".join("\t%d" % x for x in m[i]) + "\n" for i in range(N_IND))).encode()


def expected_files(stats, used, grouped):
    """stats [n_set][5][n_cells], used [n_set][n_cells] -> {suffix: bytes} of the four statistics' files and the counts'"""
    import ngsdist_amd as N
    out = {}
    for k, ext in enumerate(STATS, start=1):
        out[ext] = b"".join(groups_block(s[k], c_float) if grouped else N.format_matrix(s[k], LABELS) for s in stats)
    out[".boot_used"] = b"".join(groups_block(u, lambda x: "%d" % x) if grouped else pairs_used_block(u) for u in used)
    return out


@pytest.mark.parametrize("grouped", [False, True], ids=["pairs", "groups"])
@pytest.mark.parametrize("windows", [False, True], ids=["genome", "windows"])
def test_files_against_the_python_call_and_the_run_without_replicates(tmp_path, data, windows, grouped):
    import ngsdist_amd as N
    path, groups, g, p = data
    base = ["--geno", path, "--probs", "--n_ind", N_IND, "--n_sites", N_SITES]
    shape = ["--win_size", 100, "--win_step", 50] if windows else []
    boot = (["--win_boot_rep", R] if windows else ["--n_boot_rep", R]) + ["--boot_block_size", Q, "--seed", SEED]
    grp = ["--groups", groups] if grouped else []
    plain = run_cli(tmp_path, base + shape + grp, "plain.dist")
    out = run_cli(tmp_path, base + shape + boot + grp + ["--boot_stats"], "stats.dist")
    assert read(out) == read(plain)  # matrix 0 of every set: the run without the replicates' flags
    if windows:
        assert read(out + ".windows") == read(plain + ".windows")
    with N.Engine(N_IND, N_SITES, indep_geno=False) as e:
        e.upload_ind_major(p).commit()
        if grouped:
            e.set_groups(g, len(NAMES))
        if windows:
            lo, hi = N.window_ranges(N_SITES, 100, 50)
            maps, off = N.window_boot_maps(SEED, lo, hi, R, Q)
            call = e.run_windows_job_var_groups_stats if grouped else e.run_windows_job_var_stats
            stats, used = call(lo, hi, maps, off, Q, evol_model=1, n_rep=R)
            assert len(lo) == 7
        else:
            t = N.Taus(SEED)
            maps = np.stack([t.block_map(N_SITES // Q) for _ in range(R)])
            call = e.run_job_groups_stats if grouped else e.run_job_stats
            stats, used = call(maps, Q, evol_model=1)
            stats, used = stats[None], used[None]
    for ext, want in expected_files(stats, used, grouped).items():
        assert read(out + ext) == want, ext
    # another coverage: the interval's two files change, nothing else
    half = run_cli(tmp_path, base + shape + boot + grp + ["--boot_stats", "--boot_ci", 0.5], "half.dist")
    for ext in ("", ".boot_mean", ".boot_sd", ".boot_used"):
        assert read(half + ext) == read(out + ext), ext
    assert read(half + ".boot_lo") != read(out + ".boot_lo") and read(half + ".boot_hi") != read(out + ".boot_hi")


GROUPS = (slice(0, 3), slice(3, 6), slice(6, 7))  # the 7 windows under NGSDIST_WIN_GROUP_MAX=3


@pytest.mark.parametrize("grouped", [False, True], ids=["pairs", "groups"])
def test_windows_in_several_engine_calls(tmp_path, data, grouped):
    """The host's window w0 + k is set k of its call: one Python call per group on that group's windows (the whole table of
    maps, the group's offsets), concatenated; <out> is the estimates' block of those calls.  (Not the ungrouped run's bytes: a
    call cuts its slices by the boundaries of its own windows, DESIGN.md "The budget does not change the replicates' bits".)"""
    import ngsdist_amd as N
    path, groups, g, p = data
    base = ["--geno", path, "--probs", "--n_ind", N_IND, "--n_sites", N_SITES, "--win_size", 100, "--win_step", 50]
    boot = ["--win_boot_rep", R, "--boot_block_size", Q, "--seed", SEED]
    grp = ["--groups", groups] if grouped else []
    plain = run_cli(tmp_path, base + grp, "plain.dist")
    out = run_cli(tmp_path, base + boot + grp + ["--boot_stats"], "stats.dist", group_max=3)
    assert read(out + ".windows") == read(plain + ".windows")
    lo, hi = N.window_ranges(N_SITES, 100, 50)
    assert len(lo) == 7
    maps, off = N.window_boot_maps(SEED, lo, hi, R, Q)
    with N.Engine(N_IND, N_SITES, indep_geno=False) as e:
        e.upload_ind_major(p).commit()
        if grouped:
            e.set_groups(g, len(NAMES))
        call = e.run_windows_job_var_groups_stats if grouped else e.run_windows_job_var_stats
        parts = [call(lo[k], hi[k], maps, off[k], Q, evol_model=1, n_rep=R) for k in GROUPS]
    stats, used = (np.concatenate(x) for x in zip(*parts))
    assert read(out) == b"".join(groups_block(s[0], c_float) if grouped else N.format_matrix(s[0], LABELS) for s in stats)
    for ext, want in expected_files(stats, used, grouped).items():
        assert read(out + ext) == want, ext


@pytest.mark.parametrize("grouped", [False, True], ids=["pairs", "groups"])
def test_unequal_windows_in_several_engine_calls(tmp_path, data, grouped):
    """the test above where every group has map offsets of its own (windows in base pairs of several lengths)"""
    import ngsdist_amd as N
    from test_gpu_cli_mds import unequal_windows
    path, groups, g, p = data
    shape, lo, hi, calls = unequal_windows(tmp_path)
    base = ["--geno", path, "--probs", "--n_ind", N_IND, "--n_sites", N_SITES] + shape + (["--groups", groups] if grouped else [])
    plain = run_cli(tmp_path, base, "plain.dist")
    out = run_cli(tmp_path, base + ["--win_boot_rep", R, "--boot_block_size", Q, "--seed", SEED, "--boot_stats"], "stats.dist", group_max=3)
    assert read(out + ".windows") == read(plain + ".windows")
    maps, off = N.window_boot_maps(SEED, lo, hi, R, Q)
    assert all(off[k].tolist() != off[calls[0]].tolist() for k in calls[1:])
    with N.Engine(N_IND, N_SITES, indep_geno=False) as e:
        e.upload_ind_major(p).commit()
        if grouped:
            e.set_groups(g, len(NAMES))
        call = e.run_windows_job_var_groups_stats if grouped else e.run_windows_job_var_stats
        parts = [call(lo[k], hi[k], maps, off[k], Q, evol_model=1, n_rep=R) for k in calls]
    stats, used = (np.concatenate(x) for x in zip(*parts))
    assert read(out) == b"".join(groups_block(s[0], c_float) if grouped else N.format_matrix(s[0], LABELS) for s in stats)
    for ext, want in expected_files(stats, used, grouped).items():
        assert read(out + ext) == want, ext
