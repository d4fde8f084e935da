"""--nj end to end through the C++ host (ngsdist_amd/bin/ngsDist) on a 12 x 400 text file: <out>.nwk is, byte for byte,
nj_newick of the records the Python run form gives on the same data, seed and block size, set after set, matrix 0 first;
<out>.support.nwk matrix 0's tree of every set with nj_support's numbers; <out> of a plain run is the run without --nj, and
with replicates its first block is the first block of the run without --nj (every block: the run without the replicates'
flags).  Under NGSDIST_WIN_GROUP_MAX=3 the host sends the 7 windows to the engine in calls of 3, 3 and 1: the files are, byte for
byte, those of the Python calls on the same three groups of windows, one after the other."""
import gzip
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "ngsdist_amd", "bin", "ngsDist")
N_IND, N_SITES, R, Q, SEED = 12, 400, 8, 10, 5  # (evol_model: the host's default, 1)
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
    d = tmp_path_factory.mktemp("nj_cli")
    p = O.synth_indmajor(31, N_IND, N_SITES, miss_frac=0.1)
    sm = np.ascontiguousarray(p.transpose(1, 0, 2))  # [site][ind][3], the file order
    path = str(d / "post.txt.gz")  # (the host reads text through zlib)
    with gzip.open(path, "wt") as fh:
        for k in range(N_SITES):
            fh.write("chrSIM\t%d\t" % (k + 1) + "\t".join("%.17g" % x for x in sm[k].reshape(-1)) + "\n")
    return path, O.load_text(path, N_IND, N_SITES, in_probs=True)  # (prepared as the host prepares it)


def first_block(text):
    return b"\n".join(text.split(b"\n")[:N_IND + 2])


@pytest.mark.parametrize("reps", [False, True], ids=["plain", "replicates"])
@pytest.mark.parametrize("windows", [False, True], ids=["genome", "windows"])
def test_files_against_the_python_call_and_the_run_without_nj(tmp_path, data, windows, reps):
    import ngsdist_amd as N
    path, p = data
    base = ["--geno", path, "--probs", "--n_ind", N_IND, "--n_sites", N_SITES]
    shape = ["--win_size", 100, "--win_step", 50] if windows else []
    boot = ((["--win_boot_rep", R] if windows else ["--n_boot_rep", R]) + ["--boot_block_size", Q, "--seed", SEED]) if reps else []
    plain = run_cli(tmp_path, base + shape, "plain.dist")
    same = run_cli(tmp_path, base + shape + boot, "same.dist")  # the same command without --nj
    out = run_cli(tmp_path, base + shape + boot + ["--nj"], "nj.dist")
    assert read(out) == read(plain)  # matrix 0 of every set: the run without the replicates' flags
    assert first_block(read(out)) == first_block(read(same))
    if not reps:
        assert read(out) == read(same)
    if windows:
        assert read(out + ".windows") == read(plain + ".windows")
    with N.Engine(N_IND, N_SITES, indep_geno=False) as e:
        e.upload_ind_major(p).commit()
        if windows:
            lo, hi = N.window_ranges(N_SITES, 100, 50)
            assert len(lo) == 7
            if reps:
                maps, off = N.window_boot_maps(SEED, lo, hi, R, Q)
                child, length, status, _ = e.run_windows_job_var_nj(lo, hi, maps, off, Q, evol_model=1, n_rep=R)
            else:
                child, length, status, _ = e.run_windows_nj(lo, hi, evol_model=1)
        else:
            maps = None
            if reps:
                t = N.Taus(SEED)
                maps = np.stack([t.block_map(N_SITES // Q) for _ in range(R)])
            child, length, status, _ = e.run_job_nj(maps, Q, evol_model=1)
            child, length, status = child[None], length[None], status[None]
    check_trees(out, child, length, status, reps)


def check_trees(out, child, length, status, reps):
    """<out>.nwk and <out>.support.nwk against the records (n_set, n_mat, ...) of the Python calls"""
    import ngsdist_amd as N
    assert np.all(status == 1)
    want = b"".join(N.nj_newick(c, l, LABELS) for cs, ls in zip(child, length) for c, l in zip(cs, ls))
    assert read(out + ".nwk") == want and want.count(b"\n") == child.shape[0] * ((R if reps else 0) + 1)
    if reps:
        sup = b""
        for cs, ls, st in zip(child, length, status):
            s, used = N.nj_support(cs, st, N_IND)
            assert used == R
            sup += N.nj_newick(cs[0], ls[0], LABELS, s)
        assert read(out + ".support.nwk") == sup
    else:
        assert not os.path.exists(out + ".support.nwk")


GROUPS = (slice(0, 3), slice(3, 6), slice(6, 7))  # the 7 windows under NGSDIST_WIN_GROUP_MAX=3


@pytest.mark.parametrize("reps", [False, True], ids=["plain", "replicates"])
def test_windows_in_several_engine_calls(tmp_path, data, reps):
    """The host's window w0 + k is set k of its call: one Python call per group on that group's windows (the whole table of
    maps, the group's offsets), concatenated.  (Not the ungrouped run's bytes: a call cuts its slices by the boundaries of its
    own windows, DESIGN.md "The budget does not change the replicates' bits".)"""
    import ngsdist_amd as N
    path, p = data
    base = ["--geno", path, "--probs", "--n_ind", N_IND, "--n_sites", N_SITES, "--win_size", 100, "--win_step", 50]
    boot = ["--win_boot_rep", R, "--boot_block_size", Q, "--seed", SEED] if reps else []
    plain = run_cli(tmp_path, base, "plain.dist")
    out = run_cli(tmp_path, base + boot + ["--nj"], "nj.dist", group_max=3)
    assert read(out + ".windows") == read(plain + ".windows")
    lo, hi = N.window_ranges(N_SITES, 100, 50)
    assert len(lo) == 7
    with N.Engine(N_IND, N_SITES, indep_geno=False) as e:
        e.upload_ind_major(p).commit()
        if reps:
            maps, off = N.window_boot_maps(SEED, lo, hi, R, Q)
            parts = [e.run_windows_job_var_nj(lo[g], hi[g], maps, off[g], Q, evol_model=1, n_rep=R) for g in GROUPS]
        else:
            parts = [e.run_windows_nj(lo[g], hi[g], evol_model=1) for g in GROUPS]
    child, length, status, d0 = (np.concatenate(x) for x in zip(*parts))
    assert read(out) == b"".join(N.format_matrix(d, LABELS) for d in d0)
    check_trees(out, child, length, status, reps)


def test_unequal_windows_in_several_engine_calls(tmp_path, data):
    """the test above where every group has map offsets of its own (windows in base pairs of several lengths)"""
    import ngsdist_amd as N
    from test_gpu_cli_mds import unequal_windows
    path, p = data
    shape, lo, hi, groups = unequal_windows(tmp_path)
    base = ["--geno", path, "--probs", "--n_ind", N_IND, "--n_sites", N_SITES] + shape
    plain = run_cli(tmp_path, base, "plain.dist")
    out = run_cli(tmp_path, base + ["--win_boot_rep", R, "--boot_block_size", Q, "--seed", SEED, "--nj"], "nj.dist", group_max=3)
    assert read(out + ".windows") == read(plain + ".windows")
    maps, off = N.window_boot_maps(SEED, lo, hi, R, Q)
    assert all(off[g].tolist() != off[groups[0]].tolist() for g in groups[1:])
    with N.Engine(N_IND, N_SITES, indep_geno=False) as e:
        e.upload_ind_major(p).commit()
        parts = [e.run_windows_job_var_nj(lo[g], hi[g], maps, off[g], Q, evol_model=1, n_rep=R) for g in groups]
    child, length, status, d0 = (np.concatenate(x) for x in zip(*parts))
    assert read(out) == b"".join(N.format_matrix(d, LABELS) for d in d0)
    check_trees(out, child, length, status, True)
