"""--mds end to end through the C++ host (ngsdist_amd/bin/ngsDist) on a 12 x 400 text file: <out>.mds parses to the values
the Python run form gives on the same data, seed and block size -- eigenvalues, totals and mds_coords of the vectors, at the
printed precision ("%.10e": 11 significant digits) --, set after set, matrix 0 first; <out> of a plain run is the run without
--mds, and with replicates or windows matrix 0 of every set; the refused flag combinations exit non-zero with a message.
Under NGSDIST_WIN_GROUP_MAX=3 the host sends 7 windows to the engine in calls of 3, 3 and 1: the files are those of the Python
calls on the same three groups of windows, one after the other."""
import gzip
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "ngsdist_amd", "bin", "ngsDist")
N_IND, N_SITES, Q, SEED, K = 12, 400, 10, 5, 3  # (evol_model: the host's default, 1)
GROUPS = (slice(0, 3), slice(3, 6), slice(6, 7))  # 7 windows under NGSDIST_WIN_GROUP_MAX=3
LABELS = ["Ind_%d" % i for i in range(N_IND)]


def run_cli(tmp_path, args, name, ok=True, group_max=0):
    out = str(tmp_path / name)
    r = subprocess.run([BIN] + [str(a) for a in args] + ["--out", out, "--verbose", "0"], capture_output=True, timeout=600,
                       env=dict(os.environ, NGSDIST_WIN_GROUP_MAX=str(group_max)))
    assert (r.returncode == 0) == ok, r.stderr.decode()
    return out if ok else r.stderr.decode()


def read(path):
    with open(path, "rb") as fh:
        return fh.read()


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    from oracle import oracle as O
    d = tmp_path_factory.mktemp("mds_cli")
    p = O.synth_indmajor(31, N_IND, N_SITES, miss_frac=0.1)
    sm = np.ascontiguousarray(p.transpose(1, 0, 2))  # [site][ind][3], the file order
    path = str(d / "post.txt.gz")  # (the host reads text through zlib)
    with gzip.open(path, "wt") as fh:
        for k in range(N_SITES):
            fh.write("chrSIM\t%d\t" % (k + 1) + "\t".join("%.17g" % x for x in sm[k].reshape(-1)) + "\n")
    pos = str(d / "pos.tsv")
    with open(pos, "w") as fh:
        fh.write("".join("chrSIM\t%d\n" % (10 * k + 1) for k in range(N_SITES)))
    return path, pos, O.load_text(path, N_IND, N_SITES, in_probs=True)  # (prepared as the host prepares it)


def check_file(path, eig, vec, tot, status):
    """<out>.mds against (eig [n_set][n_mat][K], vec, tot, status) of the Python door"""
    import ngsdist_amd as N
    text = open(path).read()
    assert text.endswith("\n\n")
    blocks = text[:-2].split("\n\n")
    eig, vec, tot = eig.reshape(-1, K), vec.reshape(-1, K, N_IND), tot.reshape(-1, 2)
    assert len(blocks) == eig.shape[0] and np.all(status == 1)
    xy = N.mds_coords(eig, vec)
    worst = 0.0
    for m, b in enumerate(blocks):
        lines = [l.split("\t") for l in b.split("\n")]
        assert len(lines) == N_IND + 2 and lines[0][0] == "eig" and lines[1][0] == "total" and [l[0] for l in lines[2:]] == LABELS
        # the fields are the door's values as "%.10e" prints them
        assert lines[0][1:] == ["%.10e" % x for x in eig[m]] and lines[1][1:] == ["%.10e" % x for x in tot[m]]
        assert [l[1:] for l in lines[2:]] == [["%.10e" % x for x in row] for row in xy[m]]
        got = np.array([l[1:] for l in lines[2:]], dtype=float)
        worst = max(worst, np.abs(got - xy[m]).max() / np.abs(xy[m]).max())
    print("%s: %d blocks, coordinates parse to the door's within %.3g relative" % (os.path.basename(path), len(blocks), worst))
    assert worst <= 1e-10


def test_plain_run(tmp_path, data):
    import ngsdist_amd as N
    path, pos, p = data
    base = ["--geno", path, "--probs", "--n_ind", N_IND, "--n_sites", N_SITES]
    plain = run_cli(tmp_path, base, "plain.dist")
    out = run_cli(tmp_path, base + ["--mds", K], "mds.dist")
    assert read(out) == read(plain)
    with N.Engine(N_IND, N_SITES, indep_geno=False) as e:
        e.upload_ind_major(p).commit()
        eig, vec, tot, status, _ = e.run_job_mds(K, None, evol_model=1)
    check_file(out + ".mds", eig, vec, tot, status)


def test_bootstrap_replicates(tmp_path, data):
    import ngsdist_amd as N
    path, pos, p = data
    R = 3
    base = ["--geno", path, "--probs", "--n_ind", N_IND, "--n_sites", N_SITES]
    plain = run_cli(tmp_path, base, "plain.dist")
    out = run_cli(tmp_path, base + ["--n_boot_rep", R, "--boot_block_size", Q, "--seed", SEED, "--mds", K], "mds.dist")
    assert read(out) == read(plain)  # matrix 0 alone
    t = N.Taus(SEED)
    maps = np.stack([t.block_map(N_SITES // Q) for _ in range(R)])
    with N.Engine(N_IND, N_SITES, indep_geno=False) as e:
        e.upload_ind_major(p).commit()
        eig, vec, tot, status, _ = e.run_job_mds(K, maps, Q, evol_model=1)
    check_file(out + ".mds", eig, vec, tot, status)


def test_windows_in_sites(tmp_path, data):
    import ngsdist_amd as N
    path, pos, p = data
    base = ["--geno", path, "--probs", "--n_ind", N_IND, "--n_sites", N_SITES, "--win_size", 100, "--win_step", 50]
    plain = run_cli(tmp_path, base, "plain.dist")
    out = run_cli(tmp_path, base + ["--mds", K], "mds.dist")
    assert read(out) == read(plain) and read(out + ".windows") == read(plain + ".windows")
    lo, hi = N.window_ranges(N_SITES, 100, 50)
    assert len(lo) == 7
    with N.Engine(N_IND, N_SITES, indep_geno=False) as e:
        e.upload_ind_major(p).commit()
        eig, vec, tot, status, _ = e.run_windows_mds(K, lo, hi, evol_model=1)
    check_file(out + ".mds", eig, vec, tot, status)


def test_windows_in_base_pairs_with_replicates(tmp_path, data):
    import ngsdist_amd as N
    path, pos, p = data
    R = 2
    base = ["--geno", path, "--probs", "--n_ind", N_IND, "--n_sites", N_SITES, "--pos", pos, "--win_bp", 1000, "--win_bp_step", 700]
    plain = run_cli(tmp_path, base, "plain.dist")
    out = run_cli(tmp_path, base + ["--win_boot_rep", R, "--boot_block_size", Q, "--seed", SEED, "--mds", K], "mds.dist")
    assert read(out) == read(plain) and read(out + ".windows") == read(plain + ".windows")
    lo, hi, _ = N.window_ranges_bp(10 * np.arange(N_SITES) + 1, 1000, 700)
    assert len(lo) >= 5 and (hi - lo).min() >= Q
    maps, off = N.window_boot_maps(SEED, lo, hi, R, Q)
    with N.Engine(N_IND, N_SITES, indep_geno=False) as e:
        e.upload_ind_major(p).commit()
        eig, vec, tot, status, _ = e.run_windows_job_var_mds(K, lo, hi, maps, off, Q, evol_model=1, n_rep=R)
    check_file(out + ".mds", eig, vec, tot, status)


@pytest.mark.parametrize("R", [0, 8], ids=["plain", "replicates"])
def test_windows_in_several_engine_calls(tmp_path, data, R):
    """The host's window w0 + k is set k of its call: one Python call per group on that group's windows (the whole table of
    maps, the group's offsets), concatenated.  (Not the ungrouped run's bytes: a call cuts its slices by the boundaries of its
    own windows, DESIGN.md "The budget does not change the replicates' bits".)"""
    import ngsdist_amd as N
    path, pos, p = data
    base = ["--geno", path, "--probs", "--n_ind", N_IND, "--n_sites", N_SITES, "--win_size", 100, "--win_step", 50]
    boot = ["--win_boot_rep", R, "--boot_block_size", Q, "--seed", SEED] if R else []
    plain = run_cli(tmp_path, base, "plain.dist")
    out = run_cli(tmp_path, base + boot + ["--mds", K], "mds.dist", group_max=3)
    assert read(out + ".windows") == read(plain + ".windows")
    lo, hi = N.window_ranges(N_SITES, 100, 50)
    assert len(lo) == 7
    with N.Engine(N_IND, N_SITES, indep_geno=False) as e:
        e.upload_ind_major(p).commit()
        if R:
            maps, off = N.window_boot_maps(SEED, lo, hi, R, Q)
            parts = [e.run_windows_job_var_mds(K, lo[g], hi[g], maps, off[g], Q, evol_model=1, n_rep=R) for g in GROUPS]
        else:
            parts = [e.run_windows_mds(K, lo[g], hi[g], evol_model=1) for g in GROUPS]
    eig, vec, tot, status, d0 = (np.concatenate(x) for x in zip(*parts))
    assert read(out) == b"".join(N.format_matrix(d, LABELS) for d in d0)
    check_file(out + ".mds", eig, vec, tot, status)


def unequal_windows(d):
    """windows in base pairs of several lengths over the 400 sites, none shorter than a block, after writing their positions
    file into d: -> (the host's arguments, lo, hi, the groups of windows under NGSDIST_WIN_GROUP_MAX=3).  Windows of one length
    share their maps, so only here does a group's offset into the table of maps differ from the first group's."""
    import ngsdist_amd as N
    coords = np.cumsum(np.where(np.arange(N_SITES) < 150, 5, 20))
    path = str(d / "uneven.tsv")
    with open(path, "w") as fh:
        fh.write("".join("chrSIM\t%d\n" % x for x in coords))
    lo, hi, _ = N.window_ranges_bp(coords, 1000, 700, min_sites=Q)
    assert len(lo) >= 7 and len(set((hi - lo).tolist())) >= 3 and (hi - lo).min() >= Q
    groups = [slice(k, min(k + 3, len(lo))) for k in range(0, len(lo), 3)]
    return ["--pos", path, "--win_bp", 1000, "--win_bp_step", 700, "--win_min_sites", Q], lo, hi, groups


def test_unequal_windows_in_several_engine_calls(tmp_path, data):
    """test_windows_in_several_engine_calls where every group has map offsets of its own"""
    import ngsdist_amd as N
    path, pos, p = data
    R = 8
    shape, lo, hi, groups = unequal_windows(tmp_path)
    base = ["--geno", path, "--probs", "--n_ind", N_IND, "--n_sites", N_SITES] + shape
    plain = run_cli(tmp_path, base, "plain.dist")
    out = run_cli(tmp_path, base + ["--win_boot_rep", R, "--boot_block_size", Q, "--seed", SEED, "--mds", K], "mds.dist", group_max=3)
    assert read(out + ".windows") == read(plain + ".windows")
    maps, off = N.window_boot_maps(SEED, lo, hi, R, Q)
    assert all(off[g].tolist() != off[groups[0]].tolist() for g in groups[1:])
    with N.Engine(N_IND, N_SITES, indep_geno=False) as e:
        e.upload_ind_major(p).commit()
        parts = [e.run_windows_job_var_mds(K, lo[g], hi[g], maps, off[g], Q, evol_model=1, n_rep=R) for g in groups]
    eig, vec, tot, status, d0 = (np.concatenate(x) for x in zip(*parts))
    assert read(out) == b"".join(N.format_matrix(d, LABELS) for d in d0)
    check_file(out + ".mds", eig, vec, tot, status)


def test_refused_flag_combinations(tmp_path, data):
    path, pos, p = data
    base = ["--geno", path, "--probs", "--n_ind", N_IND, "--n_sites", N_SITES]
    groups = str(tmp_path / "groups.txt")
    open(groups, "w").write("\n".join(["a", "b", "a"] * 4))
    for extra, words in ((["--mds", K, "--groups", groups], ("--mds", "--groups")),
                         (["--mds", K, "--n_boot_rep", 3, "--boot_stats"], ("--mds", "--boot_stats")),
                         (["--mds", K, "--nj"], ("--mds", "--nj")),
                         (["--mds", K, "--n_gpus", 2], ("--mds", "--n_gpus 1")),
                         (["--mds", 0], ("--mds K",)),
                         (["--mds", N_IND], ("--mds K",)),
                         (["--mds", 17], ("--mds K",))):
        err = run_cli(tmp_path, base + extra, "no.dist", ok=False)
        assert "ERROR" in err and all(w in err for w in words), (extra, err)
