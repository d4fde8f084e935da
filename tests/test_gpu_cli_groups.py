"""--groups end to end through the C++ host (ngsdist_amd/bin/ngsDist): the G x G blocks of <out> against means recomputed
from the n x n blocks the same command prints without --groups.  Both files carry 10 decimals, so the mean of the rounded
cells and the rounded mean differ by at most 1e-10 (5e-11 from each rounding): an absolute tolerance of 1.1e-10.  <out>.used
against the number of cells that parse as finite; the number of blocks and <out>.windows are those of the run without
--groups."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "ngsdist_amd", "bin", "ngsDist")
N_IND, N_SITES = 24, 1000
NAMES = ["popA", "popB", "single", "popC"]


def run_cli(tmp_path, args, name, ok=True):
    out = str(tmp_path / name)
    r = subprocess.run([BIN] + [str(a) for a in args] + ["--out", out, "--verbose", "0"], capture_output=True, timeout=600)
    assert (r.returncode == 0) == ok, r.stderr.decode()
    return out if ok else (r.returncode, r.stderr.decode())


def parse_blocks(path, n):
    """the blocks of a printed file -> float array [n_blocks][n][n] ('nan', '-nan', 'inf' parse as what they are)"""
    lines = open(path).read().split("\n")
    assert lines[-1] == "" and (len(lines) - 1) % (n + 2) == 0
    out = []
    for k in range(0, len(lines) - 1, n + 2):
        assert lines[k] == "" and lines[k + 1] == str(n)
        out.append([[float(c) for c in l.split("\t")[1:]] for l in lines[k + 2:k + n + 2]])
    return np.array(out)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    from oracle import oracle as O
    d = tmp_path_factory.mktemp("groups_cli")
    p = O.synth_indmajor(31, N_IND, N_SITES, miss_frac=0.3)  # [n_ind][n_sites][3]
    gl = str(d / "gl.bin")
    np.ascontiguousarray(p.transpose(1, 0, 2)).tofile(gl)
    # popB comes back after popC; one individual in no group, one alone in its group
    g = np.array([0] * 7 + [1] * 6 + [-1] + [2] + [3] * 5 + [1] * 4)
    lines = ["NA" if k < 0 else NAMES[k] + "\tignored" for k in g]
    groups = str(d / "groups.txt")
    open(groups, "w").write("\n".join(lines) + "\n")
    return gl, groups, g


@pytest.mark.parametrize("extra", [[], ["--indep_geno", "--n_boot_rep", 3, "--boot_block_size", 10, "--seed", 4],
                                   ["--indep_geno", "--win_size", 100, "--win_step", 50, "--pairwise_del", "--evol_model", 2]],
                         ids=["plain", "boot", "windows_pdel"])
def test_group_blocks_against_the_matrices_of_the_run_without_groups(tmp_path, data, extra):
    gl, groups, g = data
    base = ["--geno", gl, "--probs", "--n_ind", N_IND, "--n_sites", N_SITES] + extra
    full = run_cli(tmp_path, base, "full.dist")
    grp = run_cli(tmp_path, base + ["--groups", groups], "grp.dist")
    D = parse_blocks(full, N_IND)
    M, U = parse_blocks(grp, 4), parse_blocks(grp + ".used", 4)
    assert len(D) == len(M) == len(U) == {"--n_boot_rep": 4, "--win_size": 19}.get(extra[1] if extra else "", 1)
    for d, m, u in zip(D, M, U):
        for a in range(4):
            for b in range(4):
                ia, ib = np.flatnonzero(g == a), np.flatnonzero(g == b)
                cells = np.array([d[i, j] for i in ia for j in ib if (i < j if a == b else True)])
                fin = np.isfinite(cells)
                assert u[a, b] == fin.sum(), (a, b)
                if fin.sum() == 0:
                    assert np.isnan(m[a, b])
                else:
                    assert abs(m[a, b] - cells[fin].mean()) <= 1.1e-10, (a, b, m[a, b], cells[fin].mean())
        assert np.isnan(m[2, 2]) and u[2, 2] == 0
    if "--win_size" in extra:
        assert open(full + ".windows").read() == open(grp + ".windows").read()
    else:
        assert not os.path.exists(grp + ".windows")


def test_a_bad_groups_file_is_exit_255_with_the_message(tmp_path, data):
    gl, groups, g = data
    short = str(tmp_path / "short.txt")
    open(short, "w").write("popA\n" * (N_IND - 1))
    rc, err = run_cli(tmp_path, ["--geno", gl, "--probs", "--n_ind", N_IND, "--n_sites", N_SITES, "--groups", short], "bad.dist", ok=False)
    assert rc == 255 and "invalid GROUPS file!" in err
