"""--win_cmp end to end through the C++ host (ngsdist_amd/bin/ngsDist) on a 12 x 400 text file cut into 6 windows: <out> and
<out>.windows are the run's without the flag byte for byte; <out>.win_cor, <out>.win_rms and <out>.win_cmp parse, and their
fields are win_cmp_finish on the Python door's run_windows_cmp as "%.10e" prints them; <out>.win_mds is mds_host on the RMS table
to the printed digits; with --pairwise_del a window made all-missing shows "nan" lines and the WARNING; the refused flag
combinations exit with status 255 and a message."""
import gzip
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "ngsdist_amd", "bin", "ngsDist")
N_IND, N_SITES, SIZE, STEP, K = 12, 400, 100, 60, 2  # (evol_model: the host's default, 1)
N_PAIRS = N_IND * (N_IND - 1) // 2
GONE = 2  # the window whose sites [120, 220) carry no data


def run_cli(tmp_path, args, name, ok=True):
    out = str(tmp_path / name)
    r = subprocess.run([BIN] + [str(a) for a in args] + ["--out", out, "--verbose", "0"], capture_output=True, timeout=600)
    assert (r.returncode == 0) == ok, r.stderr.decode()
    if not ok:
        assert r.returncode == 255
        return r.stderr.decode()
    return out, r.stderr.decode()


def read(path):
    with open(path, "rb") as fh:
        return fh.read()


def write_text(path, p):
    sm = np.ascontiguousarray(p.transpose(1, 0, 2))  # [site][ind][3], the file order
    with gzip.open(path, "wt") as fh:  # (the host reads text through zlib)
        for k in range(N_SITES):
            fh.write("chrSIM\t%d\t" % (k + 1) + "\t".join("%.17g" % x for x in sm[k].reshape(-1)) + "\n")


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    from oracle import oracle as O
    d = tmp_path_factory.mktemp("win_cmp_cli")
    p = O.synth_indmajor(37, N_IND, N_SITES, miss_frac=0.05)
    full = str(d / "post.txt.gz")
    write_text(full, p)
    q = p.copy()
    q[:, GONE * STEP:GONE * STEP + SIZE, :] = 1.0 / 3.0  # no data at these sites: every pair of window GONE is without a site
    holed = str(d / "holed.txt.gz")
    write_text(holed, q)
    # (prepared as the host prepares it)
    return full, O.load_text(full, N_IND, N_SITES, in_probs=True), holed, O.load_text(holed, N_IND, N_SITES, in_probs=True)


def fields(path, n_rows, header=None):
    lines = open(path).read().split("\n")
    assert lines[-1] == ""
    lines = lines[:-1]
    if header:
        assert lines[0] == header
        lines = lines[1:]
    assert len(lines) == n_rows
    return [l.split("\t") for l in lines]


def e10(x):
    return "%.10e" % x


def check_files(out, door, pairwise_del_bad=()):
    import ngsdist_amd as N
    mean, gram, status, _ = door
    W = len(mean)
    cor, rms = N.win_cmp_finish(mean, gram, status, N_PAIRS)
    assert fields(out + ".win_cor", W) == [[e10(x) for x in row] for row in cor]
    assert fields(out + ".win_rms", W) == [[e10(x) for x in row] for row in rms]
    with np.errstate(invalid="ignore"):
        sd = np.sqrt(np.diag(gram) / N_PAIRS)
    assert fields(out + ".win_cmp", W, "window\tmean\tsd\tstatus") == [[str(w), e10(mean[w]), e10(sd[w]), str(int(status[w]))] for w in range(W)]
    assert [w for w in range(W) if status[w] == 0] == list(pairwise_del_bad)
    for w in pairwise_del_bad:
        assert fields(out + ".win_cor", W)[w] == ["nan"] * W and fields(out + ".win_rms", W)[w] == ["nan"] * W
    # the tables parse back to the door's numbers at the printed precision
    got = np.array(fields(out + ".win_rms", W), dtype=float)
    keep = status == 1
    assert np.allclose(got[np.ix_(keep, keep)], rms[np.ix_(keep, keep)], rtol=1e-10, atol=0)
    return rms, status


def check_mds(path, rms, status):
    import ngsdist_amd as N
    W = len(status)
    kept = np.flatnonzero(status == 1)
    n = len(kept)
    val = np.array([rms[kept[a], kept[b]] for a in range(n) for b in range(a + 1, n)])
    eig, vec, tot, st = N.mds_host(val, n, K)
    xy = N.mds_coords(eig, vec)
    text = open(path).read()
    assert text.endswith("\n\n") and st == 1
    rows = [l.split("\t") for l in text[:-2].split("\n")]
    assert len(rows) == W + 2
    assert rows[0] == ["eig"] + [e10(x) for x in eig] and rows[1] == ["total"] + [e10(x) for x in tot]
    at = 0
    for w in range(W):
        if status[w]:
            assert rows[2 + w] == [str(w)] + [e10(x) for x in xy[at]]
            at += 1
        else:
            assert rows[2 + w] == [str(w)] + ["nan"] * K


def test_windows_compared(tmp_path, data):
    import ngsdist_amd as N
    full, p, _, _ = data
    base = ["--geno", full, "--probs", "--n_ind", N_IND, "--n_sites", N_SITES, "--win_size", SIZE, "--win_step", STEP]
    plain, _ = run_cli(tmp_path, base, "plain.dist")
    out, err = run_cli(tmp_path, base + ["--win_cmp", "--win_cmp_mds", K], "cmp.dist")
    assert read(out) == read(plain) and read(out + ".windows") == read(plain + ".windows")
    assert "WARNING" not in err
    lo, hi = N.window_ranges(N_SITES, SIZE, STEP)
    assert len(lo) == 6
    with N.Engine(N_IND, N_SITES, indep_geno=False) as e:
        e.upload_ind_major(p).commit()
        door = e.run_windows_cmp(lo, hi, evol_model=1)
    rms, status = check_files(out, door)
    check_mds(out + ".win_mds", rms, status)
    # without --win_cmp_mds there is no <out>.win_mds
    out2, _ = run_cli(tmp_path, base + ["--win_cmp"], "cmp2.dist")
    assert not os.path.exists(out2 + ".win_mds") and read(out2 + ".win_cor") == read(out + ".win_cor")


def test_a_window_without_data_under_pairwise_deletion(tmp_path, data):
    import ngsdist_amd as N
    _, _, holed, q = data
    base = ["--geno", holed, "--probs", "--n_ind", N_IND, "--n_sites", N_SITES, "--win_size", SIZE, "--win_step", STEP, "--pairwise_del"]
    plain, _ = run_cli(tmp_path, base, "plain.dist")
    out, err = run_cli(tmp_path, base + ["--win_cmp", "--win_cmp_mds", K], "cmp.dist")
    assert read(out) == read(plain) and read(out + ".windows") == read(plain + ".windows")
    assert "WARNING: 1 of the run's windows" in err
    lo, hi = N.window_ranges(N_SITES, SIZE, STEP)
    with N.Engine(N_IND, N_SITES, indep_geno=False, pairwise_del=True) as e:
        e.upload_ind_major(q).commit()
        door = e.run_windows_cmp(lo, hi, evol_model=1)
    rms, status = check_files(out, door, pairwise_del_bad=(GONE,))
    check_mds(out + ".win_mds", rms, status)


def test_refused_flag_combinations(tmp_path, data):
    full = data[0]
    base = ["--geno", full, "--probs", "--n_ind", N_IND, "--n_sites", N_SITES]
    win = ["--win_size", SIZE, "--win_step", STEP]
    groups = str(tmp_path / "groups.txt")
    open(groups, "w").write("\n".join(["a", "b", "a"] * 4))
    for extra, words in ((["--win_cmp"], ("--win_cmp", "requires windows")),
                         (win + ["--win_cmp", "--win_boot_rep", 2, "--boot_block_size", 10], ("--win_cmp", "--win_boot_rep")),
                         (win + ["--win_cmp", "--groups", groups], ("--win_cmp", "--groups")),
                         (win + ["--win_cmp", "--boot_stats"], ("--boot_stats",)),
                         (win + ["--win_cmp", "--nj"], ("--win_cmp", "--nj")),
                         (win + ["--win_cmp", "--mds", 2], ("--win_cmp", "--mds")),
                         (win + ["--win_cmp", "--n_gpus", 2], ("--n_gpus 1",)),
                         (win + ["--win_cmp_mds", 2], ("--win_cmp_mds", "--win_cmp")),
                         (win + ["--win_cmp", "--win_cmp_mds", 0], ("--win_cmp_mds K",)),
                         (win + ["--win_cmp", "--win_cmp_mds", 6], ("--win_cmp_mds K",)),
                         (win + ["--win_cmp", "--win_cmp_mds", 17], ("--win_cmp_mds K",))):
        err = run_cli(tmp_path, base + extra, "no.dist", ok=False)
        assert "ERROR" in err and all(w in err for w in words), (extra, err)
