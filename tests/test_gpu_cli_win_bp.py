"""The C++ host with windows in base pairs (--win_bp / --win_bp_step / --win_min_sites), with and without bootstrap replicates
inside them (--win_boot_rep): every printed cell against the CPU oracle on the window's sites with the window's own block
maps, the two coordinate columns of <out>.windows, and -- with called genotypes, where the arithmetic is exact -- the .dist
bytes against the concatenation of the cut-down files' runs."""
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "ngsdist_amd", "bin", "ngsDist")
N_SITES, SIZE_BP, STEP_BP = 777, 2000, 700


def N():
    import ngsdist_amd
    return ngsdist_amd


def data_set(tmp_path):
    """the positions of tests/test_gpu_windows_var.py: two chromosomes, uneven gaps"""
    rng = np.random.default_rng(3)
    gaps = rng.integers(1, 40, N_SITES)
    g2 = gaps[600:].copy()
    g2[100:] *= 12
    pos = np.concatenate([np.cumsum(gaps[:600]), np.cumsum(g2)])
    chrom = ["chrA"] * 600 + ["chrB"] * 177
    pf = str(tmp_path / "p.tsv")
    with open(pf, "w") as fh:
        fh.write("chr\tpos\n" + "".join("%s\t%d\n" % (c, p) for c, p in zip(chrom, pos)))
    lo, hi, start = N().window_ranges_bp(pos, SIZE_BP, STEP_BP, chrom)
    assert len(lo) == 49 and len(set((hi - lo).tolist())) == 28
    return pos, chrom, pf, lo, hi, start


def run_cli(tmp_path, args, name="w.dist", ok=True):
    out = str(tmp_path / name)
    r = subprocess.run([BIN] + [str(a) for a in args] + ["--out", out, "--verbose", "0"], capture_output=True, timeout=600)
    assert (r.returncode == 0) == ok, r.stderr.decode()
    return out, r


def split_blocks(text):
    assert text.startswith("\n")
    return text[1:].split("\n\n")


def cells(block, n_ind):
    lines = [l for l in block.split("\n") if l]
    m = np.array([[float(x) for x in l.split("\t")[1:]] for l in lines[1:]])
    return m[np.triu_indices(n_ind, 1)]


def check_windows_file(path, pos, chrom, lo, hi, start):
    win = open(path).read().strip().split("\n")
    assert win[0] == "window\tchr\tstart\tend\tfirst_site\tn_sites\twin_start\twin_end" and len(win) == len(lo) + 1
    for w, line in enumerate(win[1:]):
        a, b = int(lo[w]), int(hi[w])
        assert line.split("\t") == [str(w), chrom[a], str(pos[a]), str(pos[b - 1]), str(a), str(b - a), str(start[w]),
                                    str(int(start[w]) + SIZE_BP - 1)]


@pytest.mark.parametrize("mode", ["gl", "em", "gl_pdel"])
@pytest.mark.parametrize("R", [0, 3])
def test_cli_windows_in_base_pairs_against_the_oracle(tmp_path, mode, R):
    n_ind, q, seed = 12, 7, 5
    sm = np.ascontiguousarray(O.synth_indmajor(8, n_ind, N_SITES, miss_frac=0.2 if mode == "gl_pdel" else 0.0).transpose(1, 0, 2))
    sm.tofile(str(tmp_path / "g.bin"))  # [site][ind][3], the file order
    p = O.prep_binary(sm, n_ind, N_SITES)  # ... as the reference prepares it at load time
    pos, chrom, pf, lo, hi, start = data_set(tmp_path)
    flags = {"gl": ["--probs", "--indep_geno"], "em": ["--probs"], "gl_pdel": ["--probs", "--indep_geno", "--pairwise_del"]}[mode]
    out, _ = run_cli(tmp_path, ["--geno", tmp_path / "g.bin", "--n_ind", n_ind, "--n_sites", N_SITES, "--posH", pf, "--win_bp", SIZE_BP,
                                "--win_bp_step", STEP_BP, "--evol_model", 1] + flags +
                     (["--win_boot_rep", R, "--boot_block_size", q, "--seed", seed] if R else []))
    got = split_blocks(open(out).read())
    assert len(got) == len(lo) * (R + 1)
    check_windows_file(out + ".windows", pos, chrom, lo, hi, start)
    pdel, indep = mode == "gl_pdel", mode != "em"
    for w, (a, b) in enumerate(zip(lo, hi)):
        nb = int(b - a) // q
        t = O.Taus(seed)  # the cut-down run seeds its generator anew
        srcs = [np.arange(a, b)] + [int(a) + O.boot_site_src(t.block_map(nb), q) for _ in range(R)]
        for m, src in enumerate(srcs):
            d = cells(got[w * (R + 1) + m], n_ind)
            if len(src) == 0:  # shorter than one block: the reference's truncation leaves 0 / 0
                assert np.isnan(d).all(), (w, m)
                continue
            s, c = O.all_pairs(p, pairwise_del=pdel, indep_geno=indep, site_src=src)
            with np.errstate(all="ignore"):
                want = O.finish(s, c, 0, 1)
            assert np.allclose(d, want, rtol=1e-9, atol=2e-10, equal_nan=True), (w, m)  # (ten printed decimals)


def test_cli_called_genotypes_give_the_bytes_of_the_cut_down_files(tmp_path):
    """(a run of the host per window: the first 300 sites, windows every 1400 bp -- five windows of unequal length)"""
    n_ind, n_sites, R, step = 12, 300, 3, 1400
    rng = np.random.default_rng(8)
    raw = rng.dirichlet([0.6, 0.6, 0.6], size=(n_sites, n_ind))
    raw.tofile(str(tmp_path / "g.bin"))
    pos, chrom, _, _, _, _ = data_set(tmp_path)
    pos, chrom = pos[:n_sites], chrom[:n_sites]
    pf = str(tmp_path / "p300.tsv")
    with open(pf, "w") as fh:
        fh.write("".join("%s\t%d\n" % (c, p) for c, p in zip(chrom, pos)))
    lo, hi, start = N().window_ranges_bp(pos, SIZE_BP, step)
    assert len(lo) == 5 and len(set((hi - lo).tolist())) == 5 and (hi - lo).min() < 30  # one window has no block
    base = ["--n_ind", n_ind, "--probs", "--call_geno", "--indep_geno", "--evol_model", 1]
    boot = ["--boot_block_size", 30, "--seed", 5]
    for with_boot in (False, True):
        out, _ = run_cli(tmp_path, ["--geno", tmp_path / "g.bin", "--n_sites", n_sites, "--pos", pf, "--win_bp", SIZE_BP,
                                    "--win_bp_step", step] + (["--win_boot_rep", R] + boot if with_boot else []) + base)
        want = b""
        for a, b in zip(lo, hi):
            raw[a:b].tofile(str(tmp_path / "c.bin"))
            ref, _ = run_cli(tmp_path, ["--geno", tmp_path / "c.bin", "--n_sites", b - a] + (["--n_boot_rep", R] + boot if with_boot else []) + base,
                             name="c.dist")
            want += open(ref, "rb").read()
        assert open(out, "rb").read() == want


def test_cli_refusals_that_need_a_device(tmp_path):
    n_ind = 6
    p = O.synth_indmajor(8, n_ind, N_SITES)
    np.ascontiguousarray(p.transpose(1, 0, 2)).tofile(str(tmp_path / "g.bin"))
    _, _, pf, lo, _, _ = data_set(tmp_path)
    base = ["--geno", tmp_path / "g.bin", "--n_ind", n_ind, "--n_sites", N_SITES, "--probs", "--posH", pf, "--win_bp", SIZE_BP]
    _, r = run_cli(tmp_path, base + ["--max_device_bytes", 1000], ok=False)
    assert "windows (--win_size) need the whole data set on one GPU; it does not fit the device budget!" in r.stderr.decode()
    # --em_exact_win serves plain windows in base pairs
    out, _ = run_cli(tmp_path, base + ["--win_bp_step", STEP_BP, "--em_exact_win"])
    out2, _ = run_cli(tmp_path, base + ["--win_bp_step", STEP_BP], name="w2.dist")
    a, b = split_blocks(open(out).read()), split_blocks(open(out2).read())
    assert len(a) == len(b) == len(lo)
    for x, y in zip(a, b):
        assert np.allclose(cells(x, n_ind), cells(y, n_ind), rtol=1e-6, atol=1e-9)
