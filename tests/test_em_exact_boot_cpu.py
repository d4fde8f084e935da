"""NGD_OPT_EM_EXACT = 2 / --em_exact_boot (bootstrap replicates at the reference's EM stopping step): what can be checked
without a GPU -- the host's refusals (they end before any engine exists), the header's text and the ABI version, which the
new value must not move."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "ngsdist_amd", "bin", "ngsDist")


def run(*args):
    return subprocess.run([BIN] + list(args), capture_output=True, text=True)


BASE = ["--geno", "x", "--probs", "--n_ind", "3", "--n_sites", "64", "--out", "o", "--verbose", "0"]


@pytest.mark.parametrize("flags,msg", [
    (["--indep_geno"], "the reference's EM stopping step (--em_exact_boot) belongs to the EM path: not with --indep_geno / "
                       "--call_geno or genotype input!"),
    (["--call_geno"], "the reference's EM stopping step (--em_exact_boot) belongs to the EM path: not with --indep_geno / "
                      "--call_geno or genotype input!"),
    (["--win_size", "16"], "the reference's EM stopping step (--em_exact_boot) cannot be combined with windows (--win_size)!"),
])
def test_host_refuses_what_the_flag_does_not_serve(flags, msg):
    r = run(*BASE, "--em_exact_boot", *flags)
    assert r.returncode == 255  # exit(-1)
    assert "ERROR: [parse_cmd_args] " + msg in r.stderr, r.stderr


def test_genotype_input_is_refused_too():
    r = run("--geno", "x", "--n_ind", "3", "--n_sites", "64", "--out", "o", "--verbose", "0", "--em_exact_boot")
    assert r.returncode == 255 and "(--em_exact_boot) belongs to the EM path" in r.stderr


def test_replicates_pass_the_argument_checks_and_em_exact_stays_as_it_was(tmp_path):
    """--em_exact_boot --n_boot_rep gets as far as opening the input; --em_exact --n_boot_rep is refused as ever, and the
    exact match keeps --em_exact unambiguous beside the longer name"""
    r = run("--geno", str(tmp_path / "nope.bin"), "--probs", "--n_ind", "3", "--n_sites", "64", "--out", str(tmp_path / "o"),
            "--verbose", "1", "--em_exact_boot", "--n_boot_rep", "2")
    assert r.returncode == 255 and "em_exact_boot: true" in r.stderr and "--em_exact_boot" not in r.stderr, r.stderr
    assert "cannot check GENO file size!" in r.stderr
    r = run(*BASE, "--em_exact", "--n_boot_rep", "2")
    assert r.returncode == 255
    assert "(--em_exact) cannot be combined with bootstrap replicates (--n_boot_rep)!" in r.stderr


def test_header_documents_value_2():
    with open(os.path.join(ROOT, "include", "ngsdist_amd.h")) as fh:
        h = fh.read()
    m = re.search(r"#define NGD_OPT_EM_EXACT 15(.*?)#define NGD_OPT_EM_EXACT_CAP", h, re.S)
    assert m
    doc = m.group(1)
    assert re.search(r"\b2: ", doc) and "multiplicit" in doc and "job" in doc and "NGD_E_INVALID" in doc


def test_abi_version_is_still_6():
    os.environ.setdefault("NGD_NO_TORCH", "1")
    import ngsdist_amd
    from ngsdist_amd import _lib
    assert _lib.load().ngd_abi_version() == 6
    assert re.search(r"#define NGD_ABI_VERSION 6\b", open(os.path.join(ROOT, "include", "ngsdist_amd.h")).read())
