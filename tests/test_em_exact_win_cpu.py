"""NGD_OPT_EM_EXACT_WIN / --em_exact_win (windows along the genome at the reference's EM stopping step): what can be checked
without a GPU -- the option's number in the header and in Python, the ABI version, which a new option must not move, and the
host's argument checks, which end before any engine exists."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "ngsdist_amd", "bin", "ngsDist")
PATH_MSG = ("the reference's EM stopping step (--em_exact_win) belongs to the EM path: not with --indep_geno / --call_geno or "
            "genotype input!")


def run(*args):
    return subprocess.run([BIN] + list(args), capture_output=True, text=True)


BASE = ["--geno", "x", "--probs", "--n_ind", "3", "--n_sites", "64", "--out", "o", "--verbose", "0"]


def test_header_and_python_agree_on_the_option():
    os.environ.setdefault("NGD_NO_TORCH", "1")
    from ngsdist_amd import engine
    with open(os.path.join(ROOT, "include", "ngsdist_amd.h")) as fh:
        h = fh.read()
    assert re.search(r"^#define NGD_OPT_EM_EXACT_WIN 18\b", h, re.M)
    assert engine.OPTIONS["em_exact_win"] == 18
    # every other option keeps its number, and none shares the new one
    assert sorted(engine.OPTIONS.values()).count(18) == 1 and engine.OPTIONS["em_exact"] == 15
    doc = re.search(r"#define NGD_OPT_EM_EXACT_WIN 18(.*?)#define NGD_OPT_DEBUG_FORGE_JOB", h, re.S).group(1)
    for word in ("NGD_OPT_EM_EXACT", "segment-slab", "NGD_OPT_WIN_PLAN", "NGD_E_NOMEM", "NGD_E_INVALID", "replicate"):
        assert word in doc, word
    # ... and the older option's text says who lifts its refusal of the windowed calls
    doc15 = re.search(r"#define NGD_OPT_EM_EXACT 15(.*?)#define NGD_OPT_EM_EXACT_CAP", h, re.S).group(1)
    assert "NGD_OPT_EM_EXACT_WIN" in doc15


def test_abi_version_is_still_6_and_no_symbol_is_added():
    os.environ.setdefault("NGD_NO_TORCH", "1")
    from ngsdist_amd import _lib
    assert _lib.load().ngd_abi_version() == 6
    assert re.search(r"#define NGD_ABI_VERSION 6\b", open(os.path.join(ROOT, "include", "ngsdist_amd.h")).read())
    with open(os.path.join(ROOT, "ngsdist_amd", "csrc", "exports.map")) as fh:
        assert "em_exact_win" not in fh.read()


@pytest.mark.parametrize("flags,msg", [
    ([], "the reference's EM stopping step inside windows (--em_exact_win) needs windows (--win_size)!"),
    (["--win_size", "16", "--indep_geno"], PATH_MSG),
    (["--win_size", "16", "--call_geno"], PATH_MSG),
])
def test_host_refuses_what_the_flag_does_not_serve(flags, msg):
    r = run(*BASE, "--em_exact_win", *flags)
    assert r.returncode == 255  # exit(-1)
    assert "ERROR: [parse_cmd_args] " + msg in r.stderr, r.stderr


def test_genotype_input_is_refused_too():
    r = run("--geno", "x", "--n_ind", "3", "--n_sites", "64", "--out", "o", "--verbose", "0", "--em_exact_win", "--win_size", "16")
    assert r.returncode == 255 and "ERROR: [parse_cmd_args] " + PATH_MSG in r.stderr, r.stderr


@pytest.mark.parametrize("older", ["--em_exact", "--em_exact_boot"])
def test_beside_an_older_flag_that_flags_own_check_dies(older):
    r = run(*BASE, older, "--em_exact_win", "--win_size", "16")
    assert r.returncode == 255
    assert "(%s) cannot be combined with windows (--win_size)!" % older in r.stderr, r.stderr
    assert "--em_exact_win" not in r.stderr


def test_the_flag_passes_the_argument_checks_with_windows(tmp_path):
    """--em_exact_win --win_size gets as far as opening the input, with and without replicates inside the windows; the exact
    match keeps the three flag names apart"""
    for extra in ([], ["--win_boot_rep", "3", "--boot_block_size", "4", "--seed", "7"]):
        r = run("--geno", str(tmp_path / "nope.bin"), "--probs", "--n_ind", "3", "--n_sites", "64", "--out", str(tmp_path / "o"),
                "--verbose", "1", "--em_exact_win", "--win_size", "16", *extra)
        assert r.returncode == 255 and "em_exact_win: true" in r.stderr, r.stderr
        assert "em_exact: true" not in r.stderr and "em_exact_boot: true" not in r.stderr
        assert "--em_exact_win" not in r.stderr and "cannot check GENO file size!" in r.stderr
