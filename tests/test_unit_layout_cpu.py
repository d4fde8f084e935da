"""The index arithmetic of the operand images (ngsdist_amd/csrc/ngd_layout.h) from a stand-alone program on the CPU: which
contraction index holds coordinate c of site s -- k = 3 s + c, or the congruent image's order, where the four unit-sum
coordinates of a period of four sites fill a k-group of their own -- its inverse, and the k-groups a range of sites occupies.
What the engine relies on: index and inverse are a bijection on [0, 12 Q) in both layouts; a site range's k-groups hold every
index of the range for all s0 < s1 <= 40 (a range too narrow is unmapped memory during a staged load); the congruent
layout's range bounds the plain one's; the k-groups wholly below a prefix of sites hold no later site."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def layout_bin(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("unit_layout") / "unit_layout")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-o", out,
           os.path.join(ROOT, "tests", "unit_layout", "unit_layout_main.cpp"), "-I" + os.path.join(ROOT, "ngsdist_amd", "csrc")]
    r = subprocess.run(cmd, capture_output=True)
    assert r.returncode == 0, "the layout arithmetic does not build on its own:\n" + r.stderr.decode()[-2000:]
    return out


def test_index_helper_is_a_bijection_and_site_ranges_contain_their_indices(layout_bin):
    r = subprocess.run([layout_bin], capture_output=True, timeout=120)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-3000:]
    assert out.startswith("ok ") and int(out.split()[1]) > 100000, out


def test_python_restatement_of_the_quad_order():
    """twelve indices = four whole sites: t0 of sites 4q..4q+3 first, then (t1, t2) site by site"""
    def k_of(s, c):
        q, u = divmod(s, 4)
        return 12 * q + u if c == 0 else 12 * q + 4 + 2 * u + (c - 1)
    order = sorted(((k_of(s, c), s, c) for s in range(8) for c in range(3)))
    assert [k for k, _, _ in order] == list(range(24))
    assert [(s, c) for _, s, c in order[:12]] == [(0, 0), (1, 0), (2, 0), (3, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 1), (2, 2),
                                                  (3, 1), (3, 2)]
