"""tools/kernel_coverage.py: the name handling that decides whether a traced kernel counts as one of the library's, and the
static list of one source (hipcc cross-compiles: no GPU)."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
HAVE_HIPCC = bool(shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc"))


def test_names_are_compared_as_kernel_and_template_arguments():
    import kernel_coverage as K
    f = K.short_name
    assert f("void (anonymous namespace)::k_contract_mfma<6, 2>(double const*, double const*, unsigned int, double*) [clone .kd]") \
        == "k_contract_mfma<6, 2>"
    assert f('"(anonymous namespace)::k_count(unsigned long long const*, ngd_tile const*, unsigned long long*)"') == "k_count"
    assert f("void k_reduce_band_w<1,true>(void const*, unsigned int)") == "k_reduce_band_w<1, true>"
    assert f("void (anonymous namespace)::k_x<std::integral_constant<int, (4)>, false>(int).kd") \
        == "k_x<std::integral_constant<int, (4)>, false>"
    assert f("k_plain") == "k_plain"


def test_a_statistics_file_and_a_plain_list_give_the_same_names(tmp_path):
    import kernel_coverage as K
    csv_file = tmp_path / "1_kernel_stats.csv"
    csv_file.write_text('"Name","Calls","TotalDurationNs"\n'
                        '"void (anonymous namespace)::k_contract_mfma<5, 2>(double const*, unsigned int)",3,100\n'
                        '"(anonymous namespace)::k_spill_scatter(double const*, unsigned int)",1,7\n')
    txt = tmp_path / "names.txt"
    txt.write_text("# a comment\nk_contract_mfma<5, 2>\nk_spill_scatter\n")
    want = {"k_contract_mfma<5, 2>", "k_spill_scatter"}
    assert K.traced_names(str(csv_file)) == want and K.traced_names(str(txt)) == want


@pytest.mark.skipif(not HAVE_HIPCC, reason="no hipcc")
def test_the_static_list_holds_every_tile_shape_of_the_contraction():
    import kernel_coverage as K
    names = set(K.short_name(n) for n in K.demangle(K.kernels_of_file(os.path.join(K.CSRC, "contract_mfma.hip"))))
    assert {"k_contract_mfma<%d, %d>" % (rt, 4 if rt <= 4 else 2) for rt in range(1, 9)} <= names
    assert {"k_spill_weights", "k_spill_sanitize", "k_spill_scatter"} <= names and len(names) == 11
