"""Loads libngsdist_amd.so (the HIP engine behind include/ngsdist_amd.h).

There is no fallback: if the library is missing or will not load, importing
fails loudly.  Build it with `python -c "import __graft_entry__ as g; g.build()"`
or `make -C ngsdist_amd/csrc`.
"""
import ctypes as C
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
# NGSDIST_AMD_LIB: an A/B build of the same engine (tools/build_variant.sh) for the measuring tools; never a fallback
LIB_PATH = os.environ.get("NGSDIST_AMD_LIB") or os.path.join(_HERE, "libngsdist_amd.so")


class NgdConfig(C.Structure):
    _fields_ = [
        ("n_ind", C.c_uint64),
        ("n_sites", C.c_uint64),
        ("score", C.c_double * 9),
        ("pairwise_del", C.c_int32),
        ("indep_geno", C.c_int32),
        ("device", C.c_int32),
        ("kernel", C.c_int32),
        ("shard_rank", C.c_uint32),
        ("shard_world", C.c_uint32),
        ("variant", C.c_uint32),
        ("n_slices", C.c_uint32),
        ("wg_target", C.c_uint32),
        ("exact_shapes", C.c_uint32),
        ("single_image", C.c_uint32),
        ("second_image_mib", C.c_uint32),
    ]


class NgdPrep(C.Structure):
    _fields_ = [("in_logscale", C.c_int32), ("call_geno", C.c_int32), ("N_thresh", C.c_double),
                ("call_thresh", C.c_double)]


class NgdTiming(C.Structure):
    _fields_ = [
        ("ms_total", C.c_double),
        ("ms_accum", C.c_double),
        ("ms_reduce", C.c_double),
        ("ms_count", C.c_double),
        ("pair_sites", C.c_uint64),
        ("launches", C.c_uint64),
    ]


class NgdSpillTiming(C.Structure):
    _fields_ = [("ms_weights", C.c_double), ("ms_terms", C.c_double), ("ms_sanitize", C.c_double), ("ms_contract", C.c_double)] + [
        (k, C.c_uint64) for k in ("chunks", "sites", "unit_sites", "units", "slot_groups", "slot_groups_live", "matrices",
                                  "matrix_groups", "contract_launches")]


class NgdWindowsInfo(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("segments", "slab_bytes", "batches", "band_launches", "windows_by_pass",
                                          "fixup_pairs")] + [("ms", C.c_double)]


class NgdFixupInfo(C.Structure):
    _fields_ = [("flagged", C.c_uint64), ("recomputed", C.c_uint64), ("skipped", C.c_uint64), ("ms", C.c_double),
                ("by_pass", C.c_uint64)]


class NgdEmExactInfo(C.Structure):
    _fields_ = [("noted", C.c_uint64), ("changed", C.c_uint64), ("passes", C.c_uint64), ("ms", C.c_double)]


class NgdEmExactEntry(C.Structure):
    _fields_ = [("i1", C.c_uint32), ("i2", C.c_uint32), ("site", C.c_uint64), ("t_dev", C.c_uint32), ("t_ref", C.c_uint32),
                ("c_dev", C.c_double), ("c_ref", C.c_double)]


# every symbol include/ngsdist_amd.h declares (tests/test_abi.py checks the header against this)
EXPORTS = [
    "ngd_last_error", "ngd_abi_version", "ngd_device_count", "ngd_create", "ngd_destroy",
    "ngd_upload_sites", "ngd_upload_ind_major", "ngd_commit", "ngd_stage_acquire", "ngd_stage_submit",
    "ngd_upload_raw_sites", "ngd_synth_fill", "ngd_synth_fill_range", "ngd_run", "ngd_run_mult", "ngd_run_mult_device",
    "ngd_run_device", "ngd_run_batch", "ngd_run_batch_device", "ngd_run_mult_batch",
    "ngd_run_mult_batch_device", "ngd_run_job", "ngd_run_job_device", "ngd_run_job_dist", "ngd_run_batch_dist", "ngd_run_mult_batch_dist", "ngd_fetch_matrix", "ngd_drop_caches", "ngd_set_option", "ngd_last_timing", "ngd_last_plain_pass", "ngd_last_spill_timing", "ngd_last_fixup", "ngd_image_mode", "ngd_last_shader_clock", "ngd_last_em_work", "ngd_finish", "ngd_finish_stream", "ngd_format_matrix", "ngd_taus_seed", "ngd_taus_get",
    "ngd_taus_uniform", "ngd_boot_block_map", "ngd_n_pairs", "ngd_pair_index", "ngd_device_bytes", "ngd_device_memory", "ngd_shard_of_pair", "ngd_shard_map",
    "ngd_score_congruence", "ngd_run_windows", "ngd_run_windows_device", "ngd_run_windows_dist", "ngd_last_windows",
    "ngd_window_ranges", "ngd_run_windows_job", "ngd_run_windows_job_device", "ngd_run_windows_job_dist",
    "ngd_window_ranges_bp", "ngd_window_boot_maps", "ngd_run_windows_job_var", "ngd_run_windows_job_var_device",
    "ngd_run_windows_job_var_dist",
    "ngd_last_em_exact", "ngd_em_exact_entries", "ngd_em2_site",
    "ngd_n_group_pairs", "ngd_group_pair_index", "ngd_group_cells", "ngd_set_groups", "ngd_group_means_device",
    "ngd_run_job_groups", "ngd_run_windows_groups", "ngd_run_windows_job_var_groups", "ngd_last_groups_ms",
    "ngd_boot_stats_max_rep", "ngd_boot_stats_host", "ngd_boot_stats_device", "ngd_boot_stats_values_device",
    "ngd_run_job_stats", "ngd_run_windows_job_var_stats", "ngd_run_job_groups_stats", "ngd_run_windows_job_var_groups_stats",
    "ngd_last_boot_stats_ms",
    "ngd_nj_max_ind", "ngd_nj_host", "ngd_nj_values_device", "ngd_nj_device", "ngd_run_job_nj", "ngd_run_windows_nj",
    "ngd_run_windows_job_var_nj", "ngd_last_nj_ms", "ngd_nj_support", "ngd_nj_newick",
    "ngd_mds_max_ind", "ngd_mds_max_dim", "ngd_mds_host", "ngd_mds_coords", "ngd_mds_values_device", "ngd_mds_device",
    "ngd_run_job_mds", "ngd_run_windows_mds", "ngd_run_windows_job_var_mds", "ngd_last_mds_ms",
    "ngd_mds_align_host", "ngd_mds_align_values_device", "ngd_run_job_mds_align", "ngd_run_windows_job_var_mds_align",
    "ngd_last_mds_align_ms",
    "ngd_win_cmp_max_vec", "ngd_win_cmp_slice", "ngd_win_cmp_host", "ngd_win_cmp_finish", "ngd_win_cmp_values_device",
    "ngd_win_cmp_device", "ngd_run_windows_cmp", "ngd_last_win_cmp_ms",
]

NSTAT = 5  # NGD_BOOT_NSTAT: est, mean, sd, lo, hi

_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "ngsdist_amd: %s is missing -- the HIP engine was not built (run __graft_entry__.build() "
            "or `make -C ngsdist_amd/csrc`).  There is no CPU fallback." % LIB_PATH)
    # One HIP runtime per process: if PyTorch is present, let ITS libamdhip64.so.7 be
    # the one already mapped when our DT_NEEDED entry of the same soname is resolved,
    # so device pointers / streams can be shared with torch (RCCL gather in bench.py).
    if "torch" not in sys.modules and not os.environ.get("NGD_NO_TORCH"):
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    try:
        L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    except OSError as exc:
        raise ImportError("ngsdist_amd: cannot load %s: %s (no CPU fallback)" % (LIB_PATH, exc))
    vp, dp, u64, u64p = C.c_void_p, C.POINTER(C.c_double), C.c_uint64, C.POINTER(C.c_uint64)
    u32p = C.POINTER(C.c_uint32)
    L.ngd_last_error.restype = C.c_char_p
    L.ngd_abi_version.restype = C.c_int
    L.ngd_device_count.restype = C.c_int
    L.ngd_create.argtypes = [C.POINTER(NgdConfig), C.POINTER(vp)]
    L.ngd_destroy.argtypes = [vp]
    L.ngd_destroy.restype = None
    L.ngd_upload_sites.argtypes = [vp, dp, u64, u64]
    L.ngd_upload_ind_major.argtypes = [vp, dp]
    L.ngd_commit.argtypes = [vp]
    L.ngd_stage_acquire.argtypes = [vp, C.POINTER(dp), u64p]
    L.ngd_stage_submit.argtypes = [vp, u64, u64, C.POINTER(NgdPrep)]
    L.ngd_upload_raw_sites.argtypes = [vp, dp, u64, u64, C.POINTER(NgdPrep)]
    L.ngd_synth_fill.argtypes = [vp, u64, C.c_double]
    L.ngd_synth_fill_range.argtypes = [vp, u64, C.c_double, u64]
    L.ngd_run_mult.argtypes = [vp, u32p, u64, u64, dp, u64p]
    L.ngd_run_mult_device.argtypes = [vp, u32p, u64, u64, vp, vp]
    L.ngd_run.argtypes = [vp, u64p, u64, u64, dp, u64p]
    L.ngd_run_device.argtypes = [vp, u64p, u64, u64, vp, vp]
    L.ngd_run_batch.argtypes = [vp, u64p, C.c_uint32, u64, u64, dp, u64p]
    L.ngd_run_batch_device.argtypes = [vp, u64p, C.c_uint32, u64, u64, vp, vp]
    L.ngd_run_mult_batch.argtypes = [vp, u32p, C.c_uint32, u64, u64, dp, u64p]
    L.ngd_run_job.argtypes = [vp, u64p, C.c_uint32, u64, u64, dp, u64p]
    L.ngd_run_job_device.argtypes = [vp, u64p, C.c_uint32, u64, u64, vp, vp]
    L.ngd_fetch_matrix.argtypes = [vp, C.c_uint32, dp, u64p]
    L.ngd_run_job_dist.argtypes = [vp, u64p, C.c_uint32, u64, u64, u64, u64, dp]
    L.ngd_run_batch_dist.argtypes = [vp, u64p, C.c_uint32, u64, u64, u64, u64, dp]
    L.ngd_run_mult_batch_dist.argtypes = [vp, u32p, C.c_uint32, u64, u64, u64, u64, dp]
    L.ngd_run_mult_batch_device.argtypes = [vp, u32p, C.c_uint32, u64, u64, vp, vp]
    L.ngd_drop_caches.argtypes = [vp]
    L.ngd_set_option.argtypes = [vp, C.c_int, u64]
    L.ngd_last_timing.argtypes = [vp, C.POINTER(NgdTiming)]
    if hasattr(L, "ngd_last_plain_pass"):  # (an A/B build of an engine from before the symbol: NGSDIST_AMD_LIB)
        L.ngd_last_plain_pass.argtypes = [vp, u64p]
    L.ngd_last_spill_timing.argtypes = [vp, C.POINTER(NgdSpillTiming)]
    L.ngd_last_fixup.argtypes = [vp, C.POINTER(NgdFixupInfo)]
    L.ngd_image_mode.argtypes = [vp, C.POINTER(C.c_int)]
    L.ngd_image_mode.restype = C.c_int
    L.ngd_last_em_work.argtypes = [vp, u64p, u64p]
    L.ngd_last_shader_clock.argtypes = [vp, dp]
    L.ngd_finish.argtypes = [dp, u64p, u64, u64, u64, dp]
    L.ngd_finish_stream.argtypes = [dp, u64p, u64, u64, u64, dp, u64p]
    L.ngd_format_matrix.argtypes = [dp, u64, C.POINTER(C.c_char_p), C.c_char_p, u64, C.c_uint32]
    L.ngd_format_matrix.restype = C.c_int64
    L.ngd_device_memory.argtypes = [C.c_int, u64p, u64p]
    L.ngd_taus_seed.argtypes = [u32p, u64]
    L.ngd_taus_seed.restype = None
    L.ngd_taus_get.argtypes = [u32p]
    L.ngd_taus_get.restype = C.c_uint32
    L.ngd_taus_uniform.argtypes = [u32p]
    L.ngd_taus_uniform.restype = C.c_double
    L.ngd_boot_block_map.argtypes = [u32p, u64, u64p]
    L.ngd_boot_block_map.restype = None
    L.ngd_n_pairs.argtypes = [u64]
    L.ngd_n_pairs.restype = u64
    L.ngd_pair_index.argtypes = [u64, u64, u64]
    L.ngd_pair_index.restype = u64
    L.ngd_shard_of_pair.argtypes = [u64, u64, u64, C.c_uint32]
    L.ngd_shard_of_pair.restype = C.c_uint32
    L.ngd_shard_map.argtypes = [u64, C.c_uint32, C.POINTER(C.c_int32)]
    L.ngd_shard_map.restype = None
    L.ngd_score_congruence.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.ngd_score_congruence.restype = C.c_int
    L.ngd_run_windows.argtypes = [vp, u64p, u64p, u64, dp, u64p]
    L.ngd_run_windows_device.argtypes = [vp, u64p, u64p, u64, vp, vp]
    L.ngd_run_windows_dist.argtypes = [vp, u64p, u64p, u64, u64, u64, dp]
    L.ngd_last_windows.argtypes = [vp, C.POINTER(NgdWindowsInfo)]
    L.ngd_run_windows_job.argtypes = [vp, u64p, u64p, u64, u64p, C.c_uint32, u64, u64, dp, u64p]
    L.ngd_run_windows_job_device.argtypes = [vp, u64p, u64p, u64, u64p, C.c_uint32, u64, u64, vp, vp]
    L.ngd_run_windows_job_dist.argtypes = [vp, u64p, u64p, u64, u64p, C.c_uint32, u64, u64, u64, u64, dp]
    L.ngd_window_ranges.argtypes = [u32p, u64, u64, u64, u64p, u64p, u64]
    L.ngd_window_ranges.restype = C.c_int64
    L.ngd_window_ranges_bp.argtypes = [u32p, u64p, u64, u64, u64, u64, u64p, u64p, u64p, u64]
    L.ngd_window_ranges_bp.restype = C.c_int64
    L.ngd_window_boot_maps.argtypes = [u64, u64p, u64p, u64, C.c_uint32, u64, u64p, u64, u64p]
    L.ngd_window_boot_maps.restype = C.c_int64
    L.ngd_run_windows_job_var.argtypes = [vp, u64p, u64p, u64, u64p, u64, u64p, C.c_uint32, u64, dp, u64p]
    L.ngd_run_windows_job_var_device.argtypes = [vp, u64p, u64p, u64, u64p, u64, u64p, C.c_uint32, u64, vp, vp]
    L.ngd_run_windows_job_var_dist.argtypes = [vp, u64p, u64p, u64, u64p, u64, u64p, C.c_uint32, u64, u64, u64, dp]
    L.ngd_last_em_exact.argtypes = [vp, C.POINTER(NgdEmExactInfo)]
    L.ngd_em_exact_entries.argtypes = [vp, C.POINTER(NgdEmExactEntry), u64]
    L.ngd_em_exact_entries.restype = C.c_int64
    L.ngd_em2_site.argtypes = [dp, dp, dp, C.POINTER(C.c_int)]
    L.ngd_em2_site.restype = None
    L.ngd_n_group_pairs.argtypes = [C.c_uint32]
    L.ngd_n_group_pairs.restype = u64
    L.ngd_group_pair_index.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
    L.ngd_group_pair_index.restype = u64
    L.ngd_group_cells.argtypes = [C.POINTER(C.c_int32), u64, C.c_uint32, u64p]
    L.ngd_set_groups.argtypes = [vp, C.POINTER(C.c_int32), C.c_uint32]
    L.ngd_group_means_device.argtypes = [vp, vp, vp, u64, u64, u64, dp, u64p]
    L.ngd_run_job_groups.argtypes = [vp, u64p, C.c_uint32, u64, u64, u64, u64, dp, u64p]
    L.ngd_run_windows_groups.argtypes = [vp, u64p, u64p, u64, u64, u64, dp, u64p]
    L.ngd_run_windows_job_var_groups.argtypes = [vp, u64p, u64p, u64, u64p, u64, u64p, C.c_uint32, u64, u64, u64, dp, u64p]
    L.ngd_last_groups_ms.argtypes = [vp, dp]
    L.ngd_boot_stats_max_rep.argtypes = []
    L.ngd_boot_stats_max_rep.restype = C.c_uint32
    L.ngd_boot_stats_host.argtypes = [dp, u64, u64, u64, C.c_double, dp, u64p]
    L.ngd_boot_stats_device.argtypes = [vp, vp, vp, u64, u64, u64, u64, C.c_double, dp, u64p]
    L.ngd_boot_stats_values_device.argtypes = [vp, vp, u64, u64, u64, C.c_double, dp, u64p]
    L.ngd_run_job_stats.argtypes = [vp, u64p, C.c_uint32, u64, u64, u64, u64, C.c_double, dp, u64p]
    L.ngd_run_job_groups_stats.argtypes = L.ngd_run_job_stats.argtypes
    L.ngd_run_windows_job_var_stats.argtypes = [vp, u64p, u64p, u64, u64p, u64, u64p, C.c_uint32, u64, u64, u64, C.c_double, dp, u64p]
    L.ngd_run_windows_job_var_groups_stats.argtypes = L.ngd_run_windows_job_var_stats.argtypes
    L.ngd_last_boot_stats_ms.argtypes = [vp, dp]
    i32p, u32p = C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
    L.ngd_nj_max_ind.argtypes = []
    L.ngd_nj_max_ind.restype = C.c_uint32
    L.ngd_nj_host.argtypes = [dp, u64, u64, i32p, dp, u32p]
    L.ngd_nj_values_device.argtypes = [vp, vp, u64, i32p, dp, u32p]
    L.ngd_nj_device.argtypes = [vp, vp, vp, u64, u64, u64, i32p, dp, u32p]
    L.ngd_run_job_nj.argtypes = [vp, u64p, C.c_uint32, u64, u64, u64, u64, i32p, dp, u32p, dp]
    L.ngd_run_windows_nj.argtypes = [vp, u64p, u64p, u64, u64, u64, i32p, dp, u32p, dp]
    L.ngd_run_windows_job_var_nj.argtypes = [vp, u64p, u64p, u64, u64p, u64, u64p, C.c_uint32, u64, u64, u64, i32p, dp, u32p, dp]
    L.ngd_last_nj_ms.argtypes = [vp, dp]
    L.ngd_nj_support.argtypes = [i32p, u32p, u64, u64, u32p, u32p]
    L.ngd_nj_newick.argtypes = [i32p, dp, u64, C.POINTER(C.c_char_p), u32p, C.c_char_p, u64]
    L.ngd_nj_newick.restype = C.c_int64
    u32 = C.c_uint32
    L.ngd_mds_max_ind.argtypes = []
    L.ngd_mds_max_ind.restype = u32
    L.ngd_mds_max_dim.argtypes = []
    L.ngd_mds_max_dim.restype = u32
    L.ngd_mds_host.argtypes = [dp, u64, u64, u32, dp, dp, dp, u32p]
    L.ngd_mds_coords.argtypes = [dp, dp, u64, u64, u32, dp]
    L.ngd_mds_values_device.argtypes = [vp, vp, u64, u32, dp, dp, dp, u32p]
    L.ngd_mds_device.argtypes = [vp, vp, vp, u64, u64, u64, u32, dp, dp, dp, u32p]
    L.ngd_run_job_mds.argtypes = [vp, u64p, u32, u64, u64, u64, u64, u32, dp, dp, dp, u32p, dp]
    L.ngd_run_windows_mds.argtypes = [vp, u64p, u64p, u64, u64, u64, u32, dp, dp, dp, u32p, dp]
    L.ngd_run_windows_job_var_mds.argtypes = [vp, u64p, u64p, u64, u64p, u64, u64p, u32, u64, u64, u64, u32, dp, dp, dp, u32p, dp]
    L.ngd_last_mds_ms.argtypes = [vp, dp]
    L.ngd_mds_align_host.argtypes = [dp, dp, u32p, u64, u64, u64, u32, dp, dp]
    L.ngd_mds_align_values_device.argtypes = [vp, vp, u32p, u64, u64, u32, dp, dp]
    L.ngd_run_job_mds_align.argtypes = [vp, u64p, u32, u64, u64, u64, u64, u32, C.c_double, dp, dp, dp, u32p, dp, u64p, dp, dp, dp]
    L.ngd_run_windows_job_var_mds_align.argtypes = [vp, u64p, u64p, u64, u64p, u64, u64p, u32, u64, u64, u64, u32, C.c_double,
                                                    dp, dp, dp, u32p, dp, u64p, dp, dp, dp]
    L.ngd_last_mds_align_ms.argtypes = [vp, dp]
    L.ngd_win_cmp_max_vec.argtypes = []
    L.ngd_win_cmp_max_vec.restype = u32
    L.ngd_win_cmp_slice.argtypes = [u64, u64]
    L.ngd_win_cmp_slice.restype = u64
    L.ngd_win_cmp_host.argtypes = [dp, u64, u64, dp, dp, u32p]
    L.ngd_win_cmp_finish.argtypes = [dp, dp, u32p, u64, u64, dp, dp]
    L.ngd_win_cmp_values_device.argtypes = [vp, vp, u64, u64, dp, dp, u32p]
    L.ngd_win_cmp_device.argtypes = [vp, vp, vp, u64, u64, u64, dp, dp, u32p]
    L.ngd_run_windows_cmp.argtypes = [vp, u64p, u64p, u64, u64, u64, dp, dp, u32p, dp]
    L.ngd_last_win_cmp_ms.argtypes = [vp, dp]
    L.ngd_device_bytes.argtypes = [vp]
    L.ngd_device_bytes.restype = u64
    _lib = L
    return L
