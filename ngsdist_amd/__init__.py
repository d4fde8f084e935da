"""ngsdist_amd -- MI355X-native engine for the gen_dist() hot path of ngsDist.

Only what the path needs lives here: csrc/ (HIP kernels, the C ABI, the C++
host driver) and this thin ctypes door.  Importing the package does not load
the library; the first Engine()/finish()/Taus() does, and fails loudly if the
HIP engine was not built.
"""
from .engine import (DEFAULT_SCORE, KERNELS, Engine, NgdError, Taus, device_count, em2_site, finish, format_matrix, n_pairs,
                     score_congruence, score_matrix, window_boot_maps, window_ranges, window_ranges_bp, n_group_pairs,
                     group_pair_index, group_cells, expand_groups, boot_stats_host, boot_stats_max_rep, nj_host, nj_support, nj_newick,
                     nj_max_ind, mds_host, mds_coords, mds_max_ind, mds_max_dim, mds_align_host,
                     win_cmp_host, win_cmp_finish, win_cmp_slice, win_cmp_max_vec)

__all__ = ["Engine", "NgdError", "Taus", "finish", "format_matrix", "device_count", "n_pairs", "score_matrix",
           "score_congruence", "window_ranges", "window_ranges_bp", "window_boot_maps", "em2_site", "DEFAULT_SCORE", "KERNELS",
           "n_group_pairs", "group_pair_index", "group_cells", "expand_groups", "boot_stats_host", "boot_stats_max_rep",
           "nj_host", "nj_support", "nj_newick", "nj_max_ind", "mds_host", "mds_coords", "mds_max_ind", "mds_max_dim",
           "mds_align_host", "win_cmp_host", "win_cmp_finish", "win_cmp_slice", "win_cmp_max_vec"]
