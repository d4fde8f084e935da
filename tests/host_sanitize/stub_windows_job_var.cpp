// tests/host_sanitize/stub_windows_job_var.cpp -- TEST INFRASTRUCTURE, never shipped: the engine's entry point for bootstrap
// replicates inside windows of unequal length with no compute behind it, linked beside stub_engine.cpp and stub_windows.cpp so
// that the host's --win_bp --win_boot_rep path (per-window block maps, groups of windows per call, window-major printing)
// runs under AddressSanitizer / UBSan.  It reads every argument it is given -- every window's maps to their last entry -- and
// refuses what the engine refuses.  Matrix m of window w holds w + m / 100 + the pair's index / 100000, so that the printed
// matrices show which window and matrix they came from; the replicates of a window shorter than one block are 0 / 0.
#include <cmath>
#include <cstdint>

#include "../../include/ngsdist_amd.h"

extern "C" int ngd_run_windows_job_var_dist(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win,
                                            const uint64_t *block_maps, uint64_t maps_len, const uint64_t *map_off, uint32_t n_rep,
                                            uint64_t block_size, uint64_t tot_sites, uint64_t evol_model, double *dist) {
  (void)tot_sites;
  if (!e || !win_lo || !win_hi || !n_win || !dist) return NGD_E_INVALID;
  if (evol_model > 2) return NGD_E_MODEL;
  if (n_rep && (!block_maps || !map_off || !block_size)) return NGD_E_INVALID;
  static uint64_t first = 0;  // windows handed in by earlier calls of this process: the global index of win_lo[0]
  for (uint64_t w = 0; w < n_win; w++) {
    if (!(win_lo[w] < win_hi[w]) || (w && win_lo[w] < win_lo[w - 1])) return NGD_E_INVALID;
    const uint64_t n_blocks = n_rep ? (win_hi[w] - win_lo[w]) / block_size : 0;
    if (!n_blocks) continue;
    if (map_off[w] > maps_len || (uint64_t)n_rep * n_blocks > maps_len - map_off[w]) return NGD_E_INVALID;
    for (uint64_t k = 0; k < (uint64_t)n_rep * n_blocks; k++)
      if (block_maps[map_off[w] + k] >= n_blocks) return NGD_E_INVALID;
  }
  // n_ind: the first member of stub_engine.cpp's engine is its ngd_config, whose first member is n_ind
  const uint64_t n_pairs = ngd_n_pairs(*reinterpret_cast<const uint64_t *>(e)), n_mat = (uint64_t)n_rep + 1;
  for (uint64_t w = 0; w < n_win; w++) {
    const bool no_block = n_rep && (win_hi[w] - win_lo[w]) / block_size == 0;
    for (uint64_t m = 0; m < n_mat; m++)
      for (uint64_t k = 0; k < n_pairs; k++)
        dist[(w * n_mat + m) * n_pairs + k] = m && no_block ? std::nan("") : (double)(first + w) + (double)m / 100.0 + (double)k / 100000.0;
  }
  first += n_win;
  return NGD_OK;
}
