// tests/host_sanitize/stub_windows.cpp -- TEST INFRASTRUCTURE, never shipped: the engine's windowed entry point with no
// compute behind it, linked beside stub_engine.cpp so that the host's --win_size path (window list, groups of windows per
// call, printing, the .windows file) runs under AddressSanitizer / UBSan.  Every window's cells are its index + the pair's
// index / 1000, so that the printed matrices show which window they came from.
#include <cstdint>

#include "../../include/ngsdist_amd.h"

extern "C" int ngd_run_windows_dist(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win,
                                    uint64_t tot_sites, uint64_t evol_model, double *dist) {
  (void)tot_sites;
  if (!e || !win_lo || !win_hi || !n_win || !dist) return NGD_E_INVALID;
  if (evol_model > 2) return NGD_E_MODEL;
  static uint64_t first = 0;  // windows handed in by earlier calls of this process: the global index of win_lo[0]
  uint64_t n_pairs = 0;
  for (uint64_t w = 0; w < n_win; w++) {
    if (!(win_lo[w] < win_hi[w]) || (w && win_lo[w] < win_lo[w - 1])) return NGD_E_INVALID;
  }
  // n_ind: the first member of stub_engine.cpp's engine is its ngd_config, whose first member is n_ind
  n_pairs = ngd_n_pairs(*reinterpret_cast<const uint64_t *>(e));
  for (uint64_t w = 0; w < n_win; w++)
    for (uint64_t k = 0; k < n_pairs; k++) dist[w * n_pairs + k] = (double)(first + w) + (double)k / 1000.0;
  first += n_win;
  return NGD_OK;
}
