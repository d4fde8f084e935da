// tests/host_sanitize/stub_win_cmp.cpp -- TEST INFRASTRUCTURE, never shipped: the engine's comparison of windows with no
// device behind it, linked beside stub_engine.cpp so that the host's --win_cmp path (the tables, the ordination of the windows)
// runs under AddressSanitizer / UBSan.  It reads every argument it is given and refuses what the engine refuses.  Window w holds
// the made-up distances 1 + ((7 a + 13 b + 3 w + a b w) mod 10) / 10; a window shorter than 3 sites, and one that starts at
// site 20, has a NaN cell, as a pair without sites gives under --pairwise_del.  The outputs are ngd_win_cmp_host's (pure host
// arithmetic, from host_util.cpp itself, like ngd_win_cmp_finish and ngd_win_cmp_max_vec).
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/ngsdist_amd.h"

// (stub_engine.cpp's engine begins with its ngd_config, whose first member is n_ind)
static uint64_t n_ind_of(const ngd_engine *e) { return *reinterpret_cast<const uint64_t *>(e); }

extern "C" int ngd_run_windows_cmp(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win, uint64_t tot_sites,
                                   uint64_t evol_model, double *mean, double *gram, uint32_t *status, double *dist) {
  (void)tot_sites;
  if (!e || !mean || !gram || !status || !win_lo || !win_hi || !n_win || n_win > ngd_win_cmp_max_vec()) return NGD_E_INVALID;
  if (evol_model > 2) return NGD_E_MODEL;
  for (uint64_t w = 0; w < n_win; w++)
    if (!(win_lo[w] < win_hi[w]) || (w && win_lo[w] < win_lo[w - 1])) return NGD_E_INVALID;
  const uint64_t n = n_ind_of(e), n_pairs = n * (n - 1) / 2;
  if (n < 2) return NGD_E_INVALID;
  std::vector<double> d(n_win * n_pairs);
  for (uint64_t w = 0; w < n_win; w++) {
    uint64_t p = 0;
    for (uint64_t a = 0; a < n; a++)
      for (uint64_t b = a + 1; b < n; b++, p++) d[w * n_pairs + p] = 1.0 + (double)((7 * a + 13 * b + 3 * w + a * b * w) % 10) / 10.0;
    if (win_hi[w] - win_lo[w] < 3 || win_lo[w] == 20) d[w * n_pairs + n_pairs / 2] = std::nan("");
  }
  if (dist)
    for (uint64_t k = 0; k < n_win * n_pairs; k++) dist[k] = d[k];
  return ngd_win_cmp_host(d.data(), n_win, n_pairs, mean, gram, status);
}
