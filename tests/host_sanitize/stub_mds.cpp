// tests/host_sanitize/stub_mds.cpp -- TEST INFRASTRUCTURE, never shipped: the engine's classical-MDS entry points with no
// device behind them, linked beside stub_engine.cpp so that the host's --mds path (the block maps, the groups of windows, the
// files of a run) runs under AddressSanitizer / UBSan.  They read every argument they are given and refuse what the engine
// refuses.  Matrix r of set w holds the made-up distances 1 + ((7 a + 13 b + w + 3 r) mod 10) / 10 -- a replicate of a window
// shorter than one block a NaN, as the engine's 0 / 0 -- and its outputs are ngd_mds_host's (pure host arithmetic, from
// host_util.cpp itself, like ngd_mds_coords and ngd_mds_max_dim).
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/ngsdist_amd.h"

// (stub_engine.cpp's engine begins with its ngd_config, whose first member is n_ind)
static uint64_t n_ind_of(const ngd_engine *e) { return *reinterpret_cast<const uint64_t *>(e); }

// set w of n_mat matrices; has_block: the set's replicates visit a site
static int fill(uint64_t n, uint64_t w, uint64_t n_mat, bool has_block, uint64_t evol_model, uint32_t K, double *eig, double *vec,
                double *tot, uint32_t *status, double *dist0) {
  if (!eig || !vec || !tot || !status || n < 3 || n > ngd_mds_max_ind() || !K || K > n - 1 || K > ngd_mds_max_dim()) return NGD_E_INVALID;
  if (evol_model > 2) return NGD_E_MODEL;
  const uint64_t n_pairs = n * (n - 1) / 2;
  std::vector<double> d(n_mat * n_pairs);
  for (uint64_t r = 0; r < n_mat; r++) {
    uint64_t p = 0;
    for (uint64_t a = 0; a < n; a++)
      for (uint64_t b = a + 1; b < n; b++, p++)
        d[r * n_pairs + p] = r && !has_block ? std::nan("") : 1.0 + (double)((7 * a + 13 * b + w + 3 * r) % 10) / 10.0;
  }
  if (dist0)
    for (uint64_t p = 0; p < n_pairs; p++) dist0[w * n_pairs + p] = d[p];
  const uint64_t m0 = w * n_mat;
  return ngd_mds_host(d.data(), n_mat, n, K, eig + m0 * K, vec + m0 * K * n, tot + m0 * 2, status + m0);
}

static int check_windows(const uint64_t *lo, const uint64_t *hi, uint64_t n_win, const uint64_t *maps, uint64_t maps_len,
                         const uint64_t *off, uint32_t n_rep, uint64_t q) {
  if (!lo || !hi || !n_win) return NGD_E_INVALID;
  for (uint64_t w = 0; w < n_win; w++)
    if (!(lo[w] < hi[w]) || (w && lo[w] < lo[w - 1])) return NGD_E_INVALID;
  if (!n_rep) return NGD_OK;
  if (!off || !q) return NGD_E_INVALID;
  for (uint64_t w = 0; w < n_win; w++) {
    const uint64_t n_blocks = (hi[w] - lo[w]) / q;
    if (!n_blocks) continue;
    if (!maps || off[w] > maps_len || (uint64_t)n_rep * n_blocks > maps_len - off[w]) return NGD_E_INVALID;
    for (uint64_t k = 0; k < (uint64_t)n_rep * n_blocks; k++)
      if (maps[off[w] + k] >= n_blocks) return NGD_E_INVALID;
  }
  return NGD_OK;
}

extern "C" {

uint32_t ngd_mds_max_ind(void) { return 4096; }

int ngd_run_job_mds(ngd_engine *e, const uint64_t *block_maps, uint32_t n_rep, uint64_t n_blocks, uint64_t block_size,
                    uint64_t tot_sites, uint64_t evol_model, uint32_t K, double *eig, double *vec, double *tot, uint32_t *status,
                    double *dist0) {
  (void)tot_sites;
  if (!e) return NGD_E_INVALID;
  if (n_rep) {
    if (!block_maps || !n_blocks || !block_size) return NGD_E_INVALID;
    for (uint64_t k = 0; k < (uint64_t)n_rep * n_blocks; k++)
      if (block_maps[k] >= n_blocks) return NGD_E_INVALID;
  }
  return fill(n_ind_of(e), 0, (uint64_t)n_rep + 1, true, evol_model, K, eig, vec, tot, status, dist0);
}

int ngd_run_windows_mds(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win, uint64_t tot_sites,
                        uint64_t evol_model, uint32_t K, double *eig, double *vec, double *tot, uint32_t *status, double *dist0) {
  (void)tot_sites;
  if (!e) return NGD_E_INVALID;
  if (int rc = check_windows(win_lo, win_hi, n_win, nullptr, 0, nullptr, 0, 0)) return rc;
  for (uint64_t w = 0; w < n_win; w++)
    if (int rc = fill(n_ind_of(e), w, 1, true, evol_model, K, eig, vec, tot, status, dist0)) return rc;
  return NGD_OK;
}

int ngd_run_windows_job_var_mds(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win,
                                const uint64_t *block_maps, uint64_t maps_len, const uint64_t *map_off, uint32_t n_rep,
                                uint64_t block_size, uint64_t tot_sites, uint64_t evol_model, uint32_t K, double *eig, double *vec,
                                double *tot, uint32_t *status, double *dist0) {
  (void)tot_sites;
  if (!e) return NGD_E_INVALID;
  if (int rc = check_windows(win_lo, win_hi, n_win, block_maps, maps_len, map_off, n_rep, block_size)) return rc;
  for (uint64_t w = 0; w < n_win; w++)
    if (int rc = fill(n_ind_of(e), w, (uint64_t)n_rep + 1, !n_rep || (win_hi[w] - win_lo[w]) / block_size > 0, evol_model, K, eig, vec,
                      tot, status, dist0))
      return rc;
  return NGD_OK;
}

}  // extern "C"
