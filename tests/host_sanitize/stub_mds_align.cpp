// tests/host_sanitize/stub_mds_align.cpp -- TEST INFRASTRUCTURE, never shipped: the engine's aligned-MDS entry points with no
// device behind them, linked beside stub_engine.cpp, stub_mds.cpp (whose made-up matrices and ngd_mds_host outputs they start
// from) and stub_boot_stats.cpp (ngd_boot_stats_max_rep), so that the host's --mds_align path runs under AddressSanitizer /
// UBSan.  They read every argument they are given and refuse what the engine refuses; the alignment and the summaries are
// the host twins' (ngd_mds_align_host, ngd_boot_stats_host: host_util.cpp itself).
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/ngsdist_amd.h"

static uint64_t n_ind_of(const ngd_engine *e) { return *reinterpret_cast<const uint64_t *>(e); }

struct Sets {
  std::vector<double> eig, vec, tot;
  std::vector<uint32_t> status;
  Sets(uint64_t n_set, uint64_t n_mat, uint64_t n, uint32_t K)
      : eig(n_set * n_mat * K), vec(n_set * n_mat * K * n), tot(n_set * n_mat * 2), status(n_set * n_mat) {}
};

static int refuse(const ngd_engine *e, uint32_t n_rep, double ci, const void *eig0, const void *vec0, const void *tot0, const void *status,
                  const void *stats, const void *used, const void *fit) {
  if (!e || !eig0 || !vec0 || !tot0 || !status || !stats || !used || !fit) return NGD_E_INVALID;
  if (!n_rep || !(ci > 0.0 && ci < 1.0) || n_rep > ngd_boot_stats_max_rep()) return NGD_E_INVALID;
  return NGD_OK;
}

// the sets' MDS outputs -> the aligned call's outputs
static int summarise(const Sets &s, uint64_t n_set, uint64_t n_mat, uint64_t n, uint32_t K, double ci, double *eig0, double *vec0,
                     double *tot0, uint32_t *status, double *stats, uint64_t *used, double *fit, double *aligned) {
  const uint64_t kn = K * n, n_cells = K * (n + 1);
  std::vector<double> al(n_set * n_mat * kn), cells(n_set * n_mat * n_cells);
  if (int rc = ngd_mds_align_host(s.eig.data(), s.vec.data(), s.status.data(), n_set, n_mat, n, K, al.data(), fit)) return rc;
  for (uint64_t m = 0; m < n_set * n_mat; m++) {
    memcpy(&cells[m * n_cells], &al[m * kn], kn * sizeof(double));
    for (uint32_t k = 0; k < K; k++) cells[m * n_cells + kn + k] = std::isnan(fit[m]) ? std::nan("") : s.eig[m * K + k];
  }
  std::vector<uint64_t> per_cell(n_set * n_cells);
  if (int rc = ngd_boot_stats_host(cells.data(), n_set, n_mat, n_cells, ci, stats, per_cell.data())) return rc;
  for (uint64_t w = 0; w < n_set; w++) {
    used[w] = per_cell[w * n_cells];
    memcpy(eig0 + w * K, &s.eig[w * n_mat * K], K * sizeof(double));
    memcpy(vec0 + w * kn, &s.vec[w * n_mat * kn], kn * sizeof(double));
    memcpy(tot0 + w * 2, &s.tot[w * n_mat * 2], 2 * sizeof(double));
  }
  memcpy(status, s.status.data(), n_set * n_mat * sizeof(uint32_t));
  if (aligned) memcpy(aligned, al.data(), al.size() * sizeof(double));
  return NGD_OK;
}

extern "C" {

int ngd_run_job_mds_align(ngd_engine *e, const uint64_t *block_maps, uint32_t n_rep, uint64_t n_blocks, uint64_t block_size,
                          uint64_t tot_sites, uint64_t evol_model, uint32_t K, double ci, double *eig0, double *vec0, double *tot0,
                          uint32_t *status, double *stats, uint64_t *used, double *fit, double *aligned, double *dist0) {
  if (int rc = refuse(e, n_rep, ci, eig0, vec0, tot0, status, stats, used, fit)) return rc;
  const uint64_t n = n_ind_of(e), n_mat = (uint64_t)n_rep + 1;
  if (n < 3 || !K || K > n - 1 || K > ngd_mds_max_dim()) return NGD_E_INVALID;
  Sets s(1, n_mat, n, K);
  if (int rc = ngd_run_job_mds(e, block_maps, n_rep, n_blocks, block_size, tot_sites, evol_model, K, s.eig.data(), s.vec.data(),
                               s.tot.data(), s.status.data(), dist0))
    return rc;
  return summarise(s, 1, n_mat, n, K, ci, eig0, vec0, tot0, status, stats, used, fit, aligned);
}

int ngd_run_windows_job_var_mds_align(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win,
                                      const uint64_t *block_maps, uint64_t maps_len, const uint64_t *map_off, uint32_t n_rep,
                                      uint64_t block_size, uint64_t tot_sites, uint64_t evol_model, uint32_t K, double ci,
                                      double *eig0, double *vec0, double *tot0, uint32_t *status, double *stats, uint64_t *used,
                                      double *fit, double *aligned, double *dist0) {
  if (int rc = refuse(e, n_rep, ci, eig0, vec0, tot0, status, stats, used, fit)) return rc;
  const uint64_t n = n_ind_of(e), n_mat = (uint64_t)n_rep + 1;
  if (n < 3 || !K || K > n - 1 || K > ngd_mds_max_dim() || !n_win) return NGD_E_INVALID;
  Sets s(n_win, n_mat, n, K);
  if (int rc = ngd_run_windows_job_var_mds(e, win_lo, win_hi, n_win, block_maps, maps_len, map_off, n_rep, block_size, tot_sites,
                                           evol_model, K, s.eig.data(), s.vec.data(), s.tot.data(), s.status.data(), dist0))
    return rc;
  return summarise(s, n_win, n_mat, n, K, ci, eig0, vec0, tot0, status, stats, used, fit, aligned);
}

}  // extern "C"
