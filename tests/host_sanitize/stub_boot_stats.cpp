// tests/host_sanitize/stub_boot_stats.cpp -- TEST INFRASTRUCTURE, never shipped: the engine's bootstrap-summary entry points
// with no compute behind them, linked beside stub_engine.cpp (and stub_groups.cpp) so that the host's --boot_stats path (the
// block maps, the groups of windows, the six files of a run) runs under AddressSanitizer / UBSan.  They read every argument
// they are given and refuse what the engine refuses.  Cell c of set w holds w + k / 10 + c / 1000 as statistic k and n_rep as
// its count.  (ngd_boot_stats_host, pure host arithmetic, comes from host_util.cpp itself.)
#include <cstdint>
#include <cstdlib>

#include "../../include/ngsdist_amd.h"

// (stub_engine.cpp's engine begins with its ngd_config, whose first member is n_ind)
static uint64_t n_pairs_of(const ngd_engine *e) {
  const uint64_t n = *reinterpret_cast<const uint64_t *>(e);
  return n * (n - 1) / 2;
}

static uint64_t g_gp = 0;  // group pairs the group forms fill (0: not told)

static int fill(uint64_t n_set, uint64_t n_cells, uint32_t n_rep, double ci, uint64_t evol_model, double *stats, uint64_t *used) {
  if (!stats || !used || !n_rep || !(ci > 0.0 && ci < 1.0) || n_rep > ngd_boot_stats_max_rep()) return NGD_E_INVALID;
  if (evol_model > 2) return NGD_E_MODEL;
  for (uint64_t w = 0; w < n_set; w++)
    for (uint64_t c = 0; c < n_cells; c++) {
      for (uint64_t k = 0; k < NGD_BOOT_NSTAT; k++)
        stats[(w * NGD_BOOT_NSTAT + k) * n_cells + c] = (double)w + (double)k / 10.0 + (double)c / 1000.0;
      used[w * n_cells + c] = n_rep;
    }
  return NGD_OK;
}

static int check_windows(const uint64_t *lo, const uint64_t *hi, uint64_t n_win, const uint64_t *maps, uint64_t maps_len,
                         const uint64_t *off, uint32_t n_rep, uint64_t q) {
  if (!lo || !hi || !n_win || !n_rep || !off || !q) return NGD_E_INVALID;
  for (uint64_t w = 0; w < n_win; w++) {
    if (!(lo[w] < hi[w]) || (w && lo[w] < lo[w - 1])) return NGD_E_INVALID;
    const uint64_t n_blocks = (hi[w] - lo[w]) / q;
    if (!n_blocks) continue;
    if (!maps || off[w] > maps_len || (uint64_t)n_rep * n_blocks > maps_len - off[w]) return NGD_E_INVALID;
    for (uint64_t k = 0; k < (uint64_t)n_rep * n_blocks; k++)
      if (maps[off[w] + k] >= n_blocks) return NGD_E_INVALID;
  }
  return NGD_OK;
}

static int check_job(const uint64_t *maps, uint32_t n_rep, uint64_t n_blocks, uint64_t q) {
  if (!n_rep || !maps || !n_blocks || !q) return NGD_E_INVALID;
  for (uint64_t k = 0; k < (uint64_t)n_rep * n_blocks; k++)
    if (maps[k] >= n_blocks) return NGD_E_INVALID;
  return NGD_OK;
}

extern "C" {

uint32_t ngd_boot_stats_max_rep(void) { return 1279; }

// the number of group pairs the group forms fill: told by the test's command line through the environment, since
// stub_groups.cpp keeps the grouping to itself
static uint64_t group_pairs() {
  if (!g_gp) {
    const char *s = getenv("NGD_STUB_GROUP_PAIRS");
    g_gp = s ? strtoull(s, nullptr, 10) : 0;
  }
  return g_gp;
}

int ngd_run_job_stats(ngd_engine *e, const uint64_t *block_maps, uint32_t n_rep, uint64_t n_blocks, uint64_t block_size,
                      uint64_t tot_sites, uint64_t evol_model, double ci, double *stats, uint64_t *used) {
  (void)tot_sites;
  if (!e) return NGD_E_INVALID;
  if (int rc = check_job(block_maps, n_rep, n_blocks, block_size)) return rc;
  return fill(1, n_pairs_of(e), n_rep, ci, evol_model, stats, used);
}

int ngd_run_job_groups_stats(ngd_engine *e, const uint64_t *block_maps, uint32_t n_rep, uint64_t n_blocks, uint64_t block_size,
                             uint64_t tot_sites, uint64_t evol_model, double ci, double *stats, uint64_t *used) {
  (void)tot_sites;
  if (!e || !group_pairs()) return NGD_E_INVALID;
  if (int rc = check_job(block_maps, n_rep, n_blocks, block_size)) return rc;
  return fill(1, group_pairs(), n_rep, ci, evol_model, stats, used);
}

int ngd_run_windows_job_var_stats(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win,
                                  const uint64_t *block_maps, uint64_t maps_len, const uint64_t *map_off, uint32_t n_rep,
                                  uint64_t block_size, uint64_t tot_sites, uint64_t evol_model, double ci, double *stats,
                                  uint64_t *used) {
  (void)tot_sites;
  if (!e) return NGD_E_INVALID;
  if (int rc = check_windows(win_lo, win_hi, n_win, block_maps, maps_len, map_off, n_rep, block_size)) return rc;
  return fill(n_win, n_pairs_of(e), n_rep, ci, evol_model, stats, used);
}

int ngd_run_windows_job_var_groups_stats(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win,
                                         const uint64_t *block_maps, uint64_t maps_len, const uint64_t *map_off, uint32_t n_rep,
                                         uint64_t block_size, uint64_t tot_sites, uint64_t evol_model, double ci, double *stats,
                                         uint64_t *used) {
  (void)tot_sites;
  if (!e || !group_pairs()) return NGD_E_INVALID;
  if (int rc = check_windows(win_lo, win_hi, n_win, block_maps, maps_len, map_off, n_rep, block_size)) return rc;
  return fill(n_win, group_pairs(), n_rep, ci, evol_model, stats, used);
}

}  // extern "C"
