// tests/host_sanitize/stub_groups.cpp -- TEST INFRASTRUCTURE, never shipped: the engine's group-mean entry points with no
// compute behind them, linked beside stub_engine.cpp so that the host's --groups path (the groups file, the batches of
// replicates, per-window block maps, the G x G blocks of <out> and <out>.used) runs under AddressSanitizer / UBSan.  They read
// every argument they are given and refuse what the engine refuses.  Matrix m of a call holds m + gp / 100 as the mean of
// group pair gp and gp + 1 as its count -- except a group pair without a cell (a group of one on the diagonal, an empty
// group): nan and 0, as the engine has it.
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/ngsdist_amd.h"

static std::vector<uint64_t> g_size;  // members of every group of the last ngd_set_groups (one engine at a time)

// (stub_engine.cpp's engine begins with its ngd_config, whose first member is n_ind)
static uint64_t n_ind_of(const ngd_engine *e) { return *reinterpret_cast<const uint64_t *>(e); }

static int fill(uint64_t n_mat, double *mean, uint64_t *used) {
  if (g_size.empty() || !mean) return NGD_E_INVALID;
  const uint64_t G = g_size.size(), n_gp = G * (G + 1) / 2;
  for (uint64_t m = 0; m < n_mat; m++) {
    uint64_t gp = 0;
    for (uint64_t a = 0; a < G; a++)
      for (uint64_t b = a; b < G; b++, gp++) {
        const bool none = a == b ? g_size[a] < 2 : !g_size[a] || !g_size[b];
        mean[m * n_gp + gp] = none ? std::nan("") : (double)m + (double)gp / 100.0;
        if (used) used[m * n_gp + gp] = none ? 0 : gp + 1;
      }
  }
  return NGD_OK;
}

extern "C" {

int ngd_set_groups(ngd_engine *e, const int32_t *group_of, uint32_t n_groups) {
  if (!e || !group_of != !n_groups) return NGD_E_INVALID;
  std::vector<uint64_t> size(n_groups, 0);
  for (uint64_t i = 0; group_of && i < n_ind_of(e); i++) {
    if (group_of[i] < -1 || group_of[i] >= (int64_t)n_groups) return NGD_E_INVALID;
    if (group_of[i] >= 0) size[group_of[i]]++;
  }
  g_size = size;
  return NGD_OK;
}

int ngd_run_job_groups(ngd_engine *e, const uint64_t *block_maps, uint32_t n_rep, uint64_t n_blocks, uint64_t block_size,
                       uint64_t tot_sites, uint64_t evol_model, double *mean, uint64_t *used) {
  (void)tot_sites;
  if (!e || (n_rep && (!block_maps || !n_blocks || !block_size))) return NGD_E_INVALID;
  if (evol_model > 2) return NGD_E_MODEL;
  for (uint64_t k = 0; k < (uint64_t)n_rep * n_blocks; k++)
    if (block_maps[k] >= n_blocks) return NGD_E_INVALID;
  return fill((uint64_t)n_rep + 1, mean, used);
}

int ngd_run_windows_groups(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win, uint64_t tot_sites,
                           uint64_t evol_model, double *mean, uint64_t *used) {
  (void)tot_sites;
  if (!e || !win_lo || !win_hi || !n_win) return NGD_E_INVALID;
  if (evol_model > 2) return NGD_E_MODEL;
  for (uint64_t w = 0; w < n_win; w++)
    if (!(win_lo[w] < win_hi[w]) || (w && win_lo[w] < win_lo[w - 1])) return NGD_E_INVALID;
  return fill(n_win, mean, used);
}

int ngd_run_windows_job_var_groups(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win,
                                   const uint64_t *block_maps, uint64_t maps_len, const uint64_t *map_off, uint32_t n_rep,
                                   uint64_t block_size, uint64_t tot_sites, uint64_t evol_model, double *mean, uint64_t *used) {
  (void)tot_sites;
  if (!e || !win_lo || !win_hi || !n_win) return NGD_E_INVALID;
  if (evol_model > 2) return NGD_E_MODEL;
  if (n_rep && (!block_maps || !map_off || !block_size)) return NGD_E_INVALID;
  for (uint64_t w = 0; w < n_win; w++) {
    if (!(win_lo[w] < win_hi[w]) || (w && win_lo[w] < win_lo[w - 1])) return NGD_E_INVALID;
    const uint64_t n_blocks = n_rep ? (win_hi[w] - win_lo[w]) / block_size : 0;
    if (!n_blocks) continue;
    if (map_off[w] > maps_len || (uint64_t)n_rep * n_blocks > maps_len - map_off[w]) return NGD_E_INVALID;
    for (uint64_t k = 0; k < (uint64_t)n_rep * n_blocks; k++)
      if (block_maps[map_off[w] + k] >= n_blocks) return NGD_E_INVALID;
  }
  return fill(n_win * ((uint64_t)n_rep + 1), mean, used);
}

}  // extern "C"
