// engine_boot_stats.hip -- bootstrap summaries per cell: the reduction over the replicates of a set (boot_stats.hip) of device
// matrices, and that reduction as a tail (ngd_engine.h) behind the job driver and the window driver (after the group
// reduction, in the _groups forms): the run forms, where 5 doubles and a count per cell cross the link instead of n_rep + 1
// sums and counts.
#include "ngd_engine.h"

uint32_t ngd_boot_stats_max_rep(void) { return NGD_BOOT_MAX_MAT - 1; }

// what every call that summarises refuses, before anything is launched; the interval's two ranks' fractions on the way
int boot_refuse(const ngd_engine *e, const void *stats, const void *used, uint64_t n_mat, double ci, uint64_t tot_sites,
                uint64_t evol_model, bool groups, const char *who, BootCi &out) {
  const std::string w(who);
  if (!e) return fail(NGD_E_INVALID, w + ": null engine");
  if (!stats || !used) return fail(NGD_E_INVALID, w + ": null output");
  if (n_mat < 2) return fail(NGD_E_INVALID, w + ": no replicates to summarise (n_rep 0)");
  if (!(ci > 0.0 && ci < 1.0)) return fail(NGD_E_INVALID, w + ": the interval's coverage must lie in (0, 1)");
  if (n_mat - 1 > ngd_boot_stats_max_rep())
    return fail(NGD_E_INVALID, w + ": more than " + std::to_string(ngd_boot_stats_max_rep()) +
                                   " replicates (a cell's values stay in on-chip memory: ngd_boot_stats_max_rep)");
  if (groups && !e->grp.n_groups) return fail(NGD_E_INVALID, w + ": no grouping set (ngd_set_groups)");
  if (int rc = finish_refuse(e, tot_sites, evol_model, w, "no summaries")) return rc;
  out.p_lo = (1.0 - ci) / 2.0;
  out.p_hi = 1.0 - out.p_lo;
  return NGD_OK;
}

// The sets in chunks whose results stay small (~256 MB) and whose launches fit grid.x; a set's bits do not depend on the
// chunk it falls into.  Events 0 and 1 time each chunk's kernel (bst.ms: the entry points start it at 0, a windowed call
// adds up its groups of windows).
// [n_set][n_mat][n_cells] device matrices -> stats / used in host memory; d_cnt and the two arguments of ngd_finish for sums
// and counts, `values` for cells as they are (the arguments are checked)
int boot_reduce(ngd_engine *e, const double *d_a, const unsigned long long *d_cnt, bool values, uint64_t n_set, uint64_t n_mat,
                uint64_t n_cells, uint64_t tot_sites, uint64_t evol_model, BootCi ci, double *stats, uint64_t *used) {
  auto &b = e->bst;
  if (!n_cells) return NGD_OK;
  const uint64_t tiles = (n_cells + ngd_boot_tile(n_mat) - 1) / ngd_boot_tile(n_mat);
  if (tiles >= (1ull << 31)) return fail(NGD_E_INVALID, "bootstrap summaries: too many cells in a set (2^31 tiles and more)");
  const uint64_t by_bytes = (256ull << 20) / (n_cells * (NGD_BOOT_NSTAT + 1) * 8), by_grid = ((1ull << 31) - 1) / tiles;
  const uint64_t chunk = std::max<uint64_t>(1, std::min(n_set, std::min(by_bytes, by_grid)));
  int rc = b.d_stats.ensure(e, chunk * NGD_BOOT_NSTAT * n_cells);
  if (!rc) rc = b.d_used.ensure(e, chunk * n_cells);
  if (rc) return rc;
  for (uint64_t s0 = 0; s0 < n_set; s0 += chunk) {
    const uint64_t n = std::min(chunk, n_set - s0), at = s0 * n_mat * n_cells;
    HIPCHK(hipEventRecord(e->ev[0], e->st));
    HIPCHK((hipError_t)ngd_launch_boot_stats(e->st, d_a + at, d_cnt ? d_cnt + at : nullptr, values, n, (uint32_t)n_mat, n_cells, tot_sites,
                                             (uint32_t)evol_model, ci.p_lo, ci.p_hi, b.d_stats, b.d_used));
    HIPCHK(hipEventRecord(e->ev[1], e->st));
    HIPCHK(hipMemcpyAsync(stats + s0 * NGD_BOOT_NSTAT * n_cells, b.d_stats, n * NGD_BOOT_NSTAT * n_cells * sizeof(double),
                          hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipMemcpyAsync(used + s0 * n_cells, b.d_used, n * n_cells * sizeof(uint64_t), hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipStreamSynchronize(e->st));
    float ms = 0;
    hipEventElapsedTime(&ms, e->ev[0], e->ev[1]);
    b.ms += ms;
  }
  return NGD_OK;
}

int ngd_boot_stats_device(ngd_engine *e, const void *d_sum, const void *d_cnt, uint64_t n_set, uint64_t n_mat, uint64_t tot_sites,
                          uint64_t evol_model, double ci, double *stats, uint64_t *used) {
  BootCi c{};
  if (int rc = boot_refuse(e, stats, used, n_mat, ci, tot_sites, evol_model, false, "ngd_boot_stats_device", c)) return rc;
  if (!d_sum || (!d_cnt && !tot_sites) || !n_set) return fail(NGD_E_INVALID, "ngd_boot_stats_device: null matrices");
  e->bst.ms = 0;
  HIPCHK(hipSetDevice(e->device));
  return boot_reduce(e, (const double *)d_sum, (const unsigned long long *)d_cnt, false, n_set, n_mat, ngd_n_pairs(e->g.n_ind),
                     tot_sites, evol_model, c, stats, used);
}

int ngd_boot_stats_values_device(ngd_engine *e, const void *d_val, uint64_t n_set, uint64_t n_mat, uint64_t n_cells, double ci,
                                 double *stats, uint64_t *used) {
  BootCi c{};
  if (int rc = boot_refuse(e, stats, used, n_mat, ci, 0, 0, false, "ngd_boot_stats_values_device", c)) return rc;
  if (!d_val || !n_set || !n_cells) return fail(NGD_E_INVALID, "ngd_boot_stats_values_device: null matrices");
  e->bst.ms = 0;
  HIPCHK(hipSetDevice(e->device));
  return boot_reduce(e, (const double *)d_val, nullptr, true, n_set, n_mat, n_cells, 0, 0, c, stats, used);
}

// the tail of the run forms: every set's summaries into stats / used [.][5][n_cells] / [.][n_cells] -- of its cells, or
// (groups) of its group means: the group reduction first, its means kept on the device, n_cells = n_gp
static Tail stats_tail(ngd_engine *e, bool groups, uint64_t tot_sites, uint64_t evol_model, BootCi ci, double *stats, uint64_t *used) {
  return [=](uint64_t set0, uint64_t n_set, uint64_t n_mat) {
    const uint64_t n_cells = groups ? e->grp.n_gp : ngd_n_pairs(e->g.n_ind);
    double *s = stats + set0 * NGD_BOOT_NSTAT * n_cells;
    uint64_t *u = used + set0 * n_cells;
    if (!groups) return boot_reduce(e, e->d_bsum, e->d_bcnt, false, n_set, n_mat, n_cells, tot_sites, evol_model, ci, s, u);
    if (int rc = groups_reduce(e, e->d_bsum, e->d_bcnt, n_set * n_mat, tot_sites, evol_model, nullptr, nullptr)) return rc;
    return boot_reduce(e, e->grp.d_keep_mean, nullptr, true, n_set, n_mat, n_cells, 0, 0, ci, s, u);
  };
}

static int job_stats(ngd_engine *e, const uint64_t *block_maps, uint32_t n_rep, uint64_t n_blocks, uint64_t block_size,
                     uint64_t tot_sites, uint64_t evol_model, double ci, bool groups, double *stats, uint64_t *used, const char *who) {
  BootCi c{};
  if (int rc = boot_refuse(e, stats, used, (uint64_t)n_rep + 1, ci, tot_sites, evol_model, groups, who, c)) return rc;
  if (!block_maps) return fail(NGD_E_INVALID, std::string(who) + ": null argument");
  e->bst.ms = e->grp.ms = 0;  // (both, in either job form)
  return job_tail(e, block_maps, n_rep, n_blocks, block_size, stats_tail(e, groups, tot_sites, evol_model, c, stats, used));
}

int ngd_run_job_stats(ngd_engine *e, const uint64_t *block_maps, uint32_t n_rep, uint64_t n_blocks, uint64_t block_size,
                      uint64_t tot_sites, uint64_t evol_model, double ci, double *stats, uint64_t *used) {
  return job_stats(e, block_maps, n_rep, n_blocks, block_size, tot_sites, evol_model, ci, false, stats, used, "ngd_run_job_stats");
}

int ngd_run_job_groups_stats(ngd_engine *e, const uint64_t *block_maps, uint32_t n_rep, uint64_t n_blocks, uint64_t block_size,
                             uint64_t tot_sites, uint64_t evol_model, double ci, double *stats, uint64_t *used) {
  return job_stats(e, block_maps, n_rep, n_blocks, block_size, tot_sites, evol_model, ci, true, stats, used, "ngd_run_job_groups_stats");
}

// the windowed forms (n_rep == 0 has been refused: always a job's check)
static int windows_stats(ngd_engine *e, const WinJobArgs &a, uint64_t tot_sites, uint64_t evol_model, double ci, bool groups,
                         double *stats, uint64_t *used, const char *who) {
  BootCi c{};
  if (int rc = boot_refuse(e, stats, used, (uint64_t)a.n_rep + 1, ci, tot_sites, evol_model, groups, who, c)) return rc;
  e->bst.ms = 0;
  if (groups) e->grp.ms = 0;
  return windows_tail(e, a, true, who, stats_tail(e, groups, tot_sites, evol_model, c, stats, used));
}

int ngd_run_windows_job_var_stats(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win,
                                  const uint64_t *block_maps, uint64_t maps_len, const uint64_t *map_off, uint32_t n_rep,
                                  uint64_t block_size, uint64_t tot_sites, uint64_t evol_model, double ci, double *stats,
                                  uint64_t *used) {
  return windows_stats(e, WinJobArgs{win_lo, win_hi, n_win, block_maps, maps_len, map_off, n_rep, block_size}, tot_sites, evol_model,
                       ci, false, stats, used, "ngd_run_windows_job_var_stats");
}

int ngd_run_windows_job_var_groups_stats(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win,
                                         const uint64_t *block_maps, uint64_t maps_len, const uint64_t *map_off, uint32_t n_rep,
                                         uint64_t block_size, uint64_t tot_sites, uint64_t evol_model, double ci, double *stats,
                                         uint64_t *used) {
  return windows_stats(e, WinJobArgs{win_lo, win_hi, n_win, block_maps, maps_len, map_off, n_rep, block_size}, tot_sites, evol_model,
                       ci, true, stats, used, "ngd_run_windows_job_var_groups_stats");
}

int ngd_last_boot_stats_ms(const ngd_engine *e, double *ms) {
  if (!e || !ms) return fail(NGD_E_INVALID, "ngd_last_boot_stats_ms: null argument");
  *ms = e->bst.ms;
  return NGD_OK;
}
