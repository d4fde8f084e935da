// engine_boot_stats.hip -- bootstrap summaries per cell: the reduction over the replicates of a set (boot_stats.hip) of device
// matrices, and the run forms that end a job's tail on the device -- the sibling *_device call into the engine's batch
// buffers, then that reduction (after the group reduction, in the _groups forms); 5 doubles and a count per cell cross the
// link instead of n_rep + 1 sums and counts.
#include "ngd_engine.h"

uint32_t ngd_boot_stats_max_rep(void) { return NGD_BOOT_MAX_MAT - 1; }

// what every call that summarises refuses, before anything is launched; the interval's two ranks' fractions on the way
static int boot_refuse(const ngd_engine *e, const void *stats, const void *used, uint64_t n_mat, double ci, uint64_t tot_sites,
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
  if (tot_sites && e->cfg.pairwise_del)
    return fail(NGD_E_INVALID, w + ": a total number of sites cannot go with pairwise deletion (parse_args.cpp:209-210)");
  if (evol_model > 2) return fail(NGD_E_MODEL, w + ": evolutionary model not supported (ngsDist.cpp:398-399)");
  if (e->cfg.shard_world > 1)
    return fail(NGD_E_INVALID, w + ": an engine that owns a share of the pairs holds part of every matrix: no summaries");
  out.p_lo = (1.0 - ci) / 2.0;
  out.p_hi = 1.0 - out.p_lo;
  return NGD_OK;
}

// The sets in chunks whose results stay small (~256 MB) and whose launches fit grid.x; a set's bits do not depend on the
// chunk it falls into.  Events 0 and 1 time each chunk's kernel (bst.ms: the entry points start it at 0, a windowed call
// adds up its groups of windows).
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

// ngd_run_job_device into the batch buffers, where the matrices stay (ngd_fetch_matrix), then the set's summaries
static int job_stats(ngd_engine *e, const uint64_t *block_maps, uint32_t n_rep, uint64_t n_blocks, uint64_t block_size,
                     uint64_t tot_sites, uint64_t evol_model, double ci, bool groups, double *stats, uint64_t *used, const char *who) {
  BootCi c{};
  if (int rc = boot_refuse(e, stats, used, (uint64_t)n_rep + 1, ci, tot_sites, evol_model, groups, who, c)) return rc;
  if (!block_maps) return fail(NGD_E_INVALID, std::string(who) + ": null argument");
  e->bst.ms = e->grp.ms = 0;
  const uint64_t n_mat = (uint64_t)n_rep + 1;
  if (int rc = batch_buffers(e, n_rep + 1)) return rc;
  if (int rc = run_impl(e, block_maps, nullptr, n_rep, true, n_blocks, block_size, e->d_bsum, e->d_bcnt)) return rc;
  e->n_batch_valid = n_rep + 1;
  if (!groups) return boot_reduce(e, e->d_bsum, e->d_bcnt, false, 1, n_mat, ngd_n_pairs(e->g.n_ind), tot_sites, evol_model, c, stats, used);
  if (int rc = groups_reduce_keep(e, e->d_bsum, e->d_bcnt, n_mat, tot_sites, evol_model)) return rc;
  return boot_reduce(e, e->grp.d_keep_mean, nullptr, true, 1, n_mat, e->grp.n_gp, 0, 0, c, stats, used);
}

int ngd_run_job_stats(ngd_engine *e, const uint64_t *block_maps, uint32_t n_rep, uint64_t n_blocks, uint64_t block_size,
                      uint64_t tot_sites, uint64_t evol_model, double ci, double *stats, uint64_t *used) {
  return job_stats(e, block_maps, n_rep, n_blocks, block_size, tot_sites, evol_model, ci, false, stats, used, "ngd_run_job_stats");
}

int ngd_run_job_groups_stats(ngd_engine *e, const uint64_t *block_maps, uint32_t n_rep, uint64_t n_blocks, uint64_t block_size,
                             uint64_t tot_sites, uint64_t evol_model, double ci, double *stats, uint64_t *used) {
  return job_stats(e, block_maps, n_rep, n_blocks, block_size, tot_sites, evol_model, ci, true, stats, used, "ngd_run_job_groups_stats");
}

int ngd_run_windows_job_var_stats(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win,
                                  const uint64_t *block_maps, uint64_t maps_len, const uint64_t *map_off, uint32_t n_rep,
                                  uint64_t block_size, uint64_t tot_sites, uint64_t evol_model, double ci, double *stats,
                                  uint64_t *used) {
  BootCi c{};
  if (int rc = boot_refuse(e, stats, used, (uint64_t)n_rep + 1, ci, tot_sites, evol_model, false, "ngd_run_windows_job_var_stats", c))
    return rc;
  e->bst.ms = 0;
  return windows_host_stats(e, win_lo, win_hi, n_win, block_maps, maps_len, map_off, n_rep, block_size, tot_sites, evol_model, c, false,
                            stats, used, "ngd_run_windows_job_var_stats");
}

int ngd_run_windows_job_var_groups_stats(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win,
                                         const uint64_t *block_maps, uint64_t maps_len, const uint64_t *map_off, uint32_t n_rep,
                                         uint64_t block_size, uint64_t tot_sites, uint64_t evol_model, double ci, double *stats,
                                         uint64_t *used) {
  BootCi c{};
  if (int rc = boot_refuse(e, stats, used, (uint64_t)n_rep + 1, ci, tot_sites, evol_model, true,
                           "ngd_run_windows_job_var_groups_stats", c))
    return rc;
  e->bst.ms = e->grp.ms = 0;
  return windows_host_stats(e, win_lo, win_hi, n_win, block_maps, maps_len, map_off, n_rep, block_size, tot_sites, evol_model, c, true,
                            stats, used, "ngd_run_windows_job_var_groups_stats");
}

int ngd_last_boot_stats_ms(const ngd_engine *e, double *ms) {
  if (!e || !ms) return fail(NGD_E_INVALID, "ngd_last_boot_stats_ms: null argument");
  *ms = e->bst.ms;
  return NGD_OK;
}
