// engine_groups.hip -- group-mean distance matrices: the engine's grouping (ngd_set_groups), the reduction of device matrices
// to per-group-pair means (group_reduce.hip), and that reduction as a tail (ngd_engine.h) behind the job driver and the
// window driver: the run forms, where n_gp means and counts per matrix cross the link instead of n_pairs sums and counts.
#include "ngd_engine.h"

// what every call that reduces refuses, before anything is launched
static int groups_refuse(const ngd_engine *e, const void *mean, uint64_t tot_sites, uint64_t evol_model, const char *who) {
  const std::string w(who);
  if (!e) return fail(NGD_E_INVALID, w + ": null engine");
  if (!mean) return fail(NGD_E_INVALID, w + ": null output");
  if (!e->grp.n_groups) return fail(NGD_E_INVALID, w + ": no grouping set (ngd_set_groups)");
  return finish_refuse(e, tot_sites, evol_model, w, "no group means");
}

static void groups_clear(ngd_engine *e) {
  auto &g = e->grp;
  g.d_members.release(); g.d_off.release(); g.d_gp_first.release(); g.d_work.release();
  g.d_part_sum.release(); g.d_part_cnt.release(); g.d_mean.release(); g.d_used.release();
  g.d_keep_mean.release(); g.d_keep_used.release();
  g.n_groups = g.n_work = 0;
  g.n_gp = 0;
}

int ngd_set_groups(ngd_engine *e, const int32_t *group_of, uint32_t n_groups) {
  if (!e) return fail(NGD_E_INVALID, "ngd_set_groups: null engine");
  if (!group_of != !n_groups) return fail(NGD_E_INVALID, "ngd_set_groups: a list of groups and their number go together (NULL and 0 clear)");
  HIPCHK(hipSetDevice(e->device));
  if (!group_of) {
    HIPCHK(hipStreamSynchronize(e->st));
    groups_clear(e);
    return NGD_OK;
  }
  const uint64_t n = e->g.n_ind, G = n_groups;
  // the member lists: individuals sorted by group, ascending inside one, and the groups' offsets
  std::vector<uint32_t> off(G + 1, 0), members;
  for (uint64_t i = 0; i < n; i++) {
    if (group_of[i] < -1 || group_of[i] >= (int64_t)G)
      return fail(NGD_E_INVALID, "ngd_set_groups: group_of[" + std::to_string(i) + "] is outside [-1, n_groups)");
    if (group_of[i] >= 0) off[group_of[i] + 1]++;
  }
  for (uint64_t g = 0; g < G; g++) off[g + 1] += off[g];
  members.resize(std::max<uint32_t>(1, off[G]));
  {
    std::vector<uint32_t> at(off.begin(), off.end() - 1);
    for (uint64_t i = 0; i < n; i++)
      if (group_of[i] >= 0) members[at[group_of[i]]++] = (uint32_t)i;
  }
  // the work list, from the group sizes alone: group pair (a, b) in splits of whole rows of about NGD_GROUP_WG_CELLS cells
  // of the rows x columns rectangle (on the diagonal the group by itself: half of its cells exist)
  const uint64_t n_gp = ngd_n_group_pairs(n_groups);
  if (n_gp >= (1ull << 31)) return fail(NGD_E_INVALID, "ngd_set_groups: too many groups (2^31 group pairs and more)");
  std::vector<ngd_group_work> work;
  std::vector<uint32_t> gp_first(n_gp + 1, 0);
  for (uint32_t a = 0; a < n_groups; a++)
    for (uint32_t b = a; b < n_groups; b++) {
      const uint32_t na = off[a + 1] - off[a], nb = off[b + 1] - off[b];
      gp_first[ngd_group_pair_index(n_groups, a, b)] = (uint32_t)work.size();
      if (!na || !nb || (a == b && na < 2)) continue;  // no cell
      const uint32_t rows = std::max<uint32_t>(1, NGD_GROUP_WG_CELLS / nb);
      for (uint32_t r0 = 0; r0 < na; r0 += rows) work.push_back(ngd_group_work{a, b, r0, std::min(na, r0 + rows)});
      if (work.size() >= (1ull << 30)) return fail(NGD_E_INVALID, "ngd_set_groups: too many work items (2^30 and more)");
    }
  gp_first[n_gp] = (uint32_t)work.size();
  // (a work item's rectangle stays below 2^32 cells: rows x nb <= max(NGD_GROUP_WG_CELLS, nb), nb <= n_ind < 2^21)
  HIPCHK(hipStreamSynchronize(e->st));
  groups_clear(e);
  auto &g = e->grp;
  int rc = g.d_members.alloc(e, members.size(), false);
  if (!rc) rc = g.d_off.alloc(e, off.size(), false);
  if (!rc) rc = g.d_gp_first.alloc(e, gp_first.size(), false);
  if (!rc) rc = g.d_work.alloc(e, std::max<size_t>(1, work.size()), false);
  if (rc) { groups_clear(e); return rc; }
  HIPCHK(hipMemcpy(g.d_members, members.data(), members.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(g.d_off, off.data(), off.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(g.d_gp_first, gp_first.data(), gp_first.size() * 4, hipMemcpyHostToDevice));
  if (!work.empty()) HIPCHK(hipMemcpy(g.d_work, work.data(), work.size() * sizeof(ngd_group_work), hipMemcpyHostToDevice));
  g.n_groups = n_groups;
  g.n_work = (uint32_t)work.size();
  g.n_gp = n_gp;
  return NGD_OK;
}

// The matrices in chunks whose partial results and outputs stay small (2^22 entries each) and whose launches fit grid.x; a
// matrix's bits do not depend on the chunk it falls into.  Events 0 and 1 time each chunk's kernels (grp.ms: the entry
// points start it at 0, a windowed call adds up its groups of windows).
// mean == NULL: the chunks' results go one after the other into grp.d_keep_mean / d_keep_used and stay there, nothing is
// copied (the summaries of the means read them: engine_boot_stats.hip).
int groups_reduce(ngd_engine *e, const double *d_sum, const unsigned long long *d_cnt, uint64_t n_mat, uint64_t tot_sites,
                  uint64_t evol_model, double *mean, uint64_t *used) {
  auto &g = e->grp;
  const bool keep = !mean;
  const uint64_t per_mat = std::max<uint64_t>(std::max<uint64_t>(1, g.n_work), g.n_gp);
  const uint64_t chunk = std::max<uint64_t>(1, std::min<uint64_t>(n_mat, (1ull << 22) / per_mat));
  int rc = g.d_part_sum.ensure(e, chunk * std::max<uint64_t>(1, g.n_work));
  if (!rc) rc = g.d_part_cnt.ensure(e, chunk * std::max<uint64_t>(1, g.n_work));
  if (!rc) rc = keep ? g.d_keep_mean.ensure(e, n_mat * g.n_gp) : g.d_mean.ensure(e, chunk * g.n_gp);
  if (!rc) rc = keep ? g.d_keep_used.ensure(e, n_mat * g.n_gp) : g.d_used.ensure(e, chunk * g.n_gp);
  if (rc) return rc;
  const ngd_group_launch l{e->g.n_ind, g.d_members, g.d_off, g.d_work, g.d_gp_first, g.n_work, (uint32_t)g.n_gp};
  const uint64_t n_pairs = ngd_n_pairs(e->g.n_ind);
  for (uint64_t m0 = 0; m0 < n_mat; m0 += chunk) {
    const uint64_t n = std::min(chunk, n_mat - m0);
    HIPCHK(hipEventRecord(e->ev[0], e->st));
    ngd_launch_group_means(e->st, l, d_sum + m0 * n_pairs, d_cnt + m0 * n_pairs, n, tot_sites, (uint32_t)evol_model, g.d_part_sum,
                           g.d_part_cnt, keep ? g.d_keep_mean + m0 * g.n_gp : g.d_mean.get(),
                           keep ? g.d_keep_used + m0 * g.n_gp : g.d_used.get());
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->ev[1], e->st));
    if (!keep) {
      HIPCHK(hipMemcpyAsync(mean + m0 * g.n_gp, g.d_mean, n * g.n_gp * sizeof(double), hipMemcpyDeviceToHost, e->st));
      if (used) HIPCHK(hipMemcpyAsync(used + m0 * g.n_gp, g.d_used, n * g.n_gp * sizeof(uint64_t), hipMemcpyDeviceToHost, e->st));
    }
    HIPCHK(hipStreamSynchronize(e->st));
    float ms = 0;
    hipEventElapsedTime(&ms, e->ev[0], e->ev[1]);
    g.ms += ms;
  }
  return NGD_OK;
}

int ngd_group_means_device(ngd_engine *e, const void *d_sum, const void *d_cnt, uint64_t n_mat, uint64_t tot_sites,
                           uint64_t evol_model, double *mean, uint64_t *used) {
  if (int rc = groups_refuse(e, mean, tot_sites, evol_model, "ngd_group_means_device")) return rc;
  if (!d_sum || !d_cnt || !n_mat) return fail(NGD_E_INVALID, "ngd_group_means_device: null matrices");
  e->grp.ms = 0;
  HIPCHK(hipSetDevice(e->device));
  return groups_reduce(e, (const double *)d_sum, (const unsigned long long *)d_cnt, n_mat, tot_sites, evol_model, mean, used);
}

// the tail of the run forms: n_gp means and counts per matrix cross the link, set after set into mean / used [.][n_mat][n_gp]
static Tail groups_tail(ngd_engine *e, uint64_t tot_sites, uint64_t evol_model, double *mean, uint64_t *used) {
  return [=](uint64_t set0, uint64_t n_set, uint64_t n_mat) {
    const uint64_t at = set0 * n_mat * e->grp.n_gp;
    return groups_reduce(e, e->d_bsum, e->d_bcnt, n_set * n_mat, tot_sites, evol_model, mean + at, used ? used + at : nullptr);
  };
}

int ngd_run_job_groups(ngd_engine *e, const uint64_t *block_maps, uint32_t n_rep, uint64_t n_blocks, uint64_t block_size,
                       uint64_t tot_sites, uint64_t evol_model, double *mean, uint64_t *used) {
  if (int rc = groups_refuse(e, mean, tot_sites, evol_model, "ngd_run_job_groups")) return rc;
  if (n_rep && !block_maps) return fail(NGD_E_INVALID, "ngd_run_job_groups: null argument");
  e->grp.ms = 0;
  return job_tail(e, block_maps, n_rep, n_blocks, block_size, groups_tail(e, tot_sites, evol_model, mean, used));
}

// the windowed forms: `a` as ngd_run_windows_job_var's, or the windows alone (n_rep 0)
static int windows_groups(ngd_engine *e, const WinJobArgs &a, uint64_t tot_sites, uint64_t evol_model, double *mean, uint64_t *used,
                          const char *who) {
  if (int rc = groups_refuse(e, mean, tot_sites, evol_model, who)) return rc;
  e->grp.ms = 0;
  return windows_tail(e, a, false, who, groups_tail(e, tot_sites, evol_model, mean, used));
}

int ngd_run_windows_groups(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win, uint64_t tot_sites,
                           uint64_t evol_model, double *mean, uint64_t *used) {
  return windows_groups(e, WinJobArgs{win_lo, win_hi, n_win, nullptr, 0, nullptr, 0, 0}, tot_sites, evol_model, mean, used,
                        "ngd_run_windows_groups");
}

int ngd_run_windows_job_var_groups(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win,
                                   const uint64_t *block_maps, uint64_t maps_len, const uint64_t *map_off, uint32_t n_rep,
                                   uint64_t block_size, uint64_t tot_sites, uint64_t evol_model, double *mean, uint64_t *used) {
  return windows_groups(e, WinJobArgs{win_lo, win_hi, n_win, block_maps, maps_len, map_off, n_rep, block_size}, tot_sites, evol_model,
                        mean, used, "ngd_run_windows_job_var_groups");
}

int ngd_last_groups_ms(const ngd_engine *e, double *ms) {
  if (!e || !ms) return fail(NGD_E_INVALID, "ngd_last_groups_ms: null argument");
  *ms = e->grp.ms;
  return NGD_OK;
}
