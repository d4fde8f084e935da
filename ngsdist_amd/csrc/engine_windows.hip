// engine_windows.hip -- the windowed calls: their two plans, the fix-up of a batch of windows, the host-memory forms.
#include <functional>
#include <numeric>
#include <set>

#include "ngd_engine.h"

// ---- windows along the genome (ngd_run_windows*) ----
// A window's matrix is what ngd_run() gives on a data set cut down to its sites.  Two plans:
//  * per window: the weighted pass ngd_run_mult() makes with multiplicity 1 on the window's sites and 0 elsewhere (the MFMA
//    kernel walks only the window's k-groups); serves every kernel;
//  * segment slab (MFMA kernel, both operands resident or the one congruent image; the table-driven EM kernel): the segments
//    of a batch of windows -- the elementary intervals between consecutive distinct window boundaries that some window
//    covers -- are the slices of ONE accumulation pass (a slice table: each slice its own k-group range and 0/1 edge masks
//    for the MFMA kernel, its own site range for the EM kernel, which walks single sites and needs neither), their partial
//    results [segment][n_pad][n_pad] are added into the windows by the banded reduction (reduce.hip k_reduce_band), counts
//    under --pairwise_del from per-segment popcounts the same way.  The EM of a (pair, site) runs on that site of the two
//    individuals alone, so a term does not depend on the window it is added to.  A long EM segment is cut into pieces (more
//    slices of the same table) so that the launch has about as many workgroups as a plain pass.

static int windows_check(const ngd_engine *e, const uint64_t *lo, const uint64_t *hi, uint64_t n_win, const char *who) {
  if (!e) return fail(NGD_E_INVALID, std::string(who) + ": null engine");
  if (!lo || !hi || !n_win) return fail(NGD_E_INVALID, std::string(who) + ": no windows");
  if (!e->committed) return fail(NGD_E_INVALID, std::string(who) + ": call ngd_commit() first");
  if (e->cfg.shard_world > 1)
    return fail(NGD_E_INVALID, std::string(who) + ": windows on an engine that owns a share of the pairs are not supported");
  if (n_win >= (1ull << 31)) return fail(NGD_E_INVALID, std::string(who) + ": too many windows in one call");
  for (uint64_t w = 0; w < n_win; w++) {
    if (!(lo[w] < hi[w] && hi[w] <= e->g.n_sites))
      return fail(NGD_E_INVALID, std::string(who) + ": window " + std::to_string(w) + " is empty or reaches past the engine's sites");
    if (w && lo[w] < lo[w - 1]) return fail(NGD_E_INVALID, std::string(who) + ": window starts must not decrease");
  }
  return NGD_OK;
}

// the per-window plan: one weighted pass per window (blocks of gcd(lo, hi) sites, those inside the window drawn once)
static int windows_by_pass(ngd_engine *e, const uint64_t *lo, const uint64_t *hi, uint64_t n_win, double *d_sum,
                           unsigned long long *d_cnt) {
  const uint64_t n_pairs = ngd_n_pairs(e->g.n_ind);
  std::vector<uint32_t> mult;
  for (uint64_t w = 0; w < n_win; w++) {
    const uint64_t B = std::gcd(lo[w], hi[w]), n_blocks = hi[w] / B;
    mult.assign(n_blocks, 0u);
    std::fill(mult.begin() + lo[w] / B, mult.end(), 1u);
    const double fix_ms = e->fix_info.ms;
    const uint64_t fixed = e->fix_info.recomputed;
    int rc = pass_impl(e, mult.data(), 1, n_blocks, B, hi[w] - lo[w], d_sum + w * n_pairs, d_cnt + w * n_pairs, false);
    if (rc) return rc;
    e->win_info.ms += e->timing.ms_total + (e->fix_info.ms - fix_ms);
    e->win_info.fixup_pairs += e->fix_info.recomputed - fixed;
    e->win_info.windows_by_pass++;
  }
  return NGD_OK;
}

// single_image = 2 engines: the pairs the banded reduction noted (a sum below NGD_FIX_MEAN x the window's length in some
// window of the batch; under --pairwise_del x the pair's count there) recomputed with the two-operand arithmetic in every
// window of the batch, tile by tile / pair by pair over the window's sites (fixup.hip).  The stream is idle.
static int windows_fixup(ngd_engine *e, const uint64_t *lo, const uint64_t *hi, uint64_t n_win, double *d_sum) {
  const uint32_t n = *(volatile uint32_t *)e->h_fixcount;
  e->fix_info.flagged += n;
  if (!n) return NGD_OK;
  const bool all = n > e->fix_cap;
  std::vector<ngd_fix_tile> tiles;
  std::vector<unsigned long long> singles;
  if (int rc = fix_collect(e, n, all, tiles, singles)) return rc;
  if (e->opt_fix_work) {  // a caller's budget (NGD_OPT_FIXUP_WORK), in pair-sites over the windows
    double sites = 0;
    for (uint64_t w = 0; w < n_win; w++) sites += (double)(hi[w] - lo[w]);
    if (((double)tiles.size() * NGD_FIX_TILE_COST_X10 / 10.0 + (double)singles.size()) * sites > (double)e->opt_fix_work) {
      e->fix_info.skipped += n;
      return NGD_OK;
    }
  }
  const uint64_t n_pairs = ngd_n_pairs(e->g.n_ind);
  hipEvent_t t0 = e->ev[0], t1 = e->ev[1];  // (the batch's own timings have been read)
  HIPCHK(hipEventRecord(t0, e->st));
  if (!tiles.empty()) {
    int rc = e->d_fixtiles.ensure(e, tiles.size());
    if (!rc) rc = e->d_fixtparts.ensure(e, (uint64_t)NGD_FIX_CAP * 256);
    if (rc) return rc;
    HIPCHK(hipMemcpy(e->d_fixtiles, tiles.data(), tiles.size() * sizeof(ngd_fix_tile), hipMemcpyHostToDevice));
  }
  const uint32_t n1 = (uint32_t)singles.size();
  if (n1) HIPCHK(hipMemcpy(e->d_fixlist, singles.data(), (size_t)n1 * 8, hipMemcpyHostToDevice));
  for (uint64_t w = 0; w < n_win; w++) {
    const uint64_t len = hi[w] - lo[w];
    double *out = d_sum + w * n_pairs;
    if (!tiles.empty()) {  // (the slicing of fixup_pass: a pair's slices depend on the window alone)
      const uint64_t sps = std::max<uint64_t>(4096, (len + NGD_FIX_CAP - 1) / NGD_FIX_CAP);
      const uint64_t n_slices = (len + sps - 1) / sps;
      const size_t per = std::max<size_t>(1, NGD_FIX_CAP / n_slices);
      for (size_t off = 0; off < tiles.size(); off += per) {
        const uint32_t m = (uint32_t)std::min<size_t>(per, tiles.size() - off);
        ngd_launch_fixup_tiles(e->st, e->g, e->sc, e->PA, e->SM, nullptr, e->d_fixtiles + off, m, lo[w], hi[w], sps,
                               (uint32_t)n_slices, 0, e->d_fixtparts);
        ngd_launch_fixup_tiles_finish(e->st, e->g, e->d_fixtiles + off, m, e->d_fixtparts, (uint32_t)n_slices, out);
      }
    }
    if (n1) {
      const uint64_t sps = std::max<uint64_t>(1024, (len + NGD_FIX_CAP - 1) / NGD_FIX_CAP);
      const uint64_t n_slices = (len + sps - 1) / sps;
      const uint32_t per = (uint32_t)std::max<uint64_t>(1, NGD_FIX_CAP / n_slices);
      for (uint32_t off = 0; off < n1; off += per) {
        const uint32_t m = std::min<uint32_t>(per, n1 - off);
        ngd_launch_fixup(e->st, e->g, e->sc, e->PA, e->SM, nullptr, e->d_fixlist + off, m, lo[w], hi[w], sps, (uint32_t)n_slices, 0,
                         e->d_fixparts);
        ngd_launch_fixup_finish(e->st, e->g, e->d_fixlist + off, m, e->d_fixparts, (uint32_t)n_slices, out);
      }
    }
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(t1, e->st));
  HIPCHK(hipStreamSynchronize(e->st));
  float ms = 0;
  hipEventElapsedTime(&ms, t0, t1);
  e->fix_info.ms += ms;
  e->win_info.ms += ms;
  const uint64_t pairs = all ? e->n_owned_pairs : n;
  e->fix_info.recomputed += pairs;
  e->win_info.fixup_pairs += pairs * n_win;
  return NGD_OK;
}

// (the EM kernel's slice-table form exists for every workgroup shape: ngd_config.variant does not matter here)
static bool windows_slab_applies(const ngd_engine *e) {
  return (e->kernel == NGD_KERNEL_MFMA && !e->single_image) || e->kernel == NGD_KERNEL_EM_TABLE;
}

// bytes of one batch of the segment-slab plan: partial results (slices padded to the XCD deal's eights), counts, slice
// weights and tables.  The EM kernel: a plane per segment, counts, tables -- no k-group weights, no padding slices.
static uint64_t windows_batch_bytes(const ngd_engine *e, uint64_t n_seg, uint64_t span, uint64_t n_win) {
  const uint64_t plane = (uint64_t)e->g.n_pad * e->g.n_pad, n_ks = (n_seg + 7) / 8 * 8;
  if (e->kernel == NGD_KERNEL_EM_TABLE)
    return n_seg * plane * 8 + (e->cfg.pairwise_del ? n_seg * plane * 4 : 0) + n_seg * NGD_SEG_STRIDE * 8 + n_win * 16;
  const uint64_t wkg = 3 * span / 4 + n_ks * (3 + NGD_KG_TAIL) + 1 + NGD_KG_TAIL;
  return n_ks * plane * 8 + (e->cfg.pairwise_del ? n_seg * plane * 4 : 0) + wkg * 32 + n_ks * NGD_SEG_STRIDE * 8 + n_win * 16;
}

// the segment-slab plan; *fits = false (nothing launched): some window alone does not fit the budget
static int windows_slab(ngd_engine *e, const uint64_t *lo, const uint64_t *hi, uint64_t n_win, double *d_sum,
                        unsigned long long *d_cnt, uint64_t budget, bool *fits) {
  const ngd_geom &g = e->g;
  const uint64_t n_pairs = ngd_n_pairs(g.n_ind), plane = (uint64_t)g.n_pad * g.n_pad;
  const bool pdel = e->cfg.pairwise_del != 0;
  const bool fix = e->SM != nullptr;
  const bool em = e->kernel == NGD_KERNEL_EM_TABLE;
  *fits = true;
  for (uint64_t w = 0; w < n_win; w++)
    if (windows_batch_bytes(e, 1, hi[w] - lo[w], 1) > budget) {
      *fits = false;
      return NGD_OK;
    }
  // (the windowed call takes the scratch of the bootstrap's per-block partial results: their cache is dropped)
  DevBuf<double> &seg_sums = e->blk.borrow_sums();
  DevBuf<uint32_t> &seg_cnt = e->blk.borrow_counts();
  const ngd_fix_flags ff{e->d_fixlist, e->d_fixcount, e->d_fixseen, e->fix_cap};
  uint64_t batch = 0;
  for (uint64_t a = 0; a < n_win; batch++) {
    // the batch: windows a .. b-1, as many as fit the budget (its segments bounded by its distinct boundaries - 1)
    std::set<uint64_t> bnd;
    uint64_t b = a, hi_max = 0;
    while (b < n_win) {
      const uint64_t n_new = (bnd.count(lo[b]) ? 0 : 1) + (bnd.count(hi[b]) ? 0 : 1);
      const uint64_t n_seg_ub = bnd.size() + n_new - 1, hm = std::max(hi_max, hi[b]);
      if (b > a && (windows_batch_bytes(e, n_seg_ub, hm - lo[a], b + 1 - a) > budget || n_seg_ub >= (1ull << 30))) break;
      bnd.insert(lo[b]);
      bnd.insert(hi[b]);
      hi_max = hm;
      b++;
    }
    const uint64_t nb = b - a;
    const std::vector<uint64_t> x(bnd.begin(), bnd.end());  // boundaries, ascending
    auto at = [&](uint64_t s) { return (uint64_t)(std::lower_bound(x.begin(), x.end(), s) - x.begin()); };
    // interval k = [x[k], x[k + 1]) is a segment if some window of the batch covers it
    std::vector<int64_t> cover(x.size(), 0);
    for (uint64_t w = a; w < b; w++) { cover[at(lo[w])]++; cover[at(hi[w])]--; }
    // EM kernel: an interval's slices are pieces of at most `piece` sites -- the covered sites over the slices of a plain
    // pass, 64 sites or more (ngd_create's bound) -- unless the planes of the pieces would not fit the budget
    uint64_t piece = ~0ull;
    if (em) {
      uint64_t covered = 0, n_cov = 0, n_cut = 0;
      int64_t run = 0;
      for (uint64_t k = 0; k + 1 < x.size(); k++)
        if ((run += cover[k]) > 0) { covered += x[k + 1] - x[k]; n_cov++; }
      piece = std::max<uint64_t>(64, (covered + e->n_ks - 1) / std::max<uint32_t>(1, e->n_ks));
      run = 0;
      for (uint64_t k = 0; k + 1 < x.size(); k++)
        if ((run += cover[k]) > 0) n_cut += (x[k + 1] - x[k] - 1) / piece + 1;
      if (n_cut > n_cov && (windows_batch_bytes(e, n_cut, hi_max - lo[a], nb) > budget || n_cut >= (1ull << 30))) piece = ~0ull;
    }
    std::vector<uint32_t> seg_of(x.size(), 0), seg_end(x.size(), 0);  // interval k = slices [seg_of[k], seg_end[k])
    std::vector<uint64_t> tab;
    uint64_t n_seg = 0, wkg = 0, max_wkg = 0;
    int64_t run = 0;
    for (uint64_t k = 0; k + 1 < x.size(); k++) {
      run += cover[k];
      seg_of[k] = seg_end[k] = (uint32_t)n_seg;
      if (run <= 0) continue;
      if (em) {  // (the k-group entries are the MFMA kernel's: not read)
        const uint64_t len = x[k + 1] - x[k], n_p = len <= piece ? 1 : (len - 1) / piece + 1, per = (len + n_p - 1) / n_p;
        for (uint64_t s = x[k]; s < x[k + 1]; s += per, n_seg++) tab.insert(tab.end(), {0, 0, 0, s, std::min(s + per, x[k + 1])});
      } else {
        const uint64_t kg0 = 3 * x[k] / 4, kg1 = (3 * x[k + 1] + 3) / 4, n_wkg = kg1 - kg0 + 1 + NGD_KG_TAIL;
        tab.insert(tab.end(), {kg0, kg1, wkg, x[k], x[k + 1]});
        wkg += n_wkg;
        max_wkg = std::max(max_wkg, n_wkg);
        n_seg++;
      }
      seg_end[k] = (uint32_t)n_seg;
    }
    // (the XCD deal of accum_mfma.hip; padding slices have no k-group and no sites.  The EM launch needs none.)
    const uint64_t n_ks = em ? n_seg : (n_seg + 7) / 8 * 8;
    for (uint64_t q = n_seg; q < n_ks; q++) tab.insert(tab.end(), {0, 0, wkg, 0, 0});
    const uint64_t w_total = wkg + 1 + NGD_KG_TAIL;
    std::vector<unsigned long long> wt(2 * nb);
    for (uint64_t w = a; w < b; w++) {
      const uint64_t f = seg_of[at(lo[w])], l = seg_end[at(hi[w]) - 1];
      wt[2 * (w - a)] = f | (l << 32);
      wt[2 * (w - a) + 1] = hi[w] - lo[w];
    }
    int rc = seg_sums.ensure(e, n_ks * plane);
    if (!rc && pdel) rc = seg_cnt.ensure(e, n_seg * plane);
    if (!rc && !em) rc = e->blk.wslice.ensure(e, w_total * 4);
    if (!rc) rc = e->d_segtab.ensure(e, tab.size());
    if (!rc) rc = e->d_wintab.ensure(e, wt.size());
    if (rc) return rc;
    HIPCHK(hipEventRecord(e->ev[0], e->st));
    HIPCHK(hipMemcpyAsync(e->d_segtab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, e->st));
    HIPCHK(hipMemcpyAsync(e->d_wintab, wt.data(), wt.size() * 8, hipMemcpyHostToDevice, e->st));
    if (!em) ngd_launch_seg_weights(e->st, e->d_segtab, (uint32_t)n_ks, max_wkg, e->congruent ? e->sc.d : nullptr, e->blk.wslice);
    HIPCHK(hipEventRecord(e->ev[1], e->st));
    if (em)
      ngd_launch_accum_em_table_segs(e->st, g, e->PA, e->sc, e->cfg.pairwise_del, e->em_shape, e->d_tiles64, e->n_tiles64,
                                     (uint32_t)n_seg, e->d_segtab, seg_sums, e->d_emcnt);
    else
      ngd_launch_accum_mfma(e->st, g, e->PA, e->congruent ? e->PA : e->QB, e->blk.wslice, nullptr, e->d_jobs, e->n_wg, e->exact_shapes,
                            e->wg_waves, (uint32_t)n_ks, 0, g.n_kg, 0, 1, seg_sums, e->d_clk, 0, 0, e->d_segtab);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->ev[2], e->st));
    double *bs = d_sum + a * n_pairs;
    unsigned long long *bc = d_cnt + a * n_pairs;
    if (fix) {
      HIPCHK(hipMemsetAsync(e->d_fixcount, 0, sizeof(uint32_t), e->st));
      HIPCHK(hipMemsetAsync(e->d_fixseen, 0, (n_pairs / 32 + 1) * sizeof(uint32_t), e->st));
    }
    ngd_launch_reduce_band(e->st, g, seg_sums, nullptr, e->d_wintab, (uint32_t)nb, e->d_tiles, e->n_tiles, bs,
                           pdel ? nullptr : bc, fix && !pdel ? &ff : nullptr);
    HIPCHK(hipEventRecord(e->ev[3], e->st));
    e->win_info.band_launches++;
    if (pdel) {
      ngd_launch_count_blocks(e->st, g, e->mask, 0, (uint32_t)n_seg, e->d_tiles16, e->n_tiles16, seg_cnt, e->d_segtab);
      ngd_launch_reduce_band(e->st, g, nullptr, seg_cnt, e->d_wintab, (uint32_t)nb, e->d_tiles, e->n_tiles, nullptr, bc, nullptr);
      e->win_info.band_launches++;
      if (fix) ngd_launch_fix_flag(e->st, g, bs, bc, (uint32_t)nb, e->d_tiles, e->n_tiles, ff);
    }
    if (fix) HIPCHK(hipMemcpyAsync(e->h_fixcount, e->d_fixcount, sizeof(uint32_t), hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->ev[4], e->st));
    HIPCHK(hipStreamSynchronize(e->st));  // (tab, wt are host temporaries)
    read_timing(e, hi_max - lo[a], 1, batch > 0);
    if ((rc = mfma_fault(e))) return rc;
    float ms = 0;
    hipEventElapsedTime(&ms, e->ev[0], e->ev[4]);
    e->win_info.ms += ms;
    e->win_info.segments += n_seg;
    e->win_info.slab_bytes = std::max<uint64_t>(e->win_info.slab_bytes, n_ks * plane * 8 + (pdel ? n_seg * plane * 4 : 0));
    e->win_info.batches++;
    if (fix && (rc = windows_fixup(e, lo + a, hi + a, nb, bs))) return rc;
    a = b;
  }
  return NGD_OK;
}

// one call's windows into device memory [n_win][n_pairs]; the plan by NGD_OPT_WIN_PLAN
static int windows_impl(ngd_engine *e, const uint64_t *lo, const uint64_t *hi, uint64_t n_win, double *d_sum,
                        unsigned long long *d_cnt) {
  HIPCHK(hipSetDevice(e->device));
  if (int rc = eager_discard(e)) return rc;
  e->spill_timing = ngd_spill_timing{};
  const bool slab_ok = windows_slab_applies(e);
  if (e->opt_win_plan == 2 && !slab_ok)
    return fail(NGD_E_INVALID, "ngd_run_windows: the segment-slab plan needs the MFMA kernel with both operand images resident "
                               "or the one congruent image, or the table-driven EM kernel (NGD_OPT_WIN_PLAN = 2)");
  bool slab = slab_ok && e->opt_win_plan != 1;
  uint64_t budget = e->opt_win_max_bytes;
  if (slab && !budget) {  // the rule of the bootstrap's per-block partial results
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    budget = (uint64_t)((free_b + e->blk.bytes()) / 100 * 85);
  }
  if (slab && e->opt_win_plan == 0) {
    // auto: the cheaper plan by estimate (the rates partials_impl uses) -- one pass over the sites the
    // windows cover + the banded reduction's reads and writes + allocating a larger slab, against one weighted pass per
    // window (~3/4 of a plain pass over its sites -- [measured] the EM kernel: 0.72, 37 windows of 10 000 sites in 1159 ms at
    // 1000 individuals, the sites before a window loaded and skipped -- + ~0.1 ms of launches and waits)
    uint64_t covered = 0, sum_len = 0, end = 0;
    std::vector<uint64_t> bnd(lo, lo + n_win);
    bnd.insert(bnd.end(), hi, hi + n_win);
    std::sort(bnd.begin(), bnd.end());
    const uint64_t n_bnd = (uint64_t)(std::unique(bnd.begin(), bnd.end()) - bnd.begin());  // (segments < distinct boundaries)
    for (uint64_t w = 0; w < n_win; w++) {
      sum_len += hi[w] - lo[w];
      if (hi[w] > end) { covered += hi[w] - std::max(lo[w], end); end = hi[w]; }
    }
    const bool em = e->kernel == NGD_KERNEL_EM_TABLE;
    // pair-sites per ms: K1m; the table-driven EM kernel's slice-table form ([measured] tools/bench_windows.py, 1000 x 1e5,
    // 160 slices: 224.8 ms -- DESIGN.md section 6; the plain pass's 2.22e8)
    const double rate = em ? 2.22e8 : 1.05e10, np = (double)e->n_owned_pairs;
    const double plane_b = (double)e->g.n_pad * e->g.n_pad * 8;
    const double need = (double)windows_batch_bytes(e, std::min<uint64_t>(n_bnd, budget / (uint64_t)plane_b + 1), end, n_win);
    const double have = (double)e->blk.bytes();
    const double t_slab = np * (double)covered / rate + (double)(n_bnd + 2 * n_win) * np * 8 / 4e9 +
                          (need > have ? (need - have) * 12e-9 : 0.0);
    const double t_pass = np * (double)sum_len / (0.75 * rate) + 0.1 * (double)n_win;
    slab = t_slab < t_pass;
  }
  if (slab) {
    bool fits = true;
    int rc = windows_slab(e, lo, hi, n_win, d_sum, d_cnt, budget, &fits);
    if (rc || fits) return rc;
    if (e->opt_win_plan == 2)
      return fail(NGD_E_NOMEM, "ngd_run_windows: a window does not fit the segment-slab plan's budget (NGD_OPT_WIN_MAX_BYTES)");
  }
  return windows_by_pass(e, lo, hi, n_win, d_sum, d_cnt);
}

int ngd_run_windows_device(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win, void *d_sum,
                           void *d_cnt) {
  if (int rc = windows_check(e, win_lo, win_hi, n_win, "ngd_run_windows_device")) return rc;
  if (!d_sum || !d_cnt) return fail(NGD_E_INVALID, "ngd_run_windows_device: null output");
  e->win_info = ngd_windows_info{};
  e->fix_info = ngd_fixup_info{};
  e->n_batch_valid = 0;
  return windows_impl(e, win_lo, win_hi, n_win, (double *)d_sum, (unsigned long long *)d_cnt);
}

// the host-memory forms: windows in groups whose results fit ~2 GB of the engine's batch buffers; fn(first, count) takes
// each group's results out of d_bsum / d_bcnt
static int windows_chunked(ngd_engine *e, const uint64_t *lo, const uint64_t *hi, uint64_t n_win,
                           const std::function<int(uint64_t, uint64_t)> &fn) {
  const uint64_t n_pairs = ngd_n_pairs(e->g.n_ind);
  const uint64_t per = std::max<uint64_t>(1, std::min<uint64_t>(n_win, (2ull << 30) / (16 * std::max<uint64_t>(1, n_pairs))));
  e->win_info = ngd_windows_info{};
  e->fix_info = ngd_fixup_info{};
  int rc = batch_buffers(e, (uint32_t)per);
  if (rc) return rc;
  for (uint64_t w0 = 0; w0 < n_win; w0 += per) {
    const uint64_t n = std::min(per, n_win - w0);
    if ((rc = windows_impl(e, lo + w0, hi + w0, n, e->d_bsum, e->d_bcnt))) return rc;
    if ((rc = fn(w0, n))) return rc;
  }
  e->n_batch_valid = 0;
  return NGD_OK;
}

int ngd_run_windows(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win, double *sum, uint64_t *cnt) {
  if (int rc = windows_check(e, win_lo, win_hi, n_win, "ngd_run_windows")) return rc;
  HIPCHK(hipSetDevice(e->device));
  const uint64_t n_pairs = ngd_n_pairs(e->g.n_ind);
  return windows_chunked(e, win_lo, win_hi, n_win, [&](uint64_t w0, uint64_t n) {
    int rc = copy_out(e, (uint32_t)n, e->d_bsum, e->d_bcnt, sum ? sum + w0 * n_pairs : nullptr, cnt ? cnt + w0 * n_pairs : nullptr);
    e->n_batch_valid = 0;
    return rc;
  });
}

int ngd_run_windows_dist(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win, uint64_t tot_sites,
                         uint64_t evol_model, double *dist) {
  if (int rc = windows_check(e, win_lo, win_hi, n_win, "ngd_run_windows_dist")) return rc;
  if (!dist) return fail(NGD_E_INVALID, "ngd_run_windows_dist: null argument");
  if (tot_sites && e->cfg.pairwise_del)
    return fail(NGD_E_INVALID, "ngd_run_windows_dist: a total number of sites cannot go with pairwise deletion (parse_args.cpp:209-210)");
  if (evol_model > 2) return fail(NGD_E_MODEL, "ngd_run_windows_dist: evolutionary model not supported (ngsDist.cpp:398-399)");
  HIPCHK(hipSetDevice(e->device));
  const uint64_t n_pairs = ngd_n_pairs(e->g.n_ind);
  std::vector<double> h_sum;
  std::vector<uint64_t> h_cnt;
  return windows_chunked(e, win_lo, win_hi, n_win, [&](uint64_t w0, uint64_t n) {
    h_sum.resize(n * n_pairs);
    h_cnt.resize(n * n_pairs);
    int rc = copy_out(e, (uint32_t)n, e->d_bsum, e->d_bcnt, h_sum.data(), h_cnt.data());
    e->n_batch_valid = 0;
    if (rc) return rc;
    // (the tail of gen_dist() on the host, the host's libm: ngd_finish's bits)
    return ngd_finish(h_sum.data(), h_cnt.data(), n * n_pairs, tot_sites, evol_model, dist + w0 * n_pairs);
  });
}

int ngd_last_windows(const ngd_engine *e, ngd_windows_info *info) {
  if (!e || !info) return fail(NGD_E_INVALID, "ngd_last_windows: null argument");
  *info = e->win_info;
  return NGD_OK;
}
