// engine_windows.hip -- the windowed calls: their two plans, the fix-up of a batch of windows, the host-memory forms -- groups
// of windows through the batch buffers, a tail after each: the window driver of the tails --; and the jobs that draw
// bootstrap replicates inside every window.
#include <map>
#include <numeric>

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

// ---- bootstrap replicates inside the windows (ngd_run_windows_job*) ----
// Every window of a call has one length W and draws the same block maps (a run on the cut-down file seeds the generator
// anew): matrix 0 of a window is its full-data matrix, matrix r visits block map[r][b] of the window -- sites
// [lo + map[r][b] q, lo + (map[r][b] + 1) q) -- once for each b < n_blocks = W / q (ngsDist.cpp:217-289, :236, :416-437); the
// tail [lo + n_blocks q, hi) is matrix 0's alone.  The same two plans:
//  * unit slab (where the segment slab applies): the boundaries of a batch are its windows' block boundaries lo + b q and
//    ends hi, the covered intervals between them the slices of ONE accumulation pass -- where q divides the step,
//    overlapping windows share every slice and a block is one slice, else a block is a few consecutive slices.  Matrix 0 of
//    every window comes from the banded reduction as before, the replicates from the banded and weighted one (reduce.hip
//    k_reduce_band_w), counts under --pairwise_del from per-slice popcounts by the integer forms of both;
//  * per window: one run_impl() per window on multiplicity vectors over blocks of gcd(lo, q, hi) sites counted from the
//    engine's site 0 -- vector 0 is 1 on the window's sites, vector r the multiplicities of replicate r.  Serves every
//    kernel, windows that do not fit the budget, and blocks so small that a slice per block loses.
// What a slab plan tells the device -- the batches, their slices and tables -- is host arithmetic of its own: win_plan.h.

// (job: the call draws replicates -- under NGD_OPT_EM_EXACT_WIN those need NGD_OPT_EM_EXACT = 2)
static int windows_check(const ngd_engine *e, const uint64_t *lo, const uint64_t *hi, uint64_t n_win, const char *who, bool job = false) {
  if (!e) return fail(NGD_E_INVALID, std::string(who) + ": null engine");
  if (!lo || !hi || !n_win) return fail(NGD_E_INVALID, std::string(who) + ": no windows");
  if (!e->committed) return fail(NGD_E_INVALID, std::string(who) + ": call ngd_commit() first");
  if (int rc = em_exact_refuse_windows(e, who, job)) return rc;
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
    if (em_exact_win(e)) {
      // NGD_OPT_EM_EXACT_WIN (value 2 of NGD_OPT_EM_EXACT; windows_impl has refused value 1): the weighted pass does not
      // note, so the window goes through the noting plans run_impl has for a multiplicity vector, or fails there
      if (int rc = run_impl(e, nullptr, mult.data(), 1, false, n_blocks, B, d_sum + w * n_pairs, d_cnt + w * n_pairs)) return rc;
      e->win_info.ms += e->timing.ms_total + e->fix_info.ms + e->exact_info.ms;
      em_exact_call_add(e);
      e->win_info.windows_by_pass++;
      continue;
    }
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

// the per-window plan of a job: window w's n_rep + 1 matrices by the replicate loop's plans on multiplicity vectors
static int windows_job_by_pass(ngd_engine *e, const uint64_t *lo, const uint64_t *hi, uint64_t n_win, const WinBoot &bt,
                               double *d_sum, unsigned long long *d_cnt) {
  const uint64_t n_pairs = ngd_n_pairs(e->g.n_ind), n_mat = (uint64_t)bt.n_rep + 1;
  std::vector<uint32_t> mult;
  for (uint64_t w = 0; w < n_win; w++) {
    const uint64_t B = std::gcd(std::gcd(lo[w], bt.q), hi[w]), n_eb = hi[w] / B, per = bt.q / B, first = lo[w] / B;
    mult.assign(n_mat * n_eb, 0u);
    std::fill(mult.begin() + first, mult.begin() + n_eb, 1u);
    for (uint32_t r = 0; r < bt.n_rep; r++)
      for (uint64_t b = 0; b < bt.n_blocks; b++) {
        const uint32_t m = bt.mult[(uint64_t)r * bt.n_blocks + b];
        if (m) std::fill_n(mult.begin() + (r + 1) * n_eb + first + b * per, per, m);
      }
    const ngd_fixup_info fi = e->fix_info;
    int rc = run_impl(e, nullptr, mult.data(), (uint32_t)n_mat, false, n_eb, B, d_sum + w * n_mat * n_pairs,
                      d_cnt + w * n_mat * n_pairs);
    if (rc) return rc;
    e->win_info.ms += e->timing.ms_total + e->fix_info.ms;
    e->win_info.fixup_pairs += e->fix_info.recomputed;
    if (em_exact_win(e)) {  // (run_impl has noted, rechecked and patched this window's matrices: its list joins the call's)
      e->win_info.ms += e->exact_info.ms;
      em_exact_call_add(e);
    }
    // (run_impl reports its own call: the job's report is the sum over its windows)
    e->fix_info.flagged += fi.flagged; e->fix_info.recomputed += fi.recomputed; e->fix_info.skipped += fi.skipped;
    e->fix_info.ms += fi.ms; e->fix_info.by_pass += fi.by_pass;
    e->win_info.windows_by_pass++;
  }
  return NGD_OK;
}

// single_image = 2 engines, the unit slab of a job: the noted pairs' entries of the slab -- every slice of the batch --
// recomputed with the two-operand arithmetic (fixup.hip, the route of the bootstrap's per-block partial results); the
// caller then runs the weighted reductions of the batch again.  The slice table gives each slice its site range: a run of
// consecutive slices of one length that follow each other without a gap is one launch.  The stream is idle.
static int windows_job_fixup(ngd_engine *e, const std::vector<uint64_t> &tab, uint64_t n_seg, double *slab, uint64_t n_out,
                             bool *patched) {
  *patched = false;
  const uint32_t n = *(volatile uint32_t *)e->h_fixcount;
  e->fix_info.flagged += n;
  if (!n) return NGD_OK;
  const bool all = n > e->fix_cap;
  std::vector<ngd_fix_tile> tiles;
  std::vector<unsigned long long> singles;
  if (int rc = fix_collect(e, n, all, tiles, singles)) return rc;
  auto slo = [&](uint64_t k) { return tab[k * NGD_SEG_STRIDE + NGD_SEG_SLO]; };
  auto shi = [&](uint64_t k) { return tab[k * NGD_SEG_STRIDE + NGD_SEG_SHI]; };
  if (e->opt_fix_work) {  // a caller's budget (NGD_OPT_FIXUP_WORK), in pair-sites over the batch's slices
    double sites = 0;
    for (uint64_t k = 0; k < n_seg; k++) sites += (double)(shi(k) - slo(k));
    if (((double)tiles.size() * NGD_FIX_TILE_COST_X10 / 10.0 + (double)singles.size()) * sites > (double)e->opt_fix_work) {
      e->fix_info.skipped += n;
      return NGD_OK;
    }
  }
  const uint64_t plane = (uint64_t)e->g.n_pad * e->g.n_pad;
  hipEvent_t t0 = e->ev[0], t1 = e->ev[1];  // (the batch's own timings have been read)
  HIPCHK(hipEventRecord(t0, e->st));
  if (!tiles.empty()) {
    if (int rc = e->d_fixtiles.ensure(e, tiles.size())) return rc;
    HIPCHK(hipMemcpy(e->d_fixtiles, tiles.data(), tiles.size() * sizeof(ngd_fix_tile), hipMemcpyHostToDevice));
  }
  const uint32_t n1 = (uint32_t)singles.size();
  if (n1) HIPCHK(hipMemcpy(e->d_fixlist, singles.data(), (size_t)n1 * 8, hipMemcpyHostToDevice));
  const uint64_t max_wg = 1ull << 22;  // (workgroups per launch, as fixup_pass)
  for (uint64_t k = 0; k < n_seg;) {
    const uint64_t len = shi(k) - slo(k);
    uint64_t k1 = k + 1;
    while (k1 < n_seg && k1 - k < max_wg && slo(k1) == shi(k1 - 1) && shi(k1) - slo(k1) == len) k1++;
    const uint32_t run = (uint32_t)(k1 - k);
    const size_t per = (size_t)std::max<uint64_t>(1, max_wg / run);
    for (size_t off = 0; off < tiles.size(); off += per)
      ngd_launch_fixup_tiles(e->st, e->g, e->sc, e->PA, e->SM, nullptr, e->d_fixtiles + off,
                             (uint32_t)std::min<size_t>(per, tiles.size() - off), slo(k), shi(k1 - 1), len, run, 1, slab + k * plane);
    for (size_t off = 0; off < n1; off += per)
      ngd_launch_fixup(e->st, e->g, e->sc, e->PA, e->SM, nullptr, e->d_fixlist + off, (uint32_t)std::min<size_t>(per, n1 - off),
                       slo(k), shi(k1 - 1), len, run, 1, slab + k * plane);
    k = k1;
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
  e->win_info.fixup_pairs += pairs * n_out;
  *patched = true;
  return NGD_OK;
}

// single_image = 2 engines: the pairs the banded reduction noted (a sum below NGD_FIX_MEAN x the window's length in some
// window of the batch; under --pairwise_del x the pair's count there) recomputed with the two-operand arithmetic in every
// window of the batch, tile by tile / pair by pair over the window's sites (fixup.hip).  The stream is idle.
// (window w's matrix is matrix w * out_stride of d_sum: a job's matrices 0 lie n_rep + 1 matrices apart)
static int windows_fixup(ngd_engine *e, const uint64_t *lo, const uint64_t *hi, uint64_t n_win, double *d_sum,
                         uint64_t out_stride = 1) {
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
    double *out = d_sum + w * out_stride * n_pairs;
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

// what the planner (win_plan.h) needs of the engine
// (n_rep: the replicates of a job over windows of unequal length, which has no WinBoot)
static win_env windows_env(const ngd_engine *e, const WinBoot *bt, uint32_t n_rep = 0) {
  return win_env{(uint64_t)e->g.n_pad * e->g.n_pad, e->kernel == NGD_KERNEL_EM_TABLE, e->cfg.pairwise_del != 0, e->n_ks,
                 NGD_KG_TAIL, bt ? ngd_reduce_chunk(bt->n_rep) : n_rep ? ngd_reduce_chunk(n_rep) : 1, e->congruent};
}

// a job's weights, the same for every window: Wt[b][r] (zero padded to whole chunks of replicates), as integers for the counts
static int windows_job_weights(ngd_engine *e, const WinBoot &bt, uint32_t stride) {
  std::vector<double> Wt(bt.n_blocks * stride, 0.0);
  for (uint32_t r = 0; r < bt.n_rep; r++)
    for (uint64_t b = 0; b < bt.n_blocks; b++) Wt[b * stride + r] = (double)bt.mult[(uint64_t)r * bt.n_blocks + b];
  int rc = e->d_W.ensure(e, Wt.size());
  if (rc) return rc;
  HIPCHK(hipMemcpy(e->d_W, Wt.data(), Wt.size() * 8, hipMemcpyHostToDevice));
  if (!e->cfg.pairwise_del) return NGD_OK;
  std::vector<uint32_t> M(Wt.size());
  for (size_t k = 0; k < M.size(); k++) M[k] = (uint32_t)Wt[k];
  if ((rc = e->d_M.ensure(e, M.size()))) return rc;
  HIPCHK(hipMemcpy(e->d_M, M.data(), M.size() * 4, hipMemcpyHostToDevice));
  return NGD_OK;
}

// What every batch of one slab plan shares on the device: the plan of the batch at hand, the scratch its slices' partial
// results take, the output's matrices per window; a job: the weights' stride and the replicates of bt.  The batch's
// matrices go to bs / bc, which the helpers take beside it.
struct SlabCall {
  const win_batch &p;
  const WinBoot *bt;
  DevBuf<double> &seg_sums;
  DevBuf<uint32_t> &seg_cnt;
  ngd_fix_flags ff;
  uint32_t n_mat, stride;
  // a job over windows of unequal length (bt == NULL then): p is this batch's plan too, with its descriptors and classes
  const WinBootVar *bv = nullptr;
  const win_batch_var *pv = nullptr;
  uint32_t nb() const { return (uint32_t)(p.b - p.a); }
};

// the batch's tables to the device and its ONE accumulation pass: events 0 .. 2
static int slab_accumulate(ngd_engine *e, const SlabCall &B) {
  const win_batch &p = B.p;
  const bool em = e->kernel == NGD_KERNEL_EM_TABLE;
  const uint64_t plane = (uint64_t)e->g.n_pad * e->g.n_pad;
  int rc = B.seg_sums.ensure(e, p.n_ks * plane);
  if (!rc && (B.bt || B.bv)) rc = e->d_winblk.ensure(e, p.blk.size());
  if (!rc && B.bv) rc = e->d_windesc.ensure(e, B.pv->desc.size());
  if (!rc && e->cfg.pairwise_del) rc = B.seg_cnt.ensure(e, p.n_seg * plane);
  if (!rc && !em) rc = e->blk.wslice.ensure(e, p.w_total * 4);
  if (!rc) rc = e->d_segtab.ensure(e, p.tab.size());
  if (!rc) rc = e->d_wintab.ensure(e, p.wt.size());
  if (rc) return rc;
  const bool note = em && em_exact_win(e);  // NGD_OPT_EM_EXACT_WIN: the noting slice-table form, into e->d_note
  if (note && (rc = em_exact_begin(e))) return rc;
  HIPCHK(hipEventRecord(e->ev[0], e->st));
  HIPCHK(hipMemcpyAsync(e->d_segtab, p.tab.data(), p.tab.size() * 8, hipMemcpyHostToDevice, e->st));
  HIPCHK(hipMemcpyAsync(e->d_wintab, p.wt.data(), p.wt.size() * 8, hipMemcpyHostToDevice, e->st));
  if (B.bt || B.bv) HIPCHK(hipMemcpyAsync(e->d_winblk, p.blk.data(), p.blk.size() * 4, hipMemcpyHostToDevice, e->st));
  if (B.bv) HIPCHK(hipMemcpyAsync(e->d_windesc, B.pv->desc.data(), B.pv->desc.size() * 8, hipMemcpyHostToDevice, e->st));
  if (!em) ngd_launch_seg_weights(e->st, e->d_segtab, (uint32_t)p.n_ks, p.max_wkg, e->congruent ? e->sc.d : nullptr, e->blk.wslice);
  HIPCHK(hipEventRecord(e->ev[1], e->st));
  if (note)
    ngd_launch_accum_em_table_segs_note(e->st, emt_common(e), (uint32_t)p.n_seg, e->d_segtab, B.seg_sums, e->d_note);
  else if (em)
    ngd_launch_accum_em_table_segs(e->st, emt_common(e), (uint32_t)p.n_seg, e->d_segtab, B.seg_sums);
  else {
    ngd_mfma_launch l;
    l.PA = e->PA; l.QB = e->congruent ? e->PA : e->QB;
    // every slice's own weights, at the offset its entry of the table names, with its k-group range
    l.d_wk = e->blk.wslice; l.w_slice_stride = 1; l.d_seg = e->d_segtab;
    l.n_ks = (uint32_t)p.n_ks; l.n_kg_eff = e->g.n_kg;
    l.slab = B.seg_sums;
    ngd_launch_accum_mfma(e->st, mfma_engine(e), l);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(e->ev[2], e->st));
  return NGD_OK;
}

// the slices' sums into the windows' matrices: the banded reduction; a job's replicates by the banded and weighted one
// (a job: window w's full-data matrix is matrix w (n_rep + 1) of the output, its replicates follow it; matrix 0 is NOT
// reduced from these slices -- windows_job_slab has filled it from the windows' own segments).  first: the launch that
// also writes the counts without --pairwise_del and notes the pairs that want the fix-up
static void slab_reduce_sums(ngd_engine *e, const SlabCall &B, double *bs, unsigned long long *bc, bool first) {
  const bool pdel = e->cfg.pairwise_del != 0;
  const uint64_t n_pairs = ngd_n_pairs(e->g.n_ind);
  const ngd_fix_flags *ff = first && e->SM && !pdel ? &B.ff : nullptr;
  if (B.bv)  // (count and threshold are the window's own: the sites its replicates visit, from its descriptor)
    ngd_launch_reduce_band_wv(e->st, e->g, B.seg_sums, nullptr, e->d_winblk, e->d_windesc, B.nb(), e->d_W.get(), B.stride, B.bv->n_rep,
                              B.n_mat, e->d_tiles, e->n_tiles, bs + n_pairs, first && !pdel ? bc + n_pairs : nullptr, ff);
  else if (!B.bt)
    ngd_launch_reduce_band(e->st, e->g, B.seg_sums, nullptr, e->d_wintab, B.nb(), e->d_tiles, e->n_tiles, bs,
                           first && !pdel ? bc : nullptr, ff, B.n_mat);
  else {
    const uint64_t n_vis = B.bt->n_blocks * B.bt->q;  // sites a replicate visits
    ngd_launch_reduce_band_w(e->st, e->g, B.seg_sums, nullptr, e->d_winblk, B.nb(), (uint32_t)B.bt->n_blocks, e->d_W.get(), B.stride,
                             B.bt->n_rep, B.n_mat, e->d_tiles, e->n_tiles, bs + n_pairs, first && !pdel ? bc + n_pairs : nullptr,
                             n_vis, ff, NGD_FIX_MEAN * (double)n_vis);
  }
  e->win_info.band_launches++;
}

// --pairwise_del: the slices' popcounts into the windows' counts by the integer forms of both reductions; then the pairs
// that want the fix-up noted from sums and counts
static void slab_counts(ngd_engine *e, const SlabCall &B, double *bs, unsigned long long *bc) {
  const uint64_t n_pairs = ngd_n_pairs(e->g.n_ind);
  ngd_launch_count_blocks(e->st, e->g, e->mask, 0, (uint32_t)B.p.n_seg, e->d_tiles16, e->n_tiles16, B.seg_cnt, e->d_segtab);
  if (B.bv)
    ngd_launch_reduce_band_wv(e->st, e->g, nullptr, B.seg_cnt, e->d_winblk, e->d_windesc, B.nb(), e->d_M.get(), B.stride, B.bv->n_rep,
                              B.n_mat, e->d_tiles, e->n_tiles, nullptr, bc + n_pairs, nullptr);
  else if (!B.bt)
    ngd_launch_reduce_band(e->st, e->g, nullptr, B.seg_cnt, e->d_wintab, B.nb(), e->d_tiles, e->n_tiles, nullptr, bc, nullptr, B.n_mat);
  else
    ngd_launch_reduce_band_w(e->st, e->g, nullptr, B.seg_cnt, e->d_winblk, B.nb(), (uint32_t)B.bt->n_blocks, e->d_M.get(), B.stride,
                             B.bt->n_rep, B.n_mat, e->d_tiles, e->n_tiles, nullptr, bc + n_pairs, 0, nullptr, 0.0);
  e->win_info.band_launches++;
  if (!e->SM) return;
  // (a job: over every matrix of the batch -- the windows' matrices 0 are in place already and hold their final sums)
  if (B.bt || B.bv) ngd_launch_fix_flag(e->st, e->g, bs, bc, B.nb() * B.n_mat, e->d_tiles, e->n_tiles, B.ff);
  else ngd_launch_fix_flag(e->st, e->g, bs, bc, B.nb(), e->d_tiles, e->n_tiles, B.ff, B.n_mat);
}

// one batch: its accumulation pass, its reductions and counts, and the wait for them (the plan's tables are host memory)
static int slab_batch(ngd_engine *e, const SlabCall &B, double *bs, unsigned long long *bc, uint64_t span, bool add_timing) {
  const bool pdel = e->cfg.pairwise_del != 0, fix = e->SM != nullptr;
  const uint64_t n_pairs = ngd_n_pairs(e->g.n_ind);
  if (int rc = slab_accumulate(e, B)) return rc;
  if (fix) {
    HIPCHK(hipMemsetAsync(e->d_fixcount, 0, sizeof(uint32_t), e->st));
    HIPCHK(hipMemsetAsync(e->d_fixseen, 0, (n_pairs / 32 + 1) * sizeof(uint32_t), e->st));
  }
  slab_reduce_sums(e, B, bs, bc, true);
  HIPCHK(hipEventRecord(e->ev[3], e->st));
  if (pdel) slab_counts(e, B, bs, bc);
  if (fix) HIPCHK(hipMemcpyAsync(e->h_fixcount, e->d_fixcount, sizeof(uint32_t), hipMemcpyDeviceToHost, e->st));
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(e->ev[4], e->st));
  HIPCHK(hipStreamSynchronize(e->st));
  read_timing(e, span, 1, add_timing);
  if (int rc = mfma_fault(e)) return rc;
  float ms = 0;
  hipEventElapsedTime(&ms, e->ev[0], e->ev[4]);
  e->win_info.ms += ms;
  return NGD_OK;
}

// the segment-slab plan, batch by batch (win_plan.h); *fits = false (nothing launched): some window alone does not fit the budget
// bt != NULL: the unit slab of a job, outputs [n_win][n_rep + 1][n_pairs] -- the replicates alone, matrix 0 is not written;
// else window w's matrix is matrix w * out_stride of the outputs (a job's matrices 0: windows_job_slab)
static int windows_slab(ngd_engine *e, const uint64_t *lo, const uint64_t *hi, uint64_t n_win, double *d_sum,
                        unsigned long long *d_cnt, uint64_t budget, bool *fits, const WinBoot *bt = nullptr,
                        uint64_t out_stride = 1) {
  const win_env v = windows_env(e, bt);
  if (!(*fits = win_each_fits(v, lo, hi, n_win, bt, budget))) return NGD_OK;
  const uint64_t n_pairs = ngd_n_pairs(e->g.n_ind);
  const bool pdel = v.pdel, fix = e->SM != nullptr;
  const uint64_t n_mat = bt ? (uint64_t)bt->n_rep + 1 : out_stride;  // matrices of the output per window
  const uint32_t stride = bt ? win_weight_stride(v, *bt) : 0;
  int rc = bt ? windows_job_weights(e, *bt, stride) : NGD_OK;
  if (rc) return rc;
  // (the windowed call takes the scratch of the bootstrap's per-block partial results: their cache is dropped)
  win_batch p;
  const SlabCall B{p, bt, e->blk.borrow_sums(), e->blk.borrow_counts(),
                   ngd_fix_flags{e->d_fixlist, e->d_fixcount, e->d_fixseen, e->fix_cap}, (uint32_t)n_mat, stride};
  uint64_t batch = 0;
  for (uint64_t a = 0; a < n_win; a = p.b, batch++) {
    win_plan_batch(v, lo, hi, n_win, a, budget, bt, p);
    double *bs = d_sum + a * n_mat * n_pairs;
    unsigned long long *bc = d_cnt + a * n_mat * n_pairs;
    if ((rc = slab_batch(e, B, bs, bc, p.hi_max - lo[a], batch > 0))) return rc;
    if (em_exact_win(e)) {
      // NGD_OPT_EM_EXACT_WIN: the accumulation has noted; the batch's sums take the host's verdict here, behind the reductions
      // and before they can leave the engine.  A list that was too short has grown to the count: the batch runs once more
      const ngd_note_win nw = bt ? ngd_note_win{nullptr, B.nb(), bt->n_rep, 1, (uint32_t)n_mat, e->d_W.get(), stride, bt->n_blocks, bt->q}
                                 : ngd_note_win{nullptr, B.nb(), 1, 0, (uint32_t)n_mat, nullptr, 0, 0, 0};
      bool again = false;
      if ((rc = em_exact_finish_win(e, bs, lo + a, hi + a, nw, &again))) return rc;
      if (again) {
        if ((rc = slab_batch(e, B, bs, bc, p.hi_max - lo[a], true))) return rc;
        if ((rc = em_exact_finish_win(e, bs, lo + a, hi + a, nw, &again))) return rc;
        if (again) return fail(NGD_E_HIP, "NGD_OPT_EM_EXACT: internal -- the second pass noted more than the first counted");
        e->exact_info.passes = 2;
      }
      e->win_info.ms += e->exact_info.ms;
      em_exact_call_add(e);
    }
    e->win_info.segments += p.n_seg;
    e->win_info.slab_bytes = std::max<uint64_t>(e->win_info.slab_bytes, (p.n_ks * 8 + (pdel ? p.n_seg * 4 : 0)) * v.plane);
    e->win_info.batches++;
    if (fix && !bt && (rc = windows_fixup(e, lo + a, hi + a, B.nb(), bs, n_mat))) return rc;
    if (fix && bt) {  // the noted pairs' slab entries exactly, then the weighted reductions of the batch again
      bool patched = false;
      if ((rc = windows_job_fixup(e, p.tab, p.n_seg, B.seg_sums, B.nb() * n_mat, &patched))) return rc;
      if (patched) {  // (timed like the recomputation: part of the fix-up and of the call)
        HIPCHK(hipEventRecord(e->ev[0], e->st));
        slab_reduce_sums(e, B, bs, bc, false);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(e->ev[1], e->st));
        HIPCHK(hipStreamSynchronize(e->st));
        float ms2 = 0;
        hipEventElapsedTime(&ms2, e->ev[0], e->ev[1]);
        e->fix_info.ms += ms2;
        e->win_info.ms += ms2;
      }
    }
  }
  return NGD_OK;
}

// The slab plan of a job.  Matrix 0 of every window must carry ngd_run_windows_device()'s bits (NGD_OPT_WIN_PLAN = 2), and the
// unit slab's finer slices would add the same terms in another order: so matrix 0 comes from the windows' OWN segments -- the
// segment-slab plan exactly as ngd_run_windows runs it on this list of windows, batches and fix-up included, written to its
// places [w][0] of the output -- and only the replicates from the unit slab.  The cost is stated where the plans are
// compared (windows_impl): a second pass over the covered sites and the banded reduction.
static int windows_job_slab(ngd_engine *e, const uint64_t *lo, const uint64_t *hi, uint64_t n_win, double *d_sum,
                            unsigned long long *d_cnt, uint64_t budget, bool *fits, const WinBoot *bt) {
  // (before anything is launched: the unit slab's own test)
  if (!(*fits = win_each_fits(windows_env(e, bt), lo, hi, n_win, bt, budget))) return NGD_OK;
  bool fits0 = true;
  if (int rc = windows_slab(e, lo, hi, n_win, d_sum, d_cnt, budget, &fits0, nullptr, (uint64_t)bt->n_rep + 1)) return rc;
  if (!fits0) return fail(NGD_E_NOMEM, "ngd_run_windows_job: internal -- a window fits the unit slab and not its own segment");
  return windows_slab(e, lo, hi, n_win, d_sum, d_cnt, budget, fits, bt);
}

// ---- jobs over windows of unequal length (ngd_run_windows_job_var*) ----
// Window w has its own n_blocks_w = (hi - lo) / q and the maps of its class (WinBootVar, win_plan.h).  The two plans again:
// per window, one job of one window each; and the unit slab, whose replicates come from the descriptor form of the banded
// and weighted reduction (reduce.hip k_reduce_band_wv) -- the slices, the pass, matrix 0 and the fix-up are the job's.

// the weight tables of the classes one batch holds, one after the other: Wt[row][r], as integers for the counts
static int windows_var_weights(ngd_engine *e, const WinBootVar &bv, const win_batch_var &p, uint32_t stride) {
  if (!p.wt_rows) return NGD_OK;
  std::vector<double> Wt(p.wt_rows * stride, 0.0);
  for (uint32_t c : p.cls_list) {
    const uint64_t n_blocks = bv.cls_blocks[c];
    const uint32_t *mult = bv.mult + bv.cls_mult[c];
    for (uint32_t r = 0; r < bv.n_rep; r++)
      for (uint64_t b = 0; b < n_blocks; b++) Wt[(p.cls_row[c] + b) * stride + r] = (double)mult[(uint64_t)r * n_blocks + b];
  }
  int rc = e->d_W.ensure(e, Wt.size());
  if (rc) return rc;
  HIPCHK(hipMemcpy(e->d_W, Wt.data(), Wt.size() * 8, hipMemcpyHostToDevice));
  if (!e->cfg.pairwise_del) return NGD_OK;
  std::vector<uint32_t> M(Wt.size());
  for (size_t k = 0; k < M.size(); k++) M[k] = (uint32_t)Wt[k];
  if ((rc = e->d_M.ensure(e, M.size()))) return rc;
  HIPCHK(hipMemcpy(e->d_M, M.data(), M.size() * 4, hipMemcpyHostToDevice));
  return NGD_OK;
}

// the unit slab, batch by batch: the replicates alone into [n_win][n_rep + 1][n_pairs] (matrix 0: windows_job_slab_var)
static int windows_slab_var(ngd_engine *e, const uint64_t *lo, const uint64_t *hi, uint64_t n_win, double *d_sum,
                            unsigned long long *d_cnt, uint64_t budget, const WinBootVar &bv) {
  const win_env v = windows_env(e, nullptr, bv.n_rep);
  const uint64_t n_pairs = ngd_n_pairs(e->g.n_ind), n_mat = (uint64_t)bv.n_rep + 1;
  const uint32_t stride = win_weight_stride_var(v, bv.n_rep);
  win_batch_var p;
  std::vector<uint64_t> all;  // (the call's boundaries: a batch's slices do not depend on where the budget cuts the call)
  win_call_boundaries_var(lo, hi, n_win, bv.q, all);
  const SlabCall B{p, nullptr, e->blk.borrow_sums(), e->blk.borrow_counts(),
                   ngd_fix_flags{e->d_fixlist, e->d_fixcount, e->d_fixseen, e->fix_cap}, (uint32_t)n_mat, stride, &bv, &p};
  uint64_t batch = 0;
  for (uint64_t a = 0; a < n_win; a = p.b, batch++) {
    win_plan_batch_var(v, lo, hi, n_win, a, budget, bv, all, p);
    double *bs = d_sum + a * n_mat * n_pairs;
    unsigned long long *bc = d_cnt + a * n_mat * n_pairs;
    int rc = windows_var_weights(e, bv, p, stride);
    if (!rc) rc = slab_batch(e, B, bs, bc, p.hi_max - lo[a], batch > 0);
    if (rc) return rc;
    e->win_info.segments += p.n_seg;
    e->win_info.slab_bytes = std::max<uint64_t>(e->win_info.slab_bytes, (p.n_ks * 8 + (v.pdel ? p.n_seg * 4 : 0)) * v.plane);
    e->win_info.batches++;
    if (!e->SM) continue;
    // one-image engines: the noted pairs' slab entries exactly, then the weighted reductions of the batch again
    bool patched = false;
    if ((rc = windows_job_fixup(e, p.tab, p.n_seg, B.seg_sums, B.nb() * n_mat, &patched))) return rc;
    if (patched) {
      HIPCHK(hipEventRecord(e->ev[0], e->st));
      slab_reduce_sums(e, B, bs, bc, false);
      HIPCHK(hipGetLastError());
      HIPCHK(hipEventRecord(e->ev[1], e->st));
      HIPCHK(hipStreamSynchronize(e->st));
      float ms2 = 0;
      hipEventElapsedTime(&ms2, e->ev[0], e->ev[1]);
      e->fix_info.ms += ms2;
      e->win_info.ms += ms2;
    }
  }
  return NGD_OK;
}

// the slab plan: matrix 0 of every window from the windows' own segments (as windows_job_slab), the replicates from the unit slab
static int windows_job_slab_var(ngd_engine *e, const uint64_t *lo, const uint64_t *hi, uint64_t n_win, double *d_sum,
                                unsigned long long *d_cnt, uint64_t budget, bool *fits, const WinBootVar &bv) {
  if (!(*fits = win_each_fits_var(windows_env(e, nullptr, bv.n_rep), lo, hi, n_win, bv, budget))) return NGD_OK;
  bool fits0 = true;
  if (int rc = windows_slab(e, lo, hi, n_win, d_sum, d_cnt, budget, &fits0, nullptr, (uint64_t)bv.n_rep + 1)) return rc;
  if (!fits0) return fail(NGD_E_NOMEM, "ngd_run_windows_job_var: internal -- a window fits the unit slab and not its own segment");
  return windows_slab_var(e, lo, hi, n_win, d_sum, d_cnt, budget, bv);
}

// the per-window plan: the job of one window, with that window's maps; a window shorter than one block: its matrix 0 by a
// pass of its own, its replicates sum 0 and count 0 (ngsDist.cpp:236)
static int windows_job_by_pass_var(ngd_engine *e, const uint64_t *lo, const uint64_t *hi, uint64_t n_win, const WinBootVar &bv,
                                   double *d_sum, unsigned long long *d_cnt) {
  const uint64_t n_pairs = ngd_n_pairs(e->g.n_ind), n_mat = (uint64_t)bv.n_rep + 1;
  for (uint64_t w = 0; w < n_win; w++) {
    double *ws = d_sum + w * n_mat * n_pairs;
    unsigned long long *wc = d_cnt + w * n_mat * n_pairs;
    if (bv.cls[w] == NGD_WIN_NO_CLASS) {
      if (int rc = windows_by_pass(e, lo + w, hi + w, 1, ws, wc)) return rc;
      HIPCHK(hipMemsetAsync(ws + n_pairs, 0, (size_t)bv.n_rep * n_pairs * 8, e->st));
      HIPCHK(hipMemsetAsync(wc + n_pairs, 0, (size_t)bv.n_rep * n_pairs * 8, e->st));
      HIPCHK(hipStreamSynchronize(e->st));
      continue;
    }
    const WinBoot bt{bv.n_rep, bv.cls_blocks[bv.cls[w]], bv.q, bv.mult + bv.cls_mult[bv.cls[w]]};
    if (int rc = windows_job_by_pass(e, lo + w, hi + w, 1, bt, ws, wc)) return rc;
  }
  return NGD_OK;
}

// one call's windows into device memory [n_win][n_pairs] (a job, bt or bv != NULL: [n_win][n_rep + 1][n_pairs]); the plan by
// NGD_OPT_WIN_PLAN
static int windows_impl(ngd_engine *e, const uint64_t *lo, const uint64_t *hi, uint64_t n_win, double *d_sum,
                        unsigned long long *d_cnt, const WinBoot *bt = nullptr, const WinBootVar *bv = nullptr) {
  HIPCHK(hipSetDevice(e->device));
  if (int rc = eager_discard(e)) return rc;
  e->spill_timing = ngd_spill_timing{};
  const bool slab_ok = windows_slab_applies(e);
  if (e->opt_win_plan == 2 && !slab_ok)
    return fail(NGD_E_INVALID, "ngd_run_windows: the segment-slab plan needs the MFMA kernel with both operand images resident "
                               "or the one congruent image, or the table-driven EM kernel (NGD_OPT_WIN_PLAN = 2)");
  // NGD_OPT_EM_EXACT_WIN under NGD_OPT_EM_EXACT = 1: the segment slab or nothing (the per-window plan's weighted pass does not
  // note, and the plans that note for a multiplicity vector belong to value 2)
  const bool slab_only = em_exact_win(e) && !e->opt_em_exact_boot;
  if (slab_only && (e->opt_win_plan == 1 || !slab_ok))
    return fail(NGD_E_INVALID, "ngd_run_windows: NGD_OPT_EM_EXACT = 1 with NGD_OPT_EM_EXACT_WIN serves the windows by the segment-slab plan "
                               "only, and NGD_OPT_WIN_PLAN = 1 asks for the per-window plan (that one needs NGD_OPT_EM_EXACT = 2); "
                               "nothing was computed");
  bool slab = slab_ok && e->opt_win_plan != 1;
  uint64_t budget = e->opt_win_max_bytes;
  if (slab && !budget) {  // the rule of the bootstrap's per-block partial results
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    budget = (uint64_t)((free_b + e->blk.bytes()) / 100 * 85);
  }
  if (slab && e->opt_win_plan == 0 && !slab_only) {
    // auto: the cheaper plan by estimate (the rates partials_impl uses) -- one pass over the sites the
    // windows cover + the banded reduction's reads and writes + allocating a larger slab, against one weighted pass per
    // window (~3/4 of a plain pass over its sites -- [measured] the EM kernel: 0.72, 37 windows of 10 000 sites in 1159 ms at
    // 1000 individuals, the sites before a window loaded and skipped -- + ~0.1 ms of launches and waits)
    uint64_t covered = 0, sum_len = 0, end = 0;
    std::vector<uint64_t> bnd, wb;  // (every window's boundaries: its ends, and in a job the starts of its blocks)
    uint64_t blk_entries = 0;       // (a job over windows of unequal length: its rows of block starts)
    for (uint64_t w = 0; w < n_win; w++) {
      const WinBoot one{0, bv ? (hi[w] - lo[w]) / bv->q : 0, bv ? bv->q : 0, nullptr};
      blk_entries += one.n_blocks + 1;
      win_boundaries(lo[w], hi[w], bv ? &one : bt, wb);
      bnd.insert(bnd.end(), wb.begin(), wb.end());
    }
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
    const uint64_t seg_ub = std::min<uint64_t>(n_bnd, budget / (uint64_t)plane_b + 1);
    const double need = bv ? (double)win_batch_bytes_var(windows_env(e, nullptr, bv->n_rep), seg_ub, end, n_win, blk_entries, 0, bv->n_rep)
                           : (double)win_batch_bytes(windows_env(e, bt), seg_ub, end, n_win, bt);
    const double have = (double)e->blk.bytes();
    if (bv) {
      // A job over windows of unequal length.  [predicted -- the legs of the equal-length job below with every window's own
      // length and blocks.  tools/bench_windows_boot.py --bp (1000 x 1e5, 96 windows of ~990 sites,
      // 100 replicates) ranks the plans as this estimate does -- unit slab 42 .. 351 ms, per window 2.6 .. 3.7 s -- but
      // gives no rates yet; where blocks of 10 sites of overlapping windows interleave, a slab per window beats both]
      const double n_mat = (double)bv->n_rep + 1, chunks = (double)((bv->n_rep + 31) / 32);
      const double t_slab = np * (2.0 * (double)covered + (em ? 0.0 : 12.0) * (double)n_bnd) / rate + (double)n_bnd * plane_b / 4e9 +
                            (double)(4 * n_win) * np * 8 / 4e9 +
                            ((double)n_bnd + chunks * (double)blk_entries + (double)n_win * 2 * n_mat) * np * 8 / 4e9 +
                            (need > have ? (need - have) * 12e-9 : 0.0);
      double t_pass = 0;
      for (uint64_t w = 0; w < n_win; w++) {
        const uint64_t B = std::gcd(std::gcd(lo[w], bv->q), hi[w]);
        const double by_matrix = n_mat * np * (double)(hi[w] - lo[w]) / (0.75 * rate);
        const double shared = np * (double)hi[w] / rate * (em ? 1.1 : 1.0) + (em ? 0.0 : chunks * (double)(hi[w] / B) * np * 8 / 4e9);
        t_pass += ((em || B % 4 == 0) ? std::min(by_matrix, shared) : by_matrix) + 0.1 + n_mat * np * 16 / 4e9;
      }
      slab = t_slab < t_pass;
    } else if (!bt) {
      const double t_slab = np * (double)covered / rate + (double)(n_bnd + 2 * n_win) * np * 8 / 4e9 +
                            (need > have ? (need - have) * 12e-9 : 0.0);
      const double t_pass = np * (double)sum_len / (0.75 * rate) + 0.1 * (double)n_win;
      slab = t_slab < t_pass;
    } else {
      // A job.  [predicted -- nothing here has been measured on a device yet; tools/bench_windows_boot.py gives the legs]
      //  * unit slab: matrix 0 of every window by the plain segment slab first (its bits are ngd_run_windows()': one pass
      //    over the covered sites + the banded reduction), then the pass over the covered sites, every slice with the start-up of a short slice (the MFMA kernel's
      //    operand pipeline runs NGD_KG_TAIL k-groups ahead: ~12 sites' worth; the EM kernel walks single sites) and a
      //    plane of the slab to write; the banded reduction as above; the weighted one reads a window's slices once per
      //    chunk of replicates and both write (n_rep + 1) matrices of sums and counts per window;
      //  * per window: run_impl() on multiplicity vectors over blocks of gcd(lo, q, hi) sites from site 0 -- the MFMA
      //    kernel by per-block partial results of the sites [0, hi) where its blocks are whole k-groups, else ~3/4 of a
      //    pass over the window per matrix; the EM kernel by ONE spilled-terms pass over [0, hi) (1.1 plain passes).
      const double n_mat = (double)bt->n_rep + 1, chunks = (double)((bt->n_rep + 31) / 32);
      const double per_win = covered ? (double)n_bnd * (double)(hi[0] - lo[0]) / (double)covered : 0.0;  // slices of a window
      const double t_slab = np * (2.0 * (double)covered + (em ? 0.0 : 12.0) * (double)n_bnd) / rate + (double)n_bnd * plane_b / 4e9 +
                            (double)(2 * n_win + 2 * n_win) * np * 8 / 4e9 +
                            ((double)n_bnd + (double)n_win * (chunks * per_win + 2 * n_mat)) * np * 8 / 4e9 +
                            (need > have ? (need - have) * 12e-9 : 0.0);
      double t_pass = 0;
      for (uint64_t w = 0; w < n_win; w++) {
        const uint64_t B = std::gcd(std::gcd(lo[w], bt->q), hi[w]);
        const double by_matrix = n_mat * np * (double)(hi[w] - lo[w]) / (0.75 * rate);
        const double shared = np * (double)hi[w] / rate * (em ? 1.1 : 1.0) + (em ? 0.0 : chunks * (double)(hi[w] / B) * np * 8 / 4e9);
        t_pass += ((em || B % 4 == 0) ? std::min(by_matrix, shared) : by_matrix) + 0.1 + n_mat * np * 16 / 4e9;
      }
      slab = t_slab < t_pass;
    }
  }
  if (slab) {
    bool fits = true;
    int rc = bv ? windows_job_slab_var(e, lo, hi, n_win, d_sum, d_cnt, budget, &fits, *bv)
           : bt ? windows_job_slab(e, lo, hi, n_win, d_sum, d_cnt, budget, &fits, bt)
                : windows_slab(e, lo, hi, n_win, d_sum, d_cnt, budget, &fits);
    if (rc || fits) return rc;
    if (e->opt_win_plan == 2)
      return fail(NGD_E_NOMEM, "ngd_run_windows: a window does not fit the segment-slab plan's budget (NGD_OPT_WIN_MAX_BYTES)");
    if (slab_only)
      return fail(NGD_E_NOMEM, "ngd_run_windows: a window does not fit the segment-slab plan's budget (NGD_OPT_WIN_MAX_BYTES), and "
                               "NGD_OPT_EM_EXACT = 1 with NGD_OPT_EM_EXACT_WIN has no other plan (the per-window plan needs "
                               "NGD_OPT_EM_EXACT = 2); nothing was computed");
  }
  if (bv) return windows_job_by_pass_var(e, lo, hi, n_win, *bv, d_sum, d_cnt);
  if (bt) return windows_job_by_pass(e, lo, hi, n_win, *bt, d_sum, d_cnt);
  return windows_by_pass(e, lo, hi, n_win, d_sum, d_cnt);
}

// the device-memory forms: [n_win][n_pairs] (a job, bt != NULL: [n_win][n_rep + 1][n_pairs]) where the caller says
static int windows_device(ngd_engine *e, const uint64_t *lo, const uint64_t *hi, uint64_t n_win, const WinBoot *bt, void *d_sum,
                          void *d_cnt, const char *who, const WinBootVar *bv = nullptr) {
  if (!d_sum || !d_cnt) return fail(NGD_E_INVALID, std::string(who) + ": null output");
  e->win_info = ngd_windows_info{};
  e->fix_info = ngd_fixup_info{};
  e->n_batch_valid = 0;
  if (e->opt_em_exact_win) em_exact_call_begin(e);
  return windows_impl(e, lo, hi, n_win, (double *)d_sum, (unsigned long long *)d_cnt, bt, bv);
}

// the budget of a group of windows in the engine's batch buffers
// (tests only, NGD_ENABLE_TEST_HOOKS=1: NGD_TEST_WIN_GROUP_BYTES is the budget instead, so that a small call spans groups)
static uint64_t windows_group_bytes() {
  const char *hook = getenv("NGD_ENABLE_TEST_HOOKS");
  const char *bytes = hook && atoi(hook) ? getenv("NGD_TEST_WIN_GROUP_BYTES") : nullptr;
  return bytes ? strtoull(bytes, nullptr, 10) : 2ull << 30;
}

// the host-memory forms: windows in groups whose results fit ~2 GB of the engine's batch buffers; the tail (ngd_engine.h)
// takes each group's results out of d_bsum / d_bcnt -- a window is a set
// (a job, bt or bv != NULL: n_rep + 1 matrices per window, at least one window per group)
static int windows_chunked(ngd_engine *e, const uint64_t *lo, const uint64_t *hi, uint64_t n_win,
                           const Tail &tail, const WinBoot *bt, const WinBootVar *bv) {
  const uint64_t n_pairs = ngd_n_pairs(e->g.n_ind), n_mat = bv ? (uint64_t)bv->n_rep + 1 : bt ? (uint64_t)bt->n_rep + 1 : 1;
  const uint64_t per = std::max<uint64_t>(1, std::min<uint64_t>(n_win, windows_group_bytes() / (16 * n_mat * std::max<uint64_t>(1, n_pairs))));
  e->win_info = ngd_windows_info{};
  e->fix_info = ngd_fixup_info{};
  if (e->opt_em_exact_win) em_exact_call_begin(e);
  int rc = batch_buffers(e, (uint32_t)(per * n_mat));
  if (rc) return rc;
  for (uint64_t w0 = 0; w0 < n_win; w0 += per) {
    const uint64_t n = std::min(per, n_win - w0);
    const WinBootVar from = bv ? bv->from(w0) : WinBootVar{};
    if ((rc = windows_impl(e, lo + w0, hi + w0, n, e->d_bsum, e->d_bcnt, bt, bv ? &from : nullptr))) return rc;
    if ((rc = tail(w0, n, n_mat))) return rc;
  }
  e->n_batch_valid = 0;
  return NGD_OK;
}

// ... the copy tail: sums and counts (either may be NULL)
static Tail copy_tail(ngd_engine *e, double *sum, uint64_t *cnt) {
  return [=](uint64_t set0, uint64_t n_set, uint64_t n_mat) {
    const uint64_t at = set0 * n_mat * ngd_n_pairs(e->g.n_ind);
    int rc = copy_out(e, (uint32_t)(n_set * n_mat), e->d_bsum, e->d_bcnt, sum ? sum + at : nullptr, cnt ? cnt + at : nullptr);
    e->n_batch_valid = 0;
    return rc;
  };
}

// ... the distance tail: the tail of gen_dist() on every matrix (its host copies serve group after group), and what it refuses
static Tail dist_tail(ngd_engine *e, uint64_t tot_sites, uint64_t evol_model, double *dist) {
  return [=, h_sum = std::vector<double>(), h_cnt = std::vector<uint64_t>()](uint64_t set0, uint64_t n_set, uint64_t n_mat) mutable {
    const uint64_t per_set = n_mat * ngd_n_pairs(e->g.n_ind);
    h_sum.resize(n_set * per_set);
    h_cnt.resize(n_set * per_set);
    int rc = copy_out(e, (uint32_t)(n_set * n_mat), e->d_bsum, e->d_bcnt, h_sum.data(), h_cnt.data());
    e->n_batch_valid = 0;
    if (rc) return rc;
    // (the tail of gen_dist() on the host, the host's libm: ngd_finish's bits)
    return ngd_finish(h_sum.data(), h_cnt.data(), n_set * per_set, tot_sites, evol_model, dist + set0 * per_set);
  };
}

static int dist_refuse(const ngd_engine *e, const double *dist, uint64_t tot_sites, uint64_t evol_model, const char *who) {
  if (!dist) return fail(NGD_E_INVALID, std::string(who) + ": null argument");
  return finish_refuse(e, tot_sites, evol_model, who, nullptr);  // (the windows' check has refused a share of the pairs)
}

// the windows alone and the jobs of one window length (bt != NULL), checked: sums and counts, or distances
static int windows_host(ngd_engine *e, const uint64_t *lo, const uint64_t *hi, uint64_t n_win, const WinBoot *bt, double *sum,
                        uint64_t *cnt) {
  HIPCHK(hipSetDevice(e->device));
  return windows_chunked(e, lo, hi, n_win, copy_tail(e, sum, cnt), bt, nullptr);
}

static int windows_host_dist(ngd_engine *e, const uint64_t *lo, const uint64_t *hi, uint64_t n_win, const WinBoot *bt,
                             uint64_t tot_sites, uint64_t evol_model, double *dist, const char *who) {
  if (int rc = dist_refuse(e, dist, tot_sites, evol_model, who)) return rc;
  HIPCHK(hipSetDevice(e->device));
  return windows_chunked(e, lo, hi, n_win, dist_tail(e, tot_sites, evol_model, dist), bt, nullptr);
}

int ngd_run_windows_device(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win, void *d_sum,
                           void *d_cnt) {
  if (int rc = windows_check(e, win_lo, win_hi, n_win, "ngd_run_windows_device")) return rc;
  return windows_device(e, win_lo, win_hi, n_win, nullptr, d_sum, d_cnt, "ngd_run_windows_device");
}

int ngd_run_windows(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win, double *sum, uint64_t *cnt) {
  if (int rc = windows_check(e, win_lo, win_hi, n_win, "ngd_run_windows")) return rc;
  return windows_host(e, win_lo, win_hi, n_win, nullptr, sum, cnt);
}

int ngd_run_windows_dist(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win, uint64_t tot_sites,
                         uint64_t evol_model, double *dist) {
  if (int rc = windows_check(e, win_lo, win_hi, n_win, "ngd_run_windows_dist")) return rc;
  return windows_host_dist(e, win_lo, win_hi, n_win, nullptr, tot_sites, evol_model, dist, "ngd_run_windows_dist");
}

// ---- ngd_run_windows_job*: the arguments of a job, and the replicates' multiplicities counted from the block maps ----
// (bt: the job as the plans take it, its multiplicities in mult; n_rep == 0 -- the windows alone -- leaves both as they are)
static int windows_job_check(const ngd_engine *e, const uint64_t *lo, const uint64_t *hi, uint64_t n_win, const uint64_t *maps,
                             uint32_t n_rep, uint64_t n_blocks, uint64_t q, const char *who, std::vector<uint32_t> &mult,
                             WinBoot &bt) {
  if (int rc = windows_check(e, lo, hi, n_win, who, n_rep != 0)) return rc;
  if (!n_rep) return NGD_OK;  // (the windows alone: n_blocks and block_size are not read, as by ngd_run_job)
  const std::string w(who);
  if (!q) return fail(NGD_E_INVALID, w + ": block size 0");
  const uint64_t W = hi[0] - lo[0];
  for (uint64_t k = 1; k < n_win; k++)
    if (hi[k] - lo[k] != W) return fail(NGD_E_INVALID, w + ": the windows of a job must have one length (they share the block maps)");
  if (n_blocks != W / q) return fail(NGD_E_INVALID, w + ": n_blocks is not the window length / block_size (ngsDist.cpp:236)");
  if (!maps) return fail(NGD_E_INVALID, w + ": null block maps");
  if (!n_blocks) return fail(NGD_E_INVALID, w + ": empty bootstrap geometry (windows shorter than one block), as ngd_run_job");
  if (n_win * ((uint64_t)n_rep + 1) >= (1ull << 31)) return fail(NGD_E_INVALID, w + ": too many matrices in one call");
  if (n_rep > (1u << 20)) return fail(NGD_E_INVALID, w + ": more than 2^20 replicates in one call");  // (grid.y: chunks of 32)
  mult.assign((uint64_t)n_rep * n_blocks, 0u);
  for (uint32_t r = 0; r < n_rep; r++)
    for (uint64_t b = 0; b < n_blocks; b++) {
      const uint64_t src = maps[(uint64_t)r * n_blocks + b];
      if (src >= n_blocks) return fail(NGD_E_INVALID, w + ": block_map entry out of range");
      mult[(uint64_t)r * n_blocks + src]++;
    }
  bt = WinBoot{n_rep, n_blocks, q, mult.data()};
  return NGD_OK;
}

int ngd_run_windows_job_device(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win,
                               const uint64_t *block_maps, uint32_t n_rep, uint64_t n_blocks, uint64_t block_size, void *d_sum,
                               void *d_cnt) {
  std::vector<uint32_t> mult;
  WinBoot bt{};
  if (int rc = windows_job_check(e, win_lo, win_hi, n_win, block_maps, n_rep, n_blocks, block_size, "ngd_run_windows_job_device", mult, bt))
    return rc;
  if (!n_rep) return ngd_run_windows_device(e, win_lo, win_hi, n_win, d_sum, d_cnt);
  return windows_device(e, win_lo, win_hi, n_win, &bt, d_sum, d_cnt, "ngd_run_windows_job_device");
}

int ngd_run_windows_job(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win, const uint64_t *block_maps,
                        uint32_t n_rep, uint64_t n_blocks, uint64_t block_size, double *sum, uint64_t *cnt) {
  std::vector<uint32_t> mult;
  WinBoot bt{};
  if (int rc = windows_job_check(e, win_lo, win_hi, n_win, block_maps, n_rep, n_blocks, block_size, "ngd_run_windows_job", mult, bt))
    return rc;
  if (!n_rep) return ngd_run_windows(e, win_lo, win_hi, n_win, sum, cnt);
  return windows_host(e, win_lo, win_hi, n_win, &bt, sum, cnt);
}

int ngd_run_windows_job_dist(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win,
                             const uint64_t *block_maps, uint32_t n_rep, uint64_t n_blocks, uint64_t block_size,
                             uint64_t tot_sites, uint64_t evol_model, double *dist) {
  std::vector<uint32_t> mult;
  WinBoot bt{};
  if (int rc = windows_job_check(e, win_lo, win_hi, n_win, block_maps, n_rep, n_blocks, block_size, "ngd_run_windows_job_dist", mult, bt))
    return rc;
  if (!n_rep) return ngd_run_windows_dist(e, win_lo, win_hi, n_win, tot_sites, evol_model, dist);
  return windows_host_dist(e, win_lo, win_hi, n_win, &bt, tot_sites, evol_model, dist, "ngd_run_windows_job_dist");
}

// ---- ngd_run_windows_job_var*: the arguments, and every class's multiplicities counted from its block maps ----
// (a class: the windows that share map_off and n_blocks -- one set of maps, checked and counted once, one weight table)
struct WinVarStore {
  std::vector<uint32_t> cls, mult;
  std::vector<uint64_t> cls_blocks, cls_mult;
};

static int windows_job_var_check(const ngd_engine *e, const uint64_t *lo, const uint64_t *hi, uint64_t n_win, const uint64_t *maps,
                                 uint64_t maps_len, const uint64_t *map_off, uint32_t n_rep, uint64_t q, const char *who,
                                 WinVarStore &st, WinBootVar &bv) {
  if (!e) return fail(NGD_E_INVALID, std::string(who) + ": null engine");
  if (int rc = em_exact_refuse(e, who)) return rc;  // (per-window weights are not patched: neither value of the option serves it)
  if (int rc = windows_check(e, lo, hi, n_win, who)) return rc;
  if (!n_rep) return NGD_OK;  // (the windows alone: the maps and block_size are not read)
  const std::string w(who);
  if (!q) return fail(NGD_E_INVALID, w + ": block size 0");
  if (!map_off) return fail(NGD_E_INVALID, w + ": null map offsets");
  if (n_win * ((uint64_t)n_rep + 1) >= (1ull << 31)) return fail(NGD_E_INVALID, w + ": too many matrices in one call");
  if (n_rep > (1u << 20)) return fail(NGD_E_INVALID, w + ": more than 2^20 replicates in one call");  // (grid.y: chunks of 32)
  std::map<std::pair<uint64_t, uint64_t>, uint32_t> ids;
  st.cls.assign(n_win, NGD_WIN_NO_CLASS);
  for (uint64_t k = 0; k < n_win; k++) {
    const uint64_t n_blocks = (hi[k] - lo[k]) / q;
    if (!n_blocks) continue;  // (no block: no entries, the offset is not read)
    if (!maps) return fail(NGD_E_INVALID, w + ": null block maps");
    const auto ins = ids.emplace(std::make_pair(map_off[k], n_blocks), (uint32_t)st.cls_blocks.size());
    st.cls[k] = ins.first->second;
    if (!ins.second) continue;
    const uint64_t len = (uint64_t)n_rep * n_blocks;
    if (map_off[k] > maps_len || len > maps_len - map_off[k])
      return fail(NGD_E_INVALID, w + ": the block maps of window " + std::to_string(k) + " reach past maps_len");
    const uint64_t at = st.mult.size();
    st.cls_blocks.push_back(n_blocks);
    st.cls_mult.push_back(at);
    st.mult.resize(at + len, 0u);
    for (uint32_t r = 0; r < n_rep; r++)
      for (uint64_t b = 0; b < n_blocks; b++) {
        const uint64_t src = maps[map_off[k] + (uint64_t)r * n_blocks + b];
        if (src >= n_blocks) return fail(NGD_E_INVALID, w + ": block_map entry out of range (window " + std::to_string(k) + ")");
        st.mult[at + (uint64_t)r * n_blocks + src]++;
      }
  }
  bv = WinBootVar{n_rep, q, (uint32_t)st.cls_blocks.size(), st.cls.data(), st.cls_blocks.data(), st.cls_mult.data(), st.mult.data()};
  return NGD_OK;
}

int ngd_run_windows_job_var_device(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win,
                                   const uint64_t *block_maps, uint64_t maps_len, const uint64_t *map_off, uint32_t n_rep,
                                   uint64_t block_size, void *d_sum, void *d_cnt) {
  WinVarStore st;
  WinBootVar bv{};
  if (int rc = windows_job_var_check(e, win_lo, win_hi, n_win, block_maps, maps_len, map_off, n_rep, block_size,
                                     "ngd_run_windows_job_var_device", st, bv))
    return rc;
  if (!n_rep) return ngd_run_windows_device(e, win_lo, win_hi, n_win, d_sum, d_cnt);
  return windows_device(e, win_lo, win_hi, n_win, nullptr, d_sum, d_cnt, "ngd_run_windows_job_var_device", &bv);
}

// the window driver of the tails (ngd_engine.h): the arguments checked -- as a job's, or with n_rep == 0 and no job_form as
// ngd_run_windows' --, then what `refuse` refuses, then every group of windows from the batch buffers through the tail
int windows_tail(ngd_engine *e, const WinJobArgs &a, bool job_form, const char *who, const Tail &tail,
                 const std::function<int()> &refuse) {
  WinVarStore st;
  WinBootVar bv{};
  if (int rc = a.n_rep || job_form
                   ? windows_job_var_check(e, a.lo, a.hi, a.n_win, a.maps, a.maps_len, a.map_off, a.n_rep, a.block_size, who, st, bv)
                   : windows_check(e, a.lo, a.hi, a.n_win, who))
    return rc;
  if (refuse)
    if (int rc = refuse()) return rc;
  HIPCHK(hipSetDevice(e->device));
  return windows_chunked(e, a.lo, a.hi, a.n_win, tail, nullptr, a.n_rep ? &bv : nullptr);
}

int ngd_run_windows_job_var(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win, const uint64_t *block_maps,
                            uint64_t maps_len, const uint64_t *map_off, uint32_t n_rep, uint64_t block_size, double *sum,
                            uint64_t *cnt) {
  return windows_tail(e, WinJobArgs{win_lo, win_hi, n_win, block_maps, maps_len, map_off, n_rep, block_size}, true,
                      "ngd_run_windows_job_var", copy_tail(e, sum, cnt));
}

int ngd_run_windows_job_var_dist(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win,
                                 const uint64_t *block_maps, uint64_t maps_len, const uint64_t *map_off, uint32_t n_rep,
                                 uint64_t block_size, uint64_t tot_sites, uint64_t evol_model, double *dist) {
  // (n_rep == 0 is ngd_run_windows_dist, in the words of the distances' refusals too)
  const char *who = "ngd_run_windows_job_var_dist", *who_dist = n_rep ? who : "ngd_run_windows_dist";
  return windows_tail(e, WinJobArgs{win_lo, win_hi, n_win, block_maps, maps_len, map_off, n_rep, block_size}, true, who,
                      dist_tail(e, tot_sites, evol_model, dist), [&] { return dist_refuse(e, dist, tot_sites, evol_model, who_dist); });
}

int ngd_last_windows(const ngd_engine *e, ngd_windows_info *info) {
  if (!e || !info) return fail(NGD_E_INVALID, "ngd_last_windows: null argument");
  *info = e->win_info;
  return NGD_OK;
}
