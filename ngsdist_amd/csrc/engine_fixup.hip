// engine_fixup.hip -- the fix-up pass of the one-image (congruent) engines: the pairs a reduction noted, recomputed with
// two-operand arithmetic tile by tile, pair by pair or as one more whole pass (kernels: fixup.hip).
#include "ngd_engine.h"

// The whole matrix once more in the two-image arithmetic -- P and Q = score . P formed a range of k-groups at a time from
// the image and SM (layout.hip k_pq_range), K1m over the pair of scratch images range by range, every block adding to its
// plane of the slab (the walk of the single_image = 1 engines, kg_ranges.h) -- then the noting rule once more:
// exactly the pairs it picks take the new sums.  Costs a pass and a half (~70 ms at cfg 3's size) WHATEVER the data, where
// tile by tile a data set of clones costs 0.8 s: fixup_pass() takes this way when its tiles would cost more.
static int fixup_by_pass(ngd_engine *e, const uint32_t *ws, uint64_t s_hi, double *d_sum, const unsigned long long *d_cnt, double thr) {
  const ngd_geom &g = e->g;
  const uint64_t kstride = (uint64_t)g.n_ig * 64;
  const uint64_t kg_lim = std::min<uint64_t>(g.n_kg, (3 * s_hi + 3) / 4);  // (the scratch images: k = 3 s + g, layout.hip k_pq_range)
  // ranges of about 1 GiB per scratch image (two of them), every slice a piece of every range
  const kg_pass_ranges pr(kg_lim, e->n_ks, std::max<uint64_t>(256, ((uint64_t)1 << 30) / (kstride * 8)), 0);
  const uint64_t need = (std::min<uint64_t>(kg_lim, pr.piece * e->n_ks) + NGD_KG_TAIL) * kstride;
  int rc = e->fix_p.ensure(e, need);
  if (!rc) rc = e->fix_q.ensure(e, need);
  if (!rc) rc = e->d_fixnew.ensure(e, ngd_n_pairs(g.n_ind));
  if (rc) return rc;
  for (uint64_t r = 0; r < pr.n_ranges; r++) {
    const uint64_t lo = pr.lo(r), hi = pr.hi(r);
    ngd_launch_pq_range(e->st, g, e->sc, e->PA, e->SM, ws, lo, hi + NGD_KG_TAIL, e->fix_p, e->fix_q);
    ngd_mfma_launch l;
    l.PA = e->fix_p; l.QB = e->fix_q;
    l.n_ks = e->n_ks; l.kg_per_slice = pr.piece; l.n_kg_eff = hi - lo;
    l.slab = e->slab; l.resume = r > 0;
    ngd_launch_accum_mfma(e->st, mfma_engine(e), l);
  }
  ngd_launch_reduce(e->st, g, e->slab, e->n_ks, 1, e->d_tiles, e->n_tiles, e->d_fixnew, nullptr, 0, nullptr, 0.0);
  ngd_launch_fix_merge(e->st, g, e->d_fixnew, d_sum, d_cnt, thr, e->d_tiles, e->n_tiles);
  HIPCHK(hipGetLastError());
  return NGD_OK;
}

// The same for the per-block partial results of a bootstrap job whose blocks are whole k-groups: EVERY entry of the slab is
// formed again by the two-operand arithmetic, the scratch images made for a range of whole slices at a time (in eights: the
// XCD deal of accum_mfma.hip) and handed to the kernel moved back by the range's first k-group, as accumulate_single_image()
// does for ngd_config.single_image = 1.  The replicates are then reduced from the slab again (partials_impl).
static int fixup_partials_by_pass(ngd_engine *e, uint64_t s_hi) {
  const ngd_geom &g = e->g;
  const uint64_t kstride = (uint64_t)g.n_ig * 64;
  const kg_slices sl{e->blk.nks, e->blk.per_slice, 0, std::min<uint64_t>(g.n_kg, 3 * s_hi / 4)};
  if (!sl.per_slice || !sl.n_ks || sl.n_ks % 8) return fail(NGD_E_HIP, "fix-up pass: internal -- the partial results' slices are not in eights");
  const uint64_t span = std::max<uint64_t>(8 * sl.per_slice, ((uint64_t)1 << 30) / (kstride * 8));  // ~1 GiB per scratch image
  for (uint32_t ks0 = 0; ks0 < sl.n_ks;) {
    const kg_slice_group r = kg_slice_group_at(sl, span, ks0);
    const uint64_t need = (r.hi - r.lo + NGD_KG_TAIL) * kstride;
    int rc = e->fix_p.ensure(e, need);
    if (!rc) rc = e->fix_q.ensure(e, need);
    if (rc) return rc;
    ngd_launch_pq_range(e->st, g, e->sc, e->PA, e->SM, nullptr, r.lo, std::min<uint64_t>(r.hi + NGD_KG_TAIL, g.n_kg + NGD_KG_TAIL), e->fix_p, e->fix_q);
    ngd_mfma_launch l;
    l.PA = kg_moved_back(e->fix_p, e->fix_p.capacity(), kstride, NGD_KG_TAIL, sl, r);
    l.QB = kg_moved_back(e->fix_q, e->fix_q.capacity(), kstride, NGD_KG_TAIL, sl, r);
    if (!l.PA || !l.QB) return fail(NGD_E_HIP, "fix-up pass: internal -- a slice of the range reaches outside the scratch images");
    l.ks0 = r.ks0; l.n_ks = r.n; l.kg_per_slice = sl.per_slice; l.n_kg_eff = sl.kg_lim;
    l.slab = e->blk.sums();
    ngd_launch_accum_mfma(e->st, mfma_engine(e), l);
    HIPCHK(hipGetLastError());
    ks0 += r.n;
  }
  return NGD_OK;
}

// The pairs the last reduction noted (n of them; all: more than the list holds -- every pair of the engine), grouped by
// their 16 x 16 tile of individuals: tiles with NGD_FIX_TILE_MIN noted pairs or more are recomputed whole, the rest pair
// by pair.  The stream is idle.
int fix_collect(ngd_engine *e, uint32_t n, bool all, std::vector<ngd_fix_tile> &tiles, std::vector<unsigned long long> &singles) {
  if (all) {
    for (const ngd_tile &t16 : e->h_tiles16) {  // (this engine's shard of the pairs)
        const uint32_t ig = t16.ti, jg = t16.tj;
        ngd_fix_tile t{(uint16_t)ig, (uint16_t)jg, 0, {0, 0, 0, 0}};
        for (uint32_t r = 0; r < 16; r++)
          for (uint32_t c = 0; c < 16; c++) {
            const uint64_t i = (uint64_t)ig * 16 + r, j = (uint64_t)jg * 16 + c;
            if (i < j && j < e->g.n_ind) { t.mask[(r * 16 + c) >> 6] |= 1ull << ((r * 16 + c) & 63); t.n++; }
          }
        if (t.n) tiles.push_back(t);
      }
  } else {
    // Nearly identical individuals come in clusters: the noted pairs are grouped by their 16 x 16 tile of individuals on
    // the host (8-byte entries), a tile that holds NGD_FIX_TILE_MIN of them or more is recomputed whole (k_fixup_tile:
    // coalesced, 4 bytes per pair-site), the others pair by pair (k_fixup: ~400)
    std::vector<unsigned long long> list(n);
    HIPCHK(hipMemcpy(list.data(), e->d_fixlist, (size_t)n * 8, hipMemcpyDeviceToHost));  // (the stream is idle: the pass was waited for)
    std::sort(list.begin(), list.end(), [](unsigned long long x, unsigned long long y) {
      const unsigned long long tx = ((x >> 36) << 32) | ((uint32_t)x >> 4), ty = ((y >> 36) << 32) | ((uint32_t)y >> 4);
      return tx != ty ? tx < ty : x < y;
    });
    for (uint32_t k = 0; k < n;) {
      const uint32_t ig = (uint32_t)(list[k] >> 36), jg = (uint32_t)list[k] >> 4;
      uint32_t k1 = k;
      ngd_fix_tile t{(uint16_t)ig, (uint16_t)jg, 0, {0, 0, 0, 0}};
      while (k1 < n && (uint32_t)(list[k1] >> 36) == ig && ((uint32_t)list[k1] >> 4) == jg) {
        const uint32_t bit = ((uint32_t)(list[k1] >> 32) & 15) * 16 + ((uint32_t)list[k1] & 15);
        t.mask[bit >> 6] |= 1ull << (bit & 63);
        k1++;
      }
      t.n = k1 - k;
      if (t.n >= NGD_FIX_TILE_MIN) tiles.push_back(t);
      else singles.insert(singles.end(), list.begin() + k, list.begin() + k1);
      k = k1;
    }
  }
  return NGD_OK;
}

// single_image = 2 engines on the reference's matrices: the pairs the last reduction noted (sums too small for the
// congruent arithmetic to hold to 1e-9 relative: nearly identical individuals) are recomputed with two-operand arithmetic
// from p recovered out of the image and the side array (fixup.hip).  The stream is idle and *h_fixcount has arrived.
//  * a single matrix (d_sum != NULL): over the sites [0, s_hi) with the per-site weights ws (NULL: none), the sums written
//    over the MFMA pass's;
//  * per-block partial results (d_sum == NULL): the noted pairs' entries of the block scratch's sums, slice by slice -- the caller then
//    forms the replicates again.
// The tolerance is unconditional: EVERY noted pair is recomputed, in launches of bounded size, however many there are
// (round 6; rounds 4-5 gave up on all of them past a budget of ~0.33 s).  More noted pairs than the list holds (fix_cap):
// which ones is then unknown, and every pair of the engine is recomputed.  Where the tiles of a single matrix would cost
// more than the whole matrix in the two-image arithmetic (a data set of clones) it is recomputed that way, in one more
// pass (fixup_by_pass above: 86 ms at cfg 3's size where the tiles take ~0.8 s).  Only a caller who SETS a budget
// (NGD_OPT_FIXUP_WORK != 0) gets the old behaviour: noted work above it is left as the one-image pass computed it and
// ngd_last_fixup() reports the pairs as skipped.
// A pair's slices depend on the number of sites alone (not on how many other pairs were noted), so its recomputed bits do
// not depend on the rest of the data set.
int fixup_pass(ngd_engine *e, const uint32_t *ws, uint64_t s_hi, double *d_sum, uint64_t sites_per_slice,
               uint32_t n_slab_slices, bool *patched, const unsigned long long *d_cnt, double thr) {
  if (patched) *patched = false;
  const uint32_t n = *(volatile uint32_t *)e->h_fixcount;
  e->fix_info.flagged += n;
  if (!n) return NGD_OK;
  const bool capped = e->opt_fix_work != 0;  // a budget is a caller's explicit leave to skip
  const double budget = (double)e->opt_fix_work;
  const bool all = n > e->fix_cap;  // the list overflowed: which pairs were noted is not known
  const double tile_cost = NGD_FIX_TILE_COST_X10 / 10.0 * (double)s_hi;
  // (the least the pass could cost -- every tile full -- before the list is fetched and sorted)
  if (capped && (all ? (double)e->h_tiles16.size() : (double)((n + 255) / 256)) * tile_cost > budget) {
    e->fix_info.skipped += n;
    return NGD_OK;
  }
  hipEvent_t t0 = e->ev[0], t1 = e->ev[1];  // (the pass's own timings have been read)
  HIPCHK(hipEventRecord(t0, e->st));
  std::vector<ngd_fix_tile> tiles;
  std::vector<unsigned long long> singles;
  if (int rc = fix_collect(e, n, all, tiles, singles)) return rc;
  // what the recomputation costs, in pair-sites (ngd_internal.h)
  if (capped && (double)tiles.size() * tile_cost + (double)singles.size() * (double)s_hi > budget) {
    e->fix_info.skipped += n;
    return NGD_OK;
  }
  // A single matrix whose tiles would cost more than the whole matrix by the two-operand MFMA arithmetic takes that way
  // ([measured] tiles: 6.5e11 pair-sites/s of 256 each; the pass: 6 flop per pair-site at ~55 TF with its ranges' overhead
  // + 80 bytes per (individual, site) to form the scratch images at ~2.4 TB/s)
  if (d_sum && e->kernel == NGD_KERNEL_MFMA && e->exact_shapes == 0 && e->slab) {
    const double t_tiles = ((double)tiles.size() * 256.0 + (double)singles.size() * 60.0) * (double)s_hi / 6.5e11;
    const double t_pass = 6.0 * (double)e->n_owned_pairs * (double)s_hi / 55e12 + 80.0 * (double)e->g.n_pad * (double)s_hi / 2.4e12 + 2e-3;
    if (t_tiles > t_pass) {
      int rc = fixup_by_pass(e, ws, s_hi, d_sum, d_cnt, thr);
      if (rc) return rc;
      HIPCHK(hipEventRecord(t1, e->st));
      HIPCHK(hipStreamSynchronize(e->st));
      if (int rf = mfma_fault(e)) return rf;
      float ms = 0;
      hipEventElapsedTime(&ms, t0, t1);
      e->fix_info.ms += ms;
      e->fix_info.recomputed += all ? e->n_owned_pairs : n;
      e->fix_info.by_pass += 1;
      if (patched) *patched = true;
      return NGD_OK;
    }
  }
  // Per-block partial results (whole k-groups per block): where the noted tiles would cost more than the whole slab again
  // in the two-operand arithmetic, the whole slab it is (round 6; the tiles: 0.8 s for a data set of clones at cfg 3's size)
  if (!d_sum && e->kernel == NGD_KERNEL_MFMA && e->exact_shapes == 0 && e->blk.sums() && e->blk.per_slice &&
      e->blk.sums_block() % 4 == 0 && (uint64_t)e->blk.per_slice * 4 == sites_per_slice * 3) {
    const double t_tiles = ((double)tiles.size() * 256.0 + (double)singles.size() * 60.0) * (double)s_hi / 6.5e11;
    const double t_pass = 6.0 * (double)e->n_owned_pairs * (double)s_hi / 50e12 + 80.0 * (double)e->g.n_pad * (double)s_hi / 2.4e12 + 2e-3;
    // (tests only, NGD_ENABLE_TEST_HOOKS=1: NGD_TEST_FIX_PARTIALS = "pass" / "tiles" takes the choice away from the estimate)
    const char *forced = (getenv("NGD_ENABLE_TEST_HOOKS") && atoi(getenv("NGD_ENABLE_TEST_HOOKS"))) ? getenv("NGD_TEST_FIX_PARTIALS") : nullptr;
    const bool by_pass = forced ? forced[0] == 'p' : t_tiles > t_pass;
    if (by_pass) {
      int rc = fixup_partials_by_pass(e, s_hi);
      if (rc) return rc;
      HIPCHK(hipEventRecord(t1, e->st));
      HIPCHK(hipStreamSynchronize(e->st));
      if (int rf = mfma_fault(e)) return rf;
      float ms = 0;
      hipEventElapsedTime(&ms, t0, t1);
      e->fix_info.ms += ms;
      e->fix_info.recomputed += all ? e->n_owned_pairs : n;
      e->fix_info.by_pass += 1;
      if (patched) *patched = true;
      return NGD_OK;
    }
  }
  // launches of at most 2^22 workgroups (HIP bounds a launch's threads by 2^32); a pass over per-block partial results has
  // one workgroup per (tile or pair, slab slice)
  const uint64_t max_wg = 1ull << 22;
  if (!d_sum && n_slab_slices > max_wg) return fail(NGD_E_INVALID, "fix-up pass: more slab slices than a launch has workgroups");
  if (!tiles.empty()) {
    int rc = e->d_fixtiles.ensure(e, tiles.size());
    if (rc) return rc;
    HIPCHK(hipMemcpy(e->d_fixtiles, tiles.data(), tiles.size() * sizeof(ngd_fix_tile), hipMemcpyHostToDevice));
    if (d_sum) {
      // slices of 4096 sites (fewer, longer ones only where NGD_FIX_CAP of them would not cover the sites); as many tiles
      // to a launch as the partial-sum scratch holds (stream order: a launch's scratch is read before the next writes it)
      rc = e->d_fixtparts.ensure(e, (uint64_t)NGD_FIX_CAP * 256);
      if (rc) return rc;
      const uint64_t sps = std::max<uint64_t>(4096, (s_hi + NGD_FIX_CAP - 1) / NGD_FIX_CAP);
      const uint64_t n_slices = (s_hi + sps - 1) / sps;
      const size_t per = std::max<size_t>(1, NGD_FIX_CAP / n_slices);
      for (size_t off = 0; off < tiles.size(); off += per) {
        const uint32_t m = (uint32_t)std::min<size_t>(per, tiles.size() - off);
        ngd_launch_fixup_tiles(e->st, e->g, e->sc, e->PA, e->SM, ws, e->d_fixtiles + off, m, 0, s_hi, sps, (uint32_t)n_slices, 0,
                               e->d_fixtparts);
        ngd_launch_fixup_tiles_finish(e->st, e->g, e->d_fixtiles + off, m, e->d_fixtparts, (uint32_t)n_slices, d_sum);
      }
    } else {
      const size_t per = (size_t)std::max<uint64_t>(1, max_wg / n_slab_slices);
      for (size_t off = 0; off < tiles.size(); off += per) {
        const uint32_t m = (uint32_t)std::min<size_t>(per, tiles.size() - off);
        ngd_launch_fixup_tiles(e->st, e->g, e->sc, e->PA, e->SM, nullptr, e->d_fixtiles + off, m, 0, s_hi, sites_per_slice,
                               n_slab_slices, 1, e->blk.sums());
      }
    }
  }
  const uint32_t n1 = (uint32_t)singles.size();
  if (n1) HIPCHK(hipMemcpy(e->d_fixlist, singles.data(), (size_t)n1 * 8, hipMemcpyHostToDevice));
  if (n1 && d_sum) {
    const uint64_t sps = std::max<uint64_t>(1024, (s_hi + NGD_FIX_CAP - 1) / NGD_FIX_CAP);
    const uint64_t n_slices = (s_hi + sps - 1) / sps;
    const uint32_t per = (uint32_t)std::max<uint64_t>(1, NGD_FIX_CAP / n_slices);
    for (uint32_t off = 0; off < n1; off += per) {
      const uint32_t m = std::min<uint32_t>(per, n1 - off);
      ngd_launch_fixup(e->st, e->g, e->sc, e->PA, e->SM, ws, e->d_fixlist + off, m, 0, s_hi, sps, (uint32_t)n_slices, 0, e->d_fixparts);
      ngd_launch_fixup_finish(e->st, e->g, e->d_fixlist + off, m, e->d_fixparts, (uint32_t)n_slices, d_sum);
    }
  } else if (n1) {
    const uint32_t per = (uint32_t)std::max<uint64_t>(1, max_wg / n_slab_slices);
    for (uint32_t off = 0; off < n1; off += per) {
      const uint32_t m = std::min<uint32_t>(per, n1 - off);
      ngd_launch_fixup(e->st, e->g, e->sc, e->PA, e->SM, nullptr, e->d_fixlist + off, m, 0, s_hi, sites_per_slice, n_slab_slices, 1,
                       e->blk.sums());
    }
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(t1, e->st));
  HIPCHK(hipStreamSynchronize(e->st));
  float ms = 0;
  hipEventElapsedTime(&ms, t0, t1);
  e->fix_info.ms += ms;
  e->fix_info.recomputed += all ? e->n_owned_pairs : n;
  if (patched) *patched = true;
  return NGD_OK;
}
