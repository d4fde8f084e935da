// engine_plans.hip -- the launch sequences that stand in for the reference's `for i1<i2: threadpool_add(gen_dist_slave)`
// block (ngsDist.cpp:244-269): one accumulation pass, the bootstrap plans that share passes between matrices, and
// run_impl, which picks the cheapest that applies.
#include "ngd_engine.h"

// The slices of one accumulation pass.
struct pass_slices {
  // one bootstrap replicate: its per-site weights (NULL: none); for the MFMA kernel kgl is then the list of k-groups to
  // visit and per_slice / kg_lim count list entries
  const uint32_t *w = nullptr, *kgl = nullptr;
  uint64_t sites_eff = 0;
  uint32_t n_ks = 0;
  uint64_t per_slice = 0, kg_lim = 0;
  double *slab = nullptr;
  // k_per_slice != 0 (MFMA, bootstrap blocks that are not whole k-groups): slices of k_per_slice contraction indices,
  // masked by the per-slice 0/1 weights in e->blk.wslice (w_stride k-groups per slice)
  uint64_t k_per_slice = 0;
  uint32_t w_stride = 0;
  bool note = false;  // NGD_OPT_EM_EXACT, table-driven EM kernel, a plain pass: the noting form, into e->d_note
  // ... in the congruent image, whose blocks are rounded outwards to whole periods of four sites (ngd_layout.h): the slices'
  // k-group ranges and weight offsets by table instead (the windows' NGD_SEG_* table, win_plan.h), weights in e->blk.wslice
  const uint64_t *seg = nullptr;
};

// the MFMA launch over the pass's slices as they are, but for the second image and the k-group list
static ngd_mfma_launch slices_launch(const ngd_engine *e, const pass_slices &p, const double *d_w_plain) {
  ngd_mfma_launch l;
  l.PA = e->PA;
  l.d_wk = p.k_per_slice ? e->blk.wslice : (p.w ? e->d_wk : d_w_plain);
  l.n_ks = p.n_ks; l.kg_per_slice = p.per_slice; l.n_kg_eff = p.kg_lim;
  l.k_per_slice = p.k_per_slice; l.w_slice_stride = p.w_stride;
  if (p.seg) { l.d_wk = e->blk.wslice; l.d_seg = p.seg; l.w_slice_stride = 1; l.k_per_slice = 0; }
  l.slab = p.slab;
  return l;
}

// ngd_config.single_image = 1:
// QB is formed range by range into a scratch (k_qb_range: HBM work, 49 GB a pass at cfg 3) on the accumulation
// kernel's own stream, each range before the launch that reads it (the ranges: kg_ranges.h).
//  * a whole pass (slab == e->slab): EVERY slice takes a piece of every range, so that each launch has the
//    pass's full grid (a launch over a few whole slices would not fill the chip once: cfg 3 has 34 workgroups
//    per slice and room for 768); a block adds its sums over the range to its plane of the slab (`resume`).  A
//    slice is then not one contiguous run of k-groups, as it is with both images resident: the sums of the two
//    engines agree to rounding (exactly where the arithmetic is exact: called genotypes), not bit for bit.
//  * per-block partial sums (a slice = a bootstrap block, thousands of them): ranges of whole slices, in eights
//    (the XCD deal of accum_mfma.hip); the kernel is handed the scratch moved back by the range's first k-group.
// (single-image engines make no k-group lists: pass_impl() walks every k-group of a weighted pass)
// [measured, cfg 3] forming a range on a second stream beside the launch over the range before it gains nothing:
// the accumulation kernel slows by what the overlap hides, however few blocks form the range and with or
// without non-temporal accesses (profiles/r04_single_image.txt; tools/experiments/single_image_two_streams.patch).
static int accumulate_single_image(ngd_engine *e, const pass_slices &p) {
  const ngd_geom &g = e->g;
  const ngd_mfma_engine en = mfma_engine(e);
  const uint64_t kstride = (uint64_t)g.n_ig * 64;
  const uint64_t span = std::max<uint64_t>(1, e->qb_chunk_kg);
  // what the engine keeps of the second image (its first qb_res_kg k-groups, ngd_config.second_image_mib) is read
  // where it lies: one launch over that part of a whole pass, or over the slices that end inside it
  const uint64_t res = std::min<uint64_t>(e->qb_res_kg, p.kg_lim);
  ngd_mfma_launch l = slices_launch(e, p, nullptr);
  // k-groups [lo, hi) of the second image (+ the tail the operand pipeline runs ahead) into the scratch
  auto form = [&](uint64_t lo, uint64_t hi) -> int {
    const uint64_t need = (hi - lo + NGD_KG_TAIL) * kstride;
    if (need > e->qb_chunk.capacity()) {
      // a range longer than the scratch was sized for (bootstrap blocks of very many sites: a partial-sum slice
      // is a whole block): the scratch grows to hold it -- the earlier ranges' launches have to be over first
      HIPCHK(hipStreamSynchronize(e->st));
      if (int rc = e->qb_chunk.ensure(e, need)) return rc;
    }
    ngd_launch_qb_range(e->st, g, e->sc, e->PA, lo, std::min<uint64_t>(hi + NGD_KG_TAIL, g.n_kg + NGD_KG_TAIL), e->qb_chunk);
    return NGD_OK;
  };
  if (p.slab == e->slab && !p.k_per_slice) {  // a whole pass
    const double *w = l.d_wk;
    if (res) {
      l.QB = e->QB_res;
      l.kg_per_slice = std::max<uint64_t>(4, ((res + p.n_ks - 1) / p.n_ks + 3) / 4 * 4); l.n_kg_eff = res;
      ngd_launch_accum_mfma(e->st, en, l);
    }
    const kg_pass_ranges pr(p.kg_lim, p.n_ks, span, res);  // ... goes on from the resident part
    for (uint64_t r = 0; r < pr.n_ranges; r++) {
      const uint64_t lo = pr.lo(r), hi = pr.hi(r);
      if (int rc = form(lo, hi)) return rc;
      l.PA = e->PA + lo * kstride; l.QB = e->qb_chunk;
      l.d_wk = w ? w + lo * 4 : nullptr;
      l.kg_per_slice = pr.piece; l.n_kg_eff = hi - lo;
      l.resume = r > 0 || res > 0;
      ngd_launch_accum_mfma(e->st, en, l);
    }
    return NGD_OK;
  }
  const kg_slices sl{p.n_ks, p.per_slice, p.k_per_slice, p.kg_lim};
  const uint32_t ks_first = res ? kg_slices_resident(sl, res) : 0;
  if (ks_first) {
    l.QB = e->QB_res;
    l.n_ks = ks_first;
    ngd_launch_accum_mfma(e->st, en, l);
  }
  for (uint32_t ks0 = ks_first; ks0 < p.n_ks; ks0 += l.n_ks) {
    const kg_slice_group r = kg_slice_group_at(sl, span, ks0);
    if (int rc = form(r.lo, r.hi)) return rc;
    l.QB = kg_moved_back(e->qb_chunk, e->qb_chunk.capacity(), kstride, NGD_KG_TAIL, sl, r);
    if (!l.QB) return fail(NGD_E_HIP, "single-image pass: internal -- a slice of the range reaches outside the scratch of the second image");
    l.ks0 = r.ks0; l.n_ks = r.n;
    ngd_launch_accum_mfma(e->st, en, l);
  }
  return NGD_OK;
}

static void accumulate_em(ngd_engine *e, const pass_slices &p) {
  if (e->kernel != NGD_KERNEL_EM_TABLE)
    ngd_launch_accum_em(e->st, e->g, e->PA, p.w, p.sites_eff, e->sc, e->cfg.pairwise_del, e->kernel == NGD_KERNEL_EM_FAST,
                        e->d_tiles16, e->n_tiles16, p.n_ks, p.per_slice, p.slab);
  else if (p.note)
    ngd_launch_accum_em_table_note(e->st, emt_common(e), p.n_ks, p.per_slice, p.slab, e->d_note);
  else
    ngd_launch_accum_em_table(e->st, emt_common(e), p.w, p.sites_eff, p.n_ks, p.per_slice, p.slab);
}

// both images resident (single_image = 2: both operands from the one image, the congruence's diagonal on the weights -- of a
// plain pass too)
static void accumulate_two_images(ngd_engine *e, const pass_slices &p) {
  ngd_mfma_launch l = slices_launch(e, p, e->congruent ? e->d_wD.get() : nullptr);
  l.QB = e->congruent ? e->PA : e->QB;
  l.d_kgl = (!p.k_per_slice && !p.seg) ? p.kgl : nullptr;  // (a replicate's list, or the plain pass's without the unit-sum coordinate)
  ngd_launch_accum_mfma(e->st, mfma_engine(e), l);
}

static int launch_accumulate(ngd_engine *e, const pass_slices &p) {
  if (e->kernel != NGD_KERNEL_MFMA) accumulate_em(e, p);
  else if (e->single_image) return accumulate_single_image(e, p);
  else accumulate_two_images(e, p);
  return NGD_OK;
}

// bit planes that hold multiplicities up to mult_max (none drawn: one all-zero plane -- 0 planes means "unweighted")
static uint32_t count_planes(uint32_t mult_max) {
  uint32_t n = 1;
  while (n < 32 && (mult_max >> n)) n++;
  return n;
}

// --pairwise_del: the valid-site counts of one matrix of a job -- the full data set (d_mult == NULL) or the replicate whose
// block multiplicities are d_mult (on the device; at most mult_max)
static void count_matrix(ngd_engine *e, const uint32_t *d_mult, uint32_t mult_max, uint64_t n_blocks, uint64_t block_size,
                         unsigned long long *d_cnt) {
  const ngd_geom &g = e->g;
  const uint32_t n_planes = d_mult ? count_planes(mult_max) : 0;
  if (d_mult) {
    ngd_launch_weights(e->st, n_blocks, block_size, g.n_sites_pad, d_mult, e->d_ws, nullptr);
    ngd_launch_planes(e->st, e->d_ws, g.n_sites, g.n_words, n_planes, e->planes);
  }
  ngd_launch_count(e->st, g, e->mask, e->planes, n_planes, e->d_tiles, e->n_tiles, d_cnt);
}

// pairs outside this engine's shard are returned as 0 / 0; an engine that owns every pair overwrites them all
// (a device memset moves ~0.15 TB/s: 0.8 ms for the 130 MB of a 65-matrix cfg 5 batch).  counts_add: the counts are
// added to what is there (k_count adds with integer atomics)
static int zero_outputs(ngd_engine *e, uint32_t n_mat, double *d_sum, unsigned long long *d_cnt, bool counts_add) {
  const uint64_t n = (uint64_t)n_mat * ngd_n_pairs(e->g.n_ind);
  if (e->cfg.shard_world > 1) HIPCHK(hipMemsetAsync(d_sum, 0, n * sizeof(double), e->st));
  if (e->cfg.shard_world > 1 || counts_add) HIPCHK(hipMemsetAsync(d_cnt, 0, n * sizeof(unsigned long long), e->st));
  return NGD_OK;
}

// The MFMA kernel met a block whose shape it has no code path for (its sums are NaN): the run fails, loudly.
int mfma_fault(ngd_engine *e) {
  if (!e->h_clk || !((volatile unsigned long long *)e->h_clk)[2]) return NGD_OK;
  e->h_clk[2] = 0;
  return fail(NGD_E_HIP, "accum_mfma: a block shape the kernel does not list (its sums were set to NaN)");
}

void read_timing(ngd_engine *e, uint64_t n_eff, uint32_t launches, bool add) {
  if (e->d_emcnt) {  // the stream is idle: counters of the pass(es) since the last read
    unsigned long long c[4] = {0, 0, 0, 0};
    if (hipMemcpy(c, e->d_emcnt, sizeof(c), hipMemcpyDeviceToHost) == hipSuccess) {
      if (!add) e->em_counts[0] = e->em_counts[1] = 0;
      e->em_counts[0] += c[0]; e->em_counts[1] += c[1];
      if (c[3]) e->clk_mhz = (double)c[2] / (double)c[3] * e->wall_khz * 1e-3;
      hipMemsetAsync(e->d_emcnt, 0, sizeof(c), e->st);
    }
  }
  if (e->d_clk && launches) {  // (the stream is idle: the sampling wavefront's stores have landed)
    const unsigned long long c0 = ((volatile unsigned long long *)e->h_clk)[0], c1 = ((volatile unsigned long long *)e->h_clk)[1];
    if (c1) e->clk_mhz = (double)c0 / (double)c1 * e->wall_khz * 1e-3;
  }
  float ms[4] = {0, 0, 0, 0};
  hipEventElapsedTime(&ms[0], e->ev[0], e->ev[4]);
  hipEventElapsedTime(&ms[1], e->ev[1], e->ev[2]);
  hipEventElapsedTime(&ms[2], e->ev[2], e->ev[3]);
  hipEventElapsedTime(&ms[3], e->ev[3], e->ev[4]);
  ngd_timing &t = e->timing;
  if (!add) t = ngd_timing{};
  t.ms_total += ms[0]; t.ms_accum += ms[1]; t.ms_reduce += ms[2]; t.ms_count += ms[3];
  t.pair_sites += e->n_owned_pairs * n_eff;
  t.launches += launches;
}

// One accumulation pass over the resident data set: the full data set (mult == NULL) or one bootstrap
// replicate given as block multiplicities (applied inside the accumulation kernel).
// note: the plain pass in its noting form (NGD_OPT_EM_EXACT); pass_impl then rechecks what it noted
static int pass_once(ngd_engine *e, const uint32_t *mult, uint32_t mult_max, uint64_t n_blocks, uint64_t block_size,
                     uint64_t n_drawn, double *d_sum, unsigned long long *d_cnt, bool add_timing, bool note) {
  const ngd_geom &g = e->g;
  uint64_t n_eff = g.n_sites;
  const uint32_t *ws = nullptr;
  uint32_t n_list = 0;
  bool unit_skip = false;
  const bool list_pass = mult && e->kernel == NGD_KERNEL_MFMA && !e->single_image;
  HIPCHK(hipEventRecord(e->ev[0], e->st));
  if (mult) {
    n_eff = n_blocks * block_size;
    if (int rc = e->d_mult.ensure(e, n_blocks)) return rc;
    HIPCHK(hipMemcpyAsync(e->d_mult, mult, n_blocks * 4, hipMemcpyHostToDevice, e->st));
    ngd_launch_weights(e->st, n_blocks, block_size, g.n_sites_pad, e->d_mult, e->d_ws, e->d_wk, e->congruent ? e->sc.d : nullptr);
    if (list_pass) {  // the k-groups this replicate visits at all (about 1/e of the sites are not drawn)
      const uint32_t nb = ngd_kg_count_blocks(g.n_kg);
      if (!e->d_kgl) {
        int rc = e->d_kgl.alloc(e, g.n_kg + NGD_KG_LIST_PAD, false);
        if (rc) return rc;
        rc = e->d_kgcnt.alloc(e, (uint64_t)nb + 1, false);
        if (rc) return rc;
      }
      ngd_launch_kg_compact(e->st, e->d_wk, g.n_kg, (uint32_t)g.n_kg, e->d_kgcnt, e->d_kgl);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(&n_list, e->d_kgcnt + nb, sizeof(uint32_t), hipMemcpyDeviceToHost, e->st));
    }
    HIPCHK(hipStreamSynchronize(e->st));  // `mult` is pageable host memory; n_list has arrived
    ws = e->d_ws;
  }
  if (int rc = zero_outputs(e, 1, d_sum, d_cnt, e->cfg.pairwise_del)) return rc;
  if (note)
    if (int rc = em_exact_begin(e)) return rc;
  HIPCHK(hipEventRecord(e->ev[1], e->st));
  int rc_acc = NGD_OK;
  pass_slices ps;
  ps.w = ws; ps.sites_eff = n_eff; ps.n_ks = e->n_ks; ps.slab = e->slab;
  // a congruent image of a *unit* data set (ngd_commit): the k-groups of t0 = p0 + p1 + p2 multiply ones by ones -- the
  // plain pass walks the list of the others, a third shorter, and the reduction adds d_0 (n + E_i + E_j) (NGD_OPT_UNIT_SKIP)
  unit_skip = !mult && e->kernel == NGD_KERNEL_MFMA && e->d_kgskip && e->unit_ok && e->opt_unit_skip && !e->single_image;
  const double fix_mean = unit_skip ? NGD_FIX_MEAN_UNIT : NGD_FIX_MEAN;
  if (!mult && e->eager_valid && e->eager_slices && e->eager_skip != unit_skip)
    if (int rc = eager_discard(e)) return rc;  // (slices of the other kind of plain pass)
  if (e->kernel == NGD_KERNEL_STREAM)
    ngd_launch_accum_stream(e->st, g, e->PI, ws, n_eff, e->sc, e->cfg.pairwise_del,
                            e->cfg.shard_world > 1 ? e->d_pairs : nullptr, e->n_owned_pairs, d_sum);
  else if (list_pass) {  // slices are equal shares of the list (whole multiples of 4 entries: the deepest operand ring)
    ps.kgl = e->d_kgl; ps.per_slice = (((uint64_t)n_list + e->n_ks - 1) / e->n_ks + 3) / 4 * 4; ps.kg_lim = n_list;
    rc_acc = launch_accumulate(e, ps);
  } else if (!mult && e->eager_valid && e->eager_slices) {
    // the leading slices were accumulated beside the load (eager_advance): what is left, behind them
    HIPCHK(hipStreamWaitEvent(e->st, e->ev_eager, 0));
    if (e->eager_slices < e->n_ks) launch_plain_slices(e, e->st, e->eager_slices, e->n_ks - e->eager_slices, false, unit_skip);
    e->eager_valid = false;
    e->eager_slices = 0;
  } else {
    ps.per_slice = e->per_slice; ps.kg_lim = g.n_kg; ps.note = note;
    if (unit_skip) { ps.kgl = e->d_kgskip; ps.per_slice = e->skip_per_slice; ps.kg_lim = e->n_kgskip; }
    rc_acc = launch_accumulate(e, ps);
  }
  if (!mult) e->plain_kg = e->kernel != NGD_KERNEL_MFMA ? 0 : unit_skip ? e->n_kgskip : g.n_kg;
  if (rc_acc) return rc_acc;
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(e->ev[2], e->st));
  // (without --pairwise_del the reduction writes the counts too: every pair visits the same number of sites)
  const bool cnt_in_reduce = e->kernel != NGD_KERNEL_STREAM && !e->cfg.pairwise_del;
  const bool fix = e->SM != nullptr;  // (a congruent single-image MFMA engine on one of the reference's matrices)
  const ngd_fix_flags ff{e->d_fixlist, e->d_fixcount, e->d_fixseen, e->fix_cap};
  // (--pairwise_del: the pairs that want the fix-up are noted once their valid-site counts are known, below)
  const bool fix_in_reduce = fix && !e->cfg.pairwise_del;
  if (fix) HIPCHK(hipMemsetAsync(e->d_fixcount, 0, sizeof(uint32_t), e->st));
  if (e->kernel != NGD_KERNEL_STREAM)
    ngd_launch_reduce(e->st, g, e->slab, e->n_ks, 1, e->d_tiles, e->n_tiles, d_sum, cnt_in_reduce ? d_cnt : nullptr,
                      mult ? n_drawn : n_eff, fix_in_reduce ? &ff : nullptr, fix_mean * (double)(mult ? n_drawn : n_eff),
                      unit_skip ? e->d_unitE.get() : nullptr, e->sc.d[0] * (double)g.n_sites, e->sc.d[0]);
  if (fix_in_reduce) HIPCHK(hipMemcpyAsync(e->h_fixcount, e->d_fixcount, sizeof(uint32_t), hipMemcpyDeviceToHost, e->st));
  HIPCHK(hipEventRecord(e->ev[3], e->st));
  if (e->cfg.pairwise_del) {
    // (no block drawn -- a site range of a larger job: one all-zero plane, count_planes)
    if (ws) ngd_launch_planes(e->st, ws, g.n_sites, g.n_words, count_planes(mult_max), e->planes);
    ngd_launch_count(e->st, g, e->mask, e->planes, ws ? count_planes(mult_max) : 0, e->d_tiles, e->n_tiles, d_cnt);
    if (fix) {
      ngd_launch_fix_flag(e->st, g, d_sum, d_cnt, 1, e->d_tiles, e->n_tiles, ff);
      HIPCHK(hipMemcpyAsync(e->h_fixcount, e->d_fixcount, sizeof(uint32_t), hipMemcpyDeviceToHost, e->st));
    }
  } else if (!cnt_in_reduce) {
    ngd_launch_fill_cnt(e->st, g, e->d_tiles, e->n_tiles, mult ? n_drawn : n_eff, nullptr, 1, d_cnt);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(e->ev[4], e->st));
  HIPCHK(hipStreamSynchronize(e->st));
  read_timing(e, n_eff, 1, add_timing);
  if (int rc = mfma_fault(e)) return rc;
  if (unit_skip && *(volatile uint32_t *)e->h_fixcount) {
    // Without the +1/2 of every site the accumulators run to -(sites of a slice) / 2, and a sum carries 2^-53 of that per
    // rounding: fine for every sum above NGD_FIX_MEAN_UNIT per site, not for the tiny sums of nearly identical individuals
    // -- which the fix-up pass, and a caller who budgets it, are promised at the full pass's 4e-17 per site.  A data set
    // that holds such a pair is not one for this pass: it is run whole, now and from now on (until the next ngd_commit).
    e->unit_ok = false;
    return pass_once(e, mult, mult_max, n_blocks, block_size, n_drawn, d_sum, d_cnt, true, note);
  }
  if (fix)
    return fixup_pass(e, ws, n_eff, d_sum, 0, 0, nullptr, e->cfg.pairwise_del ? d_cnt : nullptr,
                      fix_mean * (double)(mult ? n_drawn : n_eff));
  return NGD_OK;
}

int pass_impl(ngd_engine *e, const uint32_t *mult, uint32_t mult_max, uint64_t n_blocks, uint64_t block_size,
              uint64_t n_drawn, double *d_sum, unsigned long long *d_cnt, bool add_timing) {
  // (value 1 refuses every call but the plain pass, and the eager pass: em_exact_refuse, ngd_set_option; value 2 serves the
  // weighted calls by plans of its own, run_impl, and never by a weighted pass of this kind)
  const bool note = e->opt_em_exact && !mult && e->kernel == NGD_KERNEL_EM_TABLE;
  int rc = pass_once(e, mult, mult_max, n_blocks, block_size, n_drawn, d_sum, d_cnt, add_timing, note);
  if (rc || !note) return rc;
  // what the pass noted, rechecked on the host before any sum leaves the engine.  A list that was too short has counted
  // what it needs: it grows to that and the pass runs once more (the count is a function of the data: it fits then)
  bool again = false;
  if ((rc = em_exact_finish(e, d_sum, &again))) return rc;
  if (again) {
    if ((rc = pass_once(e, mult, mult_max, n_blocks, block_size, n_drawn, d_sum, d_cnt, add_timing, true))) return rc;
    if ((rc = em_exact_finish(e, d_sum, &again))) return rc;
    if (again) return fail(NGD_E_HIP, "NGD_OPT_EM_EXACT: internal -- the second pass noted more than the first counted");
    e->exact_info.passes = 2;
  }
  return NGD_OK;
}

// Bootstrap by per-block partials: every site's contribution is independent of the
// replicate, so sum_rep = SUM_b multiplicity_rep[b] * S_b with S_b the block's partial sum (and the same
// for the valid-site counts).  One accumulation pass fills S_b; replicates are then weighted reductions of
// the partials, up to 32 per pass over them.  MFMA slices are whole k-groups of 4 contraction indices, so
// blocks must be multiples of 4 sites there.  *feasible = false: the caller falls back to pass_impl().
// note (NGD_OPT_EM_EXACT = 2, table-driven EM kernel): the pass over the blocks runs in its noting form, into e->d_note, in
// THIS call -- cached partial sums carry no list, and the slab this call fills is not named as the cache afterwards (it
// holds unpatched terms of the widened threshold) -- and the matrices stay on the device until the caller has patched them
// (no copies queued from here); the weights stay in e->d_W: W[(block * sub) * stride + r], stride = the matrices rounded up to ngd_reduce_chunk.
static int partials_impl(ngd_engine *e, const uint32_t *mult /*[n_rep][n_blocks]*/, const unsigned long long *drawn,
                         uint32_t n_rep, uint64_t n_blocks, uint64_t block_size, double *d_sum,
                         unsigned long long *d_cnt, bool *feasible, bool note = false) {
  const ngd_geom &g = e->g;
  const uint64_t n_pairs = ngd_n_pairs(g.n_ind);
  const uint64_t n_eff = n_blocks * block_size;
  const uint64_t plane = (uint64_t)g.n_pad * g.n_pad;
  const bool mfma = e->kernel == NGD_KERNEL_MFMA;
  const bool pdel = e->cfg.pairwise_del != 0;
  *feasible = false;
  if (e->kernel == NGD_KERNEL_STREAM || !e->opt_boot_partials) return NGD_OK;
  // MFMA slices are whole k-groups of 4 contraction indices; a block of B sites is 3 B of them.  Blocks that are not
  // whole k-groups become slices of every k-group they touch, the shared first / last k-group masked per slice.
  const bool unaligned = mfma && block_size % 4 != 0;
  if (unaligned && !e->opt_boot_unaligned) return NGD_OK;
  if (n_blocks >= (1ull << 31)) return NGD_OK;
  // split large blocks so that there are enough workgroups; slices of one block share its weight
  const uint64_t unit = mfma ? 3 * block_size / 4 : block_size;  // k-groups or sites per block
  const bool cached = !note && e->blk.has_sums(block_size, n_blocks);
  uint64_t sub = 1, nks = 0;
  if (cached) {
    sub = e->blk.sub;
    nks = e->blk.nks;
  } else {
    const uint32_t tiles_n = mfma ? std::max(1u, e->n_wg / (e->exact_shapes && e->exact_shapes < 3 ? 4 : 1))
                                  : e->kernel == NGD_KERNEL_EM_TABLE ? e->n_tiles64 : e->n_tiles16;
    const uint64_t want = e->opt_boot_wg;
    while (!unaligned && tiles_n && (uint64_t)tiles_n * n_blocks * sub < want && unit % (sub * 2) == 0 &&
           unit / (sub * 2) >= 32)
      sub *= 2;
    nks = n_blocks * sub;
    if (mfma) nks = (nks + 7) / 8 * 8;  // the XCD deal of accum_mfma.hip
  }
  if (nks >= (1ull << 31)) return NGD_OK;
  const uint64_t elems = nks * plane, c_elems = pdel ? n_blocks * plane : 0;
  const bool c_cached = !pdel || e->blk.has_counts(block_size, n_blocks);
  if (!cached || !c_cached) {
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    const uint64_t need = elems * 8 + c_elems * 4;
    const uint64_t have = e->blk.bytes();
    // default budget: most of what the device has left -- one pass over a slab of tens of GB still beats
    // hundreds of accumulation passes
    const uint64_t budget = e->opt_boot_max_bytes ? e->opt_boot_max_bytes : (uint64_t)((free_b + have) / 100 * 85);
    if (need > budget) return NGD_OK;
    if ((elems > e->blk.sums().capacity() || c_elems > e->blk.counts().capacity()) && need + (1ull << 30) > free_b + have)
      return NGD_OK;
    const double alloc_ms = need > have ? (double)(need - have) * 12e-9 : 0.0;
    if (alloc_ms > 20.0 && e->opt_boot_partials < 2) {
      // what this call costs without the partials: a list-driven pass per replicate (MFMA, ~3/4 of a pass)
      // or a batch pass per 16 replicates (EM); rates are the measured ones of DESIGN.md section 6
      const double ps = (double)e->n_owned_pairs * (double)n_eff;
      const bool table = e->kernel == NGD_KERNEL_EM_TABLE;
      const double pass_ms = mfma ? ps / 1.05e10 : table ? ps / 1.9e8 : e->kernel == NGD_KERNEL_EM_FAST ? ps / 7.5e7 : ps / 3.8e6;
      // (the table-driven kernel's spilled-terms plan, em_spill_impl: ONE EM pass + a contraction whatever the replicate
      // count -- [measured, round 6] without this term the engine bought an 84 GB slab for a single job of 10 000 blocks of
      // 10 sites, 3 ms on a device nobody has used and 5.8 s on one that has just been busy)
      const bool spill = table && e->em_shape == 0 && e->opt_em_spill && n_rep >= (e->opt_em_spill == 2 ? 2u : 3u);
      const double alt_ms = mfma ? 0.75 * pass_ms * n_rep
                            : spill ? 1.1 * pass_ms
                            : table ? std::min(0.65 * pass_ms * n_rep, 2.9 * pass_ms * ((n_rep + 15) / 16))
                                    : 1.1 * pass_ms * ((n_rep + 15) / 16);
      if (e->rent_B != block_size || e->rent_blocks != n_blocks) {
        e->rent_B = block_size; e->rent_blocks = n_blocks; e->rent_ms = 0;
      }
      if (e->rent_ms + alt_ms < alloc_ms) {
        e->rent_ms += alt_ms;
        return NGD_OK;
      }
    }
  }
  *feasible = true;
  if (e->out.on && out_trace()) fprintf(stderr, "[out] plan settled %.3f ms into the call\n", out_now() - e->out.t_call);

  HIPCHK(hipEventRecord(e->ev[0], e->st));
  uint32_t launches = 0;
  HIPCHK(hipEventRecord(e->ev[1], e->st));
  if (!cached) {
    int rc = e->blk.borrow_sums().ensure(e, elems);
    if (rc) return rc;
    e->blk.nks = (uint32_t)nks;
    e->blk.sub = (uint32_t)sub;
    e->blk.per_slice = unit / sub;
    pass_slices ps;  // a slice = a block (or an equal part of one)
    ps.sites_eff = n_eff; ps.n_ks = e->blk.nks; ps.slab = e->blk.sums();
    if (unaligned && e->congruent) {
      // the congruent image: a block's sites occupy whole periods of four sites (ngd_layout.h), which the kernel's own
      // k_per_slice arithmetic does not know -- the slices go by table, as the windows' segments do (win_plan.h): slice b =
      // the k-groups of block b, its weights d[coordinate] on the block's sites and 0 on the others the periods hold
      std::vector<uint64_t> tab;
      tab.reserve((size_t)e->blk.nks * NGD_SEG_STRIDE);
      uint64_t wkg = 0, max_wkg = 0;
      for (uint64_t b = 0; b < n_blocks; b++) {
        const uint64_t s_lo = b * block_size, s_hi = s_lo + block_size;
        const uint64_t kg0 = ngd_kg_lo(s_lo, 1), kg1 = ngd_kg_hi(s_hi, 1), n_wkg = kg1 - kg0 + 1 + NGD_KG_TAIL;
        tab.insert(tab.end(), {kg0, kg1, wkg, s_lo, s_hi});
        wkg += n_wkg;
        max_wkg = std::max(max_wkg, n_wkg);
      }
      for (uint64_t k = n_blocks; k < e->blk.nks; k++) tab.insert(tab.end(), {0, 0, wkg, 0, 0});  // (the XCD deal's padding slices)
      max_wkg = std::max<uint64_t>(max_wkg, 1 + NGD_KG_TAIL);
      rc = e->blk.wslice.ensure(e, (wkg + 1 + NGD_KG_TAIL) * 4);
      if (!rc) rc = e->d_segtab.ensure(e, tab.size());
      if (rc) return rc;
      HIPCHK(hipMemcpy(e->d_segtab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice));
      ngd_launch_seg_weights(e->st, e->d_segtab, e->blk.nks, max_wkg, e->sc.d, e->blk.wslice);
      ps.kg_lim = g.n_kg; ps.seg = e->d_segtab;
    } else if (unaligned) {
      const uint32_t w_stride = (uint32_t)((3 * block_size + 3) / 4 + 1 + NGD_KG_TAIL);
      rc = e->blk.wslice.ensure(e, (uint64_t)e->blk.nks * w_stride * 4);
      if (rc) return rc;
      ngd_launch_slice_weights(e->st, e->blk.nks, w_stride, 3 * block_size, 3 * n_eff, e->blk.wslice);
      ps.kg_lim = (3 * n_eff + 3) / 4; ps.k_per_slice = 3 * block_size; ps.w_stride = w_stride;
    } else {
      if (note && (rc = em_exact_begin(e))) return rc;
      ps.per_slice = e->blk.per_slice; ps.kg_lim = mfma ? 3 * n_eff / 4 : 0; ps.note = note;
    }
    rc = launch_accumulate(e, ps);
    if (rc) return rc;
    HIPCHK(hipGetLastError());
    // (a slab the noting form filled is not the cache: it stops in-band pairs at the widened threshold, and only the
    // matrices are patched -- an option-off job must never be reduced from it; borrow_sums() above dropped the key)
    if (!note) e->blk.sums_filled(block_size, n_blocks);
    launches = 1;
  }
  HIPCHK(hipEventRecord(e->ev[2], e->st));

  // W[slice][r]: slice-major, so that the replicates of one pass read their weights of a slice together
  const uint32_t stride = (n_rep + ngd_reduce_chunk(n_rep) - 1) / ngd_reduce_chunk(n_rep) * ngd_reduce_chunk(n_rep);
  const uint64_t n_slices = n_blocks * sub;  // the slab's padding slices (MFMA deal) are never read
  std::vector<double> W(n_slices * stride, 0.0);
  for (uint32_t r = 0; r < n_rep; r++)
    for (uint64_t b = 0; b < n_blocks; b++) {
      const double m = (double)mult[(uint64_t)r * n_blocks + b];
      if (m != 0.0)
        for (uint64_t q = 0; q < sub; q++) W[(b * sub + q) * stride + r] = m;
    }
  int rc = e->d_W.ensure(e, W.size());
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(e->d_W, W.data(), W.size() * 8, hipMemcpyHostToDevice, e->st));
  // (the weighted reductions write every pair this engine owns, sums and counts)
  if ((rc = zero_outputs(e, n_rep, d_sum, d_cnt, false))) return rc;
  const bool fix = e->SM != nullptr && mfma;  // (see pass_impl)
  const ngd_fix_flags ff{e->d_fixlist, e->d_fixcount, e->d_fixseen, e->fix_cap};
  std::vector<double> thr;
  if (fix) {  // a pair is noted if its sum in ANY matrix is below NGD_FIX_MEAN x the sites that matrix visits
    thr.resize(n_rep);
    for (uint32_t r = 0; r < n_rep; r++) thr[r] = NGD_FIX_MEAN * (double)drawn[r];
    rc = e->d_fixthr.ensure(e, (uint64_t)n_rep);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(e->d_fixthr, thr.data(), (uint64_t)n_rep * 8, hipMemcpyHostToDevice, e->st));
    HIPCHK(hipMemsetAsync(e->d_fixcount, 0, sizeof(uint32_t), e->st));
    HIPCHK(hipMemsetAsync(e->d_fixseen, 0, (n_pairs / 32 + 1) * sizeof(uint32_t), e->st));
  }
  const bool fix_in_reduce = fix && !pdel;  // (--pairwise_del: noted once the counts are known, below)
  std::vector<uint32_t> M;
  // the counts' inputs: --pairwise_del, the per-block counts (made if not cached) and the multiplicities M[block][r]; else
  // the sites every matrix visits, filled in at once
  auto counts_inputs = [&]() -> int {
    if (pdel) {
      if (!c_cached) {
        int rc = e->blk.borrow_counts().ensure(e, c_elems);
        if (rc) return rc;
        ngd_launch_count_blocks(e->st, g, e->mask, block_size, (uint32_t)n_blocks, e->d_tiles16, e->n_tiles16, e->blk.counts());
        HIPCHK(hipGetLastError());
        e->blk.counts_filled(block_size, n_blocks);
      }
      M.assign(n_blocks * stride, 0u);
      for (uint32_t r = 0; r < n_rep; r++)
        for (uint64_t b = 0; b < n_blocks; b++) M[b * stride + r] = mult[(uint64_t)r * n_blocks + b];
      if (int rc = e->d_M.ensure(e, M.size())) return rc;
      HIPCHK(hipMemcpyAsync(e->d_M, M.data(), M.size() * 4, hipMemcpyHostToDevice, e->st));
    } else {
      if (int rc = e->d_drawn.ensure(e, (uint64_t)n_rep)) return rc;
      HIPCHK(hipMemcpyAsync(e->d_drawn, drawn, (uint64_t)n_rep * 8, hipMemcpyHostToDevice, e->st));
      ngd_launch_fill_cnt(e->st, g, e->d_tiles, e->n_tiles, 0, e->d_drawn, n_rep, d_cnt);
    }
    return NGD_OK;
  };
  // ngd_run_*_dist, the job's first matrix at the head of d_bsum: a group of replicates is reduced by a launch of its own
  // and its copy to the host queued behind it, so that the copies run beside the later groups' reductions
  const bool stream_out = !note && e->out.on && d_sum == e->d_bsum && d_cnt == e->d_bcnt && e->out.queued == 0;
  if (stream_out) {
    // the counts' inputs first: they do not depend on the sums
    if ((rc = counts_inputs())) return rc;
    const uint32_t rb = ngd_reduce_chunk(n_rep);
    for (uint32_t r0 = 0; r0 < n_rep; r0 += rb) {
      const uint32_t n = std::min(rb, n_rep - r0);
      ngd_launch_reduce_w(e->st, g, e->blk.sums(), (uint32_t)n_slices, e->d_W + r0, stride, n, e->d_tiles, e->n_tiles,
                          d_sum + (uint64_t)r0 * n_pairs, fix_in_reduce ? &ff : nullptr, e->d_fixthr ? e->d_fixthr + r0 : nullptr, rb);
      if (r0 + rb >= n_rep) HIPCHK(hipEventRecord(e->ev[3], e->st));
      if (pdel)
        ngd_launch_reduce_c(e->st, g, e->blk.counts(), (uint32_t)n_blocks, e->d_M + r0, stride, n, e->d_tiles, e->n_tiles,
                            d_cnt + (uint64_t)r0 * n_pairs, rb);
      HIPCHK(hipGetLastError());
      if ((rc = out_queue(e, r0 + n))) return rc;
    }
    if (fix && pdel) ngd_launch_fix_flag(e->st, g, d_sum, d_cnt, n_rep, e->d_tiles, e->n_tiles, ff);
    if (fix) HIPCHK(hipMemcpyAsync(e->h_fixcount, e->d_fixcount, sizeof(uint32_t), hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->ev[4], e->st));
    // the host's threads are woken once the first group has been reduced: its first chunk is about to land
    const double t_q = out_now();
    HIPCHK(hipEventSynchronize(e->out.pool[0]));
    const double t_g = out_now();
    out_start_finisher(e);
    if (out_trace()) fprintf(stderr, "[out] queued %.3f ms into the call, first group reduced +%.3f ms, finisher started +%.3f\n", t_q - e->out.t_call, t_g - t_q, out_now() - t_q);
    e->out.t0 = t_q;
    // ... and chunks are declared landed as they arrive while the later groups are still being reduced -- before it is known
    // whether the fix-up pass will patch the partial results (it rarely does: then every matrix is copied and finished again)
    for (;;) {
      const hipError_t q = hipEventQuery(e->ev[4]);
      if (q == hipSuccess) break;
      if (q != hipErrorNotReady) HIPCHK(q);
      if ((rc = out_advance(e))) return rc;
      __builtin_ia32_pause();
    }
  } else {
    ngd_launch_reduce_w(e->st, g, e->blk.sums(), (uint32_t)n_slices, e->d_W, stride, n_rep, e->d_tiles, e->n_tiles, d_sum,
                        fix_in_reduce ? &ff : nullptr, e->d_fixthr);
    if (fix_in_reduce) HIPCHK(hipMemcpyAsync(e->h_fixcount, e->d_fixcount, sizeof(uint32_t), hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->ev[3], e->st));

    if ((rc = counts_inputs())) return rc;
    if (pdel) {
      ngd_launch_reduce_c(e->st, g, e->blk.counts(), (uint32_t)n_blocks, e->d_M, stride, n_rep, e->d_tiles, e->n_tiles, d_cnt);
      if (fix) {
        ngd_launch_fix_flag(e->st, g, d_sum, d_cnt, n_rep, e->d_tiles, e->n_tiles, ff);
        HIPCHK(hipMemcpyAsync(e->h_fixcount, e->d_fixcount, sizeof(uint32_t), hipMemcpyDeviceToHost, e->st));
      }
    }
  }
  HIPCHK(hipGetLastError());
  if (!stream_out) HIPCHK(hipEventRecord(e->ev[4], e->st));
  HIPCHK(hipStreamSynchronize(e->st));  // W, M, drawn are host temporaries
  if (stream_out && out_trace()) fprintf(stderr, "[out] engine stream drained +%.3f\n", out_now() - e->out.t0);
  read_timing(e, n_eff, launches, false);
  if ((rc = mfma_fault(e))) return rc;
  if (fix) {  // the noted pairs' partial results exactly, then the replicates again from the patched slab
    bool patched = false;
    rc = fixup_pass(e, nullptr, n_eff, nullptr, block_size / sub, (uint32_t)n_slices, &patched);
    if (rc) return rc;
    if (patched) {
      if (stream_out && (rc = out_requeue(e))) return rc;  // (what has been copied so far: sums from before the patch)
      ngd_launch_reduce_w(e->st, g, e->blk.sums(), (uint32_t)n_slices, e->d_W, stride, n_rep, e->d_tiles, e->n_tiles, d_sum);
      HIPCHK(hipGetLastError());
      HIPCHK(hipStreamSynchronize(e->st));
    }
  }
  return NGD_OK;
}

// EM path when the blocks are too many for per-block partials (e.g. the reference's default block size 1):
// the EM of a (pair, site) does not depend on the replicate, so up to 16 replicates share ONE accumulation pass
// (accum_em.hip k_accum_em_batch) -- and, with lead_full, so does the full-data matrix, as the row whose weight
// is 1 on every site.  Outputs: [lead_full + n_rep][n_pairs]; a replicate's bits equal the one-replicate pass's.
static int em_batch_impl(ngd_engine *e, const uint32_t *mult, const uint32_t *mult_max, const unsigned long long *drawn,
                         uint32_t n_rep, bool lead_full, uint64_t n_blocks, uint64_t block_size, double *d_sum,
                         unsigned long long *d_cnt, bool add_timing) {
  const ngd_geom &g = e->g;
  const uint64_t n_pairs = ngd_n_pairs(g.n_ind), plane = (uint64_t)g.n_pad * g.n_pad;
  const uint64_t n_eff = n_blocks * block_size;
  const uint32_t n_mat = n_rep + (lead_full ? 1u : 0u);
  const bool fast = e->kernel != NGD_KERNEL_EM_FAITHFUL;
  // the table-driven kernel's own batch form (its default shape): 8 matrices per pass, one workgroup per CU (the 8 x 8
  // accumulators of a wavefront take the registers of a second one)
  const bool table = e->kernel == NGD_KERNEL_EM_TABLE && e->em_shape == 0;
  const uint32_t per_pass = table ? 8 : 16;
  // slices of the per-pair batch kernel: the engine's own when that is its kernel, else (table-driven engine in
  // another shape) what ngd_create() would have picked for it
  uint32_t b_ks = e->n_ks;
  uint64_t b_per = e->per_slice;
  if (table) {
    // the plain pass's own slices: a matrix then adds up in the same order from either (same bits)
  } else if (e->kernel == NGD_KERNEL_EM_TABLE) {
    uint64_t ks = e->n_tiles16 ? (4096 + e->n_tiles16 - 1) / e->n_tiles16 : 1;
    ks = std::max<uint64_t>(1, std::min(ks, std::max<uint64_t>(1, g.n_sites / 256)));
    b_ks = (uint32_t)ks;
    b_per = (g.n_sites + ks - 1) / ks;
  }
  if (int rc = zero_outputs(e, n_mat, d_sum, d_cnt, e->cfg.pairwise_del)) return rc;
  DevBuf<double> &slab = e->blk.borrow_sums();  // the partial-sum slab is re-used as this pass's scratch
  for (uint32_t c0 = 0; c0 < n_mat; c0 += per_pass) {
    const uint32_t nr = std::min(per_pass, n_mat - c0);
    const int rb = nr <= 4 ? 4 : nr <= 8 ? 8 : 16;
    const bool lead = lead_full && c0 == 0;
    const uint32_t q0 = c0 - ((lead_full && c0 > 0) ? 1u : 0u);  // first replicate of the chunk
    const uint32_t nq = nr - (lead ? 1u : 0u);                     // replicates in the chunk
    if (e->opt_boot_max_bytes && (uint64_t)b_ks * rb * plane * 8 > e->opt_boot_max_bytes)  // the caller's scratch budget
      return fail(NGD_E_NOMEM, "EM batch pass: result planes exceed NGD_OPT_BOOT_MAX_BYTES");
    const uint64_t want = (uint64_t)b_ks * rb * plane;
    if (e->em_batch_nofit_elems && want >= e->em_batch_nofit_elems && want > slab.capacity())
      return fail(NGD_E_NOMEM, "EM batch pass: result planes of this size did not fit the device before");
    int rc = slab.ensure(e, want);
    if (rc == NGD_E_NOMEM && !e->opt_boot_max_bytes) e->em_batch_nofit_elems = want;  // the device's verdict: remembered
    if (rc) return rc;
    rc = e->d_W.ensure(e, g.n_sites * (uint64_t)rb);
    if (!rc) rc = e->d_M.ensure(e, std::max<uint64_t>(1, (uint64_t)nq * n_blocks));
    if (rc) return rc;
    HIPCHK(hipEventRecord(e->ev[0], e->st));
    if (nq) HIPCHK(hipMemcpyAsync(e->d_M, mult + (uint64_t)q0 * n_blocks, (uint64_t)nq * n_blocks * 4, hipMemcpyHostToDevice, e->st));
    ngd_launch_weights_batch(e->st, e->d_M, nq, (uint32_t)rb, lead ? 1 : 0, n_blocks, block_size, g.n_sites, g.n_sites,
                             e->d_W);
    HIPCHK(hipEventRecord(e->ev[1], e->st));
    if (table)
      ngd_launch_accum_em_table_batch(e->st, emt_common(e), e->d_W, rb, lead ? g.n_sites : n_eff, b_ks, b_per, slab);
    else
      ngd_launch_accum_em_batch(e->st, g, e->PA, e->d_W, rb, lead ? g.n_sites : n_eff, e->sc, e->cfg.pairwise_del, fast,
                                e->d_tiles16, e->n_tiles16, b_ks, b_per, slab);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->ev[2], e->st));
    for (uint32_t r = 0; r < nr; r++)
      ngd_launch_reduce(e->st, g, slab + (uint64_t)r * plane, b_ks, (uint32_t)rb, e->d_tiles, e->n_tiles,
                        d_sum + (uint64_t)(c0 + r) * n_pairs);
    HIPCHK(hipEventRecord(e->ev[3], e->st));
    for (uint32_t r = 0; r < nr; r++) {
      unsigned long long *cnt_r = d_cnt + (uint64_t)(c0 + r) * n_pairs;
      const bool is_lead = lead && r == 0;
      const uint32_t q = q0 + r - (lead ? 1u : 0u);
      if (!e->cfg.pairwise_del)
        ngd_launch_fill_cnt(e->st, g, e->d_tiles, e->n_tiles, is_lead ? g.n_sites : drawn[q], nullptr, 1, cnt_r);
      else
        count_matrix(e, is_lead ? nullptr : e->d_M + (uint64_t)(q - q0) * n_blocks, is_lead ? 0 : mult_max[q], n_blocks, block_size, cnt_r);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->ev[4], e->st));
    HIPCHK(hipStreamSynchronize(e->st));
    read_timing(e, lead ? g.n_sites : n_eff, 1, add_timing || c0 > 0);
  }
  return NGD_OK;
}

// EM path, many matrices, blocks too small for per-block partials: ONE pass of the table-driven EM kernel writes the
// per-(pair, unit of sites) terms of a chunk of sites (they do not depend on the replicate), one FP64 MFMA contraction
// adds the chunk to the running sums of every matrix of the job (contract_mfma.hip).  A unit is q consecutive sites of
// one bootstrap block (q = the block size or its largest divisor up to 64): every matrix weights them alike, so their
// terms are added up before they leave the EM kernel -- the bytes written and read, and the flops of the contraction,
// are those of n_sites / q.  The chunk is as many units as the scratch budget holds (NGD_OPT_EM_SPILL_BYTES).
// Outputs: [lead + n_rep][n_pairs]; every matrix agrees with its own ngd_run() pass to rounding (the sums are formed in
// another order).  *done = false: the plan does not apply (no room for a useful chunk) and nothing has been written.
// note (NGD_OPT_EM_EXACT = 2): the EM pass runs in its noting form (accum_em_table.hip SPILL && NOTE) into e->d_note, which
// is emptied once, before the first chunk -- its count runs on from chunk to chunk; any number of matrices from 1 is
// served, chunks of a few sites too (no other plan of the option could take the call).  The multiplicities stay in e->d_M.
static uint32_t spill_unit(uint64_t block_size) {
  uint32_t q = 1;
  for (uint32_t d = 2; d <= 64 && d <= block_size; d++)
    if (block_size % d == 0) q = d;
  return q;
}

static int em_spill_impl(ngd_engine *e, const uint32_t *mult, const uint32_t *mult_max, const unsigned long long *drawn,
                         uint32_t n_rep, bool lead, uint64_t n_blocks, uint64_t block_size, double *d_sum,
                         unsigned long long *d_cnt, bool *done, bool note = false) {
  const ngd_geom &g = e->g;
  *done = false;
  const uint64_t n_pairs = ngd_n_pairs(g.n_ind);
  const uint64_t n_eff = n_blocks * block_size;
  const uint32_t n_mat = n_rep + (lead ? 1u : 0u);
  const uint32_t n_rg = ngd_contract_rep_groups(n_mat);
  const uint64_t n_pg = e->n_pg_spill;  // groups of 16 pair slots (live groups only, padded to 4)
  const uint64_t s_end = lead ? g.n_sites : n_eff;
  if (!e->n_tiles64 || !n_pg || !e->d_rowpg || !s_end) return NGD_OK;
  const uint32_t q = spill_unit(block_size);
  const uint64_t kg_bytes = n_pg * 64 * 8;  // one k-group (4 units) of terms
  const uint64_t d_elems = (uint64_t)n_rg * n_pg * 256;
  size_t free_b = 0, total_b = 0;
  HIPCHK(hipMemGetInfo(&free_b, &total_b));
  const uint64_t have = e->blk.sums().bytes() + e->d_D.bytes();
  // default scratch: 6 GB of terms (a device allocation costs ~12 ms per GB once; [measured] tools/em_boot_job.py)
  uint64_t budget = e->opt_em_spill_bytes ? e->opt_em_spill_bytes : (6ull << 30);
  if (e->opt_boot_max_bytes) budget = std::min(budget, e->opt_boot_max_bytes);
  const uint64_t room = free_b + have > d_elems * 8 + (2ull << 30) ? free_b + have - d_elems * 8 - (2ull << 30) : 0;
  budget = std::min(budget, room);
  uint64_t chunk_kg = budget / kg_bytes;
  if (chunk_kg < 2) return NGD_OK;
  const uint64_t units_all = (s_end + q - 1) / q;
  chunk_kg = std::min<uint64_t>(chunk_kg - 1, (units_all + 3) / 4);  // (one k-group of tail for the operand run-ahead)
  // chunks of a few sites are launch-bound: the plan is left to the others (unless the caller set the scratch size)
  if (!note && !e->opt_em_spill_bytes && chunk_kg * 4 * q < std::min<uint64_t>(s_end, 64)) return NGD_OK;
  const uint64_t chunk_sites = chunk_kg * 4 * q;
  const uint64_t n_chunks = (s_end + chunk_sites - 1) / chunk_sites;

  DevBuf<double> &C = e->blk.borrow_sums();  // the partial-sum slab is this plan's scratch
  int rc = C.ensure(e, (chunk_kg + 1) * n_pg * 64);
  if (!rc) rc = e->d_W.ensure(e, (chunk_kg + 1) * (uint64_t)n_rg * 64);
  if (!rc) rc = e->d_M.ensure(e, std::max<uint64_t>(1, (uint64_t)n_rep * n_blocks));
  if (!rc) rc = e->d_D.ensure(e, d_elems);
  if (!rc) rc = e->d_nanflag.ensure(e, n_chunks);
  if (rc) return rc;
  while (e->ev_spill.size() < 4 * n_chunks + 1) {  // (kept for the engine's lifetime)
    hipEvent_t v = nullptr;
    HIPCHK(hipEventCreate(&v));
    e->ev_spill.push_back(v);
  }
  if (note && (rc = em_exact_begin(e))) return rc;
  *done = true;

  HIPCHK(hipEventRecord(e->ev[0], e->st));
  if (n_rep) HIPCHK(hipMemcpyAsync(e->d_M, mult, (uint64_t)n_rep * n_blocks * 4, hipMemcpyHostToDevice, e->st));
  HIPCHK(hipMemsetAsync(e->d_D, 0, d_elems * 8, e->st));
  HIPCHK(hipMemsetAsync(e->d_nanflag, 0, n_chunks * 8, e->st));
  if ((rc = zero_outputs(e, n_mat, d_sum, d_cnt, e->cfg.pairwise_del))) return rc;
  HIPCHK(hipEventRecord(e->ev[1], e->st));
  uint64_t units_done = 0;
  for (uint64_t c = 0; c < n_chunks; c++) {
    const uint64_t s_lo = c * chunk_sites, s_hi = std::min(s_end, s_lo + chunk_sites);
    const uint64_t len = s_hi - s_lo, n_units = (len + q - 1) / q, n_kg = (n_units + 3) / 4;
    units_done += n_units;
    hipEvent_t *ev = &e->ev_spill[4 * c];
    HIPCHK(hipEventRecord(ev[0], e->st));
    if (n_units & 3) HIPCHK(hipMemsetAsync(C + (n_kg - 1) * n_pg * 64, 0, kg_bytes, e->st));  // the last k-group is partial
    if (n_pg > e->n_pg_live)  // the slot groups of padding, which no wavefront of the EM pass writes
      HIPCHK(hipMemset2DAsync(C + (uint64_t)e->n_pg_live * 64, kg_bytes, 0, (n_pg - e->n_pg_live) * 512, n_kg, e->st));
    ngd_launch_spill_weights(e->st, e->d_M, n_mat, lead ? 1 : 0, s_lo, s_hi, q, g.n_sites, n_eff, n_blocks, block_size, e->d_W);
    HIPCHK(hipEventRecord(ev[1], e->st));
    // slices of the chunk's sites (whole units): enough workgroups to fill the device a few times over, a few sites each
    // at least
    uint64_t ks = std::max<uint64_t>(1, std::min<uint64_t>((8192 + e->n_tiles64 - 1) / e->n_tiles64, len / 8));
    const uint64_t sps = ((len + ks - 1) / ks + q - 1) / q * q;
    ks = (len + sps - 1) / sps;
    ngd_launch_accum_em_table_spill(e->st, emt_common(e), s_lo, s_hi, (uint32_t)ks, sps, q, e->d_rowpg, (uint32_t)n_pg, C,
                                    e->d_nanflag + c, note ? e->d_note.get() : nullptr);
    HIPCHK(hipEventRecord(ev[2], e->st));
    ngd_launch_spill_sanitize(e->st, C, e->d_nanflag + c, n_kg, (uint32_t)n_pg, e->d_M, n_mat, lead ? 1 : 0, s_lo, q,
                              g.n_sites, n_eff, n_blocks, block_size, e->d_D);
    HIPCHK(hipEventRecord(ev[3], e->st));
    ngd_launch_contract(e->st, e->d_W, C, n_mat, (uint32_t)n_pg, (uint32_t)n_kg, e->d_D);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipEventRecord(e->ev_spill[4 * n_chunks], e->st));
  HIPCHK(hipEventRecord(e->ev[2], e->st));
  ngd_launch_spill_scatter(e->st, e->d_D, (uint32_t)n_pg, e->d_tiles64, e->n_tiles64, e->d_rowpg, g.n_ind, n_mat, d_sum);
  HIPCHK(hipEventRecord(e->ev[3], e->st));
  std::vector<unsigned long long> visited;  // (alive until the synchronisation below)
  if (!e->cfg.pairwise_del) {  // every pair of matrix r counts the sites the matrix visits: one launch for the job
    visited.resize(n_mat);
    for (uint32_t r = 0; r < n_mat; r++) visited[r] = lead && r == 0 ? g.n_sites : drawn[r - (lead ? 1u : 0u)];
    rc = e->d_drawn.ensure(e, (uint64_t)n_mat);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(e->d_drawn, visited.data(), (uint64_t)n_mat * 8, hipMemcpyHostToDevice, e->st));
    ngd_launch_fill_cnt(e->st, g, e->d_tiles, e->n_tiles, 0, e->d_drawn, n_mat, d_cnt);
  }
  for (uint32_t r = 0; r < n_mat && e->cfg.pairwise_del; r++) {
    const bool is_lead = lead && r == 0;
    const uint32_t qr = r - (lead ? 1u : 0u);
    count_matrix(e, is_lead ? nullptr : e->d_M + (uint64_t)qr * n_blocks, is_lead ? 0 : mult_max[qr], n_blocks, block_size,
                 d_cnt + (uint64_t)r * n_pairs);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(e->ev[4], e->st));
  HIPCHK(hipStreamSynchronize(e->st));  // `mult` is the caller's host memory
  read_timing(e, s_end, 1, false);
  {  // where the accumulation phase went, kernel by kernel (ngd_last_spill_timing)
    ngd_spill_timing &t = e->spill_timing;
    t = ngd_spill_timing{};
    for (uint64_t c = 0; c < n_chunks; c++) {
      float ms[4] = {0, 0, 0, 0};
      for (int k = 0; k < 4; k++) hipEventElapsedTime(&ms[k], e->ev_spill[4 * c + k], e->ev_spill[4 * c + k + 1]);
      t.ms_weights += ms[0]; t.ms_terms += ms[1]; t.ms_sanitize += ms[2]; t.ms_contract += ms[3];
    }
    t.chunks = n_chunks; t.units = units_done; t.unit_sites = q; t.sites = s_end;
    t.slot_groups = n_pg; t.slot_groups_live = e->n_pg_live; t.matrices = n_mat; t.matrix_groups = n_rg;
    t.contract_launches = n_chunks * ((n_rg + 7) / 8);
  }
  return NGD_OK;
}

// The replicate loop: optionally the full data set (matrix 0, lead_full), then n_rep bootstrap replicates given
// as block maps (multiplicities are counted from them) or directly as multiplicities.  Outputs are
// [lead_full + n_rep][n_pairs].  The plan is the cheapest that applies: per-block partials (one pass, then a
// weighted reduction per batch of replicates), the EM batch pass, or one (weighted) pass per matrix.
int run_impl(ngd_engine *e, const uint64_t *block_maps, const uint32_t *mult_in, uint32_t n_rep, bool lead_full,
             uint64_t n_blocks, uint64_t block_size, double *d_sum, unsigned long long *d_cnt) {
  if (!e) return fail(NGD_E_INVALID, "ngd_run: null engine");
  if (!e->committed) return fail(NGD_E_INVALID, "ngd_run: call ngd_commit() first");
  if (n_rep)
    if (int rc = em_exact_refuse_weighted(e, "a run with a block map or multiplicities, a batch or a job")) return rc;
  HIPCHK(hipSetDevice(e->device));
  const ngd_geom &g = e->g;
  e->exact_info = ngd_em_exact_info{};
  e->exact_entries.clear();
  e->spill_timing = ngd_spill_timing{};
  e->fix_info = ngd_fixup_info{};
  e->n_batch_valid = 0;  // (the matrices of an earlier batch are not this call's: set again by copy_out() on success)
  if (!n_rep) return pass_impl(e, nullptr, 0, 0, 0, 0, d_sum, d_cnt, false);
  if (int rc = eager_discard(e)) return rc;  // (a job: its plans share passes between matrices; nothing of a plain pass is reused)

  if (!block_size || !n_blocks) return fail(NGD_E_INVALID, "ngd_run: empty bootstrap geometry");
  if (n_blocks > g.n_sites / block_size) return fail(NGD_E_INVALID, "ngd_run: n_blocks*block_size exceeds n_sites");
  const uint64_t n_pairs = ngd_n_pairs(g.n_ind);
  const uint64_t n_eff = n_blocks * block_size;
  const uint32_t lead = lead_full ? 1u : 0u;
  std::vector<unsigned long long> drawn(n_rep + lead, 0);  // sites visited, with multiplicity = gen_dist's cnt
  std::vector<uint32_t> mult_max(n_rep + lead, 0);
  // multiplicities of matrices lead..: counted into (or copied behind) a leading all-ones row, which stands for
  // the full data set when the blocks cover every site
  const uint64_t need = (uint64_t)(n_rep + lead) * n_blocks;
  if (block_maps || lead)  // pinned and kept: a replicate at block size 1 counts a million draws per call
    if (int rc = e->h_mult.ensure(need)) return rc;
  const uint32_t *mult = mult_in;  // [n_rep][n_blocks]
  if (block_maps) {
    uint32_t *base = e->h_mult + (uint64_t)lead * n_blocks;
    memset(base, 0, (uint64_t)n_rep * n_blocks * sizeof(uint32_t));
    for (uint32_t r = 0; r < n_rep; r++) {
      uint32_t *m = base + (uint64_t)r * n_blocks;
      const uint64_t *bm = block_maps + (uint64_t)r * n_blocks;
      for (uint64_t b = 0; b < n_blocks; b++) {
        if (bm[b] >= n_blocks) return fail(NGD_E_INVALID, "ngd_run: block_map entry out of range");
        mult_max[lead + r] = std::max(mult_max[lead + r], ++m[bm[b]]);
      }
      drawn[lead + r] = n_eff;
    }
    mult = base;
  } else {
    for (uint32_t r = 0; r < n_rep; r++)
      for (uint64_t b = 0; b < n_blocks; b++) {
        const uint32_t m = mult[(uint64_t)r * n_blocks + b];
        mult_max[lead + r] = std::max(mult_max[lead + r], m);
        drawn[lead + r] += (unsigned long long)m * block_size;
      }
    if (lead) {
      memcpy(e->h_mult + n_blocks, mult, (uint64_t)n_rep * n_blocks * sizeof(uint32_t));
      mult = e->h_mult + n_blocks;
    }
  }
  if (lead) {
    for (uint64_t b = 0; b < n_blocks; b++) e->h_mult[b] = 1u;
    drawn[0] = g.n_sites;
    mult_max[0] = 1;
  }
  if (e->out.on) e->out.cnt_mat.assign(drawn.begin(), drawn.end());  // (no --pairwise_del: a matrix's count, every pair's)
  double *rep_sum = d_sum + (uint64_t)lead * n_pairs;
  unsigned long long *rep_cnt = d_cnt + (uint64_t)lead * n_pairs;

  // 0. NGD_OPT_EM_EXACT = 2: only plans whose one EM launch notes -- per-block partials (the plain form over slices that are
  //    blocks), else the spilled-terms pass -- and every matrix takes its weight times (c_ref - c_dev) before anything
  //    leaves.  A list that was too short has counted what it needs: the plan runs once more.  No plan: the call fails.
  if (e->opt_em_exact) {
    if (e->kernel != NGD_KERNEL_EM_TABLE) return fail(NGD_E_INVALID, "NGD_OPT_EM_EXACT: internal -- not the table-driven EM kernel");
    const bool ride = lead && n_eff == g.n_sites;  // the full data set as the partials' all-ones row
    bool by_partials = false;
    for (int pass = 1;; pass++) {
      bool feasible = false, done = false, again = false;
      int rc = ride ? partials_impl(e, e->h_mult, drawn.data(), n_rep + 1, n_blocks, block_size, d_sum, d_cnt, &feasible, true)
                    : partials_impl(e, mult, drawn.data() + lead, n_rep, n_blocks, block_size, rep_sum, rep_cnt, &feasible, true);
      if (rc) return rc;
      if (feasible) {
        by_partials = true;
        const uint32_t n_rows = n_rep + (ride ? 1u : 0u), ch = ngd_reduce_chunk(n_rows);
        const ngd_note_weights w{n_rows, 0, e->d_W, nullptr, 1, (uint64_t)e->blk.sub * ((n_rows + ch - 1) / ch * ch), n_blocks, block_size};
        if ((rc = em_exact_finish_w(e, ride ? d_sum : rep_sum, w, &again))) return rc;
      } else {
        if (e->em_shape == 0 && e->opt_em_spill) {
          rc = em_spill_impl(e, mult, mult_max.data() + lead, drawn.data() + lead, n_rep, lead != 0, n_blocks, block_size, d_sum,
                             d_cnt, &done, true);
          if (rc == NGD_E_NOMEM) { (void)hipGetLastError(); g_err.clear(); done = false; rc = NGD_OK; }
          if (rc) return rc;
        }
        if (!done)
          return fail(NGD_E_INVALID, "NGD_OPT_EM_EXACT = 2: no plan that notes can serve this call -- per-block partials do not apply "
                                     "(NGD_OPT_BOOT_PARTIALS, the device's memory) and the spilled-terms plan does not either (variant "
                                     "0 only, NGD_OPT_EM_SPILL, scratch for two k-groups of terms); nothing was computed");
        const ngd_note_weights w{n_rep + lead, lead, nullptr, e->d_M, n_blocks, 1, n_blocks, block_size};
        if ((rc = em_exact_finish_w(e, d_sum, w, &again))) return rc;
      }
      if (!again) {
        e->exact_info.passes = (uint64_t)pass;
        break;
      }
      if (pass == 2) return fail(NGD_E_HIP, "NGD_OPT_EM_EXACT: internal -- the second pass noted more than the first counted");
    }
    if (by_partials && lead && !ride) {  // the lead matrix's own plain pass notes, and is patched, as ever
      const std::vector<ngd_em_exact_entry> first = e->exact_entries;
      const ngd_em_exact_info info1 = e->exact_info;
      if (int rc = pass_impl(e, nullptr, 0, 0, 0, 0, d_sum, d_cnt, true)) return rc;
      em_exact_merge(e, first, info1);
    }
    return NGD_OK;
  }
  // 1. per-block partials; the full data set rides along as the all-ones row when the blocks cover every site
  bool feasible = false;
  int rc;
  if (lead && n_eff == g.n_sites) {
    rc = partials_impl(e, e->h_mult, drawn.data(), n_rep + 1, n_blocks, block_size, d_sum, d_cnt, &feasible);
    if (rc || feasible) return rc;
  } else {
    rc = partials_impl(e, mult, drawn.data() + lead, n_rep, n_blocks, block_size, rep_sum, rep_cnt, &feasible);
    if (rc) return rc;
    if (feasible) return lead ? pass_impl(e, nullptr, 0, 0, 0, 0, d_sum, d_cnt, true) : NGD_OK;
  }
  // 2. EM kernels: many matrices per accumulation pass (the EM of a (pair, site) is computed once and added to up to
  //    16 accumulators per pair -- 8 in the table-driven kernel).  The faithful form keeps matrix 0 on the plain pass,
  //    whose accumulation is the reference's term by term.  The table-driven kernel's batch pass runs one workgroup per
  //    CU and costs ~1.7 plain passes: from three matrices on it beats a plain pass + a weighted pass per replicate
  //    (0.63 of a pass each: they walk only the sites a replicate drew).  Its other shapes borrow the per-pair batch
  //    kernel from three replicates on (those agree with ngd_run()'s to rounding only).
  // 2a. the table-driven kernel, three matrices or more: the terms of a chunk of sites are spilled once and
  //     contracted with every matrix's weights by MFMA -- one EM pass for the whole job, whatever the replicate count
  if (e->kernel == NGD_KERNEL_EM_TABLE && e->em_shape == 0 && e->opt_em_spill &&
      n_rep + lead >= (e->opt_em_spill == 2 ? 2u : 3u)) {
    bool done = false;
    rc = em_spill_impl(e, mult, mult_max.data() + lead, drawn.data() + lead, n_rep, lead != 0, n_blocks, block_size,
                       d_sum, d_cnt, &done);
    if (rc == NGD_E_NOMEM) { (void)hipGetLastError(); g_err.clear(); done = false; rc = NGD_OK; }
    if (rc || done) return rc;
  }
  const bool em_pair = e->kernel == NGD_KERNEL_EM_FAST || e->kernel == NGD_KERNEL_EM_FAITHFUL;
  const bool em_table_batch = e->kernel == NGD_KERNEL_EM_TABLE && e->em_shape == 0 && n_rep + lead >= 3;
  const bool em_borrow = e->kernel == NGD_KERNEL_EM_TABLE && e->em_shape != 0 && n_rep >= 3;
  if ((em_pair || em_borrow || em_table_batch) && n_rep + lead >= 2 && e->opt_em_batch) {
    const bool fold = lead && e->kernel != NGD_KERNEL_EM_FAITHFUL;
    if (lead && !fold) {
      rc = pass_impl(e, nullptr, 0, 0, 0, 0, d_sum, d_cnt, false);
      if (rc) return rc;
    }
    rc = em_batch_impl(e, mult, mult_max.data() + lead, drawn.data() + lead, n_rep, fold, n_blocks, block_size,
                       fold ? d_sum : rep_sum, fold ? d_cnt : rep_cnt, lead && !fold);
    // the batch pass wants RB result planes per slice: if the device cannot hold them (very many individuals), the
    // matrices are computed one pass each instead (the allocation is tried before anything is launched)
    if (rc != NGD_E_NOMEM) return rc;
    (void)hipGetLastError();
    g_err.clear();  // not an error of this call: the matrices are computed one pass each instead
    if (lead && !fold) {  // matrix 0 is done already
      for (uint32_t r = 0; r < n_rep; r++) {
        rc = pass_impl(e, mult + (uint64_t)r * n_blocks, mult_max[lead + r], n_blocks, block_size, drawn[lead + r],
                       rep_sum + (uint64_t)r * n_pairs, rep_cnt + (uint64_t)r * n_pairs, true);
        if (rc) return rc;
      }
      return NGD_OK;
    }
  }
  // 3. one accumulation pass per matrix
  if (lead) {
    rc = pass_impl(e, nullptr, 0, 0, 0, 0, d_sum, d_cnt, false);
    if (rc) return rc;
  }
  for (uint32_t r = 0; r < n_rep; r++) {
    rc = pass_impl(e, mult + (uint64_t)r * n_blocks, mult_max[lead + r], n_blocks, block_size, drawn[lead + r],
                   rep_sum + (uint64_t)r * n_pairs, rep_cnt + (uint64_t)r * n_pairs, lead || r > 0);
    if (rc) return rc;
  }
  return NGD_OK;
}
