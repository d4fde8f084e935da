// engine_em_exact.hip -- NGD_OPT_EM_EXACT: the full-data pass of the table-driven EM kernel stops every (pair, site) where
// the reference does.  The kernels decide the stopping rule of emOptim2.cpp:127 from ratios of power sums and may, within
// rounding of the tolerance, stop one EM step from the reference.  The noting form of the pass (accum_em_table.hip NOTE)
// lists the stops whose criterion is within 2^-36 of the threshold; here the list's sites are run again the reference's
// way on the host (ngd_em2_site, host_util.cpp) and each pair's sum takes its corrections c_ref - c_dev, in site order,
// before it leaves the engine -- the same role fixup.hip plays on the --indep_geno path.
// Value 2 of the option also serves the calls that weight sites (a block map, multiplicities, a batch, a job): the list of
// in-band (pair, site)s does not depend on the replicate, so the plan's one noting launch (per-block partials, or the
// spilled-terms pass in its noting form) gives the list, and matrix r takes m_r(site) * (c_ref - c_dev) (em_exact_finish_w).
#include "ngd_engine.h"

#include <iterator>

static const char *const kExactOnly =
    "NGD_OPT_EM_EXACT is on: it serves the plain full-data pass (ngd_run / ngd_run_device with no block map) only -- ";

int em_exact_refuse(const ngd_engine *e, const char *who) {
  if (!e || !e->opt_em_exact) return NGD_OK;
  return fail(NGD_E_INVALID, std::string(kExactOnly) + who + " is not served (replicates and windows from the same list: DESIGN.md section 8)");
}

int em_exact_refuse_weighted(const ngd_engine *e, const char *who) {
  if (e && e->opt_em_exact_boot) return NGD_OK;  // (value 2: run_impl serves it, or says which plan it lacks)
  return em_exact_refuse(e, who);
}

int em_exact_set(ngd_engine *e, uint64_t value) {
  if (value > 2) return fail(NGD_E_INVALID, "ngd_set_option: NGD_OPT_EM_EXACT is 0, 1 or 2");
  if (!value) {
    e->opt_em_exact = e->opt_em_exact_boot = false;
    return NGD_OK;
  }
  if (e->cfg.indep_geno) return fail(NGD_E_INVALID, "ngd_set_option: NGD_OPT_EM_EXACT belongs to the EM path (no --indep_geno)");
  if (e->cfg.kernel != NGD_KERNEL_AUTO && e->cfg.kernel != NGD_KERNEL_EM_TABLE)
    return fail(NGD_E_INVALID, "ngd_set_option: NGD_OPT_EM_EXACT needs the table-driven EM kernel (kernel = auto or NGD_KERNEL_EM_TABLE)");
  if (e->opt_eager) return fail(NGD_E_INVALID, "ngd_set_option: NGD_OPT_EM_EXACT and NGD_OPT_EAGER_FULL refuse each other (the eager pass does not note)");
  if (e->kernel != NGD_KERNEL_EM_TABLE) {
    // kernel = auto at 32 individuals or fewer resolved to the per-pair kernel: the engine moves to the table-driven one
    // (the geometry ngd_create gives it; the spilled-terms plan's slot map is built below for value 2, which serves jobs)
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->st));
    const ngd_geom &g = e->g;
    uint64_t ks = e->n_tiles64 ? ((e->cfg.wg_target ? e->cfg.wg_target : 16384) + e->n_tiles64 - 1) / e->n_tiles64 : 1;
    ks = std::min(ks, std::max<uint64_t>(1, g.n_sites / 64));
    if (e->cfg.n_slices) ks = std::min<uint64_t>(e->cfg.n_slices, g.n_sites);
    if (int rc = e->slab.alloc(e, ks * (uint64_t)g.n_pad * g.n_pad, true)) return rc;
    if (int rc = e->d_emcnt.alloc(e, 4, true)) return rc;
    e->em_shape = (int)e->cfg.variant;
    e->n_ks = (uint32_t)ks;
    e->per_slice = (g.n_sites + ks - 1) / ks;
    e->kernel = NGD_KERNEL_EM_TABLE;
  }
  if (value == 2 && !e->d_rowpg) {  // (an engine that was moved above, now or by an earlier value 1: it has no slot map yet)
    HIPCHK(hipSetDevice(e->device));
    std::vector<ngd_tile> tiles64(e->n_tiles64);  // (ngd_create keeps no host copy of the list)
    if (e->n_tiles64) HIPCHK(hipMemcpy(tiles64.data(), e->d_tiles64, tiles64.size() * sizeof(ngd_tile), hipMemcpyDeviceToHost));
    if (int rc = spill_slot_map(e, tiles64)) return rc;
  }
  e->opt_em_exact = true;
  e->opt_em_exact_boot = value == 2;
  return NGD_OK;
}

int em_exact_begin(ngd_engine *e) {
  const uint64_t words = NGD_NOTE_HEAD + NGD_NOTE_WORDS * e->note_cap;
  if (e->d_note.capacity() != words)  // (also a smaller list than before: NGD_OPT_EM_EXACT_CAP is what a test asks for)
    if (int rc = e->d_note.alloc(e, words, false)) return rc;
  e->note_head[0] = 0;
  e->note_head[1] = e->note_cap;
  HIPCHK(hipMemcpyAsync(e->d_note, e->note_head, sizeof(e->note_head), hipMemcpyHostToDevice, e->st));
  return NGD_OK;
}

// What the noting launch(es) since em_exact_begin listed, rechecked (stream idle): the entries sorted by (pair, site) into
// e->exact_entries, the corrections c_ref - c_dev in that order on the device (d_note_delta), the distinct pairs
// (d_note_pair) and where each pair's corrections start (d_note_first); with_sites: the entries' sites too (d_note_site).
// *again: the list was too short and has grown to what the launch counted -- nothing else has been done.
static int em_exact_recheck(ngd_engine *e, bool with_sites, bool *again, uint32_t *n_noted_pairs) {
  *again = false;
  *n_noted_pairs = 0;
  unsigned long long head[2] = {0, 0};
  HIPCHK(hipMemcpy(head, e->d_note, sizeof(head), hipMemcpyDeviceToHost));
  ngd_em_exact_info &info = e->exact_info;
  info = ngd_em_exact_info{};
  info.noted = head[0];
  info.passes = 1;
  e->exact_entries.clear();
  if (head[0] > e->note_cap) {
    if (head[0] >= (1ull << 31)) return fail(NGD_E_NOMEM, "NGD_OPT_EM_EXACT: 2^31 or more (pair, site)s noted in one pass");
    e->note_cap = head[0];
    *again = true;
    return NGD_OK;
  }
  const uint32_t n = (uint32_t)head[0];
  if (!n) return NGD_OK;
  const ngd_geom &g = e->g;
  if (int rc = e->d_note_gl.ensure(e, 6ull * n)) return rc;
  unsigned long long *d_ent = e->d_note + NGD_NOTE_HEAD;
  ngd_launch_note_gather(e->st, g, e->PA, e->d_tiles64, e->n_tiles64, d_ent, n, e->d_note_gl);
  HIPCHK(hipGetLastError());
  std::vector<unsigned long long> raw((size_t)n * NGD_NOTE_WORDS);
  std::vector<double> gl(6ull * n);
  HIPCHK(hipMemcpyAsync(raw.data(), d_ent, raw.size() * 8, hipMemcpyDeviceToHost, e->st));
  HIPCHK(hipMemcpyAsync(gl.data(), e->d_note_gl, gl.size() * 8, hipMemcpyDeviceToHost, e->st));
  HIPCHK(hipStreamSynchronize(e->st));
  // the order the entries were appended in is not reproducible; results must be: by (pair, site)
  std::vector<uint32_t> ord(n);
  for (uint32_t k = 0; k < n; k++) ord[k] = k;
  auto key = [&](uint32_t k) {
    const unsigned long long w = raw[(size_t)k * NGD_NOTE_WORDS];
    return std::make_pair(((w & 0xffffffffull) << 32) | (w >> 32), raw[(size_t)k * NGD_NOTE_WORDS + 1]);  // (i1, i2), site
  };
  std::sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return key(a) < key(b); });
  std::vector<ngd_em_exact_entry> &ent = e->exact_entries;
  ent.resize(n);
  std::vector<double> delta(n);
  std::vector<unsigned long long> pair, sites(with_sites ? n : 0);
  std::vector<uint32_t> first;
  for (uint32_t q = 0; q < n; q++) {
    const uint32_t k = ord[q];
    const unsigned long long *r = &raw[(size_t)k * NGD_NOTE_WORDS];
    ngd_em_exact_entry &x = ent[q];
    x.i1 = (uint32_t)r[0];
    x.i2 = (uint32_t)(r[0] >> 32);
    x.site = r[1];
    x.t_dev = (uint32_t)r[2];
    memcpy(&x.c_dev, &r[3], 8);
    if (!(x.i1 < x.i2 && x.i2 < g.n_ind && x.site < g.n_sites))
      return fail(NGD_E_HIP, "NGD_OPT_EM_EXACT: internal -- a noted entry names no (pair, site) of the engine");
    // the reference's own steps on this site (ngsDist.cpp:340-349) and its term (:351-353)
    double sfs[9];
    for (int c = 0; c < 9; c++) sfs[c] = (double)1 / 9;
    int it = 0;
    ngd_em2_site(&gl[6ull * k], &gl[6ull * k + 3], sfs, &it);
    double c_ref = 0;
    for (int a = 0; a < 3; a++)
      for (int b = 0; b < 3; b++) c_ref += e->sc.v[3 * a + b] * sfs[3 * a + b];
    x.t_ref = (uint32_t)it;
    x.c_ref = c_ref;
    delta[q] = c_ref - x.c_dev;
    if (with_sites) sites[q] = x.site;
    if (x.t_ref != x.t_dev) info.changed++;
    const unsigned long long pi = ngd_pair_idx(g.n_ind, x.i1, x.i2);
    if (pair.empty() || pair.back() != pi) {
      pair.push_back(pi);
      first.push_back(q);
    }
  }
  first.push_back(n);
  const uint32_t np = (uint32_t)pair.size();
  int rc = e->d_note_delta.ensure(e, n);
  if (!rc) rc = e->d_note_pair.ensure(e, np);
  if (!rc) rc = e->d_note_first.ensure(e, (uint64_t)np + 1);
  if (!rc && with_sites) rc = e->d_note_site.ensure(e, n);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(e->d_note_delta, delta.data(), (uint64_t)n * 8, hipMemcpyHostToDevice, e->st));
  HIPCHK(hipMemcpyAsync(e->d_note_pair, pair.data(), (uint64_t)np * 8, hipMemcpyHostToDevice, e->st));
  HIPCHK(hipMemcpyAsync(e->d_note_first, first.data(), ((uint64_t)np + 1) * 4, hipMemcpyHostToDevice, e->st));
  if (with_sites) HIPCHK(hipMemcpyAsync(e->d_note_site, sites.data(), (uint64_t)n * 8, hipMemcpyHostToDevice, e->st));
  HIPCHK(hipStreamSynchronize(e->st));  // (delta, pair, first, sites are host temporaries)
  *n_noted_pairs = np;
  return NGD_OK;
}

int em_exact_finish(ngd_engine *e, double *d_sum, bool *again) {
  const auto t0 = std::chrono::steady_clock::now();
  uint32_t np = 0;
  if (int rc = em_exact_recheck(e, false, again, &np)) return rc;
  if (*again || !np) return NGD_OK;
  ngd_launch_note_patch(e->st, e->d_note_pair, e->d_note_first, e->d_note_delta, np, d_sum);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(e->st));
  e->exact_info.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return NGD_OK;
}

int em_exact_finish_w(ngd_engine *e, double *d_sum, const ngd_note_weights &w, bool *again) {
  const auto t0 = std::chrono::steady_clock::now();
  uint32_t np = 0;
  if (int rc = em_exact_recheck(e, true, again, &np)) return rc;
  if (*again || !np) return NGD_OK;
  ngd_launch_note_patch_w(e->st, e->d_note_pair, e->d_note_first, e->d_note_delta, e->d_note_site, np, w, e->g.n_sites,
                          ngd_n_pairs(e->g.n_ind), d_sum);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(e->st));
  e->exact_info.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return NGD_OK;
}

// NGD_OPT_EM_EXACT_WIN: the switch that lets the windowed calls through while NGD_OPT_EM_EXACT is on.  Off, every call does
// what it did before the switch existed, refusals and their words included.
int em_exact_win_set(ngd_engine *e, uint64_t value) {
  if (value > 1) return fail(NGD_E_INVALID, "ngd_set_option: NGD_OPT_EM_EXACT_WIN is 0 or 1");
  if (value) {  // (the engines on which NGD_OPT_EM_EXACT itself is refused)
    if (e->cfg.indep_geno) return fail(NGD_E_INVALID, "ngd_set_option: NGD_OPT_EM_EXACT_WIN belongs to the EM path (no --indep_geno)");
    if (e->cfg.kernel != NGD_KERNEL_AUTO && e->cfg.kernel != NGD_KERNEL_EM_TABLE)
      return fail(NGD_E_INVALID, "ngd_set_option: NGD_OPT_EM_EXACT_WIN needs the table-driven EM kernel (kernel = auto or NGD_KERNEL_EM_TABLE)");
  }
  e->opt_em_exact_win = value != 0;
  return NGD_OK;
}

int em_exact_refuse_windows(const ngd_engine *e, const char *who, bool job) {
  if (!e || !e->opt_em_exact) return NGD_OK;
  if (!e->opt_em_exact_win) return em_exact_refuse(e, who);
  if (job && !e->opt_em_exact_boot)
    return fail(NGD_E_INVALID, std::string("NGD_OPT_EM_EXACT_WIN is on beside NGD_OPT_EM_EXACT = 1: ") + who +
                                   " is not served -- the replicates of a job need NGD_OPT_EM_EXACT = 2");
  return NGD_OK;
}

int em_exact_finish_win(ngd_engine *e, double *d_sum, const uint64_t *lo, const uint64_t *hi, ngd_note_win w, bool *again) {
  const auto t0 = std::chrono::steady_clock::now();
  uint32_t np = 0;
  if (int rc = em_exact_recheck(e, true, again, &np)) return rc;
  if (*again || !np) return NGD_OK;
  if ((uint64_t)np * w.n_win * w.n_mat >= NGD_NOTE_WIN_MAX)
    return fail(NGD_E_NOMEM, "NGD_OPT_EM_EXACT_WIN: noted pairs x windows x matrices of one batch reach 2^39 (a smaller NGD_OPT_WIN_MAX_BYTES makes smaller batches)");
  std::vector<unsigned long long> lohi(2ull * w.n_win);
  for (uint32_t k = 0; k < w.n_win; k++) {
    lohi[2ull * k] = lo[k];
    lohi[2ull * k + 1] = hi[k];
  }
  if (int rc = e->d_note_win.ensure(e, lohi.size())) return rc;
  HIPCHK(hipMemcpy(e->d_note_win, lohi.data(), lohi.size() * 8, hipMemcpyHostToDevice));
  w.lohi = e->d_note_win;
  ngd_launch_note_patch_win(e->st, e->d_note_pair, e->d_note_first, e->d_note_delta, e->d_note_site, np, w, ngd_n_pairs(e->g.n_ind), d_sum);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(e->st));
  e->exact_info.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return NGD_OK;
}

void em_exact_call_begin(ngd_engine *e) {
  e->exact_info = e->call_info = ngd_em_exact_info{};
  e->exact_entries.clear();
  e->call_entries.clear();
}

// (any number of lists: each joins the union of those before it -- em_exact_merge, fold by fold)
void em_exact_call_add(ngd_engine *e) {
  em_exact_merge(e, e->call_entries, e->call_info);
  e->call_entries = e->exact_entries;
  e->call_info = e->exact_info;
}

// Two noting launches of one call (the replicates' per-block partials and the lead matrix's own plain pass): the call's
// list is their union, each (pair, site) once.  `first` / `info1` are the earlier launch's, e->exact_* the later one's.
void em_exact_merge(ngd_engine *e, const std::vector<ngd_em_exact_entry> &first, const ngd_em_exact_info &info1) {
  auto key_less = [](const ngd_em_exact_entry &a, const ngd_em_exact_entry &b) {
    return a.i1 != b.i1 ? a.i1 < b.i1 : a.i2 != b.i2 ? a.i2 < b.i2 : a.site < b.site;
  };
  std::vector<ngd_em_exact_entry> all;
  all.reserve(first.size() + e->exact_entries.size());
  std::merge(e->exact_entries.begin(), e->exact_entries.end(), first.begin(), first.end(), std::back_inserter(all), key_less);
  all.erase(std::unique(all.begin(), all.end(), [](const ngd_em_exact_entry &a, const ngd_em_exact_entry &b) {
              return a.i1 == b.i1 && a.i2 == b.i2 && a.site == b.site;
            }), all.end());
  e->exact_entries.swap(all);
  ngd_em_exact_info &info = e->exact_info;
  info.noted = e->exact_entries.size();
  info.changed = 0;
  for (const ngd_em_exact_entry &x : e->exact_entries)
    if (x.t_ref != x.t_dev) info.changed++;
  info.passes = std::max(info.passes, info1.passes);
  info.ms += info1.ms;
}

extern "C" {

int ngd_last_em_exact(const ngd_engine *e, ngd_em_exact_info *info) {
  if (!e || !info) return fail(NGD_E_INVALID, "ngd_last_em_exact: null argument");
  *info = e->exact_info;
  return NGD_OK;
}

int64_t ngd_em_exact_entries(const ngd_engine *e, ngd_em_exact_entry *out, uint64_t cap) {
  if (!e) return fail(NGD_E_INVALID, "ngd_em_exact_entries: null engine");
  const uint64_t n = e->exact_entries.size();
  if (out && n) memcpy(out, e->exact_entries.data(), std::min(n, cap) * sizeof(ngd_em_exact_entry));
  return (int64_t)n;
}

}  // extern "C"
