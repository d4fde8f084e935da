// engine.hip -- the C ABI of include/ngsdist_amd.h: the entry points that only check their arguments and hand on to the
// engine's units (ngd_engine.h), the options and the getters.  There is no CPU fallback anywhere in the engine: if HIP is
// unusable every entry point fails with an error code.
#include "ngd_engine.h"

extern "C" {

const char *ngd_last_error(void) { return g_err.c_str(); }
int ngd_abi_version(void) { return NGD_ABI_VERSION; }

uint64_t ngd_n_pairs(uint64_t n_ind) { return n_ind * (n_ind - 1) / 2; }
uint64_t ngd_pair_index(uint64_t n_ind, uint64_t i1, uint64_t i2) { return ngd_pair_idx(n_ind, i1, i2); }
uint64_t ngd_device_bytes(const ngd_engine *e) { return e ? e->dev_bytes : 0; }

int ngd_run_device(ngd_engine *e, const uint64_t *block_map, uint64_t n_blocks, uint64_t block_size,
                   void *d_sum, void *d_cnt) {
  if (!d_sum || !d_cnt) return fail(NGD_E_INVALID, "ngd_run_device: null output");
  return run_impl(e, block_map, nullptr, block_map ? 1 : 0, false, n_blocks, block_size, (double *)d_sum,
                  (unsigned long long *)d_cnt);
}

int ngd_run_mult_device(ngd_engine *e, const uint32_t *mult, uint64_t n_blocks, uint64_t block_size, void *d_sum,
                        void *d_cnt) {
  if (!d_sum || !d_cnt || !mult) return fail(NGD_E_INVALID, "ngd_run_mult_device: null argument");
  return run_impl(e, nullptr, mult, 1, false, n_blocks, block_size, (double *)d_sum, (unsigned long long *)d_cnt);
}

int ngd_run_mult(ngd_engine *e, const uint32_t *mult, uint64_t n_blocks, uint64_t block_size, double *sum,
                 uint64_t *cnt) {
  if (!e || !mult) return fail(NGD_E_INVALID, "ngd_run_mult: null argument");
  return run_to_host(e, nullptr, mult, 1, false, n_blocks, block_size, 0, sum, cnt);
}

int ngd_run(ngd_engine *e, const uint64_t *block_map, uint64_t n_blocks, uint64_t block_size, double *sum,
            uint64_t *cnt) {
  if (!e) return fail(NGD_E_INVALID, "ngd_run: null engine");
  return run_to_host(e, block_map, nullptr, block_map ? 1 : 0, false, n_blocks, block_size, 0, sum, cnt);
}

int ngd_run_batch_device(ngd_engine *e, const uint64_t *block_maps, uint32_t n_rep, uint64_t n_blocks,
                         uint64_t block_size, void *d_sum, void *d_cnt) {
  if (!block_maps || !n_rep || !d_sum || !d_cnt) return fail(NGD_E_INVALID, "ngd_run_batch_device: null argument");
  return run_impl(e, block_maps, nullptr, n_rep, false, n_blocks, block_size, (double *)d_sum, (unsigned long long *)d_cnt);
}

int ngd_run_mult_batch_device(ngd_engine *e, const uint32_t *mult, uint32_t n_rep, uint64_t n_blocks,
                              uint64_t block_size, void *d_sum, void *d_cnt) {
  if (!mult || !n_rep || !d_sum || !d_cnt) return fail(NGD_E_INVALID, "ngd_run_mult_batch_device: null argument");
  return run_impl(e, nullptr, mult, n_rep, false, n_blocks, block_size, (double *)d_sum, (unsigned long long *)d_cnt);
}

int ngd_run_batch(ngd_engine *e, const uint64_t *block_maps, uint32_t n_rep, uint64_t n_blocks, uint64_t block_size,
                  double *sum, uint64_t *cnt) {
  if (!e || !block_maps || !n_rep) return fail(NGD_E_INVALID, "ngd_run_batch: null argument");
  return run_to_host(e, block_maps, nullptr, n_rep, false, n_blocks, block_size, n_rep, sum, cnt);
}

int ngd_run_mult_batch(ngd_engine *e, const uint32_t *mult, uint32_t n_rep, uint64_t n_blocks, uint64_t block_size,
                       double *sum, uint64_t *cnt) {
  if (!e || !mult || !n_rep) return fail(NGD_E_INVALID, "ngd_run_mult_batch: null argument");
  return run_to_host(e, nullptr, mult, n_rep, false, n_blocks, block_size, n_rep, sum, cnt);
}

int ngd_run_job_device(ngd_engine *e, const uint64_t *block_maps, uint32_t n_rep, uint64_t n_blocks,
                       uint64_t block_size, void *d_sum, void *d_cnt) {
  if (!d_sum || !d_cnt || (n_rep && !block_maps)) return fail(NGD_E_INVALID, "ngd_run_job_device: null argument");
  return run_impl(e, block_maps, nullptr, n_rep, n_rep != 0, n_blocks, block_size, (double *)d_sum,
                  (unsigned long long *)d_cnt);
}

int ngd_run_job(ngd_engine *e, const uint64_t *block_maps, uint32_t n_rep, uint64_t n_blocks, uint64_t block_size,
                double *sum, uint64_t *cnt) {
  if (!e || (n_rep && !block_maps)) return fail(NGD_E_INVALID, "ngd_run_job: null argument");
  return run_to_host(e, block_maps, nullptr, n_rep, n_rep != 0, n_blocks, block_size, n_rep + 1, sum, cnt);
}

int ngd_run_job_dist(ngd_engine *e, const uint64_t *block_maps, uint32_t n_rep, uint64_t n_blocks, uint64_t block_size,
                     uint64_t tot_sites, uint64_t evol_model, double *dist) {
  if (n_rep && !block_maps) return fail(NGD_E_INVALID, "ngd_run_job_dist: null argument");
  return run_dist(e, block_maps, nullptr, n_rep, true, n_blocks, block_size, tot_sites, evol_model, dist, "ngd_run_job_dist");
}

int ngd_run_batch_dist(ngd_engine *e, const uint64_t *block_maps, uint32_t n_rep, uint64_t n_blocks, uint64_t block_size,
                       uint64_t tot_sites, uint64_t evol_model, double *dist) {
  if (!block_maps || !n_rep) return fail(NGD_E_INVALID, "ngd_run_batch_dist: null argument");
  return run_dist(e, block_maps, nullptr, n_rep, false, n_blocks, block_size, tot_sites, evol_model, dist, "ngd_run_batch_dist");
}

int ngd_run_mult_batch_dist(ngd_engine *e, const uint32_t *mult, uint32_t n_rep, uint64_t n_blocks, uint64_t block_size,
                            uint64_t tot_sites, uint64_t evol_model, double *dist) {
  if (!mult || !n_rep) return fail(NGD_E_INVALID, "ngd_run_mult_batch_dist: null argument");
  return run_dist(e, nullptr, mult, n_rep, false, n_blocks, block_size, tot_sites, evol_model, dist, "ngd_run_mult_batch_dist");
}

int ngd_fetch_matrix(ngd_engine *e, uint32_t which, double *sum, uint64_t *cnt) {
  if (!e) return fail(NGD_E_INVALID, "ngd_fetch_matrix: null engine");
  if (which >= e->n_batch_valid) return fail(NGD_E_INVALID, "ngd_fetch_matrix: no such matrix in the engine's last batch");
  HIPCHK(hipSetDevice(e->device));
  const uint64_t n = ngd_n_pairs(e->g.n_ind);
  if (sum) HIPCHK(hipMemcpy(sum, e->d_bsum + (uint64_t)which * n, n * sizeof(double), hipMemcpyDeviceToHost));
  if (cnt) HIPCHK(hipMemcpy(cnt, e->d_bcnt + (uint64_t)which * n, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return NGD_OK;
}

int ngd_set_option(ngd_engine *e, int option, uint64_t value) {
  if (!e) return fail(NGD_E_INVALID, "ngd_set_option: null engine");
  switch (option) {
    case NGD_OPT_BOOT_PARTIALS:
      if (value > 2) return fail(NGD_E_INVALID, "ngd_set_option: NGD_OPT_BOOT_PARTIALS is 0, 1 or 2");
      e->opt_boot_partials = value;
      break;
    case NGD_OPT_BOOT_MAX_BYTES: e->opt_boot_max_bytes = value; break;
    case NGD_OPT_BOOT_WG:
      if (!value) return fail(NGD_E_INVALID, "ngd_set_option: NGD_OPT_BOOT_WG must be positive");
      e->opt_boot_wg = value;
      break;
    case NGD_OPT_BOOT_UNALIGNED: e->opt_boot_unaligned = value != 0; break;
    case NGD_OPT_EM_BATCH: e->opt_em_batch = value != 0; break;
    case NGD_OPT_EM_SPILL:
      if (value > 2) return fail(NGD_E_INVALID, "ngd_set_option: NGD_OPT_EM_SPILL is 0, 1 or 2");
      e->opt_em_spill = value;
      break;
    case NGD_OPT_EM_SPILL_BYTES: e->opt_em_spill_bytes = value; break;
    case NGD_OPT_SINGLE_IMAGE_BYTES:
      if (!e->cfg.single_image) return fail(NGD_E_INVALID, "ngd_set_option: NGD_OPT_SINGLE_IMAGE_BYTES needs ngd_config.single_image");
      if (!e->single_image) break;  // (another kernel, or second_image_mib holds the whole second image: nothing is formed)
      e->qb_chunk_kg = std::max<uint64_t>(1, (value ? value : 4ull << 30) / ((uint64_t)e->g.n_ig * 64 * 8));
      break;
    case NGD_OPT_FIXUP_WORK: e->opt_fix_work = value; break;
    case NGD_OPT_WIN_PLAN:
      if (value > 2) return fail(NGD_E_INVALID, "ngd_set_option: NGD_OPT_WIN_PLAN is 0, 1 or 2");
      e->opt_win_plan = value;
      break;
    case NGD_OPT_WIN_MAX_BYTES: e->opt_win_max_bytes = value; break;
    case NGD_OPT_NJ_MAX_BYTES: e->nj.max_bytes = value; break;
    case NGD_OPT_MDS_MAX_BYTES: e->mds.max_bytes = value; break;
    case NGD_OPT_WIN_CMP_MAX_BYTES: e->wcmp.max_bytes = value; break;
    case NGD_OPT_EM_EXACT: return em_exact_set(e, value);
    case NGD_OPT_EM_EXACT_WIN: return em_exact_win_set(e, value);
    case NGD_OPT_EM_EXACT_CAP:
      if (value >= (1ull << 31)) return fail(NGD_E_INVALID, "ngd_set_option: NGD_OPT_EM_EXACT_CAP is below 2^31 entries");
      e->note_cap = value ? value : 1ull << 20;
      break;
    case NGD_OPT_EAGER_FULL:
      if (e->pin_sites || e->committed) return fail(NGD_E_INVALID, "ngd_set_option: NGD_OPT_EAGER_FULL before the first ngd_stage_acquire");
      if (value && e->opt_em_exact) return fail(NGD_E_INVALID, "ngd_set_option: NGD_OPT_EAGER_FULL and NGD_OPT_EM_EXACT refuse each other (the eager pass does not note)");
      e->opt_eager = value != 0 && eager_supported(e);  // (kernels without a slice-range launch: silently off)
      break;
    case NGD_OPT_STAGE_PIECE_MIB:
    case NGD_OPT_STAGE_RING:
      if (e->pin_sites) return fail(NGD_E_INVALID, "ngd_set_option: the staging ring exists already (set before the first ngd_stage_acquire)");
      if (option == NGD_OPT_STAGE_RING) {
        if (value < 2 || value > ngd_engine::RING) return fail(NGD_E_INVALID, "ngd_set_option: NGD_OPT_STAGE_RING is 2 .. 8");
        e->opt_stage_ring = value;
      } else {
        if (value < 1 || value > 1024) return fail(NGD_E_INVALID, "ngd_set_option: NGD_OPT_STAGE_PIECE_MIB is 1 .. 1024");
        e->opt_stage_piece_mib = value;
      }
      break;
    case NGD_OPT_UNIT_SKIP: e->opt_unit_skip = value != 0; break;
    case NGD_OPT_DEBUG_FORGE_JOB: {  // tests only: the first block of the MFMA job list gets another shape
      // (an engine with a forged job list computes nothing right ever after: refused unless the process says it is a test)
      const char *hook = getenv("NGD_ENABLE_TEST_HOOKS");
      if (!hook || strcmp(hook, "1") != 0)
        return fail(NGD_E_INVALID, "ngd_set_option: NGD_OPT_DEBUG_FORGE_JOB is a test hook (set NGD_ENABLE_TEST_HOOKS=1)");
      if (e->kernel != NGD_KERNEL_MFMA || !e->d_jobs) return fail(NGD_E_INVALID, "ngd_set_option: no MFMA job list");
      HIPCHK(hipSetDevice(e->device));
      ngd_job j;
      HIPCHK(hipMemcpy(&j, e->d_jobs, sizeof(j), hipMemcpyDeviceToHost));
      j.rows = (uint8_t)(value & 7); j.cols = (uint8_t)((value >> 3) & 7); j.tri = (uint8_t)((value >> 6) & 1);
      HIPCHK(hipMemcpy(e->d_jobs, &j, sizeof(j), hipMemcpyHostToDevice));
      break;
    }
    default: return fail(NGD_E_INVALID, "ngd_set_option: unknown option");
  }
  return NGD_OK;
}

int ngd_drop_caches(ngd_engine *e) {
  if (!e) return fail(NGD_E_INVALID, "ngd_drop_caches: null engine");
  e->blk.drop();
  e->em_batch_nofit_elems = 0;  // (what did not fit may fit now: the partial results' slab is the same scratch)
  return NGD_OK;
}

int ngd_last_em_work(const ngd_engine *e, uint64_t *tile_sites, uint64_t *table_rounds) {
  if (!e) return fail(NGD_E_INVALID, "ngd_last_em_work: null engine");
  if (tile_sites) *tile_sites = e->em_counts[0];
  if (table_rounds) *table_rounds = e->em_counts[1];
  return NGD_OK;
}

int ngd_last_shader_clock(const ngd_engine *e, double *mhz) {
  if (!e || !mhz) return fail(NGD_E_INVALID, "ngd_last_shader_clock: null argument");
  *mhz = e->clk_mhz;
  return NGD_OK;
}

int ngd_last_fixup(const ngd_engine *e, ngd_fixup_info *info) {
  if (!e || !info) return fail(NGD_E_INVALID, "ngd_last_fixup: null argument");
  *info = e->fix_info;
  return NGD_OK;
}

int ngd_image_mode(const ngd_engine *e, int *fixup) {
  if (!e) return fail(NGD_E_INVALID, "ngd_image_mode: null engine");
  if (fixup) *fixup = e->SM != nullptr;
  if (e->kernel != NGD_KERNEL_MFMA) return 0;
  return e->congruent ? 2 : e->single_image ? 1 : 3;
}

int ngd_last_spill_timing(const ngd_engine *e, ngd_spill_timing *t) {
  if (!e || !t) return fail(NGD_E_INVALID, "ngd_last_spill_timing: null argument");
  *t = e->spill_timing;
  return NGD_OK;
}

int ngd_last_plain_pass(const ngd_engine *e, uint64_t *kgroups) {
  if (!e || !kgroups) return fail(NGD_E_INVALID, "ngd_last_plain_pass: null argument");
  *kgroups = e->plain_kg;
  return NGD_OK;
}

int ngd_last_timing(const ngd_engine *e, ngd_timing *t) {
  if (!e || !t) return fail(NGD_E_INVALID, "ngd_last_timing: null argument");
  *t = e->timing;
  return NGD_OK;
}

}  // extern "C"
