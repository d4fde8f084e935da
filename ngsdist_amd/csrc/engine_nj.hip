// engine_nj.hip -- neighbour-joining trees: the tree of every device matrix (nj.hip, one workgroup per matrix), and that
// reduction as a tail (ngd_engine.h) behind the job driver and the window driver: the run forms, where 2 n - 3 branches per
// matrix cross the link instead of n (n - 1) / 2 sums and counts.
#include "ngd_engine.h"

#include <cstdlib>

uint32_t ngd_nj_max_ind(void) { return NGD_NJ_MAX_IND; }

// the workgroup: NGD_NJ_THREADS, or what NGD_NJ_WG names (256, 512, 1024: for the measurement that chose it)
static uint32_t nj_threads() {
  if (const char *s = getenv("NGD_NJ_WG")) {
    const long v = atol(s);
    if (v == 256 || v == 512 || v == 1024) return (uint32_t)v;
  }
  return NGD_NJ_THREADS;
}

// what every call that builds trees refuses, before anything is launched
static int nj_refuse(const ngd_engine *e, const void *child, const void *len, const void *status, uint64_t tot_sites,
                     uint64_t evol_model, const char *who) {
  const std::string w(who);
  if (!e) return fail(NGD_E_INVALID, w + ": null engine");
  if (!child || !len || !status) return fail(NGD_E_INVALID, w + ": null output");
  if (e->g.n_ind < 3) return fail(NGD_E_INVALID, w + ": a tree needs three individuals or more");
  if (e->g.n_ind > ngd_nj_max_ind())
    return fail(NGD_E_INVALID, w + ": more than " + std::to_string(ngd_nj_max_ind()) +
                                   " individuals (a matrix's row sums stay in on-chip memory: ngd_nj_max_ind)");
  return finish_refuse(e, tot_sites, evol_model, w, "no trees");
}

// The matrices in chunks whose working copies (n rows of n doubles each, rows padded to an even length) fit
// NGD_OPT_NJ_MAX_BYTES, one matrix at least; a tree's bits do not depend on the chunk it falls into.  Events 0 and 1 time
// each chunk's kernel (nj.ms: the entry points start it at 0, a windowed call adds up its groups of windows).
// [n_mat][n_pairs] device matrices -> child / len / status in host memory; d_cnt and the two arguments of ngd_finish for sums
// and counts, `values` for cells as they are (the arguments are checked)
static int nj_reduce(ngd_engine *e, const double *d_a, const unsigned long long *d_cnt, bool values, uint64_t n_mat, uint64_t tot_sites,
              uint64_t evol_model, int32_t *child, double *len, uint32_t *status) {
  auto &j = e->nj;
  const uint64_t n = e->g.n_ind, n_pairs = ngd_n_pairs(n), nb = NGD_NJ_NBRANCH(n);
  const uint64_t ld = ngd_nj_ld((uint32_t)n);  // (rows of the working copy: padded to an even length)
  const uint64_t budget = j.max_bytes ? j.max_bytes : 2ull << 30;
  uint64_t chunk = std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(n_mat, (1ull << 31) - 1), budget / (n * ld * 8)));
  // (a CU holds one workgroup of this kernel and every matrix of a call takes about as long: a chunk of whole rounds of the
  // CUs leaves none of them idle behind a few stragglers -- 256 matrices a launch instead of the 268 that fit 2 GB at n = 1000)
  int n_cu = 0;
  if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, e->device) != hipSuccess) { (void)hipGetLastError(); n_cu = 0; }
  if (n_cu > 0 && chunk > (uint64_t)n_cu && chunk < n_mat) chunk -= chunk % (uint64_t)n_cu;
  int rc = j.d_work.ensure(e, chunk * n * ld);
  if (!rc) rc = j.d_child.ensure(e, chunk * nb);
  if (!rc) rc = j.d_len.ensure(e, chunk * nb);
  if (!rc) rc = j.d_status.ensure(e, chunk);
  if (rc) return rc;
  const uint32_t threads = nj_threads();
  for (uint64_t m0 = 0; m0 < n_mat; m0 += chunk) {
    const uint64_t k = std::min(chunk, n_mat - m0);
    HIPCHK(hipEventRecord(e->ev[0], e->st));
    HIPCHK((hipError_t)ngd_launch_nj(e->st, d_a + m0 * n_pairs, d_cnt ? d_cnt + m0 * n_pairs : nullptr, values, k, (uint32_t)n, tot_sites,
                                     (uint32_t)evol_model, threads, j.d_work, j.d_child, j.d_len, j.d_status));
    HIPCHK(hipEventRecord(e->ev[1], e->st));
    HIPCHK(hipMemcpyAsync(child + m0 * nb, j.d_child, k * nb * sizeof(int32_t), hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipMemcpyAsync(len + m0 * nb, j.d_len, k * nb * sizeof(double), hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipMemcpyAsync(status + m0, j.d_status, k * sizeof(uint32_t), hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipStreamSynchronize(e->st));
    float ms = 0;
    hipEventElapsedTime(&ms, e->ev[0], e->ev[1]);
    j.ms += ms;
  }
  return NGD_OK;
}

// matrix 0 of every set: its sums and counts copied out, the tail of gen_dist() on the host (ngd_finish's bits)
int tail_dist0(ngd_engine *e, const double *d_sum, const unsigned long long *d_cnt, uint64_t n_set, uint64_t n_mat, uint64_t tot_sites,
               uint64_t evol_model, double *dist0) {
  const uint64_t n_pairs = ngd_n_pairs(e->g.n_ind);
  std::vector<double> h_sum(n_set * n_pairs);
  std::vector<uint64_t> h_cnt(n_set * n_pairs);
  if (n_mat == 1) {  // (the sets' first matrices are all there is: one copy each, as the _dist sibling makes them)
    const uint32_t valid = e->n_batch_valid;  // (what the engine's batch buffers hold is the caller's to say)
    const int rc = copy_out(e, (uint32_t)n_set, d_sum, d_cnt, h_sum.data(), h_cnt.data());
    e->n_batch_valid = valid;
    if (rc) return rc;
    return ngd_finish(h_sum.data(), h_cnt.data(), n_set * n_pairs, tot_sites, evol_model, dist0);
  }
  for (uint64_t s = 0; s < n_set; s++) {
    HIPCHK(hipMemcpyAsync(&h_sum[s * n_pairs], d_sum + s * n_mat * n_pairs, n_pairs * sizeof(double), hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipMemcpyAsync(&h_cnt[s * n_pairs], d_cnt + s * n_mat * n_pairs, n_pairs * sizeof(uint64_t), hipMemcpyDeviceToHost, e->st));
  }
  HIPCHK(hipStreamSynchronize(e->st));
  return ngd_finish(h_sum.data(), h_cnt.data(), n_set * n_pairs, tot_sites, evol_model, dist0);
}

int ngd_nj_device(ngd_engine *e, const void *d_sum, const void *d_cnt, uint64_t n_mat, uint64_t tot_sites, uint64_t evol_model,
                  int32_t *child, double *len, uint32_t *status) {
  if (int rc = nj_refuse(e, child, len, status, tot_sites, evol_model, "ngd_nj_device")) return rc;
  if (!d_sum || (!d_cnt && !tot_sites) || !n_mat) return fail(NGD_E_INVALID, "ngd_nj_device: null matrices");
  e->nj.ms = 0;
  HIPCHK(hipSetDevice(e->device));
  return nj_reduce(e, (const double *)d_sum, (const unsigned long long *)d_cnt, false, n_mat, tot_sites, evol_model, child, len, status);
}

int ngd_nj_values_device(ngd_engine *e, const void *d_val, uint64_t n_mat, int32_t *child, double *len, uint32_t *status) {
  if (int rc = nj_refuse(e, child, len, status, 0, 0, "ngd_nj_values_device")) return rc;
  if (!d_val || !n_mat) return fail(NGD_E_INVALID, "ngd_nj_values_device: null matrices");
  e->nj.ms = 0;
  HIPCHK(hipSetDevice(e->device));
  return nj_reduce(e, (const double *)d_val, nullptr, true, n_mat, 0, 0, child, len, status);
}

// the tail of the run forms: 2 n - 3 branches per matrix cross the link, set after set into child / len [.][n_mat][2 n - 3]
// and status [.][n_mat] -- and matrix 0 of every set into dist0 [.][n_pairs], if that is asked for
static Tail nj_tail(ngd_engine *e, uint64_t tot_sites, uint64_t evol_model, int32_t *child, double *len, uint32_t *status,
                    double *dist0) {
  return [=](uint64_t set0, uint64_t n_set, uint64_t n_mat) {
    const uint64_t n = e->g.n_ind, nb = NGD_NJ_NBRANCH(n), m0 = set0 * n_mat;
    if (int rc = nj_reduce(e, e->d_bsum, e->d_bcnt, false, n_set * n_mat, tot_sites, evol_model, child + m0 * nb, len + m0 * nb,
                           status + m0))
      return rc;
    return dist0 ? tail_dist0(e, e->d_bsum, e->d_bcnt, n_set, n_mat, tot_sites, evol_model, dist0 + set0 * ngd_n_pairs(n)) : NGD_OK;
  };
}

int ngd_run_job_nj(ngd_engine *e, const uint64_t *block_maps, uint32_t n_rep, uint64_t n_blocks, uint64_t block_size,
                   uint64_t tot_sites, uint64_t evol_model, int32_t *child, double *len, uint32_t *status, double *dist0) {
  if (int rc = nj_refuse(e, child, len, status, tot_sites, evol_model, "ngd_run_job_nj")) return rc;
  if (n_rep && !block_maps) return fail(NGD_E_INVALID, "ngd_run_job_nj: null argument");
  e->nj.ms = 0;
  return job_tail(e, block_maps, n_rep, n_blocks, block_size, nj_tail(e, tot_sites, evol_model, child, len, status, dist0));
}

// the windowed forms: `a` as ngd_run_windows_job_var's, or the windows alone (n_rep 0)
static int windows_nj(ngd_engine *e, const WinJobArgs &a, uint64_t tot_sites, uint64_t evol_model, int32_t *child, double *len,
                      uint32_t *status, double *dist0, const char *who) {
  if (int rc = nj_refuse(e, child, len, status, tot_sites, evol_model, who)) return rc;
  e->nj.ms = 0;
  return windows_tail(e, a, false, who, nj_tail(e, tot_sites, evol_model, child, len, status, dist0));
}

int ngd_run_windows_nj(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win, uint64_t tot_sites,
                       uint64_t evol_model, int32_t *child, double *len, uint32_t *status, double *dist0) {
  return windows_nj(e, WinJobArgs{win_lo, win_hi, n_win, nullptr, 0, nullptr, 0, 0}, tot_sites, evol_model, child, len, status, dist0,
                    "ngd_run_windows_nj");
}

int ngd_run_windows_job_var_nj(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win,
                               const uint64_t *block_maps, uint64_t maps_len, const uint64_t *map_off, uint32_t n_rep,
                               uint64_t block_size, uint64_t tot_sites, uint64_t evol_model, int32_t *child, double *len,
                               uint32_t *status, double *dist0) {
  return windows_nj(e, WinJobArgs{win_lo, win_hi, n_win, block_maps, maps_len, map_off, n_rep, block_size}, tot_sites, evol_model,
                    child, len, status, dist0, "ngd_run_windows_job_var_nj");
}

int ngd_last_nj_ms(const ngd_engine *e, double *ms) {
  if (!e || !ms) return fail(NGD_E_INVALID, "ngd_last_nj_ms: null argument");
  *ms = e->nj.ms;
  return NGD_OK;
}
