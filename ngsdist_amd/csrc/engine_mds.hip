// engine_mds.hip -- classical MDS: the top K eigenpairs of every device matrix's double-centred form (mds.hip, one workgroup
// per matrix), and that reduction as a tail (ngd_engine.h) behind the job driver and the window driver: the run forms,
// where K (n + 1) + 2 numbers per matrix cross the link instead of n (n - 1) / 2 sums and counts.
#include "ngd_engine.h"

#include <cstdlib>

uint32_t ngd_mds_max_ind(void) { return NGD_MDS_MAX_IND; }

// the workgroup: NGD_MDS_THREADS, or what NGD_MDS_WG names (256, 512, 1024: for measurement; the sums' trees follow it)
static uint32_t mds_threads() {
  if (const char *s = getenv("NGD_MDS_WG")) {
    const long v = atol(s);
    if (v == 256 || v == 512 || v == 1024) return (uint32_t)v;
  }
  return NGD_MDS_THREADS;
}

// the outputs of a call: eig [.][K], vec [.][K][n], tot [.][2], status [.]
struct MdsOut {
  double *eig, *vec, *tot;
  uint32_t *status;
};

// what every call that computes coordinates refuses, before anything is launched
static int mds_refuse(const ngd_engine *e, uint32_t K, const MdsOut &o, uint64_t tot_sites, uint64_t evol_model, const char *who) {
  const std::string w(who);
  if (!e) return fail(NGD_E_INVALID, w + ": null engine");
  if (!o.eig || !o.vec || !o.tot || !o.status) return fail(NGD_E_INVALID, w + ": null output");
  if (e->g.n_ind < 3) return fail(NGD_E_INVALID, w + ": coordinates need three individuals or more");
  if (e->g.n_ind > ngd_mds_max_ind())
    return fail(NGD_E_INVALID, w + ": more than " + std::to_string(ngd_mds_max_ind()) +
                                   " individuals (a matrix's tridiagonal form stays in on-chip memory: ngd_mds_max_ind)");
  if (!K || K > e->g.n_ind - 1 || K > ngd_mds_max_dim())
    return fail(NGD_E_INVALID, w + ": K must lie in 1 .. min(n_ind - 1, " + std::to_string(ngd_mds_max_dim()) + ")");
  return finish_refuse(e, tot_sites, evol_model, w, "no coordinates");
}

// The matrices in chunks whose scratch (the working copy, n rows padded to an even length, and 4 K such rows for the
// vectors) fits NGD_OPT_MDS_MAX_BYTES, one matrix at least; a matrix's bits do not depend on the chunk it falls into.
// Events 0 and 1 time each chunk's kernel (mds.ms: the entry points start it at 0, a windowed call adds up its groups).
// [n_mat][n_pairs] device matrices -> o in host memory; d_cnt and the two arguments of ngd_finish for sums and counts,
// `values` for cells as they are (the arguments are checked)
static int mds_reduce(ngd_engine *e, const double *d_a, const unsigned long long *d_cnt, bool values, uint64_t n_mat, uint64_t tot_sites,
                      uint64_t evol_model, uint32_t K, const MdsOut &o) {
  auto &j = e->mds;
  const uint64_t n = e->g.n_ind, n_pairs = ngd_n_pairs(n), ld = ngd_nj_ld((uint32_t)n);
  const uint64_t budget = j.max_bytes ? j.max_bytes : 2ull << 30, per_mat = (n + NGD_MDS_AUX_ROWS * K) * ld * 8;
  uint64_t chunk = std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(n_mat, (1ull << 31) - 1), budget / per_mat));
  // (a CU holds one workgroup of this kernel and every matrix of a call takes about as long: whole rounds of the CUs, as nj)
  int n_cu = 0;
  if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, e->device) != hipSuccess) { (void)hipGetLastError(); n_cu = 0; }
  if (n_cu > 0 && chunk > (uint64_t)n_cu && chunk < n_mat) chunk -= chunk % (uint64_t)n_cu;
  int rc = j.d_work.ensure(e, chunk * n * ld);
  if (!rc) rc = j.d_aux.ensure(e, chunk * NGD_MDS_AUX_ROWS * K * ld);
  if (!rc) rc = j.d_eig.ensure(e, chunk * K);
  if (!rc) rc = j.d_vec.ensure(e, chunk * K * n);
  if (!rc) rc = j.d_tot.ensure(e, chunk * 2);
  if (!rc) rc = j.d_status.ensure(e, chunk);
  if (rc) return rc;
  const uint32_t threads = mds_threads();
  for (uint64_t m0 = 0; m0 < n_mat; m0 += chunk) {
    const uint64_t k = std::min(chunk, n_mat - m0);
    HIPCHK(hipEventRecord(e->ev[0], e->st));
    HIPCHK((hipError_t)ngd_launch_mds(e->st, d_a + m0 * n_pairs, d_cnt ? d_cnt + m0 * n_pairs : nullptr, values, k, (uint32_t)n, tot_sites,
                                      (uint32_t)evol_model, K, threads, j.d_work, j.d_aux, j.d_eig, j.d_vec, j.d_tot, j.d_status));
    HIPCHK(hipEventRecord(e->ev[1], e->st));
    HIPCHK(hipMemcpyAsync(o.eig + m0 * K, j.d_eig, k * K * sizeof(double), hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipMemcpyAsync(o.vec + m0 * K * n, j.d_vec, k * K * n * sizeof(double), hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipMemcpyAsync(o.tot + m0 * 2, j.d_tot, k * 2 * sizeof(double), hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipMemcpyAsync(o.status + m0, j.d_status, k * sizeof(uint32_t), hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipStreamSynchronize(e->st));
    float ms = 0;
    hipEventElapsedTime(&ms, e->ev[0], e->ev[1]);
    j.ms += ms;
  }
  return NGD_OK;
}

int ngd_mds_device(ngd_engine *e, const void *d_sum, const void *d_cnt, uint64_t n_mat, uint64_t tot_sites, uint64_t evol_model,
                   uint32_t K, double *eig, double *vec, double *tot, uint32_t *status) {
  const MdsOut o{eig, vec, tot, status};
  if (int rc = mds_refuse(e, K, o, tot_sites, evol_model, "ngd_mds_device")) return rc;
  if (!d_sum || (!d_cnt && !tot_sites) || !n_mat) return fail(NGD_E_INVALID, "ngd_mds_device: null matrices");
  e->mds.ms = 0;
  HIPCHK(hipSetDevice(e->device));
  return mds_reduce(e, (const double *)d_sum, (const unsigned long long *)d_cnt, false, n_mat, tot_sites, evol_model, K, o);
}

int ngd_mds_values_device(ngd_engine *e, const void *d_val, uint64_t n_mat, uint32_t K, double *eig, double *vec, double *tot,
                          uint32_t *status) {
  const MdsOut o{eig, vec, tot, status};
  if (int rc = mds_refuse(e, K, o, 0, 0, "ngd_mds_values_device")) return rc;
  if (!d_val || !n_mat) return fail(NGD_E_INVALID, "ngd_mds_values_device: null matrices");
  e->mds.ms = 0;
  HIPCHK(hipSetDevice(e->device));
  return mds_reduce(e, (const double *)d_val, nullptr, true, n_mat, 0, 0, K, o);
}

// the tail of the run forms: the outputs set after set -- and matrix 0 of every set into dist0 [.][n_pairs], if asked for
static Tail mds_tail(ngd_engine *e, uint64_t tot_sites, uint64_t evol_model, uint32_t K, MdsOut o, double *dist0) {
  return [=](uint64_t set0, uint64_t n_set, uint64_t n_mat) {
    const uint64_t n = e->g.n_ind, m0 = set0 * n_mat;
    const MdsOut at{o.eig + m0 * K, o.vec + m0 * K * n, o.tot + m0 * 2, o.status + m0};
    if (int rc = mds_reduce(e, e->d_bsum, e->d_bcnt, false, n_set * n_mat, tot_sites, evol_model, K, at)) return rc;
    return dist0 ? tail_dist0(e, e->d_bsum, e->d_bcnt, n_set, n_mat, tot_sites, evol_model, dist0 + set0 * ngd_n_pairs(n)) : NGD_OK;
  };
}

int ngd_run_job_mds(ngd_engine *e, const uint64_t *block_maps, uint32_t n_rep, uint64_t n_blocks, uint64_t block_size,
                    uint64_t tot_sites, uint64_t evol_model, uint32_t K, double *eig, double *vec, double *tot, uint32_t *status,
                    double *dist0) {
  const MdsOut o{eig, vec, tot, status};
  if (int rc = mds_refuse(e, K, o, tot_sites, evol_model, "ngd_run_job_mds")) return rc;
  if (n_rep && !block_maps) return fail(NGD_E_INVALID, "ngd_run_job_mds: null argument");
  e->mds.ms = 0;
  return job_tail(e, block_maps, n_rep, n_blocks, block_size, mds_tail(e, tot_sites, evol_model, K, o, dist0));
}

// the windowed forms: `a` as ngd_run_windows_job_var's, or the windows alone (n_rep 0)
static int windows_mds(ngd_engine *e, const WinJobArgs &a, uint64_t tot_sites, uint64_t evol_model, uint32_t K, const MdsOut &o,
                       double *dist0, const char *who) {
  if (int rc = mds_refuse(e, K, o, tot_sites, evol_model, who)) return rc;
  e->mds.ms = 0;
  return windows_tail(e, a, false, who, mds_tail(e, tot_sites, evol_model, K, o, dist0));
}

int ngd_run_windows_mds(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win, uint64_t tot_sites,
                        uint64_t evol_model, uint32_t K, double *eig, double *vec, double *tot, uint32_t *status, double *dist0) {
  return windows_mds(e, WinJobArgs{win_lo, win_hi, n_win, nullptr, 0, nullptr, 0, 0}, tot_sites, evol_model, K,
                     MdsOut{eig, vec, tot, status}, dist0, "ngd_run_windows_mds");
}

int ngd_run_windows_job_var_mds(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win,
                                const uint64_t *block_maps, uint64_t maps_len, const uint64_t *map_off, uint32_t n_rep,
                                uint64_t block_size, uint64_t tot_sites, uint64_t evol_model, uint32_t K, double *eig, double *vec,
                                double *tot, uint32_t *status, double *dist0) {
  return windows_mds(e, WinJobArgs{win_lo, win_hi, n_win, block_maps, maps_len, map_off, n_rep, block_size}, tot_sites, evol_model, K,
                     MdsOut{eig, vec, tot, status}, dist0, "ngd_run_windows_job_var_mds");
}

int ngd_last_mds_ms(const ngd_engine *e, double *ms) {
  if (!e || !ms) return fail(NGD_E_INVALID, "ngd_last_mds_ms: null argument");
  *ms = e->mds.ms;
  return NGD_OK;
}
