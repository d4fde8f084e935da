// engine_mds.hip -- classical MDS: the top K eigenpairs of every device matrix's double-centred form (mds.hip, one workgroup
// per matrix), and that reduction as a tail (ngd_engine.h) behind the job driver and the window driver: the run forms,
// where K (n + 1) + 2 numbers per matrix cross the link instead of n (n - 1) / 2 sums and counts.  The aligned forms go on from
// there on the device: the replicates of every set rotated onto its matrix 0 (mds_align.hip), the aligned cells summarised
// (engine_boot_stats.hip's boot_reduce).
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

// where the aligned forms have mds_reduce leave a call's matrices on the device: cells [.][K (n + 1)] (mds_align.hip), status
// [.]; n_mat matrices to a set
struct MdsSink {
  double *d_cells;
  uint32_t *d_status;
  uint64_t n_mat;
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
// With a sink (the aligned forms) every chunk's coordinates, eigenvalues and status also stay on the device, in buffers that
// hold the whole call (a chunk may cut a set in two), and only matrix 0 of every set of sink->n_mat matrices goes to the
// host: o.eig / o.vec / o.tot are [n_set][..] then, o.status [n_mat] as ever.  Events 2 and 3 time that kernel (mal.ms)
static int mds_reduce(ngd_engine *e, const double *d_a, const unsigned long long *d_cnt, bool values, uint64_t n_mat, uint64_t tot_sites,
                      uint64_t evol_model, uint32_t K, const MdsOut &o, const MdsSink *sink = nullptr) {
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
    if (!sink) {
      HIPCHK(hipMemcpyAsync(o.eig + m0 * K, j.d_eig, k * K * sizeof(double), hipMemcpyDeviceToHost, e->st));
      HIPCHK(hipMemcpyAsync(o.vec + m0 * K * n, j.d_vec, k * K * n * sizeof(double), hipMemcpyDeviceToHost, e->st));
      HIPCHK(hipMemcpyAsync(o.tot + m0 * 2, j.d_tot, k * 2 * sizeof(double), hipMemcpyDeviceToHost, e->st));
    } else {
      HIPCHK(hipEventRecord(e->ev[2], e->st));
      HIPCHK((hipError_t)ngd_launch_mds_coords(e->st, j.d_eig, j.d_vec, j.d_status, k, (uint32_t)n, K, sink->d_cells + m0 * K * (n + 1),
                                               sink->d_status + m0));
      HIPCHK(hipEventRecord(e->ev[3], e->st));
      // the sets whose matrix 0 lies in this chunk: [s0, s1), the first of them `at` matrices into the chunk, a set apart
      const uint64_t s0 = (m0 + sink->n_mat - 1) / sink->n_mat, s1 = (m0 + k + sink->n_mat - 1) / sink->n_mat, at = s0 * sink->n_mat - m0;
      auto firsts = [&](double *dst, const double *src, uint64_t per) {  // `per` doubles of each such matrix
        return hipMemcpy2DAsync(dst + s0 * per, per * sizeof(double), src + at * per, sink->n_mat * per * sizeof(double),
                                per * sizeof(double), s1 - s0, hipMemcpyDeviceToHost, e->st);
      };
      if (s1 > s0) {
        HIPCHK(firsts(o.eig, j.d_eig, K));
        HIPCHK(firsts(o.vec, j.d_vec, K * n));
        HIPCHK(firsts(o.tot, j.d_tot, 2));
      }
    }
    HIPCHK(hipMemcpyAsync(o.status + m0, j.d_status, k * sizeof(uint32_t), hipMemcpyDeviceToHost, e->st));
    HIPCHK(hipStreamSynchronize(e->st));
    float ms = 0;
    hipEventElapsedTime(&ms, e->ev[0], e->ev[1]);
    j.ms += ms;
    if (sink) {
      hipEventElapsedTime(&ms, e->ev[2], e->ev[3]);
      e->mal.ms += ms;
    }
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

// ---- the replicates of every set rotated onto its matrix 0 (mds_align.hip), and the summary of the aligned cells ----

// [n_set][n_mat] matrices in mal.d_cells, `stride` doubles apart, status in mal.d_status (or none): rotated in place; fit
// [n_set][n_mat] and, if asked for, the coordinates [n_set][n_mat][K][n] to the host.  Events 2 and 3 time the kernel
static int align_cells(ngd_engine *e, uint64_t stride, bool with_status, uint64_t n_set, uint64_t n_mat, uint32_t K, double *aligned,
                       double *fit) {
  auto &a = e->mal;
  const uint64_t n = e->g.n_ind, total = n_set * n_mat;
  if (int rc = a.d_fit.ensure(e, total)) return rc;
  HIPCHK(hipEventRecord(e->ev[2], e->st));
  HIPCHK((hipError_t)ngd_launch_mds_align(e->st, a.d_cells, stride, with_status ? a.d_status.get() : nullptr, n_set, (uint32_t)n_mat,
                                          (uint32_t)n, K, a.d_fit));
  HIPCHK(hipEventRecord(e->ev[3], e->st));
  HIPCHK(hipMemcpyAsync(fit, a.d_fit, total * sizeof(double), hipMemcpyDeviceToHost, e->st));
  if (aligned)
    HIPCHK(hipMemcpy2DAsync(aligned, K * n * sizeof(double), a.d_cells, stride * sizeof(double), K * n * sizeof(double), total,
                            hipMemcpyDeviceToHost, e->st));
  HIPCHK(hipStreamSynchronize(e->st));
  float ms = 0;
  hipEventElapsedTime(&ms, e->ev[2], e->ev[3]);
  a.ms += ms;
  return NGD_OK;
}

int ngd_mds_align_values_device(ngd_engine *e, const void *d_coords, const uint32_t *status, uint64_t n_set, uint64_t n_mat,
                                uint32_t K, double *aligned, double *fit) {
  const char *who = "ngd_mds_align_values_device";
  if (!e) return fail(NGD_E_INVALID, std::string(who) + ": null engine");
  if (!d_coords || !aligned || !fit || !n_set || !n_mat) return fail(NGD_E_INVALID, std::string(who) + ": null argument");
  if (n_set >= (1ull << 31) || n_mat >= (1ull << 31) || n_set * n_mat >= (1ull << 31))
    return fail(NGD_E_INVALID, std::string(who) + ": too many matrices (2^31 and more)");
  if (e->g.n_ind < 3 || !K || K > e->g.n_ind - 1 || K > ngd_mds_max_dim())
    return fail(NGD_E_INVALID, std::string(who) + ": K must lie in 1 .. min(n_ind - 1, " + std::to_string(ngd_mds_max_dim()) + ")");
  auto &a = e->mal;
  const uint64_t total = n_set * n_mat, stride = (uint64_t)K * e->g.n_ind;
  a.ms = 0;
  HIPCHK(hipSetDevice(e->device));
  if (int rc = a.d_cells.ensure(e, total * stride)) return rc;
  HIPCHK(hipMemcpyAsync(a.d_cells, d_coords, total * stride * sizeof(double), hipMemcpyDeviceToDevice, e->st));
  if (status) {
    if (int rc = a.d_status.ensure(e, total)) return rc;
    HIPCHK(hipMemcpyAsync(a.d_status, status, total * sizeof(uint32_t), hipMemcpyHostToDevice, e->st));
  }
  return align_cells(e, stride, status != nullptr, n_set, n_mat, K, aligned, fit);
}

// the outputs of an aligned call beyond matrix 0's MdsOut
struct AlignOut {
  double *stats;
  uint64_t *used;
  double *fit, *aligned;
};

// the tail of the aligned run forms: mds_reduce with the call's cells kept on the device, the alignment over whole sets,
// the summaries of the aligned cells and the eigenvalues (n_cells = K (n + 1)); used: a set's replicates that went in
static Tail mds_align_tail(ngd_engine *e, uint64_t tot_sites, uint64_t evol_model, uint32_t K, BootCi ci, MdsOut o, AlignOut x,
                           double *dist0) {
  return [=](uint64_t set0, uint64_t n_set, uint64_t n_mat) {
    auto &a = e->mal;
    const uint64_t n = e->g.n_ind, n_cells = (uint64_t)K * (n + 1), total = n_set * n_mat;
    int rc = a.d_cells.ensure(e, total * n_cells);
    if (!rc) rc = a.d_status.ensure(e, total);
    if (rc) return rc;
    const MdsOut at{o.eig + set0 * K, o.vec + set0 * K * n, o.tot + set0 * 2, o.status + set0 * n_mat};
    const MdsSink sink{a.d_cells, a.d_status, n_mat};
    if ((rc = mds_reduce(e, e->d_bsum, e->d_bcnt, false, total, tot_sites, evol_model, K, at, &sink))) return rc;
    if ((rc = align_cells(e, n_cells, true, n_set, n_mat, K, x.aligned ? x.aligned + set0 * n_mat * K * n : nullptr, x.fit + set0 * n_mat)))
      return rc;
    std::vector<uint64_t> used(n_set * n_cells);  // (per cell; a replicate's cells go in or stay out together)
    if ((rc = boot_reduce(e, a.d_cells, nullptr, true, n_set, n_mat, n_cells, 0, 0, ci, x.stats + set0 * NGD_BOOT_NSTAT * n_cells, used.data())))
      return rc;
    for (uint64_t s = 0; s < n_set; s++) x.used[set0 + s] = used[s * n_cells];
    return dist0 ? tail_dist0(e, e->d_bsum, e->d_bcnt, n_set, n_mat, tot_sites, evol_model, dist0 + set0 * ngd_n_pairs(n)) : NGD_OK;
  };
}

// what the aligned forms refuse: the _mds sibling's, then the summaries'
static int align_refuse(const ngd_engine *e, uint32_t K, const MdsOut &o, const AlignOut &x, uint32_t n_rep, double ci, uint64_t tot_sites,
                        uint64_t evol_model, const char *who, BootCi &c) {
  if (int rc = mds_refuse(e, K, o, tot_sites, evol_model, who)) return rc;
  if (!x.fit) return fail(NGD_E_INVALID, std::string(who) + ": null output");
  return boot_refuse(e, x.stats, x.used, (uint64_t)n_rep + 1, ci, tot_sites, evol_model, false, who, c);
}

int ngd_run_job_mds_align(ngd_engine *e, const uint64_t *block_maps, uint32_t n_rep, uint64_t n_blocks, uint64_t block_size,
                          uint64_t tot_sites, uint64_t evol_model, uint32_t K, double ci, double *eig0, double *vec0, double *tot0,
                          uint32_t *status, double *stats, uint64_t *used, double *fit, double *aligned, double *dist0) {
  const MdsOut o{eig0, vec0, tot0, status};
  const AlignOut x{stats, used, fit, aligned};
  BootCi c{};
  if (int rc = align_refuse(e, K, o, x, n_rep, ci, tot_sites, evol_model, "ngd_run_job_mds_align", c)) return rc;
  if (!block_maps) return fail(NGD_E_INVALID, "ngd_run_job_mds_align: null argument");
  e->mds.ms = e->mal.ms = e->bst.ms = 0;
  return job_tail(e, block_maps, n_rep, n_blocks, block_size, mds_align_tail(e, tot_sites, evol_model, K, c, o, x, dist0));
}

int ngd_run_windows_job_var_mds_align(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win,
                                      const uint64_t *block_maps, uint64_t maps_len, const uint64_t *map_off, uint32_t n_rep,
                                      uint64_t block_size, uint64_t tot_sites, uint64_t evol_model, uint32_t K, double ci,
                                      double *eig0, double *vec0, double *tot0, uint32_t *status, double *stats, uint64_t *used,
                                      double *fit, double *aligned, double *dist0) {
  const char *who = "ngd_run_windows_job_var_mds_align";
  const MdsOut o{eig0, vec0, tot0, status};
  const AlignOut x{stats, used, fit, aligned};
  BootCi c{};
  if (int rc = align_refuse(e, K, o, x, n_rep, ci, tot_sites, evol_model, who, c)) return rc;
  e->mds.ms = e->mal.ms = e->bst.ms = 0;
  return windows_tail(e, WinJobArgs{win_lo, win_hi, n_win, block_maps, maps_len, map_off, n_rep, block_size}, true, who,
                      mds_align_tail(e, tot_sites, evol_model, K, c, o, x, dist0));
}

int ngd_last_mds_align_ms(const ngd_engine *e, double *ms) {
  if (!e || !ms) return fail(NGD_E_INVALID, "ngd_last_mds_align_ms: null argument");
  *ms = e->mal.ms;
  return NGD_OK;
}

int ngd_last_mds_ms(const ngd_engine *e, double *ms) {
  if (!e || !ms) return fail(NGD_E_INVALID, "ngd_last_mds_ms: null argument");
  *ms = e->mds.ms;
  return NGD_OK;
}
