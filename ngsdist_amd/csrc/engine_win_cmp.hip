// engine_win_cmp.hip -- comparison of windows (include/ngsdist_amd.h "Comparison of windows"): every vector of a call packed,
// centred, into the resident operand Z (win_cmp.hip), one FP64 MFMA pass Z Z^T over it, and that as a tail (ngd_engine.h)
// behind the window driver: W (W + 2) numbers cross the link instead of W matrices of sums and counts.
#include "ngd_engine.h"

// the outputs of a call: mean [W], gram [W][W], status [W]
struct WinCmpOut {
  double *mean, *gram;
  uint32_t *status;
};

// what every call refuses, before anything is launched
static int wincmp_refuse(const ngd_engine *e, const WinCmpOut &o, uint64_t n_vec, uint64_t tot_sites, uint64_t evol_model, const char *who) {
  const std::string w(who);
  if (!e) return fail(NGD_E_INVALID, w + ": null engine");
  if (!o.mean || !o.gram || !o.status) return fail(NGD_E_INVALID, w + ": null output");
  if (!n_vec) return fail(NGD_E_INVALID, w + ": no vectors");
  if (n_vec > NGD_WIN_CMP_MAX_VEC)
    return fail(NGD_E_INVALID, w + ": more than " + std::to_string(NGD_WIN_CMP_MAX_VEC) + " vectors (ngd_win_cmp_max_vec)");
  return finish_refuse(e, tot_sites, evol_model, w, "no comparison");
}

// Z and the partials of a call of W vectors of P cells, resident until wincmp_close: their bytes are known from (W, P),
// and a call whose bytes exceed the budget (NGD_OPT_WIN_CMP_MAX_BYTES; 0: half of the free device memory now, counting
// what the engine holds of them already) is refused before anything has run.  Z is zeroed here, once: its padding
static int wincmp_open(ngd_engine *e, uint64_t W, uint64_t P, const char *who) {
  auto &c = e->wcmp;
  HIPCHK(hipSetDevice(e->device));
  const uint64_t nz = ngd_wincmp_z_doubles(W, P), np = ngd_wincmp_part_doubles(W, P), need = (nz + np) * sizeof(double);
  uint64_t budget = c.max_bytes;
  if (!budget) {
    size_t fr = 0, tot = 0;
    HIPCHK(hipMemGetInfo(&fr, &tot));
    budget = ((uint64_t)fr + c.Z.bytes() + c.part.bytes()) / 2;
  }
  if (need > budget)
    return fail(NGD_E_INVALID, std::string(who) + ": the operand and the partial sums of " + std::to_string(W) + " vectors of " +
                                   std::to_string(P) + " cells need " + std::to_string(need) + " bytes of device memory, the budget is " +
                                   std::to_string(budget) + " (NGD_OPT_WIN_CMP_MAX_BYTES)");
  int rc = c.Z.ensure(e, nz);
  if (!rc) rc = c.part.ensure(e, np);
  if (!rc) rc = c.d_mean.ensure(e, W);
  if (!rc) rc = c.d_status.ensure(e, W);
  if (!rc) rc = c.d_gram.ensure(e, W * W);
  if (rc) return rc;
  HIPCHK(hipMemsetAsync(c.Z, 0, nz * sizeof(double), e->st));
  for (double &m : c.ms) m = 0;
  return NGD_OK;
}

// vectors [w0, w0 + n_vec) of the call's W: [n_vec][P] device vectors -> their means and status, their rows of Z.  d_cnt and
// the two arguments of ngd_finish for sums and counts, `values` for cells as they are (the arguments are checked).
// Events 0 .. 2 time the two kernels
static int wincmp_reduce(ngd_engine *e, const double *d_a, const unsigned long long *d_cnt, bool values, uint64_t w0, uint64_t n_vec,
                         uint64_t W, uint64_t P, uint64_t tot_sites, uint64_t evol_model) {
  auto &c = e->wcmp;
  HIPCHK(hipEventRecord(e->ev[0], e->st));
  HIPCHK((hipError_t)ngd_launch_wincmp_stats(e->st, d_a, d_cnt, values, n_vec, P, tot_sites, (uint32_t)evol_model, w0, c.d_mean, c.d_status));
  HIPCHK(hipEventRecord(e->ev[1], e->st));
  HIPCHK((hipError_t)ngd_launch_wincmp_pack(e->st, d_a, d_cnt, values, n_vec, P, tot_sites, (uint32_t)evol_model, w0, W, c.d_mean,
                                            c.d_status, c.Z));
  HIPCHK(hipEventRecord(e->ev[2], e->st));
  HIPCHK(hipStreamSynchronize(e->st));
  float ms = 0;
  hipEventElapsedTime(&ms, e->ev[0], e->ev[1]);
  c.ms[0] += ms;
  hipEventElapsedTime(&ms, e->ev[1], e->ev[2]);
  c.ms[1] += ms;
  return NGD_OK;
}

// Z -> gram; mean, gram and status to the caller.  Events 0 .. 2 time the two kernels
static int wincmp_close(ngd_engine *e, uint64_t W, uint64_t P, const WinCmpOut &o) {
  auto &c = e->wcmp;
  HIPCHK(hipEventRecord(e->ev[0], e->st));
  HIPCHK((hipError_t)ngd_launch_wincmp_gram(e->st, c.Z, W, P, c.part));
  HIPCHK(hipEventRecord(e->ev[1], e->st));
  HIPCHK((hipError_t)ngd_launch_wincmp_sum(e->st, c.part, W, P, c.d_status, c.d_gram));
  HIPCHK(hipEventRecord(e->ev[2], e->st));
  // (staged: a refused or failed call leaves the caller's arrays as they were until everything has been computed)
  std::vector<double> mean(W);
  std::vector<uint32_t> status(W);
  HIPCHK(hipMemcpyAsync(mean.data(), c.d_mean, W * sizeof(double), hipMemcpyDeviceToHost, e->st));
  HIPCHK(hipMemcpyAsync(status.data(), c.d_status, W * sizeof(uint32_t), hipMemcpyDeviceToHost, e->st));
  HIPCHK(hipMemcpyAsync(o.gram, c.d_gram, W * W * sizeof(double), hipMemcpyDeviceToHost, e->st));
  HIPCHK(hipStreamSynchronize(e->st));
  std::copy(mean.begin(), mean.end(), o.mean);
  std::copy(status.begin(), status.end(), o.status);
  float ms = 0;
  hipEventElapsedTime(&ms, e->ev[0], e->ev[1]);
  c.ms[2] += ms;
  hipEventElapsedTime(&ms, e->ev[1], e->ev[2]);
  c.ms[3] += ms;
  return NGD_OK;
}

static int wincmp_call(ngd_engine *e, const double *d_a, const unsigned long long *d_cnt, bool values, uint64_t W, uint64_t P,
                       uint64_t tot_sites, uint64_t evol_model, const WinCmpOut &o, const char *who) {
  if (int rc = wincmp_open(e, W, P, who)) return rc;
  if (int rc = wincmp_reduce(e, d_a, d_cnt, values, 0, W, W, P, tot_sites, evol_model)) return rc;
  return wincmp_close(e, W, P, o);
}

int ngd_win_cmp_device(ngd_engine *e, const void *d_sum, const void *d_cnt, uint64_t n_vec, uint64_t tot_sites, uint64_t evol_model,
                       double *mean, double *gram, uint32_t *status) {
  const char *who = "ngd_win_cmp_device";
  const WinCmpOut o{mean, gram, status};
  if (int rc = wincmp_refuse(e, o, n_vec, tot_sites, evol_model, who)) return rc;
  if (!d_sum || (!d_cnt && !tot_sites)) return fail(NGD_E_INVALID, std::string(who) + ": null matrices");
  if (e->g.n_ind < 2) return fail(NGD_E_INVALID, std::string(who) + ": a matrix of one individual has no cell");
  return wincmp_call(e, (const double *)d_sum, (const unsigned long long *)d_cnt, false, n_vec, ngd_n_pairs(e->g.n_ind), tot_sites,
                     evol_model, o, who);
}

int ngd_win_cmp_values_device(ngd_engine *e, const void *d_val, uint64_t n_vec, uint64_t n_cells, double *mean, double *gram,
                              uint32_t *status) {
  const char *who = "ngd_win_cmp_values_device";
  const WinCmpOut o{mean, gram, status};
  if (int rc = wincmp_refuse(e, o, n_vec, 0, 0, who)) return rc;
  if (!d_val) return fail(NGD_E_INVALID, std::string(who) + ": null vectors");
  if (!n_cells) return fail(NGD_E_INVALID, std::string(who) + ": no cells");
  return wincmp_call(e, (const double *)d_val, nullptr, true, n_vec, n_cells, 0, 0, o, who);
}

int ngd_run_windows_cmp(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win, uint64_t tot_sites,
                        uint64_t evol_model, double *mean, double *gram, uint32_t *status, double *dist) {
  const char *who = "ngd_run_windows_cmp";
  const WinCmpOut o{mean, gram, status};
  // (no windows: the windows' own check says so, in its words)
  if (int rc = wincmp_refuse(e, o, n_win ? n_win : 1, tot_sites, evol_model, who)) return rc;
  if (e->g.n_ind < 2) return fail(NGD_E_INVALID, std::string(who) + ": a matrix of one individual has no cell");
  const uint64_t P = ngd_n_pairs(e->g.n_ind);
  // the tail: a group's sets (one matrix each) into Z at set0 -- and finished into dist, if asked for (every matrix is its
  // set's matrix 0: ngd_finish's bits)
  const Tail tail = [=](uint64_t set0, uint64_t n_set, uint64_t n_mat) {
    if (int rc = wincmp_reduce(e, e->d_bsum, e->d_bcnt, false, set0, n_set * n_mat, n_win, P, tot_sites, evol_model)) return rc;
    return dist ? tail_dist0(e, e->d_bsum, e->d_bcnt, n_set, n_mat, tot_sites, evol_model, dist + set0 * P) : NGD_OK;
  };
  // Z and the partials are there before the windows are planned: the batches' 85 % rule sees what is left
  if (int rc = windows_tail(e, WinJobArgs{win_lo, win_hi, n_win, nullptr, 0, nullptr, 0, 0}, false, who, tail,
                            [&] { return wincmp_open(e, n_win, P, who); }))
    return rc;
  return wincmp_close(e, n_win, P, o);
}

int ngd_last_win_cmp_ms(const ngd_engine *e, double ms[4]) {
  if (!e || !ms) return fail(NGD_E_INVALID, "ngd_last_win_cmp_ms: null argument");
  for (int k = 0; k < 4; k++) ms[k] = e->wcmp.ms[k];
  return NGD_OK;
}
