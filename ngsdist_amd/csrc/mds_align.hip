// mds_align.hip -- the MDS replicates of a set rotated onto its matrix 0 (include/ngsdist_amd.h "Classical MDS", alignment, is
// the contract: Y_r = X_r Q with Q the orthogonal polar factor of M = X_r^T X_0, fit_r = |Y_r - X_0|^2).
//
// k_mds_coords turns a chunk of mds.hip's outputs into cells: per matrix X as [K][n], then its K eigenvalues -- the layout
// the summaries reduce -- in a buffer that holds the whole call (a chunk of the MDS kernel may cut a set in two).
// k_mds_align: one workgroup of 256 threads per (set, replicate), no workgroup talks to another, no atomics, every sum a
// fixed tree -- a lane's own rows in ascending order, the butterfly over the lanes, the waves' slots in order -- so a
// matrix's bits are a function of (X_r, X_0, K) alone.
//   M      for every row a of X_r a lane keeps K partial sums over its individuals; one barrier for all K^2 entries
//   Q      wave 0: lane i owns row i of M and of V in LDS (no lane reads what another wrote; what lanes share goes through
//          the butterfly, whose result has the same bits in every lane, so the wave's branches are uniform).  One-sided
//          Jacobi on the columns of M scaled by a power of two, cyclic order; the columns below the floor replaced by
//          Gram-Schmidt of e_0, e_1, ..; then Q = U V^T by K^2 threads behind a barrier
//   Y      thread i rotates individual i: its K coordinates are read before any is written, so Y replaces X in place
#include "ngd_internal.h"

#define MAL_THREADS NGD_MDS_ALIGN_THREADS
#define MAL_WAVES (MAL_THREADS / 64u)
#define MAL_K NGD_MDS_MAX_DIM
#define MAL_LD (MAL_K + 1u)  // a lane's row in LDS: an odd stride, the lanes' rows fall into different banks
#define MAL_SWEEPS 64
#define MAL_EPS 2.220446049250313e-16
#define MAL_FLOOR 1e-12
// a thread per entry of M and of Q, a lane of wave 0 per row, a bit of `done` per column
static_assert(MAL_K * MAL_K <= MAL_THREADS && MAL_K <= 32 && MAL_THREADS % 64 == 0, "k_mds_align: K^2 threads, K lanes, whole waves");

__device__ inline double mal_wave_sum(double x) {
#pragma unroll
  for (int off = 32; off; off >>= 1) x += __shfl_xor(x, off);
  return x;
}
__device__ inline double mal_wave_max(double x) {
#pragma unroll
  for (int off = 32; off; off >>= 1) x = fmax(x, __shfl_xor(x, off));
  return x;
}

// one workgroup per matrix of the chunk: cells [K][n] = vec scaled by the roots of eig (ngd_mds_coords' formula), then eig
__global__ __launch_bounds__(MAL_THREADS) void k_mds_coords(const double *__restrict__ d_eig, const double *__restrict__ d_vec,
                                                            const uint32_t *__restrict__ d_status, uint32_t n, uint32_t K,
                                                            double *__restrict__ d_cells, uint32_t *__restrict__ d_status_out) {
  __shared__ double root[MAL_K];
  const uint32_t tid = threadIdx.x;
  const uint64_t m = blockIdx.x, kn = (uint64_t)K * n;
  const double *eig = d_eig + m * K, *vec = d_vec + m * kn;
  double *cells = d_cells + m * (kn + K);
  if (tid < K) {
    const double l = eig[tid];
    root[tid] = l > 0.0 ? sqrt(l) : l - l;  // (0 for an eigenvalue <= 0, NaN for NaN)
    cells[kn + tid] = l;
  }
  if (!tid) d_status_out[m] = d_status[m];
  __syncthreads();
  for (uint32_t k = 0; k < K; k++) {
    const double s = root[k];
    for (uint32_t i = tid; i < n; i += MAL_THREADS) cells[(uint64_t)k * n + i] = vec[(uint64_t)k * n + i] * s;
  }
}

// d_cells: [n_set * n_mat] matrices of `stride` doubles, [K][n] coordinates first; d_status NULL: every matrix has status 1
__global__ __launch_bounds__(MAL_THREADS) void k_mds_align(double *d_cells, uint64_t stride, const uint32_t *__restrict__ d_status,
                                                           uint32_t n_mat, uint32_t n, uint32_t K, double *__restrict__ d_fit) {
  __shared__ double part[MAL_K][MAL_WAVES][MAL_K];
  __shared__ double Mq[MAL_K * MAL_K];  // M as the sums give it; later Q
  __shared__ double A[MAL_K * MAL_LD], V[MAL_K * MAL_LD];
  __shared__ double slots[MAL_WAVES];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint64_t m = blockIdx.x, m0 = m - m % n_mat;
  double *x = d_cells + m * stride;
  const double *x0 = d_cells + m0 * stride;
  if (d_status && (!d_status[m] || !d_status[m0])) {  // (the whole workgroup alike)
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    for (uint64_t i = tid; i < stride; i += MAL_THREADS) x[i] = nan;
    if (!tid) d_fit[m] = nan;
    return;
  }
  if (m == m0) {
    if (!tid) d_fit[m] = 0.0;
    return;
  }

  // ---- M[a][b] = SUM_i X_r[a][i] X_0[b][i] ----
  for (uint32_t a = 0; a < K; a++) {
    double acc[MAL_K];
#pragma unroll
    for (uint32_t b = 0; b < MAL_K; b++) acc[b] = 0.0;
    for (uint32_t i = tid; i < n; i += MAL_THREADS) {
      const double xr = x[(uint64_t)a * n + i];
#pragma unroll
      for (uint32_t b = 0; b < MAL_K; b++)
        if (b < K) acc[b] += xr * x0[(uint64_t)b * n + i];
    }
#pragma unroll
    for (uint32_t b = 0; b < MAL_K; b++)
      if (b < K) {  // (K is the workgroup's: the butterfly runs in whole waves)
        const double s = mal_wave_sum(acc[b]);
        if (!lane) part[a][wave][b] = s;
      }
  }
  __syncthreads();
  if (tid < K * K) {
    const uint32_t a = tid / K, b = tid % K;
    double s = 0.0;
    for (uint32_t w = 0; w < MAL_WAVES; w++) s += part[a][w][b];
    Mq[tid] = s;
  }
  __syncthreads();

  // ---- the polar factor: wave 0, lane i on row i ----
  if (!wave) {
    const bool mine = lane < K;
    double *ar = A + lane * MAL_LD, *vr = V + lane * MAL_LD;  // (touched by the lanes below K alone)
    double big = 0.0;
    if (mine)
      for (uint32_t j = 0; j < K; j++) big = fmax(big, fabs(Mq[lane * K + j]));
    big = mal_wave_max(big);
    const bool any = big > 0.0 && isfinite(big);
    const int ex = any ? ilogb(big) : 0;
    if (mine)
      for (uint32_t j = 0; j < K; j++) {
        ar[j] = any ? scalbn(Mq[lane * K + j], -ex) : 0.0;
        vr[j] = j == lane ? 1.0 : 0.0;
      }
    for (int sweep = 0; any && sweep < MAL_SWEEPS; sweep++) {
      double top = 0.0;
      for (uint32_t j = 0; j < K; j++) {
        const double v = mine ? ar[j] : 0.0;
        top = fmax(top, mal_wave_sum(v * v));
      }
      const double floor2 = (MAL_FLOOR * MAL_FLOOR) * top;
      bool rotated = false;
      for (uint32_t p = 0; p + 1 < K; p++)
        for (uint32_t r = p + 1; r < K; r++) {
          const double xp = mine ? ar[p] : 0.0, yr = mine ? ar[r] : 0.0;
          const double a = mal_wave_sum(xp * xp), b = mal_wave_sum(yr * yr), g = mal_wave_sum(xp * yr);
          if (!(a > floor2) || !(b > floor2) || !(fabs(g) > MAL_EPS * sqrt(a * b))) continue;  // (the wave alike)
          const double zeta = (b - a) / (2.0 * g), t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
          const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
          if (mine) {
            const double vx = vr[p], vy = vr[r];
            ar[p] = c * xp - s * yr;
            ar[r] = s * xp + c * yr;
            vr[p] = c * vx - s * vy;
            vr[r] = s * vx + c * vy;
          }
          rotated = true;
        }
      if (!rotated) break;
    }
    // U: the columns above the floor normalised (A holds U from here on); `done` has a bit per finished column
    double top = 0.0;
    for (uint32_t j = 0; j < K; j++) {
      const double v = mine ? ar[j] : 0.0;
      top = fmax(top, sqrt(mal_wave_sum(v * v)));
    }
    uint32_t done = 0;
    for (uint32_t j = 0; j < K; j++) {
      const double v = mine ? ar[j] : 0.0, nrm = sqrt(mal_wave_sum(v * v));
      if (nrm > MAL_FLOOR * top) {
        done |= 1u << j;
        if (mine) ar[j] = v / nrm;
      }
    }
    // ... the others from e_0, e_1, .. in order, twice against the finished columns: the first that keeps enough of itself
    const double keep = 0.5 / sqrt((double)K);
    uint32_t next = 0;
    for (uint32_t j = 0; j < K; j++) {
      if (done >> j & 1) continue;
      for (; next < K; next++) {
        double w = lane == next ? 1.0 : 0.0;
        for (int pass = 0; pass < 2; pass++)
          for (uint32_t u = 0; u < K; u++) {
            if (!(done >> u & 1)) continue;
            const double au = mine ? ar[u] : 0.0, dot = mal_wave_sum(au * w);
            w -= dot * au;
          }
        const double s = sqrt(mal_wave_sum(w * w));
        if (s > keep) {
          if (mine) ar[j] = w / s;
          break;
        }
      }
      done |= 1u << j;
      next++;
    }
  }
  __syncthreads();
  double q = 0.0;
  if (tid < K * K) {  // Q[a][b] = SUM_j U[a][j] V[b][j]
    const uint32_t a = tid / K, b = tid % K;
    for (uint32_t j = 0; j < K; j++) q += A[a * MAL_LD + j] * V[b * MAL_LD + j];
    Mq[tid] = q;
  }
  __syncthreads();

  // ---- Y = X_r Q in place; fit ----
  double f = 0.0;
  for (uint32_t i = tid; i < n; i += MAL_THREADS) {
    double xi[MAL_K];
#pragma unroll
    for (uint32_t a = 0; a < MAL_K; a++) xi[a] = a < K ? x[(uint64_t)a * n + i] : 0.0;
    for (uint32_t b = 0; b < K; b++) {
      double s = 0.0;
#pragma unroll
      for (uint32_t a = 0; a < MAL_K; a++)
        if (a < K) s += xi[a] * Mq[a * K + b];
      x[(uint64_t)b * n + i] = s;
      const double d = s - x0[(uint64_t)b * n + i];
      f += d * d;
    }
  }
  f = mal_wave_sum(f);
  if (!lane) slots[wave] = f;
  __syncthreads();
  if (!tid) {
    double s = 0.0;
    for (uint32_t w = 0; w < MAL_WAVES; w++) s += slots[w];
    d_fit[m] = s;
  }
}

int ngd_launch_mds_coords(hipStream_t st, const double *d_eig, const double *d_vec, const uint32_t *d_status, uint64_t n_mat,
                          uint32_t n_ind, uint32_t K, double *d_cells, uint32_t *d_status_out) {
  if (!n_mat) return (int)hipSuccess;
  if (n_ind < 3 || !K || K > NGD_MDS_MAX_DIM || K > n_ind - 1 || n_mat >= (1ull << 31)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_mds_coords, dim3((uint32_t)n_mat), dim3(MAL_THREADS), 0, st, d_eig, d_vec, d_status, n_ind, K, d_cells, d_status_out);
  return (int)hipGetLastError();
}

int ngd_launch_mds_align(hipStream_t st, double *d_cells, uint64_t stride, const uint32_t *d_status, uint64_t n_set, uint32_t n_mat,
                         uint32_t n_ind, uint32_t K, double *d_fit) {
  if (!n_set || !n_mat) return (int)hipSuccess;
  if (n_ind < 3 || !K || K > NGD_MDS_MAX_DIM || K > n_ind - 1 || stride < (uint64_t)K * n_ind || n_set * n_mat >= (1ull << 31))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_mds_align, dim3((uint32_t)(n_set * n_mat)), dim3(MAL_THREADS), 0, st, d_cells, stride, d_status, n_mat, n_ind, K, d_fit);
  return (int)hipGetLastError();
}
