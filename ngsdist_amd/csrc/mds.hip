// mds.hip -- classical MDS (principal coordinates) of every distance matrix on the device (include/ngsdist_amd.h "Classical
// MDS" is the contract: the top K eigenpairs of the double-centred matrix B and the two sums of its eigenvalues, by a direct
// method, so that accuracy does not hang on the gaps between eigenvalues).
//
// One workgroup per matrix, matrices on grid.x; no workgroup talks to another, no atomics, every sum a fixed tree of the
// workgroup's shape -- so a matrix's bits are a function of its cells and K alone.  The working matrix S is the full
// symmetric n x n of doubles in device scratch, rows padded to an even length as nj.hip's (8 MB at n = 1000: beyond LDS);
// the tridiagonal matrix (d, e), the current reflector v and the vector w of the rank-2 update live in LDS, 32 bytes a row.
//   fill        both triangles of A = -0.5 d^2 from the pairs (the cells as they are, or finished by group_cell); a cell
//               that is not finite ends the matrix (status 0).  Column means, one thread per column; centred in place
//   tridiagonal n - 2 Householder steps on the trailing block, each: the reflector of row k -- the workgroup's maximum of
//               the row's tail first: a tail no larger than eps^2 max|B| is left alone (H = I), any other is scaled by a
//               power of two to a largest magnitude in [1, 2) before its norm is taken by the workgroup's tree (LAPACK
//               dlarfg's remedy: no square leaves the normal range, whatever the scale of the cells, so tau = 2 / v^T v
//               to rounding and H is orthogonal) -- it stays in row k, tau on the diagonal --, p = tau S v with a wave per
//               row and lanes along it, w = p - (tau/2)(p.v) v, then S -= v w^T + w v^T on both triangles (so that every
//               row stays contiguous)
//   eigenvalues all n of T, scaled by a power of two into [1, 2), by bisection on Sturm counts, one thread per eigenvalue
//   vectors     the top K of T by inverse iteration: a lane per vector solves (T - shift)x = x by LU with partial pivoting
//               (its factors in device scratch), wave 0 then orthonormalises the vectors in order; three rounds
//   back        the reflectors in reverse, a wave per vector; normalised, the sign fixed, written out
// Scratch a wave reads was written by other waves of its workgroup: plain pointers, behind the barrier after the writes.
// Where a wave works alone on a vector (orthonormalisation, back-transform) lane l owns the components l, l + 64, ..: no
// lane reads what another wrote.
#include "ngd_internal.h"

#define MDS_MAX_WAVES 16u
#define MDS_LOADS 8  // 16-byte loads a lane has in flight along a row (nj.hip's scan: unconditional, back to back)
#define MDS_ITER 3   // solves per vector
#define MDS_EPS 2.220446049250313e-16
#define MDS_PIVMIN 1e-290

__device__ inline double mds_wave_sum(double x) {
#pragma unroll
  for (int off = 32; off; off >>= 1) x += __shfl_xor(x, off);
  return x;
}
__device__ inline double mds_wave_max(double x) {
#pragma unroll
  for (int off = 32; off; off >>= 1) x = fmax(x, __shfl_xor(x, off));
  return x;
}
// the workgroup's sum: lanes by the butterfly, the waves in order.  Two sets of slots take turns (`slots` alternates
// between calls), so that a wave may start the next sum while another still reads this one's
__device__ inline double mds_wg_sum(double x, double *slots, uint32_t lane, uint32_t wave, uint32_t n_waves) {
  x = mds_wave_sum(x);
  if (!lane) slots[wave] = x;
  __syncthreads();
  double s = 0.0;
  for (uint32_t w = 0; w < n_waves; w++) s += slots[w];
  return s;
}
__device__ inline double mds_wg_max(double x, double *slots, uint32_t lane, uint32_t wave, uint32_t n_waves) {
  x = mds_wave_max(x);
  if (!lane) slots[wave] = x;
  __syncthreads();
  double s = 0.0;
  for (uint32_t w = 0; w < n_waves; w++) s = fmax(s, slots[w]);
  return s;
}

// the start vector of inverse iteration: a fixed function of (component, vector), uniform in (-1, 1), never 0
__device__ inline double mds_start(uint32_t i, uint32_t k) {
  uint32_t h = (i + 1) * 2654435761u ^ (k + 1) * 2246822519u;
  h ^= h >> 15; h *= 2246822519u; h ^= h >> 13; h *= 3266489917u; h ^= h >> 16;
  return ((double)(h >> 8) + 0.5) * (1.0 / 8388608.0) - 1.0;
}

__device__ inline double mds_piv(double x) { return fabs(x) < MDS_EPS ? (signbit(x) ? -MDS_EPS : MDS_EPS) : x; }

// z <- (T - sh I)^-1 z by one lane: LU with partial pivoting, the forward substitution beside it, pivots below the floor
// raised to it; d, e in LDS, the rows of U and z in device scratch
__device__ inline void mds_solve(const double *d, const double *e, uint32_t n, double sh, double *u0, double *u1, double *u2, double *z) {
  double a = d[0] - sh, b = e[0], x = z[0];
  for (uint32_t i = 0; i + 1 < n; i++) {
    const double sub = e[i], dn = d[i + 1] - sh, un = i + 2 < n ? e[i + 1] : 0.0, zn = z[i + 1];
    if (fabs(a) >= fabs(sub)) {
      const double l = a != 0.0 ? sub / a : 0.0;
      u0[i] = a; u1[i] = b; u2[i] = 0.0;
      z[i] = x;
      a = dn - l * b; b = un; x = zn - l * x;
    } else {
      const double l = a / sub;
      u0[i] = sub; u1[i] = dn; u2[i] = un;
      z[i] = zn;
      a = b - l * dn; b = -(l * un); x = x - l * zn;
    }
  }
  double z2 = x / mds_piv(a);
  z[n - 1] = z2;
  double z1 = (z[n - 2] - u1[n - 2] * z2) / mds_piv(u0[n - 2]);
  z[n - 2] = z1;
  for (uint32_t i = n - 2; i-- > 0;) {
    const double zi = ((z[i] - u1[i] * z1) - u2[i] * z2) / mds_piv(u0[i]);
    z[i] = zi;
    z2 = z1;
    z1 = zi;
  }
}

template <bool VALUES>
__global__ __launch_bounds__(NGD_MDS_THREADS) void k_mds(const double *__restrict__ d_a, const unsigned long long *__restrict__ d_cnt,
                                                         uint32_t n, uint64_t tot_sites, uint32_t model, uint32_t K, double *d_work,
                                                         double *d_aux, double *__restrict__ d_eig, double *__restrict__ d_vec,
                                                         double *__restrict__ d_tot, uint32_t *__restrict__ d_status) {
  // d[ld] | e[ld] | v[ld] | w[ld] | two sets of the waves' slots [2][16]   (16-byte aligned: rows are read two columns at a time)
  extern __shared__ double2 mds_lds[];
  const uint32_t tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, n_waves = nt >> 6;
  const uint32_t ld = ngd_nj_ld(n);
  double *d = (double *)mds_lds, *e = d + ld, *v = e + ld, *w = v + ld, *slot_a = w + ld, *slot_b = slot_a + MDS_MAX_WAVES;
  const uint64_t n_pairs = (uint64_t)n * (n - 1) / 2;
  double *S = d_work + (uint64_t)blockIdx.x * n * ld;
  double *Z = d_aux + (uint64_t)blockIdx.x * NGD_MDS_AUX_ROWS * K * ld, *U0 = Z + (uint64_t)K * ld, *U1 = U0 + (uint64_t)K * ld,
         *U2 = U1 + (uint64_t)K * ld;
  const double *a_ = d_a + (uint64_t)blockIdx.x * n_pairs;
  const unsigned long long *cnt = d_cnt ? d_cnt + (uint64_t)blockIdx.x * n_pairs : nullptr;  // (not read when tot_sites > 0, nor by VALUES)
  double *eig = d_eig + (uint64_t)blockIdx.x * K, *vec = d_vec + (uint64_t)blockIdx.x * K * n, *tot2 = d_tot + (uint64_t)blockIdx.x * 2;
  const double tot = (double)tot_sites;

  // ---- fill: the pairs of row a lie side by side (ngd_pair_index); both triangles of A = -0.5 d^2 ----
  int bad = 0;
  for (uint32_t a = wave; a + 1 < n; a += n_waves) {
    const uint64_t p0 = (uint64_t)a * n - (uint64_t)a * (a + 1) / 2;  // pair (a, a + 1)
    for (uint32_t b = a + 1 + lane; b < n; b += 64) {
      const uint64_t p = p0 + (b - a - 1);
      const double c = VALUES ? a_[p] : group_cell(a_[p], tot_sites ? tot : (double)cnt[p], model);
      if (!isfinite(c)) bad = 1;
      const double x = -0.5 * (c * c);
      S[(uint64_t)a * ld + b] = x;
      S[(uint64_t)b * ld + a] = x;
    }
  }
  for (uint32_t a = tid; a < n; a += nt) {
    S[(uint64_t)a * ld + a] = 0.0;
    if (ld != n) S[(uint64_t)a * ld + n] = 0.0;  // (the padding column is read, times zero)
  }
  for (uint32_t a = tid; a < ld; a += nt) d[a] = e[a] = v[a] = w[a] = 0.0;
  bad = __syncthreads_or(bad);
  if (bad) {  // (the whole workgroup alike)
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    for (uint32_t k = tid; k < K * n; k += nt) vec[k] = nan;
    if (tid < K) eig[tid] = nan;
    if (tid < 2) tot2[tid] = nan;
    if (!tid) d_status[blockIdx.x] = 0;
    return;
  }
  // ---- centre: thread a walks column a in ascending order (the matrix is symmetric bit for bit): coalesced ----
  double part = 0.0;
  for (uint32_t a = tid; a < n; a += nt) {
    double acc = 0.0;
    for (uint32_t b = 0; b < n; b++) acc += S[(uint64_t)b * ld + a];
    acc /= (double)n;
    w[a] = acc;
    part += acc;
  }
  const double grand = mds_wg_sum(part, slot_a, lane, wave, n_waves) / (double)n;  // (its barrier publishes w)
  double bmax = 0.0;
  for (uint32_t a = wave; a < n; a += n_waves) {
    const double wa = w[a];
    for (uint32_t b = lane; b < n; b += 64) {
      const double x = (S[(uint64_t)a * ld + b] - (wa + w[b])) + grand;
      S[(uint64_t)a * ld + b] = x;
      bmax = fmax(bmax, fabs(x));
    }
  }
  // a row tail no larger than eps^2 max|B| counts as eliminated (a perturbation far below the method's own eps max|B|): the
  // residue of a matrix of few distinct rows shrinks by about eps a step, and followed to the end of the normal range its
  // bits would depend on the scale of the cells.  (The maximum's barrier ends the reads of w)
  const double negl = mds_wg_max(bmax, slot_b, lane, wave, n_waves) * (MDS_EPS * MDS_EPS);
  for (uint32_t a = tid; a < n; a += nt) w[a] = 0.0;
  __syncthreads();

  // ---- tridiagonal: step k eliminates row / column k beyond k + 1 ----
  for (uint32_t k = 0; k + 2 < n; k++) {
    double *rowk = S + (uint64_t)k * ld;
    // the reflector: H = I - tau v v^T, v[k + 1] = 1, H x = beta e_1
    double big = 0.0;
    for (uint32_t c = k + 2 + tid; c < n; c += nt) big = fmax(big, fabs(rowk[c]));
    const double alpha = rowk[k + 1], dk = rowk[k];
    big = mds_wg_max(big, slot_b, lane, wave, n_waves);
    if (!(big > negl)) {  // nothing to eliminate (the whole workgroup alike): H = I
      if (!tid) { d[k] = dk; e[k] = alpha; rowk[k] = 0.0; }
      __syncthreads();  // (the next step's maximum takes the same slots)
      continue;
    }
    // the norm from the row scaled by a power of two to a largest magnitude in [1, 2) (exact; LAPACK dlarfg's remedy): the
    // squares of a row near 1e-154 and below would leave the normal range, and tau with them 2 / v^T v
    big = fmax(big, fabs(alpha));
    const int ex = isfinite(big) ? ilogb(big) : 0;
    const double as = scalbn(alpha, -ex);
    double ss = 0.0;
    for (uint32_t c = k + 2 + tid; c < n; c += nt) {
      const double x = scalbn(rowk[c], -ex);
      ss += x * x;
    }
    ss = mds_wg_sum(ss, slot_a, lane, wave, n_waves);
    const double beta = -copysign(sqrt(as * as + ss), as), tau = (beta - as) / beta, sc = 1.0 / (as - beta);
    for (uint32_t c = k + 1 + tid; c < n; c += nt) {
      const double vv = c == k + 1 ? 1.0 : scalbn(rowk[c], -ex) * sc;
      v[c] = vv;
      rowk[c] = vv;
    }
    if (!tid) { d[k] = dk; e[k] = scalbn(beta, ex); rowk[k] = tau; v[k] = 0.0; w[k] = 0.0; }
    __syncthreads();
    // p = tau S v: a wave per row of the trailing block, two columns per lane and load, MDS_LOADS loads issued before the
    // first is used.  No load is conditional: a pair of columns past the row is clamped to its last pair and masked; the
    // column before the block (k, where k + 1 is odd) and the padding column meet v = 0
    const uint32_t c_lo = (k + 1) & ~1u, c_last = ld - 2;
    for (uint32_t r = k + 1 + wave; r < n; r += n_waves) {
      const double *row = S + (uint64_t)r * ld;
      double acc = 0.0;
      for (uint32_t c0 = c_lo + 2 * lane; c0 < ld; c0 += MDS_LOADS * 128) {
        double2 s2[MDS_LOADS];
#pragma unroll
        for (int u = 0; u < MDS_LOADS; u++) s2[u] = *(const double2 *)(row + min(c0 + u * 128, c_last));
#pragma unroll
        for (int u = 0; u < MDS_LOADS; u++) {
          const uint32_t c = c0 + u * 128;
          const double2 v2 = *(const double2 *)(v + min(c, c_last));
          const bool ok = c < ld;
          acc += ok ? s2[u].x * v2.x : 0.0;
          acc += ok ? s2[u].y * v2.y : 0.0;
        }
      }
      acc = mds_wave_sum(acc);
      if (!lane) w[r] = tau * acc;
    }
    __syncthreads();
    // w = p - (tau / 2) (p . v) v
    double pv = 0.0;
    for (uint32_t r = k + 1 + tid; r < n; r += nt) pv += w[r] * v[r];
    const double half = -0.5 * tau * mds_wg_sum(pv, slot_b, lane, wave, n_waves);
    for (uint32_t r = k + 1 + tid; r < n; r += nt) w[r] += half * v[r];
    __syncthreads();
    // S -= v w^T + w v^T (cell (r, c) and cell (c, r) get the same bits)
    for (uint32_t r = k + 1 + wave; r < n; r += n_waves) {
      double *row = S + (uint64_t)r * ld;
      const double vr = v[r], wr = w[r];
      for (uint32_t c0 = c_lo + 2 * lane; c0 < ld; c0 += MDS_LOADS * 128) {
        double2 s2[MDS_LOADS];
#pragma unroll
        for (int u = 0; u < MDS_LOADS; u++) s2[u] = *(const double2 *)(row + min(c0 + u * 128, c_last));
#pragma unroll
        for (int u = 0; u < MDS_LOADS; u++) {
          const uint32_t c = c0 + u * 128, cc = min(c, c_last);
          const double2 v2 = *(const double2 *)(v + cc), w2 = *(const double2 *)(w + cc);
          double2 o;
          o.x = s2[u].x - (vr * w2.x + wr * v2.x);
          o.y = s2[u].y - (vr * w2.y + wr * v2.y);
          if (c < ld) *(double2 *)(row + c) = o;
        }
      }
    }
    __syncthreads();
  }
  if (!tid) {
    d[n - 2] = S[(uint64_t)(n - 2) * ld + (n - 2)];
    e[n - 2] = S[(uint64_t)(n - 2) * ld + (n - 1)];
    d[n - 1] = S[(uint64_t)(n - 1) * ld + (n - 1)];
    e[n - 1] = 0.0;
  }
  __syncthreads();

  // ---- T scaled by a power of two into [1, 2): exact, and the floors are then absolute ----
  double tn = 0.0;
  for (uint32_t i = tid; i < n; i += nt) tn = fmax(tn, fabs(d[i]) + (i ? fabs(e[i - 1]) : 0.0) + fabs(e[i]));
  const double tnorm = mds_wg_max(tn, slot_a, lane, wave, n_waves);
  if (!(tnorm > 0.0) || !isfinite(tnorm)) {  // T = 0: a matrix without variation (or cells beyond the contract); the workgroup alike
    const double z = tnorm > 0.0 ? tnorm - tnorm : 0.0;
    for (uint32_t k = tid; k < K * n; k += nt) vec[k] = k / n == k % n ? 1.0 + z : z;
    if (tid < K) eig[tid] = z;
    if (tid < 2) tot2[tid] = z;
    if (!tid) d_status[blockIdx.x] = 1;
    return;
  }
  const int ex = ilogb(tnorm);
  for (uint32_t i = tid; i < n; i += nt) {
    const double ei = scalbn(e[i], -ex);
    d[i] = scalbn(d[i], -ex);
    e[i] = ei;
    w[i] = ei * ei;
  }
  __syncthreads();
  // ---- eigenvalue j of T in ascending order, into v[j]: the least x with more than j eigenvalues below it ----
  for (uint32_t j = tid; j < n; j += nt) {
    double lo = -2.5, hi = 2.5;
    for (int it = 0; it < 64; it++) {
      const double mid = lo + 0.5 * (hi - lo);
      if (!(mid > lo) || !(mid < hi) || hi - lo < 1e-17) break;
      double q = d[0] - mid;
      if (fabs(q) < MDS_PIVMIN) q = -MDS_PIVMIN;
      uint32_t c = q < 0.0;
      for (uint32_t i = 1; i < n; i++) {
        q = (d[i] - mid) - w[i - 1] / q;
        if (fabs(q) < MDS_PIVMIN) q = -MDS_PIVMIN;
        c += q < 0.0;
      }
      if (c > j) hi = mid;
      else lo = mid;
    }
    v[j] = lo + 0.5 * (hi - lo);
  }
  __syncthreads();
  if (!tid) {  // the sums in ascending rank
    double sum = 0.0, pos = 0.0;
    for (uint32_t j = 0; j < n; j++) {
      const double l = scalbn(v[j], ex);
      sum += l;
      if (l > 0.0) pos += l;
    }
    tot2[0] = sum;
    tot2[1] = pos;
    d_status[blockIdx.x] = 1;
  }
  if (tid < K) eig[tid] = scalbn(v[n - 1 - tid], ex);

  // ---- the top K vectors of T ----
  for (uint32_t i = tid; i < K * n; i += nt) Z[(uint64_t)(i / n) * ld + i % n] = mds_start(i % n, i / n);
  __syncthreads();
  for (int it = 0; it < MDS_ITER; it++) {
    if (!lane)
      for (uint32_t k = wave; k < K; k += n_waves) {
        double sh = v[n - 1];  // a shift closer than `pert` to the one before it moves below it
        const double pert = 20.0 * MDS_EPS;
        for (uint32_t j = 1; j <= k; j++) {
          const double l = v[n - 1 - j];
          sh = sh - l < pert ? sh - pert : l;
        }
        mds_solve(d, e, n, sh, U0 + (uint64_t)k * ld, U1 + (uint64_t)k * ld, U2 + (uint64_t)k * ld, Z + (uint64_t)k * ld);
      }
    __syncthreads();
    if (!wave)
      for (uint32_t k = 0; k < K; k++) {  // in order: scaled by its largest component, twice against the vectors before, normalised
        double *z = Z + (uint64_t)k * ld;
        double big = 0.0;
        for (uint32_t i = lane; i < n; i += 64) big = fmax(big, fabs(z[i]));
        big = mds_wave_max(big);
        if (big > 0.0 && isfinite(big))
          for (uint32_t i = lane; i < n; i += 64) z[i] /= big;
        for (int pass = 0; pass < 2; pass++)
          for (uint32_t j = 0; j < k; j++) {
            const double *y = Z + (uint64_t)j * ld;
            double dot = 0.0;
            for (uint32_t i = lane; i < n; i += 64) dot += z[i] * y[i];
            dot = mds_wave_sum(dot);
            for (uint32_t i = lane; i < n; i += 64) z[i] -= dot * y[i];
          }
        double ss = 0.0;
        for (uint32_t i = lane; i < n; i += 64) ss += z[i] * z[i];
        const double nrm = sqrt(mds_wave_sum(ss));
        if (nrm > 0.0)
          for (uint32_t i = lane; i < n; i += 64) z[i] /= nrm;
      }
    __syncthreads();
  }
  // ---- back through the reflectors, a wave per vector; normalised, the component of largest magnitude positive ----
  for (uint32_t kv = wave; kv < K; kv += n_waves) {
    double *z = Z + (uint64_t)kv * ld;
    for (uint32_t k = n - 2; k-- > 0;) {
      const double *x = S + (uint64_t)k * ld;
      const double tau = x[k];
      if (tau == 0.0) continue;  // (the wave alike)
      const uint32_t c_lo = ((k + 1) & ~63u) + lane;
      double dot = 0.0;
      for (uint32_t c = c_lo; c < n; c += 64)
        if (c > k) dot += x[c] * z[c];
      const double f = tau * mds_wave_sum(dot);
      for (uint32_t c = c_lo; c < n; c += 64)
        if (c > k) z[c] -= f * x[c];
    }
    double ss = 0.0;
    for (uint32_t i = lane; i < n; i += 64) ss += z[i] * z[i];
    const double nrm = sqrt(mds_wave_sum(ss));
    double big = -1.0, top = 0.0;
    uint32_t at = 0xFFFFFFFFu;
    for (uint32_t i = lane; i < n; i += 64) {
      const double zi = nrm > 0.0 ? z[i] / nrm : z[i];
      z[i] = zi;
      if (fabs(zi) > big) { big = fabs(zi); top = zi; at = i; }
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) {  // the largest magnitude, the lowest index on a tie
      const double ob = __shfl_xor(big, off), ot = __shfl_xor(top, off);
      const uint32_t oa = __shfl_xor(at, off);
      const bool take = (ob > big) | ((ob == big) & (oa < at));
      big = take ? ob : big;
      top = take ? ot : top;
      at = take ? oa : at;
    }
    const bool flip = top < 0.0;
    for (uint32_t i = lane; i < n; i += 64) vec[(uint64_t)kv * n + i] = flip ? -z[i] : z[i];
  }
}

int ngd_launch_mds(hipStream_t st, const double *d_a, const unsigned long long *d_cnt, bool values, uint64_t n_mat, uint32_t n_ind,
                   uint64_t tot_sites, uint32_t model, uint32_t K, uint32_t threads, double *d_work, double *d_aux, double *d_eig,
                   double *d_vec, double *d_tot, uint32_t *d_status) {
  if (!n_mat) return (int)hipSuccess;
  if (n_ind < 3 || n_ind > NGD_MDS_MAX_IND || !K || K > NGD_MDS_MAX_DIM || K > n_ind - 1 || n_mat >= (1ull << 31) ||
      (threads != 256 && threads != 512 && threads != 1024))
    return (int)hipErrorInvalidValue;
  const uint32_t ld = ngd_nj_ld(n_ind), lds = 8 * (4 * ld + 2 * MDS_MAX_WAVES);
  if (lds >= 65536) {  // (dynamic LDS beyond 64 KB is the kernel's to ask for: n_ind from 2039 on)
    const hipError_t rc = hipFuncSetAttribute(values ? (const void *)k_mds<true> : (const void *)k_mds<false>,
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (rc != hipSuccess) return (int)rc;
  }
  if (values)
    hipLaunchKernelGGL((k_mds<true>), dim3((uint32_t)n_mat), dim3(threads), lds, st, d_a, d_cnt, n_ind, tot_sites, model, K, d_work, d_aux,
                       d_eig, d_vec, d_tot, d_status);
  else
    hipLaunchKernelGGL((k_mds<false>), dim3((uint32_t)n_mat), dim3(threads), lds, st, d_a, d_cnt, n_ind, tot_sites, model, K, d_work, d_aux,
                       d_eig, d_vec, d_tot, d_status);
  return (int)hipGetLastError();
}
