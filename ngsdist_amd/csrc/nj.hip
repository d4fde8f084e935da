// nj.hip -- a neighbour-joining tree per distance matrix on the device (include/ngsdist_amd.h "Neighbour-joining trees" is
// the contract: canonical neighbour joining, every operation a per-element formula, the joined pair the smallest in the total
// order on (Q, a, b) -- so a tree's bits are a function of its matrix alone).
//
// One workgroup per matrix, matrices on grid.x; no workgroup talks to another, no atomics.  The working matrix is the full
// symmetric n x n of doubles in device scratch, rows padded to an even length (8 MB at n = 1000: beyond LDS), the row sums r[] and the node id of every
// slot live in LDS.  The live nodes are kept a dense prefix of the slots: a join puts the new node u into the lower of the
// pair's two slots and moves the last live slot into the higher one, so the scan shrinks with m and its reads stay
// coalesced.  The contract does not depend on that: Q(a,b) subtracts the row sum of the lower node id first wherever the two
// nodes stand.
// Phase one fills the matrix from the pairs -- the cells as they are (VALUES), or finished from (sum, cnt) by group_cell as
// k_boot_stats does -- and checks that every cell is finite; a matrix with one that is not has no tree (status 0).  The row
// sums follow, one thread per row in ascending column order.  Then, per join, separated by __syncthreads():
//   scan     a wave per row of the live upper triangle, lanes along the row (coalesced); every lane keeps its best key
//   argmin   wave shuffles, then the waves through LDS; lane 0 of wave 0 publishes the pair, d_ij, r_i, r_j and the ids
//   update   one thread per other live slot k: d_uk, r_k, row and column u, and the move of the last slot
// The scratch a wave reads was written by other waves of its workgroup: it is read through a plain pointer (no
// const __restrict__, nothing non-temporal), behind the barrier that follows the writes.
#include "ngd_internal.h"

#define NJ_EMPTY 0xFFFFFFFFu  // no candidate yet (node ids stay below 2^16: NGD_NJ_MAX_IND)
#define NJ_MAX_WAVES 16u

// (q, ab) beats (qo, abo) in the total order on (Q, a, b), ab = a << 16 | b; any candidate beats none.  (A NaN q -- cells so
// large that Q overflows -- never wins a comparison: the pair returned is then some live pair, not a pinned one.)
// (no branch: the scan's loads must stay back to back, a branch per element makes the compiler wait for each)
__device__ inline bool nj_better(double q, uint32_t ab, double qo, uint32_t abo) {
  return (ab != NJ_EMPTY) & ((abo == NJ_EMPTY) | (q < qo) | ((q == qo) & (ab < abo)));
}

__device__ inline void nj_wave_min(double &q, uint32_t &ab, uint32_t &st) {
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    const double oq = __shfl_xor(q, off);
    const uint32_t oab = __shfl_xor(ab, off), ost = __shfl_xor(st, off);
    const bool take = nj_better(oq, oab, q, ab);
    q = take ? oq : q;
    ab = take ? oab : ab;
    st = take ? ost : st;
  }
}

#define NJ_LOADS 8  // 16-byte loads a lane has in flight in the scan: a row of 1024 slots is one batch of a wave

template <bool VALUES>
__global__ __launch_bounds__(NGD_NJ_THREADS) void k_nj(const double *__restrict__ d_a, const unsigned long long *__restrict__ d_cnt,
                                                       uint32_t n, uint64_t tot_sites, uint32_t model, double *d_work,
                                                       int32_t *__restrict__ d_child, double *__restrict__ d_len,
                                                       uint32_t *__restrict__ d_status) {
  // r[ld] | the waves' q[16] | d_ij, r_i, r_j, - | id[ld] | the waves' ab[16], st[16] | si, sj, id_i, id_j   (16-byte aligned:
  // the scan reads r and id two slots at a time)
  extern __shared__ double2 nj_lds[];
  const uint32_t tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, n_waves = nt >> 6;
  const uint32_t ld = ngd_nj_ld(n);  // a row of the working matrix: n rounded up to even, so that every row starts 16-byte aligned
  double *r = (double *)nj_lds, *wq = r + ld, *bc = wq + NJ_MAX_WAVES;
  uint32_t *id = (uint32_t *)(bc + 4), *wab = id + ld, *wst = wab + NJ_MAX_WAVES, *win = wst + NJ_MAX_WAVES;
  const uint64_t n_pairs = (uint64_t)n * (n - 1) / 2, nb = 2 * (uint64_t)n - 3;
  double *D = d_work + (uint64_t)blockIdx.x * n * ld;
  const double *a_ = d_a + (uint64_t)blockIdx.x * n_pairs;
  const unsigned long long *cnt = d_cnt ? d_cnt + (uint64_t)blockIdx.x * n_pairs : nullptr;  // (not read when tot_sites > 0, nor by VALUES)
  int32_t *child = d_child + (uint64_t)blockIdx.x * nb;
  double *len = d_len + (uint64_t)blockIdx.x * nb;
  const double tot = (double)tot_sites;

  // ---- phase one: the pairs of row a lie side by side (ngd_pair_index); both triangles are written ----
  int bad = 0;
  for (uint32_t a = wave; a + 1 < n; a += n_waves) {
    const uint64_t p0 = (uint64_t)a * n - (uint64_t)a * (a + 1) / 2;  // pair (a, a + 1)
    for (uint32_t b = a + 1 + lane; b < n; b += 64) {
      const uint64_t p = p0 + (b - a - 1);
      const double v = VALUES ? a_[p] : group_cell(a_[p], tot_sites ? tot : (double)cnt[p], model);
      if (!isfinite(v)) bad = 1;
      D[(uint64_t)a * ld + b] = v;
      D[(uint64_t)b * ld + a] = v;
    }
  }
  for (uint32_t a = tid; a < n; a += nt) {
    D[(uint64_t)a * ld + a] = 0.0;
    id[a] = a;
  }
  bad = __syncthreads_or(bad);
  if (bad) {  // (the whole workgroup alike)
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    for (uint32_t k = tid; k < nb; k += nt) {
      child[k] = -1;
      len[k] = nan;
    }
    if (!tid) d_status[blockIdx.x] = 0;
    return;
  }
  // ---- row sums: ascending b from 0.0; thread a walks column a (the matrix is symmetric bit for bit): coalesced ----
  for (uint32_t a = tid; a < n; a += nt) {
    double acc = 0.0;
    for (uint32_t b = 0; b < n; b++)
      if (b != a) acc += D[(uint64_t)b * ld + a];
    r[a] = acc;
  }
  __syncthreads();

  uint32_t m = n;
  for (uint32_t t = 0; m > 3; t++, m--) {
    // ---- scan: Q of every live pair, the best key of every lane ----
    const double mm2 = (double)(m - 2);
    double bq = 0.0;
    uint32_t bab = NJ_EMPTY, bst = 0;
    for (uint32_t s = wave; s + 1 < m; s += n_waves) {
      const double rs = r[s];
      const uint32_t ids = id[s];
      const double *row = D + (uint64_t)s * ld;
      // Two columns per lane and load (16 bytes, aligned: c is even), NJ_LOADS loads issued back to back before the first
      // is used: a CU's one workgroup keeps the memory system busy by the bytes it has in flight.  No
      // load is conditional -- a column past the live slots is clamped to the last live pair of columns and its candidates
      // masked -- and no candidate costs a branch.  The first column of a row's first pair may be s itself, the last pair's
      // second column m or the row's padding: masked too
      const uint32_t c_last = (m - 1) & ~1u;
      for (uint32_t c0 = ((s + 1) & ~1u) + 2 * lane; c0 < m; c0 += NJ_LOADS * 128) {
        double2 d2[NJ_LOADS];
#pragma unroll
        for (int u = 0; u < NJ_LOADS; u++) d2[u] = *(const double2 *)(row + min(c0 + u * 128, c_last));
#pragma unroll
        for (int u = 0; u < NJ_LOADS; u++) {
          const uint32_t c = c0 + u * 128, cc = min(c, c_last);
          const double2 r2 = *(const double2 *)(r + cc);
          const uint2 i2 = *(const uint2 *)(id + cc);
#define NJ_CONSIDER(ok, d, rc, idc, col)                                                                     \
          {                                                                                                   \
            const bool lo = ids < (idc); /* the lower node id's row sum is subtracted first */                \
            const double q = (mm2 * (d) - (lo ? rs : (rc))) - (lo ? (rc) : rs);                               \
            const uint32_t ab = lo ? (ids << 16 | (idc)) : ((idc) << 16 | ids);                               \
            const bool take = (ok) & nj_better(q, ab, bq, bab);                                               \
            bq = take ? q : bq;                                                                               \
            bab = take ? ab : bab;                                                                            \
            bst = take ? (s << 16 | (col)) : bst;                                                             \
          }
          NJ_CONSIDER((c > s) & (c < m), d2[u].x, r2.x, i2.x, c)
          NJ_CONSIDER(c + 1 < m, d2[u].y, r2.y, i2.y, c + 1)
#undef NJ_CONSIDER
        }
      }
    }
    // ---- argmin: the key is a total order, so any reduction tree gives the same pair ----
    nj_wave_min(bq, bab, bst);
    if (!lane) { wq[wave] = bq; wab[wave] = bab; wst[wave] = bst; }
    __syncthreads();
    if (!wave) {
      if (lane < n_waves) { bq = wq[lane]; bab = wab[lane]; bst = wst[lane]; }
      else bab = NJ_EMPTY;
      nj_wave_min(bq, bab, bst);
      if (!lane) {
        const uint32_t s = bst >> 16, c = bst & 0xFFFFu, ida = bab >> 16;
        const bool s_is_i = id[s] == ida;  // i: the lower node id
        const uint32_t si = s_is_i ? s : c, sj = s_is_i ? c : s;
        win[0] = si; win[1] = sj; win[2] = id[si]; win[3] = id[sj];
        bc[0] = D[(uint64_t)s * ld + c]; bc[1] = r[si]; bc[2] = r[sj];
      }
    }
    __syncthreads();
    // ---- update: u takes the lower slot of the pair, the last live slot L moves into the higher one ----
    const uint32_t si = win[0], sj = win[1], su = min(si, sj), sr = max(si, sj), L = m - 1;
    const double dij = bc[0], ri = bc[1], rj = bc[2];
    double *rowi = D + (uint64_t)si * ld, *rowj = D + (uint64_t)sj * ld, *rowu = D + (uint64_t)su * ld, *rowr = D + (uint64_t)sr * ld;
    const double *rowL = D + (uint64_t)L * ld;
    for (uint32_t k = tid; k < m; k += nt) {
      if (k == si || k == sj) continue;
      const double dik = rowi[k], djk = rowj[k];
      const double duk = 0.5 * ((dik + djk) - dij);
      const double rk = ((r[k] - dik) - djk) + duk;
      rowu[k] = duk;
      D[(uint64_t)k * ld + su] = duk;
      if (k == L) {  // (L != sr here) the moving slot's own entries: its row sum, its id, its distance to u
        r[sr] = rk;
        id[sr] = id[L];
        rowr[su] = duk;
        rowu[sr] = duk;
      } else {
        r[k] = rk;
        if (sr != L) {
          const double v = rowL[k];
          rowr[k] = v;
          D[(uint64_t)k * ld + sr] = v;
        }
      }
    }
    if (!tid) {
      const double li = 0.5 * dij + (ri - rj) / (2.0 * mm2);
      child[2 * t] = (int32_t)win[2];
      child[2 * t + 1] = (int32_t)win[3];
      len[2 * t] = li;
      len[2 * t + 1] = dij - li;
      r[su] = 0.5 * ((ri + rj) - (double)m * dij);
      id[su] = n + t;
    }
    __syncthreads();
  }
  // ---- m = 3: the three branches to the centre, a < b < c by node id ----
  if (!tid) {
    uint32_t s0 = 0, s1 = 1, s2 = 2, x;
    if (id[s0] > id[s1]) { x = s0; s0 = s1; s1 = x; }
    if (id[s1] > id[s2]) { x = s1; s1 = s2; s2 = x; }
    if (id[s0] > id[s1]) { x = s0; s0 = s1; s1 = x; }
    const double dab = D[(uint64_t)s0 * ld + s1], dac = D[(uint64_t)s0 * ld + s2], dbc = D[(uint64_t)s1 * ld + s2];
    child[nb - 3] = (int32_t)id[s0];
    child[nb - 2] = (int32_t)id[s1];
    child[nb - 1] = (int32_t)id[s2];
    len[nb - 3] = 0.5 * ((dab + dac) - dbc);
    len[nb - 2] = 0.5 * ((dab + dbc) - dac);
    len[nb - 1] = 0.5 * ((dac + dbc) - dab);
    d_status[blockIdx.x] = 1;
  }
}

int ngd_launch_nj(hipStream_t st, const double *d_a, const unsigned long long *d_cnt, bool values, uint64_t n_mat, uint32_t n_ind,
                  uint64_t tot_sites, uint32_t model, uint32_t threads, double *d_work, int32_t *d_child, double *d_len,
                  uint32_t *d_status) {
  if (!n_mat) return (int)hipSuccess;
  if (n_ind < 3 || n_ind > NGD_NJ_MAX_IND || n_mat >= (1ull << 31) || (threads != 256 && threads != 512 && threads != 1024))
    return (int)hipErrorInvalidValue;
  const uint32_t ld = ngd_nj_ld(n_ind), lds = 8 * (ld + NJ_MAX_WAVES + 4) + 4 * (ld + 2 * NJ_MAX_WAVES + 4);
  if (values)
    hipLaunchKernelGGL((k_nj<true>), dim3((uint32_t)n_mat), dim3(threads), lds, st, d_a, d_cnt, n_ind, tot_sites, model, d_work, d_child,
                       d_len, d_status);
  else
    hipLaunchKernelGGL((k_nj<false>), dim3((uint32_t)n_mat), dim3(threads), lds, st, d_a, d_cnt, n_ind, tot_sites, model, d_work, d_child,
                       d_len, d_status);
  return (int)hipGetLastError();
}
