// group_reduce.hip -- group-mean distance matrices on the device: the tail of gen_dist() (ngsDist.cpp:372-401) on every cell
// of [n_mat][n_pairs] sums and counts, and per matrix the mean of the finite cells of every pair of groups (a, b), a <= b.
//
// Work items (ngd_group_work, built by ngd_set_groups from the group sizes alone): group pair (a, b) is the rectangle of
// its rows -- the members of a -- by its columns -- the members of b --, cut into splits of whole rows of about
// NGD_GROUP_WG_CELLS cells.  On the diagonal (a == b) the rectangle is the group by itself and only the cells whose column
// lies behind their row exist.  One workgroup per (matrix, work item): thread t takes the rectangle's cells t, t + 256, ...
// in row-major order -- consecutive threads consecutive columns, so contiguous groups read contiguous memory --, adds the
// finite ones in that order and counts them; the 256 partial results go through a fixed tree (wave shuffles, then LDS in
// wave order) into one (sum, count) per work item, and k_group_finish adds a group pair's splits in ascending order.  No
// atomics anywhere: the order of additions is a function of (n_ind, group_of) alone, whatever else a launch holds.
// Per cell: 8 bytes read (the sum), 16 without --tot_sites (+ the count).
#include "ngd_internal.h"

#define NGD_GROUP_THREADS 256

// (a cell's value: group_cell, ngd_internal.h)

__global__ __launch_bounds__(NGD_GROUP_THREADS) void k_group_means(const double *__restrict__ d_sum,
                                                                   const unsigned long long *__restrict__ d_cnt,
                                                                   uint64_t n_ind, uint64_t n_pairs, const uint32_t *__restrict__ members,
                                                                   const uint32_t *__restrict__ goff,
                                                                   const ngd_group_work *__restrict__ work, uint32_t n_work,
                                                                   uint64_t tot_sites, uint32_t model, double *__restrict__ part_sum,
                                                                   unsigned long long *__restrict__ part_cnt) {
  const uint64_t item = blockIdx.x;  // (matrix of this launch, work item), flattened: a launch may hold more matrices than grid.y
  const uint64_t m = item / n_work;
  const ngd_group_work w = work[item % n_work];
  const uint32_t *rows = members + goff[w.a], *cols = members + goff[w.b];
  const uint32_t n_cols = goff[w.b + 1] - goff[w.b];
  const uint32_t n_cells = (w.r1 - w.r0) * n_cols;  // (< 2^32: ngd_set_groups)
  const bool diag = w.a == w.b;
  const double *sum = d_sum + m * n_pairs;
  const unsigned long long *cnt = d_cnt + m * n_pairs;
  const double tot = (double)tot_sites;
  double acc = 0;
  unsigned long long used = 0;
  for (uint32_t c = threadIdx.x; c < n_cells; c += NGD_GROUP_THREADS) {
    const uint32_t r = w.r0 + c / n_cols, k = c % n_cols;
    if (diag && k <= r) continue;
    const uint32_t i = rows[r], j = cols[k];
    const uint64_t p = ngd_pair_idx(n_ind, i < j ? i : j, i < j ? j : i);
    const double d = group_cell(sum[p], tot_sites ? tot : (double)cnt[p], model);
    if (isfinite(d)) { acc += d; used++; }
  }
  // the fixed tree: lanes 32, 16, ... 1 of a wave, then the waves in order
  for (int off = 32; off > 0; off >>= 1) {
    acc += __shfl_down(acc, off, 64);
    used += __shfl_down(used, off, 64);
  }
  __shared__ double s_acc[NGD_GROUP_THREADS / 64];
  __shared__ unsigned long long s_used[NGD_GROUP_THREADS / 64];
  if ((threadIdx.x & 63) == 0) { s_acc[threadIdx.x >> 6] = acc; s_used[threadIdx.x >> 6] = used; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < NGD_GROUP_THREADS / 64; k++) { acc += s_acc[k]; used += s_used[k]; }
    part_sum[item] = acc;
    part_cnt[item] = used;
  }
}

// one thread per (matrix, group pair): its splits in ascending order; no finite cell -- no work item among them -- is a
// positive quiet NaN
__global__ __launch_bounds__(NGD_GROUP_THREADS) void k_group_finish(const double *__restrict__ part_sum,
                                                                    const unsigned long long *__restrict__ part_cnt,
                                                                    const uint32_t *__restrict__ gp_first, uint32_t n_gp, uint32_t n_work,
                                                                    uint64_t n_out, double *__restrict__ mean,
                                                                    unsigned long long *__restrict__ used) {
  const uint64_t o = (uint64_t)blockIdx.x * NGD_GROUP_THREADS + threadIdx.x;
  if (o >= n_out) return;
  const uint64_t m = o / n_gp;
  const uint32_t gp = (uint32_t)(o % n_gp);
  double acc = 0;
  unsigned long long n = 0;
  for (uint32_t k = gp_first[gp]; k < gp_first[gp + 1]; k++) {
    acc += part_sum[m * n_work + k];
    n += part_cnt[m * n_work + k];
  }
  mean[o] = n ? acc / (double)n : __longlong_as_double(0x7FF8000000000000ll);
  used[o] = n;
}

void ngd_launch_group_means(hipStream_t st, const ngd_group_launch &l, const double *d_sum, const unsigned long long *d_cnt,
                            uint64_t n_mat, uint64_t tot_sites, uint32_t model, double *part_sum, unsigned long long *part_cnt,
                            double *mean, unsigned long long *used) {
  if (l.n_work)
    hipLaunchKernelGGL(k_group_means, dim3((uint32_t)(n_mat * l.n_work)), dim3(NGD_GROUP_THREADS), 0, st, d_sum, d_cnt, l.n_ind,
                       l.n_ind * (l.n_ind - 1) / 2, l.members, l.goff, l.work, l.n_work, tot_sites, model, part_sum, part_cnt);
  const uint64_t n_out = n_mat * l.n_gp;
  hipLaunchKernelGGL(k_group_finish, dim3((uint32_t)((n_out + NGD_GROUP_THREADS - 1) / NGD_GROUP_THREADS)), dim3(NGD_GROUP_THREADS), 0,
                     st, part_sum, part_cnt, l.gp_first, l.n_gp, l.n_work, n_out, mean, used);
}
