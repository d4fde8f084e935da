// boot_stats.hip -- bootstrap summaries per cell on the device: the tail of gen_dist() (ngsDist.cpp:372-401) on every cell of
// a set's n_mat = R + 1 matrices and, per cell, the estimate (matrix 0), the number of finite replicates, their mean, their
// standard deviation and two order statistics (include/ngsdist_amd.h "Bootstrap summaries" is the contract).
//
// One thread per cell of a set.  A workgroup of C threads owns C consecutive cells of one set and an LDS tile [n_mat][C] of
// doubles: thread t loads its cell of every matrix into column t -- consecutive lanes consecutive cells, so every global
// read is coalesced (8 B sum + 8 B count, or 8 B value) -- and from then on works in its own column only: no barrier, no
// atomics, no cross-lane traffic.  Element r of column t lies at (r * C + t) * 8 bytes: r * C * 8 is a multiple of the
// 256-byte bank row for C = 64 and 32, so lanes that stand at different rows -- the heap's data-dependent indices -- still
// hit the banks of their lane number, conflict-free (C = 16: a quarter wave, two rows' lanes at most share a bank).
// Per column: est = row 0; mean and sd by two passes over rows 1 .. R in ascending order; the finite replicates compacted
// to rows 0 .. m - 1; a max-heap over them sheds its m - 1 - k_hi largest, which leaves s_(k_hi) at the root; a min-heap
// over the k_hi + 1 that remain sheds its k_lo smallest, which leaves s_(k_lo) at the root.  Comparisons of finite doubles
// only: exact, and a function of the column's values alone -- not of the tile width, the launch or the chunk.
// C is the widest of 64, 32, 16 whose tile fits the 160 KiB a workgroup may have on gfx950; n_mat * 16 * 8 bytes beyond it
// is refused by the engine (ngd_boot_stats_max_rep).  HBM traffic: 16 (8) bytes read per (cell, matrix), 48 written per cell.
#include "ngd_internal.h"

// v sinks from position i of the heap col[0 .. n) (MAX: the largest at the root, else the smallest)
template <int C, bool MAX>
__device__ inline void boot_sift(double *col, uint32_t i, uint32_t n) {
  const double v = col[i * C];
  for (;;) {
    uint32_t ch = 2 * i + 1;
    if (ch >= n) break;
    double cv = col[ch * C];
    if (ch + 1 < n) {
      const double c2 = col[(ch + 1) * C];
      if (MAX ? c2 > cv : c2 < cv) { ch++; cv = c2; }
    }
    if (!(MAX ? cv > v : cv < v)) break;
    col[i * C] = cv;
    i = ch;
  }
  col[i * C] = v;
}

template <int C, bool MAX>
__device__ inline void boot_heapify(double *col, uint32_t n) {
  for (uint32_t i = n / 2; i-- > 0;) boot_sift<C, MAX>(col, i, n);
}

// the root leaves the heap col[0 .. n): n - 1 elements remain
template <int C, bool MAX>
__device__ inline void boot_pop(double *col, uint32_t n) {
  col[0] = col[(n - 1) * C];
  boot_sift<C, MAX>(col, 0, n - 1);
}

template <int C, bool VALUES>
__global__ __launch_bounds__(C) void k_boot_stats(const double *__restrict__ d_a, const unsigned long long *__restrict__ d_cnt,
                                                  uint32_t n_mat, uint64_t n_cells, uint32_t tiles_per_set, uint64_t tot_sites,
                                                  uint32_t model, double p_lo, double p_hi, double *__restrict__ d_stats,
                                                  unsigned long long *__restrict__ d_used) {
  extern __shared__ double boot_tile[];  // [n_mat][C]
  const uint64_t set = blockIdx.x / tiles_per_set;  // (set, tile) flattened: a launch may hold more sets than grid.y
  const uint64_t cell = (uint64_t)(blockIdx.x % tiles_per_set) * C + threadIdx.x;
  if (cell >= n_cells) return;  // (no barrier below: a thread reads what it wrote itself)
  double *col = boot_tile + threadIdx.x;
  const double *a = d_a + set * n_mat * n_cells + cell;
  const unsigned long long *cnt = d_cnt + set * n_mat * n_cells + cell;
  const double tot = (double)tot_sites;
  // (16 rows' loads in flight per thread: with three waves to a CU at R = 100 -- the tile is 52 KB of the CU's 160 --
  // fewer leave the memory system idle)
#pragma unroll 16
  for (uint32_t r = 0; r < n_mat; r++) {
    const uint64_t at = (uint64_t)r * n_cells;
    col[r * C] = VALUES ? a[at] : group_cell(a[at], tot_sites ? tot : (double)cnt[at], model);
  }
  const double nan = __longlong_as_double(0x7FF8000000000000ll);
  const double est = col[0];
  // the finite replicates in ascending r: their sum from 0.0, then the squared deviations from their mean
  uint32_t m = 0;
  double acc = 0.0;
  for (uint32_t r = 1; r < n_mat; r++) {
    const double v = col[r * C];
    if (isfinite(v)) { acc += v; m++; }
  }
  const double mean = m ? acc / (double)m : nan;
  double ss = 0.0;
  uint32_t k = 0;
  for (uint32_t r = 1; r < n_mat; r++) {
    const double v = col[r * C];
    if (!isfinite(v)) continue;
    const double d = v - mean;
    ss += d * d;
    col[k++ * C] = v;  // (k < r: behind the reads)
  }
  const double sd = m >= 2 ? sqrt(ss / (double)(m - 1)) : nan;
  double lo = nan, hi = nan;
  if (m) {
    const uint32_t last = m - 1;
    uint32_t k_lo = (uint32_t)floor(p_lo * (double)last), k_hi = (uint32_t)ceil(p_hi * (double)last);
    if (k_hi > last) k_hi = last;  // (p_hi < 1: never; the heap's bounds do not hang on it)
    if (k_lo > k_hi) k_lo = k_hi;
    boot_heapify<C, true>(col, m);
    for (uint32_t n = m; n > k_hi + 1; n--) boot_pop<C, true>(col, n);
    hi = col[0];
    if (k_lo == k_hi) {
      lo = hi;
    } else {
      boot_heapify<C, false>(col, k_hi + 1);
      for (uint32_t n = k_hi + 1; n > k_hi + 1 - k_lo; n--) boot_pop<C, false>(col, n);
      lo = col[0];
    }
  }
  double *out = d_stats + set * NGD_BOOT_NSTAT * n_cells + cell;
  out[0] = est;
  out[n_cells] = mean;
  out[2 * n_cells] = sd;
  out[3 * n_cells] = lo;
  out[4 * n_cells] = hi;
  d_used[set * n_cells + cell] = m;
}

template <int C, bool VALUES>
static int boot_launch(hipStream_t st, const double *d_a, const unsigned long long *d_cnt, uint64_t n_set, uint32_t n_mat,
                       uint64_t n_cells, uint64_t tot_sites, uint32_t model, double p_lo, double p_hi, double *d_stats,
                       unsigned long long *d_used) {
  const uint32_t lds = n_mat * C * 8, tiles = (uint32_t)((n_cells + C - 1) / C);
  // (dynamic LDS above 64 KB is the kernel's to ask for)
  hipError_t rc = hipFuncSetAttribute((const void *)k_boot_stats<C, VALUES>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (rc != hipSuccess) return (int)rc;
  hipLaunchKernelGGL((k_boot_stats<C, VALUES>), dim3((uint32_t)(n_set * tiles)), dim3(C), lds, st, d_a, d_cnt, n_mat, n_cells, tiles,
                     tot_sites, model, p_lo, p_hi, d_stats, d_used);
  return (int)hipGetLastError();
}

int ngd_launch_boot_stats(hipStream_t st, const double *d_a, const unsigned long long *d_cnt, bool values, uint64_t n_set,
                          uint32_t n_mat, uint64_t n_cells, uint64_t tot_sites, uint32_t model, double p_lo, double p_hi,
                          double *d_stats, unsigned long long *d_used) {
  if (!n_set || !n_cells) return (int)hipSuccess;
#define NGD_BOOT_ARM(C)                                                                                                   \
  return values ? boot_launch<C, true>(st, d_a, d_cnt, n_set, n_mat, n_cells, tot_sites, model, p_lo, p_hi, d_stats, d_used) \
                : boot_launch<C, false>(st, d_a, d_cnt, n_set, n_mat, n_cells, tot_sites, model, p_lo, p_hi, d_stats, d_used)
  switch (ngd_boot_tile(n_mat)) {
    case 64: NGD_BOOT_ARM(64);
    case 32: NGD_BOOT_ARM(32);
    case 16: NGD_BOOT_ARM(16);
  }
#undef NGD_BOOT_ARM
  return (int)hipErrorInvalidValue;  // (n_mat beyond NGD_BOOT_MAX_MAT)
}
