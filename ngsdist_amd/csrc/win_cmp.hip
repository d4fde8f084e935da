// win_cmp.hip -- comparison of the windows of a genome scan (include/ngsdist_amd.h "Comparison of windows"): W vectors of P
// cells each (a window's matrix 0, finished by group_cell; or doubles as they are), their means and the centred Gram matrix
//     gram[a][b] = SUM_c (x_ac - mean[a]) (x_bc - mean[b]),
// one symmetric rank-P update Z Z^T on the FP64 matrix pipe.
//   k_wincmp_stats   one workgroup per vector: finiteness through the workgroup's `or`, the sum by the project's fixed tree
//                    (a lane's own cells in order, the shuffle butterfly, the waves' slots in order) -> status, mean
//   k_wincmp_pack    x - mean (zeros for a status-0 vector) into the resident operand Z, in the fragment-major layout of
//                    ngd_internal.h ("individual" = vector, k = cell): both MFMA operands are single 512-byte fragment
//                    loads from the same array.  The host zeroes Z once up front, so the padding (vectors up to the next
//                    tile block, cells up to the next k-group, the run-ahead k-group) holds zeros
//   k_wincmp_gram    a wavefront owns T x T tiles of 16 x 16 vector pairs over one slice of the cell axis and writes its
//                    partial to scratch; only tile blocks on or above the diagonal exist.  Operand pipeline: contract_mfma.hip's
//   k_wincmp_sum     a cell's partials added in ascending slice order, the upper triangle mirrored into the lower, NaN rows
//                    and columns written from status
// A tile's accumulator sees the slice's k-groups in ascending order whatever the tile block it falls into, and the cut of
// the cell axis is a function of (W, P) alone (ngd_win_cmp_slice, win_cmp_geom.h): gram[a][b] is a function of the cells of a and b and of
// (W, P), never of the other vectors, of where a and b stand, or of the device.  No atomics.
#include <algorithm>

#include "ngd_internal.h"
#include "win_cmp_geom.h"

namespace {

constexpr uint32_t kThreads = 256;

// the sum of a workgroup's values by the fixed tree; every thread gets it
__device__ __forceinline__ double wg_sum(double v, double *slots) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);
  if (!lane) slots[wave] = v;
  __syncthreads();
  double s = slots[0];
  for (uint32_t w = 1; w < kThreads / 64; w++) s += slots[w];
  return s;
}

template <bool VALUES>
__device__ __forceinline__ double cell_of(const double *__restrict__ a, const unsigned long long *__restrict__ cnt, uint64_t at, double tot,
                                          uint32_t model) {
  if (VALUES) return a[at];
  return group_cell(a[at], tot != 0.0 ? tot : (double)cnt[at], model);
}

// vector v of the launch is vector w0 + v of the call
template <bool VALUES>
__global__ __launch_bounds__(kThreads) void k_wincmp_stats(const double *__restrict__ d_a, const unsigned long long *__restrict__ d_cnt,
                                                           uint64_t n_cells, uint64_t tot_sites, uint32_t model, uint64_t w0,
                                                           double *__restrict__ d_mean, uint32_t *__restrict__ d_status) {
  __shared__ double slots[kThreads / 64];
  const uint64_t base = (uint64_t)blockIdx.x * n_cells;
  const double tot = (double)tot_sites;
  int bad = 0;
  double s = 0.0;
  for (uint64_t c = threadIdx.x; c < n_cells; c += kThreads) {
    const double x = cell_of<VALUES>(d_a, d_cnt, base + c, tot, model);
    if (!isfinite(x)) bad = 1;
    s += x;
  }
  bad = __syncthreads_or(bad);
  s = wg_sum(s, slots);
  if (!threadIdx.x) {
    d_status[w0 + blockIdx.x] = bad ? 0u : 1u;
    d_mean[w0 + blockIdx.x] = bad ? __longlong_as_double(0x7FF8000000000000ll) : s / (double)n_cells;
  }
}

// thread = (vector v = blockIdx.y * 16 + (tid & 15), k-group kg = blockIdx.x * 16 + (tid >> 4)): the k-group's four cells
// of the vector, 16 vectors of a k-group side by side (128 contiguous bytes of Z where they share a fragment)
template <bool VALUES>
__global__ __launch_bounds__(kThreads) void k_wincmp_pack(const double *__restrict__ d_a, const unsigned long long *__restrict__ d_cnt,
                                                          uint64_t n_vec, uint64_t n_cells, uint64_t tot_sites, uint32_t model,
                                                          uint64_t w0, const double *__restrict__ d_mean,
                                                          const uint32_t *__restrict__ d_status, uint32_t n_gz, double *__restrict__ Z) {
  const uint64_t v = (uint64_t)blockIdx.y * 16 + (threadIdx.x & 15), kg = (uint64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  if (v >= n_vec || kg * 4 >= n_cells) return;
  const uint64_t w = w0 + v, base = v * n_cells;
  const bool ok = d_status[w] != 0;
  const double mean = ok ? d_mean[w] : 0.0, tot = (double)tot_sites;
  double *z = Z + (kg * n_gz + (w >> 4)) * 64 + (w & 15);
#pragma unroll
  for (uint32_t q = 0; q < 4; q++) {
    const uint64_t c = kg * 4 + q;
    z[q * 16] = ok && c < n_cells ? cell_of<VALUES>(d_a, d_cnt, base + c, tot, model) - mean : 0.0;
  }
}

// one operand fragment: 512 B for the wavefront, lane l takes bytes [8l, 8l+8) at base + OFF (contract_mfma.hip)
template <int OFF>
__device__ __forceinline__ void load_frag(double &dst, uint32_t lane_off, const double *base) {
  asm volatile("global_load_dwordx2 %0, %1, %2 offset:%3" : "=&v"(dst) : "v"(lane_off), "s"(base), "n"(OFF));
}
template <int N, int I = 0>
struct frag_loader {
  static __device__ __forceinline__ void go(double *dst, uint32_t lane_off, const double *base) {
    load_frag<512 * I>(dst[I], lane_off, base);
    if constexpr (I + 1 < N) frag_loader<N, I + 1>::go(dst, lane_off, base);
  }
};

// Wavefront j = blockIdx.x * 4 + wave: tile block j % n_blk (row-major over the upper triangle of the n_br x n_br blocks of
// T x T tiles), slice j / n_blk = k-groups [slice * kg_per_slice, ...) below n_kg.  Its T x T accumulators go to
// part[(slice * n_gz * n_gz + gi * n_gz + gj) * 256 + v * 64 + lane] as the registers are: row 4 v + (lane >> 4) of the
// tile, column lane & 15.  Wavefronts of a workgroup share their slice's operands through the caches.
template <int T>
__global__ __launch_bounds__(256, 3) void k_wincmp_gram(const double *__restrict__ Z, uint32_t n_gz, uint32_t n_br, uint32_t n_blk,
                                                        uint64_t n_jobs, uint64_t n_kg, uint64_t kg_per_slice, double *__restrict__ part) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const uint64_t job = (uint64_t)blockIdx.x * 4 + wave;
  if (job >= n_jobs) return;
  const uint64_t slice = job / n_blk;
  uint32_t t = (uint32_t)(job % n_blk), bi = 0;
  while (t >= n_br - bi) {
    t -= n_br - bi;
    bi++;
  }
  const uint32_t gi0 = bi * T, gj0 = (bi + t) * T;
  const uint64_t kg0 = slice * kg_per_slice, kg1 = kg0 + kg_per_slice < n_kg ? kg0 + kg_per_slice : n_kg;
  const uint32_t lane_off = lane * 8;

  ngd_d4 acc[T][T];
#pragma unroll
  for (int m = 0; m < T; m++)
#pragma unroll
    for (int n = 0; n < T; n++) acc[m][n] = (ngd_d4){0.0, 0.0, 0.0, 0.0};

  const uint64_t step = (uint64_t)n_gz * 64;  // doubles per k-group
  const double *pa = Z + kg0 * step + (uint64_t)gi0 * 64;
  const double *pb = Z + kg0 * step + (uint64_t)gj0 * 64;
  double a[T], b[T];
  frag_loader<T>::go(a, lane_off, pa);
  frag_loader<T>::go(b, lane_off, pb);
  for (uint64_t kg = kg0; kg < kg1; kg++) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int m = 0; m < T; m++) asm volatile("" : "+v"(a[m]));  // pins the MFMAs behind the wait
#pragma unroll
    for (int n = 0; n < T; n++) asm volatile("" : "+v"(b[n]));
#pragma unroll
    for (int m = 0; m < T; m++)
#pragma unroll
      for (int n = 0; n < T; n++) acc[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[m], b[n], acc[m][n], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);  // the refill stays BEHIND the MFMAs that read the registers
    pa += step;
    pb += step;
    frag_loader<T>::go(a, lane_off, pa);  // (the last trip fetches the next slice's first k-group, or Z's tail: never consumed)
    frag_loader<T>::go(b, lane_off, pb);
    __builtin_amdgcn_sched_barrier(0);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // drain the run-ahead: the registers are free again
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int m = 0; m < T; m++)
#pragma unroll
    for (int n = 0; n < T; n++) {
      double *d = part + ((slice * n_gz + (gi0 + m)) * n_gz + (gj0 + n)) * 256 + lane;
#pragma unroll
      for (int v = 0; v < 4; v++) d[v * 64] = acc[m][n][v];
    }
}

// thread = cell (a, b) of gram, a = blockIdx.y * 16 + threadIdx.y, b = blockIdx.x * 16 + threadIdx.x
__global__ __launch_bounds__(256) void k_wincmp_sum(const double *__restrict__ part, uint32_t n_gz, uint64_t n_slices, uint64_t n_vec,
                                                    const uint32_t *__restrict__ d_status, double *__restrict__ gram) {
  const uint64_t a = (uint64_t)blockIdx.y * 16 + threadIdx.y, b = (uint64_t)blockIdx.x * 16 + threadIdx.x;
  if (a >= n_vec || b >= n_vec) return;
  if (!d_status[a] || !d_status[b]) {
    gram[a * n_vec + b] = __longlong_as_double(0x7FF8000000000000ll);
    return;
  }
  const uint64_t r = a < b ? a : b, c = a < b ? b : a;
  const uint64_t tile = (r >> 4) * n_gz + (c >> 4), plane = (uint64_t)n_gz * n_gz;
  const uint32_t at = (uint32_t)(((r & 15) >> 2) * 64 + ((r & 3) << 4) + (c & 15));
  const double *p = part + tile * 256 + at;
  double s = p[0];
  for (uint64_t sl = 1; sl < n_slices; sl++) s += p[sl * plane * 256];
  gram[a * n_vec + b] = s;
}

}  // namespace

uint64_t ngd_wincmp_z_doubles(uint64_t n_vec, uint64_t n_cells) {
  return ((n_cells + 3) / 4 + 1) * ngd_wincmp_groups(n_vec) * 64;  // + the run-ahead k-group
}

uint64_t ngd_wincmp_part_doubles(uint64_t n_vec, uint64_t n_cells) {
  const uint64_t s = ngd_win_cmp_slice(n_vec, n_cells), n_gz = ngd_wincmp_groups(n_vec);
  return (n_cells + s - 1) / s * n_gz * n_gz * 256;
}

int ngd_launch_wincmp_stats(hipStream_t st, const double *d_a, const unsigned long long *d_cnt, bool values, uint64_t n_vec,
                            uint64_t n_cells, uint64_t tot_sites, uint32_t model, uint64_t w0, double *d_mean, uint32_t *d_status) {
  if (!n_vec) return (int)hipSuccess;
  if (!n_cells || n_vec > NGD_WIN_CMP_MAX_VEC) return (int)hipErrorInvalidValue;
  if (values)
    hipLaunchKernelGGL((k_wincmp_stats<true>), dim3((uint32_t)n_vec), dim3(kThreads), 0, st, d_a, d_cnt, n_cells, tot_sites, model, w0,
                       d_mean, d_status);
  else
    hipLaunchKernelGGL((k_wincmp_stats<false>), dim3((uint32_t)n_vec), dim3(kThreads), 0, st, d_a, d_cnt, n_cells, tot_sites, model, w0,
                       d_mean, d_status);
  return (int)hipGetLastError();
}

int ngd_launch_wincmp_pack(hipStream_t st, const double *d_a, const unsigned long long *d_cnt, bool values, uint64_t n_vec,
                           uint64_t n_cells, uint64_t tot_sites, uint32_t model, uint64_t w0, uint64_t n_vec_call, const double *d_mean,
                           const uint32_t *d_status, double *Z) {
  if (!n_vec) return (int)hipSuccess;
  const uint64_t gx = ((n_cells + 3) / 4 + 15) / 16;
  if (!n_cells || w0 + n_vec > n_vec_call || n_vec_call > NGD_WIN_CMP_MAX_VEC || gx >= (1ull << 31)) return (int)hipErrorInvalidValue;
  const dim3 grid((uint32_t)gx, (uint32_t)((n_vec + 15) / 16));
  const uint32_t n_gz = ngd_wincmp_groups(n_vec_call);
  if (values)
    hipLaunchKernelGGL((k_wincmp_pack<true>), grid, dim3(kThreads), 0, st, d_a, d_cnt, n_vec, n_cells, tot_sites, model, w0, d_mean,
                       d_status, n_gz, Z);
  else
    hipLaunchKernelGGL((k_wincmp_pack<false>), grid, dim3(kThreads), 0, st, d_a, d_cnt, n_vec, n_cells, tot_sites, model, w0, d_mean,
                       d_status, n_gz, Z);
  return (int)hipGetLastError();
}

int ngd_launch_wincmp_gram(hipStream_t st, const double *Z, uint64_t n_vec, uint64_t n_cells, double *part) {
  const uint64_t s = ngd_win_cmp_slice(n_vec, n_cells);
  if (!s) return (int)hipErrorInvalidValue;
  const uint32_t T = ngd_wincmp_tile_edge(n_vec), n_gz = ngd_wincmp_groups(n_vec), n_br = n_gz / T, n_blk = n_br * (n_br + 1) / 2;
  const uint64_t n_slices = (n_cells + s - 1) / s, n_jobs = n_slices * n_blk, n_wg = (n_jobs + 3) / 4, n_kg = (n_cells + 3) / 4;
  if (n_wg >= (1ull << 31)) return (int)hipErrorInvalidValue;
#define NGD_WG(TT) \
  hipLaunchKernelGGL((k_wincmp_gram<TT>), dim3((uint32_t)n_wg), dim3(256), 0, st, Z, n_gz, n_br, n_blk, n_jobs, n_kg, s / 4, part)
  switch (T) {
    case 1: NGD_WG(1); break;
    case 2: NGD_WG(2); break;
    case 3: NGD_WG(3); break;
    default: NGD_WG(4); break;
  }
#undef NGD_WG
  return (int)hipGetLastError();
}

int ngd_launch_wincmp_sum(hipStream_t st, const double *part, uint64_t n_vec, uint64_t n_cells, const uint32_t *d_status, double *gram) {
  const uint64_t s = ngd_win_cmp_slice(n_vec, n_cells);
  if (!s) return (int)hipErrorInvalidValue;
  const uint32_t g = (uint32_t)((n_vec + 15) / 16);
  hipLaunchKernelGGL(k_wincmp_sum, dim3(g, g), dim3(16, 16), 0, st, part, ngd_wincmp_groups(n_vec), (n_cells + s - 1) / s, n_vec, d_status,
                     gram);
  return (int)hipGetLastError();
}
