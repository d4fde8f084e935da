// reduce.hip -- (1) fixed-order reduction of the per-slice slabs into the
// per-pair sums, (2) per-pair valid-site counts for --pairwise_del
// (reference ngsDist.cpp:335-338 + :362: cnt++ only on sites where neither
// individual is missing), from bit masks: cnt = popcount(mask_i & mask_j),
// bootstrap multiplicities entering as bit-planes, (3) bootstrap replicates
// as weighted reductions of per-block partial (sum, cnt), many replicates per
// pass over the partials.
#include <type_traits>

#include "ngd_internal.h"

namespace {

// A block that is NOT drawn (weight 0) must add nothing even when its partial sum is NaN (the EM of an all-zero site,
// 0/0 as on the CPU): 0 x NaN would poison replicates that never visit the site.  A select per (slice, replicate)
// makes this memory-bound kernel VALU-bound ([measured] cfg 5: 0.43 -> 1.31 ms; a branch per slice 0.89 ms), so the main
// loop only NOTES a non-finite partial and a pair that met one is summed again with the undrawn blocks left out.
__device__ __forceinline__ bool ngd_finite(double v) { return __builtin_fabs(v) <= 1.7976931348623157e308; }

// grid = owned 128-tiles x 128 rows; 128 threads = columns.  Eight interleaved partial sums (slice
// ks goes to partial ks % 8) keep eight loads in flight per thread; they are combined in a fixed tree,
// so the result is a fixed function of the slabs (deterministic), just not the left-to-right sum.
// d_cnt != NULL: the pair's count is written too (no --pairwise_del: the same number of sites for every pair,
// ngsDist.cpp:362) -- one launch less per matrix, which a 0.3 ms job notices.
__global__ __launch_bounds__(128) void k_reduce(const double *__restrict__ slab, uint32_t n_ks,
                                                 uint32_t planes_per_slice, const ngd_tile *__restrict__ tiles,
                                                 uint32_t n_pad, uint64_t n_ind, double *__restrict__ d_sum,
                                                 unsigned long long *__restrict__ d_cnt, unsigned long long cnt_value,
                                                 ngd_fix_flags fix, double fix_thr, const long long *__restrict__ unit_E,
                                                 double unit_c, double unit_d0) {
  const uint32_t tile = blockIdx.x >> 7, row = blockIdx.x & 127;
  const uint32_t i = tiles[tile].ti * NGD_TILE + row;
  const uint32_t j = tiles[tile].tj * NGD_TILE + threadIdx.x;
  if (!(i < j && j < n_ind)) return;
  const uint64_t plane = (uint64_t)n_pad * n_pad * planes_per_slice;  // distance between consecutive slices
  const double *p = slab + (uint64_t)i * n_pad + j;
  double s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t ks = 0;
  for (; ks + 8 <= n_ks; ks += 8) {
#pragma unroll
    for (int u = 0; u < 8; u++) s[u] += p[(uint64_t)(ks + u) * plane];
  }
  for (int u = 0; ks < n_ks; ks++, u++) s[u] += p[(uint64_t)ks * plane];
  const uint64_t idx = ngd_pair_idx(n_ind, i, j);
  double sum = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
  // a pass that left the unit-sum coordinate's k-groups out (engine_plans.hip): its products are d_0 (n + E_i + E_j) to
  // within n 2^-106.  The constant first -- it cancels nearly exactly against the slab sum -- so that the correction is
  // rounded at the result's own magnitude (E in units of 2^-53: an exact integer sum, converted once)
  if (unit_E) sum = (unit_c + sum) + unit_d0 * ((double)(unit_E[i] + unit_E[j]) * 0x1p-53);
  d_sum[idx] = sum;
  if (d_cnt) d_cnt[idx] = cnt_value;
  // single_image = 2 engines: a sum this small is not held to 1e-9 relative by the congruent arithmetic -- noted for the
  // fix-up pass (fixup.hip); rare, so one atomic per noted pair
  if (fix.list && sum < fix_thr) {
    const uint32_t slot = atomicAdd(fix.count, 1u);
    if (slot < fix.cap) fix.list[slot] = ((unsigned long long)i << 32) | j;
  }
}

// Bootstrap replicates from per-block partial sums, RB replicates per pass over the slab:
//   sum[r][pair] = SUM_slice W[slice][r] * slab[slice][pair],  slices in ascending order,
// W = multiplicity of the slice's block in replicate r (reference rnd_map_data, ngsDist.cpp:416-437: a
// block drawn m times is visited m times).  W is slice-major (stride w_stride, zero padded to a multiple
// of RB), so the RB weights of a slice are one scalar load; grid.y = replicate chunk.  One order of
// summation for every replicate and every batch size: a replicate's result does not depend on which
// call (single or batched) produced it.
template <int RB>
__global__ __launch_bounds__(128) void k_reduce_wb(const double *__restrict__ slab, uint32_t n_ks,
                                                    const double *__restrict__ W, uint32_t w_stride,
                                                    uint32_t n_rep, const ngd_tile *__restrict__ tiles,
                                                    uint32_t n_pad, uint64_t n_ind, uint64_t n_pairs,
                                                    double *__restrict__ d_sum, ngd_fix_flags fix,
                                                    const double *__restrict__ fix_thr) {
  const uint32_t tile = blockIdx.x >> 7, row = blockIdx.x & 127;
  const uint32_t i = tiles[tile].ti * NGD_TILE + row;
  const uint32_t j = tiles[tile].tj * NGD_TILE + threadIdx.x;
  if (!(i < j && j < n_ind)) return;
  const uint32_t r0 = blockIdx.y * RB;
  const uint64_t plane = (uint64_t)n_pad * n_pad;
  const double *p = slab + (uint64_t)i * n_pad + j;
  const double *w = W + r0;
  double acc[RB];
#pragma unroll
  for (int r = 0; r < RB; r++) acc[r] = 0;
  if (RB == 1) {  // one replicate: about 1/e of the blocks are not drawn at all -> their slices are not read
    for (uint32_t ks = 0; ks < n_ks; ks++) {
      const double wk = w[(uint64_t)ks * w_stride];  // uniform across the workgroup
      if (wk != 0.0) acc[0] = __builtin_fma(wk, p[ks * plane], acc[0]);
    }
  } else {
    constexpr int U = 4;  // slices in flight per thread
    uint32_t ks = 0;
    bool bad = false;  // a non-finite partial among this pair's slices
    for (; ks + U <= n_ks; ks += U) {
      double v[U];
#pragma unroll
      for (int u = 0; u < U; u++) v[u] = p[(uint64_t)(ks + u) * plane];
#pragma unroll
      for (int u = 0; u < U; u++) bad |= !ngd_finite(v[u]);
#pragma unroll
      for (int u = 0; u < U; u++)
#pragma unroll
        for (int r = 0; r < RB; r++) acc[r] = __builtin_fma(w[(uint64_t)(ks + u) * w_stride + r], v[u], acc[r]);
    }
    for (; ks < n_ks; ks++) {
      const double v = p[(uint64_t)ks * plane];
      bad |= !ngd_finite(v);
#pragma unroll
      for (int r = 0; r < RB; r++) acc[r] = __builtin_fma(w[(uint64_t)ks * w_stride + r], v, acc[r]);
    }
    if (__builtin_expect(bad, 0)) {  // again, slices in the same order, blocks that are not drawn left out
#pragma unroll
      for (int r = 0; r < RB; r++) acc[r] = 0;
      for (ks = 0; ks < n_ks; ks++) {
        const double v = p[(uint64_t)ks * plane];
#pragma unroll
        for (int r = 0; r < RB; r++) {
          const double wr = w[(uint64_t)ks * w_stride + r];
          if (wr != 0.0) acc[r] = __builtin_fma(wr, v, acc[r]);
        }
      }
    }
  }
  const uint64_t idx = ngd_pair_idx(n_ind, i, j);
  bool small = false;
#pragma unroll
  for (int r = 0; r < RB; r++)
    if (r0 + r < n_rep) {
      d_sum[(uint64_t)(r0 + r) * n_pairs + idx] = acc[r];
      if (fix.list) small = small || acc[r] < fix_thr[r0 + r];
    }
  // single_image = 2 engines (see k_reduce): noted once, whichever replicate chunk sees a small sum first
  if (small && !((atomicOr(&fix.seen[idx >> 5], 1u << (idx & 31)) >> (idx & 31)) & 1u)) {
    const uint32_t slot = atomicAdd(fix.count, 1u);
    if (slot < fix.cap) fix.list[slot] = ((unsigned long long)i << 32) | j;
  }
}

// single_image = 2 engines under --pairwise_del (ngsDist.cpp:335-338): which pairs want the fix-up pass is decided HERE,
// once a pair's valid-site counts are known, not in the reductions above -- a pair that shares no valid site with its
// partner in a matrix has the sum 0 there, exactly, and must not be noted (a data set with many missing sites would
// otherwise note thousands of empty pairs, pass the engine's limit and have the fix-up pass skipped for the few pairs that need
// it: tools/fuzz_parity.py cases 202651, 202706, 202716, 207606).  The bound of the congruent arithmetic is per VISITED
// site, so the threshold is per pair too: noted if, in any of the n_rep matrices, 0 < cnt and sum < mean x cnt.
__global__ __launch_bounds__(128) void k_fix_flag(const double *__restrict__ d_sum, const unsigned long long *__restrict__ d_cnt,
                                                   uint32_t n_rep, const ngd_tile *__restrict__ tiles, uint64_t n_ind,
                                                   uint64_t n_pairs, double mean, ngd_fix_flags fix) {
  const uint32_t tile = blockIdx.x >> 7, row = blockIdx.x & 127;
  const uint32_t i = tiles[tile].ti * NGD_TILE + row;
  const uint32_t j = tiles[tile].tj * NGD_TILE + threadIdx.x;
  if (!(i < j && j < n_ind)) return;
  const uint64_t idx = ngd_pair_idx(n_ind, i, j);
  bool small = false;
  for (uint32_t r = 0; r < n_rep; r++) {
    const unsigned long long c = d_cnt[(uint64_t)r * n_pairs + idx];
    small = small || (c != 0 && d_sum[(uint64_t)r * n_pairs + idx] < mean * (double)c);
  }
  if (small) {
    const uint32_t slot = atomicAdd(fix.count, 1u);
    if (slot < fix.cap) fix.list[slot] = ((unsigned long long)i << 32) | j;
  }
}

// The fix-up pass by a whole two-operand pass (engine.hip fixup_by_pass): d_new holds every pair's sum in the two-image
// arithmetic; it replaces the one-image sum of exactly the pairs the noting rule picks (sum below mean x the sites visited;
// under --pairwise_del x the pair's own count, never a pair without a valid site) -- all others keep their bits.
__global__ __launch_bounds__(128) void k_fix_merge(const double *__restrict__ d_new, double *__restrict__ d_sum,
                                                    const unsigned long long *__restrict__ d_cnt, double thr, double mean,
                                                    const ngd_tile *__restrict__ tiles, uint64_t n_ind) {
  const uint32_t tile = blockIdx.x >> 7, row = blockIdx.x & 127;
  const uint32_t i = tiles[tile].ti * NGD_TILE + row;
  const uint32_t j = tiles[tile].tj * NGD_TILE + threadIdx.x;
  if (!(i < j && j < n_ind)) return;
  const uint64_t idx = ngd_pair_idx(n_ind, i, j);
  const double old = d_sum[idx];
  bool small;
  if (d_cnt) {
    const unsigned long long c = d_cnt[idx];
    small = c != 0 && old < mean * (double)c;
  } else {
    small = old < thr;
  }
  if (small) d_sum[idx] = d_new[idx];
}

// The same for the valid-site counts of --pairwise_del: cnt[r][pair] = SUM_b M[b][r] * C[b][pair] with
// C = per-block popcounts (k_count_blocks) and M the block multiplicities (uint32, block-major).
template <int RB>
__global__ __launch_bounds__(128) void k_reduce_cb(const uint32_t *__restrict__ C, uint32_t n_blocks,
                                                    const uint32_t *__restrict__ M, uint32_t m_stride,
                                                    uint32_t n_rep, const ngd_tile *__restrict__ tiles,
                                                    uint32_t n_pad, uint64_t n_ind, uint64_t n_pairs,
                                                    unsigned long long *__restrict__ d_cnt) {
  const uint32_t tile = blockIdx.x >> 7, row = blockIdx.x & 127;
  const uint32_t i = tiles[tile].ti * NGD_TILE + row;
  const uint32_t j = tiles[tile].tj * NGD_TILE + threadIdx.x;
  if (!(i < j && j < n_ind)) return;
  const uint32_t r0 = blockIdx.y * RB;
  const uint64_t plane = (uint64_t)n_pad * n_pad;
  const uint32_t *p = C + (uint64_t)i * n_pad + j;
  const uint32_t *m = M + r0;
  unsigned long long acc[RB];
#pragma unroll
  for (int r = 0; r < RB; r++) acc[r] = 0;
  constexpr int U = 4;
  uint32_t b = 0;
  for (; b + U <= n_blocks; b += U) {
    uint32_t v[U];
#pragma unroll
    for (int u = 0; u < U; u++) v[u] = p[(uint64_t)(b + u) * plane];
#pragma unroll
    for (int u = 0; u < U; u++)
#pragma unroll
      for (int r = 0; r < RB; r++) acc[r] += (unsigned long long)m[(uint64_t)(b + u) * m_stride + r] * v[u];
  }
  for (; b < n_blocks; b++) {
    const uint32_t v = p[(uint64_t)b * plane];
#pragma unroll
    for (int r = 0; r < RB; r++) acc[r] += (unsigned long long)m[(uint64_t)b * m_stride + r] * v;
  }
  const uint64_t idx = ngd_pair_idx(n_ind, i, j);
#pragma unroll
  for (int r = 0; r < RB; r++)
    if (r0 + r < n_rep) d_cnt[(uint64_t)(r0 + r) * n_pairs + idx] = acc[r];
}

// grid.y = replicate: cnt[r][pair] = values[r] (no --pairwise_del: every visited site counts, ngsDist.cpp:362)
__global__ __launch_bounds__(128) void k_fill_cnt(const ngd_tile *__restrict__ tiles, uint64_t n_ind,
                                                   unsigned long long value,
                                                   const unsigned long long *__restrict__ values,
                                                   uint64_t n_pairs, unsigned long long *__restrict__ d_cnt) {
  const uint32_t tile = blockIdx.x >> 7, row = blockIdx.x & 127;
  const uint32_t i = tiles[tile].ti * NGD_TILE + row;
  const uint32_t j = tiles[tile].tj * NGD_TILE + threadIdx.x;
  if (!(i < j && j < n_ind)) return;
  d_cnt[(uint64_t)blockIdx.y * n_pairs + ngd_pair_idx(n_ind, i, j)] = values ? values[blockIdx.y] : value;
}

constexpr int CW = 64;  // mask words staged per step

// Workgroup = 32 x 32 pairs of one 128-tile (grid = owned 128-tiles x 16 sub-tiles), thread = 2 x 2 pairs: four
// LDS reads feed four popcounts (the one-pair-per-thread form was LDS-bandwidth bound: two reads per popcount).
// LDS holds CW words of the 32 + 32 individuals (and of the planes).
__global__ __launch_bounds__(256) void k_count(const unsigned long long *__restrict__ mask,
                                                const unsigned long long *__restrict__ planes,
                                                uint32_t n_planes, uint32_t n_words,
                                                const ngd_tile *__restrict__ tiles, uint64_t n_ind,
                                                unsigned long long *__restrict__ d_cnt) {
  __shared__ unsigned long long mi[32][CW + 1], mj[32][CW + 1], pl[32][CW];
  const uint32_t tile = blockIdx.x >> 4, sa = (blockIdx.x >> 2) & 3, sb = blockIdx.x & 3;
  const uint32_t ti = tiles[tile].ti, tj = tiles[tile].tj;
  if (ti == tj && sa > sb) return;  // below the diagonal
  const uint32_t i0 = ti * NGD_TILE + sa * 32, j0 = tj * NGD_TILE + sb * 32;
  if (i0 >= n_ind || j0 >= n_ind) return;
  const uint32_t ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
  unsigned long long cnt[2][2] = {{0, 0}, {0, 0}};
  // grid.y splits the words (sites): integer atomics make the sum independent of the order
  const uint32_t per_y = ((n_words + gridDim.y - 1) / gridDim.y + CW - 1) / CW * CW;
  const uint32_t w_begin = blockIdx.y * per_y, w_end = w_begin + per_y < n_words ? w_begin + per_y : n_words;
  for (uint32_t w0 = w_begin; w0 < w_end; w0 += CW) {
    for (uint32_t t = threadIdx.x; t < 32 * CW; t += 256) {
      const uint32_t r = t / CW, c = t % CW;
      const uint32_t w = w0 + c;
      const uint32_t ii = i0 + r, jj = j0 + r;
      mi[r][c] = (w < n_words && ii < n_ind) ? mask[(uint64_t)ii * n_words + w] : 0ull;
      mj[r][c] = (w < n_words && jj < n_ind) ? mask[(uint64_t)jj * n_words + w] : 0ull;
    }
    for (uint32_t t = threadIdx.x; t < n_planes * CW; t += 256) {
      const uint32_t b = t / CW, c = t % CW;
      const uint32_t w = w0 + c;
      pl[b][c] = w < n_words ? planes[(uint64_t)b * n_words + w] : 0ull;
    }
    __syncthreads();
    if (n_planes == 0) {
      uint32_t q00 = 0, q01 = 0, q10 = 0, q11 = 0;  // at most 64 x CW per chunk: 32 bits are plenty
#pragma unroll 4
      for (int c = 0; c < CW; c++) {
        const unsigned long long a0 = mi[ty][c], a1 = mi[ty + 16][c], b0 = mj[tx][c], b1 = mj[tx + 16][c];
        q00 += __popcll(a0 & b0); q01 += __popcll(a0 & b1);
        q10 += __popcll(a1 & b0); q11 += __popcll(a1 & b1);
      }
      cnt[0][0] += q00; cnt[0][1] += q01; cnt[1][0] += q10; cnt[1][1] += q11;
    } else {
      for (int c = 0; c < CW; c++) {
        const unsigned long long a0 = mi[ty][c], a1 = mi[ty + 16][c], b0 = mj[tx][c], b1 = mj[tx + 16][c];
        const unsigned long long m00 = a0 & b0, m01 = a0 & b1, m10 = a1 & b0, m11 = a1 & b1;
        for (uint32_t b = 0; b < n_planes; b++) {
          const unsigned long long p = pl[b][c];
          cnt[0][0] += (unsigned long long)__popcll(m00 & p) << b; cnt[0][1] += (unsigned long long)__popcll(m01 & p) << b;
          cnt[1][0] += (unsigned long long)__popcll(m10 & p) << b; cnt[1][1] += (unsigned long long)__popcll(m11 & p) << b;
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int a = 0; a < 2; a++)
#pragma unroll
    for (int b = 0; b < 2; b++) {
      const uint32_t i = i0 + ty + 16 * a, j = j0 + tx + 16 * b;
      if (i < j && j < n_ind) atomicAdd(&d_cnt[ngd_pair_idx(n_ind, i, j)], cnt[a][b]);  // d_cnt was zeroed
    }
}

// Per-block valid-site counts C[b][i][j] = popcount(mask_i & mask_j over the sites of block b): the cnt half
// of the per-block partials.  Workgroup = 16x16 pairs; grid.y strides over the blocks.  A block is any
// site range [b*B, (b+1)*B), so its first and last mask words are trimmed.
// seg != NULL (windows along the genome): block b is the segment [seg[b].s_lo, seg[b].s_hi) of the slice table instead.
__global__ __launch_bounds__(256) void k_count_blocks(const unsigned long long *__restrict__ mask,
                                                       uint32_t n_words, uint64_t block_size, uint32_t n_blocks,
                                                       const ngd_tile *__restrict__ tiles, uint32_t n_pad,
                                                       uint64_t n_ind, uint32_t *__restrict__ C,
                                                       const uint64_t *__restrict__ seg) {
  __shared__ unsigned long long mi[16][CW + 1], mj[16][CW + 1];
  const uint32_t ig = tiles[blockIdx.x].ti, jg = tiles[blockIdx.x].tj;
  const uint32_t ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
  const uint32_t i = ig * 16 + ty, j = jg * 16 + tx;
  for (uint32_t b = blockIdx.y; b < n_blocks; b += gridDim.y) {
    const uint64_t s_lo = seg ? seg[(uint64_t)b * NGD_SEG_STRIDE + NGD_SEG_SLO] : (uint64_t)b * block_size;  // sites [s_lo, s_hi)
    const uint64_t s_hi = seg ? seg[(uint64_t)b * NGD_SEG_STRIDE + NGD_SEG_SHI] : s_lo + block_size;
    const uint32_t w_lo = (uint32_t)(s_lo >> 6), w_hi = (uint32_t)((s_hi - 1) >> 6);
    uint32_t cnt = 0;
    for (uint32_t w0 = w_lo; w0 <= w_hi; w0 += CW) {
      for (uint32_t t = threadIdx.x; t < 16 * CW; t += 256) {
        const uint32_t r = t / CW, c = t % CW;
        const uint32_t w = w0 + c;
        unsigned long long keep = 0;
        if (w <= w_hi) {
          keep = ~0ull;
          if (w == w_lo) keep &= ~0ull << (s_lo & 63);
          if (w == w_hi && (s_hi & 63)) keep &= ~0ull >> (64 - (s_hi & 63));
        }
        const uint32_t ii = ig * 16 + r, jj = jg * 16 + r;
        mi[r][c] = (keep && ii < n_ind) ? mask[(uint64_t)ii * n_words + w] & keep : 0ull;
        mj[r][c] = (keep && jj < n_ind) ? mask[(uint64_t)jj * n_words + w] : 0ull;
      }
      __syncthreads();
      const uint32_t left = w_hi - w0 + 1;
      const uint32_t nw = left < (uint32_t)CW ? left : (uint32_t)CW;
      for (uint32_t c = 0; c < nw; c++) cnt += __popcll(mi[ty][c] & mj[tx][c]);
      __syncthreads();
    }
    C[((uint64_t)b * n_pad + i) * n_pad + j] = cnt;
  }
}

// Windows along the genome (engine.hip windows_slab), the banded reduction: k_reduce_wb's tiling and output order, a group
// of RB consecutive windows per grid.y.  The group reads the union of its windows' segments ONCE, in ascending order, and
// adds each to the windows that contain it -- reads scale with the segments, not windows x segments as k_reduce_wb on 0/1
// weights would.  win[2 w] = first segment | end segment << 32 of window w (segments of the batch), win[2 w + 1] = its
// length in sites.  CNT = false: slab of per-segment sums -> d_sum, and (d_cnt != NULL, no --pairwise_del) the window's
// length as every pair's count; single_image = 2 engines note a pair whose sum in any window is below NGD_FIX_MEAN x the
// window's length.  CNT = true: per-segment valid-site counts (k_count_blocks over the segments) -> d_cnt, exactly.
template <int RB, bool CNT>
__global__ __launch_bounds__(128) void k_reduce_band(const void *__restrict__ slab_v, const unsigned long long *__restrict__ win,
                                                      uint32_t n_win, const ngd_tile *__restrict__ tiles, uint32_t n_pad,
                                                      uint64_t n_ind, uint64_t n_pairs, double *__restrict__ d_sum,
                                                      unsigned long long *__restrict__ d_cnt, ngd_fix_flags fix) {
  typedef typename std::conditional<CNT, uint32_t, double>::type T;
  typedef typename std::conditional<CNT, unsigned long long, double>::type A;
  const uint32_t tile = blockIdx.x >> 7, row = blockIdx.x & 127;
  const uint32_t i = tiles[tile].ti * NGD_TILE + row;
  const uint32_t j = tiles[tile].tj * NGD_TILE + threadIdx.x;
  if (!(i < j && j < n_ind)) return;
  const uint32_t w0 = blockIdx.y * RB;
  uint32_t f[RB], l[RB];  // the group's windows as segment ranges (uniform across the workgroup)
  uint32_t a = 0xffffffffu, b = 0;
#pragma unroll
  for (int r = 0; r < RB; r++) {
    const unsigned long long t = w0 + r < n_win ? win[2 * (uint64_t)(w0 + r)] : 0ull;
    f[r] = (uint32_t)t;
    l[r] = (uint32_t)(t >> 32);
    if (f[r] < l[r]) { a = a < f[r] ? a : f[r]; b = b > l[r] ? b : l[r]; }
  }
  const uint64_t plane = (uint64_t)n_pad * n_pad;
  const T *p = reinterpret_cast<const T *>(slab_v) + (uint64_t)i * n_pad + j;
  A acc[RB];
#pragma unroll
  for (int r = 0; r < RB; r++) acc[r] = 0;
  constexpr int U = 4;  // segments in flight per thread
  uint32_t s = a;
  for (; s + U <= b; s += U) {
    T v[U];
#pragma unroll
    for (int u = 0; u < U; u++) v[u] = p[(uint64_t)(s + u) * plane];
#pragma unroll
    for (int u = 0; u < U; u++)
#pragma unroll
      for (int r = 0; r < RB; r++)
        if (s + u >= f[r] && s + u < l[r]) acc[r] += (A)v[u];  // (a select, never 0 x v: nothing outside a window enters it)
  }
  for (; s < b; s++) {
    const T v = p[(uint64_t)s * plane];
#pragma unroll
    for (int r = 0; r < RB; r++)
      if (s >= f[r] && s < l[r]) acc[r] += (A)v;
  }
  const uint64_t idx = ngd_pair_idx(n_ind, i, j);
  bool small = false;
#pragma unroll
  for (int r = 0; r < RB; r++)
    if (w0 + r < n_win) {
      const uint64_t o = (uint64_t)(w0 + r) * n_pairs + idx;
      if (CNT) {
        d_cnt[o] = (unsigned long long)acc[r];
      } else {
        const unsigned long long len = win[2 * (uint64_t)(w0 + r) + 1];
        d_sum[o] = (double)acc[r];
        if (d_cnt) d_cnt[o] = len;
        if (fix.list) small = small || (double)acc[r] < NGD_FIX_MEAN * (double)len;
      }
    }
  if (!CNT && small && !((atomicOr(&fix.seen[idx >> 5], 1u << (idx & 31)) >> (idx & 31)) & 1u)) {
    const uint32_t slot = atomicAdd(fix.count, 1u);
    if (slot < fix.cap) fix.list[slot] = ((unsigned long long)i << 32) | j;
  }
}

// Bootstrap replicates inside windows (engine_windows.hip, the unit slab): the banded AND weighted reduction,
//   sum[w][r][pair] = SUM_b Wt[b][r] * SUM_{s in slices of block b of window w} slab[s][pair],
// k_reduce_wb's tiling, pair order and output order; grid.y = (window of the batch) x (chunk of RB replicates).  A
// workgroup reads its window's slices ONCE per chunk, in ascending order, one fma per slice with the weight of the slice's
// block.  blk[w][0 .. n_blocks] = first slice of each block of window w (blk[w][n_blocks] = the end of its last block: the
// window's tail, which only its full-data matrix visits, is never read here).  Every window of a call draws the same block
// maps, so Wt is [n_blocks][w_stride], zero padded to a multiple of RB: the RB weights of a block are one uniform load.
// A non-finite partial result is treated as in k_reduce_wb: noted in the main loop, and a pair that met one is summed again
// with the blocks a replicate did not draw left out (an all-zero individual on the EM path).
// Matrix r of window w goes to d_out[(w * mat_stride + r) * n_pairs] (the caller has moved d_out past the window's full-data
// matrix).  CNT = false: sums; d_cnt != NULL (no --pairwise_del): cnt_value as every pair's count; single_image = 2 engines
// note a pair whose sum in any matrix is below fix_thr.  CNT = true: per-slice valid-site counts (k_count_blocks) and uint32
// multiplicities -> d_cnt, in integers: exact.
template <int RB, bool CNT>
__global__ __launch_bounds__(128) void k_reduce_band_w(const void *__restrict__ slab_v, const uint32_t *__restrict__ blk,
                                                        uint32_t n_blocks, const void *__restrict__ Wt_v, uint32_t w_stride,
                                                        uint32_t n_rep, uint32_t n_chunks, uint32_t mat_stride,
                                                        const ngd_tile *__restrict__ tiles, uint32_t n_pad, uint64_t n_ind,
                                                        uint64_t n_pairs, double *__restrict__ d_sum,
                                                        unsigned long long *__restrict__ d_cnt, unsigned long long cnt_value,
                                                        ngd_fix_flags fix, double fix_thr) {
  typedef typename std::conditional<CNT, uint32_t, double>::type T;
  typedef typename std::conditional<CNT, unsigned long long, double>::type A;
  const uint32_t tile = blockIdx.x >> 7, row = blockIdx.x & 127;
  const uint32_t i = tiles[tile].ti * NGD_TILE + row;
  const uint32_t j = tiles[tile].tj * NGD_TILE + threadIdx.x;
  if (!(i < j && j < n_ind)) return;
  const uint32_t w = blockIdx.y / n_chunks, r0 = (blockIdx.y % n_chunks) * RB;
  const uint32_t *bf = blk + (uint64_t)w * (n_blocks + 1);  // (uniform across the workgroup, like the weights)
  const T *Wt = reinterpret_cast<const T *>(Wt_v) + r0;
  const uint64_t plane = (uint64_t)n_pad * n_pad;
  const T *p = reinterpret_cast<const T *>(slab_v) + (uint64_t)i * n_pad + j;
  A acc[RB];
#pragma unroll
  for (int r = 0; r < RB; r++) acc[r] = 0;
  const uint32_t s_begin = bf[0], s_end = bf[n_blocks];
  constexpr int U = 4;  // slices in flight per thread
  uint32_t s = s_begin, b = 0, next = n_blocks ? bf[1] : s_end;  // slice s lies in block b, which ends before slice `next`
  bool bad = false;  // a non-finite partial among this pair's slices
  for (; s + U <= s_end; s += U) {
    T v[U];
#pragma unroll
    for (int u = 0; u < U; u++) v[u] = p[(uint64_t)(s + u) * plane];
    if (!CNT) {
#pragma unroll
      for (int u = 0; u < U; u++) bad |= !ngd_finite((double)v[u]);
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      while (s + u >= next) next = bf[++b + 1];
      const T *wb = Wt + (uint64_t)b * w_stride;
#pragma unroll
      for (int r = 0; r < RB; r++) {
        if (CNT) acc[r] += (A)wb[r] * (A)v[u];
        else acc[r] = (A)__builtin_fma((double)wb[r], (double)v[u], (double)acc[r]);
      }
    }
  }
  for (; s < s_end; s++) {
    const T v = p[(uint64_t)s * plane];
    if (!CNT) bad |= !ngd_finite((double)v);
    while (s >= next) next = bf[++b + 1];
    const T *wb = Wt + (uint64_t)b * w_stride;
#pragma unroll
    for (int r = 0; r < RB; r++) {
      if (CNT) acc[r] += (A)wb[r] * (A)v;
      else acc[r] = (A)__builtin_fma((double)wb[r], (double)v, (double)acc[r]);
    }
  }
  if (!CNT && __builtin_expect(bad, 0)) {  // again, slices in the same order, blocks that are not drawn left out
#pragma unroll
    for (int r = 0; r < RB; r++) acc[r] = 0;
    for (b = 0; b < n_blocks; b++) {
      const T *wb = Wt + (uint64_t)b * w_stride;
      for (s = bf[b]; s < bf[b + 1]; s++) {
        const T v = p[(uint64_t)s * plane];
#pragma unroll
        for (int r = 0; r < RB; r++)
          if (wb[r] != 0) acc[r] = (A)__builtin_fma((double)wb[r], (double)v, (double)acc[r]);
      }
    }
  }
  const uint64_t idx = ngd_pair_idx(n_ind, i, j);
  bool small = false;
#pragma unroll
  for (int r = 0; r < RB; r++)
    if (r0 + r < n_rep) {
      const uint64_t o = ((uint64_t)w * mat_stride + r0 + r) * n_pairs + idx;
      if (CNT) {
        d_cnt[o] = (unsigned long long)acc[r];
      } else {
        d_sum[o] = (double)acc[r];
        if (d_cnt) d_cnt[o] = cnt_value;
        if (fix.list) small = small || (double)acc[r] < fix_thr;
      }
    }
  // single_image = 2 engines (see k_reduce): noted once, whichever window, matrix or launch of the batch sees a small sum first
  if (!CNT && small && !((atomicOr(&fix.seen[idx >> 5], 1u << (idx & 31)) >> (idx & 31)) & 1u)) {
    const uint32_t slot = atomicAdd(fix.count, 1u);
    if (slot < fix.cap) fix.list[slot] = ((unsigned long long)i << 32) | j;
  }
}

// k_reduce_band_w's walk for one window whose row of block starts (bf), n_blocks, weight table at replicate r0 (Wt), count
// and threshold arrive as arguments -- all uniform across the workgroup.  It restates that kernel's body statement for
// statement: routing k_reduce_band_w itself through this function changes the code the compiler emits for it (every
// instantiation, 2 % to 19 % in instruction count either way), and the equal-length job keeps the kernel it was measured with.
template <int RB, bool CNT, typename T>
__device__ __forceinline__ void band_w_window(const void *__restrict__ slab_v, uint32_t i, uint32_t j, uint32_t w, uint32_t r0,
                                              const uint32_t *bf, uint32_t n_blocks, const T *Wt,
                                              uint32_t w_stride, uint32_t n_rep, uint32_t mat_stride, uint32_t n_pad,
                                              uint64_t n_ind, uint64_t n_pairs, double *__restrict__ d_sum,
                                              unsigned long long *__restrict__ d_cnt, unsigned long long cnt_value,
                                              ngd_fix_flags fix, double fix_thr) {
  typedef typename std::conditional<CNT, unsigned long long, double>::type A;
  const uint64_t plane = (uint64_t)n_pad * n_pad;
  const T *p = reinterpret_cast<const T *>(slab_v) + (uint64_t)i * n_pad + j;
  A acc[RB];
#pragma unroll
  for (int r = 0; r < RB; r++) acc[r] = 0;
  const uint32_t s_begin = bf[0], s_end = bf[n_blocks];
  constexpr int U = 4;  // slices in flight per thread
  uint32_t s = s_begin, b = 0, next = n_blocks ? bf[1] : s_end;  // slice s lies in block b, which ends before slice `next`
  bool bad = false;  // a non-finite partial among this pair's slices
  for (; s + U <= s_end; s += U) {
    T v[U];
#pragma unroll
    for (int u = 0; u < U; u++) v[u] = p[(uint64_t)(s + u) * plane];
    if (!CNT) {
#pragma unroll
      for (int u = 0; u < U; u++) bad |= !ngd_finite((double)v[u]);
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      while (s + u >= next) next = bf[++b + 1];
      const T *wb = Wt + (uint64_t)b * w_stride;
#pragma unroll
      for (int r = 0; r < RB; r++) {
        if (CNT) acc[r] += (A)wb[r] * (A)v[u];
        else acc[r] = (A)__builtin_fma((double)wb[r], (double)v[u], (double)acc[r]);
      }
    }
  }
  for (; s < s_end; s++) {
    const T v = p[(uint64_t)s * plane];
    if (!CNT) bad |= !ngd_finite((double)v);
    while (s >= next) next = bf[++b + 1];
    const T *wb = Wt + (uint64_t)b * w_stride;
#pragma unroll
    for (int r = 0; r < RB; r++) {
      if (CNT) acc[r] += (A)wb[r] * (A)v;
      else acc[r] = (A)__builtin_fma((double)wb[r], (double)v, (double)acc[r]);
    }
  }
  if (!CNT && __builtin_expect(bad, 0)) {  // again, slices in the same order, blocks that are not drawn left out
#pragma unroll
    for (int r = 0; r < RB; r++) acc[r] = 0;
    for (b = 0; b < n_blocks; b++) {
      const T *wb = Wt + (uint64_t)b * w_stride;
      for (s = bf[b]; s < bf[b + 1]; s++) {
        const T v = p[(uint64_t)s * plane];
#pragma unroll
        for (int r = 0; r < RB; r++)
          if (wb[r] != 0) acc[r] = (A)__builtin_fma((double)wb[r], (double)v, (double)acc[r]);
      }
    }
  }
  const uint64_t idx = ngd_pair_idx(n_ind, i, j);
  bool small = false;
#pragma unroll
  for (int r = 0; r < RB; r++)
    if (r0 + r < n_rep) {
      const uint64_t o = ((uint64_t)w * mat_stride + r0 + r) * n_pairs + idx;
      if (CNT) {
        d_cnt[o] = (unsigned long long)acc[r];
      } else {
        d_sum[o] = (double)acc[r];
        if (d_cnt) d_cnt[o] = cnt_value;
        if (fix.list) small = small || (double)acc[r] < fix_thr;
      }
    }
  // single_image = 2 engines (see k_reduce): noted once, whichever window, matrix or launch of the batch sees a small sum first
  if (!CNT && small && !((atomicOr(&fix.seen[idx >> 5], 1u << (idx & 31)) >> (idx & 31)) & 1u)) {
    const uint32_t slot = atomicAdd(fix.count, 1u);
    if (slot < fix.cap) fix.list[slot] = ((unsigned long long)i << 32) | j;
  }
}

// Windows of UNEQUAL length (ngd_run_windows_job_var*): the same reduction, but what k_reduce_band_w takes once per launch --
// n_blocks, the weight table, the count, the fix-up threshold -- is the window's own.  desc[w] = {where the window's row of
// block starts begins in blk, n_blocks_w, where its weight table [n_blocks_w][w_stride] begins in Wt (elements), the sites a
// replicate visits n_blocks_w q} (win_plan.h NGD_WIN_DESC_*): four words indexed by blockIdx.y alone, so uniform across the
// workgroup -- scalar loads, nothing per lane.  Windows of one class point at one table.  A window with no block reads no
// slice and writes sum 0, count 0.
template <int RB, bool CNT>
__global__ __launch_bounds__(128) void k_reduce_band_wv(const void *__restrict__ slab_v, const uint32_t *__restrict__ blk,
                                                         const uint64_t *__restrict__ desc, const void *__restrict__ Wt_v,
                                                         uint32_t w_stride, uint32_t n_rep, uint32_t n_chunks, uint32_t mat_stride,
                                                         const ngd_tile *__restrict__ tiles, uint32_t n_pad, uint64_t n_ind,
                                                         uint64_t n_pairs, double *__restrict__ d_sum,
                                                         unsigned long long *__restrict__ d_cnt, ngd_fix_flags fix, double fix_mean) {
  typedef typename std::conditional<CNT, uint32_t, double>::type T;
  const uint32_t tile = blockIdx.x >> 7, row = blockIdx.x & 127;
  const uint32_t i = tiles[tile].ti * NGD_TILE + row;
  const uint32_t j = tiles[tile].tj * NGD_TILE + threadIdx.x;
  if (!(i < j && j < n_ind)) return;
  const uint32_t w = blockIdx.y / n_chunks, r0 = (blockIdx.y % n_chunks) * RB;
  const uint64_t *d = desc + (uint64_t)w * NGD_WIN_DESC;
  const uint64_t n_vis = d[NGD_WIN_DESC_VIS];
  band_w_window<RB, CNT, T>(slab_v, i, j, w, r0, blk + d[NGD_WIN_DESC_BLK], (uint32_t)d[NGD_WIN_DESC_NB],
                            reinterpret_cast<const T *>(Wt_v) + d[NGD_WIN_DESC_WT] + r0, w_stride, n_rep, mat_stride, n_pad, n_ind,
                            n_pairs, d_sum, d_cnt, n_vis, fix, fix_mean * (double)n_vis);
}

template <int RB>
void reduce_band_wv(hipStream_t st, const ngd_geom &g, const double *slab, const uint32_t *C, const uint32_t *d_blk,
                    const uint64_t *d_desc, uint32_t n_win, const void *d_Wt, uint32_t w_stride, uint32_t n_rep, uint32_t mat_stride,
                    const ngd_tile *d_tiles, uint32_t n_tiles, double *d_sum, unsigned long long *d_cnt, const ngd_fix_flags &f) {
  const uint64_t n_pairs = g.n_ind * (g.n_ind - 1) / 2;
  const uint32_t n_chunks = (n_rep + RB - 1) / RB, per = 65535u / n_chunks;  // (grid.y holds 65 535)
  for (uint32_t w0 = 0; w0 < n_win; w0 += per) {
    const uint32_t n = n_win - w0 < per ? n_win - w0 : per;
    const dim3 grid(n_tiles * NGD_TILE, n * n_chunks);
    const uint64_t *desc = d_desc + (uint64_t)w0 * NGD_WIN_DESC;  // (its offsets count from the batch's tables)
    const uint64_t off = (uint64_t)w0 * mat_stride * n_pairs;
    if (C)
      hipLaunchKernelGGL((k_reduce_band_wv<RB, true>), grid, dim3(128), 0, st, (const void *)C, d_blk, desc, d_Wt, w_stride, n_rep,
                         n_chunks, mat_stride, d_tiles, g.n_pad, g.n_ind, n_pairs, nullptr, d_cnt + off, f, 0.0);
    else
      hipLaunchKernelGGL((k_reduce_band_wv<RB, false>), grid, dim3(128), 0, st, (const void *)slab, d_blk, desc, d_Wt, w_stride,
                         n_rep, n_chunks, mat_stride, d_tiles, g.n_pad, g.n_ind, n_pairs, d_sum + off,
                         d_cnt ? d_cnt + off : nullptr, f, NGD_FIX_MEAN);
  }
}

template <int RB>
void reduce_band_w(hipStream_t st, const ngd_geom &g, const double *slab, const uint32_t *C, const uint32_t *d_blk,
                   uint32_t n_win, uint32_t n_blocks, const void *d_Wt, uint32_t w_stride, uint32_t n_rep, uint32_t mat_stride,
                   const ngd_tile *d_tiles, uint32_t n_tiles, double *d_sum, unsigned long long *d_cnt,
                   unsigned long long cnt_value, const ngd_fix_flags &f, double fix_thr) {
  const uint64_t n_pairs = g.n_ind * (g.n_ind - 1) / 2;
  const uint32_t n_chunks = (n_rep + RB - 1) / RB, per = 65535u / n_chunks;  // (grid.y holds 65 535)
  for (uint32_t w0 = 0; w0 < n_win; w0 += per) {
    const uint32_t n = n_win - w0 < per ? n_win - w0 : per;
    const dim3 grid(n_tiles * NGD_TILE, n * n_chunks);
    const uint32_t *blk = d_blk + (uint64_t)w0 * (n_blocks + 1);
    const uint64_t off = (uint64_t)w0 * mat_stride * n_pairs;
    if (C)
      hipLaunchKernelGGL((k_reduce_band_w<RB, true>), grid, dim3(128), 0, st, (const void *)C, blk, n_blocks, d_Wt, w_stride,
                         n_rep, n_chunks, mat_stride, d_tiles, g.n_pad, g.n_ind, n_pairs, nullptr, d_cnt + off, 0ull, f, 0.0);
    else
      hipLaunchKernelGGL((k_reduce_band_w<RB, false>), grid, dim3(128), 0, st, (const void *)slab, blk, n_blocks, d_Wt,
                         w_stride, n_rep, n_chunks, mat_stride, d_tiles, g.n_pad, g.n_ind, n_pairs, d_sum + off,
                         d_cnt ? d_cnt + off : nullptr, cnt_value, f, fix_thr);
  }
}

template <int RB>
void reduce_wb(hipStream_t st, const ngd_geom &g, const double *slab, uint32_t n_ks, const double *d_W,
               uint32_t w_stride, uint32_t n_rep, const ngd_tile *d_tiles, uint32_t n_tiles, double *d_sum,
               const ngd_fix_flags &fix, const double *d_thr) {
  hipLaunchKernelGGL((k_reduce_wb<RB>), dim3(n_tiles * NGD_TILE, (n_rep + RB - 1) / RB), dim3(128), 0, st, slab,
                     n_ks, d_W, w_stride, n_rep, d_tiles, g.n_pad, g.n_ind, g.n_ind * (g.n_ind - 1) / 2, d_sum, fix, d_thr);
}

template <int RB>
void reduce_cb(hipStream_t st, const ngd_geom &g, const uint32_t *C, uint32_t n_blocks, const uint32_t *d_M,
               uint32_t m_stride, uint32_t n_rep, const ngd_tile *d_tiles, uint32_t n_tiles,
               unsigned long long *d_cnt) {
  hipLaunchKernelGGL((k_reduce_cb<RB>), dim3(n_tiles * NGD_TILE, (n_rep + RB - 1) / RB), dim3(128), 0, st, C,
                     n_blocks, d_M, m_stride, n_rep, d_tiles, g.n_pad, g.n_ind, g.n_ind * (g.n_ind - 1) / 2, d_cnt);
}

}  // namespace

void ngd_launch_reduce(hipStream_t st, const ngd_geom &g, const double *slab, uint32_t n_ks,
                       uint32_t planes_per_slice, const ngd_tile *d_tiles, uint32_t n_tiles, double *d_sum,
                       unsigned long long *d_cnt, unsigned long long cnt_value, const ngd_fix_flags *fix, double fix_thr,
                       const long long *unit_E, double unit_c, double unit_d0) {
  if (!n_tiles) return;
  hipLaunchKernelGGL(k_reduce, dim3(n_tiles * NGD_TILE), dim3(128), 0, st, slab, n_ks, planes_per_slice, d_tiles,
                     g.n_pad, g.n_ind, d_sum, d_cnt, cnt_value, fix ? *fix : ngd_fix_flags{nullptr, nullptr, nullptr, 0}, fix_thr,
                     unit_E, unit_c, unit_d0);
}

void ngd_launch_fix_flag(hipStream_t st, const ngd_geom &g, const double *d_sum, const unsigned long long *d_cnt,
                         uint32_t n_rep, const ngd_tile *d_tiles, uint32_t n_tiles, const ngd_fix_flags &fix, uint32_t mat_stride) {
  if (!n_tiles || !n_rep) return;
  // (the kernel's distance between two matrices: mat_stride matrices of n_pairs entries)
  hipLaunchKernelGGL(k_fix_flag, dim3(n_tiles * NGD_TILE), dim3(128), 0, st, d_sum, d_cnt, n_rep, d_tiles, g.n_ind,
                     ngd_n_pairs(g.n_ind) * mat_stride, NGD_FIX_MEAN, fix);
}

void ngd_launch_fix_merge(hipStream_t st, const ngd_geom &g, const double *d_new, double *d_sum, const unsigned long long *d_cnt,
                          double thr, const ngd_tile *d_tiles, uint32_t n_tiles) {
  if (!n_tiles) return;
  hipLaunchKernelGGL(k_fix_merge, dim3(n_tiles * NGD_TILE), dim3(128), 0, st, d_new, d_sum, d_cnt, thr, NGD_FIX_MEAN, d_tiles,
                     g.n_ind);
}

// replicates per pass over the partials; the weight arrays are padded to a multiple of it
uint32_t ngd_reduce_chunk(uint32_t n_rep) { return n_rep <= 1 ? 1 : n_rep <= 4 ? 4 : n_rep <= 16 ? 16 : 32; }

void ngd_launch_reduce_w(hipStream_t st, const ngd_geom &g, const double *slab, uint32_t n_ks, const double *d_W,
                         uint32_t w_stride, uint32_t n_rep, const ngd_tile *d_tiles, uint32_t n_tiles,
                         double *d_sum, const ngd_fix_flags *fix, const double *d_thr, uint32_t chunk) {
  if (!n_tiles || !n_rep) return;
  const ngd_fix_flags f = fix && d_thr ? *fix : ngd_fix_flags{nullptr, nullptr, nullptr, 0};
  // chunk: one group of a larger job launched on its own (the caller has offset W, d_sum and d_thr to the group's first
  // replicate) keeps the job's template -- a replicate's bits do not depend on it, its speed does
  switch (chunk ? chunk : ngd_reduce_chunk(n_rep)) {
    case 1: reduce_wb<1>(st, g, slab, n_ks, d_W, w_stride, n_rep, d_tiles, n_tiles, d_sum, f, d_thr); break;
    case 4: reduce_wb<4>(st, g, slab, n_ks, d_W, w_stride, n_rep, d_tiles, n_tiles, d_sum, f, d_thr); break;
    case 16: reduce_wb<16>(st, g, slab, n_ks, d_W, w_stride, n_rep, d_tiles, n_tiles, d_sum, f, d_thr); break;
    default: reduce_wb<32>(st, g, slab, n_ks, d_W, w_stride, n_rep, d_tiles, n_tiles, d_sum, f, d_thr);
  }
}

void ngd_launch_reduce_c(hipStream_t st, const ngd_geom &g, const uint32_t *C, uint32_t n_blocks, const uint32_t *d_M,
                         uint32_t m_stride, uint32_t n_rep, const ngd_tile *d_tiles, uint32_t n_tiles,
                         unsigned long long *d_cnt, uint32_t chunk) {
  if (!n_tiles || !n_rep) return;
  switch (chunk ? chunk : ngd_reduce_chunk(n_rep)) {
    case 1: reduce_cb<1>(st, g, C, n_blocks, d_M, m_stride, n_rep, d_tiles, n_tiles, d_cnt); break;
    case 4: reduce_cb<4>(st, g, C, n_blocks, d_M, m_stride, n_rep, d_tiles, n_tiles, d_cnt); break;
    case 16: reduce_cb<16>(st, g, C, n_blocks, d_M, m_stride, n_rep, d_tiles, n_tiles, d_cnt); break;
    default: reduce_cb<32>(st, g, C, n_blocks, d_M, m_stride, n_rep, d_tiles, n_tiles, d_cnt);
  }
}

void ngd_launch_count_blocks(hipStream_t st, const ngd_geom &g, const unsigned long long *mask, uint64_t block_size,
                             uint32_t n_blocks, const ngd_tile *d_tiles16, uint32_t n_tiles16, uint32_t *C, const uint64_t *d_seg) {
  if (!n_tiles16 || !n_blocks) return;
  hipLaunchKernelGGL(k_count_blocks, dim3(n_tiles16, n_blocks < 1024 ? n_blocks : 1024), dim3(256), 0, st, mask,
                     g.n_words, block_size, n_blocks, d_tiles16, g.n_pad, g.n_ind, C, d_seg);
}

uint32_t ngd_band_windows() { return 16; }

void ngd_launch_reduce_band(hipStream_t st, const ngd_geom &g, const double *slab, const uint32_t *C,
                            const unsigned long long *d_win, uint32_t n_win, const ngd_tile *d_tiles, uint32_t n_tiles,
                            double *d_sum, unsigned long long *d_cnt, const ngd_fix_flags *fix, uint32_t mat_stride) {
  if (!n_tiles || !n_win) return;
  // (window w's matrix at [w * mat_stride][n_pairs]: the kernel's distance between two windows' matrices)
  const uint64_t n_pairs = g.n_ind * (g.n_ind - 1) / 2, w_pairs = n_pairs * mat_stride;
  const ngd_fix_flags f = fix ? *fix : ngd_fix_flags{nullptr, nullptr, nullptr, 0};
  for (uint32_t w0 = 0; w0 < n_win; w0 += 16 * 32768) {  // (grid.y holds 65 535)
    const uint32_t n = n_win - w0 < 16 * 32768 ? n_win - w0 : 16 * 32768;
    const dim3 grid(n_tiles * NGD_TILE, (n + 15) / 16);
    if (C)
      hipLaunchKernelGGL((k_reduce_band<16, true>), grid, dim3(128), 0, st, (const void *)C, d_win + 2 * (uint64_t)w0, n, d_tiles,
                         g.n_pad, g.n_ind, w_pairs, nullptr, d_cnt + (uint64_t)w0 * w_pairs, f);
    else
      hipLaunchKernelGGL((k_reduce_band<16, false>), grid, dim3(128), 0, st, (const void *)slab, d_win + 2 * (uint64_t)w0, n,
                         d_tiles, g.n_pad, g.n_ind, w_pairs, d_sum + (uint64_t)w0 * w_pairs,
                         d_cnt ? d_cnt + (uint64_t)w0 * w_pairs : nullptr, f);
  }
}

void ngd_launch_reduce_band_w(hipStream_t st, const ngd_geom &g, const double *slab, const uint32_t *C, const uint32_t *d_blk,
                              uint32_t n_win, uint32_t n_blocks, const void *d_Wt, uint32_t w_stride, uint32_t n_rep,
                              uint32_t mat_stride, const ngd_tile *d_tiles, uint32_t n_tiles, double *d_sum,
                              unsigned long long *d_cnt, unsigned long long cnt_value, const ngd_fix_flags *fix, double fix_thr) {
  if (!n_tiles || !n_win || !n_rep || !n_blocks) return;
  const ngd_fix_flags f = fix ? *fix : ngd_fix_flags{nullptr, nullptr, nullptr, 0};
  switch (ngd_reduce_chunk(n_rep)) {  // (the weights' stride is a multiple of it)
    case 1: reduce_band_w<1>(st, g, slab, C, d_blk, n_win, n_blocks, d_Wt, w_stride, n_rep, mat_stride, d_tiles, n_tiles, d_sum, d_cnt, cnt_value, f, fix_thr); break;
    case 4: reduce_band_w<4>(st, g, slab, C, d_blk, n_win, n_blocks, d_Wt, w_stride, n_rep, mat_stride, d_tiles, n_tiles, d_sum, d_cnt, cnt_value, f, fix_thr); break;
    case 16: reduce_band_w<16>(st, g, slab, C, d_blk, n_win, n_blocks, d_Wt, w_stride, n_rep, mat_stride, d_tiles, n_tiles, d_sum, d_cnt, cnt_value, f, fix_thr); break;
    default: reduce_band_w<32>(st, g, slab, C, d_blk, n_win, n_blocks, d_Wt, w_stride, n_rep, mat_stride, d_tiles, n_tiles, d_sum, d_cnt, cnt_value, f, fix_thr);
  }
}

void ngd_launch_reduce_band_wv(hipStream_t st, const ngd_geom &g, const double *slab, const uint32_t *C, const uint32_t *d_blk,
                               const uint64_t *d_desc, uint32_t n_win, const void *d_Wt, uint32_t w_stride, uint32_t n_rep,
                               uint32_t mat_stride, const ngd_tile *d_tiles, uint32_t n_tiles, double *d_sum,
                               unsigned long long *d_cnt, const ngd_fix_flags *fix) {
  if (!n_tiles || !n_win || !n_rep) return;
  const ngd_fix_flags f = fix ? *fix : ngd_fix_flags{nullptr, nullptr, nullptr, 0};
  switch (ngd_reduce_chunk(n_rep)) {  // (the weights' stride is a multiple of it)
    case 1: reduce_band_wv<1>(st, g, slab, C, d_blk, d_desc, n_win, d_Wt, w_stride, n_rep, mat_stride, d_tiles, n_tiles, d_sum, d_cnt, f); break;
    case 4: reduce_band_wv<4>(st, g, slab, C, d_blk, d_desc, n_win, d_Wt, w_stride, n_rep, mat_stride, d_tiles, n_tiles, d_sum, d_cnt, f); break;
    case 16: reduce_band_wv<16>(st, g, slab, C, d_blk, d_desc, n_win, d_Wt, w_stride, n_rep, mat_stride, d_tiles, n_tiles, d_sum, d_cnt, f); break;
    default: reduce_band_wv<32>(st, g, slab, C, d_blk, d_desc, n_win, d_Wt, w_stride, n_rep, mat_stride, d_tiles, n_tiles, d_sum, d_cnt, f);
  }
}

void ngd_launch_fill_cnt(hipStream_t st, const ngd_geom &g, const ngd_tile *d_tiles, uint32_t n_tiles,
                         unsigned long long value, const unsigned long long *d_values, uint32_t n_rep,
                         unsigned long long *d_cnt) {
  if (!n_tiles || !n_rep) return;
  const uint64_t n_pairs = g.n_ind * (g.n_ind - 1) / 2;
  for (uint32_t r0 = 0; r0 < n_rep; r0 += 32768) {  // (grid.y holds 65 535)
    const uint32_t n = n_rep - r0 < 32768 ? n_rep - r0 : 32768;
    hipLaunchKernelGGL(k_fill_cnt, dim3(n_tiles * NGD_TILE, n), dim3(128), 0, st, d_tiles, g.n_ind, value,
                       d_values ? d_values + r0 : nullptr, n_pairs, d_cnt + (uint64_t)r0 * n_pairs);
  }
}

void ngd_launch_count(hipStream_t st, const ngd_geom &g, const unsigned long long *mask,
                      const unsigned long long *planes, uint32_t n_planes, const ngd_tile *d_tiles,
                      uint32_t n_tiles, unsigned long long *d_cnt) {
  if (!n_tiles) return;
  // enough workgroups to fill the chip: split the sites when the pair tiles alone are too few
  uint32_t ny = 1;
  while ((uint64_t)n_tiles * 12 * ny < 8192 && (uint64_t)ny * 2 * CW <= g.n_words) ny *= 2;
  hipLaunchKernelGGL(k_count, dim3(n_tiles * 16, ny), dim3(256), 0, st, mask, planes, n_planes, g.n_words, d_tiles,
                     g.n_ind, d_cnt);
}

// NGD_OPT_EM_EXACT: the host's verdict on the noted (pair, site)s, one thread per distinct pair: the pair's corrections
// c_ref - c_dev are added to its sum one by one, in site order (the order the host sorted them in)
namespace {
__global__ __launch_bounds__(256) void k_note_patch(const unsigned long long *__restrict__ pair, const uint32_t *__restrict__ first,
                                                    const double *__restrict__ delta, uint32_t n, double *__restrict__ d_sum) {
  const uint32_t q = blockIdx.x * 256 + threadIdx.x;
  if (q >= n) return;
  double s = d_sum[pair[q]];
  for (uint32_t k = first[q]; k < first[q + 1]; k++) s = s + delta[k];
  d_sum[pair[q]] = s;
}
// NGD_OPT_EM_EXACT = 2: one thread per (noted pair, matrix); the pair's corrections in site order, each weighted by the
// matrix's multiplicity of the site's block -- product first, then the sum (-ffp-contract=off), like the weighted passes
__global__ __launch_bounds__(256) void k_note_patch_w(const unsigned long long *__restrict__ pair, const uint32_t *__restrict__ first,
                                                      const double *__restrict__ delta, const unsigned long long *__restrict__ site,
                                                      uint32_t n, ngd_note_weights w, uint64_t n_sites, uint64_t n_pairs,
                                                      double *__restrict__ d_sum) {
  const uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (uint64_t)n * w.n_mat) return;
  const uint32_t r = (uint32_t)(idx / n), q = (uint32_t)(idx % n);
  double *out = d_sum + (uint64_t)r * n_pairs + pair[q];
  double s = *out;
  for (uint32_t k = first[q]; k < first[q + 1]; k++) {
    const uint64_t st = site[k];
    double m = 0.0;
    if (r < w.lead) m = st < n_sites ? 1.0 : 0.0;
    else {
      const uint64_t b = st / w.block_size, at = b * w.bs + (uint64_t)(r - w.lead) * w.rs;
      if (b < w.n_blocks) m = w.W ? w.W[at] : (double)w.M[at];
    }
    if (m != 0.0) s = s + m * delta[k];
  }
  *out = s;
}
// NGD_OPT_EM_EXACT_WIN: one thread per (noted pair, window of the batch, matrix of the launch); the pair's corrections in
// site order, each weighted by what the matrix makes of the site -- 1 inside [lo, hi) for a window's full-data matrix, the
// multiplicity of block (site - lo) / q for a replicate, 0 in the tail behind the last whole block (ngsDist.cpp:236) --
// product first, then the sum, like k_note_patch_w.  A cell no correction reaches is not written.
__global__ __launch_bounds__(256) void k_note_patch_win(const unsigned long long *__restrict__ pair, const uint32_t *__restrict__ first,
                                                        const double *__restrict__ delta, const unsigned long long *__restrict__ site,
                                                        uint32_t n, ngd_note_win w, uint64_t n_pairs, double *__restrict__ d_sum) {
  const uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (uint64_t)n * w.n_win * w.n_mat) return;
  const uint32_t q = (uint32_t)(idx % n);
  const uint64_t wm = idx / n;
  const uint32_t win = (uint32_t)(wm % w.n_win), r = (uint32_t)(wm / w.n_win);
  const uint64_t lo = w.lohi[2 * (uint64_t)win], hi = w.lohi[2 * (uint64_t)win + 1];
  double *out = d_sum + ((uint64_t)win * w.out_stride + w.mat0 + r) * n_pairs + pair[q];
  double s = *out;
  bool touched = false;
  for (uint32_t k = first[q]; k < first[q + 1]; k++) {
    const uint64_t st = site[k];
    if (st < lo || st >= hi) continue;
    double m = 1.0;
    if (w.W) {
      const uint64_t b = (st - lo) / w.q;
      m = b < w.n_blocks ? w.W[b * w.w_stride + r] : 0.0;
    }
    if (m != 0.0) {
      s = s + m * delta[k];
      touched = true;
    }
  }
  if (touched) *out = s;
}
}  // namespace

void ngd_launch_note_patch_win(hipStream_t st, const unsigned long long *d_pair, const uint32_t *d_first, const double *d_delta,
                               const unsigned long long *d_site, uint32_t n_pairs_noted, const ngd_note_win &w, uint64_t n_pairs,
                               double *d_sum) {
  if (!n_pairs_noted || !w.n_win || !w.n_mat || (w.W && !w.q)) return;
  const uint64_t n = (uint64_t)n_pairs_noted * w.n_win * w.n_mat;
  // (n < NGD_NOTE_WIN_MAX threads: the caller has checked)
  hipLaunchKernelGGL(k_note_patch_win, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_pair, d_first, d_delta, d_site,
                     n_pairs_noted, w, n_pairs, d_sum);
}

void ngd_launch_note_patch_w(hipStream_t st, const unsigned long long *d_pair, const uint32_t *d_first, const double *d_delta,
                             const unsigned long long *d_site, uint32_t n_pairs_noted, const ngd_note_weights &w,
                             uint64_t n_sites, uint64_t n_pairs, double *d_sum) {
  if (!n_pairs_noted || !w.n_mat || !w.block_size) return;
  const uint64_t n = (uint64_t)n_pairs_noted * w.n_mat;
  hipLaunchKernelGGL(k_note_patch_w, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_pair, d_first, d_delta, d_site,
                     n_pairs_noted, w, n_sites, n_pairs, d_sum);
}

void ngd_launch_note_patch(hipStream_t st, const unsigned long long *d_pair, const uint32_t *d_first, const double *d_delta,
                           uint32_t n_pairs_noted, double *d_sum) {
  if (!n_pairs_noted) return;
  hipLaunchKernelGGL(k_note_patch, dim3((n_pairs_noted + 255) / 256), dim3(256), 0, st, d_pair, d_first, d_delta, n_pairs_noted,
                     d_sum);
}
