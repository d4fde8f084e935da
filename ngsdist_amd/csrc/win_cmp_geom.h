// win_cmp_geom.h -- the geometry of the comparison of windows (include/ngsdist_amd.h "Comparison of windows"), in one place for
// the kernels' launchers (win_cmp.hip) and the host twin (host_util.cpp): plain host arithmetic on (n_vec, n_cells).
#pragma once
#include <stdint.h>

#define NGD_WIN_CMP_MAX_VEC 65536u  // 4096 groups of 16 vectors: the grids' y extent and the tile indices hold them

// the Gram kernel's tile block: T x T tiles of 16 x 16 vectors, T by the number of vector groups
inline uint32_t ngd_wincmp_tile_edge(uint64_t n_vec) {
  const uint64_t n_g = (n_vec + 15) / 16;
  return (uint32_t)(n_g < 4 ? n_g : 4);
}
// vector groups of 16 in the operand Z: whole tile blocks
inline uint32_t ngd_wincmp_groups(uint64_t n_vec) {
  const uint32_t T = ngd_wincmp_tile_edge(n_vec), n_g = (uint32_t)((n_vec + 15) / 16);
  return T ? (n_g + T - 1) / T * T : 0;
}
// tile blocks on or above the diagonal
inline uint64_t ngd_wincmp_blocks(uint64_t n_vec) {
  const uint64_t n_br = ngd_wincmp_groups(n_vec) / ngd_wincmp_tile_edge(n_vec);
  return n_br * (n_br + 1) / 2;
}
// Cells per slice, a multiple of 4: ngd_win_cmp_slice().  The Gram kernel starts one wavefront per (tile block, slice); about
// 4096 are wanted (256 CUs x 4 SIMDs x 4) and a slice is never shorter than 256 cells (64 k-groups), so few vectors give
// many slices and thousands of vectors one or two: the partials stay near 4096 x T^2 x 2 x 2 KiB = 256 MiB until one slice's
// W x W doubles exceed that.  A function of (n_vec, n_cells) alone: the contract's bit rule depends on it.
inline uint64_t ngd_wincmp_slice(uint64_t n_vec, uint64_t n_cells) {
  if (!n_vec || !n_cells || n_vec > NGD_WIN_CMP_MAX_VEC) return 0;
  const uint64_t n_blk = ngd_wincmp_blocks(n_vec), want = 4096 / n_blk ? 4096 / n_blk : 1;
  uint64_t s = (n_cells + want - 1) / want;
  if (s < 256) s = 256;
  return (s + 3) & ~3ull;
}
