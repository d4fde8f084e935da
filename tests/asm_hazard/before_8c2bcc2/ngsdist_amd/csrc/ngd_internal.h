// Internal declarations shared by the engine and its kernels (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ngsdist_amd.h"

#define NGD_TILE 128     // pair tile edge owned by one workgroup of the MFMA kernel
#define NGD_IG 16        // individuals per fragment group (one MFMA operand edge)
#define NGD_IG_PER_TILE (NGD_TILE / NGD_IG)
#define NGD_KG_TAIL 8    // zeroed k-groups appended to the operand images (pipeline run-ahead)
#define NGD_KG_LIST_PAD 16  // entries appended to a k-group list, all pointing at the first tail k-group

typedef double ngd_d4 __attribute__((ext_vector_type(4)));

struct ngd_score {
  double v[9];
};

// Geometry of the resident data set.
//
// Fragment-major operand layout ("PA", and "QB" = score-weighted copy):
//   the contraction index is k = 3*s + g  (site s, genotype g);
//   element (i, k) lives at  ((k/4)*n_ig + i/16)*64 + (k%4)*16 + i%16.
// One 64-double group (512 B) is exactly the per-lane operand image of
// v_mfma_f64_16x16x4_f64 (lane l <-> individual l&15, k-offset l>>4), so a
// wavefront fetches an operand with one fully coalesced 512-B load and 16
// consecutive individuals of one (site, genotype) are 128 contiguous bytes.
struct ngd_geom {
  uint64_t n_ind;
  uint64_t n_sites;
  uint64_t n_sites_pad;  // multiple of 16 -> n_kg multiple of 12
  uint64_t n_kg;         // k groups of 4 = 3*n_sites_pad/4
  uint32_t n_ig;         // individual groups of 16, padded to a multiple of 8
  uint32_t n_t;          // 128-individual tiles per edge
  uint32_t n_pad;        // n_t * 128
  uint32_t n_words;      // 64-site mask words per individual
};

__host__ __device__ inline uint64_t ngd_frag_off(uint64_t k, uint32_t i, uint32_t n_ig) {
  return ((k >> 2) * n_ig + (i >> 4)) * 64 + (k & 3) * 16 + (i & 15);
}

// row-major upper-triangle pair index, ngsDist.cpp:244-245
__host__ __device__ inline uint64_t ngd_pair_idx(uint64_t n, uint64_t i, uint64_t j) {
  return i * (2 * n - i - 1) / 2 + (j - i - 1);
}

// miss_data(), reference gen_func.cpp:862-868 (EPSILON = 1e-5, gen_func.hpp:16)
__host__ __device__ inline bool ngd_miss(double p0, double p1, double p2) {
  double a = p0 - p1, b = p1 - p2;
  a = (a >= 0 ? a : -a);
  b = (b >= 0 ? b : -b);
  return a < 1e-5 && b < 1e-5;
}

struct ngd_tile {
  uint16_t ti, tj;  // tile coordinates (units depend on the list: 128 or 16 individuals)
};

// One wavefront's work in the MFMA kernel: the block of pairs whose first row / column groups (of 16
// individuals) are ig0 / jg0, rows x cols MFMA tiles (1..4 each), upper triangle only if tri.
// rows == 0 marks a padding entry of the list.
struct ngd_job {
  uint16_t ig0, jg0;
  uint8_t rows, cols, tri, pad;
};

// ---- kernel launchers (each in its own .hip file) -------------------------
// layout.hip
void ngd_launch_layout(hipStream_t st, const ngd_geom &g, const double *raw, int raw_ind_major,
                       uint64_t s0, uint64_t n_sites_chunk, const ngd_score &score, int pairwise_del,
                       double *PA, double *QB, double *PI, unsigned long long *mask);
void ngd_launch_prep_layout(hipStream_t st, const ngd_geom &g, const double *raw, uint64_t s0, uint64_t n_chunk,
                            int in_logscale, int call_geno, double N_thresh, double call_thresh,
                            const ngd_score &score, int pairwise_del, double *PA, double *QB, double *PI,
                            unsigned long long *mask, int *nan_flag);
void ngd_launch_synth(hipStream_t st, const ngd_geom &g, uint64_t seed, double miss_frac, uint64_t site0,
                      const ngd_score &score, int pairwise_del, double *PA, double *QB, double *PI,
                      unsigned long long *mask);
void ngd_launch_weights(hipStream_t st, uint64_t n_blocks, uint64_t block_size, uint64_t n_sites,
                        const uint32_t *d_mult, uint32_t *d_ws, double *d_wk);
// list of the k-groups with a non-zero bootstrap weight (ascending), NGD_KG_LIST_PAD entries of padding;
// d_counts: ngd_kg_count_blocks(n_kg) + 1 words of scratch, the last one receives the list length
uint32_t ngd_kg_count_blocks(uint64_t n_kg);
void ngd_launch_kg_compact(hipStream_t st, const double *d_wk, uint64_t n_kg, uint32_t tail_kg, uint32_t *d_counts,
                           uint32_t *d_list);
void ngd_launch_weights_batch(hipStream_t st, const uint32_t *d_mult, uint32_t n_rep, uint32_t rb, int lead_full,
                              uint64_t n_blocks, uint64_t block_size, uint64_t n_sites, uint64_t n_sites_alloc,
                              double *d_W);
// W[slice][j][c] = 1 if contraction index 4 (kg0(slice) + j) + c lies in [slice k_per_slice, (slice+1) k_per_slice)
// and below k_total, else 0; kg0(slice) = slice * k_per_slice / 4; j < stride
void ngd_launch_slice_weights(hipStream_t st, uint32_t n_slices, uint32_t stride, uint64_t k_per_slice, uint64_t k_total,
                              double *d_W);
void ngd_launch_planes(hipStream_t st, const uint32_t *d_ws, uint64_t n_sites, uint32_t n_words,
                       uint32_t n_planes, unsigned long long *d_planes);

// accum_stream.hip : one wavefront per pair
void ngd_launch_accum_stream(hipStream_t st, const ngd_geom &g, const double *PI, const uint32_t *d_ws,
                             uint64_t n_sites_eff, const ngd_score &score, int pairwise_del,
                             const uint64_t *d_pairs, uint64_t n_owned, double *d_sum);

// accum_mfma.hip : FP64 MFMA tiles, split over site slices into slabs
// d_wk / d_kgl: bootstrap weights per contraction index and the list of k-groups to visit; with a list,
// kg_per_slice and n_kg_eff count LIST entries.  k_per_slice != 0: slices are k_per_slice contraction indices
// (not whole k-groups) and d_wk holds w_slice_stride k-groups of 0/1 weights PER SLICE (ngd_launch_slice_weights).
void ngd_launch_accum_mfma(hipStream_t st, const ngd_geom &g, const double *PA, const double *QB,
                           const double *d_wk, const uint32_t *d_kgl, const ngd_job *d_jobs, uint32_t n_wg,
                           int exact_shapes, uint32_t wg_waves, uint32_t n_ks, uint64_t kg_per_slice, uint64_t n_kg_eff,
                           uint64_t k_per_slice, uint32_t w_slice_stride, double *slab,
                           unsigned long long *d_clk /* [2] or NULL: shader-cycle / constant-rate counter deltas of one wavefront */);

// accum_em.hip : per-site EM, one thread per pair of a 16x16 tile
void ngd_launch_accum_em(hipStream_t st, const ngd_geom &g, const double *PA, const uint32_t *d_ws,
                         uint64_t n_sites_eff, const ngd_score &score, int pairwise_del, int fast,
                         const ngd_tile *d_tiles16, uint32_t n_tiles16, uint32_t n_ks,
                         uint64_t sites_per_slice, double *slab);

// accum_em_table.hip : per-site EM with per-individual tables shared by a 64 x 64 tile of pairs
void ngd_launch_accum_em_table(hipStream_t st, const ngd_geom &g, const double *PA, const uint32_t *d_ws,
                               uint64_t n_sites_eff, const ngd_score &score, int pairwise_del, int shape,
                               const ngd_tile *d_tiles64, uint32_t n_tiles64, uint32_t n_ks, uint64_t sites_per_slice,
                               double *slab, unsigned long long *d_counters /* [4]: += (tile, site) visits, table rounds; [2..3] = clock counters */);

// accum_em_table.hip, rb (4 or 8) matrices in one pass: d_Wb is [n_sites][rb] doubles, slab [n_ks][rb][n_pad][n_pad]
void ngd_launch_accum_em_table_batch(hipStream_t st, const ngd_geom &g, const double *PA, const double *d_Wb, int rb,
                                     uint64_t n_sites_eff, const ngd_score &score, int pairwise_del,
                                     const ngd_tile *d_tiles64, uint32_t n_tiles64, uint32_t n_ks,
                                     uint64_t sites_per_slice, double *slab, unsigned long long *d_counters);

// accum_em_table.hip, terms unsummed: sites [s_lo, s_hi) of every pair slot into C (fragment-major: k-groups of 4 sites
// x n_tiles64 * 256 groups of 16 pair slots); *d_nanflag = 1 if a term was not finite
void ngd_launch_accum_em_table_spill(hipStream_t st, const ngd_geom &g, const double *PA, uint64_t s_lo, uint64_t s_hi,
                                     const ngd_score &score, int pairwise_del, const ngd_tile *d_tiles64,
                                     uint32_t n_tiles64, uint32_t n_ks, uint64_t sites_per_slice, double *C,
                                     unsigned long long *d_counters, unsigned long long *d_nanflag);

// contract_mfma.hip : running sums D[matrix][pair slot] += W[matrix][site] * C[site][pair slot] over a chunk of sites
uint32_t ngd_contract_rep_groups(uint32_t n_mat);  // groups of 16 matrices
void ngd_launch_spill_weights(hipStream_t st, const uint32_t *d_mult, uint32_t n_mat, int lead, uint64_t s_lo,
                              uint64_t s_hi, uint64_t n_sites, uint64_t n_eff, uint64_t n_blocks, uint64_t block_size,
                              double *d_Wt);
void ngd_launch_spill_sanitize(hipStream_t st, double *C, const unsigned long long *d_flag, uint64_t n_kg, uint32_t n_pg,
                               const uint32_t *d_mult, uint32_t n_mat, int lead, uint64_t s_lo, uint64_t n_sites,
                               uint64_t n_eff, uint64_t n_blocks, uint64_t block_size, double *D);
void ngd_launch_contract(hipStream_t st, const double *d_Wt, const double *C, uint32_t n_mat, uint32_t n_pg, uint32_t n_kg,
                         double *D);
void ngd_launch_spill_scatter(hipStream_t st, const double *D, uint32_t n_pg, const ngd_tile *d_tiles64, uint32_t n_tiles64,
                              uint64_t n_ind, uint32_t n_mat, double *d_sum);

// rb (4, 8 or 16) replicates in one pass; d_Wb is [n_sites][rb] doubles, slab [n_ks][rb][n_pad][n_pad]
void ngd_launch_accum_em_batch(hipStream_t st, const ngd_geom &g, const double *PA, const double *d_Wb, int rb,
                               uint64_t n_sites_eff, const ngd_score &score, int pairwise_del, int fast,
                               const ngd_tile *d_tiles16, uint32_t n_tiles16, uint32_t n_ks,
                               uint64_t sites_per_slice, double *slab);

// reduce.hip : deterministic slab reduction + valid-site counting
// planes_per_slice: the slab holds that many result planes per slice (EM batch kernel), `slab` points at
// the first slice's plane of the wanted result
// d_cnt != NULL: every pair's count is set to cnt_value in the same launch (no --pairwise_del)
void ngd_launch_reduce(hipStream_t st, const ngd_geom &g, const double *slab, uint32_t n_ks,
                       uint32_t planes_per_slice, const ngd_tile *d_tiles, uint32_t n_tiles, double *d_sum,
                       unsigned long long *d_cnt = nullptr, unsigned long long cnt_value = 0);
uint32_t ngd_reduce_chunk(uint32_t n_rep);  // replicates per pass; weight strides are multiples of it
void ngd_launch_reduce_w(hipStream_t st, const ngd_geom &g, const double *slab, uint32_t n_ks, const double *d_W,
                         uint32_t w_stride, uint32_t n_rep, const ngd_tile *d_tiles, uint32_t n_tiles,
                         double *d_sum);
void ngd_launch_reduce_c(hipStream_t st, const ngd_geom &g, const uint32_t *C, uint32_t n_blocks, const uint32_t *d_M,
                         uint32_t m_stride, uint32_t n_rep, const ngd_tile *d_tiles, uint32_t n_tiles,
                         unsigned long long *d_cnt);
void ngd_launch_count_blocks(hipStream_t st, const ngd_geom &g, const unsigned long long *mask, uint64_t block_size,
                             uint32_t n_blocks, const ngd_tile *d_tiles16, uint32_t n_tiles16, uint32_t *C);
void ngd_launch_count(hipStream_t st, const ngd_geom &g, const unsigned long long *mask,
                      const unsigned long long *planes, uint32_t n_planes, const ngd_tile *d_tiles,
                      uint32_t n_tiles, unsigned long long *d_cnt);  // owned 128-tiles
void ngd_launch_fill_cnt(hipStream_t st, const ngd_geom &g, const ngd_tile *d_tiles, uint32_t n_tiles,
                         unsigned long long value, const unsigned long long *d_values, uint32_t n_rep,
                         unsigned long long *d_cnt);
