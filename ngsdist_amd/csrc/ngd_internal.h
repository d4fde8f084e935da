// Internal declarations shared by the engine and its kernels (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ngsdist_amd.h"
#include "ngd_layout.h"
#include "win_plan.h"
#include "win_cmp_geom.h"

#define NGD_TILE 128     // pair tile edge owned by one workgroup of the MFMA kernel
#define NGD_IG 16        // individuals per fragment group (one MFMA operand edge)
#define NGD_IG_PER_TILE (NGD_TILE / NGD_IG)
#define NGD_KG_TAIL 8    // zeroed k-groups appended to the operand images (pipeline run-ahead)
#define NGD_KG_LIST_PAD 16  // entries appended to a k-group list, all pointing at the first tail k-group

typedef double ngd_d4 __attribute__((ext_vector_type(4)));

struct ngd_score {
  double v[9];
  // single_image = 2 (host_util.cpp ngd_score_congruence()): score = SUM_r d[r] c_r c_r^T.  The ONE operand image then holds
  // t_r = c_r . p per site instead of p, both operands of the MFMA kernel are read from it, and d[r] rides on the
  // per-index weights.  congruent = 0: the image holds p.
  double c[9], d[3];
  int congruent;
  // congruent images of the reference's two matrices (parse_args.cpp:25-27, :134-137) hold t = (p0 + p1 + p2, +-(p2 - p0),
  // p1): with min(p0, p2) kept beside the image (one double per individual and site), p comes back to the last bit or
  // so -- what the fix-up pass of nearly identical pairs recomputes from (fixup.hip).  fix = 1: the image has that form
  // (fix_sign = the sign of p2 in t_1); 0: any other symmetric matrix, no fix-up.
  int fix;
  double fix_sign;
};

// Geometry of the resident data set.
//
// Fragment-major operand layout ("PA", and "QB" = score-weighted copy):
//   the contraction index is k = 3*s + g  (site s, genotype g) -- except in the ONE image of a congruent engine
//   (single_image = 2), where twelve indices are still four whole sites but the four t0 of a period fill a k-group of
//   their own: k = ngd_k_of(s, coordinate, 1), ngd_layout.h (which also turns site ranges into k-group ranges);
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

// The block shapes accum_mfma.hip has a code path for, per block form (ngd_engine::exact_shapes: 0 full 4 x 4 pattern;
// 1 / 3 blocks of up to 4 x 4 tiles, any shape falls back to the full pattern; 2 / 4 / 5 blocks of up to 2 x 4).
// ngd_create() checks the job list it built against this; the kernel poisons (NaN) a block whose shape it does not list.
inline bool ngd_mfma_shape_listed(int form, uint32_t rows, uint32_t cols, uint32_t tri) {
  if (rows == 0) return true;  // padding entry
  if (form == 0 || form == 1 || form == 3) return rows <= 4 && cols <= 4;
  if (tri) return (rows == 2 && cols >= 2 && cols <= 4) || (rows == 1 && cols == 1);
  return rows == 2 && cols >= 1 && cols <= 4;
}

// ---- kernel launchers (each in its own .hip file) -------------------------
// layout.hip
// (PI: the individual-major copy of the streaming kernel -- or, with score.congruent and score.fix, the side array
// SM[site][individual] = min(p0, p2) of the fix-up pass)
void ngd_launch_layout(hipStream_t st, const ngd_geom &g, const double *raw, int raw_ind_major,
                       uint64_t s0, uint64_t n_sites_chunk, const ngd_score &score, int pairwise_del,
                       double *PA, double *QB, double *PI, unsigned long long *mask);
// single-image engines: QB of k-groups [kg_lo, kg_hi) from PA, element (i, k) at ngd_frag_off(k, i) - kg_lo * n_ig * 64
void ngd_launch_qb_range(hipStream_t st, const ngd_geom &g, const ngd_score &score, const double *PA, uint64_t kg_lo,
                         uint64_t kg_hi, double *QBs);
void ngd_launch_prep_layout(hipStream_t st, const ngd_geom &g, const double *raw, uint64_t s0, uint64_t n_chunk,
                            int in_logscale, int call_geno, double N_thresh, double call_thresh,
                            const ngd_score &score, int pairwise_del, double *PA, double *QB, double *PI,
                            unsigned long long *mask, int *nan_flag);
void ngd_launch_synth(hipStream_t st, const ngd_geom &g, uint64_t seed, double miss_frac, uint64_t site0,
                      const ngd_score &score, int pairwise_del, double *PA, double *QB, double *PI,
                      unsigned long long *mask);
// (d3 != NULL: the congruence's diagonal per coordinate, and the image's layout is the congruent one -- quad, ngd_layout.h)
void ngd_launch_weights(hipStream_t st, uint64_t n_blocks, uint64_t block_size, uint64_t n_sites,
                        const uint32_t *d_mult, uint32_t *d_ws, double *d_wk, const double *d3 = nullptr);
// list of the k-groups with a non-zero bootstrap weight (ascending), NGD_KG_LIST_PAD entries of padding;
// d_counts: ngd_kg_count_blocks(n_kg) + 1 words of scratch, the last one receives the list length
uint32_t ngd_kg_count_blocks(uint64_t n_kg);
void ngd_launch_kg_compact(hipStream_t st, const double *d_wk, uint64_t n_kg, uint32_t tail_kg, uint32_t *d_counts,
                           uint32_t *d_list);
void ngd_launch_weights_batch(hipStream_t st, const uint32_t *d_mult, uint32_t n_rep, uint32_t rb, int lead_full,
                              uint64_t n_blocks, uint64_t block_size, uint64_t n_sites, uint64_t n_sites_alloc,
                              double *d_W);
// W[slice][j][c] = 1 if contraction index 4 (kg0(slice) + j) + c lies in [slice k_per_slice, (slice+1) k_per_slice)
// and below k_total, else 0; kg0(slice) = slice * k_per_slice / 4; j < stride.  Images with k = 3 s + g only: the blocks of
// a congruent engine's image go by slice table (ngd_launch_seg_weights)
void ngd_launch_slice_weights(hipStream_t st, uint32_t n_slices, uint32_t stride, uint64_t k_per_slice, uint64_t k_total,
                              double *d_W);
// single_image = 2: the weights of a plain pass, d3[coordinate of k] for every contraction index of the image (+ tail)
void ngd_launch_index_weights(hipStream_t st, uint64_t n_k, const double *d3, double *d_W);
// single_image = 2 on the reference's matrices: E[i] += SUM_s (t0_i(s) - 1) in units of 2^-53 (exact: 64-bit integers, so
// the result does not depend on the order) over the t0 k-groups of the image; *d_flag |= 1 if some t0 is not finite or
// |t0 - 1| > 2^-40 (the data set is then not *unit*: no pass may take the coordinate's products as a constant)
void ngd_launch_unit_scan(hipStream_t st, const ngd_geom &g, const double *T, long long *d_E, int *d_flag);
void ngd_launch_planes(hipStream_t st, const uint32_t *d_ws, uint64_t n_sites, uint32_t n_words,
                       uint32_t n_planes, unsigned long long *d_planes);

// accum_stream.hip : one wavefront per pair
void ngd_launch_accum_stream(hipStream_t st, const ngd_geom &g, const double *PI, const uint32_t *d_ws,
                             uint64_t n_sites_eff, const ngd_score &score, int pairwise_del,
                             const uint64_t *d_pairs, uint64_t n_owned, double *d_sum);

// Windows along the genome (engine_windows.hip windows_slab) and, in a congruent engine's image, bootstrap blocks that are
// not whole periods of four sites (engine_plans.hip partials_impl): the slice table's layout NGD_SEG_* is win_plan.h's.
// layout.hip: the weights of every segment of the table (w_total k-groups in all)
void ngd_launch_seg_weights(hipStream_t st, const uint64_t *d_seg, uint32_t n_seg, uint64_t max_wkg, const double *d3,
                            double *d_W);

// accum_mfma.hip : FP64 MFMA tiles, split over site slices into slabs
// what ngd_create() fixes for the engine's lifetime
struct ngd_mfma_engine {
  const ngd_geom &g;
  const ngd_job *d_jobs;
  uint32_t n_wg;
  int exact_shapes;  // 3: n_wg = 1 workgroup of wg_waves wavefronts per slice
  uint32_t wg_waves;
  unsigned long long *d_clk;  // [2] or NULL: shader-cycle / constant-rate counter deltas of one wavefront
};
// one launch; what it does not set is off
struct ngd_mfma_launch {
  const double *PA = nullptr, *QB = nullptr;  // the two operand images
  // d_wk / d_kgl: bootstrap weights per contraction index and the list of k-groups to visit; with a list,
  // kg_per_slice and n_kg_eff count LIST entries.  k_per_slice != 0: slices are k_per_slice contraction indices
  // (not whole k-groups) and d_wk holds w_slice_stride k-groups of 0/1 weights PER SLICE (ngd_launch_slice_weights).
  const double *d_wk = nullptr;
  const uint32_t *d_kgl = nullptr;
  uint32_t n_ks = 0;
  uint64_t kg_per_slice = 0, n_kg_eff = 0, k_per_slice = 0;
  uint32_t w_slice_stride = 0;
  double *slab = nullptr;
  uint32_t ks0 = 0;     // the launch covers slices ks0 .. ks0 + n_ks - 1 (multiples of 8)
  uint32_t resume = 0;  // 1: every block continues from its plane of the slab (a pass in ranges)
  // slice table [n_ks][NGD_SEG_STRIDE] (windows): each slice's own k-group range and weight offset; needs d_wk and w_slice_stride != 0
  const uint64_t *d_seg = nullptr;
};
void ngd_launch_accum_mfma(hipStream_t st, const ngd_mfma_engine &en, const ngd_mfma_launch &l);

// accum_em.hip : per-site EM, one thread per pair of a 16x16 tile
void ngd_launch_accum_em(hipStream_t st, const ngd_geom &g, const double *PA, const uint32_t *d_ws,
                         uint64_t n_sites_eff, const ngd_score &score, int pairwise_del, int fast,
                         const ngd_tile *d_tiles16, uint32_t n_tiles16, uint32_t n_ks,
                         uint64_t sites_per_slice, double *slab);

// accum_em_table.hip : per-site EM with per-individual tables shared by a 64 x 64 tile of pairs
// what every launcher of the file is handed (`shape`: the batch and spilled-terms forms have one of their own)
struct ngd_emt_common {
  const ngd_geom &g;
  const double *PA;
  const ngd_score &score;
  int pairwise_del, shape;
  const ngd_tile *d_tiles64;
  uint32_t n_tiles64;
  unsigned long long *d_counters;  // [4]: += (tile, site) visits, table rounds; [2..3] = clock counters
};
void ngd_launch_accum_em_table(hipStream_t st, const ngd_emt_common &c, const uint32_t *d_ws, uint64_t n_sites_eff, uint32_t n_ks,
                               uint64_t sites_per_slice, double *slab);

// NGD_OPT_EM_EXACT: the noting form of the plain pass.  The rows' thresholds are widened by (1 + NGD_EM_EXACT_BETA), so
// that no step before the one a pair stops at can be the reference's stopping step; a stop whose criterion is not below
// the threshold narrowed by as much -- R < Q (1 - beta) -- is within rounding of the tolerance, and is noted for the
// host's recheck (engine_em_exact.hip).  The note buffer: [0] entries noted (counts on past the capacity), [1] the
// capacity in entries, then from word NGD_NOTE_HEAD on NGD_NOTE_WORDS words per entry:
//   i1 | i2 << 32,  site,  the step the pair stopped at (1 .. 50),  the bits of the term it added
// (word 0 leaves the accumulation kernel as workgroup | row of the tile << 32 | column << 40; ngd_launch_note_gather rewrites it)
#define NGD_EM_EXACT_BETA 0x1p-36
#define NGD_NOTE_HEAD 4
#define NGD_NOTE_WORDS 4
void ngd_launch_accum_em_table_note(hipStream_t st, const ngd_emt_common &c, uint32_t n_ks, uint64_t sites_per_slice, double *slab,
                                    unsigned long long *d_note);
// layout.hip: the six likelihoods of every noted (pair, site) out of the image: gl[6 e ..] = GL_i1[0..2], GL_i2[0..2]
void ngd_launch_note_gather(hipStream_t st, const ngd_geom &g, const double *PA, const ngd_tile *d_tiles64, uint32_t n_tiles64,
                            unsigned long long *d_entries, uint32_t n, double *d_gl);
// reduce.hip: d_sum[pair[q]] += delta[first[q]] + ... + delta[first[q + 1] - 1], added one by one in that order
void ngd_launch_note_patch(hipStream_t st, const unsigned long long *d_pair, const uint32_t *d_first, const double *d_delta,
                           uint32_t n_pairs_noted, double *d_sum);
// reduce.hip, NGD_OPT_EM_EXACT = 2: the same corrections into n_mat matrices that weight sites by bootstrap block.  Matrix
// r < lead is the full data set (weight 1 on every site); matrix lead + q weights a site of block b = site / block_size by
// W[b * bs + q * rs] (doubles; per-block partials) or M[b * bs + q * rs] (multiplicities; the spilled-terms plan), and
// by 0 from site n_blocks * block_size on (ngsDist.cpp:236).  d_sum[r * n_pairs + pair] += (double)m * delta, one by one in
// site order, where m != 0.
struct ngd_note_weights {
  uint32_t n_mat, lead;
  const double *W;
  const uint32_t *M;
  uint64_t rs, bs, n_blocks, block_size;
};
void ngd_launch_note_patch_w(hipStream_t st, const unsigned long long *d_pair, const uint32_t *d_first, const double *d_delta,
                             const unsigned long long *d_site, uint32_t n_pairs_noted, const ngd_note_weights &w,
                             uint64_t n_sites, uint64_t n_pairs, double *d_sum);
// reduce.hip, NGD_OPT_EM_EXACT_WIN: the same corrections into the matrices of a batch of windows (engine_windows.hip, the slab
// plans).  Window w of the batch is sites [lohi[2 w], lohi[2 w + 1]); the launch patches matrices mat0 .. mat0 + n_mat - 1 of
// every window, window w's matrix m at d_sum[(w * out_stride + m) * n_pairs ..].  W == NULL: full-data matrices, weight 1 on the
// window's sites.  Else matrix mat0 + r weights a site of block b = (site - lo) / q by W[b * w_stride + r] where b < n_blocks,
// and by 0 behind the last whole block.  pairs x n_win x n_mat must be below NGD_NOTE_WIN_MAX.
struct ngd_note_win {
  const unsigned long long *lohi;
  uint32_t n_win, n_mat, mat0, out_stride;
  const double *W;
  uint32_t w_stride;
  uint64_t n_blocks, q;
};
#define NGD_NOTE_WIN_MAX (1ull << 39)
void ngd_launch_note_patch_win(hipStream_t st, const unsigned long long *d_pair, const uint32_t *d_first, const double *d_delta,
                               const unsigned long long *d_site, uint32_t n_pairs_noted, const ngd_note_win &w, uint64_t n_pairs,
                               double *d_sum);

// accum_em_table.hip, windows along the genome: slice ks = sites [s_lo, s_hi) of entry ks of the slice table (NGD_SEG_SLO /
// NGD_SEG_SHI; any length from 1, any first site, all below g.n_sites), slab [n_seg][n_pad][n_pad]; every `shape` has the form
void ngd_launch_accum_em_table_segs(hipStream_t st, const ngd_emt_common &c, uint32_t n_seg, const uint64_t *d_seg, double *slab);
// ... and its noting form (NGD_OPT_EM_EXACT_WIN): entries as ngd_launch_accum_em_table_note leaves them, sites absolute
void ngd_launch_accum_em_table_segs_note(hipStream_t st, const ngd_emt_common &c, uint32_t n_seg, const uint64_t *d_seg, double *slab,
                                         unsigned long long *d_note);

// accum_em_table.hip, rb (4 or 8) matrices in one pass: d_Wb is [n_sites][rb] doubles, slab [n_ks][rb][n_pad][n_pad]
void ngd_launch_accum_em_table_batch(hipStream_t st, const ngd_emt_common &c, const double *d_Wb, int rb, uint64_t n_sites_eff,
                                     uint32_t n_ks, uint64_t sites_per_slice, double *slab);

// accum_em_table.hip, terms not summed over the slice: sites [s_lo, s_hi) in units of q consecutive sites (one term per
// pair slot and unit) into C (fragment-major: k-groups of 4 units x n_pg groups of 16 pair slots; d_rowpg[tile * 64 + row] + g =
// slot group of the row's group g of 16 columns, for the groups that hold a pair); *d_nanflag = 1 if a term was not finite;
// d_note != NULL: the noting form
void ngd_launch_accum_em_table_spill(hipStream_t st, const ngd_emt_common &c, uint64_t s_lo, uint64_t s_hi, uint32_t n_ks,
                                     uint64_t sites_per_slice, uint32_t q, const uint32_t *d_rowpg, uint32_t n_pg, double *C,
                                     unsigned long long *d_nanflag, unsigned long long *d_note);

// contract_mfma.hip : running sums D[matrix][pair slot] += W[matrix][unit] * C[unit][pair slot] over a chunk of sites
// (a unit = q consecutive sites of one bootstrap block; site s_lo is the first site of the chunk's unit 0)
uint32_t ngd_contract_rep_groups(uint32_t n_mat);  // groups of 16 matrices
void ngd_launch_spill_weights(hipStream_t st, const uint32_t *d_mult, uint32_t n_mat, int lead, uint64_t s_lo,
                              uint64_t s_hi, uint32_t q, uint64_t n_sites, uint64_t n_eff, uint64_t n_blocks,
                              uint64_t block_size, double *d_Wt);
void ngd_launch_spill_sanitize(hipStream_t st, double *C, const unsigned long long *d_flag, uint64_t n_kg, uint32_t n_pg,
                               const uint32_t *d_mult, uint32_t n_mat, int lead, uint64_t s_lo, uint32_t q, uint64_t n_sites,
                               uint64_t n_eff, uint64_t n_blocks, uint64_t block_size, double *D);
// n_pg must be a multiple of 4 (ngd_create pads the slot groups)
void ngd_launch_contract(hipStream_t st, const double *d_Wt, const double *C, uint32_t n_mat, uint32_t n_pg, uint32_t n_kg,
                         double *D);
void ngd_launch_spill_scatter(hipStream_t st, const double *D, uint32_t n_pg, const ngd_tile *d_tiles64, uint32_t n_tiles64,
                              const uint32_t *d_rowpg, uint64_t n_ind, uint32_t n_mat, double *d_sum);

// accum_em_table.hip: slices ks0 .. ks0 + n_sub - 1 of a plain pass on their own, lds_pad more bytes of LDS per workgroup
void ngd_launch_accum_em_table_slices(hipStream_t st, const ngd_emt_common &c, uint32_t ks0, uint32_t n_sub, uint64_t sites_per_slice,
                                      double *slab, uint32_t lds_pad);
// accum_em.hip: rb (4, 8 or 16) replicates in one pass; d_Wb is [n_sites][rb] doubles, slab [n_ks][rb][n_pad][n_pad]
void ngd_launch_accum_em_batch(hipStream_t st, const ngd_geom &g, const double *PA, const double *d_Wb, int rb,
                               uint64_t n_sites_eff, const ngd_score &score, int pairwise_del, int fast,
                               const ngd_tile *d_tiles16, uint32_t n_tiles16, uint32_t n_ks,
                               uint64_t sites_per_slice, double *slab);

// fixup.hip : single_image = 2 engines, the pairs whose sums the congruent arithmetic cannot hold to 1e-9 relative
// (mean per-site term below NGD_FIX_MEAN: nearly identical individuals) recomputed with two-operand arithmetic from
// p recovered out of the image T and the side array SM[site][individual] = min(p0, p2).
#define NGD_FIX_MEAN 1e-6  // flag a pair whose sum is below this x the sites its matrix visits (error bound: 4e-17 per site)
// The plain pass that leaves the unit-sum coordinate out (NGD_OPT_UNIT_SKIP) delivers its sums only if NONE is below this x
// the sites: without the +1/2 of every site its accumulators run to -(sites of a slice) / 2 and the constant cancels them at
// the end, so a sum carries ~2^-53 of n / 2 per rounding -- [measured] 7e-13 absolute at 3000 sites, 5e-10 at 1e6 -- instead
// of 4e-17 per site.  Were every rounding of a slice aligned, a sum at this mean would be off by 2^-53 x (sites of a slice)
// / 4 / 1e-3 relative: 1e-10 at 4000 sites (cfg 3's slices), 1e-9 at 36 000 -- and create_slices plans up to ~137 000 for the
// largest data sets that fit the device (tools/unit_skip_slices.py).  The roundings are not aligned, and the formula is not
// approached: [measured] a pair at 1.2e-3 per site is within 1.9e-14 relative of the full pass's sum with slices of a few
// hundred sites, 1.4e-13 with 32 768, 2e-12 with 262 144 (oracle: 2.6e-14, 1.6e-13, 2e-12); one at 2e-3 3.4e-13 and 3.7e-13
// (profiles/unit_skip/threshold_edges.txt, tests/test_gpu_unit_skip_edges.py) -- fifty times inside 1e-10 at twice the
// longest slice the engine plans, so the rule does not follow the slice length.  Only nearly identical individuals lie
// below this mean.  A data set with such a pair takes the full pass (engine_plans.hip pass_once), whose sums the fix-up rule
// above is written for
#define NGD_FIX_MEAN_UNIT 1e-3
#define NGD_FIX_CAP 4096u  // pairs (or tiles) recomputed per LAUNCH of the fix-up kernels (the size of their scratch)
// The reductions note up to NGD_FIX_LIST pairs (ngd_engine::fix_cap: the capacity of the list) and the pass recomputes
// every one of them (more than the list holds: every pair of the engine, tile by tile).  Its cost in pair-sites of work --
// a pair recomputed alone counts its sites once ([measured] 1.25e10 pair-sites/s: ~400 bytes of 64-byte sectors per
// pair-site), a 16 x 16 tile of pairs recomputed whole counts them NGD_FIX_TILE_COST times (2.9e9 tile-sites/s) however
// many of its 256 pairs are noted -- only matters to a caller that sets a budget (NGD_OPT_FIXUP_WORK; rounds 4-5 had a
// built-in one of 4.1e9, ~0.33 s, beyond which NO noted pair was recomputed: removed in round 6).  A small data set may
// have every pair recomputed: identical called genotypes over a handful of sites are thousands of sums of exactly 0, all
// noted (0 may be a cancelled 1e-20).
#define NGD_FIX_LIST (1u << 20)
#define NGD_FIX_TILE_COST_X10 43u  // (4.3)
struct ngd_fix_flags {     // what the reduction kernels need to note the pairs that want the fix-up
  unsigned long long *list;  // [cap] (i << 32) | j
  uint32_t *count;           // pairs noted (may exceed the capacity: then the fix-up is skipped)
  uint32_t *seen;            // [n_pairs / 32 + 1] one bit per pair, for reductions that visit a pair once per replicate chunk
  uint32_t cap;              // entries the list holds; pairs noted beyond it are counted, not listed
};
// a 16 x 16 tile of pairs (row group ig, column group jg of 16 individuals) that holds noted pairs: bit r * 16 + c of mask
struct ngd_fix_tile {
  uint16_t ig, jg;
  uint32_t n;  // noted pairs in the tile
  unsigned long long mask[4];
};
#define NGD_FIX_TILE_MIN 5u  // a tile with at least this many noted pairs is recomputed whole (k_fixup_tile: it costs what 4.3 single pairs do), the rest pair by pair
// out_mode 0: the partial sums of tile q's 256 pairs over slice sl go to out[(q * n_slices + sl) * 256 ..]; 1: the noted pairs'
// slab entries.  ngd_launch_fixup_tiles_finish: d_sum[pair] = the noted pairs' slices added in ascending order
void ngd_launch_fixup_tiles(hipStream_t st, const ngd_geom &g, const ngd_score &score, const double *T, const double *SM,
                            const uint32_t *d_ws, const ngd_fix_tile *d_tiles, uint32_t n_tiles, uint64_t s_lo, uint64_t s_hi,
                            uint64_t sites_per_slice, uint32_t n_slices, int out_mode, double *out);
void ngd_launch_fixup_tiles_finish(hipStream_t st, const ngd_geom &g, const ngd_fix_tile *d_tiles, uint32_t n_tiles,
                                   const double *parts, uint32_t n_slices, double *d_sum);
// out_mode 0: the partial sum of pair slot q over slice sl goes to out[q * n_slices + sl]; 1: to the slab entry
// out[(sl * n_pad + i) * n_pad + j] (per-block partial results).  Slice sl = sites [s_lo + sl * sites_per_slice, ...) below s_hi.
void ngd_launch_fixup(hipStream_t st, const ngd_geom &g, const ngd_score &score, const double *T, const double *SM,
                      const uint32_t *d_ws, const unsigned long long *d_list, uint32_t n_list, uint64_t s_lo, uint64_t s_hi,
                      uint64_t sites_per_slice, uint32_t n_slices, int out_mode, double *out);
// out_mode 0's second step: d_sum[pair] = the pair's slices added in ascending order
void ngd_launch_fixup_finish(hipStream_t st, const ngd_geom &g, const unsigned long long *d_list, uint32_t n_list,
                             const double *parts, uint32_t n_slices, double *d_sum);

// reduce.hip : deterministic slab reduction + valid-site counting
// planes_per_slice: the slab holds that many result planes per slice (EM batch kernel), `slab` points at
// the first slice's plane of the wanted result
// d_cnt != NULL: every pair's count is set to cnt_value in the same launch (no --pairwise_del)
// fix != NULL (single_image = 2 engines): pairs whose sum is below fix_thr are noted for the fix-up pass
// unit_E != NULL (a pass that left the unit-sum coordinate's k-groups out): pair (i, j) takes
// (unit_c + S) + unit_d0 * 2^-53 * (unit_E[i] + unit_E[j]), S the slab sum -- unit_c = d_0 x the sites the pass visited
void ngd_launch_reduce(hipStream_t st, const ngd_geom &g, const double *slab, uint32_t n_ks,
                       uint32_t planes_per_slice, const ngd_tile *d_tiles, uint32_t n_tiles, double *d_sum,
                       unsigned long long *d_cnt = nullptr, unsigned long long cnt_value = 0,
                       const ngd_fix_flags *fix = nullptr, double fix_thr = 0, const long long *unit_E = nullptr,
                       double unit_c = 0, double unit_d0 = 0);
// --pairwise_del: the pairs of d_sum / d_cnt ([n_rep][n_pairs]) that want the fix-up pass, decided with their valid-site
// counts in hand (a pair with no valid site in a matrix is exactly 0 there and is not noted); fix.count zeroed by the caller
// layout.hip / reduce.hip : the fix-up pass as ONE two-operand pass over scratch images formed a range of k-groups at a time
void ngd_launch_pq_range(hipStream_t st, const ngd_geom &g, const ngd_score &score, const double *T, const double *SM,
                         const uint32_t *d_ws, uint64_t kg_lo, uint64_t kg_end, double *Ps, double *Qs);
void ngd_launch_fix_merge(hipStream_t st, const ngd_geom &g, const double *d_new, double *d_sum, const unsigned long long *d_cnt,
                          double thr, const ngd_tile *d_tiles, uint32_t n_tiles);
void ngd_launch_fix_flag(hipStream_t st, const ngd_geom &g, const double *d_sum, const unsigned long long *d_cnt,
                         uint32_t n_rep, const ngd_tile *d_tiles, uint32_t n_tiles, const ngd_fix_flags &fix,
                         uint32_t mat_stride = 1 /* matrix r of the n_rep is matrix r * mat_stride of d_sum / d_cnt */);
// host_util.cpp: ngd_finish_stream over n_mat matrices, counts per cell (cnt) or one per matrix (cnt_mat)
int ngd_finish_matrices_stream(const double *sum, const uint64_t *cnt, const uint64_t *cnt_mat, uint32_t n_mat, uint64_t n_pairs,
                               uint64_t evol_model, double *dist, const volatile uint64_t *landed);
uint32_t ngd_reduce_chunk(uint32_t n_rep);  // replicates per pass; weight strides are multiples of it
// fix != NULL: a pair is noted if its sum in ANY replicate r is below d_thr[r]
void ngd_launch_reduce_w(hipStream_t st, const ngd_geom &g, const double *slab, uint32_t n_ks, const double *d_W,
                         uint32_t w_stride, uint32_t n_rep, const ngd_tile *d_tiles, uint32_t n_tiles,
                         double *d_sum, const ngd_fix_flags *fix = nullptr, const double *d_thr = nullptr, uint32_t chunk = 0);
void ngd_launch_reduce_c(hipStream_t st, const ngd_geom &g, const uint32_t *C, uint32_t n_blocks, const uint32_t *d_M,
                         uint32_t m_stride, uint32_t n_rep, const ngd_tile *d_tiles, uint32_t n_tiles,
                         unsigned long long *d_cnt, uint32_t chunk = 0);
void ngd_launch_count_blocks(hipStream_t st, const ngd_geom &g, const unsigned long long *mask, uint64_t block_size,
                             uint32_t n_blocks, const ngd_tile *d_tiles16, uint32_t n_tiles16, uint32_t *C,
                             const uint64_t *d_seg = nullptr /* windows: block b = segment b of the slice table */);
// windows along the genome: the banded reduction (k_reduce_band) of per-segment sums (C == NULL) or valid-site counts
// (slab unused) into [n_win][n_pairs]; d_win[2 w] = first | end segment << 32, d_win[2 w + 1] = window length; a sum
// launch also writes the length as the count when d_cnt != NULL and notes pairs for the fix-up when fix != NULL
uint32_t ngd_band_windows();  // windows per group (grid.y)
void ngd_launch_reduce_band(hipStream_t st, const ngd_geom &g, const double *slab, const uint32_t *C,
                            const unsigned long long *d_win, uint32_t n_win, const ngd_tile *d_tiles, uint32_t n_tiles,
                            double *d_sum, unsigned long long *d_cnt, const ngd_fix_flags *fix,
                            uint32_t mat_stride = 1 /* window w's matrix is matrix w * mat_stride of the output */);
// bootstrap replicates inside windows: the banded and weighted reduction (k_reduce_band_w) of per-slice sums (C == NULL) or
// valid-site counts into matrices [w * mat_stride + r][n_pairs], r < n_rep; d_blk[w][0 .. n_blocks] = first slice of each
// block of window w; d_Wt = [n_blocks][w_stride] doubles (sums) or uint32 (counts), w_stride a multiple of
// ngd_reduce_chunk(n_rep) and zero padded.  A sum launch writes cnt_value as every count when d_cnt != NULL and notes the
// pairs whose sum in any matrix is below fix_thr when fix != NULL
void ngd_launch_reduce_band_w(hipStream_t st, const ngd_geom &g, const double *slab, const uint32_t *C, const uint32_t *d_blk,
                              uint32_t n_win, uint32_t n_blocks, const void *d_Wt, uint32_t w_stride, uint32_t n_rep,
                              uint32_t mat_stride, const ngd_tile *d_tiles, uint32_t n_tiles, double *d_sum,
                              unsigned long long *d_cnt, unsigned long long cnt_value, const ngd_fix_flags *fix, double fix_thr);
// ... over windows of unequal length (k_reduce_band_wv): d_desc[w] = the window's NGD_WIN_DESC words (win_plan.h) -- its row
// of d_blk, its n_blocks, its table of d_Wt, the sites a replicate visits: the count a sum launch writes when d_cnt != NULL,
// and x NGD_FIX_MEAN the threshold below which a pair is noted when fix != NULL
void ngd_launch_reduce_band_wv(hipStream_t st, const ngd_geom &g, const double *slab, const uint32_t *C, const uint32_t *d_blk,
                               const uint64_t *d_desc, uint32_t n_win, const void *d_Wt, uint32_t w_stride, uint32_t n_rep,
                               uint32_t mat_stride, const ngd_tile *d_tiles, uint32_t n_tiles, double *d_sum,
                               unsigned long long *d_cnt, const ngd_fix_flags *fix);
void ngd_launch_count(hipStream_t st, const ngd_geom &g, const unsigned long long *mask,
                      const unsigned long long *planes, uint32_t n_planes, const ngd_tile *d_tiles,
                      uint32_t n_tiles, unsigned long long *d_cnt);  // owned 128-tiles
void ngd_launch_fill_cnt(hipStream_t st, const ngd_geom &g, const ngd_tile *d_tiles, uint32_t n_tiles,
                         unsigned long long value, const unsigned long long *d_values, uint32_t n_rep,
                         unsigned long long *d_cnt);

// d = sum / cnt, then the model's transform: ngd_finish's operations in its order (host_util.cpp finish_range), compiled
// without fast-math and with -ffp-contract=off like it -- the division and the products carry the host's bits, log is the
// device's (group_reduce.hip, boot_stats.hip)
#ifdef __HIPCC__
__device__ inline double group_cell(double s, double c, uint32_t model) {
  double d = s / c;
  if (model == 1) d = -log(1 - d);
  else if (model == 2) d = -log(1 - (d * 4 / 3)) * 3 / 4;
  return d;
}
#endif

// boot_stats.hip : per-cell summaries over the n_mat = R + 1 matrices of a set (include/ngsdist_amd.h "Bootstrap summaries")
#define NGD_BOOT_LDS_BYTES 163840u  // the LDS a workgroup may have on gfx950 (160 KiB, the CU's)
#define NGD_BOOT_MIN_TILE 16u       // the narrowest tile of cells: it sets the largest n_mat
#define NGD_BOOT_MAX_MAT (NGD_BOOT_LDS_BYTES / (NGD_BOOT_MIN_TILE * 8u))
// cells per workgroup at n_mat matrices: the widest of 64, 32, 16 whose [n_mat][C] doubles fit (0: none does)
inline uint32_t ngd_boot_tile(uint64_t n_mat) {
  for (uint32_t c = 64; c >= NGD_BOOT_MIN_TILE; c >>= 1)
    if (n_mat * c * 8 <= NGD_BOOT_LDS_BYTES) return c;
  return 0;
}
// [n_set][n_mat][n_cells] sums and counts (d_cnt is not read when tot_sites > 0) or, `values`, the cells' values as they
// are (d_cnt, tot_sites and model unused) -> d_stats [n_set][5][n_cells], d_used [n_set][n_cells].  2 <= n_mat <=
// NGD_BOOT_MAX_MAT and n_set * ceil(n_cells / tile) below 2^31 (grid.x): the caller's to see to.  Returns a hipError_t.
int ngd_launch_boot_stats(hipStream_t st, const double *d_a, const unsigned long long *d_cnt, bool values, uint64_t n_set,
                          uint32_t n_mat, uint64_t n_cells, uint64_t tot_sites, uint32_t model, double p_lo, double p_hi,
                          double *d_stats, unsigned long long *d_used);

// nj.hip : a neighbour-joining tree per matrix (include/ngsdist_amd.h "Neighbour-joining trees"), one workgroup per matrix
#define NGD_NJ_MAX_IND 4096u  // row sums (8 B) and node ids (4 B) per live slot in LDS: 48 KiB at this many
#define NGD_NJ_THREADS 1024u  // the workgroup (DESIGN.md section 6 "Neighbour-joining trees": chosen by measurement)
__host__ __device__ inline uint32_t ngd_nj_ld(uint32_t n_ind) { return (n_ind + 1) & ~1u; }  // doubles per row of the working matrix (even)
// [n_mat][n_pairs] sums and counts (d_cnt is not read when tot_sites > 0) or, `values`, the cells as they are -> d_child /
// d_len [n_mat][2 n_ind - 3], d_status [n_mat]; d_work: n_mat * n_ind * ngd_nj_ld(n_ind) doubles of scratch.  3 <= n_ind <=
// NGD_NJ_MAX_IND, n_mat below 2^31 (grid.x), threads 256, 512 or 1024: the caller's to see to.  Returns a hipError_t.
int ngd_launch_nj(hipStream_t st, const double *d_a, const unsigned long long *d_cnt, bool values, uint64_t n_mat, uint32_t n_ind,
                  uint64_t tot_sites, uint32_t model, uint32_t threads, double *d_work, int32_t *d_child, double *d_len,
                  uint32_t *d_status);

// mds.hip : classical MDS per matrix (include/ngsdist_amd.h "Classical MDS"), one workgroup per matrix
#define NGD_MDS_MAX_IND 4096u  // d, e, v, w (8 B each) per row in LDS: 128 KiB at this many
#define NGD_MDS_MAX_DIM 16u    // K: a wave per vector in the back-transform of a 1024-thread workgroup
#define NGD_MDS_THREADS 1024u  // the workgroup
#define NGD_MDS_AUX_ROWS 4u    // per vector: z and the three rows of U, ngd_nj_ld(n_ind) doubles each
// [n_mat][n_pairs] sums and counts (d_cnt is not read when tot_sites > 0) or, `values`, the cells as they are -> d_eig
// [n_mat][K], d_vec [n_mat][K][n_ind], d_tot [n_mat][2], d_status [n_mat]; scratch: d_work n_mat * n_ind * ngd_nj_ld(n_ind)
// doubles, d_aux n_mat * NGD_MDS_AUX_ROWS * K * ngd_nj_ld(n_ind).  3 <= n_ind <= NGD_MDS_MAX_IND, 1 <= K <= min(n_ind - 1,
// NGD_MDS_MAX_DIM), n_mat below 2^31 (grid.x), threads 256, 512 or 1024: the caller's to see to.  Returns a hipError_t.
int ngd_launch_mds(hipStream_t st, const double *d_a, const unsigned long long *d_cnt, bool values, uint64_t n_mat, uint32_t n_ind,
                   uint64_t tot_sites, uint32_t model, uint32_t K, uint32_t threads, double *d_work, double *d_aux, double *d_eig,
                   double *d_vec, double *d_tot, uint32_t *d_status);

// mds_align.hip : a set's MDS replicates rotated onto its matrix 0 (include/ngsdist_amd.h "Classical MDS", alignment)
#define NGD_MDS_ALIGN_THREADS 256u  // the workgroup (DESIGN.md section 3 "Alignment of the replicates")
// a chunk's d_eig / d_vec / d_status as ngd_launch_mds wrote them -> d_cells [n_mat][K (n_ind + 1)]: per matrix the
// coordinates [K][n_ind], then its K eigenvalues; d_status_out [n_mat].  Limits as ngd_launch_mds'.  Returns a hipError_t.
int ngd_launch_mds_coords(hipStream_t st, const double *d_eig, const double *d_vec, const uint32_t *d_status, uint64_t n_mat,
                          uint32_t n_ind, uint32_t K, double *d_cells, uint32_t *d_status_out);
// d_cells [n_set][n_mat] matrices `stride` doubles apart, each [K][n_ind] coordinates and whatever follows them: every
// replicate's coordinates rotated in place, d_fit [n_set][n_mat]; d_status [n_set][n_mat] or NULL (every matrix has status
// 1): a matrix left out has all its `stride` doubles and its fit NaN.  n_set * n_mat below 2^31 (grid.x), stride >= K *
// n_ind: the caller's to see to.  Returns a hipError_t.
int ngd_launch_mds_align(hipStream_t st, double *d_cells, uint64_t stride, const uint32_t *d_status, uint64_t n_set, uint32_t n_mat,
                         uint32_t n_ind, uint32_t K, double *d_fit);

// win_cmp.hip : comparison of windows (include/ngsdist_amd.h "Comparison of windows"): means, status and the centred Gram
// matrix of n_vec vectors of n_cells cells each
// (the geometry -- NGD_WIN_CMP_MAX_VEC, the tile block, Z's vector groups, the slice rule: win_cmp_geom.h)
// doubles of the resident operand Z (fragment-major: k-groups of 4 cells x ngd_wincmp_groups(n_vec) groups of 16 vectors, +
// the run-ahead k-group) and of the partials [slice][group][group][256]; both known from (n_vec, n_cells)
uint64_t ngd_wincmp_z_doubles(uint64_t n_vec, uint64_t n_cells);
uint64_t ngd_wincmp_part_doubles(uint64_t n_vec, uint64_t n_cells);
// [n_vec][n_cells] sums and counts (d_cnt is not read when tot_sites > 0) or, `values`, the cells as they are: the launch's
// vector v is vector w0 + v of the call -> d_mean / d_status [w0 + v]; then x - mean into Z, which the caller has zeroed
// once (n_vec_call: the vectors of the whole call, which sets Z's geometry).  n_cells >= 1, n_vec_call <=
// NGD_WIN_CMP_MAX_VEC: the caller's to see to.  Each returns a hipError_t.
int ngd_launch_wincmp_stats(hipStream_t st, const double *d_a, const unsigned long long *d_cnt, bool values, uint64_t n_vec,
                            uint64_t n_cells, uint64_t tot_sites, uint32_t model, uint64_t w0, double *d_mean, uint32_t *d_status);
int ngd_launch_wincmp_pack(hipStream_t st, const double *d_a, const unsigned long long *d_cnt, bool values, uint64_t n_vec,
                           uint64_t n_cells, uint64_t tot_sites, uint32_t model, uint64_t w0, uint64_t n_vec_call, const double *d_mean,
                           const uint32_t *d_status, double *Z);
// Z -> the partials of every (slice, tile on or above the diagonal); then gram [n_vec][n_vec] from them and d_status
int ngd_launch_wincmp_gram(hipStream_t st, const double *Z, uint64_t n_vec, uint64_t n_cells, double *part);
int ngd_launch_wincmp_sum(hipStream_t st, const double *part, uint64_t n_vec, uint64_t n_cells, const uint32_t *d_status, double *gram);

// group_reduce.hip : group-mean distance matrices (ngd_set_groups, ngd_group_means_device, ngd_run_*_groups)
// One work item: rows [r0, r1) of group pair (a, b) -- positions in group a's member list --, every column of group b
#define NGD_GROUP_WG_CELLS 4096  // cells of a work item's rectangle, about: whole rows, at least one
struct ngd_group_work {
  uint32_t a, b, r0, r1;
};
// a grouping on the device: members sorted by group and ascending inside one, goff[g] .. goff[g + 1] the members of group g,
// the work items sorted by group pair, gp_first[gp] .. gp_first[gp + 1] those of group pair gp (none: no cell)
struct ngd_group_launch {
  uint64_t n_ind;
  const uint32_t *members, *goff;
  const ngd_group_work *work;
  const uint32_t *gp_first;
  uint32_t n_work, n_gp;
};
// [n_mat][n_pairs] sums and counts -> mean / used [n_mat][n_gp]; part_sum / part_cnt: n_mat * n_work entries of scratch;
// n_mat * max(n_work, n_gp / 256 + 1) below 2^31 (grid.x).  tot_sites > 0: d_cnt is not read
void ngd_launch_group_means(hipStream_t st, const ngd_group_launch &l, const double *d_sum, const unsigned long long *d_cnt,
                            uint64_t n_mat, uint64_t tot_sites, uint32_t model, double *part_sum, unsigned long long *part_cnt,
                            double *mean, unsigned long long *used);
