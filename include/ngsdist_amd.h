/*
 * ngsdist_amd.h -- C ABI of the MI355X pairwise-distance engine.
 *
 * This is the drop-in boundary for the ONE hot path of fgvieira/ngsDist: the
 * per-replicate fan-out of gen_dist() over all pairs of individuals.  The
 * reference has no FFI layer; the seam is the task `void gen_dist_slave(void*)`
 * handed to threadpool_add() (reference ngsDist.cpp:251, task type
 * threadpool.h:71-74) around `double gen_dist(params*, uint64_t, uint64_t)`
 * (ngsDist.hpp:55-56).  Each entry point below names the reference lines it
 * stands in for.  INTEGRATION.md shows the patch a maintainer of the
 * reference would apply to call it.
 *
 * Conventions
 *  - plain C, no C++/torch/HIP types in any signature; device pointers and
 *    streams travel as void*;
 *  - every function returns NGD_OK (0) or a negative NGD_E_* code and leaves a
 *    message retrievable with ngd_last_error(); nothing calls exit();
 *  - the caller owns every host buffer; the engine owns every device buffer
 *    and keeps no host pointer after a call returns;
 *  - calls on one engine are not thread-safe (one caller, like main()).
 *  - pair order is the reference's: row-major upper triangle, i1 < i2
 *    (ngsDist.cpp:244-245); n_pairs = n_ind*(n_ind-1)/2.
 *  - results are deterministic run to run (no floating-point atomics): the same calls in the same order on a new engine
 *    give the same bits.  Two calls of the same bootstrap job on ONE engine may take different plans (NGD_OPT_BOOT_PARTIALS
 *    = 1 serves the first calls of a geometry without the per-block partial results while their slab would cost more to
 *    allocate than it has saved) and then agree to rounding, not bit for bit; 0 or 2 pin the plan.
 *  - there is no CPU fallback: without a HIP device ngd_create() fails.
 */
#ifndef NGSDIST_AMD_H
#define NGSDIST_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NGD_ABI_VERSION 6 /* 6: ngd_run_job_dist, ngd_run_batch_dist, ngd_run_mult_batch_dist (and, added under 6: ngd_run_windows*, ngd_last_windows, ngd_window_ranges, ngd_run_windows_job / _job_device / _job_dist; NGD_OPT_EM_EXACT / _EM_EXACT_CAP, ngd_last_em_exact, ngd_em_exact_entries, ngd_em2_site; ngd_set_groups, ngd_group_means_device, ngd_run_job_groups, ngd_run_windows_groups, ngd_run_windows_job_var_groups, ngd_last_groups_ms, ngd_n_group_pairs, ngd_group_pair_index, ngd_group_cells); 5: ngd_finish_stream, ngd_fixup_info.by_pass, NGD_OPT_STAGE_PIECE_MIB / _STAGE_RING / _EAGER_FULL, NGD_OPT_FIXUP_WORK 0 = no budget (every noted pair is recomputed); 4: ngd_last_spill_timing, ngd_last_fixup, ngd_image_mode, ngd_config.single_image 0 = auto / 3 = two images; 3: ngd_config.single_image / second_image_mib (were reserved, zero), ngd_fetch_matrix, ngd_score_congruence */

#define NGD_OK 0
#define NGD_E_INVALID (-1)  /* bad argument / bad state                    */
#define NGD_E_NODEVICE (-2) /* no usable HIP device                        */
#define NGD_E_HIP (-3)      /* a HIP runtime call failed                   */
#define NGD_E_NOMEM (-4)    /* host or device allocation failed            */
#define NGD_E_MODEL (-5)    /* evolutionary model 3..6 (reference: error())*/
#define NGD_E_NAN (-6)      /* "NaN found! Is the file format correct?" (read_data.cpp:42-45) */

/* which kernel serves the per-pair accumulation */
#define NGD_KERNEL_AUTO 0   /* indep: MFMA (the streaming kernel where the MFMA kernel's 8 slab planes of n_pad^2 doubles  */
                            /* cannot fit the device: tens of thousands of individuals); EM: the table kernel above 32     */
                            /* individuals, the fast per-pair kernel up to 32                                              */
#define NGD_KERNEL_STREAM 1 /* indep: one wavefront per pair, streams 48 B per pair-site */
#define NGD_KERNEL_MFMA 2   /* indep: FP64 MFMA tiles over the (pair, site) contraction */
#define NGD_KERNEL_EM_FAITHFUL 3 /* EM: iterates bit-identical to emOptim2.cpp */
#define NGD_KERNEL_EM_FAST 4     /* EM: division-free power iteration, same stopping rule */
#define NGD_KERNEL_EM_TABLE 5    /* EM: the fast form with per-individual tables shared by a 64x64 tile of pairs */

typedef struct ngd_engine ngd_engine;

/* The subset of the reference's `params` (ngsDist.hpp:11-44) that gen_dist()
 * reads, plus placement. */
typedef struct ngd_config {
  uint64_t n_ind;       /* params.n_ind; bounded by device memory (NGD_E_NOMEM: two n_pairs-long result arrays +  */
                        /* n_pad^2 doubles per slice), never above 1 048 448 (16-bit tile indices)          */
  uint64_t n_sites;     /* params.n_sites of the loaded data set              */
  double score[9];      /* params.score[g1][g2] row-major, parse_args.cpp:25-27,134-137 */
  int32_t pairwise_del; /* params.pairwise_del, ngsDist.cpp:335-338           */
  int32_t indep_geno;   /* params.indep_geno, ngsDist.cpp:348-353             */
  int32_t device;       /* HIP device ordinal; -1 = current device            */
  int32_t kernel;       /* NGD_KERNEL_*                                       */
  uint32_t shard_rank;  /* this engine computes the pair tiles that            */
  uint32_t shard_world; /*   ngd_shard_of_pair() gives it; 0/1 = everything   */
  /* Launch geometry; 0 = the measured defaults, which is what a host wants.  They change
   * speed only, never results beyond the order of additions over site slices. */
  uint32_t variant;      /* NGD_KERNEL_EM_TABLE: workgroup shape 0..4 (accum_em_table.hip)            */
  uint32_t n_slices;     /* slices of the site axis per launch (MFMA: rounded up to a multiple of 8);  */
                         /* held to what the data set allows (>= 128 k-groups / >= 1 site per slice)  */
  uint32_t wg_target;    /* workgroups wanted per launch, from which n_slices is derived when it is 0 */
  uint32_t exact_shapes; /* NGD_KERNEL_MFMA, block form: issue only the MFMA tiles a block of pairs needs (narrow edge    */
                         /* blocks, triangular diagonal blocks).  0 = auto: off above 384 padded individuals, else up to  */
                         /* 208 individuals form 6, up to 256 form 4, else form 2.  1 = never (full 4 x 4 pattern);       */
                         /* 7 = the full pattern, four blocks to a workgroup, except that the blocks ON the diagonal leave */
                         /* out the six tiles below it and sit in workgroups of their own (a one-image engine fetches     */
                         /* their four operand fragments once for rows and columns).  Fewer MFMAs, no faster: such blocks */
                         /* run ahead of their slice and its operands then leave HBM more than once; */
                         /* 2 = blocks of up to 4 x 4 tiles of 16 x 16 pairs, one single-wavefront workgroup per block;   */
                         /* 3 = the same with blocks of up to 2 x 4; 4 / 5 = 2 / 3 with a slice's blocks in ONE workgroup */
                         /* that moves through the sites in step (<= 12 / <= 16 blocks; a prefetching wavefront where one */
                         /* fits); 6 = 5 with the operands staged through LDS.  Fallbacks, all silent and result-         */
                         /* neutral: 4 -> 2 and 5 / 6 -> 3 where a slice's blocks do not fit one workgroup; 6 -> 5 for    */
                         /* any pass that carries per-index weights -- bootstrap passes, masked partial-sum slices and    */
                         /* EVERY pass of a single_image = 2 engine (its plain pass is weighted by the congruence)        */
  uint32_t single_image; /* NGD_KERNEL_MFMA: how many operand images the engine holds.  Two (p and q = score . p,           */
                         /* ngsDist.cpp:351-353 regrouped) are 48 bytes per (padded individual, site); ONE is 24, i.e.    */
                         /* up to twice the sites per engine and half the HBM reads per pass:                              */
                         /* 2 = ONE image in coordinates in which the (symmetric) score matrix is diagonal, score = SUM_r  */
                         /*     d_r c_r c_r^T: the image holds t_r = c_r . p, both operands are read from it, d rides on   */
                         /*     the per-index weights.  The speed of two images.  The squares differ in sign: sums are     */
                         /*     exact for called genotypes (c, d dyadic for the reference's matrices) and otherwise carry  */
                         /*     an ABSOLUTE error of <= 4e-17 per site -- 1e-9 relative wherever a pair's mean per-site    */
                         /*     term is above 4e-8.  For the reference's two matrices (parse_args.cpp:25-27, :134-137) the */
                         /*     pairs below that -- nearly identical individuals -- are then RECOMPUTED with the two-operand */
                         /*     arithmetic (the fix-up pass: every pair whose sum is below 1e-6 x the sites visited -- under */
                         /*     --pairwise_del x the pair's own valid sites, and never a pair without one; it needs         */
                         /*     min(p0, p2) beside the image, 8 more bytes per individual and site: 32 in all), so 1e-9    */
                         /*     relative holds at any distance, unconditionally: every qualifying pair is recomputed,      */
                         /*     however many there are (clusters of copies tile by tile, 60 times cheaper than pair by     */
                         /*     pair; where the tiles would cost more than the whole matrix in the two-image arithmetic --  */
                         /*     a data set of clones -- one more pass over scratch images formed a range of sites at a time */
                         /*     does it: ~70 ms at 1000 x 1e6 whatever the data; replicates from per-block partial results  */
                         /*     go tile by tile at any count, up to ~0.8 s at that size).  ngd_last_fixup() reports what a  */
                         /*     run recomputed.  Only a caller that SETS a                                                  */
                         /*     budget (NGD_OPT_FIXUP_WORK) can have pairs left at the absolute bound.                     */
                         /*     Any other symmetric matrix: no fix-up.  NGD_E_INVALID for an asymmetric matrix.            */
                         /* 1 = p resident, q formed for a range of sites at a time before the launch that reads it: the   */
                         /*     arithmetic of two images (sums equal to rounding, per-block partial sums bit for bit), any  */
                         /*     score matrix, a fifth more time (55.6 ms at 1000 x 1e6 instead of 45.6)                    */
                         /* 3 = two images, always                                                                         */
                         /* 0 = auto: 2 where its fix-up pass exists (the reference's matrices) and the kernel runs its     */
                         /*     full 4 x 4 block form (exact_shapes resolves to 0: more than 384 padded individuals, or    */
                         /*     exact_shapes = 1 / 7 asked for -- the block forms of a few hundred individuals take no     */
                         /*     per-index weights in their fastest variant), else two images.  ngd_image_mode() tells what */
                         /*     an engine holds.                                                                           */
  uint32_t second_image_mib; /* single_image = 1: MiB of q kept resident all the same, from the first site on      */
                         /* (what the device has to spare): only the rest is formed range by range, and the extra */
                         /* time shrinks in proportion                                                             */
} ngd_config;

/* Per-run device timings (HIP events on the engine's stream). */
typedef struct ngd_timing {
  double ms_total;      /* first launch of the run -> results ready           */
  double ms_accum;      /* the dominant accumulation kernel alone             */
  double ms_reduce;     /* split-site slab reduction                          */
  double ms_count;      /* valid-site counting (pairwise deletion only)       */
  uint64_t pair_sites;  /* (pairs this engine owns) x (sites visited)         */
  uint64_t launches;    /* accumulation kernel launches in the run            */
} ngd_timing;

const char *ngd_last_error(void);
int ngd_abi_version(void);
/* number of visible HIP devices (0 if none); never fails */
int ngd_device_count(void);

/* Engine lifetime.  Stands in for the thread pool + pth_struct array set up in
 * ngsDist.cpp:197-208 and torn down in :291-306. */
int ngd_create(const ngd_config *cfg, ngd_engine **out);
void ngd_destroy(ngd_engine *e);

/* Input: the prepared, NORMAL-space array gen_dist() reads (params.geno_lkl
 * after ngsDist.cpp:165-174).  Two host layouts are accepted:
 *   ngd_upload_sites     p[(s*n_ind + i)*3 + g], sites s0 .. s0+n-1 -- the
 *                        order of the binary file (read_data.cpp:28-31), so a
 *                        host can stream a file through in chunks;
 *   ngd_upload_ind_major p[(i*n_sites + s)*3 + g] -- the reference's in-memory
 *                        order in_geno_lkl[i][s][g], whole data set at once.
 * ngd_commit() ends the upload (derives the per-individual missing-site masks
 * of gen_func.cpp:862-868 and the score-weighted operand).  After commit the
 * data set is immutable; bootstrap never moves data (see ngd_run). */
int ngd_upload_sites(ngd_engine *e, const double *p, uint64_t s0, uint64_t n);
int ngd_upload_ind_major(ngd_engine *e, const double *p);
int ngd_commit(ngd_engine *e);

/* Raw input: the doubles of a BINARY GL file exactly as stored (read_data.cpp:28-31,
 * [site][individual][3]); the engine performs the reference's kernel-input construction
 * on the device -- log unless in_logscale, normalisation (post_prob), the NaN check of
 * read_data.cpp:37-45, then call_geno and exp of ngsDist.cpp:165-174 -- instead of the
 * host.  Device log/exp agree with glibc's to the last ulp or so: use the host path
 * (ngd_upload_sites) where called genotypes must be decided bit-for-bit as on the CPU.
 *
 * Zero-copy pipeline: ngd_stage_acquire() lends one of the engine's pinned host buffers
 * (*capacity_sites sites of n_ind*3 doubles; a ring of NGD_OPT_STAGE_RING buffers of
 * NGD_OPT_STAGE_PIECE_MIB MiB); the caller reads the file straight into it and calls
 * ngd_stage_submit(), which returns at once: the copy runs on a copy stream of its own, the
 * preparation kernel behind it on the engine's stream, and the next acquire hands out the
 * next buffer of the ring (waiting only for the copy out of THAT buffer, a turn ago).  ngd_upload_raw_sites() is the blocking
 * convenience form.  NGD_E_NAN is reported by ngd_commit() at the latest.
 *
 * Upload contract (every path above: ngd_upload_sites, ngd_upload_ind_major, ngd_upload_raw_sites, ngd_stage_*):
 *   - before a successful ngd_commit(), sites may be written any number of times, by any of the paths, in any order;
 *   - each site holds the last values written to it, whether it is missing (--pairwise_del) included;
 *   - after ngd_commit() has returned NGD_E_NAN the engine accepts a fresh upload (then ngd_commit() again);
 *   - a site that is never written holds unspecified values: writing every site is the caller's responsibility (the
 *     engine does not track it). */
typedef struct ngd_prep {
  int32_t in_logscale; /* --log_scale                           */
  int32_t call_geno;   /* --call_geno (or -N / -C)              */
  double N_thresh;     /* --N_thresh                            */
  double call_thresh;  /* --call_thresh                         */
} ngd_prep;
int ngd_stage_acquire(ngd_engine *e, double **host_buf, uint64_t *capacity_sites);
int ngd_stage_submit(ngd_engine *e, uint64_t s0, uint64_t n, const ngd_prep *prep);
int ngd_upload_raw_sites(ngd_engine *e, const double *raw, uint64_t s0, uint64_t n, const ngd_prep *prep);

/* Test/bench input: fills the engine with this repository's counter-based
 * synthetic data set (bit-identical to oracle ngo_synth_one) on
 * the device, then commits.  Not part of the reference's surface. */
int ngd_synth_fill(ngd_engine *e, uint64_t seed, double miss_frac);
/* Same generator, but the engine's site 0 is site `site0` of the synthetic data set: an engine
 * that holds one contiguous range of sites (site sharding, below). */
int ngd_synth_fill_range(ngd_engine *e, uint64_t seed, double miss_frac, uint64_t site0);

/* One replicate = everything between rnd_map_data() and the matrix print:
 * the `for i1<i2: threadpool_add(gen_dist_slave)` + threadpool_wait block,
 * ngsDist.cpp:244-269, with gen_dist()'s loop :333-364.
 *   block_map == NULL : the full data set (rep 0), n_blocks/block_size ignored;
 *   else                block_map[b] (b < n_blocks) is the source block that
 *                       rnd_map_data (ngsDist.cpp:416-437) puts at block b,
 *                       i.e. floor(draw_rnd(0, n_blocks)); sites at or beyond
 *                       n_blocks*block_size are not visited (:236).
 * Outputs (host, caller-owned, n_pairs entries each, either may be NULL):
 *   sum[k] : gen_dist()'s `dist` before ngsDist.cpp:376;
 *   cnt[k] : gen_dist()'s `cnt` before the tot_sites override (:372-373).
 * Pairs outside this engine's shard are returned as 0 / 0. */
int ngd_run(ngd_engine *e, const uint64_t *block_map, uint64_t n_blocks,
            uint64_t block_size, double *sum, uint64_t *cnt);

/* Same, but results stay on the device: d_sum (double[n_pairs]) and d_cnt
 * (uint64_t[n_pairs]) are DEVICE pointers owned by the caller (e.g. the
 * storage of a torch tensor used for the RCCL gather).  Returns after the
 * engine's stream has finished. */
int ngd_run_device(ngd_engine *e, const uint64_t *block_map, uint64_t n_blocks,
                   uint64_t block_size, void *d_sum, void *d_cnt);

/* Site sharding.  gen_dist()'s sum and cnt are sums over sites, so a data set can also be split
 * along the SITE axis: every engine (GPU) holds a contiguous range of sites of all individuals,
 * computes all pairs over its range, and the per-engine (sum, cnt) are ADDED (one RCCL
 * reduce; exact for called genotypes, <= 1e-12 relative otherwise -- the addition order differs
 * from one engine's).  For a bootstrap replicate an engine needs the multiplicity of each of ITS
 * blocks, which is not a block map of its own: ngd_run_mult() takes the multiplicities directly
 * (mult[b] = number of draws of the engine's block b; ranges must be whole blocks).  cnt is then
 * block_size * SUM mult[b] (or the multiplicity-weighted valid-site count with --pairwise_del). */
int ngd_run_mult(ngd_engine *e, const uint32_t *mult, uint64_t n_blocks, uint64_t block_size,
                 double *sum, uint64_t *cnt);
int ngd_run_mult_device(ngd_engine *e, const uint32_t *mult, uint64_t n_blocks,
                        uint64_t block_size, void *d_sum, void *d_cnt);

/* n_rep bootstrap replicates in ONE call: n_rep turns of the replicate loop ngsDist.cpp:217-289 (each
 * = rnd_map_data :416-437 + the fan-out/wait :244-269).  block_maps is [n_rep][n_blocks], replicate r's
 * map being what the r-th rnd_map_data() call would draw (the taus stream is consumed by nothing else,
 * so a host may draw all maps up front: ngd_boot_block_map n_rep times); mult is [n_rep][n_blocks]
 * (site sharding, as ngd_run_mult).  Outputs are [n_rep][n_pairs].  The engine computes per-block partial
 * (sum, cnt) once and forms up to 32 replicates per pass over them, so a batch costs little more than
 * one replicate; a replicate's result is the same whether it came from a batch or from ngd_run().
 * When the partials do not apply (streaming kernel, not enough device memory for one partial result per
 * block -- e.g. block size 1 on a large data set) this is n_rep weighted accumulation passes on the
 * --indep_geno path (each walks only the sites its replicate drew).  On the EM path the term of a (pair, site)
 * does not depend on the replicate, so the matrices share the per-site EM: the table-driven kernel (from three
 * matrices on, NGD_OPT_EM_SPILL) writes the terms of a chunk of sites once and ONE FP64 MFMA contraction with
 * every matrix's weights adds the chunk to all of them -- one EM pass whatever the replicate count; matrices then
 * agree with their own ngd_run() pass to rounding (<= 1e-12 relative), counts exactly.  Otherwise (option off, two
 * matrices, the per-pair kernels) one pass serves 8 matrices (table-driven kernel) or 16 (per-pair kernels), each
 * accumulator taking the term with the site's weight in its matrix: same bits as from ngd_run() in the table-driven
 * kernel's default variant and in the per-pair kernels; its other variants (1..4) borrow the per-pair batch kernel
 * and agree with their own ngd_run() to rounding only. */
int ngd_run_batch(ngd_engine *e, const uint64_t *block_maps, uint32_t n_rep, uint64_t n_blocks,
                  uint64_t block_size, double *sum, uint64_t *cnt);
int ngd_run_batch_device(ngd_engine *e, const uint64_t *block_maps, uint32_t n_rep, uint64_t n_blocks,
                         uint64_t block_size, void *d_sum, void *d_cnt);
int ngd_run_mult_batch(ngd_engine *e, const uint32_t *mult, uint32_t n_rep, uint64_t n_blocks,
                       uint64_t block_size, double *sum, uint64_t *cnt);
int ngd_run_mult_batch_device(ngd_engine *e, const uint32_t *mult, uint32_t n_rep, uint64_t n_blocks,
                              uint64_t block_size, void *d_sum, void *d_cnt);

/* The WHOLE replicate loop ngsDist.cpp:217-289 in one call: matrix 0 is the full data set (what
 * ngd_run(e, NULL, ...) returns), matrices 1..n_rep the bootstrap replicates of block_maps
 * ([n_rep][n_blocks], drawn as for ngd_run_batch).  Outputs are [n_rep + 1][n_pairs].  Knowing the whole
 * job lets the engine share work between the matrices: when the blocks cover every site the full-data
 * matrix is the all-ones combination of the same per-block partials as the replicates; on the EM path
 * (no --indep_geno) with blocks too small for partials -- e.g. the default --boot_block_size 1 -- up to 16
 * matrices, the full-data one included, share ONE pass of the per-site EM, which does not depend on the
 * replicate.  Replicates carry the same bits as from ngd_run() (to rounding where ngd_run_batch says so: the
 * spilled-terms plan of the table-driven EM kernel); matrix 0 agrees with ngd_run(e, NULL) to rounding (exactly for
 * called genotypes) because its sum may be formed in a different order.
 * n_rep = 0 is ngd_run(e, NULL, ...). */
int ngd_run_job(ngd_engine *e, const uint64_t *block_maps, uint32_t n_rep, uint64_t n_blocks,
                uint64_t block_size, double *sum, uint64_t *cnt);
int ngd_run_job_device(ngd_engine *e, const uint64_t *block_maps, uint32_t n_rep, uint64_t n_blocks,
                       uint64_t block_size, void *d_sum, void *d_cnt);
/* ngd_run_batch / ngd_run_mult_batch / ngd_run_job with sum = cnt = NULL leave their matrices in the engine; this copies
 * matrix `which` of that last call (0 = the first it computed) to the caller -- a host that prints the matrices one after
 * the other (ngsDist.cpp:282-287) then needs two n_pairs-long buffers, not (n_boot_rep + 1) of them.  Valid until the
 * engine's next run call. */
int ngd_fetch_matrix(ngd_engine *e, uint32_t which, double *sum, uint64_t *cnt);
/* A job AND the tail of gen_dist() (ngsDist.cpp:217-289 with :372-401) in one call: `dist` ([n_rep + 1][n_pairs] for
 * ngd_run_job_dist -- [1][n_pairs] when n_rep = 0 --, [n_rep][n_pairs] for ngd_run_batch_dist / ngd_run_mult_batch_dist; any host memory)
 * receives what ngd_run_job() / ngd_run_batch() / ngd_run_mult_batch() followed by ngd_finish() on every matrix would give, bit
 * for bit.
 * The sums (and, --pairwise_del, the counts) leave the device in chunks of about 8 MiB on a stream of the engine's own into
 * pinned memory the engine keeps, and up to 64 host threads turn each chunk into distances as it lands; in the
 * per-block-partials plan a group of 32 replicates is reduced by a launch of its own and its copy follows at once, beside
 * the reductions of the later groups.  The matrices stay in the engine as after sum = cnt = NULL (ngd_fetch_matrix).
 * tot_sites and evol_model as for ngd_finish() (tot_sites > 0: the count of every cell, --tot_sites, ngsDist.cpp:372-373;
 * NGD_E_INVALID with --pairwise_del, parse_args.cpp:209-210).  NGD_E_MODEL for evol_model > 2 before anything is launched;
 * NGD_E_INVALID on an engine that owns a share of the pairs (ngd_config.shard_world > 1: its matrices are partial). */
int ngd_run_job_dist(ngd_engine *e, const uint64_t *block_maps, uint32_t n_rep, uint64_t n_blocks, uint64_t block_size,
                     uint64_t tot_sites, uint64_t evol_model, double *dist);
int ngd_run_batch_dist(ngd_engine *e, const uint64_t *block_maps, uint32_t n_rep, uint64_t n_blocks, uint64_t block_size,
                       uint64_t tot_sites, uint64_t evol_model, double *dist); /* replicates only, as ngd_run_batch */
int ngd_run_mult_batch_dist(ngd_engine *e, const uint32_t *mult, uint32_t n_rep, uint64_t n_blocks, uint64_t block_size,
                            uint64_t tot_sites, uint64_t evol_model, double *dist);

/* Bootstrap replicates re-use per-block partial (sum, cnt) computed on the first
 * run that carries a block map (valid for that block size / block count;
 * recomputed automatically when either changes).  This forgets them, so that a
 * benchmark can charge the partial-sum pass to every timed step. */
int ngd_drop_caches(ngd_engine *e);

/* Plan selection for the replicate loop, per engine and changeable between runs (defaults in brackets).  The engine
 * picks the cheapest plan that applies by itself; these exist to pin one for a comparison or to bound memory.
 * Every plan returns the same counts and sums equal to rounding ("Plans"). */
#define NGD_OPT_BOOT_PARTIALS 1  /* [1] bootstrap replicates from per-block partial (sum, cnt): 0 never, 1 when they */
                                 /*     fit and pay for their allocation, 2 allocate even a large slab at once       */
#define NGD_OPT_BOOT_MAX_BYTES 2 /* [0 = 85 % of free device memory] budget of those partials (and, when set, of the     */
                                 /*     EM batch pass's result planes: beyond it, one pass per matrix)                */
#define NGD_OPT_BOOT_WG 3        /* [4096] workgroups wanted in the pass that fills them                             */
#define NGD_OPT_BOOT_UNALIGNED 4 /* [1] MFMA path: partials also for block sizes that are not multiples of 4 sites   */
#define NGD_OPT_EM_BATCH 5       /* [1] EM kernels without partials: up to 16 (per-pair) / 8 (table-driven) matrices  */
                                 /*     per accumulation pass                                                         */
#define NGD_OPT_EM_SPILL 6       /* [1] table-driven EM kernel without partials, 3 matrices or more: ONE pass writes   */
                                 /*     the per-(pair, site) terms of a chunk of sites, one FP64 MFMA contraction with  */
                                 /*     the matrices' weights adds the chunk to every matrix (any replicate count);     */
                                 /*     0 never, 1 from 3 matrices on, 2 from 2 on.  Matrices then agree with their own */
                                 /*     ngd_run() pass to rounding (<= 1e-12 relative), not bit for bit                 */
#define NGD_OPT_EM_SPILL_BYTES 7 /* [0 = 6 GB] device scratch for those terms (bounds the sites per chunk)             */
#define NGD_OPT_SINGLE_IMAGE_BYTES 8 /* [0 = 4 GB] ngd_config.single_image engines: bytes of the second operand image */
                                 /*     formed at a time (a pass is so many launches; never less than 64 k-groups per */
                                 /*     slice, or eight bootstrap blocks of a partial-sum pass); set before the first run */
#define NGD_OPT_FIXUP_WORK 9     /* [0 = no budget: every noted pair is recomputed] one-image engines, the fix-up pass of    */
                                 /* nearly identical pairs: a budget in pair-sites of recomputation (a pair alone counts its   */
                                 /* sites once, a 16 x 16 tile of pairs recomputed whole 4.3 times; ~1.2e10 a second).  A run   */
                                 /* whose noted pairs cost more keeps the one-image sums of ALL of them (absolute error <=     */
                                 /* 4e-17 per site instead of 1e-9 relative) and says so in ngd_last_fixup().skipped           */
#define NGD_OPT_STAGE_PIECE_MIB 10 /* [32] ngd_stage_acquire: MiB of raw input per pinned buffer                        */
#define NGD_OPT_STAGE_RING 11     /* [6] ... and how many of them (2 .. 8); both before the first ngd_stage_acquire    */
#define NGD_OPT_EAGER_FULL 12     /* [0] 1: a staged load (ngd_stage_*) of sites in ascending order starts the plain         */
                                 /* full-data pass beside itself: leading slices of the site axis are accumulated, on a       */
                                 /* low-priority stream, as soon as all their sites are prepared; the first ngd_run() with    */
                                 /* no block map launches only what is left.  Same bits as without it.  For a host whose     */
                                 /* first call after ngd_commit IS that pass (no bootstrap): anything else drops the work.    */
                                 /* MFMA kernel above 384 padded individuals and the table-driven EM kernel; else ignored.    */
#define NGD_OPT_WIN_PLAN 13       /* [0] ngd_run_windows*: 0 auto (the cheaper plan by estimate), 1 one weighted pass per       */
                                 /*     window only, 2 the segment-slab plan only (NGD_E_NOMEM if a window cannot fit it).     */
                                 /*     Engines with the segment-slab plan: the MFMA kernel with both operand images resident  */
                                 /*     or the one congruent image, and NGD_KERNEL_EM_TABLE (what auto picks above 32          */
                                 /*     individuals without indep_geno) with any ngd_config.variant.  On every other engine    */
                                 /*     (one image + ranges of the second, NGD_KERNEL_EM_FAST / _EM_FAITHFUL / _STREAM) 0 and  */
                                 /*     1 take the per-window plan and 2 is refused (NGD_E_INVALID)                            */
#define NGD_OPT_WIN_MAX_BYTES 14  /* [0 = 85 % of free device memory, the rule of NGD_OPT_BOOT_MAX_BYTES] budget of one batch   */
                                 /*     of the segment-slab plan: its partial results and counts, + the MFMA kernel's slice    */
                                 /*     weights.  An EM engine's batch is 8 n_pad^2 bytes per slice (+ 4 n_pad^2 per slice     */
                                 /*     under pairwise_del), n_pad = n_ind rounded up to 128                                   */
#define NGD_OPT_EM_EXACT 15       /* [0] 1: the plain full-data pass of the table-driven EM kernel (ngd_run with no block map)  */
                                 /*     stops every (pair, site) at the REFERENCE's step.  The kernels decide the stopping rule */
                                 /*     fabs(lik - oldLik) < 0.001 (emOptim2.cpp:127) from ratios of power sums; within rounding */
                                 /*     of the tolerance they may stop one EM step from the reference, which changes that site's */
                                 /*     term by tens of percent.  With the option the pass notes every stop whose criterion is   */
                                 /*     within 2^-36 (relative) of the threshold, the host reruns those sites the reference's   */
                                 /*     way (ngd_em2_site) and the pair's sum takes c_ref - c_dev before it leaves the engine.    */
                                 /*     Pairs without a noted site carry the bits of the option-off pass; results are           */
                                 /*     reproducible run to run.  ngd_last_em_exact() / ngd_em_exact_entries() report the pass. */
                                 /*     kernel = auto then means NGD_KERNEL_EM_TABLE at any number of individuals (an engine of */
                                 /*     32 or fewer stays on it when the option goes back to 0).  NGD_E_INVALID on an           */
                                 /*     --indep_geno engine, for an explicit kernel other than NGD_KERNEL_EM_TABLE, and         */
                                 /*     together with NGD_OPT_EAGER_FULL (either refuses the other).                            */
                                 /*     While it is 1, ngd_run* with a block map or multiplicities, the batch, job and windowed */
                                 /*     calls return NGD_E_INVALID before anything is launched            */
                                 /*     2: everything 1 means, and ngd_run* with a block map or multiplicities, the batch and    */
                                 /*     the job calls (_device / _dist forms included) are served: the list of in-band (pair,    */
                                 /*     site)s does not depend on the replicate, so the plan's one EM launch notes it (per-block */
                                 /*     partials, else the spilled-terms pass in its noting form) and matrix r takes its         */
                                 /*     multiplicity of the site's block times (c_ref - c_dev), in site order, before any sum    */
                                 /*     leaves the engine.  ngd_last_em_exact() / ngd_em_exact_entries() then report the call:  */
                                 /*     each noted (pair, site) once.  A call neither plan can serve (ngd_config.variant != 0 or */
                                 /*     NGD_OPT_EM_SPILL = 0 where partials do not apply) fails with NGD_E_INVALID and computes  */
                                 /*     nothing; the windowed calls stay refused, unless NGD_OPT_EM_EXACT_WIN lets them through. */
                                 /*     Values above 2: NGD_E_INVALID                                                            */
#define NGD_OPT_EM_EXACT_CAP 16   /* [0 = 2^20] entries the list of noted (pair, site)s holds, 32 bytes each.  A pass that notes */
                                 /*     more is counted in full, the list grows to the count and the pass runs ONCE more        */
#define NGD_OPT_UNIT_SKIP 17      /* [1] one-image engines in congruent coordinates on the reference's matrices, no              */
                                 /*     --pairwise_del: the plain full-data pass (ngd_run with no block map; the lead matrix    */
                                 /*     of a job whose blocks do not cover every site) leaves out the k-groups of the           */
                                 /*     coordinate p0 + p1 + p2 -- 1 for normalised input: a third of the pass multiplies ones  */
                                 /*     by ones -- and adds their products as a constant per pair, n / 2 plus an exact          */
                                 /*     per-individual correction ngd_commit derives.  Only for a data set ngd_commit found to  */
                                 /*     be *unit* (every such sum finite and within 2^-40 of 1); else, and with 0, the pass     */
                                 /*     visits every k-group.  The two agree to ~1e-14 relative, not bit for bit.  The          */
                                 /*     skipping pass carries 2^-53 of n / 2 per rounding: if it finds a pair whose mean        */
                                 /*     per-site term is below 1e-3 (nearly identical individuals) its sums are dropped, the    */
                                 /*     pass runs whole, and so does every later one on this data set.                          */
#define NGD_OPT_EM_EXACT_WIN 18   /* [0] 1: while NGD_OPT_EM_EXACT is 1 or 2 the windowed calls are served instead of refused,   */
                                 /*     every window at the reference's stopping steps; it does nothing while NGD_OPT_EM_EXACT   */
                                 /*     is 0, and with 0 every call does what NGD_OPT_EM_EXACT alone says.  The segment-slab     */
                                 /*     plan's one accumulation pass per batch notes (the slice-table form of the noting kernel), */
                                 /*     the host rechecks the list behind the banded reductions, and every matrix of every window */
                                 /*     of the batch takes its weight of the site -- 1 inside the window; a replicate: the        */
                                 /*     multiplicity of block (site - lo) / block_size, 0 in the tail -- times (c_ref - c_dev),   */
                                 /*     in site order, before any sum leaves the engine (_device, host and _dist forms alike).    */
                                 /*     ngd_last_em_exact() / ngd_em_exact_entries() report the call: the union over batches and  */
                                 /*     passes, each (pair, site) once; passes the maximum, ms the sum.                           */
                                 /*     NGD_OPT_EM_EXACT = 1: ngd_run_windows* by the segment-slab plan only -- NGD_OPT_WIN_PLAN   */
                                 /*     = 1 fails with NGD_E_INVALID, a window beyond NGD_OPT_WIN_MAX_BYTES with NGD_E_NOMEM,      */
                                 /*     nothing computed; ngd_run_windows_job* stay refused (replicates need value 2).            */
                                 /*     NGD_OPT_EM_EXACT = 2: both plans and the jobs; the per-window plan goes window by window  */
                                 /*     through the noting plans of value 2 and fails as they do where none applies.              */
                                 /*     NGD_E_INVALID for values above 1, and for 1 on the engines that refuse NGD_OPT_EM_EXACT   */
                                 /*     (--indep_geno, an explicit kernel other than NGD_KERNEL_EM_TABLE)                         */
#define NGD_OPT_NJ_MAX_BYTES 19    /* [0 = 2 GB] device scratch of the neighbour-joining kernel (ngd_nj_*, ngd_run_*_nj): a full n x n */
                                 /*     matrix of doubles (rows padded to an even length) per matrix of a launch; never fewer    */
                                 /*     than one matrix.  Any value gives the same bits                                          */
#define NGD_OPT_MDS_MAX_BYTES 20   /* [0 = 2 GB] device scratch of the classical-MDS kernel (ngd_mds_*, ngd_run_*_mds): per matrix of a */
                                 /*     launch a full n x n matrix of doubles (rows padded to an even length) and 4 K rows     */
                                 /*     more; never fewer than one matrix.  Any value gives the same bits                        */
#define NGD_OPT_WIN_CMP_MAX_BYTES 21 /* [0 = half of the free device memory at the call] device memory of the comparison of       */
                                 /*     windows (ngd_win_cmp_*, ngd_run_windows_cmp): the operand and the partial sums, resident  */
                                 /*     for the whole call.  A call that needs more is refused with NGD_E_INVALID.                */
#define NGD_OPT_DEBUG_FORGE_JOB 100 /* tests only: the first block of the MFMA kernel's job list gets the shape rows | cols << 3 |  */
                                 /*     tri << 6 -- a shape the kernel's block form does not list must fail the run with      */
                                 /*     NGD_E_HIP (its sums poisoned with NaN), never return zeros                            */
                                 /*     Refused (NGD_E_INVALID) unless the environment has NGD_ENABLE_TEST_HOOKS=1: the       */
                                 /*     engine's job list stays forged, every later run of it fails                           */
int ngd_set_option(ngd_engine *e, int option, uint64_t value);

int ngd_last_timing(const ngd_engine *e, ngd_timing *t);
/* k-groups (four contraction indices each) the last plain full-data pass of an MFMA engine visited: all of the image's, or
 * two thirds of them where NGD_OPT_UNIT_SKIP applied; 0 for the other kernels. */
int ngd_last_plain_pass(const ngd_engine *e, uint64_t *kgroups);
/* What the engine holds (ngd_config.single_image resolved): 3 = two operand images, 1 = one image + the second formed a
 * range at a time, 2 = one image in congruent coordinates; 0 = not an MFMA engine.  *fixup (may be NULL) = 1 if the
 * engine recomputes the pairs its congruent arithmetic cannot hold to 1e-9 relative (the reference's score matrices). */
int ngd_image_mode(const ngd_engine *e, int *fixup);
/* The fix-up pass of the last run call (single_image = 2 engines on the reference's matrices; zeros otherwise): pairs
 * whose sum in a matrix of the job was below 1e-6 x the sites the matrix visits, how many were recomputed with the
 * two-operand arithmetic of ngsDist.cpp:351-353 (all of the engine's pairs when more than 2^20 were noted at once), how
 * many were left as the one-image pass computed them (never, unless the caller set a budget with NGD_OPT_FIXUP_WORK and
 * the work exceeded it: absolute error <= 4e-17 per site), and the device time of the recomputation. */
typedef struct ngd_fixup_info {
  uint64_t flagged, recomputed, skipped;
  double ms;
  uint64_t by_pass; /* recomputations that went the whole-matrix way: so many noted pairs that ONE more pass in the    */
                    /* two-image arithmetic over scratch images (a pass and a half: ~70 ms at 1000 x 1e6) was cheaper  */
                    /* than their tiles -- a data set of clones; the noted pairs take its sums, the others keep theirs */
                    /* (a bootstrap job's per-block partial results, blocks of whole k-groups: EVERY entry of the slab  */
                    /* is formed again that way, all pairs take the two-image engine's bits)                           */
} ngd_fixup_info;
int ngd_last_fixup(const ngd_engine *e, ngd_fixup_info *info);
/* The accumulation phase of the last run that took the spilled-terms plan (EM path, bootstrap blocks too small for
 * per-block partials: NGD_OPT_EM_SPILL), kernel by kernel, HIP events on the engine's stream summed over the job's chunks
 * of sites -- for roofline accounting (bench.py --workload emboot).  All zero if the last run took another plan. */
typedef struct ngd_spill_timing {
  double ms_weights;          /* k_spill_weights + the memsets of a chunk's partial last k-group                     */
  double ms_terms;            /* k_accum_em_table<SPILL>: the per-site EM (emOptim2.cpp:112-135), terms written       */
  double ms_sanitize;         /* k_spill_sanitize (a no-op unless a term was not finite)                             */
  double ms_contract;         /* k_contract_mfma: running sums += weights x terms                                    */
  uint64_t chunks;            /* chunks of sites the job went through (NGD_OPT_EM_SPILL_BYTES)                       */
  uint64_t sites;             /* sites visited                                                                       */
  uint64_t unit_sites;        /* q: consecutive sites of one bootstrap block whose terms leave the EM kernel as one   */
  uint64_t units;             /* K of the contraction = terms written and read per pair slot                         */
  uint64_t slot_groups;       /* groups of 16 pair slots (N of the contraction / 16), padding included               */
  uint64_t slot_groups_live;  /* ... of them written by the EM pass (hold at least one pair)                         */
  uint64_t matrices;          /* matrices of the job                                                                 */
  uint64_t matrix_groups;     /* groups of 16 matrices (M of the contraction / 16)                                   */
  uint64_t contract_launches; /* k_contract_mfma launches (one per chunk and 128 matrices)                           */
} ngd_spill_timing;
int ngd_last_spill_timing(const ngd_engine *e, ngd_spill_timing *t);
/* The shader clock (MHz) the last MFMA / table-driven EM accumulation launch ran at: one wavefront in the middle of
 * the grid reads the shader-cycle counter and the constant-rate counter around its work.  0 = not sampled (other
 * kernels).  For roofline accounting: a kernel's rate against the peak AT THE CLOCK THE CHIP HELD. */
int ngd_last_shader_clock(const ngd_engine *e, double *mhz);
/* Work done by the table-driven EM kernel (NGD_KERNEL_EM_TABLE) in the last run, for roofline accounting: the number
 * of (64 x 64 pair tile, site) visits and of table rounds (16 EM steps of a tile's 128 individuals each) -- the
 * data-dependent part of its operation count (the EM's iteration count, emOptim2.cpp:118-133).  Zero for other kernels. */
int ngd_last_em_work(const ngd_engine *e, uint64_t *tile_sites, uint64_t *table_rounds);

/* NGD_OPT_EM_EXACT: the recheck of the last plain pass, or of the last call served under value 2 (zeros when the option was off) */
typedef struct ngd_em_exact_info {
  uint64_t noted;   /* (pair, site)s whose stop was within 2^-36 of the tolerance                                   */
  uint64_t changed; /* ... of them, those the reference stops at another step than the device did                   */
  uint64_t passes;  /* accumulation passes: 1, or 2 when the list had to grow                                       */
  double ms;        /* gather + host recheck + patch, wall clock                                                    */
} ngd_em_exact_info;
int ngd_last_em_exact(const ngd_engine *e, ngd_em_exact_info *info);
/* ... and its entries, sorted by (i1, i2, site): the step and term of the device, the step and term of the reference's
 * em2() on the same six likelihoods.  Returns the number of entries of the last pass (or a negative NGD_E_* code) and
 * writes the first min(count, cap) of them if out is not NULL. */
typedef struct ngd_em_exact_entry {
  uint32_t i1, i2;
  uint64_t site;
  uint32_t t_dev, t_ref;
  double c_dev, c_ref;
} ngd_em_exact_entry;
int64_t ngd_em_exact_entries(const ngd_engine *e, ngd_em_exact_entry *out, uint64_t cap);
/* One site of the reference's default mode, ngsDist.cpp:340-349: em2() of emOptim2.cpp:112-135 (with emStep2, normalize
 * and lik2) over the 3 x 3 sfs, tolerance 0.001, at most 50 steps, in the reference's order of operations and with the
 * host's log().  sfs is read as the start (the reference fills it with 1/9) and receives the result; *n_iter (may be
 * NULL) the number of EM steps taken.  Pure host arithmetic: callable without a device. */
void ngd_em2_site(const double gl1[3], const double gl2[3], double sfs[9], int *n_iter);

/* Windows along the genome: one matrix per window [lo, hi) of the engine's sites, each exactly what ngd_run() gives on a
 * data set that holds only those sites (gen_dist() over an input cut down to the window; --pairwise_del counts, called
 * genotypes and the EM path alike).  win_lo / win_hi: n_win engine-local ranges, lo < hi <= n_sites, lo non-decreasing;
 * windows may overlap and nest.  NGD_E_INVALID for anything else, and on an engine that owns a share of the pairs.
 * Outputs are [n_win][n_pairs] with the meaning of ngd_run() (host memory; ..._device: device pointers of the caller's).
 * Two plans (NGD_OPT_WIN_PLAN):
 *  - segment slab (MFMA kernel, engines with both operands resident or the one congruent image; the table-driven EM
 *    kernel NGD_KERNEL_EM_TABLE, every workgroup shape of ngd_config.variant): the elementary
 *    intervals between consecutive window boundaries are the slices of ONE accumulation pass into per-segment partial
 *    results, then a banded reduction adds each window's segments, in ascending order, for a group of consecutive windows
 *    per read of their segments; --pairwise_del counts the same way from per-segment popcounts.  Calls whose segments do
 *    not fit the budget (NGD_OPT_WIN_MAX_BYTES) go in batches of consecutive windows; a segment two batches share is
 *    computed in both.  One-image engines (single_image = 2) then recompute with the two-operand arithmetic the pairs
 *    whose sum in some window is below 1e-6 x the window's length (x the pair's count under --pairwise_del).  On an EM
 *    engine a long interval is cut into several slices (as many workgroups as a plain pass), the per-site EM term is
 *    the same in every window that holds the site, and a term that is not finite (an all-zero individual) reaches
 *    exactly those windows; sums agree with the per-window plan's to rounding (<= 1e-12 relative);
 *  - per window (every other kernel, or when cheaper): one weighted pass per window over that window's sites (the pass
 *    ngd_run_mult() makes with 0/1 multiplicities).
 * Sums agree with the cut-down data set's ngd_run() to rounding (<= 1e-9 relative), counts exactly. */
int ngd_run_windows(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win, double *sum,
                    uint64_t *cnt);
int ngd_run_windows_device(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win, void *d_sum,
                           void *d_cnt);
/* ... and the tail of gen_dist() on every window (as ngd_finish() with tot_sites / evol_model: the host's libm, as
 * ngd_run_job_dist): dist is [n_win][n_pairs] host memory.  NGD_E_MODEL for evol_model > 2 before anything is launched. */
int ngd_run_windows_dist(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win, uint64_t tot_sites,
                         uint64_t evol_model, double *dist);
/* Bootstrap replicates INSIDE every window: for each window exactly what the reference prints when run on a file cut down to
 * the window's sites with --n_boot_rep n_rep --boot_block_size block_size (the replicate loop ngsDist.cpp:217-289, the
 * truncation :236, rnd_map_data :416-437).  The windows of a call have ONE length W (NGD_E_INVALID otherwise): every cut-down
 * run seeds the generator anew, so all of them draw the same n_rep block maps, block_maps [n_rep][n_blocks] with
 * n_blocks = W / block_size rounded down (ngd_boot_block_map from a fresh state, n_rep times).  Outputs are
 * [n_win][n_rep + 1][n_pairs]: matrix 0 of a window is its full-data matrix (ngd_run_windows), matrix r visits the sites
 * [lo + m q, lo + (m + 1) q), m = block_maps[r - 1][b], once for each b; the tail [lo + n_blocks q, hi) is matrix 0's alone.  A
 * replicate's count is n_blocks * block_size, under --pairwise_del the multiplicity-weighted number of valid sites, exactly.
 * n_rep = 0 is ngd_run_windows*, bit for bit (block_maps, n_blocks, block_size are then not read).
 * NGD_E_INVALID: anything ngd_run_windows refuses (an engine that owns a share of the pairs included), windows of unequal
 * length, block_size 0, n_blocks != W / block_size, a map entry >= n_blocks, null maps -- and W < block_size (no block: the
 * "empty bootstrap geometry" ngd_run_job refuses on an engine of W sites; a host prints the replicates of such a window as
 * 0 / 0 itself, ngsDist.cpp:236).
 * The plans are those of ngd_run_windows (NGD_OPT_WIN_PLAN, NGD_OPT_WIN_MAX_BYTES; 2 returns NGD_E_INVALID / NGD_E_NOMEM alike):
 *  - unit slab (where the segment slab applies): the block boundaries lo + b q and the ends hi of a batch of windows cut
 *    the sites into the slices of ONE accumulation pass for ALL replicates of all windows -- where block_size divides the
 *    windows' step a block is one slice and overlapping windows share all of them, else a block is a few slices --; a
 *    window's replicates are the banded and weighted reduction of its slices (32 replicates per read of them), counts under
 *    --pairwise_del the same in integers.  Matrix 0 of every window is computed by the segment-slab plan of
 *    ngd_run_windows_device() on the same list of windows, from the windows' own segments, and carries its bits (finer
 *    slices would add the same terms in another order): one more pass over the covered sites and one banded reduction.  A non-finite partial result (an all-zero individual on the EM path)
 *    reaches exactly the matrices that visit its sites.  One-image engines recompute the noted pairs' entries of the slab with
 *    the two-operand arithmetic and reduce again: 1e-9 relative at any distance in every matrix (ngd_last_fixup,
 *    ngd_windows_info.fixup_pairs); matrix 0 is fixed as ngd_run_windows fixes it;
 *  - per window (every other engine; windows that do not fit the budget; where cheaper by estimate -- block size 1):
 *    ngd_run_mult_batch()'s plans on multiplicity vectors over blocks of B = gcd(lo, block_size, hi) sites (hi too, so that
 *    the window's end is a block boundary for matrix 0), one call per window.  The vectors count blocks from the engine's
 *    site 0: the host builds (n_rep + 1) x hi / B uint32 entries per window -- at block size 1 and a window near site 1e6
 *    with 100 replicates 400 MB, built anew for every window; a plan for a few windows or coarse blocks.
 * Sums of the two plans, and of the cut-down data set's ngd_run_job(), agree to rounding (<= 1e-12 relative; <= 1e-9 against
 * the reference's order of additions), counts exactly.  ngd_last_windows() tells which plan ran. */
int ngd_run_windows_job(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win, const uint64_t *block_maps,
                        uint32_t n_rep, uint64_t n_blocks, uint64_t block_size, double *sum, uint64_t *cnt);
int ngd_run_windows_job_device(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win,
                               const uint64_t *block_maps, uint32_t n_rep, uint64_t n_blocks, uint64_t block_size, void *d_sum,
                               void *d_cnt);
/* ... and the tail of gen_dist() on every matrix (as ngd_run_windows_dist): dist is [n_win][n_rep + 1][n_pairs] host memory;
 * the windows go through the engine's batch buffers in groups of at least one.  NGD_E_MODEL for evol_model > 2 and
 * NGD_E_INVALID for tot_sites with --pairwise_del, both before anything is launched. */
int ngd_run_windows_job_dist(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win,
                             const uint64_t *block_maps, uint32_t n_rep, uint64_t n_blocks, uint64_t block_size,
                             uint64_t tot_sites, uint64_t evol_model, double *dist);
/* The same over windows of UNEQUAL length (windows in coordinates, ngd_window_ranges_bp): the meaning of ngd_run_windows_job*
 * window by window, with n_blocks_w = (hi_w - lo_w) / block_size rounded down.  Window w's maps are [n_rep][n_blocks_w] at
 * block_maps + map_off[w] (ngd_window_boot_maps draws them as the cut-down runs would; windows may share an offset), maps_len
 * the entries of block_maps.  Outputs are [n_win][n_rep + 1][n_pairs]: matrix 0 of a window is its ngd_run_windows matrix,
 * matrix r visits blocks block_maps[map_off[w] + (r - 1) n_blocks_w + b]; a replicate's count is n_blocks_w * block_size,
 * under --pairwise_del the multiplicity-weighted number of valid sites, exactly.  A window shorter than one block
 * (n_blocks_w = 0) has replicates with sum 0 and count 0 -- what the reference's truncation (ngsDist.cpp:236) leaves; the
 * _dist form prints ngd_finish's 0 / 0 there.  n_rep = 0 is ngd_run_windows*, bit for bit.
 * NGD_E_INVALID, before anything is launched: anything ngd_run_windows refuses, block_size 0, a null table,
 * map_off[w] + n_rep n_blocks_w > maps_len, a map entry >= n_blocks_w; and while NGD_OPT_EM_EXACT is on (either value, with
 * or without NGD_OPT_EM_EXACT_WIN) the call is refused in the words of every other call that option does not serve.
 * The plans are those of ngd_run_windows_job (NGD_OPT_WIN_PLAN, NGD_OPT_WIN_MAX_BYTES):
 *  - unit slab: as there -- the block boundaries lo_w + b q and the ends hi_w of a batch cut the sites into the slices of
 *    ONE accumulation pass, matrix 0 comes from the plain segment slab with ngd_run_windows_device()'s bits -- and the
 *    replicates from the descriptor form of the banded and weighted reduction: every workgroup first reads four words of
 *    its window (where its row of block starts begins, n_blocks_w, where its weight table begins, the sites a replicate
 *    visits), so the count and the fix-up threshold are the window's own.  Windows that share map_off and n_blocks_w share
 *    a weight table; a batch holds the tables of its own classes only.  The slices of a batch are cut by the boundaries of
 *    every window of the call inside its span, so the MFMA kernel's replicates carry the same bits under any
 *    NGD_OPT_WIN_MAX_BYTES (matrix 0 is ngd_run_windows_device()'s at the same budget);
 *  - per window: one ngd_run_windows_job of one window each, with that window's maps.
 * Windows of one length through this call give ngd_run_windows_job*'s bits in both plans. */
int ngd_run_windows_job_var(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win,
                            const uint64_t *block_maps, uint64_t maps_len, const uint64_t *map_off, uint32_t n_rep,
                            uint64_t block_size, double *sum, uint64_t *cnt);
int ngd_run_windows_job_var_device(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win,
                                   const uint64_t *block_maps, uint64_t maps_len, const uint64_t *map_off, uint32_t n_rep,
                                   uint64_t block_size, void *d_sum, void *d_cnt);
int ngd_run_windows_job_var_dist(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win,
                                 const uint64_t *block_maps, uint64_t maps_len, const uint64_t *map_off, uint32_t n_rep,
                                 uint64_t block_size, uint64_t tot_sites, uint64_t evol_model, double *dist);
/* What the last ngd_run_windows* call did */
typedef struct ngd_windows_info {
  uint64_t segments;       /* slices of the segment-slab plan's accumulation passes, summed over its batches          */
  uint64_t slab_bytes;     /* bytes of the largest batch's per-segment partial results (sums + counts)               */
  uint64_t batches;        /* batches of the segment-slab plan                                                        */
  uint64_t band_launches;  /* banded-reduction launches (sums and counts)                                             */
  uint64_t windows_by_pass;/* windows served by a weighted pass of their own (the per-window plan)                    */
  uint64_t fixup_pairs;    /* pairs the one-image fix-up recomputed, summed over the windows it recomputed them in    */
  double ms;               /* device time of the call (HIP events on the engine's stream)                             */
} ngd_windows_info;
int ngd_last_windows(const ngd_engine *e, ngd_windows_info *info);
/* The window list of --win_size / --win_step (pure host arithmetic): sites [0, n_sites) split into chromosomes --
 * maximal runs of equal chrom_id (chrom_id == NULL: one sequence); in each chromosome starting at c0 the windows
 * [c0 + k step, c0 + k step + size) that fit inside it, k = 0, 1, ...  Returns the number of windows and, if lo / hi are
 * not NULL, writes the first min(count, cap) of them; NGD_E_INVALID for size or step 0 and for a chromosome id that
 * shows up again after another one (a positions file not grouped by chromosome). */
int64_t ngd_window_ranges(const uint32_t *chrom_id, uint64_t n_sites, uint64_t size, uint64_t step, uint64_t *lo, uint64_t *hi,
                          uint64_t cap);
/* The window list of --win_bp / --win_bp_step (pure host arithmetic): chromosomes as above; in a chromosome whose sites have
 * positions p_0 <= ... <= p_{m-1}, all >= 1, window k = 0, 1, ... covers the coordinates [1 + k step_bp, 1 + k step_bp +
 * size_bp) for every k with 1 + k step_bp <= p_{m-1} (trailing partial windows are kept: the chromosome's length is not
 * known).  Its sites are those whose position lies in the interval, a range [lo, hi); a window with fewer than
 * max(1, min_sites) sites is left out and the kept ones are numbered in output order, so that lo does not decrease and
 * lo < hi, as ngd_run_windows* wants.  bp_start (may be NULL) receives 1 + k step_bp of each kept window.  Returns the
 * count and writes the first min(count, cap) windows.  NGD_E_INVALID: size_bp or step_bp 0, pos == NULL, a position of 0, a
 * position or size >= 2^62, positions that descend inside a chromosome (equal ones are allowed), a chromosome id that shows
 * up again after another one.  Time is proportional to sites + kept windows: runs of windows that cannot be kept are
 * jumped over. */
int64_t ngd_window_ranges_bp(const uint32_t *chrom_id, const uint64_t *pos, uint64_t n_sites, uint64_t size_bp, uint64_t step_bp,
                             uint64_t min_sites, uint64_t *lo, uint64_t *hi, uint64_t *bp_start, uint64_t cap);
/* The block maps ngd_run_windows_job_var* takes, drawn as the reference would on every window's cut-down file: each such
 * run seeds its generator anew, so a window of L sites draws its n_rep maps of n_blocks = L / block_size blocks from a
 * fresh ngd_taus_seed(seed) (ngd_boot_block_map, n_rep times) -- a sequence that depends on n_blocks alone: windows with
 * one n_blocks, those of one length among them, share one set of maps and one offset.  Window w's maps are
 * [n_rep][n_blocks_w] at block_maps + map_off[w]; a window shorter than one block has no entries (map_off[w] = 0).
 * Returns the number of entries needed and writes map_off[0 .. n_win); nothing is written beyond block_maps[cap)
 * (block_maps may be NULL with cap 0).  NGD_E_INVALID: block_size 0, a null lo / hi / map_off, hi < lo. */
int64_t ngd_window_boot_maps(uint64_t seed, const uint64_t *lo, const uint64_t *hi, uint64_t n_win, uint32_t n_rep,
                             uint64_t block_size, uint64_t *block_maps, uint64_t cap, uint64_t *map_off);

/* Group-mean distance matrices, reduced on the device: per matrix the G x G table of mean distances within and between
 * groups of individuals (populations) instead of the n x n matrix -- n_gp = G (G + 1) / 2 numbers cross the host link.
 * A grouping is group_of[i] for every individual: a value in [0, n_groups) names its group, -1 leaves it out of every
 * group.  Group pairs (a, b), a <= b, are numbered as the row-major upper triangle with the diagonal:
 * gp = a G - a (a - 1) / 2 + (b - a).  The cells of (a, b) are the pairs i1 < i2 with one individual in a and the other in
 * b, whichever has the lower index (a == b: both in a).  A cell's value d is ngd_finish()'s, operation by operation, from
 * the matrix's (sum, cnt) and (tot_sites, evol_model); the division and the products carry the host's bits (no fast-math),
 * log is the device's.  used[m][gp] = the cells whose d is finite, mean[m][gp] = their sum / used, a positive quiet NaN
 * where used is 0 (a group of one on the diagonal, an empty group, no shared valid site under --pairwise_del): cells that
 * are not finite are left out and counted, cells - used of them (ngd_group_cells).  No floating-point atomics: the order
 * of additions is a function of (n_ind, group_of) alone -- not of the matrices a call or a launch holds. */
uint64_t ngd_n_group_pairs(uint32_t n_groups);
uint64_t ngd_group_pair_index(uint32_t n_groups, uint32_t a, uint32_t b); /* a <= b */
/* cells[n_gp]: the cells of every group pair.  Pure host arithmetic, needs no device.  NGD_E_INVALID: a null argument,
 * n_groups 0, an entry of group_of outside [-1, n_groups). */
int ngd_group_cells(const int32_t *group_of, uint64_t n_ind, uint32_t n_groups, uint64_t *cells);
/* The engine's grouping (group_of: n_ind entries): the member lists, their offsets and the launch's work list go to device
 * memory of the engine's.  NULL / 0 clears it and frees that memory.  NGD_E_INVALID: an entry outside
 * [-1, n_groups), n_groups 0 with a list, a list with n_groups 0; a refused call leaves the grouping as it was. */
int ngd_set_groups(ngd_engine *e, const int32_t *group_of, uint32_t n_groups);
/* mean / used [n_mat][n_gp] (host memory; used may be NULL) of any [n_mat][n_pairs] matrices in device memory -- the
 * caller's, as a *_device call wrote them; whatever wrote them has finished.  d_cnt is not read when tot_sites > 0.
 * NGD_E_INVALID, before anything is launched: no grouping set, a null pointer, n_mat 0, tot_sites with --pairwise_del, an
 * engine that owns a share of the pairs; NGD_E_MODEL for evol_model > 2.  A failed call leaves grouping and engine usable. */
int ngd_group_means_device(ngd_engine *e, const void *d_sum, const void *d_cnt, uint64_t n_mat, uint64_t tot_sites,
                           uint64_t evol_model, double *mean, uint64_t *used);
/* ngd_run_job_device / ngd_run_windows_device / ngd_run_windows_job_var_device into the engine's batch buffers (the windows
 * in groups of ~2 GB of results) followed by that reduction: plans, fix-up, NGD_OPT_EM_EXACT* and refusals are the sibling's,
 * and the means are ngd_group_means_device()'s on the sibling's output bit for bit at the same options.  Outputs:
 * [n_rep + 1][n_gp], [n_win][n_gp], [n_win][n_rep + 1][n_gp].  Windows of one length go through the _var form (whose bits
 * are ngd_run_windows_job*'s).  The refusals of ngd_group_means_device come first, before anything is launched. */
int ngd_run_job_groups(ngd_engine *e, const uint64_t *block_maps, uint32_t n_rep, uint64_t n_blocks, uint64_t block_size,
                       uint64_t tot_sites, uint64_t evol_model, double *mean, uint64_t *used);
int ngd_run_windows_groups(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win, uint64_t tot_sites,
                           uint64_t evol_model, double *mean, uint64_t *used);
int ngd_run_windows_job_var_groups(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win,
                                   const uint64_t *block_maps, uint64_t maps_len, const uint64_t *map_off, uint32_t n_rep,
                                   uint64_t block_size, uint64_t tot_sites, uint64_t evol_model, double *mean, uint64_t *used);
/* device time (HIP events) of the group reduction's kernels in the last of these calls, summed over its launches */
int ngd_last_groups_ms(const ngd_engine *e, double *ms);

/* Bootstrap summaries per cell, reduced on the device (added under ABI 6): per cell of a set an estimate, a standard
 * error and a percentile interval leave the device instead of R + 1 sums and counts.
 * A *set* is one window's (or the whole run's) n_mat = R + 1 matrices over n_cells cells -- n_pairs pairs, or n_gp group
 * pairs.  A cell's values are v_0 .. v_R; F = the replicates r >= 1 with v_r finite, m = |F|, s_(0) <= .. <= s_(m-1)
 * those values sorted by numeric value (ties in any order).  Per cell:
 *   stat 0  est   v_0, whatever it is (nan / inf pass through)
 *   stat 1  mean  (SUM_{r in F} v_r) / m, the terms added one by one in ascending r starting from 0.0; a positive quiet
 *                 NaN if m = 0
 *   stat 2  sd    sqrt(SUM_{r in F} (v_r - mean)^2 / (m - 1)), same order, no contraction; a positive quiet NaN if m < 2
 *   stat 3  lo    s_(k_lo), k_lo = floor(p_lo * (double)(m - 1)); NaN if m = 0
 *   stat 4  hi    s_(k_hi), k_hi = ceil(p_hi * (double)(m - 1)); NaN if m = 0
 *           used  m
 * p_lo = (1 - ci) / 2 and p_hi = 1 - p_lo are computed once on the host in double from the caller's ci in (0, 1).  Order
 * statistics, not interpolation: lo and hi are values the engine computed.  Replicates that are not finite are left out
 * and counted, as the group means leave cells out; a window shorter than one block has replicates 0 / 0 and so m = 0.
 * From sums and counts a cell's value is ngd_finish()'s, operation by operation (the division and the products carry the
 * host's bits, log is the device's).  Outputs, in host memory: stats[n_set][NGD_BOOT_NSTAT][n_cells] doubles and
 * used[n_set][n_cells].  A cell's bits depend on its own values alone, never on the launch or the set it shares a call with.
 * The device keeps a cell's n_mat values in on-chip memory: R <= ngd_boot_stats_max_rep(), more is refused. */
#define NGD_BOOT_NSTAT 5
uint32_t ngd_boot_stats_max_rep(void);
/* The definitions above in plain host arithmetic on val[n_set][n_mat][n_cells], for callers of the *_dist forms; needs no
 * device, any n_mat >= 2.  NGD_E_INVALID: a null pointer, n_set 0, n_mat < 2, ci outside (0, 1). */
int ngd_boot_stats_host(const double *val, uint64_t n_set, uint64_t n_mat, uint64_t n_cells, double ci, double *stats,
                        uint64_t *used);
/* ... on the device, of [n_set][n_mat][n_pairs] sums and counts in device memory -- the caller's, as a *_device call wrote
 * them (d_cnt is not read when tot_sites > 0) --, or of [n_set][n_mat][n_cells] values as they are.  NGD_E_INVALID, before
 * anything is launched: a null pointer, n_set 0, n_mat < 2, ci outside (0, 1) (NaN included), n_mat - 1 above
 * ngd_boot_stats_max_rep(), tot_sites with --pairwise_del, an engine that owns a share of the pairs; NGD_E_MODEL for
 * evol_model > 2.  A refused call leaves outputs and engine as they were. */
int ngd_boot_stats_device(ngd_engine *e, const void *d_sum, const void *d_cnt, uint64_t n_set, uint64_t n_mat, uint64_t tot_sites,
                          uint64_t evol_model, double ci, double *stats, uint64_t *used);
int ngd_boot_stats_values_device(ngd_engine *e, const void *d_val, uint64_t n_set, uint64_t n_mat, uint64_t n_cells, double ci,
                                 double *stats, uint64_t *used);
/* ngd_run_job_device (one set) / ngd_run_windows_job_var_device (one set per window; windows of one length go through it
 * too) into the engine's batch buffers, followed by that reduction: plans, fix-up, NGD_OPT_EM_EXACT* and refusals are the
 * sibling's, and the statistics are ngd_boot_stats_device()'s on the sibling's output bit for bit at the same options.
 * The _groups forms run the group reduction first and summarise the n_gp means of every matrix while they are still in
 * device memory (NGD_E_INVALID without a grouping).  n_rep 0 is refused.  Outputs: stats [5][n_cells] / [n_win][5][n_cells],
 * used [n_cells] / [n_win][n_cells], n_cells = n_pairs or n_gp. */
int ngd_run_job_stats(ngd_engine *e, const uint64_t *block_maps, uint32_t n_rep, uint64_t n_blocks, uint64_t block_size,
                      uint64_t tot_sites, uint64_t evol_model, double ci, double *stats, uint64_t *used);
int ngd_run_windows_job_var_stats(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win,
                                  const uint64_t *block_maps, uint64_t maps_len, const uint64_t *map_off, uint32_t n_rep,
                                  uint64_t block_size, uint64_t tot_sites, uint64_t evol_model, double ci, double *stats,
                                  uint64_t *used);
int ngd_run_job_groups_stats(ngd_engine *e, const uint64_t *block_maps, uint32_t n_rep, uint64_t n_blocks, uint64_t block_size,
                             uint64_t tot_sites, uint64_t evol_model, double ci, double *stats, uint64_t *used);
int ngd_run_windows_job_var_groups_stats(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win,
                                         const uint64_t *block_maps, uint64_t maps_len, const uint64_t *map_off, uint32_t n_rep,
                                         uint64_t block_size, uint64_t tot_sites, uint64_t evol_model, double ci, double *stats,
                                         uint64_t *used);
/* device time (HIP events) of the summary kernels in the last of these calls, summed over its launches */
int ngd_last_boot_stats_ms(const ngd_engine *e, double *ms);

/* Neighbour-joining trees (added under ABI 6): one unrooted tree per matrix leaves the device -- 2n - 3 branches --
 * instead of n (n - 1) / 2 sums and counts.  Canonical neighbour joining (Saitou & Nei 1987; Studier & Keppler 1988), stated
 * so that a tree's bits are a function of its matrix alone, never of storage, launch, chunk or reduction order.  Every
 * floating-point operation is a per-element formula evaluated exactly as parenthesised, in double, without contraction;
 * the one sum whose order matters is given its order.
 *   input      d[a][b] for the leaves 0 .. n - 1, n = n_ind >= 3, from a matrix's n_pairs cells in ngd_pair_index order;
 *              internal nodes get the ids n, n + 1, .. in order of creation; m = the number of live nodes
 *   at start   r_a = SUM_{b != a} d[a][b], the terms added one by one in ascending b starting from 0.0
 *   while m > 3
 *     for live a < b (node ids):  Q(a,b) = ((double)(m - 2) * d_ab - r_a) - r_b
 *     join the pair (i, j), i < j, that is smallest in the total order on (Q, a, b): a tie in Q goes to the lower a,
 *       then to the lower b
 *     l_i = 0.5 * d_ij + (r_i - r_j) / (2.0 * (double)(m - 2)),  l_j = d_ij - l_i   (negative lengths are left as they come)
 *     new node u; for every other live k:  d_uk = 0.5 * ((d_ik + d_jk) - d_ij),  r_k = ((r_k - d_ik) - d_jk) + d_uk
 *     r_u = 0.5 * ((r_i + r_j) - (double)m * d_ij)   (the closed form of SUM_k d_uk: no order)
 *   at m = 3, a < b < c, the three branches to the centre:
 *     l_a = 0.5 * ((d_ab + d_ac) - d_bc),  l_b = 0.5 * ((d_ab + d_bc) - d_ac),  l_c = 0.5 * ((d_ac + d_bc) - d_ab)
 * Record of a matrix: NGD_NJ_NBRANCH(n) = 2n - 3 entries of child (int32) and len (double), and one status (uint32).
 * Join t (t < n - 3) makes node n + t: entries 2t and 2t + 1 of child are i and j, the same entries of len l_i and l_j; the
 * last three entries are a, b, c and their lengths.  Outputs, in host memory: child[n_mat][2n - 3], len[n_mat][2n - 3],
 * status[n_mat].
 * A matrix with any cell that is not finite (NaN, +-inf: no shared site under --pairwise_del, the replicates of a window
 * shorter than one block) has no tree: status 0, every child -1, every len a positive quiet NaN; otherwise status 1.  The
 * other matrices of the call are not affected.  (Finite cells so large that a Q overflows are outside the contract: some
 * tree is returned, its choice of pairs is not pinned.)
 * From sums and counts a cell's value is ngd_finish()'s, operation by operation (the division and the products carry the
 * host's bits, log is the device's).
 * Ties at m = 4: the complementary pairs (a,b) and (c,d) of four live nodes have algebraically equal Q, so rounding picks
 * between two records of the SAME unrooted tree -- best and second-best Q there differ by ~5e-16 relative on random data,
 * while at every m >= 5 the smallest gap seen was 3e-5.  Device and host twin follow the same formulas and so pick alike
 * for the same cells; values that differ in the last bits (the device's log) may pick the other record.  ngd_nj_support()
 * counts both alike. */
#define NGD_NJ_NBRANCH(n) (2 * (n) - 3)
/* the most individuals the device form serves (the row sums and node ids of a matrix stay in on-chip memory); more is
 * NGD_E_INVALID */
uint32_t ngd_nj_max_ind(void);
/* The contract in plain host arithmetic on val[n_mat][n_pairs]; needs no device, any n_ind >= 3; matrices are spread over
 * host threads, which changes no bit.  NGD_E_INVALID: a null pointer, n_mat 0, n_ind < 3. */
int ngd_nj_host(const double *val, uint64_t n_mat, uint64_t n_ind, int32_t *child, double *len, uint32_t *status);
/* ... on the device (one workgroup per matrix, nj.hip), of [n_mat][n_pairs] values as they are, or of sums and counts in
 * device memory as a *_device call wrote them (d_cnt is not read when tot_sites > 0); n_ind is the engine's.  The matrices
 * go through device scratch (a full n x n matrix of doubles each) in chunks of NGD_OPT_NJ_MAX_BYTES; chunking changes no
 * bit.  NGD_E_INVALID, before anything is launched: a null pointer, n_mat 0, n_ind < 3 or above ngd_nj_max_ind(), tot_sites
 * with --pairwise_del, an engine that owns a share of the pairs; NGD_E_MODEL for evol_model > 2.  A refused call leaves
 * outputs and engine as they were. */
int ngd_nj_values_device(ngd_engine *e, const void *d_val, uint64_t n_mat, int32_t *child, double *len, uint32_t *status);
int ngd_nj_device(ngd_engine *e, const void *d_sum, const void *d_cnt, uint64_t n_mat, uint64_t tot_sites, uint64_t evol_model,
                  int32_t *child, double *len, uint32_t *status);
/* ngd_run_job_device (one set of n_rep + 1 matrices) / ngd_run_windows_device (one matrix per window) /
 * ngd_run_windows_job_var_device (one set per window) into the engine's batch buffers, followed by that reduction: plans,
 * fix-up, NGD_OPT_EM_EXACT* and refusals are the sibling's, and the trees are ngd_nj_device()'s on the sibling's output
 * bit for bit at the same options.  n_rep = 0 is allowed: a plain run's one tree.  Outputs: child / len
 * [n_set][n_rep + 1][2n - 3], status [n_set][n_rep + 1]; dist0, unless NULL, receives [n_set][n_pairs]: matrix 0 of every
 * set finished by ngd_finish() on the host from its sums and counts -- the bits the _dist sibling gives. */
int ngd_run_job_nj(ngd_engine *e, const uint64_t *block_maps, uint32_t n_rep, uint64_t n_blocks, uint64_t block_size,
                   uint64_t tot_sites, uint64_t evol_model, int32_t *child, double *len, uint32_t *status, double *dist0);
int ngd_run_windows_nj(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win, uint64_t tot_sites,
                       uint64_t evol_model, int32_t *child, double *len, uint32_t *status, double *dist0);
int ngd_run_windows_job_var_nj(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win,
                               const uint64_t *block_maps, uint64_t maps_len, const uint64_t *map_off, uint32_t n_rep,
                               uint64_t block_size, uint64_t tot_sites, uint64_t evol_model, int32_t *child, double *len,
                               uint32_t *status, double *dist0);
/* device time (HIP events) of the tree kernels in the last of these calls, summed over its launches */
int ngd_last_nj_ms(const ngd_engine *e, double *ms);
/* Bootstrap support of matrix 0's tree, pure host: join t of matrix 0 defines the bipartition "leaves under node n + t |
 * the rest"; support[t] (n - 3 entries) is the number of matrices r >= 1 with status 1 whose tree has the same
 * bipartition, *n_used the number of those matrices.  Bipartitions are compared as leaf sets normalised to the side
 * without leaf 0 (the two m = 4 records of one tree count alike).  Matrix 0 with status 0: every support 0.
 * NGD_E_INVALID: a null pointer, n_mat 0, n_ind < 3, a child entry out of range in a tree with status 1. */
int ngd_nj_support(const int32_t *child, const uint32_t *status, uint64_t n_mat, uint64_t n_ind, uint32_t *support,
                   uint32_t *n_used);
/* One record as a Newick line, pure host, sized like ngd_format_matrix (call with out = NULL): "(x,y,z);\n", a leaf
 * "label:%.10f", an internal node "(x,y)" followed by its support number if support (n - 3 entries, by join) is not NULL,
 * then ":%.10f"; children in recorded order; a tree with status 0 (child[0] < 0) is ";\n"; labels NULL (or a NULL entry):
 * "Ind_<i>".  NGD_E_INVALID: a null pointer, n_ind < 3, an entry that names a node no earlier join made.  Returns the
 * number of bytes (no terminator), written only if cap is large enough, or a negative NGD_E_* code. */
int64_t ngd_nj_newick(const int32_t *child, const double *len, uint64_t n_ind, const char *const *labels, const uint32_t *support,
                      char *out, uint64_t cap);

/* Classical MDS (added under ABI 6): the principal coordinates (Torgerson / Gower: R's cmdscale) of every matrix, computed where the matrix lies: K (n + 1) + 2
 * numbers per matrix cross the link instead of n (n - 1) / 2 sums and counts.
 *   input      d_ab for the individuals 0 .. n - 1, n = n_ind >= 3, from a matrix's n_pairs cells in ngd_pair_index order,
 *              d_aa = 0
 *   centred    A_ab = -0.5 * d_ab^2;  B = A - rowmean - colmean + grandmean   (symmetric, B 1 = 0)
 *   outputs    eig[K]     the K algebraically largest eigenvalues of B, in descending order
 *              vec[K][n]  a unit eigenvector for each; the component of largest magnitude is positive, the lowest index
 *                         wins an exact tie
 *              tot[2]     { the sum of all n eigenvalues, the sum of the positive ones }
 *              status     uint32
 *   1 <= K <= min(n - 1, ngd_mds_max_dim()).  Coordinates are vec[k][i] * sqrt(max(eig[k], 0)): ngd_mds_coords().
 * Outputs, in host memory: eig[n_mat][K], vec[n_mat][K][n], tot[n_mat][2], status[n_mat].
 * A matrix with any cell that is not finite (NaN, +-inf) has status 0 and every eigenvalue, vector entry and total a
 * positive quiet NaN; the other matrices of the call are not affected.  Every finite matrix has status 1, whatever its
 * spectrum: all cells zero (every eigenvalue 0, the vectors the first K unit vectors), all cells equal (one eigenvalue of
 * multiplicity n - 1: some orthonormal basis of its space), a matrix that is not Euclidean (negative eigenvalues; they
 * count in tot[0] alone).  (Cells whose squares overflow, |d| above about 1e150, are outside the contract.)
 * Method: a direct one, so that accuracy does not depend on the gaps between eigenvalues -- Householder tridiagonalisation,
 * all n eigenvalues of the tridiagonal matrix by bisection on Sturm counts, the top K vectors by inverse iteration from a
 * fixed start vector with modified Gram-Schmidt against the vectors before them (a repeated eigenvalue gets a perturbed
 * shift), the reflectors applied in reverse.  With S = max |eigenvalue|: eigenvalues and residuals |B v - eig v|_2 within
 * 1e-9 S, totals within 1e-9 of the sum of |eigenvalue|, |V V^T - I| <= 1e-9; a vector whose eigenvalue lies 1e-3 S or more
 * from every other one agrees with any other solver's to 1 - 1e-9 in the dot product (inside a cluster only the space is
 * determined).
 * From sums and counts a cell's value is ngd_finish()'s, operation by operation (the division and the products carry the
 * host's bits, log is the device's).
 * Determinism: a matrix's output bits are a function of its cells and K alone, never of its position in the call, the chunk
 * or what else the launch holds (no atomics, fixed reduction trees).  Device and host twin follow the same method but need
 * not agree bit for bit (their sums run in different orders), and the environment variable NGD_MDS_WG (256, 512 or 1024:
 * the workgroup, for measurement) changes the device's trees and so may change bits. */
/* the most individuals the device form serves (the tridiagonal matrix stays in on-chip memory) and the most dimensions K;
 * more is NGD_E_INVALID */
uint32_t ngd_mds_max_ind(void);
uint32_t ngd_mds_max_dim(void);
/* The contract in plain host arithmetic on val[n_mat][n_pairs]; needs no device, any n_ind >= 3; matrices are spread over
 * host threads, which changes no bit.  NGD_E_INVALID: a null pointer, n_mat 0, n_ind < 3, K = 0, K > n_ind - 1 or above
 * ngd_mds_max_dim(). */
int ngd_mds_host(const double *val, uint64_t n_mat, uint64_t n_ind, uint32_t K, double *eig, double *vec, double *tot,
                 uint32_t *status);
/* coords[n_mat][n_ind][K] = vec[k][i] * sqrt(max(eig[k], 0)), pure host (NaN where eig is NaN).  NGD_E_INVALID as above. */
int ngd_mds_coords(const double *eig, const double *vec, uint64_t n_mat, uint64_t n_ind, uint32_t K, double *coords);
/* ... on the device (one workgroup per matrix, mds.hip), of [n_mat][n_pairs] values as they are, or of sums and counts in
 * device memory as a *_device call wrote them (d_cnt is not read when tot_sites > 0); n_ind is the engine's.  The matrices
 * go through device scratch in chunks of NGD_OPT_MDS_MAX_BYTES; chunking changes no bit.  NGD_E_INVALID, before anything
 * is launched: a null pointer, n_mat 0, n_ind < 3 or above ngd_mds_max_ind(), K = 0, K > n_ind - 1 or above
 * ngd_mds_max_dim(), tot_sites with --pairwise_del, an engine that owns a share of the pairs; NGD_E_MODEL for evol_model
 * > 2.  A refused call leaves outputs and engine as they were. */
int ngd_mds_values_device(ngd_engine *e, const void *d_val, uint64_t n_mat, uint32_t K, double *eig, double *vec, double *tot,
                          uint32_t *status);
int ngd_mds_device(ngd_engine *e, const void *d_sum, const void *d_cnt, uint64_t n_mat, uint64_t tot_sites, uint64_t evol_model,
                   uint32_t K, double *eig, double *vec, double *tot, uint32_t *status);
/* ngd_run_job_device / ngd_run_windows_device / ngd_run_windows_job_var_device into the engine's batch buffers, followed by
 * that reduction: plans, fix-up, NGD_OPT_EM_EXACT* and refusals are the sibling's, and the outputs are ngd_mds_device()'s
 * on the sibling's output bit for bit at the same options.  n_rep = 0 is allowed.  Outputs: eig [n_set][n_rep + 1][K], vec
 * [n_set][n_rep + 1][K][n], tot [n_set][n_rep + 1][2], status [n_set][n_rep + 1]; dist0, unless NULL, receives
 * [n_set][n_pairs]: matrix 0 of every set finished by ngd_finish() on the host -- the bits the _dist sibling gives. */
int ngd_run_job_mds(ngd_engine *e, const uint64_t *block_maps, uint32_t n_rep, uint64_t n_blocks, uint64_t block_size,
                    uint64_t tot_sites, uint64_t evol_model, uint32_t K, double *eig, double *vec, double *tot, uint32_t *status,
                    double *dist0);
int ngd_run_windows_mds(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win, uint64_t tot_sites,
                        uint64_t evol_model, uint32_t K, double *eig, double *vec, double *tot, uint32_t *status, double *dist0);
int ngd_run_windows_job_var_mds(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win,
                                const uint64_t *block_maps, uint64_t maps_len, const uint64_t *map_off, uint32_t n_rep,
                                uint64_t block_size, uint64_t tot_sites, uint64_t evol_model, uint32_t K, double *eig, double *vec,
                                double *tot, uint32_t *status, double *dist0);
/* device time (HIP events) of the MDS kernels in the last of these calls, summed over its launches */
int ngd_last_mds_ms(const ngd_engine *e, double *ms);
/* Alignment of bootstrap replicates (added under ABI 6): an MDS solution is defined up to an orthogonal transformation --
 * signs are arbitrary, axes of close eigenvalues rotate into each other from replicate to replicate -- so the replicates
 * of a set are rotated onto its matrix 0 (orthogonal Procrustes) before anything is averaged over them.
 * A set is n_mat = n_rep + 1 matrices with their outputs eig[K], vec[K][n], status; X_r[i][k] = vec_r[k][i] *
 * sqrt(max(eig_r[k], 0)), stored [K][n] (axis by axis).
 *   No translation step: B 1 = 0, so every column of X with a non-zero eigenvalue is centred already, up to rounding.
 *   No scaling step: the spread of the replicates is the quantity being estimated.
 *   for every replicate r >= 1 with status 1, where matrix 0 has status 1 too:
 *     M = X_r^T X_0   (K x K)
 *     Q = U V^T for M = U S V^T, the orthogonal polar factor of M; reflections are allowed (signs are arbitrary)
 *     Y_r = X_r Q,   fit_r = |Y_r - X_0|_F^2   (not normalised)
 *   Y_0 = X_0, fit_0 = 0.
 *   A replicate with status 0, and every matrix of a set whose matrix 0 has status 0, has Y and fit a positive quiet NaN:
 *   the summaries leave it out and count it as left out, as ngd_boot_stats_* treat every cell that is not finite.
 * Where M is singular (a zero column of coordinates from eig <= 0, all-zero matrices, K above the rank) Q is not unique,
 * and only this is pinned: |Q Q^T - I| <= 1e-9; fit_r within 1e-9 (|X_r|^2 + |X_0|^2) of |X_r|^2 + |X_0|^2 - 2 SUM sigma;
 * bits that are a function of (X_r, X_0, K) alone.  Where sigma_min(M) >= 1e-3 sigma_max(M), Y_r agrees with any other
 * solver's to 1e-9 max(|X_0|, |X_r|) (the polar factor moves by 2 |dM| / (sigma_{K-1} + sigma_K): three orders of margin
 * at rounding level).
 * Method: the K^2 sums of M as fixed trees; M scaled by a power of two to a largest magnitude in [1, 2) (so that scaling
 * both configurations by a power of two scales Y and fit exactly); a one-sided (Hestenes) Jacobi on its columns in the
 * cyclic order (0,1), (0,2), .., (K-2,K-1), at most 64 sweeps, a pair left alone when |g| <= eps sqrt(a b) or when either
 * column's squared norm is no more than 1e-24 of the largest at the sweep's start; the columns that end no longer than
 * 1e-12 of the longest are replaced: e_0, e_1, .. in order, each orthogonalised twice against the finished columns, the
 * first whose residual exceeds 0.5 / sqrt(K) taken.  Device and host twin follow the same method and agree to the
 * tolerances above, not bit for bit (their sums run in different orders).
 * Summary of a set: the cells [K][n] of Y followed by the [K] eigenvalues of the same matrices, n_cells = K (n + 1); the
 * value at position 0 is matrix 0's, positions 1 .. n_rep the replicates' (the eigenvalues of a matrix left out are NaN
 * too); summarised by the definitions of "Bootstrap summaries" bit for bit: stats [NGD_BOOT_NSTAT][n_cells]; used is the
 * number of replicates that went in. */
/* The contract in plain host arithmetic, of eig [n_set][n_mat][K], vec [n_set][n_mat][K][n_ind] and status
 * [n_set][n_mat] (NULL: every matrix has status 1) as the calls above give them: aligned [n_set][n_mat][K][n_ind], fit
 * [n_set][n_mat].  NGD_E_INVALID: a null pointer, n_set or n_mat 0, n_ind < 3, K = 0, K > n_ind - 1 or above
 * ngd_mds_max_dim(). */
int ngd_mds_align_host(const double *eig, const double *vec, const uint32_t *status, uint64_t n_set, uint64_t n_mat, uint64_t n_ind,
                       uint32_t K, double *aligned, double *fit);
/* The alignment alone, on the device (one workgroup per matrix, mds_align.hip), of coordinates as they are: d_coords
 * [n_set][n_mat][K][n] float64 in device memory (read only); status [n_set][n_mat] in HOST memory, NULL: every matrix has
 * status 1; n_ind is the engine's.  Outputs in host memory as above.  NGD_E_INVALID, before anything is launched: a null
 * pointer, n_set or n_mat 0, n_set * n_mat of 2^31 and more, n_ind < 3, K = 0, K > n_ind - 1 or above ngd_mds_max_dim(). */
int ngd_mds_align_values_device(ngd_engine *e, const void *d_coords, const uint32_t *status, uint64_t n_set, uint64_t n_mat,
                                uint32_t K, double *aligned, double *fit);
/* ngd_run_job_mds / ngd_run_windows_job_var_mds, then the alignment of every set and its summary, all on the device: K (n
 * + 1) + 2 numbers of matrix 0, 5 K (n + 1) statistics and n_rep + 1 fits per set cross the link, whatever n_rep.  Plans,
 * fix-up, options and refusals are the _mds sibling's, then those of the summaries: n_rep 0, ci outside (0, 1), n_rep above
 * ngd_boot_stats_max_rep(); a refused call leaves outputs and engine as they were.  Outputs: eig0 [n_set][K], vec0
 * [n_set][K][n], tot0 [n_set][2] -- matrix 0's, the _mds sibling's bit for bit --, status [n_set][n_rep + 1], stats
 * [n_set][NGD_BOOT_NSTAT][K (n + 1)], used [n_set] (the replicates that went in), fit [n_set][n_rep + 1]; aligned, unless
 * NULL, receives [n_set][n_rep + 1][K][n]; dist0, unless NULL, [n_set][n_pairs] as in the sibling.  aligned and fit are
 * ngd_mds_align_values_device()'s on the sibling's coordinates, stats ngd_boot_stats_values_device()'s on the aligned
 * cells and the eigenvalues, bit for bit. */
int ngd_run_job_mds_align(ngd_engine *e, const uint64_t *block_maps, uint32_t n_rep, uint64_t n_blocks, uint64_t block_size,
                          uint64_t tot_sites, uint64_t evol_model, uint32_t K, double ci, double *eig0, double *vec0, double *tot0,
                          uint32_t *status, double *stats, uint64_t *used, double *fit, double *aligned, double *dist0);
int ngd_run_windows_job_var_mds_align(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win,
                                      const uint64_t *block_maps, uint64_t maps_len, const uint64_t *map_off, uint32_t n_rep,
                                      uint64_t block_size, uint64_t tot_sites, uint64_t evol_model, uint32_t K, double ci,
                                      double *eig0, double *vec0, double *tot0, uint32_t *status, double *stats, uint64_t *used,
                                      double *fit, double *aligned, double *dist0);
/* device time (HIP events) of the two alignment kernels in the last of these calls, summed over its launches */
int ngd_last_mds_align_ms(const ngd_engine *e, double *ms);

/* Comparison of windows (added under ABI 6): the windows of a genome scan related to one another where their matrices lie --
 * W (W + 2) numbers cross the link instead of W matrices.
 *   input      W vectors x_w of P cells each: in the run forms a window's matrix 0, every cell finished as ngd_finish()
 *              does (the division and the products carry the host's bits, log is the device's), P = n (n - 1) / 2; in
 *              the values form doubles as they are, any P >= 1
 *   per vector status[w]  1 if every cell is finite, else 0: such a vector is left out and disturbs no other
 *              mean[w]    (SUM_c x_wc) / P by a fixed tree
 *   per pair   gram[a][b] SUM_c (x_ac - mean[a]) (x_bc - mean[b]): a full W x W array, symmetric bit for bit
 * Row and column of a status-0 vector are a positive quiet NaN, and so is its mean: written from the status, not produced
 * by arithmetic.
 * Bits: gram[a][b] is a function of the cells of a and b and of (W, P) alone -- not of the other vectors, of where a and b
 * stand among them, of how the windows fell into groups, of the device's CU count or of any NGD_OPT_* budget.  Scaling
 * every cell by 2^k scales mean by 2^k and gram by 4^k exactly (short of overflow and underflow).  No atomics; every sum
 * has a fixed order: the cell axis is cut into slices of ngd_win_cmp_slice(W, P) cells, a slice's products are added in
 * ascending k-groups of four cells on the FP64 matrix pipe, a pair's slices in ascending order.
 * Accuracy: |gram[a][b] - exact| <= 1e-9 sqrt(exact[a][a] exact[b][b]).
 * Derived on the host by ngd_win_cmp_finish() (plain C++, IEEE sqrt only):
 *   cor[a][b]  gram[a][b] / sqrt(gram[a][a] gram[b][b]), the Mantel statistic of the two matrices; NaN if either diagonal is
 *              exactly 0.  An all-zero vector and a vector of one power-of-two value give exact zeros and hence NaN; a
 *              vector of one other repeated value is not pinned (its mean may round, and the diagonal is then a tiny
 *              positive number or 0).
 *   rms[a][b]  sqrt(max(0, gram[a][a] + gram[b][b] - 2 gram[a][b] + P (mean[a] - mean[b])^2) / P), the diagonal exactly 0:
 *              the root-mean-square difference of the cells.  The contract is on rms^2: within 1e-9 of (gram[a][a] +
 *              gram[b][b] + P (mean[a] - mean[b])^2) / P -- the RMS of two nearly identical vectors is therefore only good
 *              to about 1e-8 of that scale's root (the difference is formed from the sums, not from the cells).  Two
 *              vectors with the same cells have rms exactly 0.
 *   Anything that touches a status-0 vector is NaN.
 * Device and host twin follow the same definition but need not agree bit for bit. */
/* the most vectors a call takes (the kernels' tile indices); more is NGD_E_INVALID */
uint32_t ngd_win_cmp_max_vec(void);
/* cells per slice of the cell axis at (n_vec, n_cells), a multiple of 4; 0 for n_vec 0, n_cells 0 or n_vec above the limit.
 * Pure host arithmetic. */
uint64_t ngd_win_cmp_slice(uint64_t n_vec, uint64_t n_cells);
/* The contract in plain host arithmetic on values[n_vec][n_cells] (sums in slices of ngd_win_cmp_slice() cells); needs no
 * device; vectors are spread over host threads, which changes no bit.  Outputs mean[n_vec], gram[n_vec][n_vec],
 * status[n_vec].  NGD_E_INVALID: a null pointer, n_vec 0 or above ngd_win_cmp_max_vec(), n_cells 0. */
int ngd_win_cmp_host(const double *values, uint64_t n_vec, uint64_t n_cells, double *mean, double *gram, uint32_t *status);
/* cor[n_vec][n_vec] and rms[n_vec][n_vec] as defined above, pure host.  NGD_E_INVALID: a null pointer, n_vec or n_cells 0. */
int ngd_win_cmp_finish(const double *mean, const double *gram, const uint32_t *status, uint64_t n_vec, uint64_t n_cells, double *cor,
                       double *rms);
/* ... on the device (win_cmp.hip), of [n_vec][n_cells] values in device memory as they are -- any n_cells >= 1, not tied to
 * the engine's n_ind --, or of [n_vec][n_pairs] sums and counts as a *_device call wrote them (d_cnt is not read when
 * tot_sites > 0).  Outputs in host memory.  The operand (8 bytes per cell, vectors padded to whole tile blocks) and the
 * partial sums are resident for the call; their bytes follow from (n_vec, n_cells) and a call that exceeds
 * NGD_OPT_WIN_CMP_MAX_BYTES is refused with NGD_E_INVALID and a message that names the bytes needed.  NGD_E_INVALID, before
 * anything is launched: a null pointer, n_vec 0 or above ngd_win_cmp_max_vec(), n_cells 0, tot_sites with --pairwise_del, an
 * engine that owns a share of the pairs; NGD_E_MODEL for evol_model > 2.  A refused call leaves outputs and engine as they
 * were. */
int ngd_win_cmp_values_device(ngd_engine *e, const void *d_val, uint64_t n_vec, uint64_t n_cells, double *mean, double *gram,
                              uint32_t *status);
int ngd_win_cmp_device(ngd_engine *e, const void *d_sum, const void *d_cnt, uint64_t n_vec, uint64_t tot_sites, uint64_t evol_model,
                       double *mean, double *gram, uint32_t *status);
/* ngd_run_windows_device into the engine's batch buffers, group of windows by group, each group's matrices packed into the
 * operand as it stands there; then the comparison.  Plans, fix-up, NGD_OPT_EM_EXACT_WIN and the windows' refusals are
 * ngd_run_windows' unchanged (the operand is allocated before the windows are planned, so the batches' budget sees what
 * is left), and the outputs are ngd_win_cmp_device()'s on the sibling's output bit for bit.  dist, unless NULL, receives
 * [n_win][n_pairs]: every window's matrix finished by ngd_finish() on the host -- ngd_run_windows_dist()'s bits. */
int ngd_run_windows_cmp(ngd_engine *e, const uint64_t *win_lo, const uint64_t *win_hi, uint64_t n_win, uint64_t tot_sites,
                        uint64_t evol_model, double *mean, double *gram, uint32_t *status, double *dist);
/* device time (HIP events) of the four kernels in the last of these calls, summed over its launches: ms[4] = the vectors'
 * statistics, the packing, the Gram pass, the sum of its partials */
int ngd_last_win_cmp_ms(const ngd_engine *e, double ms[4]);

/* The tail of gen_dist(), ngsDist.cpp:372-401, on the HOST with the host's
 * libm so that -0.0 / inf / nan cells print exactly as the reference's do:
 *   cnt = tot_sites if tot_sites > 0; d = sum/cnt;
 *   model 0: d; 1: -log(1-d); 2: -log(1-d*4/3)*3/4; 3..6: NGD_E_MODEL. */
int ngd_finish(const double *sum, const uint64_t *cnt, uint64_t n_pairs,
               uint64_t tot_sites, uint64_t evol_model, double *dist);
/* The same over cells that are still arriving (a job's matrices leaving the device chunk by chunk): cells [0, *landed)
 * of sum and cnt are final; the caller -- another thread -- raises *landed, in any steps, up to n_pairs, and the call
 * returns when every cell is finished.  One wake-up of the host threads for the whole job: the tail runs beside the
 * copies (ngsDist.cpp:372-401 on up to millions of cells per bootstrap job). */
int ngd_finish_stream(const double *sum, const uint64_t *cnt, uint64_t n_pairs, uint64_t tot_sites, uint64_t evol_model,
                      double *dist, const volatile uint64_t *landed);

/* The print block of one matrix, ngsDist.cpp:282-287 with join() gen_func.cpp:479-496:
 * "\n<n_ind>\n", then per individual its label and n_ind cells "\t%.10f", newline.  `dist` is
 * ngd_finish()'s output (pair order); the matrix is its symmetric expansion with a zero diagonal
 * (dist_matrix, ngsDist.cpp:200,:411).  Cells are formatted exactly as printf's "%.10f" does
 * (-0.0000000000, inf, nan, -nan included), rows in parallel on n_threads host threads (0 = auto).
 * Returns the number of bytes of the block (no terminator); they are written to `out` only if
 * cap is large enough (call with out = NULL to size), or a negative NGD_E_* code. */
int64_t ngd_format_matrix(const double *dist, uint64_t n_ind, const char *const *labels, char *out,
                          uint64_t cap, uint32_t n_threads);

/* Bootstrap block map exactly as the reference draws it (gsl_rng_taus seeded
 * with --seed, ngsDist.cpp:179-180; one draw per block, :421-423).  The state
 * is three uint32 carried across replicates by the caller. */
void ngd_taus_seed(uint32_t state[3], uint64_t seed);
uint32_t ngd_taus_get(uint32_t state[3]);
double ngd_taus_uniform(uint32_t state[3]);
void ngd_boot_block_map(uint32_t state[3], uint64_t n_blocks, uint64_t *block_map);

/* geometry helpers */
uint64_t ngd_n_pairs(uint64_t n_ind);
uint64_t ngd_pair_index(uint64_t n_ind, uint64_t i1, uint64_t i2); /* i1 < i2 */
/* the shard (0 .. shard_world-1) that computes pair i1 < i2: 128 x 128 pair tiles of
 * the upper triangle, dealt by cost (off-diagonal tiles first) to the least loaded
 * shard -- the rule ngd_create() uses.  Pure host arithmetic. */
uint32_t ngd_shard_of_pair(uint64_t n_ind, uint64_t i1, uint64_t i2, uint32_t shard_world);
/* the same for every pair, in pair order: owner[ngd_pair_index(n_ind, i1, i2)] (n_pairs entries) */
void ngd_shard_map(uint64_t n_ind, uint32_t shard_world, int32_t *owner);
/* ngd_config.single_image = 2: the symmetric score matrix as a sum of three weighted squares,
 * score = SUM_r d[r] c_r c_r^T with c row-major (c[3 r + g]) -- Lagrange's reduction, dyadic c and d for the reference's
 * two matrices (parse_args.cpp:25-27, :134-137).  NGD_E_INVALID for an asymmetric matrix.  Pure host arithmetic. */
int ngd_score_congruence(const double score[9], double c[9], double d[3]);
/* free / total memory of a device (device < 0: the current one): lets a host decide whether a data set fits one
 * engine or has to go through it a range of sites at a time (site sharding in time instead of across GPUs) */
int ngd_device_memory(int device, uint64_t *free_bytes, uint64_t *total_bytes);
/* bytes of device memory the engine holds for this configuration */
uint64_t ngd_device_bytes(const ngd_engine *e);

#ifdef __cplusplus
}
#endif
#endif /* NGSDIST_AMD_H */
