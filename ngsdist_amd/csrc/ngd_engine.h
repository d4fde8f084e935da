// ngd_engine.h -- the engine behind the C ABI of include/ngsdist_amd.h, as its translation units see it (engine*.hip):
// the engine's state, memory that arrives piece by piece, and what one unit asks of another.  Private to this directory.
#pragma once
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "kg_ranges.h"
#include "ngd_buffers.h"
#include "ngd_internal.h"
#include "ngd_shard.h"

#pragma GCC visibility push(hidden)


// The per-block partial results of a bootstrap job (sums [slices][n_pad][n_pad]; counts [n_blocks][n_pad][n_pad] under
// --pairwise_del; 0/1 weights per slice where blocks are not whole k-groups), cached from job to job -- and the scratch of
// the EM batch pass, the spilled-terms plan and the windows' segment slab.  A borrower takes the memory through borrow_*(),
// which drops that cache's key; only partials_impl, having filled it, names it again.
struct BlockScratch {
  DevBuf<double> wslice;
  // the geometry of the cached sums: slices of per_slice k-groups (sites), `sub` to a block
  uint64_t per_slice = 0;
  uint32_t nks = 0, sub = 0;
  bool has_sums(uint64_t B, uint64_t blocks) const { return boot_B == B && boot_blocks == blocks; }
  bool has_counts(uint64_t B, uint64_t blocks) const { return cnt_B == B && cnt_blocks == blocks; }
  uint64_t sums_block() const { return boot_B; }
  const DevBuf<double> &sums() const { return slab_boot; }
  const DevBuf<uint32_t> &counts() const { return cnt_boot; }
  DevBuf<double> &borrow_sums() { boot_B = boot_blocks = 0; return slab_boot; }
  DevBuf<uint32_t> &borrow_counts() { cnt_B = cnt_blocks = 0; return cnt_boot; }
  void sums_filled(uint64_t B, uint64_t blocks) { boot_B = B; boot_blocks = blocks; }
  void counts_filled(uint64_t B, uint64_t blocks) { cnt_B = B; cnt_blocks = blocks; }
  void drop() { boot_B = boot_blocks = cnt_B = cnt_blocks = 0; }
  uint64_t bytes() const { return slab_boot.bytes() + cnt_boot.bytes(); }  // what a budget rule already holds

 private:
  DevBuf<double> slab_boot;
  DevBuf<uint32_t> cnt_boot;
  uint64_t boot_B = 0, boot_blocks = 0, cnt_B = 0, cnt_blocks = 0;  // block size and blocks of what is cached (0: nothing)
};

// (device, st, dev_bytes and the piece ranges: ngd_mem, ngd_buffers.h)
struct ngd_engine : ngd_mem {
  ngd_config cfg{};
  ngd_geom g{};
  ngd_score sc{};
  int kernel = 0;  // resolved NGD_KERNEL_*
  hipEvent_t ev[5] = {};
  // resident data set
  DevBuf<double> PA, QB, PI;
  // ngd_config.single_image (MFMA kernel): QB is not resident; a launch forms it for a range of k-groups at a time
  bool single_image = false;    // (ngd_config.single_image = 1: q is formed range by range)
  bool congruent = false;       // ngd_config.single_image = 2: the image holds t (sc.c, sc.d), read for both operands
  DevBuf<double> d_wD;          // ... and these are the weights of a plain pass: sc.d[coordinate] per contraction index
  // ... on the reference's matrices without --pairwise_del (sc.fix: t0 = p0 + p1 + p2, 1 for normalised input) the plain
  // pass leaves the t0 k-groups out -- kg % 3 == 0 in the image's layout, ngd_layout.h -- and the reduction adds their
  // products as a constant (NGD_OPT_UNIT_SKIP): the list of the other k-groups (+ NGD_KG_LIST_PAD), made by ngd_create;
  // E_i = SUM_s (t0_i(s) - 1) in units of 2^-53 (+ one word: the scan's flag) and the *unit* mark, made by ngd_commit
  DevBuf<uint32_t> d_kgskip;
  uint64_t n_kgskip = 0, skip_per_slice = 0;
  DevBuf<long long> d_unitE;
  bool unit_ok = false;
  uint64_t opt_unit_skip = 1;
  uint64_t plain_kg = 0;  // k-groups the last plain pass visited (ngd_last_plain_pass)
  // ... and, for the reference's matrices (sc.fix), the fix-up pass of the pairs its arithmetic cannot hold to 1e-9
  // relative (fixup.hip): SM[site][individual] = min(p0, p2) beside the image, the pairs a reduction noted, scratch
  DevBuf<double> SM;
  DevBuf<unsigned long long> d_fixlist;
  DevBuf<uint32_t> d_fixcount, d_fixseen;
  PinBuf<uint32_t> h_fixcount;
  DevBuf<double> d_fixparts, d_fixthr;
  DevBuf<ngd_fix_tile> d_fixtiles;  // 16 x 16 tiles of pairs that hold several noted pairs (fixup_pass)
  DevBuf<double> d_fixtparts;       // ... and their per-slice partial sums
  DevBuf<double> fix_p, fix_q, d_fixnew;  // the fix-up pass as a whole two-operand pass (fixup_by_pass)
  ngd_fixup_info fix_info{};
  std::vector<ngd_tile> h_tiles16;  // host copy of the owned 16 x 16 tiles that hold a pair (the fix-up pass's "every pair")
  uint32_t fix_cap = 0;  // pairs the reductions can note for the fix-up pass (ngd_internal.h NGD_FIX_LIST): the capacity of d_fixlist
  uint64_t opt_fix_work = 0;  // NGD_OPT_FIXUP_WORK: the pass's budget in pair-sites (0 = none: every noted pair is recomputed)
  DevBuf<double> QB_res;        // ... except its first qb_res_kg k-groups (ngd_config.second_image_mib), formed at ngd_commit()
  uint64_t qb_res_kg = 0;
  DevBuf<double> qb_chunk;      // the scratch a range is formed in
  uint64_t qb_chunk_kg = 0;     // k-groups a range may span (NGD_OPT_SINGLE_IMAGE_BYTES)
  DevBuf<unsigned long long> mask, planes;
  // bootstrap
  DevBuf<uint32_t> d_mult, d_ws;
  DevBuf<double> d_wk;  // multiplicity per contraction index k, as a double (MFMA kernel)
  DevBuf<uint32_t> d_kgl, d_kgcnt;  // k-groups a replicate visits (list + compaction scratch)
  PinBuf<uint32_t> h_mult;          // multiplicities counted from block maps
  // shard
  DevBuf<ngd_tile> d_tiles, d_tiles16, d_tiles64;
  uint32_t n_tiles = 0, n_tiles16 = 0, n_tiles64 = 0;
  int em_shape = 0;  // accum_em_table.hip: workgroup shape
  DevBuf<unsigned long long> d_emcnt;  // [4] work counters of the table-driven EM kernel + its clock counters
  unsigned long long em_counts[2] = {0, 0};  // ... of the last run
  // [2] MFMA kernel: shader-cycle / constant-rate counter deltas of one wavefront.  Pinned HOST memory mapped into the
  // device's address space: the wavefront's two stores cross PCIe, and reading them after the stream has been waited for
  // is a plain load (a 16-byte hipMemcpy per pass was 10 us of a 350 us job at cfg 2)
  PinBuf<unsigned long long> h_clk;
  unsigned long long *d_clk = nullptr;  // (the device's pointer to it)
  double clk_mhz = 0;                   // shader clock of the last accumulation launch (0: not sampled)
  double wall_khz = 100000.0;           // rate of the constant counter (hipDeviceAttributeWallClockRate)
  // MFMA kernel: per-wavefront 64x64 jobs, 4 per workgroup; "tri" = blocks on the diagonal
  DevBuf<ngd_job> d_jobs;
  uint32_t n_wg = 0;
  uint32_t wg_waves = 4;  // wavefronts (jobs) per workgroup of the MFMA kernel
  int exact_shapes = 0;  // small n_ind: one code path per block shape (accum_mfma.hip EXACT): 1 = blocks of 4 x 4 tiles, 2 = 2 x 4
  bool tri_diag = false;  // full 4 x 4 blocks (exact_shapes == 0) whose DIAGONAL blocks leave their lower triangle out
  DevBuf<uint64_t> d_pairs;
  uint64_t n_owned_pairs = 0;
  // scratch + results
  DevBuf<double> slab;
  uint32_t n_ks = 0;
  uint64_t per_slice = 0;
  DevBuf<double> d_sum;
  DevBuf<unsigned long long> d_cnt;
  BlockScratch blk;  // bootstrap by per-block partial sums, and the scratch the other plans borrow
  // a large slab costs ~12 ms per GB to allocate: until the passes it would have saved add up to that, calls are
  // served without it (rent_ms = their estimated cost so far, for the geometry rent_B / rent_blocks)
  double rent_ms = 0;
  uint64_t rent_B = 0, rent_blocks = 0;
  // per-call bootstrap weights (slice-major doubles / block-major uint32) and per-replicate site totals
  DevBuf<double> d_W;
  DevBuf<uint32_t> d_M;
  DevBuf<unsigned long long> d_drawn;
  // batch results for the host-pointer entry points
  DevBuf<double> d_bsum;
  DevBuf<unsigned long long> d_bcnt;
  uint32_t n_batch_valid = 0;  // matrices of the last batch / job call, still in d_bsum / d_bcnt (ngd_fetch_matrix)
  // ngd_run_job_dist / ngd_run_mult_batch_dist: the matrices of d_bsum / d_bcnt leave the device in chunks on a stream
  // of their own -- in the per-block-partials plan a group of replicates as soon as its reduction is over, beside the
  // reductions of the later groups -- into pinned memory of the engine's, and the tail of gen_dist() (host_util.cpp) works
  // the cells of a chunk as soon as it has landed
  struct OutStream {
    bool on = false, pdel = false;
    hipStream_t st = nullptr, st2 = nullptr;  // chunks alternate between two copy streams
    uint32_t n_chunk_seq = 0, n_landed = 0;    // chunks queued / declared landed so far in this call
    PinBuf<double> h_sum;
    PinBuf<uint64_t> h_cnt;
    uint32_t n_mat = 0, queued = 0;          // matrices of this call; matrices [0, queued) have their copies on st
    std::vector<hipEvent_t> pool;            // events, made on demand and kept
    uint32_t n_used = 0;
    std::vector<std::pair<hipEvent_t, uint32_t>> chunks;  // (the copy's event, matrices in host memory once it has happened)
    std::vector<uint64_t> cnt_mat;           // no --pairwise_del: a matrix's count (the sites it visits), ngsDist.cpp:362
    uint64_t evol_model = 0, tot_sites = 0;  // tot_sites > 0: the count of every cell (ngsDist.cpp:372-373)
    double *dist = nullptr;
    volatile uint64_t landed = 0;            // cells of h_sum (h_cnt) that are final: raised by the calling thread
    std::thread finisher;
    int finisher_rc = 0;
    double t0 = 0, t_call = 0;  // NGD_TRACE_OUT
  } out;
  DevBuf<double> staging;
  uint64_t staging_sites = 0;
  // raw-input pipeline: a ring of slots (RingSlot: a pinned host buffer, its device buffer, two events); the copies run on
  // a stream of their own (the copy engine never waits for a preparation kernel), K0 follows each on the engine's stream
  static constexpr int RING = 8;
  RingSlot ring[RING];
  uint64_t opt_stage_piece_mib = 32, opt_stage_ring = 6;  // NGD_OPT_STAGE_PIECE_MIB, NGD_OPT_STAGE_RING
  // NGD_OPT_EAGER_FULL: the plain full-data pass starts DURING a staged load -- whenever enough leading slices of the site
  // axis have all their sites prepared, they are accumulated on a low-priority stream of their own beside the copies and
  // preparation kernels of the pieces still arriving; the first ngd_run() then launches what is left and reduces
  bool opt_eager = false;
  hipStream_t st_eager = nullptr;
  hipEvent_t ev_eager = nullptr;
  uint64_t stage_prefix = 0;   // sites [0, stage_prefix) have been submitted, in order
  bool stage_in_order = true;
  uint32_t eager_slices = 0;   // slices [0, eager_slices) of the plain pass have been launched on st_eager
  bool eager_valid = false;
  bool eager_skip = false;     // ... as slices of the pass that leaves the unit-sum coordinate out (d_kgskip): the data set is not
                               // known to be *unit* before ngd_commit -- a plain pass of the other kind drops them
  hipStream_t st_copy[2] = {nullptr, nullptr};
  uint64_t n_staged = 0;
  int ring_slots = 0;
  std::thread ring_reaper;  // gives the ring back after ngd_commit, beside whatever the caller does next
  // The ring GROWS: its first buffer is made by the first ngd_stage_acquire, the others by a thread beside the load
  // (hipHostMalloc: 5 ms per 32-MiB buffer); the load turns through the buffers that exist (ring_ready of them)
  std::thread ring_maker;
  std::atomic<int> ring_ready{0};
  std::atomic<bool> ring_stop{false};  // the load is over: no more buffers are needed
  int ring_maker_rc = 0;
  int pin_cur = 0, pin_lent = -1;
  uint64_t pin_sites = 0;
  DevBuf<int> d_nan;
  bool committed = false;
  // the thread that maps the piece ranges (ngd_buffers.h PieceRange; dev_alloc_pieces, piece_worker)
  std::thread piece_thread;
  std::mutex piece_mu;
  std::condition_variable piece_cv;
  bool piece_done = true;  // nothing left to map (or the worker gave up: piece_rc)
  int piece_rc = 0;
  std::string piece_err;
  ngd_timing timing{};
  // plan options (ngd_set_option)
  uint64_t opt_boot_partials = 1, opt_boot_max_bytes = 0, opt_boot_wg = 4096, opt_boot_unaligned = 1, opt_em_batch = 1;
  uint64_t opt_em_spill = 1, opt_em_spill_bytes = 0;
  // the EM batch pass's result planes did not fit this device at this many elements: a request as large is not tried
  // again (0: nothing has failed) -- until ngd_drop_caches(), or until a smaller request (fewer matrices per pass) comes
  uint64_t em_batch_nofit_elems = 0;
  // EM bootstrap by spilled terms + one MFMA contraction (contract_mfma.hip): running sums and per-chunk NaN flags
  DevBuf<double> d_D;
  DevBuf<unsigned long long> d_nanflag;
  // ... its pair slots: groups of 16 consecutive columns of one row of a 64 x 64 tile, dealt to the groups that hold a
  // pair only; d_rowpg[tile * 64 + row] + g = slot group of the row's column group g (a signed 32-bit number: the first live
  // group's slot group minus that group's index), n_pg_spill = their number (+ padding to 4)
  DevBuf<uint32_t> d_rowpg;
  uint32_t n_pg_spill = 0, n_pg_live = 0;
  std::vector<hipEvent_t> ev_spill;  // per chunk: before the weights, the EM pass, the sanitiser, the contraction; + one at the end
  ngd_spill_timing spill_timing{};
  // windows along the genome (ngd_run_windows*): the segment-slab plan's slice table and window table (its partial
  // results, counts and slice weights borrow blk)
  DevBuf<uint64_t> d_segtab;
  DevBuf<unsigned long long> d_wintab;
  DevBuf<uint32_t> d_winblk;  // a job's replicates (ngd_run_windows_job*): [window][block] first slice of the block
  DevBuf<uint64_t> d_windesc;  // ... over windows of unequal length (ngd_run_windows_job_var*): [window][NGD_WIN_DESC]
  uint64_t opt_win_plan = 0, opt_win_max_bytes = 0;  // NGD_OPT_WIN_PLAN, NGD_OPT_WIN_MAX_BYTES
  ngd_windows_info win_info{};
  // NGD_OPT_EM_EXACT (engine_em_exact.hip): the plain pass of the table-driven EM kernel notes the (pair, site)s whose stop
  // is within 2^-36 of the tolerance; the host reruns them the reference's way and the pairs' sums are patched
  bool opt_em_exact = false;
  bool opt_em_exact_boot = false;      // value 2: the calls that weight sites are served too (run_impl: noting plans only)
  bool opt_em_exact_win = false;       // NGD_OPT_EM_EXACT_WIN: while opt_em_exact is on, the windowed calls are served too
  uint64_t note_cap = 1ull << 20;      // entries the list is to hold (NGD_OPT_EM_EXACT_CAP; grown by a pass that noted more)
  DevBuf<unsigned long long> d_note;   // the note buffer (ngd_internal.h): count, capacity, the entries
  unsigned long long note_head[NGD_NOTE_HEAD] = {0, 0, 0, 0};  // what a pass starts from (alive while its copy is in flight)
  DevBuf<double> d_note_gl, d_note_delta;  // the entries' likelihoods; the corrections in (pair, site) order
  DevBuf<unsigned long long> d_note_pair;  // ... the distinct pairs' indices
  DevBuf<uint32_t> d_note_first;           // ... and where each pair's corrections start (+ one past the last)
  DevBuf<unsigned long long> d_note_site;  // ... and the corrections' sites (value 2: a matrix weights each by its block)
  DevBuf<unsigned long long> d_note_win;   // NGD_OPT_EM_EXACT_WIN: [window of the batch][2] = lo, hi (k_note_patch_win)
  ngd_em_exact_info exact_info{};
  std::vector<ngd_em_exact_entry> exact_entries;  // of the last plain pass, sorted
  // a windowed call under NGD_OPT_EM_EXACT_WIN notes batch by batch, pass by pass (window by window in the per-window
  // plan): what the call has gathered so far, while exact_info / exact_entries hold the launch at hand
  ngd_em_exact_info call_info{};
  std::vector<ngd_em_exact_entry> call_entries;
  // groups of individuals (ngd_set_groups): the grouping as group_reduce.hip reads it, and the reduction's scratch and
  // results -- everything here goes when the grouping is cleared
  struct Groups {
    uint32_t n_groups = 0, n_work = 0;  // n_groups 0: no grouping set
    uint64_t n_gp = 0;
    DevBuf<uint32_t> d_members, d_off, d_gp_first;
    DevBuf<ngd_group_work> d_work;
    DevBuf<double> d_part_sum, d_mean;
    DevBuf<unsigned long long> d_part_cnt, d_used;
    DevBuf<double> d_keep_mean;              // the means of a call's every matrix, kept for the summaries (groups_reduce, mean == NULL)
    DevBuf<unsigned long long> d_keep_used;
    double ms = 0;  // ngd_last_groups_ms
  } grp;
  // bootstrap summaries (engine_boot_stats.hip): a chunk of sets' statistics and counts on their way to the host
  struct BootStats {
    DevBuf<double> d_stats;
    DevBuf<unsigned long long> d_used;
    double ms = 0;  // ngd_last_boot_stats_ms
  } bst;
  // neighbour-joining trees (engine_nj.hip): a chunk of matrices' working copies (n x n doubles each) and their records
  struct Nj {
    DevBuf<double> d_work, d_len;
    DevBuf<int32_t> d_child;
    DevBuf<uint32_t> d_status;
    uint64_t max_bytes = 0;  // NGD_OPT_NJ_MAX_BYTES
    double ms = 0;           // ngd_last_nj_ms
  } nj;
  // classical MDS (engine_mds.hip): a chunk of matrices' working copies, their vectors' scratch and their outputs
  struct Mds {
    DevBuf<double> d_work, d_aux, d_eig, d_vec, d_tot;
    DevBuf<uint32_t> d_status;
    uint64_t max_bytes = 0;  // NGD_OPT_MDS_MAX_BYTES
    double ms = 0;           // ngd_last_mds_ms
  } mds;
  // ... and the alignment of a call's replicates (engine_mds.hip): the cells of all its matrices -- coordinates [K][n], then
  // the K eigenvalues --, their status and their fit
  struct MdsAlign {
    DevBuf<double> d_cells, d_fit;
    DevBuf<uint32_t> d_status;
    double ms = 0;  // ngd_last_mds_align_ms
  } mal;
  // comparison of windows (engine_win_cmp.hip): the operand Z and the partials, resident for a whole call; the call's means,
  // status and Gram matrix on their way to the host
  struct WinCmp {
    DevBuf<double> Z, part, d_mean, d_gram;
    DevBuf<uint32_t> d_status;
    uint64_t max_bytes = 0;         // NGD_OPT_WIN_CMP_MAX_BYTES
    double ms[4] = {0, 0, 0, 0};    // ngd_last_win_cmp_ms: stats, pack, gram, sum
  } wcmp;
};

// what the launchers of accum_mfma.hip / accum_em_table.hip are handed of the engine (ngd_internal.h)
inline ngd_mfma_engine mfma_engine(const ngd_engine *e) {
  return ngd_mfma_engine{e->g, e->d_jobs, e->n_wg, e->exact_shapes, e->wg_waves, e->d_clk};
}
inline ngd_emt_common emt_common(const ngd_engine *e) {
  return ngd_emt_common{e->g, e->PA, e->sc, e->cfg.pairwise_del, e->em_shape, e->d_tiles64, e->n_tiles64, e->d_emcnt};
}

// The operand images and slabs (a GiB and more): an address range reserved at once, physical pieces of 256 MiB created,
// mapped and zeroed behind it by a thread of the engine's own, in the order a load needs them.
// [measured, round 6, tools/alloc_cost.hip, rocprofv3 --hip-trace of the C++ host, gpurun_out/r6/e2e_4.jsonl] On a box whose
// device memory has been used before -- every box after its first few jobs -- the driver clears memory as it hands it out:
// hipMalloc of cfg 3's 24.6 GB image takes 0.3 ms on pristine memory and 1.0-1.2 s otherwise (hiptrace_cfg3_3: 984 ms in
// ONE hipMalloc; ~30 GB/s), while the link moves the file at 57 GB/s.  One allocation up front therefore cost more than the
// whole load; piece by piece, beside the load, it costs max(clearing, load).  The pieces read at the same 5.3 TB/s as one
// hipMalloc (tools/alloc_cost.hip) and K1m runs at the same 45.6 ms on them (gpurun_out/r6/bench_cfg3_vmm.json).
// Anything the piecewise calls refuse up front falls back to hipMalloc; a failure later (out of memory) is reported by
// the first call that needs the memory (ngd_stage_submit / ngd_upload_* / ngd_commit: NGD_E_NOMEM).
// (pieces of ONE size per range: hipMemSetAccess refuses a shorter last piece -- [measured] 1 GiB + 512 MiB: invalid
// argument; 15 x 256 MiB: fine -- so a range is rounded up to whole pieces, at most 256 MiB more than asked for)
template <typename T>
int dev_alloc_pieces(ngd_engine *e, DevBuf<T> &buf, uint64_t count, bool zero, PieceKind kind = PIECE_WHOLE,
                     uint64_t bytes_per_site = 0) {
  const uint64_t bytes = count * sizeof(T);
  if (bytes < ((uint64_t)512 << 20)) return buf.alloc(e, count, zero);
  hipMemAllocationProp prop = {};
  prop.type = hipMemAllocationTypePinned;
  prop.location.type = hipMemLocationTypeDevice;
  prop.location.id = e->device;
  size_t gran = 0;
  if (hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityRecommended) != hipSuccess || !gran) {
    (void)hipGetLastError();
    return buf.alloc(e, count, zero);
  }
  if (kPiece % gran) return buf.alloc(e, count, zero);
  std::unique_ptr<PieceRange> r(new PieceRange());
  r->size = (size_t)((bytes + kPiece - 1) / kPiece * kPiece);
  r->zero = zero;
  r->kind = kind;
  r->bytes_per_site = bytes_per_site;
  if (hipMemAddressReserve(&r->va, r->size, 0, nullptr, 0) != hipSuccess) {
    (void)hipGetLastError();
    return buf.alloc(e, count, zero);
  }
  if (int rc = buf.release()) return rc;
  buf.adopt(e, r.get(), count);
  e->piece_ranges.push_back(std::move(r));
  return NGD_OK;
}

// ---- what one unit asks of another: C++ linkage, and hidden -- none of it enters the dynamic symbol table ----
// (the entry points a unit defines take their C linkage from their declarations in include/ngsdist_amd.h; everything
// else in a unit is static)
// engine_mem.hip
int piece_start(ngd_engine *e);
int piece_join(ngd_engine *e);
int piece_wait_sites(ngd_engine *e, uint64_t s_end);
// engine_create.hip
int spill_slot_map(ngd_engine *e, const std::vector<ngd_tile> &tiles64);  // d_rowpg, n_pg_spill, n_pg_live
// engine_stage.hip
void stage_reap(ngd_engine *e);
void ring_maker_join(ngd_engine *e);
bool eager_supported(const ngd_engine *e);
void launch_plain_slices(ngd_engine *e, hipStream_t st, uint32_t ks0, uint32_t n, bool beside_a_load, bool unit_skip);
int eager_discard(ngd_engine *e);
// engine_fixup.hip
int fix_collect(ngd_engine *e, uint32_t n, bool all, std::vector<ngd_fix_tile> &tiles, std::vector<unsigned long long> &singles);
int fixup_pass(ngd_engine *e, const uint32_t *ws, uint64_t s_hi, double *d_sum, uint64_t sites_per_slice,
               uint32_t n_slab_slices, bool *patched, const unsigned long long *d_cnt = nullptr, double thr = 0.0);
// engine_plans.hip
int mfma_fault(ngd_engine *e);
void read_timing(ngd_engine *e, uint64_t n_eff, uint32_t launches, bool add);
int pass_impl(ngd_engine *e, const uint32_t *mult, uint32_t mult_max, uint64_t n_blocks, uint64_t block_size,
              uint64_t n_drawn, double *d_sum, unsigned long long *d_cnt, bool add_timing);
int run_impl(ngd_engine *e, const uint64_t *block_maps, const uint32_t *mult_in, uint32_t n_rep, bool lead_full,
             uint64_t n_blocks, uint64_t block_size, double *d_sum, unsigned long long *d_cnt);
// engine_em_exact.hip
int em_exact_refuse(const ngd_engine *e, const char *who);  // NGD_E_INVALID while the option is on: `who` is not served
int em_exact_set(ngd_engine *e, uint64_t value);            // NGD_OPT_EM_EXACT
int em_exact_begin(ngd_engine *e);                          // before the noting pass: the list is there and empty
int em_exact_finish(ngd_engine *e, double *d_sum, bool *again);  // after it (stream idle): recheck + patch, or grow the list
int em_exact_refuse_weighted(const ngd_engine *e, const char *who);  // as em_exact_refuse, but value 2 lets `who` through
// value 2, after a plan's noting launch (stream idle): recheck + the weighted patch of every matrix of d_sum, or grow the list
int em_exact_finish_w(ngd_engine *e, double *d_sum, const ngd_note_weights &w, bool *again);
void em_exact_merge(ngd_engine *e, const std::vector<ngd_em_exact_entry> &first, const ngd_em_exact_info &info1);
// NGD_OPT_EM_EXACT_WIN
int em_exact_win_set(ngd_engine *e, uint64_t value);
inline bool em_exact_win(const ngd_engine *e) { return e->opt_em_exact && e->opt_em_exact_win; }  // windowed calls note
int em_exact_refuse_windows(const ngd_engine *e, const char *who, bool job);  // em_exact_refuse, unless the option serves `who`
// after a batch's noting launch and its banded reductions (stream idle): recheck + k_note_patch_win, or grow the list
int em_exact_finish_win(ngd_engine *e, double *d_sum, const uint64_t *lo, const uint64_t *hi, ngd_note_win w, bool *again);
void em_exact_call_begin(ngd_engine *e);  // a windowed call starts: nothing gathered
void em_exact_call_add(ngd_engine *e);    // exact_info / exact_entries join the call's union, which both then hold
// engine_out.hip
bool out_trace();
double out_now();
int out_queue(ngd_engine *e, uint32_t m_hi);
int out_advance(ngd_engine *e);
int out_requeue(ngd_engine *e);
void out_start_finisher(ngd_engine *e);
int copy_out(ngd_engine *e, uint32_t n_mat, const double *d_sum, const unsigned long long *d_cnt, double *sum,
             uint64_t *cnt);
int batch_buffers(ngd_engine *e, uint32_t n_rep);
int run_to_host(ngd_engine *e, const uint64_t *block_maps, const uint32_t *mult, uint32_t n_rep, bool lead_full,
                uint64_t n_blocks, uint64_t block_size, uint32_t n_batch, double *sum, uint64_t *cnt);
int run_dist(ngd_engine *e, const uint64_t *block_maps, const uint32_t *mult, uint32_t n_rep, bool lead_full,
             uint64_t n_blocks, uint64_t block_size, uint64_t tot_sites, uint64_t evol_model, double *dist, const char *who);
// what every call that finishes matrices refuses (tot_sites with pairwise deletion, an unknown model, an engine that owns
// a share of the pairs); no_what ends the last one's message -- NULL where the caller has words of its own for such an
// engine, or the check of its windows has refused it already
int finish_refuse(const ngd_engine *e, uint64_t tot_sites, uint64_t evol_model, const std::string &who, const char *no_what);

// ---- tails: what a call does on the device with the matrices it has just left in the batch buffers ----
// A tail takes the matrices standing in d_bsum / d_bcnt as [n_set][n_mat][n_pairs] -- a job's one set, the sets of a group
// of windows -- where set0 is the first of them among the call's sets: the tail owns its outputs and their offsets.  Each
// unit builds its own from a call's outputs and parameters (engine_groups.hip, engine_boot_stats.hip, engine_nj.hip, engine_mds.hip; the
// copy and the distances in engine_windows.hip) and hands it to one of the two drivers; everything is checked before.
using Tail = std::function<int(uint64_t set0, uint64_t n_set, uint64_t n_mat)>;
// engine_out.hip: ngd_run_job_device into the batch buffers, where the matrices stay (ngd_fetch_matrix), then tail(0, 1,
// n_rep + 1); n_rep == 0: the full-data matrix alone, the maps are not read
int job_tail(ngd_engine *e, const uint64_t *block_maps, uint32_t n_rep, uint64_t n_blocks, uint64_t block_size, const Tail &tail);
// engine_windows.hip: the arguments of ngd_run_windows_job_var (n_rep == 0: of ngd_run_windows, the rest is not read) ...
struct WinJobArgs {
  const uint64_t *lo, *hi;
  uint64_t n_win;
  const uint64_t *maps;
  uint64_t maps_len;
  const uint64_t *map_off;
  uint32_t n_rep;
  uint64_t block_size;
};
// ... checked -- as a job's (that check refuses under NGD_OPT_EM_EXACT), or with n_rep == 0 as ngd_run_windows' unless the
// call is a job form whatever its n_rep (job_form) -- then what `refuse` refuses (if given: the tail's own, where the call's
// order of refusals puts them after the windows'), then the windows in groups through the batch buffers, the tail after each
int windows_tail(ngd_engine *e, const WinJobArgs &a, bool job_form, const char *who, const Tail &tail,
                 const std::function<int()> &refuse = nullptr);
// engine_groups.hip: [n_mat][n_pairs] device matrices -> mean / used [n_mat][n_gp] in host memory; mean == NULL: they stay
// on the device instead, grp.d_keep_mean / d_keep_used [n_mat][n_gp], for the summaries (the arguments are checked)
int groups_reduce(ngd_engine *e, const double *d_sum, const unsigned long long *d_cnt, uint64_t n_mat, uint64_t tot_sites,
                  uint64_t evol_model, double *mean, uint64_t *used);
// engine_boot_stats.hip: what every call that summarises refuses, before anything is launched (`groups`: without a grouping
// too); the two ranks' fractions of the interval on the way
struct BootCi {
  double p_lo, p_hi;
};
int boot_refuse(const ngd_engine *e, const void *stats, const void *used, uint64_t n_mat, double ci, uint64_t tot_sites,
                uint64_t evol_model, bool groups, const char *who, BootCi &out);
// ... and [n_set][n_mat][n_cells] device matrices -> stats [n_set][5][n_cells] / used [n_set][n_cells] in host memory; d_cnt
// and the two arguments of ngd_finish for sums and counts, `values` for cells as they are (the arguments are checked);
// adds its kernels' time to bst.ms
int boot_reduce(ngd_engine *e, const double *d_a, const unsigned long long *d_cnt, bool values, uint64_t n_set, uint64_t n_mat,
                uint64_t n_cells, uint64_t tot_sites, uint64_t evol_model, BootCi ci, double *stats, uint64_t *used);
// engine_nj.hip: matrix 0 of each of the n_set sets of [n_set][n_mat][n_pairs] sums and counts, finished on the host into
// dist0 [n_set][n_pairs] (ngd_finish's bits: what the tails that keep their matrices on the device hand out beside them)
int tail_dist0(ngd_engine *e, const double *d_sum, const unsigned long long *d_cnt, uint64_t n_set, uint64_t n_mat, uint64_t tot_sites,
               uint64_t evol_model, double *dist0);
#pragma GCC visibility pop
