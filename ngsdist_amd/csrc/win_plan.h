// win_plan.h -- what the segment-slab plan of the windowed calls (engine_windows.hip windows_slab) tells the device: which
// windows form a batch under the memory budget, the slices of the batch's ONE accumulation pass, and the tables the banded
// reductions read.  Host arithmetic only: nothing of HIP is included, and what the planner needs of the engine arrives as
// plain values (win_env), so that a plain C++ program can plan too (tests/win_plan/win_plan_main.cpp).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <iterator>
#include <vector>

#include "ngd_layout.h"

// The slice table: an entry per segment of sites [s_lo, s_hi) -- k-groups [kg0, kg1) = [3 s_lo / 4, ceil(3 s_hi / 4)), or
// rounded outwards to whole periods of four sites in a congruent engine's image (win_env::quad, ngd_layout.h) -- its
// 0/1 weights (d3[coordinate] inside the segment, 0 outside) at k-group woff of the weight array, kg1 - kg0 + 1 + NGD_KG_TAIL
// k-groups of them (the operand pipeline's run-ahead reads past kg1).  The table-driven EM kernel and k_count_blocks read
// s_lo / s_hi alone (an EM engine's table leaves the other entries 0).
#define NGD_SEG_STRIDE 5
#define NGD_SEG_KG0 0
#define NGD_SEG_KG1 1
#define NGD_SEG_WOFF 2
#define NGD_SEG_SLO 3
#define NGD_SEG_SHI 4

// a job (ngd_run_windows_job*): the replicates every window of the call draws
struct WinBoot {
  uint32_t n_rep;
  uint64_t n_blocks, q;
  const uint32_t *mult;  // [n_rep][n_blocks]: draws of block b in replicate r
};

struct win_env {
  uint64_t plane;  // doubles of one partial result: n_pad * n_pad
  bool em;         // the table-driven EM kernel (else the MFMA kernel)
  bool pdel;       // --pairwise_del
  uint32_t n_ks;   // slices of a plain pass (the EM kernel's piece rule)
  uint64_t tail;   // NGD_KG_TAIL
  uint32_t chunk;  // a job: ngd_reduce_chunk(n_rep)
  bool quad = false;  // the MFMA kernel on the congruent image: its layout (ngd_layout.h)
};

// a job's weights Wt[b][r]: replicates per block, zero padded to whole chunks
inline uint32_t win_weight_stride(const win_env &v, const WinBoot &bt) { return (bt.n_rep + v.chunk - 1) / v.chunk * v.chunk; }

// the boundaries a window brings to its batch, ascending: its ends, and in a job the starts of its blocks
inline void win_boundaries(uint64_t lo, uint64_t hi, const WinBoot *bt, std::vector<uint64_t> &wb) {
  wb.clear();
  wb.push_back(lo);
  for (uint64_t b = 1; bt && b <= bt->n_blocks; b++) wb.push_back(lo + b * bt->q);
  if (wb.back() != hi) wb.push_back(hi);
}

// bytes of one batch: partial results (slices padded to the XCD deal's eights), counts, slice weights and tables.  The EM
// kernel: a plane per segment, counts, tables -- no k-group weights, no padding slices.  A job (bt != NULL): + every
// window's table of block starts and the replicates' weights (doubles; uint32 for the counts).
inline uint64_t win_batch_bytes(const win_env &v, uint64_t n_seg, uint64_t span, uint64_t n_win, const WinBoot *bt) {
  const uint64_t n_ks = (n_seg + 7) / 8 * 8, cnt = v.pdel ? n_seg * v.plane * 4 : 0;
  const uint64_t job = bt ? n_win * (bt->n_blocks + 1) * 4 + bt->n_blocks * win_weight_stride(v, *bt) * (v.pdel ? 12 : 8) : 0;
  if (v.em) return n_seg * v.plane * 8 + cnt + n_seg * NGD_SEG_STRIDE * 8 + n_win * 16 + job;
  // (a segment's k-groups: at most 3 len / 4 + 2, or + 6 rounded outwards to periods, + 1 + tail of run-ahead)
  const uint64_t wkg = 3 * span / 4 + n_ks * ((v.quad ? 7 : 3) + v.tail) + 1 + v.tail;
  return n_ks * v.plane * 8 + cnt + wkg * 32 + n_ks * NGD_SEG_STRIDE * 8 + n_win * 16 + job;
}

// false: some window alone does not fit the budget (a job's window: its blocks and its tail)
inline bool win_each_fits(const win_env &v, const uint64_t *lo, const uint64_t *hi, uint64_t n_win, const WinBoot *bt, uint64_t budget) {
  for (uint64_t w = 0; w < n_win; w++)
    if (win_batch_bytes(v, bt ? bt->n_blocks + 1 : 1, hi[w] - lo[w], 1, bt) > budget) return false;
  return true;
}

// One batch: windows [a, b) of the call.  Slices [0, n_seg) are real, [n_seg, n_ks) the MFMA launch's padding: no k-group,
// no sites, their weights the last 1 + tail k-groups of the w_total.
struct win_batch {
  uint64_t a = 0, b = 0, hi_max = 0;  // (hi_max: the last site any of its windows reaches)
  uint64_t n_seg = 0, n_ks = 0, max_wkg = 0, w_total = 0;
  std::vector<uint64_t> tab;           // [n_ks][NGD_SEG_STRIDE]
  std::vector<unsigned long long> wt;  // k_reduce_band: [b - a][2] = window's slices first | end << 32, its sites hi - lo
  std::vector<uint32_t> blk;  // a job, k_reduce_band_w: [b - a][n_blocks + 1] the first slice of each block, the end of the last
  // (the planner's scratch, kept from batch to batch: the batch's boundaries x, ascending, and what is counted along them)
  std::vector<uint64_t> x, wb, merged;
  std::vector<int64_t> cover;
  std::vector<uint32_t> seg_of, seg_end;
};

// The tables of the batch [a, b) whose distinct boundaries are p.x, ascending: its slice table and every window's range of
// slices.  bytes(n_seg): what the batch takes with n_seg slices (the EM kernel's pieces must fit the budget too).
template <class Bytes>
inline void win_plan_slices(const win_env &v, const uint64_t *lo, const uint64_t *hi, uint64_t a, uint64_t b, uint64_t hi_max,
                            uint64_t budget, Bytes bytes, win_batch &p) {
  std::vector<uint64_t> &x = p.x;
  const uint64_t nb = b - a, n_x = x.size();
  auto at = [&](uint64_t s) { return (uint64_t)(std::lower_bound(x.begin(), x.end(), s) - x.begin()); };
  // interval k = [x[k], x[k + 1]) is a segment if some window of the batch covers it
  std::vector<int64_t> &cover = p.cover;
  cover.assign(n_x, 0);
  for (uint64_t w = a; w < b; w++) { cover[at(lo[w])]++; cover[at(hi[w])]--; }
  for (uint64_t k = 1; k < n_x; k++) cover[k] += cover[k - 1];
  auto covered = [&](uint64_t k) { return cover[k] > 0; };
  // EM kernel: an interval's slices are pieces of at most `piece` sites -- the covered sites over the slices of a plain
  // pass, 64 sites or more (ngd_create's bound) -- unless the planes of the pieces would not fit the budget
  uint64_t piece = ~0ull;
  if (v.em) {
    uint64_t sites = 0, n_cov = 0, n_cut = 0;
    for (uint64_t k = 0; k + 1 < n_x; k++)
      if (covered(k)) { sites += x[k + 1] - x[k]; n_cov++; }
    piece = std::max<uint64_t>(64, (sites + v.n_ks - 1) / std::max<uint32_t>(1, v.n_ks));
    for (uint64_t k = 0; k + 1 < n_x; k++)
      if (covered(k)) n_cut += (x[k + 1] - x[k] - 1) / piece + 1;
    if (n_cut > n_cov && (bytes(n_cut) > budget || n_cut >= (1ull << 30))) piece = ~0ull;
  }
  // the slice table; interval k = slices [seg_of[k], seg_end[k]), none where no window covers it
  std::vector<uint32_t> &seg_of = p.seg_of, &seg_end = p.seg_end;
  seg_of.assign(n_x, 0);
  seg_end.assign(n_x, 0);
  uint64_t n_seg = 0, wkg = 0;
  p.tab.clear();
  p.max_wkg = 0;
  for (uint64_t k = 0; k + 1 < n_x; k++) {
    seg_of[k] = seg_end[k] = (uint32_t)n_seg;
    if (!covered(k)) continue;
    if (v.em) {  // (the k-group entries are the MFMA kernel's: not read)
      const uint64_t len = x[k + 1] - x[k], n_p = len <= piece ? 1 : (len - 1) / piece + 1, per = (len + n_p - 1) / n_p;
      for (uint64_t s = x[k]; s < x[k + 1]; s += per, n_seg++) p.tab.insert(p.tab.end(), {0, 0, 0, s, std::min(s + per, x[k + 1])});
    } else {
      const uint64_t kg0 = ngd_kg_lo(x[k], v.quad), kg1 = ngd_kg_hi(x[k + 1], v.quad), n_wkg = kg1 - kg0 + 1 + v.tail;
      p.tab.insert(p.tab.end(), {kg0, kg1, wkg, x[k], x[k + 1]});
      wkg += n_wkg;
      p.max_wkg = std::max(p.max_wkg, n_wkg);
      n_seg++;
    }
    seg_end[k] = (uint32_t)n_seg;
  }
  seg_of[n_x - 1] = seg_end[n_x - 1] = (uint32_t)n_seg;  // (the last boundary: where the slices end)
  // (the XCD deal of accum_mfma.hip; padding slices have no k-group and no sites.  The EM launch needs none.)
  const uint64_t n_ks = v.em ? n_seg : (n_seg + 7) / 8 * 8;
  for (uint64_t k = n_seg; k < n_ks; k++) p.tab.insert(p.tab.end(), {0, 0, wkg, 0, 0});
  p.a = a; p.b = b; p.hi_max = hi_max;
  p.n_seg = n_seg; p.n_ks = n_ks; p.w_total = wkg + 1 + v.tail;
  p.wt.resize(2 * nb);
  for (uint64_t w = a; w < b; w++) {
    const uint64_t f = seg_of[at(lo[w])], l = seg_end[at(hi[w]) - 1];
    p.wt[2 * (w - a)] = f | (l << 32);
    p.wt[2 * (w - a) + 1] = hi[w] - lo[w];
  }
}

// The next batch of windows lo[] / hi[] (starts not decreasing, each alone within the budget): from window `a` on as many
// as fit the budget, their segments bounded by their distinct boundaries - 1.
inline void win_plan_batch(const win_env &v, const uint64_t *lo, const uint64_t *hi, uint64_t n_win, uint64_t a, uint64_t budget,
                           const WinBoot *bt, win_batch &p) {
  std::vector<uint64_t> &x = p.x, &wb = p.wb, &merged = p.merged;  // (one merge of two sorted lists per window)
  x.clear();
  uint64_t b = a, hi_max = 0;
  while (b < n_win) {
    win_boundaries(lo[b], hi[b], bt, wb);
    merged.clear();
    std::set_union(x.begin(), x.end(), wb.begin(), wb.end(), std::back_inserter(merged));
    const uint64_t n_seg_ub = merged.size() - 1, hm = std::max(hi_max, hi[b]);
    if (b > a && (win_batch_bytes(v, n_seg_ub, hm - lo[a], b + 1 - a, bt) > budget || n_seg_ub >= (1ull << 30))) break;
    x.swap(merged);
    hi_max = hm;
    b++;
  }
  win_plan_slices(v, lo, hi, a, b, hi_max, budget,
                  [&](uint64_t n_seg) { return win_batch_bytes(v, n_seg, hi_max - lo[a], b - a, bt); }, p);
  const std::vector<uint32_t> &seg_of = p.seg_of;
  auto at = [&](uint64_t s) { return (uint64_t)(std::lower_bound(x.begin(), x.end(), s) - x.begin()); };
  p.blk.clear();
  if (!bt) return;
  const uint64_t nb = b - a;
  p.blk.resize(nb * (bt->n_blocks + 1));
  for (uint64_t w = a; w < b; w++) {
    uint64_t i = at(lo[w]);  // (the window's block starts ascend: one walk along the boundaries)
    for (uint64_t k = 0; k <= bt->n_blocks; k++) {
      while (x[i] < lo[w] + k * bt->q) i++;
      p.blk[(w - a) * (bt->n_blocks + 1) + k] = seg_of[i];
    }
  }
}

// ---- a job over windows of UNEQUAL length (ngd_run_windows_job_var*) ----
// Window w has n_blocks_w = (hi - lo) / q blocks and draws the maps of its class: windows that share map_off and n_blocks_w
// share one weight table.  k_reduce_band_wv reads a descriptor per window instead of one n_blocks / table / count per call.
#define NGD_WIN_DESC 4       // words of a window's descriptor:
#define NGD_WIN_DESC_BLK 0   //  where its row of block starts begins in blk (n_blocks_w + 1 entries)
#define NGD_WIN_DESC_NB 1    //  n_blocks_w
#define NGD_WIN_DESC_WT 2    //  where its weight table begins (elements: rows of `stride` weights)
#define NGD_WIN_DESC_VIS 3   //  the sites a replicate visits, n_blocks_w q
#define NGD_WIN_NO_CLASS 0xffffffffu

struct WinBootVar {
  uint32_t n_rep;
  uint64_t q;
  uint32_t n_cls;
  const uint32_t *cls;         // [n_win] the window's class, NGD_WIN_NO_CLASS for a window shorter than one block
  const uint64_t *cls_blocks;  // [n_cls] n_blocks of the class
  const uint64_t *cls_mult;    // [n_cls] where `mult` holds the class's [n_rep][n_blocks] draws
  const uint32_t *mult;
  WinBootVar from(uint64_t w0) const { WinBootVar t = *this; t.cls += w0; return t; }  // the same job, windows w0 on
};

inline uint32_t win_weight_stride_var(const win_env &v, uint32_t n_rep) { return (n_rep + v.chunk - 1) / v.chunk * v.chunk; }

// bytes of one batch: the plain batch's + the rows of block starts, the descriptors, and wt_rows rows of weights
inline uint64_t win_batch_bytes_var(const win_env &v, uint64_t n_seg, uint64_t span, uint64_t n_win, uint64_t blk_entries,
                                    uint64_t wt_rows, uint32_t n_rep) {
  return win_batch_bytes(v, n_seg, span, n_win, nullptr) + blk_entries * 4 + n_win * NGD_WIN_DESC * 8 +
         wt_rows * win_weight_stride_var(v, n_rep) * (v.pdel ? 12 : 8);
}

inline bool win_each_fits_var(const win_env &v, const uint64_t *lo, const uint64_t *hi, uint64_t n_win, const WinBootVar &bv,
                              uint64_t budget) {
  for (uint64_t w = 0; w < n_win; w++) {
    const uint64_t n_blocks = (hi[w] - lo[w]) / bv.q;
    if (win_batch_bytes_var(v, n_blocks + 1, hi[w] - lo[w], 1, n_blocks + 1, n_blocks, bv.n_rep) > budget) return false;
  }
  return true;
}

struct win_batch_var : win_batch {
  // blk: every window's row of block starts, one after the other (a window with no block: its first slice alone)
  std::vector<uint64_t> desc;            // [b - a][NGD_WIN_DESC]
  std::vector<uint32_t> cls_list;        // the classes the batch holds, in the order its windows bring them
  std::vector<uint64_t> cls_row;         // [n_cls] the first row of the class's weights in the batch's table, ~0: not held
  uint64_t wt_rows = 0;                  // rows of the batch's weight table
};

// every boundary the windows of one call bring, ascending and distinct: their block starts and ends
inline void win_call_boundaries_var(const uint64_t *lo, const uint64_t *hi, uint64_t n_win, uint64_t q, std::vector<uint64_t> &all) {
  all.clear();
  for (uint64_t w = 0; w < n_win; w++) {
    if (w && lo[w] == lo[w - 1] && hi[w] == hi[w - 1]) continue;  // (a window that comes again brings nothing new)
    for (uint64_t s = lo[w]; s + q <= hi[w]; s += q) all.push_back(s);
    all.push_back(lo[w] + (hi[w] - lo[w]) / q * q);
    all.push_back(hi[w]);
  }
  std::sort(all.begin(), all.end());
  all.erase(std::unique(all.begin(), all.end()), all.end());
}

// The next batch, as win_plan_batch -- but its slices are cut by the boundaries of EVERY window of the call (`all`,
// win_call_boundaries_var) that fall inside its span, not by its own windows' alone: a block is then added up from the same
// slices whatever the budget makes of the batches, and the MFMA kernel's replicates carry the same bits under any
// NGD_OPT_WIN_MAX_BYTES.  (The EM kernel's pieces of a long slice still follow the batch.)  A window of a neighbouring batch
// that reaches into this one costs it a few more slices; with no budget `all` is what the windows' own merge gives.
inline void win_plan_batch_var(const win_env &v, const uint64_t *lo, const uint64_t *hi, uint64_t n_win, uint64_t a, uint64_t budget,
                               const WinBootVar &bv, const std::vector<uint64_t> &all, win_batch_var &p) {
  std::vector<uint64_t> &x = p.x;
  p.cls_row.assign(bv.n_cls, ~0ull);
  p.cls_list.clear();
  const auto first = std::lower_bound(all.begin(), all.end(), lo[a]);
  uint64_t b = a, hi_max = 0, blk_entries = 0, wt_rows = 0;
  while (b < n_win) {
    const uint64_t n_blocks = (hi[b] - lo[b]) / bv.q, hm = std::max(hi_max, hi[b]);
    const uint64_t n_seg_ub = (uint64_t)(std::upper_bound(first, all.end(), hm) - first) - 1;
    const bool fresh = n_blocks && p.cls_row[bv.cls[b]] == ~0ull;
    const uint64_t be = blk_entries + n_blocks + 1, wr = wt_rows + (fresh ? n_blocks : 0);
    if (b > a && (win_batch_bytes_var(v, n_seg_ub, hm - lo[a], b + 1 - a, be, wr, bv.n_rep) > budget || n_seg_ub >= (1ull << 30))) break;
    if (fresh) { p.cls_row[bv.cls[b]] = wt_rows; p.cls_list.push_back(bv.cls[b]); }
    blk_entries = be;
    wt_rows = wr;
    hi_max = hm;
    b++;
  }
  x.assign(first, std::upper_bound(first, all.end(), hi_max));
  p.wt_rows = wt_rows;
  win_plan_slices(v, lo, hi, a, b, hi_max, budget,
                  [&](uint64_t n_seg) { return win_batch_bytes_var(v, n_seg, hi_max - lo[a], b - a, blk_entries, wt_rows, bv.n_rep); }, p);
  auto at = [&](uint64_t s) { return (uint64_t)(std::lower_bound(x.begin(), x.end(), s) - x.begin()); };
  const uint32_t stride = win_weight_stride_var(v, bv.n_rep);
  p.blk.clear();
  p.desc.clear();
  for (uint64_t w = a; w < b; w++) {
    const uint64_t n_blocks = (hi[w] - lo[w]) / bv.q;
    p.desc.insert(p.desc.end(), {p.blk.size(), n_blocks, n_blocks ? p.cls_row[bv.cls[w]] * stride : 0, n_blocks * bv.q});
    uint64_t i = at(lo[w]);
    for (uint64_t k = 0; k <= n_blocks; k++) {
      while (x[i] < lo[w] + k * bv.q) i++;
      p.blk.push_back(p.seg_of[i]);
    }
  }
}
