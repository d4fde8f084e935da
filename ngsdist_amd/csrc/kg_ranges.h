// kg_ranges.h -- how a single-image pass walks the k-groups of the second operand image, which is formed a range at a time
// into a scratch (engine_plans.hip accumulate_single_image; the two by-pass routes of engine_fixup.hip).  Host arithmetic
// only: nothing of HIP is included, so that a plain C++ program can walk the ranges too (tests/kg_ranges/kg_ranges_main.cpp).
#pragma once
#include <stdint.h>

#include <algorithm>

// A whole pass in ranges: the piece of a range one slice takes (k-groups: whole pipeline trips, and long enough to carry
// a block's 128 KB of running sums in and out) so that a range is about `span` k-groups.
inline uint64_t qb_piece(uint64_t kg_lim, uint32_t n_ks, uint64_t span, uint64_t *n_ranges) {
  uint64_t r = std::max<uint64_t>(1, (kg_lim + span - 1) / span);
  const uint64_t piece = std::max<uint64_t>(64, ((kg_lim + r * n_ks - 1) / (r * n_ks) + 3) / 4 * 4);
  *n_ranges = std::max<uint64_t>(1, (kg_lim + piece * n_ks - 1) / (piece * n_ks));
  return piece;
}

// The ranges of a whole pass over k-groups [rest0, kg_lim) (the engine keeps the head [0, rest0) of the second image
// resident): EVERY slice takes `piece` k-groups of every range [lo, hi), so that each launch has the pass's full grid.
// None when kg_lim <= rest0.
struct kg_pass_ranges {
  uint64_t kg_lim, rest0, n_ks, piece = 0, n_ranges = 0;
  kg_pass_ranges(uint64_t kg_lim_, uint32_t n_ks_, uint64_t span, uint64_t rest0_) : kg_lim(kg_lim_), rest0(rest0_), n_ks(n_ks_) {
    if (kg_lim > rest0) piece = qb_piece(kg_lim - rest0, n_ks_, span, &n_ranges);
  }
  uint64_t lo(uint64_t r) const { return std::min<uint64_t>(rest0 + r * piece * n_ks, kg_lim); }
  uint64_t hi(uint64_t r) const { return std::min<uint64_t>(lo(r) + piece * n_ks, kg_lim); }
};

// The slices of a pass whose slices are runs of k-groups of their own (per-block partial sums: a slice = a bootstrap
// block, thousands of them): whole k-groups, per_slice each (k_per_slice == 0), or k_per_slice contraction indices each,
// the k-groups shared with a neighbour masked per slice.  No slice reaches past kg_lim.
struct kg_slices {
  uint32_t n_ks;
  uint64_t per_slice, k_per_slice, kg_lim;
  uint64_t kg0(uint64_t ks) const { return k_per_slice ? (ks * k_per_slice) >> 2 : ks * per_slice; }
  uint64_t kg1(uint64_t ks) const {
    return std::min<uint64_t>(kg_lim, k_per_slice ? ((ks + 1) * k_per_slice + 3) >> 2 : (ks + 1) * per_slice);
  }
};

// ... walked in ranges of whole slices, in eights (the XCD deal of accum_mfma.hip): slices [ks0, ks0 + n) and the
// k-groups [lo, hi) they touch -- eight slices however long, more of them while the range stays within `span`.
struct kg_slice_group {
  uint32_t ks0, n;
  uint64_t lo, hi;
};
inline kg_slice_group kg_slice_group_at(const kg_slices &s, uint64_t span, uint32_t ks0) {
  uint32_t n = 8;
  while (ks0 + n < s.n_ks && s.kg1(ks0 + n + 7) - s.kg0(ks0) <= span && s.kg0(ks0 + n) < s.kg_lim) n += 8;
  n = std::min(n, s.n_ks - ks0);
  const uint64_t lo = std::min<uint64_t>(s.kg0(ks0), s.kg_lim);
  return kg_slice_group{ks0, n, lo, std::max(lo, s.kg1(ks0 + n - 1))};
}

// the leading slices, in eights, that end inside the resident head [0, res) of the second image: read where it lies
inline uint32_t kg_slices_resident(const kg_slices &s, uint64_t res) {
  uint32_t ks = 0;
  while (ks + 8 <= s.n_ks && s.kg1(ks + 7) <= res && s.kg0(ks + 7) < s.kg_lim) ks += 8;
  return ks;
}

// The kernel indexes an operand image by absolute k-group, so a launch over the slices of `r` is handed the scratch (cap
// doubles, k-groups [r.lo, r.hi + tail) of kstride doubles formed in it) moved back by the range's first k-group: an
// address below the scratch, formed as an integer.  Every k-group a launched slice can touch -- its own [kg0, kg1) and the
// `tail` k-groups its operand pipeline (the prefetching wavefront included) runs ahead -- must lie inside the scratch as
// just formed: NULL where one would not.
inline const double *kg_moved_back(const double *scratch, uint64_t cap, uint64_t kstride, uint64_t tail, const kg_slices &s,
                                   const kg_slice_group &r) {
  const uint64_t first = s.kg0(r.ks0), last = std::max(first, s.kg1(r.ks0 + r.n - 1));
  if ((first < r.lo && first < s.kg_lim) || last > r.hi || (r.hi - r.lo + tail) * kstride > cap) return nullptr;
  return reinterpret_cast<const double *>(reinterpret_cast<uintptr_t>(scratch) - r.lo * kstride * sizeof(double));
}
