// The k-group range walk of the single-image passes (ngsdist_amd/csrc/kg_ranges.h) on its own, for tests/test_kg_ranges_cpu.py:
// a case per line of stdin -- n_ks per_slice k_per_slice kg_lim span res rest0 -- and per case on stdout
//   F first            slices [0, first) end inside the resident head [0, res) of the second image
//   G ks0 n lo hi      the ranges of whole slices from `first` on
//   M a b              the moved-back scratch of the range: a = 1 if it points lo k-groups below the scratch, b = 1 if a
//                      scratch one double too short is refused
//   P lo hi piece      the ranges of a whole pass over [rest0, kg_lim)
//   E
#include <cstdio>
#include <vector>

#include "kg_ranges.h"

int main() {
  unsigned long long n_ks, per_slice, k_per_slice, kg_lim, span, res, rest0;
  const uint64_t kstride = 2, tail = 8;
  while (scanf("%llu %llu %llu %llu %llu %llu %llu", &n_ks, &per_slice, &k_per_slice, &kg_lim, &span, &res, &rest0) == 7) {
    const kg_slices sl{(uint32_t)n_ks, per_slice, k_per_slice, kg_lim};
    const uint32_t first = res ? kg_slices_resident(sl, res) : 0;
    printf("F %u\n", first);
    for (uint32_t ks0 = first; ks0 < sl.n_ks;) {
      const kg_slice_group r = kg_slice_group_at(sl, span, ks0);
      printf("G %u %u %llu %llu\n", r.ks0, r.n, (unsigned long long)r.lo, (unsigned long long)r.hi);
      std::vector<double> scratch((r.hi - r.lo + tail) * kstride);
      const double *back = kg_moved_back(scratch.data(), scratch.size(), kstride, tail, sl, r);
      const bool there = back && reinterpret_cast<uintptr_t>(back) + r.lo * kstride * sizeof(double) == reinterpret_cast<uintptr_t>(scratch.data());
      printf("M %d %d\n", there ? 1 : 0, kg_moved_back(scratch.data(), scratch.size() - 1, kstride, tail, sl, r) ? 0 : 1);
      if (!r.n) return 2;
      ks0 += r.n;
    }
    const kg_pass_ranges pr(kg_lim, (uint32_t)n_ks, span, rest0);
    for (uint64_t r = 0; r < pr.n_ranges; r++)
      printf("P %llu %llu %llu\n", (unsigned long long)pr.lo(r), (unsigned long long)pr.hi(r), (unsigned long long)pr.piece);
    printf("E\n");
  }
  return 0;
}
