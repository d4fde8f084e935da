// The index arithmetic of ngsdist_amd/csrc/ngd_layout.h on its own (tests/test_unit_layout_cpu.py): prints one line per
// check that fails, "ok" and the number of checks otherwise.
#include <cstdio>
#include <set>
#include <vector>

#include "ngd_layout.h"

int main() {
  unsigned long long n_checks = 0, n_bad = 0;
  auto bad = [&](const char *what, unsigned long long a, unsigned long long b, int quad) {
    if (n_bad++ < 20) printf("FAIL %s a=%llu b=%llu quad=%d\n", what, a, b, quad);
  };
  for (int quad = 0; quad < 2; quad++) {
    // (site, coordinate) <-> index: a bijection of [0, 4 Q) x [0, 3) onto [0, 12 Q), inverse included
    for (uint64_t Q : {1ull, 2ull, 3ull, 7ull, 64ull, 1000ull}) {
      std::vector<int> hit(12 * Q, 0);
      for (uint64_t s = 0; s < 4 * Q; s++)
        for (uint32_t c = 0; c < 3; c++) {
          const uint64_t k = ngd_k_of(s, c, quad);
          n_checks++;
          if (k >= 12 * Q) { bad("index outside the periods of its sites", s, k, quad); continue; }
          hit[k]++;
          uint64_t s2; uint32_t c2;
          ngd_site_of(k, quad, &s2, &c2);
          if (s2 != s || c2 != c) bad("inverse", s, k, quad);
          // the period: twelve indices are four whole sites in both layouts
          if (k / 12 != s / 4) bad("period", s, k, quad);
          // quad: the unit-sum coordinate alone fills the k-groups 3 q, position s & 3
          if (quad && ((k / 4) % 3 == 0) != (c == 0)) bad("t0 k-group", s, k, quad);
          if (quad && c == 0 && (k & 3) != (s & 3)) bad("t0 position", s, k, quad);
          if (quad && c == 1 && k != 12 * (s / 4) + 4 + 2 * (s & 3)) bad("t1 index", s, k, quad);
          if (quad && c == 2 && k != ngd_k_of(s, 1, 1) + 1) bad("t2 follows t1", s, k, quad);
          if (!quad && k != 3 * s + c) bad("plain layout", s, k, quad);
        }
      for (uint64_t k = 0; k < 12 * Q; k++) { n_checks++; if (hit[k] != 1) bad("not a bijection at index", k, hit[k], quad); }
    }
    // a site range's k-groups hold every index of the range; the whole k-groups below a prefix hold no other site's
    for (uint64_t s1 = 1; s1 <= 40; s1++)
      for (uint64_t s0 = 0; s0 < s1; s0++) {
        const uint64_t lo = ngd_kg_lo(s0, quad), hi = ngd_kg_hi(s1, quad);
        for (uint64_t s = s0; s < s1; s++)
          for (uint32_t c = 0; c < 3; c++) {
            const uint64_t kg = ngd_k_of(s, c, quad) >> 2;
            n_checks++;
            if (kg < lo || kg >= hi) bad("range does not contain its site", s0 * 100 + s1, s, quad);
          }
        // the quad form's range bounds the plain layout's as well (what a load waits for)
        n_checks++;
        if (ngd_kg_lo(s0, 1) > ngd_kg_lo(s0, 0) || ngd_kg_hi(s1, 1) < ngd_kg_hi(s1, 0)) bad("quad range is no superset", s0, s1, quad);
        // tight to a period: no more than the range's own periods
        if (quad && (lo != 3 * (s0 / 4) || hi != 3 * ((s1 + 3) / 4))) bad("quad range", s0, s1, quad);
      }
    for (uint64_t s1 = 0; s1 <= 40; s1++) {
      const uint64_t w = ngd_kg_whole(s1, quad);
      for (uint64_t k = 0; k < 4 * w; k++) {
        uint64_t s; uint32_t c;
        ngd_site_of(k, quad, &s, &c);
        n_checks++;
        if (s >= s1) bad("whole k-groups hold a later site", s1, k, quad);
      }
    }
  }
  if (n_bad) { printf("%llu checks failed\n", n_bad); return 1; }
  printf("ok %llu\n", n_checks);
  return 0;
}
