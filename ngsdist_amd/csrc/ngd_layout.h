// ngd_layout.h -- which contraction index k of a fragment-major operand image holds coordinate c of site s, and which
// k-groups (four consecutive indices, one 512-byte fragment per group of 16 individuals) a range of sites occupies.
// Plain arithmetic for the host and the device: nothing of HIP is included, so that a plain C++ program can use it too
// (tests/unit_layout/unit_layout_main.cpp).
//
// Two layouts, both with twelve indices = three k-groups = four WHOLE sites 4q .. 4q+3 per period q:
//   quad = 0 (every image but the congruent one):  k = 3 s + c.
//   quad = 1 (the one image of a congruent engine, ngd_config.single_image = 2):  the four t0 = c_0 . p of the period fill
//            k-group 3q, position u = s & 3; (t1, t2) of site 4q+u follow at 12q + 4 + 2u and the index after it.  The
//            unit-sum coordinate of the reference's matrices thus lives in k-groups of its own (kg % 3 == 0), which a
//            pass that takes its contribution as a constant leaves out (engine_plans.hip, NGD_OPT_UNIT_SKIP).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NGD_HD __host__ __device__
#else
#define NGD_HD
#endif

NGD_HD inline uint64_t ngd_k_of(uint64_t s, uint32_t c, int quad) {
  if (!quad) return 3 * s + c;
  const uint64_t base = 12 * (s >> 2), u = s & 3;
  return c == 0 ? base + u : base + 4 + 2 * u + (c - 1);
}

// the inverse: site and coordinate of index k
NGD_HD inline void ngd_site_of(uint64_t k, int quad, uint64_t *s, uint32_t *c) {
  if (!quad) {
    *s = k / 3;
    *c = (uint32_t)(k % 3);
    return;
  }
  const uint64_t q = k / 12, r = k % 12;
  if (r < 4) {
    *s = 4 * q + r;
    *c = 0;
  } else {
    *s = 4 * q + ((r - 4) >> 1);
    *c = 1 + (uint32_t)((r - 4) & 1);
  }
}

// Sites [s0, s1) occupy k-groups [ngd_kg_lo(s0), ngd_kg_hi(s1)): every index of every site of the range lies inside.
// quad = 1 rounds outwards to whole periods -- a superset of quad = 0's range, so the quad form bounds both layouts.
NGD_HD inline uint64_t ngd_kg_lo(uint64_t s0, int quad) { return quad ? 3 * (s0 >> 2) : (3 * s0) >> 2; }
NGD_HD inline uint64_t ngd_kg_hi(uint64_t s1, int quad) { return quad ? 3 * ((s1 + 3) >> 2) : (3 * s1 + 3) >> 2; }
// ... and the k-groups [0, ngd_kg_whole(s1)) hold indices of the sites [0, s1) ONLY (what a pass may read once those
// sites are complete)
NGD_HD inline uint64_t ngd_kg_whole(uint64_t s1, int quad) { return quad ? 3 * (s1 >> 2) : (3 * s1) >> 2; }
