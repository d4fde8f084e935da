// The planner of the windowed calls' slab plans (ngsdist_amd/csrc/win_plan.h) on its own, for tests/test_win_plan_cpu.py:
// a case per line of stdin -- em pdel n_ks tail chunk plane budget n_rep n_blocks q n_win lo[0] hi[0] lo[1] hi[1] ...
// (n_rep = 0: no job) -- and per case on stdout
//   N n_bnd                                  distinct boundaries of the whole call (the auto plan's estimate)
//   S bytes ...                              per window, what the single-window fit test compares with the budget
//   F fits                                   0: some window alone does not fit, nothing is planned
//   B a b hi_max n_seg n_ks max_wkg w_total bytes      a batch, and the bytes formula on what it holds
//   T kg0 kg1 woff slo shi                   its slice table, n_ks rows
//   W first end len                          its window table, b - a rows
//   K blk[0] .. blk[n_blocks]                a job: the block starts of each window
//   E
#include <cstdio>
#include <vector>

#include "win_plan.h"

int main() {
  unsigned long long em, pdel, n_ks, tail, chunk, plane, budget, n_rep, n_blocks, q, n_win;
  while (scanf("%llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu", &em, &pdel, &n_ks, &tail, &chunk, &plane, &budget, &n_rep,
               &n_blocks, &q, &n_win) == 11) {
    std::vector<uint64_t> lo(n_win), hi(n_win);
    for (uint64_t w = 0; w < n_win; w++) {
      unsigned long long l, h;
      if (scanf("%llu %llu", &l, &h) != 2) return 2;
      lo[w] = l; hi[w] = h;
    }
    const win_env v{plane, em != 0, pdel != 0, (uint32_t)n_ks, tail, (uint32_t)chunk};
    const std::vector<uint32_t> mult(n_rep * n_blocks, 1u);
    const WinBoot job{(uint32_t)n_rep, n_blocks, q, mult.data()}, *bt = n_rep ? &job : nullptr;
    std::vector<uint64_t> bnd, wb;
    for (uint64_t w = 0; w < n_win; w++) {
      win_boundaries(lo[w], hi[w], bt, wb);
      bnd.insert(bnd.end(), wb.begin(), wb.end());
    }
    std::sort(bnd.begin(), bnd.end());
    printf("N %llu\nS", (unsigned long long)(std::unique(bnd.begin(), bnd.end()) - bnd.begin()));
    for (uint64_t w = 0; w < n_win; w++)
      printf(" %llu", (unsigned long long)win_batch_bytes(v, bt ? bt->n_blocks + 1 : 1, hi[w] - lo[w], 1, bt));
    const bool fits = win_each_fits(v, lo.data(), hi.data(), n_win, bt, budget);
    printf("\nF %d\n", fits ? 1 : 0);
    win_batch p;
    for (uint64_t a = 0; fits && a < n_win; a = p.b) {
      win_plan_batch(v, lo.data(), hi.data(), n_win, a, budget, bt, p);
      if (p.a != a || p.b <= a || p.b > n_win) return 3;  // (the test reads no further)
      if (p.tab.size() != p.n_ks * NGD_SEG_STRIDE || p.wt.size() != 2 * (p.b - a) || p.blk.size() != (bt ? (p.b - a) * (n_blocks + 1) : 0))
        return 4;
      printf("B %llu %llu %llu %llu %llu %llu %llu %llu\n", (unsigned long long)p.a, (unsigned long long)p.b, (unsigned long long)p.hi_max,
             (unsigned long long)p.n_seg, (unsigned long long)p.n_ks, (unsigned long long)p.max_wkg, (unsigned long long)p.w_total,
             (unsigned long long)win_batch_bytes(v, p.n_seg, p.hi_max - lo[a], p.b - a, bt));
      for (uint64_t k = 0; k < p.n_ks; k++) {
        const uint64_t *t = &p.tab[k * NGD_SEG_STRIDE];
        printf("T %llu %llu %llu %llu %llu\n", (unsigned long long)t[NGD_SEG_KG0], (unsigned long long)t[NGD_SEG_KG1],
               (unsigned long long)t[NGD_SEG_WOFF], (unsigned long long)t[NGD_SEG_SLO], (unsigned long long)t[NGD_SEG_SHI]);
      }
      for (uint64_t w = 0; w < p.b - a; w++)
        printf("W %llu %llu %llu\n", p.wt[2 * w] & 0xffffffffull, p.wt[2 * w] >> 32, p.wt[2 * w + 1]);
      for (uint64_t w = 0; bt && w < p.b - a; w++) {
        printf("K");
        for (uint64_t k = 0; k <= n_blocks; k++) printf(" %u", p.blk[w * (n_blocks + 1) + k]);
        printf("\n");
      }
    }
    printf("E\n");
  }
  return 0;
}
