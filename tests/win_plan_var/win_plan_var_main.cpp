// The per-window forms of the slab planner (ngsdist_amd/csrc/win_plan.h: win_each_fits_var, win_plan_batch_var) on their own,
// for tests/test_win_plan_var_cpu.py: a case per line of stdin --
//   em pdel n_ks tail chunk plane quad budget n_rep q n_win   lo[0] hi[0] cls[0]   lo[1] hi[1] cls[1] ...
// (cls: the window's class, -1 for a window shorter than one block) -- and per case on stdout
//   S bytes ...                              per window, what the single-window fit test compares with the budget
//   F fits                                   0: some window alone does not fit, nothing is planned
//   B a b hi_max n_seg n_ks max_wkg w_total bytes wt_rows      a batch, and the bytes formula on what it holds
//   T kg0 kg1 woff slo shi                   its slice table, n_ks rows
//   W first end len                          its window table, b - a rows
//   D blk_off n_blocks wt_off n_vis          its descriptors, b - a rows
//   K blk ...                                every window's row of block starts (n_blocks + 1 entries)
//   C cls:row ...                            the classes it holds, in order, with the first row of each one's weights
//   Q equal                                  windows of one length: 1 if the tables equal win_plan_batch's (no budget)
//   E
#include <cstdio>
#include <vector>

#include "win_plan.h"

typedef unsigned long long ull;

int main() {
  ull em, pdel, n_ks, tail, chunk, plane, quad, budget, n_rep, q, n_win;
  while (scanf("%llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu", &em, &pdel, &n_ks, &tail, &chunk, &plane, &quad, &budget, &n_rep,
               &q, &n_win) == 11) {
    std::vector<uint64_t> lo(n_win), hi(n_win), cls_blocks, cls_mult;
    std::vector<uint32_t> cls(n_win);
    bool one_length = true;
    for (uint64_t w = 0; w < n_win; w++) {
      ull l, h;
      long long c;
      if (scanf("%llu %llu %lld", &l, &h, &c) != 3) return 2;
      lo[w] = l; hi[w] = h;
      cls[w] = c < 0 ? NGD_WIN_NO_CLASS : (uint32_t)c;
      if (c >= 0 && (uint64_t)c >= cls_blocks.size()) cls_blocks.resize(c + 1, 0);
      if (c >= 0) cls_blocks[c] = (h - l) / q;
      one_length = one_length && h - l == hi[0] - lo[0];
    }
    uint64_t n_mult = 0;
    for (uint64_t b : cls_blocks) { cls_mult.push_back(n_mult); n_mult += n_rep * b; }
    const std::vector<uint32_t> mult(n_mult, 1u);
    win_env v{plane, em != 0, pdel != 0, (uint32_t)n_ks, tail, (uint32_t)chunk};
    v.quad = quad != 0;
    const WinBootVar bv{(uint32_t)n_rep, q, (uint32_t)cls_blocks.size(), cls.data(), cls_blocks.data(), cls_mult.data(), mult.data()};
    printf("S");
    for (uint64_t w = 0; w < n_win; w++) {
      const uint64_t nb = (hi[w] - lo[w]) / q;
      printf(" %llu", (ull)win_batch_bytes_var(v, nb + 1, hi[w] - lo[w], 1, nb + 1, nb, bv.n_rep));
    }
    const bool fits = win_each_fits_var(v, lo.data(), hi.data(), n_win, bv, budget);
    printf("\nF %d\n", fits ? 1 : 0);
    win_batch_var p;
    std::vector<uint64_t> all;
    win_call_boundaries_var(lo.data(), hi.data(), n_win, q, all);
    for (uint64_t a = 0; fits && a < n_win; a = p.b) {
      win_plan_batch_var(v, lo.data(), hi.data(), n_win, a, budget, bv, all, p);
      if (p.a != a || p.b <= a || p.b > n_win) return 3;  // (the test reads no further)
      if (p.tab.size() != p.n_ks * NGD_SEG_STRIDE || p.wt.size() != 2 * (p.b - a) || p.desc.size() != NGD_WIN_DESC * (p.b - a)) return 4;
      printf("B %llu %llu %llu %llu %llu %llu %llu %llu %llu\n", (ull)p.a, (ull)p.b, (ull)p.hi_max, (ull)p.n_seg, (ull)p.n_ks,
             (ull)p.max_wkg, (ull)p.w_total,
             (ull)win_batch_bytes_var(v, p.n_seg, p.hi_max - lo[a], p.b - a, p.blk.size(), p.wt_rows, bv.n_rep), (ull)p.wt_rows);
      for (uint64_t k = 0; k < p.n_ks; k++) {
        const uint64_t *t = &p.tab[k * NGD_SEG_STRIDE];
        printf("T %llu %llu %llu %llu %llu\n", (ull)t[NGD_SEG_KG0], (ull)t[NGD_SEG_KG1], (ull)t[NGD_SEG_WOFF], (ull)t[NGD_SEG_SLO],
               (ull)t[NGD_SEG_SHI]);
      }
      for (uint64_t w = 0; w < p.b - a; w++) printf("W %llu %llu %llu\n", p.wt[2 * w] & 0xffffffffull, p.wt[2 * w] >> 32, p.wt[2 * w + 1]);
      for (uint64_t w = 0; w < p.b - a; w++) {
        const uint64_t *d = &p.desc[w * NGD_WIN_DESC];
        printf("D %llu %llu %llu %llu\nK", (ull)d[NGD_WIN_DESC_BLK], (ull)d[NGD_WIN_DESC_NB], (ull)d[NGD_WIN_DESC_WT], (ull)d[NGD_WIN_DESC_VIS]);
        if (d[NGD_WIN_DESC_BLK] + d[NGD_WIN_DESC_NB] + 1 > p.blk.size()) return 5;
        for (uint64_t k = 0; k <= d[NGD_WIN_DESC_NB]; k++) printf(" %u", p.blk[d[NGD_WIN_DESC_BLK] + k]);
        printf("\n");
      }
      printf("C");
      for (uint32_t c : p.cls_list) printf(" %u:%llu", c, (ull)p.cls_row[c]);
      printf("\n");
    }
    if (one_length && fits && n_rep) {
      const uint64_t n_blocks = (hi[0] - lo[0]) / q;
      const std::vector<uint32_t> m1(n_rep * n_blocks, 1u);
      const WinBoot bt{(uint32_t)n_rep, n_blocks, q, m1.data()};
      win_batch p0;
      win_plan_batch(v, lo.data(), hi.data(), n_win, 0, ~0ull, &bt, p0);
      win_plan_batch_var(v, lo.data(), hi.data(), n_win, 0, ~0ull, bv, all, p);
      printf("Q %d\n", p0.b == n_win && p.b == n_win && p0.tab == p.tab && p0.wt == p.wt && p0.blk == p.blk && p0.n_seg == p.n_seg &&
                           p0.n_ks == p.n_ks && p0.max_wkg == p.max_wkg && p0.w_total == p.w_total ? 1 : 0);
    }
    printf("E\n");
  }
  return 0;
}
