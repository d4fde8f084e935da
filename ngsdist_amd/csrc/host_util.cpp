// host_util.cpp -- the host-side pieces of the C ABI that must use the HOST's
// libm / integer arithmetic to reproduce the reference's printed cells exactly:
// the tail of gen_dist() (reference ngsDist.cpp:372-401) and the bootstrap block
// draw (ngsDist.cpp:416-423 over gsl_rng_taus, seeded at :179-180).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <condition_variable>
#include <functional>
#include <limits>
#include <mutex>
#include <thread>
#include <unordered_set>
#include <vector>

#include "../../include/ngsdist_amd.h"
#include "ngd_shard.h"
#include "win_cmp_geom.h"

namespace {
// gsl_rng_taus: GSL is a third-party dependency of the reference (README.md:20,
// "gsl v1.15") that is not under /root/reference.  Algorithm restated from its
// published description (L'Ecuyer 1996 combined Tausworthe, three components,
// seeding by the 69069 LCG, six warm-up draws); pinned by GSL's own known
// answer in tests/test_abi.py (seed 1, 10000th output = 2733957125).
inline uint32_t taus_step(uint32_t s, int a, int b, uint32_t c, int d) {
  return ((s & c) << d) ^ (((s << a) ^ s) >> b);
}
inline uint32_t taus_get(uint32_t st[3]) {
  st[0] = taus_step(st[0], 13, 19, 4294967294u, 12);
  st[1] = taus_step(st[1], 2, 25, 4294967288u, 4);
  st[2] = taus_step(st[2], 3, 11, 4294967280u, 17);
  return st[0] ^ st[1] ^ st[2];
}
}  // namespace

// d = sum / cnt (ngsDist.cpp:376) for a range of cells, apart from the model's transform: a loop the compiler can
// vectorise (IEEE division is correctly rounded at any width: the same bits as the scalar loop; -ffp-contract=off and no
// fast-math here).  (double)c for counts below 2^52 -- any site count -- is the exponent trick: exact, and free of the
// unsigned 64-bit conversion no AVX2 instruction does.
__attribute__((target_clones("avx2", "default"))) static void divide_range(const double *sum, const uint64_t *cnt, uint64_t lo,
                                                                           uint64_t hi, uint64_t tot_sites, double *dist) {
  const uint64_t magic = 0x4330000000000000ull;  // 2^52 as a bit pattern
  if (tot_sites > 0) {
    const double c = (double)tot_sites;
    for (uint64_t k = lo; k < hi; k++) dist[k] = sum[k] / c;
    return;
  }
  uint64_t big = 0;
  for (uint64_t k = lo; k < hi; k++) big |= cnt[k];
  if (big >> 52) {  // (never a site count; kept exact all the same)
    for (uint64_t k = lo; k < hi; k++) dist[k] = sum[k] / (double)cnt[k];
    return;
  }
  for (uint64_t k = lo; k < hi; k++) {
    const uint64_t bits = cnt[k] | magic;
    double c;
    memcpy(&c, &bits, 8);
    dist[k] = sum[k] / (c - 4503599627370496.0);
  }
}

static void finish_range(const double *sum, const uint64_t *cnt, uint64_t lo, uint64_t hi, uint64_t tot_sites,
                         uint64_t evol_model, double *dist) {
  // in pieces that stay in the cache between the two passes
  for (uint64_t a = lo; a < hi; a += 4096) {
    const uint64_t b = std::min(hi, a + 4096);
    divide_range(sum, cnt, a, b, tot_sites, dist);
    if (evol_model == 1) {
      for (uint64_t k = a; k < b; k++) dist[k] = -log(1 - dist[k]);
    } else if (evol_model == 2) {
      for (uint64_t k = a; k < b; k++) dist[k] = -log(1 - (dist[k] * 4 / 3)) * 3 / 4;
    }
  }
}

// "%.10f" of one cell, byte-for-byte what printf writes (the reference formats every cell with
// snprintf("%.10f"), gen_func.cpp:483-486), without going through printf's arbitrary-precision path:
// x = m * 2^q exactly, so round-half-even(x * 10^10) is an integer computed exactly in 128 bits
// (m < 2^53, 10^10 < 2^34); printf rounds the exact binary value the same way (round-to-nearest mode).
// Values of 2^29 and above, which no distance reaches, and non-finite cells go to snprintf itself.
static inline char *fmt_fixed10(double x, char *o) {
  uint64_t bits;
  memcpy(&bits, &x, 8);
  const int e = (int)((bits >> 52) & 0x7FF);
  uint64_t m = bits & ((1ull << 52) - 1);
  if (e >= 1023 + 29) return o + snprintf(o, 400, "%.10f", x);  // large, inf, nan
  if (bits >> 63) *o++ = '-';
  int q;  // x = m * 2^q
  if (e == 0) q = -1074;
  else { m |= 1ull << 52; q = e - 1075; }
  const unsigned __int128 P = (unsigned __int128)m * 10000000000ull;
  uint64_t N;
  const int sh = -q;  // e < 1052 -> q < 0
  if (sh >= 100) N = 0;  // P < 2^87: below one half of the last digit
  else {
    N = (uint64_t)(P >> sh);
    const unsigned __int128 rem = P & (((unsigned __int128)1 << sh) - 1), half = (unsigned __int128)1 << (sh - 1);
    if (rem > half || (rem == half && (N & 1))) N++;
  }
  const uint64_t ip = N / 10000000000ull;
  uint64_t fp = N - ip * 10000000000ull;
  if (ip < 10) {  // (every distance but a saturated one)
    *o++ = (char)('0' + ip);
  } else {
    char tmp[24];
    int n = 0;
    uint64_t v = ip;
    do { tmp[n++] = (char)('0' + v % 10); v /= 10; } while (v);
    while (n) *o++ = tmp[--n];
  }
  *o++ = '.';
  // ten digits, two at a time (32-bit arithmetic: fp < 10^10 = two halves below 10^5)
  static const char kPairs[] =
      "00010203040506070809101112131415161718192021222324252627282930313233343536373839404142434445464748495051525354555657585960"
      "616263646566676869707172737475767778798081828384858687888990919293949596979899";
  const uint32_t hi = (uint32_t)(fp / 100000), lo = (uint32_t)(fp - (uint64_t)hi * 100000);
  const uint32_t h0 = hi / 1000, h1 = hi % 1000;  // hi = h0 (2 digits) h1 (3 digits)
  memcpy(o, kPairs + 2 * h0, 2);
  o[2] = (char)('0' + h1 / 100);
  memcpy(o + 3, kPairs + 2 * (h1 % 100), 2);
  const uint32_t l0 = lo / 1000, l1 = lo % 1000;
  memcpy(o + 5, kPairs + 2 * l0, 2);
  o[7] = (char)('0' + l1 / 100);
  memcpy(o + 8, kPairs + 2 * (l1 % 100), 2);
  return o + 10;
}

// A small persistent pool for the per-cell host work (the tail of gen_dist over up to millions of cells per call).
// Spawning and joining 16 threads costs ~0.3 ms per call ([measured] on the GPU box: 62 437 cells 0.32 ms, 8.1e6 cells in
// one call 2.8 ms but in 8 calls 5.4 ms), which is most of the tail of a multi-GPU step and half of a chunked cfg 5
// tail.  Workers sleep on a condition variable between calls; one job at a time (a second caller runs its job inline
// on its own thread).  Never destroyed: worker threads must not outlive their mutex at process exit.
namespace {
struct HostPool {
  std::mutex m, busy;
  std::condition_variable cv_go, cv_done;
  std::vector<std::thread> workers;
  std::function<void(unsigned)> job;
  unsigned n_parts = 0, next = 0, done = 0;
  uint64_t generation = 0;
  explicit HostPool(unsigned n) {
    for (unsigned t = 0; t < n; t++)
      workers.emplace_back([this]() {
        uint64_t seen = 0;
        std::unique_lock<std::mutex> lk(m);
        for (;;) {
          cv_go.wait(lk, [&] { return generation != seen; });
          seen = generation;
          while (next < n_parts) {
            const unsigned part = next++;
            lk.unlock();
            job(part);
            lk.lock();
            if (++done == n_parts) cv_done.notify_one();
          }
        }
      });
    for (auto &w : workers) w.detach();
  }
  // runs fn(0) .. fn(n - 1), the caller taking parts too; returns when all are done
  void run(unsigned n, const std::function<void(unsigned)> &fn) {
    std::unique_lock<std::mutex> one(busy, std::try_to_lock);
    if (!one.owns_lock() || n <= 1) {  // pool in use by another thread (or nothing to split): do it here
      for (unsigned k = 0; k < n; k++) fn(k);
      return;
    }
    std::unique_lock<std::mutex> lk(m);
    job = fn;
    n_parts = n; next = 0; done = 0;
    generation++;
    cv_go.notify_all();
    while (next < n_parts) {
      const unsigned part = next++;
      lk.unlock();
      fn(part);
      lk.lock();
      ++done;
    }
    cv_done.wait(lk, [&] { return done == n_parts; });
    n_parts = 0;
  }
};
HostPool &host_pool() {
  static HostPool *p = new HostPool(std::min(15u, std::max(1u, std::thread::hardware_concurrency()) - 1));
  return *p;
}
// ... and a wide one for the tail of a whole bootstrap job (millions of cells in one call): a burst of a millisecond on as
// many cores as the box has, up to 64 ([measured, round 6, 256 hardware threads, a CPU quota of 16] 8.1e6 cells of model 1:
// 2.4 ms on 16 threads; a quota counts CPU time per period, and 40 ms of it in a burst is far inside one).  Made on first use.
HostPool &host_pool_wide() {
  static HostPool *p = new HostPool(std::min(63u, std::max(1u, std::thread::hardware_concurrency()) - 1));
  return *p;
}
}  // namespace


extern "C" {

// The print block of one matrix, ngsDist.cpp:282-287: "\n<n_ind>\n", then per individual its label and
// n_ind cells "\t%.10f" (join(), gen_func.cpp:479-496) and a newline.  Rows are formatted by threads.
int64_t ngd_format_matrix(const double *dist, uint64_t n_ind, const char *const *labels, char *out, uint64_t cap,
                          uint32_t n_threads) {
  if (!dist || !labels || n_ind < 2) return NGD_E_INVALID;
  unsigned nt = n_threads ? n_threads : std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
  if (n_ind < 64) nt = 1;
  nt = (unsigned)std::min<uint64_t>(nt, n_ind);
  // shares of rows, finer than the threads (rows near the top hold more upper-triangle cells: dist is read row-wise there,
  // column-wise below the diagonal); every share formats into a buffer of its own, sized by the longest a cell can be
  const unsigned n_parts = nt == 1 ? 1 : (unsigned)std::min<uint64_t>(n_ind, 4ull * nt);
  // The shares' buffers are the calling thread's and are kept from call to call (a job prints a hundred matrices of 13 MB: a
  // fresh vector per share and call is an mmap, its zero fill and its page faults every time)
  struct Scratch {
    std::vector<char *> buf;
    std::vector<size_t> cap;
    ~Scratch() { for (char *b : buf) free(b); }
    bool reserve(unsigned t, size_t need) {  // (keeps the contents: a share may grow while it is being written)
      if (t < cap.size() && cap[t] >= need) return true;
      if (t >= buf.size()) return false;
      char *nb = (char *)realloc(buf[t], need);
      if (!nb) return false;
      buf[t] = nb;
      cap[t] = need;
      return true;
    }
  };
  static thread_local Scratch scratch_tl;
  Scratch &scratch = scratch_tl;  // (the pool's threads must see the CALLER's buffers, not thread-local ones of their own)
  if (scratch.buf.size() < n_parts) { scratch.buf.resize(n_parts, nullptr); scratch.cap.resize(n_parts, 0); }
  std::vector<size_t> part_len(n_parts, 0);
  std::atomic<bool> oom{false};
  std::vector<size_t> label_len(n_ind);
  for (uint64_t i = 0; i < n_ind; i++) label_len[i] = strlen(labels[i]);
  // (more threads asked for than the pool of 16 holds: the wide pool's 64 -- [measured, round 6] threads of the call's own,
  // made and joined per matrix, took three times as long as 16 pooled ones)
  const bool wide = n_threads > 16;
  auto run_parts = [&](const std::function<void(unsigned)> &fn) {
    if (nt == 1) {
      for (unsigned t = 0; t < n_parts; t++) fn(t);
    } else {
      (wide ? host_pool_wide() : host_pool()).run(n_parts, fn);
    }
  };
  char head[32];
  const int hn = snprintf(head, sizeof(head), "\n%lu\n", (unsigned long)n_ind);

  // The regular matrix -- every cell prints as "d.dddddddddd", 12 bytes: what distances are -- is formatted ONCE per pair
  // (the printed matrix is symmetric: the general form below formats every cell twice and walks a column of the upper
  // triangle for the cells under the diagonal) into 12-byte slots in pair order; the rows, all of one known length, are
  // then put together from the slots straight into `out`.  Any other cell (a sign, nan, inf, 10 and above) anywhere: the
  // general form.
  if (out && nt > 1) {
    uint64_t total_fixed = (uint64_t)hn;
    std::vector<uint64_t> row_at(n_ind);
    for (uint64_t i = 0; i < n_ind; i++) { row_at[i] = total_fixed; total_fixed += label_len[i] + n_ind * 13 + 1; }
    const uint64_t n_pairs = n_ind * (n_ind - 1) / 2;
    struct Slots { char *p = nullptr; size_t cap = 0; ~Slots() { free(p); } };
    static thread_local Slots slots_tl;
    Slots &slots = slots_tl;
    if (cap >= total_fixed && (slots.cap >= n_pairs * 12 || [&] {
          char *np_ = (char *)realloc(slots.p, n_pairs * 12);
          if (np_) { slots.p = np_; slots.cap = n_pairs * 12; }
          return np_ != nullptr;
        }())) {
      std::atomic<bool> irregular{false};
      char *const sl = slots.p;
      run_parts([&](unsigned t) {
        const uint64_t lo = n_pairs * t / n_parts, hi = n_pairs * (t + 1) / n_parts;
        char tmp[448];
        for (uint64_t k = lo; k < hi; k++) {
          const char *e = fmt_fixed10(dist[k], tmp);
          if (e - tmp != 12) { irregular.store(true, std::memory_order_relaxed); return; }
          memcpy(sl + 12 * k, tmp, 12);
        }
      });
      if (!irregular.load()) {
        memcpy(out, head, (size_t)hn);
        run_parts([&](unsigned t) {
          const uint64_t lo = n_ind * t / n_parts, hi = n_ind * (t + 1) / n_parts;
          for (uint64_t i = lo; i < hi; i++) {
            char *o = out + row_at[i];
            memcpy(o, labels[i], label_len[i]);
            o += label_len[i];
            uint64_t k = i - 1;  // cell (j, i), j < i: pair index j (2n - j - 1) / 2 + (i - j - 1), its step from j to j + 1 is n - j - 2
            for (uint64_t j = 0; j < i; j++) {
              *o++ = '\t';
              memcpy(o, sl + 12 * k, 12);
              o += 12;
              k += n_ind - j - 2;
            }
            memcpy(o, "\t0.0000000000", 13);
            o += 13;
            const char *row = sl + 12 * (i * (2 * n_ind - i - 1) / 2);  // the slots of cells (i, j), j > i, side by side
            for (uint64_t j = i + 1; j < n_ind; j++, row += 12) {
              *o++ = '\t';
              memcpy(o, row, 12);
              o += 12;
            }
            *o = '\n';
          }
        });
        return (int64_t)total_fixed;
      }
    }
  }
  auto rows = [&](unsigned t) {
    const uint64_t lo = n_ind * t / n_parts, hi = n_ind * (t + 1) / n_parts;
    size_t need = 0;
    for (uint64_t i = lo; i < hi; i++) need += label_len[i] + n_ind * 24 + 1;  // ("\t" + sign + 9 digits + "." + 10 = 22 at most below 2^29)
    if (!scratch.reserve(t, need + 512)) { oom = true; return; }
    char *o = scratch.buf[t], *lim = o + scratch.cap[t] - 450;  // (a cell snprintf may write -- 2^29 and above, 1e300 -- needs up to ~330)
    auto grow = [&]() {  // huge cells (never for distances)
      const size_t used = (size_t)(o - scratch.buf[t]);
      if (!scratch.reserve(t, scratch.cap[t] * 2 + 1024)) { oom = true; return false; }
      o = scratch.buf[t] + used;
      lim = scratch.buf[t] + scratch.cap[t] - 450;
      return true;
    };
    for (uint64_t i = lo; i < hi; i++) {
      if (o + label_len[i] > lim && !grow()) return;
      memcpy(o, labels[i], label_len[i]);
      o += label_len[i];
      // dist_matrix is symmetric with a zero diagonal (gen_dist_slave :411, init_ptr :200): cells (j, i), j < i, walk down
      // a column of the upper triangle -- pair index j (2n - j - 1) / 2 + (i - j - 1), its step from j to j + 1 is n - j - 2
      uint64_t k = i - 1;  // (j = 0)
      for (uint64_t j = 0; j < i; j++) {
        if (o > lim && !grow()) return;
        *o++ = '\t';
        o = fmt_fixed10(dist[k], o);
        k += n_ind - j - 2;
      }
      if (o > lim && !grow()) return;
      *o++ = '\t';
      o = fmt_fixed10(0.0, o);
      const double *row = dist + i * (2 * n_ind - i - 1) / 2 - (i + 1);  // row[j] = cell (i, j), j > i
      for (uint64_t j = i + 1; j < n_ind; j++) {
        if (o > lim && !grow()) return;
        *o++ = '\t';
        o = fmt_fixed10(row[j], o);
      }
      *o++ = '\n';
    }
    part_len[t] = (size_t)(o - scratch.buf[t]);
  };
  run_parts(rows);
  if (oom) return NGD_E_NOMEM;
  uint64_t total = (uint64_t)hn;
  std::vector<uint64_t> at(n_parts);
  for (unsigned t = 0; t < n_parts; t++) { at[t] = total; total += part_len[t]; }
  if (out && cap >= total) {
    memcpy(out, head, (size_t)hn);
    run_parts([&](unsigned t) { memcpy(out + at[t], scratch.buf[t], part_len[t]); });  // (13 MB for 1000 individuals: in parallel too)
  }
  return (int64_t)total;
}

void ngd_taus_seed(uint32_t st[3], uint64_t seed) {
  uint32_t s = (uint32_t)seed;
  if (s == 0) s = 1;
  st[0] = 69069u * s;
  st[1] = 69069u * st[0];
  st[2] = 69069u * st[1];
  for (int i = 0; i < 6; i++) taus_get(st);
}

double ngd_taus_uniform(uint32_t st[3]) { return taus_get(st) / 4294967296.0; }

uint32_t ngd_taus_get(uint32_t st[3]) { return taus_get(st); }

void ngd_boot_block_map(uint32_t st[3], uint64_t n_blocks, uint64_t *block_map) {
  for (uint64_t b = 0; b < n_blocks; b++) {
    // draw_rnd(r, 0, n_blocks) = min + gsl_rng_uniform(r) * (max - min), gen_func.cpp:117-119
    double r = 0 + ngd_taus_uniform(st) * (double)(n_blocks - 0);
    block_map[b] = (uint64_t)floor(r);
  }
}

// Which shard computes pair (i1 < i2): the owner of its 128 x 128 pair tile (ngd_shard.h).
uint32_t ngd_shard_of_pair(uint64_t n_ind, uint64_t i1, uint64_t i2, uint32_t shard_world) {
  if (shard_world <= 1) return 0;
  static thread_local uint32_t c_nt = 0, c_world = 0;
  static thread_local std::vector<uint32_t> c_owner;
  const uint32_t n_t = (uint32_t)((n_ind + 127) / 128);
  if (c_nt != n_t || c_world != shard_world) {
    c_owner = ngd_tile_owners(n_t, shard_world);
    c_nt = n_t;
    c_world = shard_world;
  }
  return c_owner[ngd_tile_id(n_t, i1 / 128, i2 / 128)];
}

// The same for every pair at once, in the reference's pair order (ngsDist.cpp:244-245): what a host needs to pack the
// cells it owns for the ONE all-gather of a pair-sharded job.
void ngd_shard_map(uint64_t n_ind, uint32_t shard_world, int32_t *owner) {
  const uint32_t n_t = (uint32_t)((n_ind + 127) / 128);
  const std::vector<uint32_t> own = ngd_tile_owners(n_t, shard_world ? shard_world : 1);
  uint64_t k = 0;
  for (uint64_t i = 0; i < n_ind; i++)
    for (uint64_t j = i + 1; j < n_ind; j++) owner[k++] = (int32_t)own[ngd_tile_id(n_t, i / 128, j / 128)];
}

// ngd_config.single_image = 2 (engine.hip): the symmetric score matrix as a sum of three weighted squares, S = SUM_r d[r] c_r c_r^T
// (Lagrange's reduction; c row-major: c[3 r + g]).  With t_r = c_r . p per site, p1^T S p2 = SUM_r d[r] t_r(p1) t_r(p2):
// ONE image (t) serves both operands of the MFMA kernel and d rides on the per-index weights.  Every step divides by a
// diagonal entry or by twice an off-diagonal one only: for the reference's two matrices (parse_args.cpp:25-27, :134-137:
// entries 0, 0.5, 1) c and d are small dyadic numbers, t is exact for called genotypes and so are the sums.
// NGD_E_INVALID if S is not symmetric or the reconstruction does not give S back to 1e-13 of its largest entry.  Pure host arithmetic.
int ngd_score_congruence(const double *S, double *c, double *d) {
  double A[3][3];
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) {
      if (S[3 * a + b] != S[3 * b + a] || !std::isfinite(S[3 * a + b])) return NGD_E_INVALID;
      A[a][b] = S[3 * a + b];
    }
  int n = 0;
  for (int r = 0; r < 9; r++) c[r] = 0;
  for (int r = 0; r < 3; r++) d[r] = 0;
  double scale = 0;
  for (int k = 0; k < 9; k++) scale = std::max(scale, std::fabs(S[k]));
  const double tiny = 1e-14 * scale;  // what an elimination in floating point leaves of an exact zero
  auto deflate = [&](const double *row, double w) {  // A -= w row row^T, the square joins the list
    for (int g = 0; g < 3; g++) c[3 * n + g] = row[g];
    d[n++] = w;
    for (int a = 0; a < 3; a++)
      for (int b = 0; b < 3; b++) {
        A[a][b] -= w * row[a] * row[b];
        if (std::fabs(A[a][b]) <= tiny) A[a][b] = 0;
      }
  };
  auto clear = [&](int a) {  // the eliminated variable's row and column are zero by construction
    for (int g = 0; g < 3; g++) A[a][g] = A[g][a] = 0;
  };
  while (n < 3) {
    int pa = -1;
    for (int a = 0; a < 3; a++)
      if (A[a][a] != 0 && (pa < 0 || std::fabs(A[a][a]) > std::fabs(A[pa][pa]))) pa = a;
    if (pa >= 0) {  // a square on the diagonal: A[a][a] (x_a + SUM_b A[a][b] / A[a][a] x_b)^2
      const double piv = A[pa][pa];
      double row[3];
      for (int g = 0; g < 3; g++) row[g] = A[pa][g] / piv;
      deflate(row, piv);
      clear(pa);
      continue;
    }
    int qa = -1, qb = -1;
    for (int a = 0; a < 3; a++)
      for (int b = a + 1; b < 3; b++)
        if (A[a][b] != 0 && (qa < 0 || std::fabs(A[a][b]) > std::fabs(A[qa][qb]))) { qa = a; qb = b; }
    if (qa < 0) break;  // nothing left: rank below 3, the remaining weights stay 0
    if (n > 1) return NGD_E_INVALID;  // (two squares needed)
    // no square, a mixed term: with r_a, r_b the two rows, 2 / beta r_a r_b = 1 / (2 beta) ((r_a + r_b)^2 - (r_a - r_b)^2)
    const double beta = A[qa][qb];
    double plus[3], minus[3];
    for (int g = 0; g < 3; g++) { plus[g] = A[qa][g] + A[qb][g]; minus[g] = A[qa][g] - A[qb][g]; }
    deflate(plus, 1.0 / (2 * beta));
    deflate(minus, -1.0 / (2 * beta));
    clear(qa);
    clear(qb);
  }
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) {
      double r = 0;
      for (int k = 0; k < 3; k++) r += d[k] * c[3 * k + a] * c[3 * k + b];
      if (std::fabs(r - S[3 * a + b]) > 1e-13 * scale) return NGD_E_INVALID;
    }
  return NGD_OK;
}

int ngd_finish(const double *sum, const uint64_t *cnt, uint64_t n_pairs, uint64_t tot_sites,
               uint64_t evol_model, double *dist) {
  if (evol_model > 2) return NGD_E_MODEL;  // reference: error("... model not yet supported")
  if (!sum || !cnt || !dist) return NGD_E_INVALID;
  // per-cell and order-free, so threads change nothing but the wall time
  unsigned nt = 1;
  if (n_pairs >= (1u << 15)) nt = std::min(n_pairs >= (1u << 17) ? 16u : 8u, std::max(1u, std::thread::hardware_concurrency()));  // (waking the pool costs ~50 us)
  const bool wide = n_pairs >= (1u << 19) && std::thread::hardware_concurrency() > 16;
  if (wide) nt = std::min(64u, std::thread::hardware_concurrency());
  if (nt <= 1) {
    finish_range(sum, cnt, 0, n_pairs, tot_sites, evol_model, dist);
  } else {
    const unsigned parts = n_pairs >= (1u << 20) ? 4 * nt : nt;  // large jobs: finer than the threads, so that they finish together
    const uint64_t per = (n_pairs + parts - 1) / parts;
    (wide ? host_pool_wide() : host_pool()).run(parts, [&](unsigned k) {
      const uint64_t lo = k * per, hi = std::min(n_pairs, lo + per);
      if (lo < hi) finish_range(sum, cnt, lo, hi, tot_sites, evol_model, dist);
    });
  }
  return NGD_OK;
}

// ngd_finish() over cells that are still ARRIVING (a job's matrices coming off the device chunk by chunk): the pool is
// woken once for the whole job and a share of cells is worked as soon as *landed says it is final, so the tail of
// gen_dist() runs beside the copies instead of one pool wake-up per chunk ([measured, round 6] 8.1e6 cells: 1.3 ms in one
// call, 2.7 ms in 8).  Shares are handed out in ascending order; a thread whose share has not landed yet spins on the counter.
int ngd_finish_stream(const double *sum, const uint64_t *cnt, uint64_t n_pairs, uint64_t tot_sites, uint64_t evol_model,
                      double *dist, const volatile uint64_t *landed) {
  if (evol_model > 2) return NGD_E_MODEL;
  if (!sum || !cnt || !dist || !landed) return NGD_E_INVALID;
  const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
  const bool wide = n_pairs >= (1u << 19) && hw > 16;
  const unsigned nt = wide ? std::min(64u, hw) : std::min(16u, hw);
  const unsigned parts = (unsigned)std::min<uint64_t>(std::max<uint64_t>(1, n_pairs / 16384), 8 * nt);
  const uint64_t per = (n_pairs + parts - 1) / parts;
  auto share = [&](unsigned k) {
    const uint64_t lo = k * per, hi = std::min(n_pairs, lo + per);
    if (lo >= hi) return;
    for (unsigned spins = 0; *landed < hi; spins++) {
      if (spins < 4096) __builtin_ia32_pause();
      else std::this_thread::yield();
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    finish_range(sum, cnt, lo, hi, tot_sites, evol_model, dist);
  };
  if (nt <= 1 || parts <= 1) {
    for (unsigned k = 0; k < parts; k++) share(k);
  } else {
    (wide ? host_pool_wide() : host_pool()).run(parts, share);
  }
  return NGD_OK;
}

// --win_size / --win_step: per chromosome (a maximal run of equal ids) the windows of `size` sites every `step` sites that
// fit inside it.  The host and the Python package both call this, so that they agree on the list.
// One site of the reference's EM for two individuals: em2() (emOptim2.cpp:112-135) around emStep2 (:91-109), normalize
// (:69-75) and lik2 (:77-89), restated for GL1.x == 1 and dim == 9 -- the operation order is the reference's: every
// product is (sfs * g1) * g2, sums run left to right from 0, the step's posterior is normalised twice (the site's own
// terms, then their "sum over sites", 0 + inner).  Built like the tail of gen_dist() above: g++ -O3, glibc log, no FMA
// contraction -- the engine's NGD_OPT_EM_EXACT recheck decides the stopping step with it (engine_em_exact.hip).
static inline void em2_normalize(double *tmp) {
  double s = 0;
  for (int i = 0; i < 9; i++) s += tmp[i];
  for (int i = 0; i < 9; i++) tmp[i] /= s;
}
static inline double em2_lik(const double *sfs, const double *g1, const double *g2) {
  double res = 0, tmp = 0;
  int inc = 0;
  for (int x = 0; x < 3; x++)
    for (int y = 0; y < 3; y++) tmp += sfs[inc++] * g1[x] * g2[y];
  res += log(tmp);
  return res;
}
void ngd_em2_site(const double gl1[3], const double gl2[3], double sfs[9], int *n_iter) {
  const double tole = 0.001;  // ngsDist.cpp:349
  const int max_iter = 50;
  double old_lik = em2_lik(sfs, gl1, gl2), inner[9], post[9];
  int it = 0;
  while (it < max_iter) {
    int inc = 0;
    for (int x = 0; x < 9; x++) post[x] = 0.0;
    for (int x = 0; x < 3; x++)
      for (int y = 0; y < 3; y++) {
        inner[inc] = sfs[inc] * gl1[x] * gl2[y];
        inc++;
      }
    em2_normalize(inner);
    for (int x = 0; x < 9; x++) post[x] += inner[x];
    em2_normalize(post);
    for (int i = 0; i < 9; i++) sfs[i] = post[i];
    it++;
    const double lik = em2_lik(sfs, gl1, gl2);
    if (fabs(lik - old_lik) < tole) break;
    old_lik = lik;
  }
  if (n_iter) *n_iter = it;
}

int64_t ngd_window_ranges(const uint32_t *chrom_id, uint64_t n_sites, uint64_t size, uint64_t step, uint64_t *lo, uint64_t *hi,
                          uint64_t cap) {
  if (!size || !step) return NGD_E_INVALID;
  std::unordered_set<uint32_t> seen;  // ids of the chromosomes met so far (a reappearing one is an error)
  uint64_t count = 0;
  for (uint64_t c0 = 0; c0 < n_sites;) {
    uint64_t c1 = c0 + 1;
    if (chrom_id) {
      while (c1 < n_sites && chrom_id[c1] == chrom_id[c0]) c1++;
      if (!seen.insert(chrom_id[c0]).second) return NGD_E_INVALID;
    } else {
      c1 = n_sites;
    }
    for (uint64_t s = c0; c1 - s >= size; s += step) {
      if (lo && hi && count < cap) {
        lo[count] = s;
        hi[count] = s + size;
      }
      count++;
      if (step > c1 - s) break;  // (s + step would pass the chromosome's end)
    }
    c0 = c1;
  }
  return (int64_t)count;
}

// Windows in coordinates: window k of a chromosome covers [1 + k step_bp, 1 + k step_bp + size_bp).  Positions ascend inside
// a chromosome, so the sites of a window are a range [a, b) and both ends only move forwards.  A window that holds fewer than
// `need` sites can reach `need` only by gaining the site at b: the walk goes straight to the first window that does, so its
// time is sites + kept windows, whatever the coordinate span.
int64_t ngd_window_ranges_bp(const uint32_t *chrom_id, const uint64_t *pos, uint64_t n_sites, uint64_t size_bp, uint64_t step_bp,
                             uint64_t min_sites, uint64_t *lo, uint64_t *hi, uint64_t *bp_start, uint64_t cap) {
  const uint64_t lim = 1ull << 62;
  if (!size_bp || !step_bp || !pos || size_bp >= lim) return NGD_E_INVALID;
  const uint64_t need = std::max<uint64_t>(1, min_sites);
  std::unordered_set<uint32_t> seen;
  uint64_t count = 0;
  for (uint64_t c0 = 0; c0 < n_sites;) {
    uint64_t c1 = c0 + 1;
    if (chrom_id) {
      while (c1 < n_sites && chrom_id[c1] == chrom_id[c0]) c1++;
      if (!seen.insert(chrom_id[c0]).second) return NGD_E_INVALID;
    } else {
      c1 = n_sites;
    }
    for (uint64_t s = c0; s < c1; s++)
      if (!pos[s] || pos[s] >= lim || (s > c0 && pos[s] < pos[s - 1])) return NGD_E_INVALID;
    const uint64_t k_max = (pos[c1 - 1] - 1) / step_bp;
    uint64_t a = c0, b = c0;
    for (uint64_t k = 0; k <= k_max;) {
      const uint64_t start = 1 + k * step_bp;
      while (a < c1 && pos[a] < start) a++;
      if (b < a) b = a;
      while (b < c1 && pos[b] < start + size_bp) b++;
      if (b - a >= need) {
        if (count < cap) {
          if (lo) lo[count] = a;
          if (hi) hi[count] = b;
          if (bp_start) bp_start[count] = start;
        }
        count++;
        k++;
        continue;
      }
      if (b == c1) break;  // (nothing left to gain)
      // the first window whose end passes pos[b]: 1 + k' step + size > pos[b]
      const uint64_t gain = pos[b] > size_bp ? (pos[b] - size_bp - 1) / step_bp + 1 : 0;
      k = std::max(k + 1, gain);
    }
    c0 = c1;
  }
  return (int64_t)count;
}

// The block maps of windows of unequal length.  A run of the reference on a window's cut-down file seeds its generator
// anew (ngsDist.cpp:179-180) and draws n_rep maps of n_blocks = L / block_size blocks (:236, :416-437): what it draws
// depends on n_blocks alone, so windows with one n_blocks -- those of one length among them -- share one set of maps.
int64_t ngd_window_boot_maps(uint64_t seed, const uint64_t *lo, const uint64_t *hi, uint64_t n_win, uint32_t n_rep,
                             uint64_t block_size, uint64_t *block_maps, uint64_t cap, uint64_t *map_off) {
  if (!block_size || (n_win && (!lo || !hi || !map_off))) return NGD_E_INVALID;
  for (uint64_t w = 0; w < n_win; w++)
    if (hi[w] < lo[w]) return NGD_E_INVALID;
  std::vector<uint64_t> order(n_win);  // windows by n_blocks, then by index: a class's offset is set where it first appears
  for (uint64_t w = 0; w < n_win; w++) order[w] = w;
  auto nb = [&](uint64_t w) { return (hi[w] - lo[w]) / block_size; };
  std::sort(order.begin(), order.end(), [&](uint64_t x, uint64_t y) { return nb(x) != nb(y) ? nb(x) < nb(y) : x < y; });
  std::vector<uint64_t> first;  // the first window of every class, then in call order
  for (uint64_t k = 0; k < n_win; k++)
    if (!k || nb(order[k]) != nb(order[k - 1])) first.push_back(order[k]);
  std::sort(first.begin(), first.end());
  uint64_t total = 0;
  std::vector<uint64_t> m;
  for (uint64_t w : first) {
    const uint64_t n_blocks = nb(w);
    map_off[w] = n_blocks && n_rep ? total : 0;
    if (!n_blocks || !n_rep) continue;
    if (block_maps && total < cap) {
      uint32_t st[3];
      ngd_taus_seed(st, seed);
      m.resize((uint64_t)n_rep * n_blocks);
      for (uint32_t r = 0; r < n_rep; r++) ngd_boot_block_map(st, n_blocks, &m[(uint64_t)r * n_blocks]);
      std::copy_n(m.begin(), std::min<uint64_t>(m.size(), cap - total), block_maps + total);
    }
    total += (uint64_t)n_rep * n_blocks;
  }
  // (every other window: the offset of its class's first window, which precedes it in `order`)
  for (uint64_t k = 1; k < n_win; k++)
    if (nb(order[k]) == nb(order[k - 1])) map_off[order[k]] = map_off[order[k - 1]];
  return (int64_t)total;
}

// ---- groups of individuals (--groups): pairs of groups (a, b), a <= b, numbered as the row-major upper triangle WITH the
// diagonal; a group pair's cells are the pairs of individuals i1 < i2 with one in a and one in b (a == b: both in a) ----
uint64_t ngd_n_group_pairs(uint32_t n_groups) { return (uint64_t)n_groups * ((uint64_t)n_groups + 1) / 2; }

uint64_t ngd_group_pair_index(uint32_t n_groups, uint32_t a, uint32_t b) {
  const uint64_t G = n_groups, A = a;
  return A * G - (A ? A * (A - 1) / 2 : 0) + (b - a);
}

int ngd_group_cells(const int32_t *group_of, uint64_t n_ind, uint32_t n_groups, uint64_t *cells) {
  if (!group_of || !n_groups || !cells) return NGD_E_INVALID;
  std::vector<uint64_t> size(n_groups, 0);
  for (uint64_t i = 0; i < n_ind; i++) {
    if (group_of[i] < -1 || group_of[i] >= (int64_t)n_groups) return NGD_E_INVALID;
    if (group_of[i] >= 0) size[group_of[i]]++;
  }
  for (uint32_t a = 0; a < n_groups; a++)
    for (uint32_t b = a; b < n_groups; b++)
      cells[ngd_group_pair_index(n_groups, a, b)] = a == b ? size[a] * (size[a] - (size[a] ? 1 : 0)) / 2 : size[a] * size[b];
  return NGD_OK;
}

}  // extern "C"

// The same for the engine's own use (engine.hip run_dist: a job's tail inside the call), over n_mat matrices of n_pairs cells:
// the counts per cell (cnt), or -- without --pairwise_del, where every pair of a matrix has the same count, ngsDist.cpp:362 --
// one per matrix (cnt_mat), so that no array of counts has to leave the device.  The division is the reference's either
// way (sum / (double)count).
int ngd_finish_matrices_stream(const double *sum, const uint64_t *cnt, const uint64_t *cnt_mat, uint32_t n_mat, uint64_t n_pairs,
                               uint64_t evol_model, double *dist, const volatile uint64_t *landed) {
  if (evol_model > 2) return NGD_E_MODEL;
  if (!sum || (!cnt && !cnt_mat) || !dist || !landed) return NGD_E_INVALID;
  const uint64_t total = (uint64_t)n_mat * n_pairs;
  const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
  const bool wide = total >= (1u << 19) && hw > 16;
  const unsigned nt = wide ? std::min(64u, hw) : std::min(16u, hw);
  // shares of 4096 cells (finish_range's own grain): the cells of the LAST chunk to land are then spread over all the threads
  const unsigned parts = (unsigned)std::min<uint64_t>(std::max<uint64_t>(1, total / 4096), 1u << 20);
  const uint64_t per = (total + parts - 1) / parts;
  auto share = [&](unsigned k) {
    const uint64_t lo = (uint64_t)k * per, hi = std::min(total, lo + per);
    if (lo >= hi) return;
    for (unsigned spins = 0; *landed < hi; spins++) {  // (the engine may be recomputing noted pairs meanwhile: then sleep)
      if (spins < 4096) __builtin_ia32_pause();  // (~0.1 ms; the threads' CPU time counts against the process's quota)
      else std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    if (cnt) {
      finish_range(sum, cnt, lo, hi, 0, evol_model, dist);
      return;
    }
    for (uint64_t a = lo; a < hi;) {  // matrix by matrix: one count each
      const uint64_t m = a / n_pairs, b = std::min(hi, (m + 1) * n_pairs);
      if (cnt_mat[m]) {
        finish_range(sum, nullptr, a, b, cnt_mat[m], evol_model, dist);
      } else {  // (a matrix that visits no site: 0 / 0 as the per-cell form has it)
        const uint64_t zero = 0;
        for (uint64_t c = a; c < b; c++) finish_range(sum + c, &zero, 0, 1, 0, evol_model, dist + c);
      }
      a = b;
    }
  };
  if (nt <= 1 || parts <= 1) {
    for (unsigned k = 0; k < parts; k++) share(k);
  } else {
    // the shares are dealt by a counter of their own, in ascending order (the pool's mutex per part would cost more than a share)
    std::atomic<unsigned> next{0};
    (wide ? host_pool_wide() : host_pool()).run(std::min(nt, parts), [&](unsigned) {
      for (unsigned k; (k = next.fetch_add(1, std::memory_order_relaxed)) < parts;) share(k);
    });
  }
  return NGD_OK;
}

// ---- bootstrap summaries (--boot_stats): the definitions of include/ngsdist_amd.h "Bootstrap summaries" in plain host
// arithmetic, cell by cell: est, then the finite replicates' mean and standard deviation in ascending r (no contraction:
// -ffp-contract=off), then two order statistics of their sorted values ----
int ngd_boot_stats_host(const double *val, uint64_t n_set, uint64_t n_mat, uint64_t n_cells, double ci, double *stats,
                        uint64_t *used) {
  if (!val || !stats || !used || !n_set || n_mat < 2 || !(ci > 0.0 && ci < 1.0)) return NGD_E_INVALID;
  const double p_lo = (1.0 - ci) / 2.0, p_hi = 1.0 - p_lo;
  const uint64_t nan_bits = 0x7FF8000000000000ull;
  double nan;
  memcpy(&nan, &nan_bits, 8);
  std::vector<double> f;
  f.reserve(n_mat);
  for (uint64_t s = 0; s < n_set; s++)
    for (uint64_t c = 0; c < n_cells; c++) {
      const double *v = val + s * n_mat * n_cells + c;
      double *out = stats + s * NGD_BOOT_NSTAT * n_cells + c;
      f.clear();
      double acc = 0.0;
      for (uint64_t r = 1; r < n_mat; r++) {
        const double x = v[r * n_cells];
        if (std::isfinite(x)) { acc += x; f.push_back(x); }
      }
      const uint64_t m = f.size();
      const double mean = m ? acc / (double)m : nan;
      double ss = 0.0;
      for (double x : f) {
        const double d = x - mean;
        ss += d * d;
      }
      out[0] = v[0];
      out[n_cells] = mean;
      out[2 * n_cells] = m >= 2 ? std::sqrt(ss / (double)(m - 1)) : nan;
      out[3 * n_cells] = out[4 * n_cells] = nan;
      if (m) {
        std::sort(f.begin(), f.end());
        const uint64_t k_lo = (uint64_t)std::floor(p_lo * (double)(m - 1));
        const uint64_t k_hi = std::min<uint64_t>(m - 1, (uint64_t)std::ceil(p_hi * (double)(m - 1)));
        out[3 * n_cells] = f[std::min(k_lo, k_hi)];
        out[4 * n_cells] = f[k_hi];
      }
      used[s * n_cells + c] = m;
    }
  return NGD_OK;
}

// ---- neighbour-joining trees (--nj): the contract of include/ngsdist_amd.h "Neighbour-joining trees" in plain host
// arithmetic (no contraction: -ffp-contract=off), matrix by matrix.  The live nodes are a dense prefix of the slots, as in
// nj.hip; the formulas do not depend on it -- Q(a,b) subtracts the row sum of the lower node id first ----
namespace {
void nj_one(const double *val, uint64_t n, int32_t *child, double *len, uint32_t *status, std::vector<double> &D, std::vector<double> &r,
            std::vector<uint32_t> &id) {
  const uint64_t n_pairs = n * (n - 1) / 2, nb = 2 * n - 3;
  bool bad = false;
  for (uint64_t p = 0; p < n_pairs && !bad; p++) bad = !std::isfinite(val[p]);
  if (bad) {
    const uint64_t nan_bits = 0x7FF8000000000000ull;
    double nan;
    memcpy(&nan, &nan_bits, 8);
    for (uint64_t k = 0; k < nb; k++) { child[k] = -1; len[k] = nan; }
    *status = 0;
    return;
  }
  D.assign(n * n, 0.0);
  r.assign(n, 0.0);
  id.resize(n);
  uint64_t p = 0;
  for (uint64_t a = 0; a < n; a++) {
    id[a] = (uint32_t)a;
    for (uint64_t b = a + 1; b < n; b++, p++) D[a * n + b] = D[b * n + a] = val[p];
  }
  for (uint64_t a = 0; a < n; a++) {
    double acc = 0.0;
    for (uint64_t b = 0; b < n; b++)
      if (b != a) acc += D[a * n + b];
    r[a] = acc;
  }
  uint64_t m = n;
  for (uint64_t t = 0; m > 3; t++, m--) {
    const double mm2 = (double)(m - 2);
    bool have = false;
    double bq = 0.0;
    uint32_t ba = 0, bb = 0;
    uint64_t bs = 0, bc = 0;
    for (uint64_t s = 0; s + 1 < m; s++)
      for (uint64_t c = s + 1; c < m; c++) {
        const bool lo = id[s] < id[c];
        const uint32_t a = lo ? id[s] : id[c], b = lo ? id[c] : id[s];
        const double q = (mm2 * D[s * n + c] - (lo ? r[s] : r[c])) - (lo ? r[c] : r[s]);
        if (!have || q < bq || (q == bq && (a < ba || (a == ba && b < bb)))) { have = true; bq = q; ba = a; bb = b; bs = s; bc = c; }
      }
    const uint64_t si = id[bs] == ba ? bs : bc, sj = id[bs] == ba ? bc : bs, su = std::min(si, sj), sr = std::max(si, sj), L = m - 1;
    const double dij = D[si * n + sj], ri = r[si], rj = r[sj];
    const double li = 0.5 * dij + (ri - rj) / (2.0 * mm2);
    child[2 * t] = (int32_t)ba;
    child[2 * t + 1] = (int32_t)bb;
    len[2 * t] = li;
    len[2 * t + 1] = dij - li;
    for (uint64_t k = 0; k < m; k++) {
      if (k == si || k == sj) continue;
      const double dik = D[si * n + k], djk = D[sj * n + k];
      const double duk = 0.5 * ((dik + djk) - dij);
      r[k] = ((r[k] - dik) - djk) + duk;
      D[su * n + k] = D[k * n + su] = duk;
    }
    r[su] = 0.5 * ((ri + rj) - (double)m * dij);
    id[su] = (uint32_t)(n + t);
    if (sr != L) {  // the last live slot moves into the freed one
      for (uint64_t k = 0; k < L; k++)
        if (k != sr) D[sr * n + k] = D[k * n + sr] = D[L * n + k];
      r[sr] = r[L];
      id[sr] = id[L];
    }
  }
  uint64_t s0 = 0, s1 = 1, s2 = 2;
  if (id[s0] > id[s1]) std::swap(s0, s1);
  if (id[s1] > id[s2]) std::swap(s1, s2);
  if (id[s0] > id[s1]) std::swap(s0, s1);
  const double dab = D[s0 * n + s1], dac = D[s0 * n + s2], dbc = D[s1 * n + s2];
  child[nb - 3] = (int32_t)id[s0];
  child[nb - 2] = (int32_t)id[s1];
  child[nb - 1] = (int32_t)id[s2];
  len[nb - 3] = 0.5 * ((dab + dac) - dbc);
  len[nb - 2] = 0.5 * ((dab + dbc) - dac);
  len[nb - 1] = 0.5 * ((dac + dbc) - dab);
  *status = 1;
}

// the bipartitions of one record's joins as leaf sets (n bits in W words each) normalised to the side without leaf 0;
// false: a child entry out of range
bool nj_splits(const int32_t *child, uint64_t n, uint64_t W, std::vector<uint64_t> &sets) {
  const uint64_t n_join = n - 3;
  sets.assign(n_join * W, 0);
  for (uint64_t t = 0; t < n_join; t++) {
    uint64_t *s = &sets[t * W];
    for (int k = 0; k < 2; k++) {
      const int64_t c = child[2 * t + k];
      if (c < 0 || (uint64_t)c >= n + t) return false;
      if ((uint64_t)c < n) s[c / 64] |= 1ull << (c % 64);
      else
        for (uint64_t w = 0; w < W; w++) s[w] |= sets[((uint64_t)c - n) * W + w];
    }
  }
  for (uint64_t t = 0; t < n_join; t++) {  // (after the unions: those need the sets as they grew)
    uint64_t *s = &sets[t * W];
    if (!(s[0] & 1)) continue;
    for (uint64_t w = 0; w < W; w++) s[w] = ~s[w];
    if (n % 64) s[W - 1] &= (1ull << (n % 64)) - 1;
  }
  return true;
}
}  // namespace

int ngd_nj_host(const double *val, uint64_t n_mat, uint64_t n_ind, int32_t *child, double *len, uint32_t *status) {
  if (!val || !child || !len || !status || !n_mat || n_ind < 3) return NGD_E_INVALID;
  const uint64_t n_pairs = n_ind * (n_ind - 1) / 2, nb = 2 * n_ind - 3;
  const unsigned parts = (unsigned)std::min<uint64_t>(n_mat, 1024);
  host_pool().run(parts, [&](unsigned part) {
    std::vector<double> D, r;
    std::vector<uint32_t> id;
    for (uint64_t k = part; k < n_mat; k += parts) nj_one(val + k * n_pairs, n_ind, child + k * nb, len + k * nb, status + k, D, r, id);
  });
  return NGD_OK;
}

int ngd_nj_support(const int32_t *child, const uint32_t *status, uint64_t n_mat, uint64_t n_ind, uint32_t *support, uint32_t *n_used) {
  if (!child || !status || !support || !n_used || !n_mat || n_ind < 3) return NGD_E_INVALID;
  const uint64_t n = n_ind, nb = 2 * n - 3, n_join = n - 3, W = (n + 63) / 64;
  std::vector<uint32_t> sup(n_join, 0);
  uint32_t used = 0;
  if (status[0] && n_join) {
    std::vector<uint64_t> ref, rep;
    if (!nj_splits(child, n, W, ref)) return NGD_E_INVALID;
    // matrix 0's bipartitions, sorted; equal ones (none in a tree of distinct splits) would count alike
    std::vector<uint64_t> order(n_join);
    for (uint64_t t = 0; t < n_join; t++) order[t] = t;
    auto less = [&](const uint64_t *a, const uint64_t *b) { return std::lexicographical_compare(a, a + W, b, b + W); };
    std::sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return less(&ref[a * W], &ref[b * W]); });
    for (uint64_t m = 1; m < n_mat; m++) {
      if (!status[m]) continue;
      if (!nj_splits(child + m * nb, n, W, rep)) return NGD_E_INVALID;
      used++;
      for (uint64_t t = 0; t < n_join; t++) {
        const uint64_t *s = &rep[t * W];
        auto it = std::lower_bound(order.begin(), order.end(), s, [&](uint64_t a, const uint64_t *b) { return less(&ref[a * W], b); });
        for (; it != order.end() && std::equal(s, s + W, &ref[*it * W]); ++it) sup[*it]++;
      }
    }
  } else {
    for (uint64_t m = 1; m < n_mat; m++) used += status[m] != 0;
  }
  for (uint64_t t = 0; t < n_join; t++) support[t] = sup[t];
  *n_used = used;
  return NGD_OK;
}

int64_t ngd_nj_newick(const int32_t *child, const double *len, uint64_t n_ind, const char *const *labels, const uint32_t *support,
                      char *out, uint64_t cap) {
  if (!child || !len || n_ind < 3) return NGD_E_INVALID;
  const uint64_t n = n_ind, nb = 2 * n - 3;
  // (two walks: the first sizes, the second writes -- only into a buffer that holds the whole line)
  const int64_t need = out ? ngd_nj_newick(child, len, n_ind, labels, support, nullptr, 0) : 0;
  if (need < 0) return need;
  char *const dst = out && (uint64_t)need <= cap ? out : nullptr;
  if (out && !dst) return need;
  uint64_t pos = 0;
  auto put = [&](const char *s, size_t k) {
    if (dst) memcpy(dst + pos, s, k);
    pos += k;
  };
  if (child[0] < 0) {
    put(";\n", 2);
    return (int64_t)pos;
  }
  char tmp[512];
  auto put_len = [&](double v) { put(tmp, (size_t)snprintf(tmp, sizeof tmp, ":%.10f", v)); };
  // an entry is a node with the branch above it; (entry, phase) on a stack: no recursion down a caterpillar tree.  The node
  // of entry e may only have been made by an earlier join than the one e belongs to: the walk ends
  std::vector<std::pair<uint64_t, int>> stack;
  put("(", 1);
  for (uint64_t top = nb - 3; top < nb; top++) {
    if (top > nb - 3) put(",", 1);
    stack.emplace_back(top, 0);
    while (!stack.empty()) {
      const uint64_t e = stack.back().first;
      const int phase = stack.back().second;
      stack.pop_back();
      const int64_t c = child[e];
      const uint64_t limit = e >= nb - 3 ? n + (n - 3) : n + e / 2;  // (ids the entry may name)
      if (c < 0 || (uint64_t)c >= limit) return NGD_E_INVALID;
      if ((uint64_t)c < n) {
        if (labels && labels[c]) put(labels[c], strlen(labels[c]));
        else put(tmp, (size_t)snprintf(tmp, sizeof tmp, "Ind_%lu", (unsigned long)c));
        put_len(len[e]);
        continue;
      }
      const uint64_t t = (uint64_t)c - n;
      if (phase == 0) {
        put("(", 1);
        stack.emplace_back(e, 1);
        stack.emplace_back(2 * t, 0);
      } else if (phase == 1) {
        put(",", 1);
        stack.emplace_back(e, 2);
        stack.emplace_back(2 * t + 1, 0);
      } else {
        put(")", 1);
        if (support) put(tmp, (size_t)snprintf(tmp, sizeof tmp, "%u", support[t]));
        put_len(len[e]);
      }
    }
  }
  put(");\n", 3);
  return (int64_t)pos;
}

// ---- classical MDS (--mds): the contract of include/ngsdist_amd.h "Classical MDS" in plain host arithmetic, matrix by
// matrix, by the method of mds.hip: the double-centred matrix, Householder tridiagonalisation (the reflectors stay in the
// rows they eliminate; each one's norm from its row scaled by a power of two, a negligible row tail left alone), every eigenvalue of the tridiagonal matrix by bisection on Sturm counts, the top K vectors by
// inverse iteration with modified Gram-Schmidt, and the reflectors applied in reverse ----
namespace {
const uint32_t kMdsMaxDim = 16;  // ngd_mds_max_dim()
const int kMdsIter = 3;          // solves per vector
const double kMdsEps = 2.220446049250313e-16, kMdsPivMin = 1e-290;

struct MdsWork {
  std::vector<double> S, d, e, e2, lam, w, u0, u1, u2, z;
};

// the start vector of inverse iteration: a fixed function of (component, vector), uniform in (-1, 1), never 0
inline double mds_start(uint32_t i, uint32_t k) {
  uint32_t h = (i + 1) * 2654435761u ^ (k + 1) * 2246822519u;
  h ^= h >> 15; h *= 2246822519u; h ^= h >> 13; h *= 3266489917u; h ^= h >> 16;
  return ((double)(h >> 8) + 0.5) * (1.0 / 8388608.0) - 1.0;
}

// eigenvalues of the (scaled) tridiagonal matrix below x
inline uint64_t mds_count(const double *d, const double *e2, uint64_t n, double x) {
  double q = d[0] - x;
  if (std::fabs(q) < kMdsPivMin) q = -kMdsPivMin;
  uint64_t c = q < 0;
  for (uint64_t i = 1; i < n; i++) {
    q = (d[i] - x) - e2[i - 1] / q;
    if (std::fabs(q) < kMdsPivMin) q = -kMdsPivMin;
    c += q < 0;
  }
  return c;
}

inline double mds_piv(double x, double floor_) { return std::fabs(x) < floor_ ? (std::signbit(x) ? -floor_ : floor_) : x; }

// z <- (T - sh I)^-1 z: LU with partial pivoting, the forward substitution beside it; pivots below `floor_` are raised to it
void mds_solve(const double *d, const double *e, uint64_t n, double sh, double floor_, double *u0, double *u1, double *u2, double *z) {
  double a = d[0] - sh, b = e[0], x = z[0];
  for (uint64_t i = 0; i + 1 < n; i++) {
    const double sub = e[i], dn = d[i + 1] - sh, un = i + 2 < n ? e[i + 1] : 0.0, zn = z[i + 1];
    if (std::fabs(a) >= std::fabs(sub)) {
      const double l = a != 0 ? sub / a : 0.0;
      u0[i] = a; u1[i] = b; u2[i] = 0.0;
      z[i] = x;
      a = dn - l * b; b = un; x = zn - l * x;
    } else {
      const double l = a / sub;
      u0[i] = sub; u1[i] = dn; u2[i] = un;
      z[i] = zn;
      a = b - l * dn; b = -(l * un); x = x - l * zn;
    }
  }
  u0[n - 1] = a;
  z[n - 1] = x / mds_piv(a, floor_);
  z[n - 2] = (z[n - 2] - u1[n - 2] * z[n - 1]) / mds_piv(u0[n - 2], floor_);
  for (uint64_t i = n - 2; i-- > 0;) z[i] = ((z[i] - u1[i] * z[i + 1]) - u2[i] * z[i + 2]) / mds_piv(u0[i], floor_);
}

void mds_one(const double *val, uint64_t n, uint32_t K, double *eig, double *vec, double *tot, uint32_t *status, MdsWork &W) {
  const uint64_t n_pairs = n * (n - 1) / 2;
  bool bad = false;
  for (uint64_t p = 0; p < n_pairs && !bad; p++) bad = !std::isfinite(val[p]);
  if (bad) {
    const uint64_t nan_bits = 0x7FF8000000000000ull;
    double nan;
    memcpy(&nan, &nan_bits, 8);
    for (uint64_t k = 0; k < K; k++) eig[k] = nan;
    for (uint64_t k = 0; k < K * n; k++) vec[k] = nan;
    tot[0] = tot[1] = nan;
    *status = 0;
    return;
  }
  *status = 1;
  W.S.assign(n * n, 0.0);
  for (auto *v : {&W.d, &W.e, &W.e2, &W.lam, &W.w, &W.u0, &W.u1, &W.u2}) v->assign(n, 0.0);
  W.z.assign((uint64_t)K * n, 0.0);
  double *S = W.S.data(), *d = W.d.data(), *e = W.e.data(), *e2 = W.e2.data(), *lam = W.lam.data(), *w = W.w.data(), *Z = W.z.data();
  // A = -0.5 d^2, centred: B_ab = (A_ab - (mean_a + mean_b)) + grand (symmetric bit for bit)
  for (uint64_t a = 0, p = 0; a + 1 < n; a++)
    for (uint64_t b = a + 1; b < n; b++, p++) S[a * n + b] = S[b * n + a] = -0.5 * (val[p] * val[p]);
  double grand = 0.0;
  for (uint64_t a = 0; a < n; a++) {
    double acc = 0.0;
    for (uint64_t b = 0; b < n; b++) acc += S[b * n + a];
    w[a] = acc / (double)n;
  }
  for (uint64_t a = 0; a < n; a++) grand += w[a];
  grand /= (double)n;
  for (uint64_t a = 0; a < n; a++)
    for (uint64_t b = 0; b < n; b++) S[a * n + b] = (S[a * n + b] - (w[a] + w[b])) + grand;
  // a row tail of the trailing block no larger than eps^2 max|B| counts as eliminated (a perturbation of B far below the
  // method's own eps max|B|): the residue of a matrix of few distinct rows shrinks by about eps a step, and followed to the
  // end of the normal range its bits would depend on how far away that end is -- on the scale of the cells
  double bnorm = 0.0;
  for (uint64_t i = 0; i < n * n; i++) bnorm = std::fmax(bnorm, std::fabs(S[i]));
  const double negl = bnorm * kMdsEps * kMdsEps;
  // T = Q^T B Q: step k eliminates row / column k beyond k + 1; row k keeps tau (at k) and v (beyond, v[k + 1] = 1)
  for (uint64_t k = 0; k + 2 < n; k++) {
    double *x = S + k * n;
    const double alpha = x[k + 1];
    double big = 0.0;
    for (uint64_t c = k + 2; c < n; c++) big = std::fmax(big, std::fabs(x[c]));
    d[k] = x[k];
    if (!(big > negl)) {  // nothing to eliminate: H = I
      e[k] = alpha;
      x[k] = 0.0;
      x[k + 1] = 1.0;
      for (uint64_t c = k + 2; c < n; c++) x[c] = 0.0;
      continue;
    }
    // the norm from the row scaled by a power of two to a largest magnitude in [1, 2) (exact; LAPACK dlarfg's remedy): the
    // squares of a row near 1e-154 and below -- the rounding residue of a matrix of few distinct rows gets there -- would
    // leave the normal range, and tau with them 2 / v^T v
    big = std::fmax(big, std::fabs(alpha));
    const int ex = std::isfinite(big) ? std::ilogb(big) : 0;
    const double as = std::scalbn(alpha, -ex);
    double ss = 0.0;
    for (uint64_t c = k + 2; c < n; c++) {
      x[c] = std::scalbn(x[c], -ex);
      ss += x[c] * x[c];
    }
    const double beta = -std::copysign(std::sqrt(as * as + ss), as), tau = (beta - as) / beta, sc = 1.0 / (as - beta);
    e[k] = std::scalbn(beta, ex);
    x[k] = tau;
    x[k + 1] = 1.0;
    for (uint64_t c = k + 2; c < n; c++) x[c] *= sc;
    double pv = 0.0;
    for (uint64_t r = k + 1; r < n; r++) {
      const double *row = S + r * n;
      double acc = 0.0;
      for (uint64_t c = k + 1; c < n; c++) acc += row[c] * x[c];
      w[r] = tau * acc;
      pv += w[r] * x[r];
    }
    const double half = -0.5 * tau * pv;
    for (uint64_t r = k + 1; r < n; r++) w[r] += half * x[r];
    for (uint64_t r = k + 1; r < n; r++) {
      double *row = S + r * n;
      const double xr = x[r], wr = w[r];
      for (uint64_t c = k + 1; c < n; c++) row[c] -= xr * w[c] + wr * x[c];
    }
  }
  d[n - 2] = S[(n - 2) * n + (n - 2)];
  e[n - 2] = S[(n - 2) * n + (n - 1)];
  d[n - 1] = S[(n - 1) * n + (n - 1)];
  e[n - 1] = 0.0;
  double tnorm = 0.0;
  for (uint64_t i = 0; i < n; i++) tnorm = std::max(tnorm, std::fabs(d[i]) + (i ? std::fabs(e[i - 1]) : 0.0) + std::fabs(e[i]));
  if (!(tnorm > 0.0) || !std::isfinite(tnorm)) {  // T = 0: a matrix without variation (or cells beyond the contract)
    const double v = tnorm > 0.0 ? tnorm - tnorm : 0.0;  // (NaN where T overflowed)
    for (uint64_t k = 0; k < K; k++) {
      eig[k] = v;
      for (uint64_t i = 0; i < n; i++) vec[k * n + i] = i == k ? 1.0 + v : v;
    }
    tot[0] = tot[1] = v;
    return;
  }
  // T scaled by a power of two into [1, 2): exact, and the floors below are then absolute
  const int ex = std::ilogb(tnorm);
  for (uint64_t i = 0; i < n; i++) {
    d[i] = std::scalbn(d[i], -ex);
    e[i] = std::scalbn(e[i], -ex);
    e2[i] = e[i] * e[i];
  }
  for (uint64_t j = 0; j < n; j++) {  // eigenvalue j in ascending order: the least x with count(x) > j
    double lo = -2.5, hi = 2.5;
    for (int it = 0; it < 64; it++) {
      const double mid = lo + 0.5 * (hi - lo);
      if (!(mid > lo) || !(mid < hi) || hi - lo < 1e-17) break;
      if (mds_count(d, e2, n, mid) > j) hi = mid;
      else lo = mid;
    }
    lam[j] = lo + 0.5 * (hi - lo);
  }
  double sum = 0.0, pos = 0.0;
  for (uint64_t j = 0; j < n; j++) {
    const double l = std::scalbn(lam[j], ex);
    sum += l;
    if (l > 0.0) pos += l;
  }
  tot[0] = sum;
  tot[1] = pos;
  // the top K vectors of T
  const double floor_ = kMdsEps, pert = 10.0 * kMdsEps * 2.0;
  double sh[kMdsMaxDim];
  for (uint32_t k = 0; k < K; k++) {
    eig[k] = std::scalbn(lam[n - 1 - k], ex);
    sh[k] = lam[n - 1 - k];
    if (k && sh[k - 1] - sh[k] < pert) sh[k] = sh[k - 1] - pert;
    for (uint64_t i = 0; i < n; i++) Z[k * n + i] = mds_start((uint32_t)i, k);
  }
  auto orthonormalise = [&](uint32_t k) {
    double *z = Z + k * n;
    double big = 0.0;
    for (uint64_t i = 0; i < n; i++) big = std::max(big, std::fabs(z[i]));
    if (big > 0.0 && std::isfinite(big)) for (uint64_t i = 0; i < n; i++) z[i] /= big;
    for (int pass = 0; pass < 2; pass++)
      for (uint32_t j = 0; j < k; j++) {
        const double *y = Z + j * n;
        double dot = 0.0;
        for (uint64_t i = 0; i < n; i++) dot += z[i] * y[i];
        for (uint64_t i = 0; i < n; i++) z[i] -= dot * y[i];
      }
    double ss = 0.0;
    for (uint64_t i = 0; i < n; i++) ss += z[i] * z[i];
    const double nrm = std::sqrt(ss);
    if (nrm > 0.0) for (uint64_t i = 0; i < n; i++) z[i] /= nrm;
  };
  for (int it = 0; it < kMdsIter; it++)
    for (uint32_t k = 0; k < K; k++) {
      mds_solve(d, e, n, sh[k], floor_, W.u0.data(), W.u1.data(), W.u2.data(), Z + k * n);
      orthonormalise(k);
    }
  // back through the reflectors, normalised, the component of largest magnitude positive (the lowest index on a tie)
  for (uint64_t k = n - 2; k-- > 0;) {
    const double *x = S + k * n;
    const double tau = x[k];
    if (tau == 0.0) continue;
    for (uint32_t v = 0; v < K; v++) {
      double *z = Z + v * n, dot = 0.0;
      for (uint64_t c = k + 1; c < n; c++) dot += x[c] * z[c];
      const double f = tau * dot;
      for (uint64_t c = k + 1; c < n; c++) z[c] -= f * x[c];
    }
  }
  for (uint32_t v = 0; v < K; v++) {
    double *z = Z + v * n, ss = 0.0, big = -1.0;
    uint64_t at = 0;
    for (uint64_t i = 0; i < n; i++) ss += z[i] * z[i];
    const double nrm = std::sqrt(ss);
    for (uint64_t i = 0; i < n; i++) {
      if (nrm > 0.0) z[i] /= nrm;
      if (std::fabs(z[i]) > big) { big = std::fabs(z[i]); at = i; }
    }
    const bool flip = z[at] < 0.0;
    for (uint64_t i = 0; i < n; i++) vec[v * n + i] = flip ? -z[i] : z[i];
  }
}
}  // namespace

uint32_t ngd_mds_max_dim(void) { return kMdsMaxDim; }

int ngd_mds_host(const double *val, uint64_t n_mat, uint64_t n_ind, uint32_t K, double *eig, double *vec, double *tot, uint32_t *status) {
  if (!val || !eig || !vec || !tot || !status || !n_mat || n_ind < 3 || !K || K > n_ind - 1 || K > kMdsMaxDim) return NGD_E_INVALID;
  const uint64_t n_pairs = n_ind * (n_ind - 1) / 2;
  const unsigned parts = (unsigned)std::min<uint64_t>(n_mat, 1024);
  host_pool().run(parts, [&](unsigned part) {
    MdsWork W;
    for (uint64_t m = part; m < n_mat; m += parts)
      mds_one(val + m * n_pairs, n_ind, K, eig + m * K, vec + m * K * n_ind, tot + m * 2, status + m, W);
  });
  return NGD_OK;
}

int ngd_mds_coords(const double *eig, const double *vec, uint64_t n_mat, uint64_t n_ind, uint32_t K, double *coords) {
  if (!eig || !vec || !coords || !n_mat || n_ind < 3 || !K || K > n_ind - 1 || K > kMdsMaxDim) return NGD_E_INVALID;
  for (uint64_t m = 0; m < n_mat; m++)
    for (uint32_t k = 0; k < K; k++) {
      const double l = eig[m * K + k], s = l > 0.0 ? std::sqrt(l) : l - l;  // (0 for an eigenvalue <= 0, NaN for NaN)
      for (uint64_t i = 0; i < n_ind; i++) coords[(m * n_ind + i) * K + k] = vec[(m * K + k) * n_ind + i] * s;
    }
  return NGD_OK;
}

// ---- alignment of a set's MDS replicates to its matrix 0 (--mds_align): the contract of include/ngsdist_amd.h "Classical
// MDS", alignment, in plain host arithmetic by the method of mds_align.hip: M = X_r^T X_0 from sums in ascending i, its
// orthogonal polar factor by a one-sided Jacobi in cyclic order on M scaled by a power of two, the columns below the floor
// completed by Gram-Schmidt of the unit vectors in order, Y = X_r Q, fit = |Y - X_0|^2 ----
namespace {
const int kAlignSweeps = 64;
const double kAlignFloor = 1e-12;  // a column this far below the largest counts as zero

// q [K][K] = U V^T of m [K][K] = U S V^T (row-major; K <= kMdsMaxDim)
void align_polar(const double *m, uint32_t K, double *q) {
  double A[kMdsMaxDim * kMdsMaxDim], V[kMdsMaxDim * kMdsMaxDim], nrm[kMdsMaxDim], w[kMdsMaxDim];
  bool done[kMdsMaxDim];
  double big = 0.0;
  for (uint32_t i = 0; i < K * K; i++) big = std::max(big, std::fabs(m[i]));
  const bool any = big > 0.0 && std::isfinite(big);
  const int ex = any ? std::ilogb(big) : 0;
  for (uint32_t i = 0; i < K * K; i++) {
    A[i] = any ? std::scalbn(m[i], -ex) : 0.0;
    V[i] = i / K == i % K ? 1.0 : 0.0;
  }
  for (int sweep = 0; any && sweep < kAlignSweeps; sweep++) {
    double top = 0.0;
    for (uint32_t j = 0; j < K; j++) {
      double s = 0.0;
      for (uint32_t i = 0; i < K; i++) s += A[i * K + j] * A[i * K + j];
      top = std::max(top, s);
    }
    const double floor2 = (kAlignFloor * kAlignFloor) * top;
    bool rotated = false;
    for (uint32_t p = 0; p + 1 < K; p++)
      for (uint32_t r = p + 1; r < K; r++) {
        double a = 0.0, b = 0.0, g = 0.0;
        for (uint32_t i = 0; i < K; i++) {
          const double x = A[i * K + p], y = A[i * K + r];
          a += x * x;
          b += y * y;
          g += x * y;
        }
        if (!(a > floor2) || !(b > floor2) || !(std::fabs(g) > kMdsEps * std::sqrt(a * b))) continue;
        const double zeta = (b - a) / (2.0 * g), t = std::copysign(1.0, zeta) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / std::sqrt(1.0 + t * t), s = c * t;
        for (uint32_t i = 0; i < K; i++) {
          const double x = A[i * K + p], y = A[i * K + r], vx = V[i * K + p], vy = V[i * K + r];
          A[i * K + p] = c * x - s * y;
          A[i * K + r] = s * x + c * y;
          V[i * K + p] = c * vx - s * vy;
          V[i * K + r] = s * vx + c * vy;
        }
        rotated = true;
      }
    if (!rotated) break;
  }
  // U: the columns above the floor normalised (A holds U from here on) ...
  double top = 0.0;
  for (uint32_t j = 0; j < K; j++) {
    double s = 0.0;
    for (uint32_t i = 0; i < K; i++) s += A[i * K + j] * A[i * K + j];
    nrm[j] = std::sqrt(s);
    top = std::max(top, nrm[j]);
  }
  for (uint32_t j = 0; j < K; j++) {
    done[j] = nrm[j] > kAlignFloor * top;
    if (done[j])
      for (uint32_t i = 0; i < K; i++) A[i * K + j] /= nrm[j];
  }
  // ... the others from e_0, e_1, .. in order, twice against the finished columns: the first that keeps enough of itself
  const double keep = 0.5 / std::sqrt((double)K);
  uint32_t next = 0;
  for (uint32_t j = 0; j < K; j++) {
    if (done[j]) continue;
    for (; next < K; next++) {
      for (uint32_t i = 0; i < K; i++) w[i] = i == next ? 1.0 : 0.0;
      for (int pass = 0; pass < 2; pass++)
        for (uint32_t u = 0; u < K; u++) {
          if (!done[u]) continue;
          double dot = 0.0;
          for (uint32_t i = 0; i < K; i++) dot += A[i * K + u] * w[i];
          for (uint32_t i = 0; i < K; i++) w[i] -= dot * A[i * K + u];
        }
      double s = 0.0;
      for (uint32_t i = 0; i < K; i++) s += w[i] * w[i];
      s = std::sqrt(s);
      if (s > keep) {
        for (uint32_t i = 0; i < K; i++) A[i * K + j] = w[i] / s;
        break;
      }
    }
    done[j] = true;
    next++;
  }
  for (uint32_t a = 0; a < K; a++)
    for (uint32_t b = 0; b < K; b++) {
      double s = 0.0;
      for (uint32_t j = 0; j < K; j++) s += A[a * K + j] * V[b * K + j];
      q[a * K + b] = s;
    }
}

// x [K][n] = vec [K][n] scaled by the roots of eig (ngd_mds_coords' formula)
void align_coords(const double *eig, const double *vec, uint64_t n, uint32_t K, double *x) {
  for (uint32_t k = 0; k < K; k++) {
    const double l = eig[k], s = l > 0.0 ? std::sqrt(l) : l - l;
    for (uint64_t i = 0; i < n; i++) x[k * n + i] = vec[k * n + i] * s;
  }
}
}  // namespace

int ngd_mds_align_host(const double *eig, const double *vec, const uint32_t *status, uint64_t n_set, uint64_t n_mat, uint64_t n_ind,
                       uint32_t K, double *aligned, double *fit) {
  if (!eig || !vec || !aligned || !fit || !n_set || !n_mat || n_ind < 3 || !K || K > n_ind - 1 || K > kMdsMaxDim) return NGD_E_INVALID;
  const uint64_t n = n_ind, total = n_set * n_mat, nan_bits = 0x7FF8000000000000ull;
  double nan;
  memcpy(&nan, &nan_bits, 8);
  const unsigned parts = (unsigned)std::min<uint64_t>(total, 1024);
  host_pool().run(parts, [&](unsigned part) {
    std::vector<double> x0(K * n);
    double M[kMdsMaxDim * kMdsMaxDim], Q[kMdsMaxDim * kMdsMaxDim], xi[kMdsMaxDim];
    for (uint64_t m = part; m < total; m += parts) {
      const uint64_t m0 = m / n_mat * n_mat;
      double *y = aligned + m * K * n;
      if (status && (!status[m] || !status[m0])) {
        for (uint64_t i = 0; i < K * n; i++) y[i] = nan;
        fit[m] = nan;
        continue;
      }
      align_coords(eig + m * K, vec + m * K * n, n, K, y);
      if (m == m0) {
        fit[m] = 0.0;
        continue;
      }
      align_coords(eig + m0 * K, vec + m0 * K * n, n, K, x0.data());
      for (uint32_t a = 0; a < K; a++)
        for (uint32_t b = 0; b < K; b++) {
          double s = 0.0;
          for (uint64_t i = 0; i < n; i++) s += y[a * n + i] * x0[b * n + i];
          M[a * K + b] = s;
        }
      align_polar(M, K, Q);
      double f = 0.0;
      for (uint64_t i = 0; i < n; i++) {
        for (uint32_t a = 0; a < K; a++) xi[a] = y[a * n + i];
        for (uint32_t b = 0; b < K; b++) {
          double s = 0.0;
          for (uint32_t a = 0; a < K; a++) s += xi[a] * Q[a * K + b];
          y[b * n + i] = s;
          const double d = s - x0[b * n + i];
          f += d * d;
        }
      }
      fit[m] = f;
    }
  });
  return NGD_OK;
}

// ---- comparison of windows (--win_cmp): the contract of include/ngsdist_amd.h "Comparison of windows" in plain host
// arithmetic -- sums in slices of ngd_win_cmp_slice() cells, a slice's cells in order, the slices in ascending order --, the
// cut of the cell axis that win_cmp.hip follows too (win_cmp_geom.h), and the derived tables.
uint32_t ngd_win_cmp_max_vec(void) { return NGD_WIN_CMP_MAX_VEC; }
uint64_t ngd_win_cmp_slice(uint64_t n_vec, uint64_t n_cells) { return ngd_wincmp_slice(n_vec, n_cells); }

namespace {
// SUM_c f(c) over [0, P) in slices of s cells
template <typename F>
inline double sliced_sum(uint64_t P, uint64_t s, F f) {
  double total = 0.0;
  for (uint64_t c0 = 0; c0 < P; c0 += s) {
    const uint64_t c1 = std::min(P, c0 + s);
    double part = 0.0;
    for (uint64_t c = c0; c < c1; c++) part += f(c);
    total = c0 ? total + part : part;
  }
  return total;
}
}  // namespace

int ngd_win_cmp_host(const double *values, uint64_t n_vec, uint64_t n_cells, double *mean, double *gram, uint32_t *status) {
  if (!values || !mean || !gram || !status || !n_vec || !n_cells || n_vec > ngd_win_cmp_max_vec()) return NGD_E_INVALID;
  const uint64_t W = n_vec, P = n_cells, s = ngd_win_cmp_slice(W, P);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const unsigned parts = (unsigned)std::min<uint64_t>(W, 1024);
  std::vector<double> Z(W * P);
  host_pool().run(parts, [&](unsigned part) {
    for (uint64_t w = part; w < W; w += parts) {
      const double *x = values + w * P;
      bool ok = true;
      for (uint64_t c = 0; c < P; c++) ok = ok && std::isfinite(x[c]);
      status[w] = ok ? 1u : 0u;
      mean[w] = ok ? sliced_sum(P, s, [&](uint64_t c) { return x[c]; }) / (double)P : nan;
      for (uint64_t c = 0; c < P; c++) Z[w * P + c] = ok ? x[c] - mean[w] : 0.0;
    }
  });
  host_pool().run(parts, [&](unsigned part) {
    for (uint64_t a = part; a < W; a += parts)
      for (uint64_t b = a; b < W; b++) {
        const double *za = &Z[a * P], *zb = &Z[b * P];
        const double g = status[a] && status[b] ? sliced_sum(P, s, [&](uint64_t c) { return za[c] * zb[c]; }) : nan;
        gram[a * W + b] = gram[b * W + a] = g;
      }
  });
  return NGD_OK;
}

int ngd_win_cmp_finish(const double *mean, const double *gram, const uint32_t *status, uint64_t n_vec, uint64_t n_cells, double *cor,
                       double *rms) {
  if (!mean || !gram || !status || !cor || !rms || !n_vec || !n_cells) return NGD_E_INVALID;
  const uint64_t W = n_vec;
  const double nan = std::numeric_limits<double>::quiet_NaN(), P = (double)n_cells;
  for (uint64_t a = 0; a < W; a++)
    for (uint64_t b = 0; b < W; b++) {
      const uint64_t at = a * W + b;
      if (!status[a] || !status[b]) {
        cor[at] = rms[at] = nan;
        continue;
      }
      const double gaa = gram[a * W + a], gbb = gram[b * W + b], gab = gram[at], dm = mean[a] - mean[b];
      // (two diagonals near 2^-1000, or near 2^+600, leave no normal product: the roots one by one then)
      const double prod = gaa * gbb;
      cor[at] = gaa == 0.0 || gbb == 0.0 ? nan : gab / (std::isnormal(prod) ? std::sqrt(prod) : std::sqrt(gaa) * std::sqrt(gbb));
      const double q = gaa + gbb - 2 * gab + P * (dm * dm);
      rms[at] = a == b ? 0.0 : std::sqrt((q > 0.0 ? q : 0.0) / P);
    }
  return NGD_OK;
}
