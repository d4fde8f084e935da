// engine_create.hip -- devices, and an engine's life: ngd_create (checks, shard, job list, resident images, slices) and
// ngd_destroy.
#include "ngd_engine.h"

// Single-image engines: k-groups of the second operand image formed at a time by default (4 GB of them)
static uint64_t single_image_span(const ngd_geom &g) {
  return std::max<uint64_t>(1, std::min<uint64_t>(g.n_kg, (4ull << 30) / ((uint64_t)g.n_ig * 64 * 8)));
}

int ngd_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int ngd_device_memory(int device, uint64_t *free_bytes, uint64_t *total_bytes) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n < 1) return fail(NGD_E_NODEVICE, "ngd_device_memory: no HIP device");
  int cur = 0;
  HIPCHK(hipGetDevice(&cur));
  if (device < 0) device = cur;
  if (device >= n) return fail(NGD_E_NODEVICE, "ngd_device_memory: device ordinal out of range");
  HIPCHK(hipSetDevice(device));
  size_t f = 0, t = 0;
  HIPCHK(hipMemGetInfo(&f, &t));
  HIPCHK(hipSetDevice(cur));
  if (free_bytes) *free_bytes = f;
  if (total_bytes) *total_bytes = t;
  return NGD_OK;
}

// What is about ORDER: every thread of the engine's joined and every stream idle; then the members go -- each buffer and
// ring slot frees itself (ngd_buffers.h) --; then the streams and events they were used on.
void ngd_destroy(ngd_engine *e) {
  if (!e) return;
  hipSetDevice(e->device);
  if (e->piece_thread.joinable()) e->piece_thread.join();
  if (e->st) hipStreamSynchronize(e->st);
  if (e->st_eager) hipStreamSynchronize(e->st_eager);  // (slices started beside a load and never asked for)
  ring_maker_join(e);
  stage_reap(e);
  if (e->out.st) hipStreamSynchronize(e->out.st);
  if (e->out.st2) hipStreamSynchronize(e->out.st2);
  const hipStream_t streams[] = {e->st_copy[0], e->st_copy[1], e->st_eager, e->out.st, e->out.st2, e->st};
  std::vector<hipEvent_t> events(e->ev, e->ev + 5);
  events.push_back(e->ev_eager);
  events.insert(events.end(), e->out.pool.begin(), e->out.pool.end());
  events.insert(events.end(), e->ev_spill.begin(), e->ev_spill.end());
  delete e;
  for (hipEvent_t v : events)
    if (v) hipEventDestroy(v);
  for (hipStream_t st : streams)
    if (st) hipStreamDestroy(st);
}

// ngd_create's hold on the engine it is making: a step that fails has said why (fail()) and returns; the engine goes, the
// message stays
namespace {
struct create_bail {
  void operator()(ngd_engine *e) const {
    std::string keep = g_err;
    ngd_destroy(e);
    (void)hipGetLastError();  // reported through the step's code; not again by the next launch's check
    g_err = keep;
  }
};
}  // namespace

#define TRY(x)                        \
  do {                                \
    int rc_ = (x);                    \
    if (rc_ != NGD_OK) return rc_;    \
  } while (0)

static int create_check(const ngd_config *cfg, uint32_t world) {
  if (cfg->n_ind < 2) return fail(NGD_E_INVALID, "ngd_create: need at least 2 individuals");
  if (cfg->n_sites < 1) return fail(NGD_E_INVALID, "ngd_create: need at least 1 site");
  // tile lists index groups of 16 individuals with 16 bits; what bounds n_ind in practice is device memory (two
  // n_pairs-long result arrays + one n_pad x n_pad plane per slice), checked below before any list is built
  if ((cfg->n_ind + 127) / 128 * 8 > 65535) return fail(NGD_E_INVALID, "ngd_create: n_ind above 1 048 448 (16-bit tile indices)");
  if (cfg->single_image > 3) return fail(NGD_E_INVALID, "ngd_create: single_image is 0 (auto), 1, 2 or 3 (two images)");
  if (cfg->second_image_mib && cfg->single_image != 1)
    return fail(NGD_E_INVALID, "ngd_create: second_image_mib belongs to single_image = 1 engines");
  if (cfg->exact_shapes > 7)
    return fail(NGD_E_INVALID, "ngd_create: exact_shapes must be 0 (auto), 1 (never), 2 (blocks of 4 x 4 tiles), 3 (2 x 4), 4 "
                               "(4 x 4, a slice's jobs in one workgroup), 5 (2 x 4, one workgroup), 6 (5 with operands "
                               "through LDS) or 7 (full blocks, triangular on the diagonal)");
  if (cfg->variant > 4) return fail(NGD_E_INVALID, "ngd_create: no such kernel variant");
  if (cfg->shard_rank >= world) return fail(NGD_E_INVALID, "ngd_create: shard_rank >= shard_world");
  return NGD_OK;
}

static int create_device(const ngd_config *cfg, int &dev, int &kernel) {
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev < 1)
    return fail(NGD_E_NODEVICE, "ngd_create: no HIP device (this engine has no CPU path)");
  dev = cfg->device;
  if (dev < 0) HIPCHK(hipGetDevice(&dev));
  if (dev >= n_dev) return fail(NGD_E_NODEVICE, "ngd_create: device ordinal out of range");
  HIPCHK(hipSetDevice(dev));
  kernel = cfg->kernel;
  if (cfg->indep_geno) {
    if (kernel == NGD_KERNEL_AUTO) kernel = NGD_KERNEL_MFMA;
    if (kernel != NGD_KERNEL_MFMA && kernel != NGD_KERNEL_STREAM)
      return fail(NGD_E_INVALID, "ngd_create: kernel does not serve --indep_geno");
  } else {
    // up to 32 individuals the whole job is three 16 x 16 tiles of the per-pair kernel, against one 64 x 64 tile of the
    // table kernel that is 7-25 % occupied ([measured] 300 000 sites: n_ind = 24: 2.5 ms vs 4.5 ms; 48: 5.6 vs 5.5; 64: 9.3
    // vs 6.0; 200: 86 vs 51; 400: 306 vs 151)
    if (kernel == NGD_KERNEL_AUTO) kernel = cfg->n_ind <= 32 ? NGD_KERNEL_EM_FAST : NGD_KERNEL_EM_TABLE;
    if (kernel != NGD_KERNEL_EM_FAST && kernel != NGD_KERNEL_EM_FAITHFUL && kernel != NGD_KERNEL_EM_TABLE)
      return fail(NGD_E_INVALID, "ngd_create: kernel does not serve the EM path");
  }
  return NGD_OK;
}

// before any list is built: the two result arrays + the fewest slab planes this kernel works with must fit at all
static int create_fits(const ngd_config *cfg, int &kernel) {
  size_t free_b = 0, total_b = 0;
  HIPCHK(hipMemGetInfo(&free_b, &total_b));
  const uint64_t n_pad = (cfg->n_ind + 127) / 128 * 128;
  // tens of thousands of individuals: the MFMA kernel's 8 planes of n_pad^2 doubles (its XCD deal wants 8 slices) no
  // longer fit beside the results -- `auto` then means the streaming kernel, which writes the results directly
  if (cfg->kernel == NGD_KERNEL_AUTO && kernel == NGD_KERNEL_MFMA &&
      ngd_n_pairs(cfg->n_ind) * 16 + 8 * n_pad * n_pad * 8 > total_b)
    kernel = NGD_KERNEL_STREAM;
  const uint64_t planes = kernel == NGD_KERNEL_MFMA ? 8 : kernel == NGD_KERNEL_STREAM ? 0 : 1;
  if (ngd_n_pairs(cfg->n_ind) * 16 + planes * n_pad * n_pad * 8 > total_b)
    return fail(NGD_E_NOMEM, "ngd_create: the result arrays and slabs of this many individuals exceed the device's memory");
  return NGD_OK;
}

static int create_geometry(ngd_engine *e, const ngd_config *cfg, uint32_t world, int dev, int kernel) {
  e->cfg = *cfg;
  e->cfg.shard_world = world;
  e->device = dev;
  e->kernel = kernel;
  memcpy(e->sc.v, cfg->score, sizeof(e->sc.v));
  {
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) == hipSuccess && khz > 0) e->wall_khz = khz;
  }

  ngd_geom &g = e->g;
  g.n_ind = cfg->n_ind;
  g.n_sites = cfg->n_sites;
  g.n_sites_pad = (cfg->n_sites + 15) / 16 * 16;  // -> n_kg is a multiple of 12
  g.n_kg = 3 * g.n_sites_pad / 4;
  g.n_t = (uint32_t)((cfg->n_ind + NGD_TILE - 1) / NGD_TILE);
  g.n_pad = g.n_t * NGD_TILE;
  g.n_ig = g.n_pad / NGD_IG;
  g.n_words = (uint32_t)((cfg->n_sites + 63) / 64);

  if (hipStreamCreateWithFlags(&e->st, hipStreamNonBlocking) != hipSuccess)
    return fail(NGD_E_HIP, "ngd_create: hipStreamCreate failed");
  for (auto &v : e->ev)
    if (hipEventCreate(&v) != hipSuccess) return fail(NGD_E_HIP, "ngd_create: hipEventCreate failed");
  return NGD_OK;
}

// ---- shard: upper-triangular 128-tiles dealt by cost over ranks (ngd_shard.h) ----
static void create_shard(ngd_engine *e, const std::vector<uint32_t> &owner, std::vector<ngd_tile> &tiles,
                         std::vector<ngd_tile> &tiles16, std::vector<ngd_tile> &tiles64) {
  const ngd_config *cfg = &e->cfg;
  const ngd_geom &g = e->g;
  uint32_t tid = 0;
  for (uint32_t ti = 0; ti < g.n_t; ti++)
    for (uint32_t tj = ti; tj < g.n_t; tj++, tid++) {
      if (owner[tid] != cfg->shard_rank) continue;
      tiles.push_back({(uint16_t)ti, (uint16_t)tj});
      for (uint32_t a = 0; a < 2; a++)  // 64 x 64 tiles of the table-driven EM kernel
        for (uint32_t b = 0; b < 2; b++) {
          const uint32_t i64 = 2 * ti + a, j64 = 2 * tj + b;
          if (i64 > j64 || (uint64_t)i64 * 64 >= g.n_ind || (uint64_t)j64 * 64 >= g.n_ind) continue;
          tiles64.push_back({(uint16_t)i64, (uint16_t)j64});
        }
      for (uint32_t a = 0; a < NGD_IG_PER_TILE; a++)
        for (uint32_t b = 0; b < NGD_IG_PER_TILE; b++) {
          uint32_t ig = ti * NGD_IG_PER_TILE + a, jg = tj * NGD_IG_PER_TILE + b;
          if (ig > jg) continue;                                  // strictly lower: no i<j pair
          if ((uint64_t)ig * 16 >= g.n_ind || (uint64_t)jg * 16 >= g.n_ind) continue;  // all padding
          tiles16.push_back({(uint16_t)ig, (uint16_t)jg});
        }
    }
  e->n_tiles = (uint32_t)tiles.size();
  e->n_tiles16 = (uint32_t)tiles16.size();
  e->n_tiles64 = (uint32_t)tiles64.size();
}

// job list of the MFMA kernel (ngd_job, units of 16 individuals).
static int create_jobs(ngd_engine *e, const std::vector<uint32_t> &owner, const std::vector<ngd_tile> &tiles, std::vector<ngd_job> &jobs) {
  const ngd_config *cfg = &e->cfg;
  const ngd_geom &g = e->g;
  const uint32_t world = cfg->shard_world;
  const uint32_t n_igv = (uint32_t)((g.n_ind + 15) / 16);  // groups that hold at least one individual
  // auto: up to 384 individuals only the tiles a block needs are issued (accum_mfma.hip EXACT); where a slice's jobs fit
  // one workgroup they run in step, each operand fragment leaving HBM once: up to 13 groups of 16 individuals as 16
  // blocks of 2 x 4 tiles with the operands staged through LDS, up to 16 groups as 10 blocks of 4 x 4 ([measured]
  // 100 000 sites, ms per matrix, plain / in step: n_ind = 100: 0.143 / 0.108; 200: 0.356 / 0.262; 250: 0.427 / 0.387;
  // the forms fall back where a slice's jobs do not fit one workgroup)
  e->exact_shapes = cfg->exact_shapes ? (cfg->exact_shapes == 1 || cfg->exact_shapes == 7 ? 0 : (int)cfg->exact_shapes - 1)
                                      : (g.n_pad > 384 ? 0 : n_igv <= 13 ? 5 : n_igv <= 16 ? 3 : 1);
  // Above 384 padded individuals every block runs the full 4 x 4 pattern (form 0).  ngd_config.exact_shapes = 7: the
  // blocks ON the diagonal leave out the 6 tiles below it (10 of 16; on a one-image engine their row fragments are their
  // column fragments: 4 loads per k-group instead of 8) -- measured, not the default (see accum_mfma.hip).
  e->tri_diag = cfg->exact_shapes == 7;
  if (e->exact_shapes == 2 || e->exact_shapes >= 4) {
    // strips of two row groups, cut into blocks of four column groups from the diagonal on (the first block of a strip
    // is triangular: 7 tiles of 8); an odd last row is its diagonal tile.  Under pair-tile sharding blocks must not
    // straddle a 128-tile (8 groups): the first block of a strip then ends at the next multiple of four.
    const bool aligned = world > 1;
    for (uint32_t r = 0; r < n_igv; r += 2) {
      if (n_igv - r == 1) {
        if (owner[ngd_tile_id(g.n_t, r / 8, r / 8)] == cfg->shard_rank) jobs.push_back({(uint16_t)r, (uint16_t)r, 1, 1, 1, 0});
        break;
      }
      for (uint32_t c = r; c < n_igv;) {
        uint32_t w = std::min(4u, n_igv - c);
        if (aligned && c % 4) w = std::min(w, 4 - c % 4);
        if (owner[ngd_tile_id(g.n_t, r / 8, c / 8)] == cfg->shard_rank)
          jobs.push_back({(uint16_t)r, (uint16_t)c, 2, (uint8_t)w, (uint8_t)(c == r), 0});
        c += w;
      }
    }
    auto cost = [](const ngd_job &j) { return j.tri ? j.rows * j.cols - (j.rows > 1 ? 1 : 0) : j.rows * j.cols; };
    std::stable_sort(jobs.begin(), jobs.end(), [&](const ngd_job &a, const ngd_job &b) { return cost(a) > cost(b); });
  } else if (e->exact_shapes) {  // (1, or 3: the same blocks, one workgroup per slice)
    // blocks of up to 4 x 4 groups over the valid groups only; the last block row / column is narrower,
    // blocks on the diagonal are triangular.  Most expensive first, four to a workgroup.
    const uint32_t nb = (n_igv + 3) / 4;
    for (uint32_t bi = 0; bi < nb; bi++)
      for (uint32_t bj = bi; bj < nb; bj++) {
        if (owner[ngd_tile_id(g.n_t, bi / 2, bj / 2)] != cfg->shard_rank) continue;
        const uint8_t r = (uint8_t)std::min(4u, n_igv - 4 * bi), c = (uint8_t)std::min(4u, n_igv - 4 * bj);
        jobs.push_back({(uint16_t)(4 * bi), (uint16_t)(4 * bj), r, c, (uint8_t)(bi == bj), 0});
      }
    auto cost = [](const ngd_job &j) { return j.tri ? j.rows * (j.rows + 1) / 2 : j.rows * j.cols; };
    std::stable_sort(jobs.begin(), jobs.end(), [&](const ngd_job &a, const ngd_job &b) { return cost(a) > cost(b); });
  } else {
    // Off-diagonal 128-tile -> its four 64x64 blocks in one workgroup (they share operands); the blocks of
    // the diagonal tiles (two on the diagonal, one above it) follow, packed four to a workgroup.  Every
    // block runs the full 4x4 pattern, so all workgroups of a slice progress at one rate --
    // tri_diag: the blocks ON the diagonal are triangular (10 tiles of 16) and come last, in workgroups of their
    // own, so that the four jobs of a workgroup still move through the sites together.
    std::vector<ngd_job> diag, ondiag;
    auto live = [&](uint32_t r, uint32_t c) { return r < n_igv && c < n_igv; };
    for (const ngd_tile &t : tiles) {
      const uint16_t r0 = t.ti * NGD_IG_PER_TILE, c0 = t.tj * NGD_IG_PER_TILE;
      if (t.ti != t.tj) {
        for (uint16_t a = 0; a < 2; a++)
          for (uint16_t b = 0; b < 2; b++) {
            ngd_job j = {(uint16_t)(r0 + 4 * a), (uint16_t)(c0 + 4 * b), 4, 4, 0, 0};
            if (!live(j.ig0, j.jg0)) j.rows = 0;  // only padding individuals
            jobs.push_back(j);
          }
      } else {
        const uint8_t tri = e->tri_diag ? 1 : 0;
        const ngd_job d[3] = {{r0, c0, 4, 4, tri, 0}, {r0, (uint16_t)(c0 + 4), 4, 4, 0, 0},
                              {(uint16_t)(r0 + 4), (uint16_t)(c0 + 4), 4, 4, tri, 0}};
        for (const ngd_job &j : d)
          if (live(j.ig0, j.jg0)) (j.tri ? ondiag : diag).push_back(j);
      }
    }
    for (const ngd_job &j : diag) jobs.push_back(j);
    if (!ondiag.empty()) {
      while (jobs.size() % 4) jobs.push_back({0, 0, 0, 0, 0, 0});  // (a workgroup of triangular blocks only)
      for (const ngd_job &j : ondiag) jobs.push_back(j);
    }
  }
  if (e->exact_shapes >= 3) {
    // One workgroup per slice, its wavefronts in step (accum_mfma.hip EXACT = 3 / 4): wavefront w runs on SIMD w % 4, so
    // the jobs are dealt, most expensive first, to the least loaded of four bins and wavefront w takes bin w % 4's
    // next job.  At most 12 wavefronts of 4 x 4 blocks (3 per SIMD at that kernel's register count) or 16 of 2 x 4:
    // else the plain exact form of the same blocks.
    const bool small = e->exact_shapes >= 4;
    auto cost = [&](const ngd_job &j) {
      return small ? (j.tri ? j.rows * j.cols - (j.rows > 1 ? 1 : 0) : j.rows * j.cols)
                   : (j.tri ? j.rows * (j.rows + 1) / 2 : j.rows * j.cols);
    };
    std::vector<ngd_job> bin[4];
    uint32_t load[4] = {0, 0, 0, 0};
    for (const ngd_job &j : jobs) {
      uint32_t b = 0;
      for (uint32_t q = 1; q < 4; q++)
        if (load[q] < load[b]) b = q;
      bin[b].push_back(j);
      load[b] += cost(j);
    }
    std::stable_sort(bin, bin + 4, [](const std::vector<ngd_job> &a, const std::vector<ngd_job> &b) { return a.size() > b.size(); });
    if (jobs.empty() || bin[0].size() > (small ? 4u : 3u)) {
      e->exact_shapes = small ? 2 : 1;
    } else {  // (the fuller bins first: no padding wavefront before the last real one)
      jobs.clear();
      for (size_t d = 0; d < bin[0].size(); d++)
        for (uint32_t b = 0; b < 4; b++)
          if (d < bin[b].size()) jobs.push_back(bin[b][d]);
    }
  }
  for (const ngd_job &j : jobs)  // every block must have a code path in the kernel's form (accum_mfma.hip)
    if (!ngd_mfma_shape_listed(e->exact_shapes, j.rows, j.cols, j.tri))
      return fail(NGD_E_HIP, "ngd_create: internal -- a block shape the MFMA kernel's form does not list");
  const uint32_t jobs_per_wg = e->exact_shapes >= 3 ? (uint32_t)jobs.size() : e->exact_shapes ? 1 : 4;
  e->wg_waves = jobs_per_wg;
  while (jobs.size() % jobs_per_wg) jobs.push_back({0, 0, 0, 0, 0, 0});
  e->n_wg = (uint32_t)(jobs.size() / jobs_per_wg);
  return NGD_OK;
}

// the pairs this engine owns (the streaming kernel under sharding: their list)
static void create_owned_pairs(ngd_engine *e, const std::vector<ngd_tile> &tiles, std::vector<uint64_t> &pairs) {
  const ngd_geom &g = e->g;
  const int kernel = e->kernel;
  const uint32_t world = e->cfg.shard_world;
  if (kernel == NGD_KERNEL_STREAM && world > 1) {
    for (const ngd_tile &t : tiles)
      for (uint64_t i = (uint64_t)t.ti * NGD_TILE; i < std::min<uint64_t>(g.n_ind, (t.ti + 1ull) * NGD_TILE); i++)
        for (uint64_t j = std::max<uint64_t>(i + 1, (uint64_t)t.tj * NGD_TILE);
             j < std::min<uint64_t>(g.n_ind, (t.tj + 1ull) * NGD_TILE); j++)
          pairs.push_back(ngd_pair_idx(g.n_ind, i, j));
    std::sort(pairs.begin(), pairs.end());
    e->n_owned_pairs = pairs.size();
  } else {
    e->n_owned_pairs = 0;
    for (const ngd_tile &t : tiles)
      for (uint64_t i = (uint64_t)t.ti * NGD_TILE; i < std::min<uint64_t>(g.n_ind, (t.ti + 1ull) * NGD_TILE); i++) {
        uint64_t jlo = std::max<uint64_t>(i + 1, (uint64_t)t.tj * NGD_TILE);
        uint64_t jhi = std::min<uint64_t>(g.n_ind, (t.tj + 1ull) * NGD_TILE);
        if (jhi > jlo) e->n_owned_pairs += jhi - jlo;
      }
  }
}

static int create_lists_to_device(ngd_engine *e, const std::vector<ngd_tile> &tiles, const std::vector<ngd_tile> &tiles16,
                                  const std::vector<ngd_tile> &tiles64, const std::vector<uint64_t> &pairs,
                                  const std::vector<ngd_job> &jobs) {
  auto to_device = [&](auto &buf, const auto &v, const char *what) -> int {
    if (int rc_a = buf.alloc(e, v.size(), false)) return rc_a;
    if (!v.empty() && hipMemcpy(buf, v.data(), v.size() * sizeof(v[0]), hipMemcpyHostToDevice) != hipSuccess)
      return fail(NGD_E_HIP, std::string("ngd_create: ") + what + " upload failed");
    return NGD_OK;
  };
  TRY(to_device(e->d_tiles, tiles, "tile list"));
  TRY(to_device(e->d_tiles16, tiles16, "tile list"));
  e->h_tiles16 = tiles16;
  TRY(to_device(e->d_tiles64, tiles64, "tile list"));
  TRY(to_device(e->d_pairs, pairs, "pair list"));
  TRY(to_device(e->d_jobs, jobs, "job list"));
  return NGD_OK;
}

// ---- resident images (zero-filled: padding individuals/sites contribute nothing) ----
static int create_images(ngd_engine *e) {
  const ngd_config *cfg = &e->cfg;
  const ngd_geom &g = e->g;
  const int kernel = e->kernel;
  const uint64_t n_pairs = ngd_n_pairs(g.n_ind);
  // + NGD_KG_TAIL zeroed k-groups: the MFMA kernel's operand pipeline runs ahead of its slice
  const uint64_t frag_elems = (g.n_kg + NGD_KG_TAIL) * (uint64_t)g.n_ig * 64;
  if (kernel == NGD_KERNEL_STREAM) {
    TRY(dev_alloc_pieces(e, e->PI, g.n_ind * g.n_sites_pad * 3, true));  // (a row of sites per individual: a load needs all of it)
  } else {
    TRY(dev_alloc_pieces(e, e->PA, frag_elems, true, PIECE_FRAG));
    e->single_image = kernel == NGD_KERNEL_MFMA && cfg->single_image == 1;
    if (kernel == NGD_KERNEL_MFMA && (cfg->single_image == 2 || cfg->single_image == 0)) {
      const bool ok = ngd_score_congruence(cfg->score, e->sc.c, e->sc.d) == NGD_OK;
      if (!ok && cfg->single_image == 2)
        return fail(NGD_E_INVALID, "ngd_create: single_image = 2 needs a symmetric score matrix (single_image = 1 takes any)");
      if (ok) {
        // the reference's two matrices (parse_args.cpp:25-27, :134-137): t = (p0 + p1 + p2, +-(p2 - p0), p1) -- the third
        // square of --avg_nuc_dist has weight 0 and an empty row, which then carries p1 all the same -- is the form the
        // fix-up pass recovers p from (fixup.hip)
        double *c = e->sc.c;
        if (e->sc.d[2] == 0 && c[6] == 0 && c[7] == 0 && c[8] == 0) c[7] = 1.0;
        const bool form = c[0] == 1 && c[1] == 1 && c[2] == 1 && c[4] == 0 && (c[3] == 1 || c[3] == -1) && c[5] == -c[3] &&
                          c[6] == 0 && c[7] == 1 && c[8] == 0;
        e->sc.fix = form ? 1 : 0;
        e->sc.fix_sign = c[5];
      }
      // auto: one image in congruent coordinates where it is safe (the fix-up pass exists for this matrix) and where memory
      // matters -- the block forms of a few hundred individuals take no per-index weights in their fastest variant
      e->congruent = ok && (cfg->single_image == 2 || (e->sc.fix && e->exact_shapes == 0));
      e->sc.congruent = e->congruent ? 1 : 0;
      if (!e->congruent) e->sc.fix = 0;
    }
    if (e->single_image) {  // ... and as much of the second image as the caller has memory to spare for
      e->qb_res_kg = std::min<uint64_t>(g.n_kg, ((uint64_t)cfg->second_image_mib << 20) / ((uint64_t)g.n_ig * 64 * 8));
      if (e->qb_res_kg == g.n_kg) { e->single_image = false; e->qb_res_kg = 0; }  // all of it: the two-image engine
    }
    if (kernel == NGD_KERNEL_MFMA && !e->single_image && !e->congruent) TRY(dev_alloc_pieces(e, e->QB, frag_elems, true, PIECE_FRAG));
    if (e->qb_res_kg) TRY(e->QB_res.alloc(e, (e->qb_res_kg + NGD_KG_TAIL) * (uint64_t)g.n_ig * 64, false));
  }
  if (cfg->pairwise_del) {
    TRY(e->mask.alloc(e, g.n_ind * (uint64_t)g.n_words, true));
    TRY(e->planes.alloc(e, 32ull * g.n_words, true));
  }
  TRY(e->d_ws.alloc(e, g.n_sites_pad + 4 * NGD_KG_TAIL, true));
  if (kernel == NGD_KERNEL_MFMA) TRY(e->d_wk.alloc(e, 4 * (g.n_kg + NGD_KG_TAIL), true));
  if (e->congruent) {
    TRY(e->d_wD.alloc(e, 4 * (g.n_kg + NGD_KG_TAIL), false));
    ngd_launch_index_weights(e->st, 4 * (g.n_kg + NGD_KG_TAIL), e->sc.d, e->d_wD);
  }
  if (e->congruent && e->sc.fix && !cfg->pairwise_del && g.n_kg < (1ull << 32)) {
    // the k-groups a plain pass walks when it leaves the unit-sum coordinate out (ngd_engine.h): all but every third,
    // padded as ngd_launch_kg_compact pads a list -- entries that point at the first zeroed tail k-group
    std::vector<uint32_t> list;
    list.reserve(g.n_kg / 3 * 2 + NGD_KG_LIST_PAD);
    for (uint64_t kg = 0; kg < g.n_kg; kg++)
      if (kg % 3) list.push_back((uint32_t)kg);
    e->n_kgskip = list.size();
    list.insert(list.end(), NGD_KG_LIST_PAD, (uint32_t)g.n_kg);
    TRY(e->d_kgskip.alloc(e, list.size(), false));
    if (hipMemcpy(e->d_kgskip, list.data(), list.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
      return fail(NGD_E_HIP, "ngd_create: k-group list upload failed");
    TRY(e->d_unitE.alloc(e, g.n_ind + 1, true));
  }
  if (e->congruent && e->sc.fix) {
    TRY(dev_alloc_pieces(e, e->SM, g.n_sites * g.n_ind, true, PIECE_SITE_MAJOR, g.n_ind * 8));
    e->fix_cap = (uint32_t)std::min<uint64_t>(n_pairs, NGD_FIX_LIST);
    TRY(e->d_fixlist.alloc(e, e->fix_cap, false));
    TRY(e->d_fixcount.alloc(e, 1, true));
    TRY(e->d_fixseen.alloc(e, n_pairs / 32 + 1, true));
    TRY(e->d_fixparts.alloc(e, NGD_FIX_CAP, false));
    if (e->h_fixcount.alloc(1))
      return fail(NGD_E_NOMEM, "ngd_create: no pinned host memory for the fix-up count");
    *e->h_fixcount = 0;
  }
  TRY(e->d_sum.alloc(e, n_pairs, true));
  TRY(e->d_cnt.alloc(e, n_pairs, true));
  return NGD_OK;
}

// ---- split over the site axis: slices -> slabs, reduced in fixed order ----
// Pair slots of the spilled-terms plan (em_spill_impl): a row of a tile takes one slot group per group of 16 columns that
// holds a pair -- none for a diagonal tile's lower triangle or for the columns at and beyond n_ind.  tiles64: the engine's
// owned 64 x 64 tiles, in the order of d_tiles64.  (ngd_create for a table-driven engine; em_exact_set for one it moves there)
int spill_slot_map(ngd_engine *e, const std::vector<ngd_tile> &tiles64) {
  const ngd_geom &g = e->g;
  std::vector<uint32_t> rowpg((size_t)tiles64.size() * 64, 0xffffffffu);
  uint64_t n_live = 0;
  for (size_t t = 0; t < tiles64.size(); t++)
    for (uint32_t row = 0; row < 64; row++) {
      const uint64_t i = (uint64_t)tiles64[t].ti * 64 + row, j0 = (uint64_t)tiles64[t].tj * 64;
      if (i >= g.n_ind || j0 >= g.n_ind) continue;
      const uint64_t first = tiles64[t].ti == tiles64[t].tj ? row + 1 : 0, last = std::min<uint64_t>(63, g.n_ind - 1 - j0);
      if (first > last) continue;
      rowpg[t * 64 + row] = (uint32_t)n_live - (uint32_t)(first >> 4);  // (+ a column group's index = its slot group)
      n_live += (last >> 4) - (first >> 4) + 1;
    }
  if (n_live + 4 < (1ull << 31)) {  // (else: the plan is not offered, em_spill_impl)
    e->n_pg_live = (uint32_t)n_live;
    e->n_pg_spill = (uint32_t)((n_live + 3) / 4 * 4);  // a wavefront of the contraction takes 2 or 4 slot groups
    TRY(e->d_rowpg.alloc(e, rowpg.size(), false));
    if (!rowpg.empty() && hipMemcpy(e->d_rowpg, rowpg.data(), rowpg.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
      return fail(NGD_E_HIP, "spill_slot_map: slot map upload failed");
  }
  return NGD_OK;
}

static int create_slices(ngd_engine *e, const std::vector<ngd_tile> &tiles64) {
  const ngd_config *cfg = &e->cfg;
  const ngd_geom &g = e->g;
  const int kernel = e->kernel, dev = e->device;
  if (kernel == NGD_KERNEL_MFMA) {
    uint64_t want = cfg->wg_target ? cfg->wg_target : 8192;
    const uint32_t wg_per_slice = std::max(1u, e->n_wg);
    uint64_t ks = (want * (e->exact_shapes && e->exact_shapes < 3 ? 4 : 1) + wg_per_slice - 1) / wg_per_slice;  // EXACT: 1-wave workgroups
    uint64_t max_ks = std::max<uint64_t>(8, g.n_kg / 128);  // at least 128 k-groups per slice
    ks = std::min(ks, max_ks);
    ks = std::max<uint64_t>(8, (ks + 7) / 8 * 8);
    {
      // Workgroups all last the same, so an XCD works through its share (n_wg * ks / 8 workgroups) in rounds of
      // as many as it holds at a time, and a last round that is nearly empty costs as much as a full one
      // ([measured] cfg 3, 34 workgroups per slice: ks = 232 -> 10.27 rounds, 47.5 ms; 240 -> 10.63, 46.1 ms;
      // 248 -> 10.98, 44.65 ms; cfg 2, 10 single-wavefront jobs per slice: 584 -> 1.90 rounds, 448 -> 1.46 rounds,
      // 0.41 ms, 304 -> 0.99 rounds, 0.345 ms and half the slabs to reduce).  Among the slice counts from half the
      // target to 15 % above it take the one whose last round is fullest.
      hipDeviceProp_t prop;
      const uint32_t cus_per_xcd = hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount >= 8
                                       ? (uint32_t)prop.multiProcessorCount / 8 : 32;
      // (in-step forms: whole workgroups of wg_waves jobs + the prefetching wavefront, 20 / 12 wavefronts to a CU)
      const uint32_t sync_wgs = e->exact_shapes >= 3
                                    ? std::max(1u, (e->exact_shapes >= 4 ? 20u : 12u) / std::min(16u, e->wg_waves + 1)) : 0;
      const double slots = (double)cus_per_xcd * (e->exact_shapes >= 3 ? sync_wgs : e->exact_shapes == 2 ? 24 : e->exact_shapes ? 12 : 3);
      // ... plus what the slice count costs afterwards: the slab reduction reads one plane per slice ([measured] 0.8 us
      // per slice at n_ind = 1000, i.e. ~5 TB/s), against an accumulation pass at ~0.8 of the FP64 peak.  It decides
      // between slice counts that fill their rounds equally well: a 1/8 site shard of cfg 3 takes 112 slices instead
      // of 248 (6.36 instead of 6.54 ms per matrix, the accumulation itself is flat from 88 to 500 slices).
      const double accum_s = 6.0 * (double)e->n_owned_pairs * (double)g.n_sites / (0.8 * 78.6e12);
      const double reduce_s_per_slice = 8.0 * (double)e->n_owned_pairs / 5e12;
      // A single-image engine walks the pass in ranges (accumulate_single_image()): every launch has all the slices, and every
      // block adds to its plane of the slab at the end of each ([measured] cfg 3, 248 slices, 12 ranges: +0.53 ms per
      // launch, 2.1 us per slice -- 2.7 reductions' worth).  Fewer slices then: as few as fill their rounds.
      const uint64_t qb_ranges =
          e->single_image ? (g.n_kg - e->qb_res_kg + single_image_span(g) - 1) / single_image_span(g) + (e->qb_res_kg ? 1 : 0) : 0;
      const double per_slice_s = reduce_s_per_slice * (1.0 + 2.7 * (double)qb_ranges);
      double best = 1e30;
      uint64_t best_ks = ks;
      for (uint64_t c = e->single_image ? 8 : std::max<uint64_t>(8, ks / 3 / 8 * 8); c <= std::min(max_ks, ks * 115 / 100); c += 8) {
        const double rounds = (double)wg_per_slice * (double)(c / 8) / slots;
        const double waste = std::ceil(rounds - 1e-9) / rounds + (double)c * per_slice_s / std::max(accum_s, 1e-9);
        if (waste < best) { best = waste; best_ks = c; }
      }
      ks = best_ks;
    }
    if (cfg->n_slices) ks = std::min<uint64_t>(cfg->n_slices, max_ks);  // a caller's count is held to the same bound
    ks = std::max<uint64_t>(8, (ks + 7) / 8 * 8);
    e->n_ks = (uint32_t)ks;
    e->per_slice = ((g.n_kg + ks - 1) / ks + 3) / 4 * 4;  // whole pipeline trips (accum_mfma.hip DEPTH)
    // (the pass over the list of ngd_engine.h: the same slices -- a slice count fills its dispatch rounds as well or as
    // badly whatever the slices' length -- of equal shares of the list)
    e->skip_per_slice = ((e->n_kgskip + ks - 1) / ks + 3) / 4 * 4;
    TRY(dev_alloc_pieces(e, e->slab, ks * (uint64_t)g.n_pad * g.n_pad, false));
    // ([0..1] the clock sample; [2] set by a block whose shape the kernel does not list: mfma_fault())
    if (e->h_clk.alloc(4, hipHostMallocMapped) || hipHostGetDevicePointer((void **)&e->d_clk, e->h_clk, 0) != hipSuccess)
      return fail(NGD_E_NOMEM, "ngd_create: no pinned host memory for the clock sample");
    e->h_clk[0] = e->h_clk[1] = e->h_clk[2] = e->h_clk[3] = 0;
    if (e->single_image) {
      // scratch for QB: one range of a whole pass (accumulate_single_image(); partial-sum passes grow it if a bootstrap
      // block is longer)
      e->qb_chunk_kg = single_image_span(g);
      uint64_t n_ranges = 0;
      const uint64_t rest_kg = g.n_kg - e->qb_res_kg;  // (what is not resident: ngd_config.second_image_mib)
      const uint64_t range_kg = std::min<uint64_t>(rest_kg, qb_piece(rest_kg, e->n_ks, e->qb_chunk_kg, &n_ranges) * e->n_ks);
      TRY(e->qb_chunk.alloc(e, (range_kg + NGD_KG_TAIL) * (uint64_t)g.n_ig * 64, false));
    }
  } else if (kernel == NGD_KERNEL_EM_TABLE) {
    // 64 x 64 tiles x slices of sites; a workgroup works a site in ~10 us, so slices of a few thousand sites keep
    // the tail of the launch short without making the slab large
    e->em_shape = (int)cfg->variant;
    uint64_t want = cfg->wg_target ? cfg->wg_target : 16384;
    uint64_t ks = e->n_tiles64 ? (want + e->n_tiles64 - 1) / e->n_tiles64 : 1;
    uint64_t max_ks = std::max<uint64_t>(1, g.n_sites / 64);
    ks = std::min(ks, max_ks);
    if (cfg->n_slices) ks = std::min<uint64_t>(cfg->n_slices, g.n_sites);  // never more slices than sites
    e->n_ks = (uint32_t)ks;
    e->per_slice = (g.n_sites + ks - 1) / ks;
    TRY(dev_alloc_pieces(e, e->slab, ks * (uint64_t)g.n_pad * g.n_pad, true));
    TRY(e->d_emcnt.alloc(e, 4, true));
    TRY(spill_slot_map(e, tiles64));
  } else if (kernel == NGD_KERNEL_EM_FAST || kernel == NGD_KERNEL_EM_FAITHFUL) {
    uint64_t want = cfg->wg_target ? cfg->wg_target : 4096;
    uint64_t ks = e->n_tiles16 ? (want + e->n_tiles16 - 1) / e->n_tiles16 : 1;
    uint64_t max_ks = std::max<uint64_t>(1, g.n_sites / 256);
    ks = std::min(ks, max_ks);
    if (cfg->n_slices) ks = std::min<uint64_t>(cfg->n_slices, g.n_sites);  // never more slices than sites
    e->n_ks = (uint32_t)ks;
    e->per_slice = (g.n_sites + ks - 1) / ks;
    TRY(dev_alloc_pieces(e, e->slab, ks * (uint64_t)g.n_pad * g.n_pad, false));
  }
  return NGD_OK;
}
#undef TRY

int ngd_create(const ngd_config *cfg, ngd_engine **out) {
  if (!cfg || !out) return fail(NGD_E_INVALID, "ngd_create: null argument");
  *out = nullptr;
  const uint32_t world = cfg->shard_world ? cfg->shard_world : 1;
  int dev = 0, kernel = 0;
  if (int rc = create_check(cfg, world)) return rc;
  if (int rc = create_device(cfg, dev, kernel)) return rc;
  if (int rc = create_fits(cfg, kernel)) return rc;
  std::unique_ptr<ngd_engine, create_bail> made(new (std::nothrow) ngd_engine());
  ngd_engine *e = made.get();
  if (!e) return fail(NGD_E_NOMEM, "ngd_create: host allocation failed");
  if (int rc = create_geometry(e, cfg, world, dev, kernel)) return rc;
  std::vector<ngd_tile> tiles, tiles16, tiles64;
  std::vector<uint64_t> pairs;
  std::vector<ngd_job> jobs;
  const std::vector<uint32_t> owner = ngd_tile_owners(e->g.n_t, world);
  create_shard(e, owner, tiles, tiles16, tiles64);
  if (int rc = create_jobs(e, owner, tiles, jobs)) return rc;
  create_owned_pairs(e, tiles, pairs);
  if (int rc = create_lists_to_device(e, tiles, tiles16, tiles64, pairs, jobs)) return rc;
  if (int rc = create_images(e)) return rc;
  if (int rc = create_slices(e, tiles64)) return rc;
  // upload staging (ngd_upload_sites / _ind_major): at most ~256 MiB of raw doubles, allocated by the first upload that
  // needs it (a staged load -- ngd_stage_* -- never does)
  e->staging_sites = std::max<uint64_t>(1, std::min<uint64_t>(e->g.n_sites, (256ull << 20) / (e->g.n_ind * 24)));
  if (hipStreamSynchronize(e->st) != hipSuccess) return fail(NGD_E_HIP, "ngd_create: sync failed");
  if (int prc = piece_start(e)) return prc;  // the images' and slabs' memory arrives behind this call (dev_alloc_pieces)
  *out = made.release();
  return NGD_OK;
}
