// engine_mem.hip -- the thread that maps, piece by piece, the address ranges dev_alloc_pieces reserved (ngd_engine.h), and
// what a load waits for.
#include "ngd_engine.h"

// The worker: always the piece of the range that is furthest behind (relative to its size), so that the images of a data
// set grow together along the site axis; ranges nothing writes during a load (PIECE_WHOLE: slabs) after them.
static void piece_worker(ngd_engine *e) {
  auto give_up = [&](const char *what, hipError_t err) {
    std::lock_guard<std::mutex> lk(e->piece_mu);
    e->piece_rc = err == hipErrorOutOfMemory ? NGD_E_NOMEM : NGD_E_HIP;
    e->piece_err = std::string("device memory, piece by piece: ") + what + ": " + hipGetErrorString(err);
    e->piece_done = true;
    e->piece_cv.notify_all();
  };
  hipError_t err = hipSetDevice(e->device);
  if (err != hipSuccess) return give_up("hipSetDevice", err);
  hipStream_t sa = nullptr;
  if ((err = hipStreamCreateWithFlags(&sa, hipStreamNonBlocking)) != hipSuccess) return give_up("hipStreamCreate", err);
  hipMemAllocationProp prop = {};
  prop.type = hipMemAllocationTypePinned;
  prop.location.type = hipMemLocationTypeDevice;
  prop.location.id = e->device;
  hipMemAccessDesc acc = {};
  acc.location = prop.location;
  acc.flags = hipMemAccessFlagsProtReadWrite;
  // test hook (NGD_ENABLE_TEST_HOOKS=1): the NGD_TEST_FAIL_PIECE-th piece "runs out of memory" -- the path a real failure takes
  long fail_at = -1, n_made = 0;
  if (const char *hook = getenv("NGD_ENABLE_TEST_HOOKS"))
    if (!strcmp(hook, "1"))
      if (const char *k = getenv("NGD_TEST_FAIL_PIECE")) fail_at = atol(k);
  for (;;) {
    PieceRange *r = nullptr;
    for (int whole = 0; whole < 2 && !r; whole++) {
      double best = 2.0;
      for (auto &q : e->piece_ranges) {
        if ((q->kind == PIECE_WHOLE) != (whole == 1) || q->n_mapped * kPiece >= q->size) continue;
        const double f = (double)(q->n_mapped * kPiece) / (double)q->size;
        if (f < best) { best = f; r = q.get(); }
      }
    }
    if (!r) break;
    const size_t off = r->n_mapped * kPiece, len = std::min(kPiece, r->size - off);
    hipMemGenericAllocationHandle_t h;
    if (fail_at >= 0 && n_made++ == fail_at) { hipStreamDestroy(sa); return give_up("hipMemCreate (test hook)", hipErrorOutOfMemory); }
    if ((err = hipMemCreate(&h, len, &prop, 0)) != hipSuccess) { hipStreamDestroy(sa); return give_up("hipMemCreate", err); }
    r->hs.push_back(h);
    if ((err = hipMemMap((char *)r->va + off, len, 0, h, 0)) != hipSuccess) { hipStreamDestroy(sa); return give_up("hipMemMap", err); }
    r->n_mapped++;
    if ((err = hipMemSetAccess((char *)r->va + off, len, &acc, 1)) != hipSuccess) { hipStreamDestroy(sa); return give_up("hipMemSetAccess", err); }
    if (r->zero) {
      if ((err = hipMemsetAsync((char *)r->va + off, 0, len, sa)) != hipSuccess || (err = hipStreamSynchronize(sa)) != hipSuccess) {
        hipStreamDestroy(sa);
        return give_up("zero fill", err);
      }
    }
    std::lock_guard<std::mutex> lk(e->piece_mu);
    r->ready = off + len;
    e->piece_cv.notify_all();
  }
  hipStreamDestroy(sa);
  std::lock_guard<std::mutex> lk(e->piece_mu);
  e->piece_done = true;
  e->piece_cv.notify_all();
}

// (a reserved address range costs nothing: what the ranges will take is checked against the device's free memory HERE, so
// that a data set that cannot fit is refused by ngd_create -- NGD_E_NOMEM -- and not by the first upload)
int piece_start(ngd_engine *e) {
  if (e->piece_ranges.empty()) return NGD_OK;
  size_t free_b = 0, total_b = 0, want = 0;
  for (auto &q : e->piece_ranges) want += q->size;
  if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && want > free_b)
    return fail(NGD_E_NOMEM, "ngd_create: the images and slabs of this data set exceed the device's free memory");
  e->piece_done = false;
  e->piece_thread = std::thread(piece_worker, e);
  return NGD_OK;
}

// every piece of every range is there (or the worker has failed: its error)
int piece_join(ngd_engine *e) {
  if (e->piece_thread.joinable()) e->piece_thread.join();
  if (e->piece_rc) return fail(e->piece_rc, e->piece_err.c_str());
  return NGD_OK;
}

// ... or only what the sites [0, s_end) of the data set reach in the ranges a load writes
int piece_wait_sites(ngd_engine *e, uint64_t s_end) {
  if (e->piece_ranges.empty()) return NGD_OK;
  std::unique_lock<std::mutex> lk(e->piece_mu);
  for (auto &q : e->piece_ranges) {
    size_t need = q->size;
    if (s_end < e->g.n_sites) {
      // (every k-group a site below s_end has an index in -- rounded outwards to whole periods of four sites, which bounds
      // both layouts of ngd_layout.h -- and one more)
      if (q->kind == PIECE_FRAG) need = std::min<size_t>(q->size, (ngd_kg_hi(s_end, 1) + 1) * (size_t)e->g.n_ig * 512);
      else if (q->kind == PIECE_SITE_MAJOR) need = std::min<size_t>(q->size, (size_t)(s_end * q->bytes_per_site));
      else if (q.get() == e->slab.range()) continue;  // (nothing of a load goes there)
    } else if (q.get() == e->slab.range()) {
      continue;
    }
    e->piece_cv.wait(lk, [&] { return q->ready >= need || e->piece_done; });
    if (q->ready < need && e->piece_rc) return fail(e->piece_rc, e->piece_err.c_str());  // (what IS mapped serves its sites)
  }
  return NGD_OK;
}
