// ngd_buffers.h -- the owning types of the engine's memory (ngd_engine.h): a device allocation (hipMalloc, or an address
// range whose physical pieces arrive behind ngd_create), a pinned host allocation, a slot of the staging ring.  Each frees
// itself; a device buffer also keeps the engine's ngd_device_bytes() figure, by its own size.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/ngsdist_amd.h"

#pragma GCC visibility push(hidden)

// ONE error state for the library's every unit (ngd_last_error(), engine.hip)
inline thread_local std::string g_err;

inline int fail(int code, const std::string &msg) {
  g_err = msg;
  return code;
}

// A failed HIP call also leaves its code behind as the thread's "last error"; it is reported HERE, once, and cleared, so
// that the hipGetLastError() after a later, unrelated kernel launch does not report it a second time (found by
// tests/test_gpu_abi_misuse.py: an engine too large for the device poisoned the next engine's first launch).
#define HIPCHK(call)                                                                       \
  do {                                                                                     \
    hipError_t _e = (call);                                                                \
    if (_e != hipSuccess) {                                                                \
      (void)hipGetLastError();                                                             \
      return fail(_e == hipErrorOutOfMemory ? NGD_E_NOMEM : NGD_E_HIP,                     \
                  std::string(#call) + ": " + hipGetErrorString(_e));                      \
    }                                                                                      \
  } while (0)

// Images and slabs of a GiB and more: an address range reserved at once, its physical memory created, mapped and
// zeroed 256 MiB at a time by a thread of the engine's own (dev_alloc_pieces, piece_worker) -- the staged load starts at
// once and waits, piece by piece, only for the part of an image it is about to write (piece_wait_sites).
inline constexpr size_t kPiece = (size_t)256 << 20;
enum PieceKind { PIECE_FRAG, PIECE_SITE_MAJOR, PIECE_WHOLE };  // how far into the range a site reaches
struct PieceRange {
  void *va = nullptr;
  size_t size = 0, ready = 0, n_mapped = 0;  // ready: bytes from the start that are mapped (and zeroed), under piece_mu
  bool zero = false;
  PieceKind kind = PIECE_WHOLE;
  uint64_t bytes_per_site = 0;  // PIECE_SITE_MAJOR
  std::vector<hipMemGenericAllocationHandle_t> hs;
};

// (the piece thread has been joined; an empty range asks nothing more of piece_worker or piece_wait_sites)
inline void release_pieces(PieceRange &r) {
  for (size_t c = 0; c < r.n_mapped; c++) (void)hipMemUnmap((char *)r.va + c * kPiece, std::min(kPiece, r.size - c * kPiece));
  for (auto &h : r.hs) (void)hipMemRelease(h);
  if (r.va) (void)hipMemAddressFree(r.va, r.size);
  r.hs.clear();
  r.va = nullptr;
  r.size = r.ready = r.n_mapped = 0;
}

// the part of ngd_engine its buffers see
struct ngd_mem {
  int device = 0;
  hipStream_t st = nullptr;
  uint64_t dev_bytes = 0;  // ngd_device_bytes(): kept by DevBuf alone
  std::vector<std::unique_ptr<PieceRange>> piece_ranges;
};

inline int dev_malloc(ngd_mem *m, void **out, uint64_t bytes) {
  // NGD_TRACE_ALLOC=1: what every allocation of 64 MiB and more costs (the driver clears memory other processes have used
  // as it hands it out: seconds for tens of GB on a device that has just been busy, DESIGN.md section 3 "K0")
  static const bool trace = getenv("NGD_TRACE_ALLOC") != nullptr;
  const auto t0 = std::chrono::steady_clock::now();
  void *p = nullptr;
  HIPCHK(hipMalloc(&p, bytes));
  *out = p;
  if (trace && bytes >= (64u << 20))
    fprintf(stderr, "> alloc: hipMalloc of %.2f GB took %.3f s\n", (double)bytes / 1e9,
            std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
  m->dev_bytes += bytes;
  return NGD_OK;
}

template <typename T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  DevBuf(DevBuf &&o) noexcept
      : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)), m_(std::exchange(o.m_, nullptr)),
        range_(std::exchange(o.range_, nullptr)) {}
  ~DevBuf() { (void)release(); }

  // `count` elements from hipMalloc (zero: filled on the engine's stream); an empty buffer if count is 0
  int alloc(ngd_mem *m, uint64_t count, bool zero) {
    if (int rc = release()) return rc;
    if (!count) return NGD_OK;
    if (int rc = dev_malloc(m, (void **)&p_, count * sizeof(T))) return rc;
    cap_ = count;
    m_ = m;
    if (zero) HIPCHK(hipMemsetAsync(p_, 0, bytes(), m->st));
    return NGD_OK;
  }
  // ... or the whole of a reserved address range of the engine's (dev_alloc_pieces)
  void adopt(ngd_mem *m, PieceRange *r, uint64_t count) {
    p_ = (T *)r->va;
    cap_ = count;
    m_ = m;
    range_ = r;
    m->dev_bytes += bytes();
  }
  // grow-only scratch: the old memory is freed first; on failure the buffer is empty
  int ensure(ngd_mem *m, uint64_t need) { return need <= cap_ ? NGD_OK : alloc(m, need, false); }
  int release() {
    if (!p_) return NGD_OK;
    if (range_) release_pieces(*range_);
    else HIPCHK(hipFree(p_));
    uncount();
    p_ = nullptr;
    cap_ = 0;
    range_ = nullptr;
    return NGD_OK;
  }
  // leaves the engine's figure now; the memory itself goes with the buffer, wherever it has been moved to (ngd_commit)
  void uncount() {
    if (m_) m_->dev_bytes -= bytes();
    m_ = nullptr;
  }
  T *get() const { return p_; }
  operator T *() const { return p_; }
  uint64_t capacity() const { return cap_; }
  uint64_t bytes() const { return cap_ * sizeof(T); }
  const PieceRange *range() const { return range_; }

 private:
  T *p_ = nullptr;
  uint64_t cap_ = 0;  // elements
  ngd_mem *m_ = nullptr;
  PieceRange *range_ = nullptr;  // (of m_->piece_ranges) the memory is that range, not a hipMalloc
};

// Pinned host memory (hipHostMalloc), the same shape
template <typename T>
class PinBuf {
 public:
  PinBuf() = default;
  PinBuf(const PinBuf &) = delete;
  PinBuf &operator=(const PinBuf &) = delete;
  PinBuf(PinBuf &&o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
  ~PinBuf() { (void)release(); }
  int alloc(uint64_t count, unsigned flags = hipHostMallocDefault) {
    if (int rc = release()) return rc;
    void *p = nullptr;
    HIPCHK(hipHostMalloc(&p, count * sizeof(T), flags));
    p_ = (T *)p;
    cap_ = count;
    return NGD_OK;
  }
  int ensure(uint64_t need) { return need <= cap_ ? NGD_OK : alloc(need); }
  int release() {
    if (p_) HIPCHK(hipHostFree(p_));
    p_ = nullptr;
    cap_ = 0;
    return NGD_OK;
  }
  T *get() const { return p_; }
  operator T *() const { return p_; }
  uint64_t capacity() const { return cap_; }
  uint64_t bytes() const { return cap_ * sizeof(T); }

 private:
  T *p_ = nullptr;
  uint64_t cap_ = 0;
};

// A slot of the staging ring: a pinned host buffer the caller fills, its device twin, and the two events of a turn
struct RingSlot {
  PinBuf<double> pin;
  DevBuf<double> draw;
  hipEvent_t pin_free = nullptr;  // the copy out of pin is done: the caller may fill it again
  hipEvent_t k0_done = nullptr;   // K0 has read draw: the next copy may overwrite it
  RingSlot() = default;
  RingSlot(RingSlot &&o) noexcept
      : pin(std::move(o.pin)), draw(std::move(o.draw)), pin_free(std::exchange(o.pin_free, nullptr)),
        k0_done(std::exchange(o.k0_done, nullptr)) {}
  ~RingSlot() {
    if (pin_free) (void)hipEventDestroy(pin_free);
    if (k0_done) (void)hipEventDestroy(k0_done);
  }
};

#pragma GCC visibility pop
