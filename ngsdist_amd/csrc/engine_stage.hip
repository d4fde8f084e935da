// engine_stage.hip -- a data set on its way in: the uploads, the staging ring of a raw load and the full-data pass that
// may start beside it, ngd_commit, the synthetic fill.
#include "ngd_engine.h"

static int upload_common(ngd_engine *e, const double *p, int ind_major, uint64_t s0, uint64_t n) {
  if (!e || !p) return fail(NGD_E_INVALID, "upload: null argument");
  if (e->committed) return fail(NGD_E_INVALID, "upload: data set already committed");
  if (s0 + n > e->g.n_sites || s0 + n < s0) return fail(NGD_E_INVALID, "upload: site range out of bounds");
  HIPCHK(hipSetDevice(e->device));
  if (int rc = piece_join(e)) return rc;
  if (int rc = eager_discard(e)) return rc;  // (sites may be uploaded again: nothing accumulated beside a staged load is kept)
  e->stage_in_order = false;
  if (!e->staging)
    if (int rc = e->staging.alloc(e, e->staging_sites * e->g.n_ind * 3, false)) return rc;
  const uint64_t n_ind = e->g.n_ind;
  for (uint64_t done = 0; done < n;) {
    const uint64_t c = std::min(e->staging_sites, n - done);
    if (ind_major) {
      // rows = individuals, each row = c sites x 24 B out of an n_sites-long row
      HIPCHK(hipMemcpy2DAsync(e->staging, c * 24, p + (s0 + done) * 3, e->g.n_sites * 24, c * 24, n_ind,
                              hipMemcpyHostToDevice, e->st));
    } else {
      HIPCHK(hipMemcpyAsync(e->staging, p + done * n_ind * 3, c * n_ind * 24, hipMemcpyHostToDevice, e->st));
    }
    ngd_launch_layout(e->st, e->g, e->staging, ind_major, s0 + done, c, e->sc, e->cfg.pairwise_del, e->PA,
                      e->QB, e->congruent ? e->SM : e->PI, e->mask);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->st));  // staging buffer is reused by the next chunk
    done += c;
  }
  return NGD_OK;
}

int ngd_upload_sites(ngd_engine *e, const double *p, uint64_t s0, uint64_t n) {
  return upload_common(e, p, 0, s0, n);
}

int ngd_upload_ind_major(ngd_engine *e, const double *p) {
  if (!e) return fail(NGD_E_INVALID, "upload: null engine");
  return upload_common(e, p, 1, 0, e->g.n_sites);
}

// [measured, round 6] `tools/host_read_pipeline`: pieces of 32-64 MiB through a ring of 4-8 pinned buffers keep the copy
// engine at the link's rate (56.9 of 57.6 GB/s) while the caller fills the next ones; one piece costs 0.6-1.1 ms of copy,
// far above a launch.  Pinned memory is allocated at ~6.5 GiB/s, so the ring is kept to 192 MiB.
// A slot is allocated when the ring first comes to it: the copy engine is then already busy with the slots before it
// (6 x (hipHostMalloc + hipMalloc) up front were 40-50 ms before the first byte moved).
void stage_reap(ngd_engine *e) {
  if (e->ring_reaper.joinable()) e->ring_reaper.join();
}

// ---- the full-data pass beside a staged load (NGD_OPT_EAGER_FULL) ----
bool eager_supported(const ngd_engine *e) {
  if (e->kernel == NGD_KERNEL_EM_TABLE) return e->n_ks > 1;
  return e->kernel == NGD_KERNEL_MFMA && e->exact_shapes == 0 && !e->single_image && e->n_ks >= 16;
}

// slices [ks0, ks0 + n) of the plain pass on `st` (results: their planes of e->slab, as a whole launch leaves them)
void launch_plain_slices(ngd_engine *e, hipStream_t st, uint32_t ks0, uint32_t n, bool beside_a_load, bool unit_skip) {
  const ngd_geom &g = e->g;
  if (e->kernel == NGD_KERNEL_EM_TABLE) {
    // beside a load ONE workgroup per CU (12 KB more LDS than its tables need): the chip is not full of workgroups that
    // last tens of milliseconds when the next piece's preparation kernel wants wave slots and registers
    ngd_launch_accum_em_table_slices(st, emt_common(e), ks0, n, e->per_slice, e->slab, beside_a_load ? 12u << 10 : 0u);
  } else {
    ngd_mfma_launch l;
    l.PA = e->PA; l.QB = e->congruent ? e->PA : e->QB;
    l.d_wk = e->congruent ? e->d_wD : nullptr;
    l.ks0 = ks0; l.n_ks = n; l.kg_per_slice = e->per_slice; l.n_kg_eff = g.n_kg;
    if (unit_skip) { l.d_kgl = e->d_kgskip; l.kg_per_slice = e->skip_per_slice; l.n_kg_eff = e->n_kgskip; }  // (pass_once)
    l.slab = e->slab;
    ngd_launch_accum_mfma(st, mfma_engine(e), l);
  }
}

// which plain pass the slices started beside a load belong to: the one ngd_run() will want if the data set turns out *unit*
// (every data set a staged load prepares is: K0 normalises)
static bool eager_unit_skip(const ngd_engine *e) {
  if (e->eager_slices) return e->eager_skip;
  return e->d_kgskip && e->opt_unit_skip;
}

// after the piece of sites [s0, s0 + n) has been submitted (its preparation kernel is on e->st, k0_done[b] recorded)
static int eager_advance(ngd_engine *e, uint64_t s0, uint64_t n, int b) {
  if (!e->opt_eager || !e->stage_in_order) return NGD_OK;
  if (s0 != e->stage_prefix) { e->stage_in_order = false; return NGD_OK; }  // (out of order: what is launched stays valid)
  e->stage_prefix = s0 + n;
  const ngd_geom &g = e->g;
  if (e->stage_prefix >= g.n_sites) return NGD_OK;  // the last piece: ngd_run() launches what is left
  uint32_t done;
  if (e->kernel == NGD_KERNEL_EM_TABLE) {
    done = (uint32_t)std::min<uint64_t>(e->n_ks, e->stage_prefix / e->per_slice);
  } else {
    // a slice's k-groups + the NGD_KG_TAIL groups its operand pipeline runs ahead: every index of theirs belongs to a site
    // below the prefix (ngd_layout.h: whole periods of four sites in the congruent image)
    uint64_t kg_ready = ngd_kg_whole(e->stage_prefix, e->congruent), per_slice = e->per_slice;
    // the pass that leaves the unit-sum coordinate out walks a list: entry 2 q + r is k-group 3 q + 1 + r, so the list's
    // first 2 kg_ready / 3 entries are the listed k-groups below kg_ready (a multiple of 3 in the congruent image)
    if (eager_unit_skip(e)) { kg_ready = kg_ready / 3 * 2; per_slice = e->skip_per_slice; }
    const uint64_t full = kg_ready > NGD_KG_TAIL ? (kg_ready - NGD_KG_TAIL) / per_slice : 0;
    done = (uint32_t)std::min<uint64_t>(e->n_ks, full) / 8 * 8;  // (launches of whole eights of slices: the XCD deal)
  }
  const uint32_t batch = e->kernel == NGD_KERNEL_EM_TABLE ? std::max(1u, e->n_ks / 32) : std::max(8u, e->n_ks / 8 / 8 * 8);
  if (done < e->eager_slices + batch) return NGD_OK;
  // ONE batch in flight at a time, and a bounded one: what is launched here runs beside the load at a reduced rate (the
  // table-driven EM kernel with one workgroup per CU: 0.56 of its speed) and must not still be running long after it
  // ([measured] every completed slice launched at once: cfg 4's matrix 4.0 s instead of 2.26)
  if (e->eager_valid) {
    const hipError_t q = hipEventQuery(e->ev_eager);
    if (q == hipErrorNotReady) { (void)hipGetLastError(); return NGD_OK; }
    HIPCHK(q);
  }
  done = std::min(done, e->eager_slices + (e->kernel == NGD_KERNEL_EM_TABLE ? batch : 2 * batch));
  {  // the slab's planes of these slices must be mapped (its memory arrives after the images': dev_alloc_pieces)
    std::lock_guard<std::mutex> lk(e->piece_mu);
    for (auto &q : e->piece_ranges)
      if (q.get() == e->slab.range() && q->ready < std::min<size_t>(q->size, (size_t)done * g.n_pad * g.n_pad * 8)) return NGD_OK;  // (next piece)
  }
  if (!e->st_eager) {
    // (a stream confined to a part of the CUs -- hipExtStreamCreateWithCUMask, 7/8 or 3/4 of them -- lets the EM kernel keep
    // two workgroups per CU there and does more beside the load, but the preparation kernels then wait for the few CUs
    // left: [measured] cfg 4 end to end 2.78-2.83 and 2.89-2.92 s against 2.77-2.80 with the plain low-priority stream)
    int least = 0, greatest = 0;
    HIPCHK(hipDeviceGetStreamPriorityRange(&least, &greatest));
    HIPCHK(hipStreamCreateWithPriority(&e->st_eager, hipStreamNonBlocking, least));
    HIPCHK(hipEventCreateWithFlags(&e->ev_eager, hipEventDisableTiming));
  }
  HIPCHK(hipStreamWaitEvent(e->st_eager, e->ring[b].k0_done, 0));  // this piece's preparation -- and every earlier one's -- is done
  if (!e->eager_slices) e->eager_skip = eager_unit_skip(e);  // (one kind of slices per load)
  launch_plain_slices(e, e->st_eager, e->eager_slices, done - e->eager_slices, true, e->eager_skip);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(e->ev_eager, e->st_eager));
  e->eager_slices = done;
  e->eager_valid = true;
  return NGD_OK;
}

// anything but the plain pass is about to use the slab (or the engine is going away): what was started is waited for and dropped
int eager_discard(ngd_engine *e) {
  if (e->eager_valid) HIPCHK(hipStreamSynchronize(e->st_eager));
  e->eager_valid = false;
  e->eager_slices = 0;
  return NGD_OK;
}

// A pinned buffer of the ring comes from hipHostMalloc (which allocates, zeroes and pins 4-KB pages at ~6.5 GiB/s: 5 ms per
// 32-MiB slot, ~25 ms before the ring has turned once).  Round 6 tried huge-page host memory registered with the runtime
// (posix_memalign + MADV_HUGEPAGE + hipHostRegister: the copies first to last byte 0.468 -> 0.440 s) and took it out again:
// in a process that created and destroyed engine after engine (tools/fuzz_large.py, case ~55 of 80) the GPU faulted on a HOST
// heap address -- registered ranges are handed back to malloc and come round again at the same addresses, and a
// registration that is released late takes the next one's mapping with it.  hipHostMalloc's buffers never share addresses.
static int pin_alloc(ngd_engine *e, int b, uint64_t bytes) { return e->ring[b].pin.alloc(bytes / 8); }

// every slot's device twin and events at once (cheap); pinned buffer 0 at once, the others by ring_maker
static int stage_slots(ngd_engine *e) {
  const uint64_t bytes = e->pin_sites * e->g.n_ind * 24;
  for (int b = 0; b < e->ring_slots; b++) {
    int rc = e->ring[b].draw.alloc(e, bytes / 8, false);
    if (rc) return rc;
    HIPCHK(hipEventCreateWithFlags(&e->ring[b].pin_free, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&e->ring[b].k0_done, hipEventDisableTiming));
  }
  if (int rc = pin_alloc(e, 0, bytes)) return rc;
  e->ring_ready = 1;
  e->ring_stop = false;
  e->ring_maker_rc = 0;
  if (e->ring_slots > 1) {
    const int dev = e->device, n = e->ring_slots;
    e->ring_maker = std::thread([e, dev, n, bytes]() {
      if (hipSetDevice(dev) != hipSuccess) { e->ring_maker_rc = NGD_E_HIP; return; }
      for (int b = 1; b < n && !e->ring_stop.load(std::memory_order_relaxed); b++) {
        if (pin_alloc(e, b, bytes)) {  // (the load goes on with the buffers it has)
          e->ring_maker_rc = NGD_E_NOMEM;
          return;
        }
        e->ring_ready.store(b + 1, std::memory_order_release);
      }
    });
  }
  return NGD_OK;
}

static int stage_init(ngd_engine *e) {
  if (e->pin_sites) return NGD_OK;
  stage_reap(e);
  e->pin_sites = std::max<uint64_t>(1, std::min<uint64_t>(e->g.n_sites, (e->opt_stage_piece_mib << 20) / (e->g.n_ind * 24)));
  // (a data set of fewer pieces than the ring has slots takes only that many)
  e->ring_slots = (int)std::min<uint64_t>(e->opt_stage_ring, (e->g.n_sites + e->pin_sites - 1) / e->pin_sites);
  // ONE copy stream ([measured] copies alternating two streams load cfg 3 in the same 0.53 s, and a stream costs 7 ms to create)
  if (!e->st_copy[0]) HIPCHK(hipStreamCreateWithFlags(&e->st_copy[0], hipStreamNonBlocking));
  e->n_staged = 0;
  e->pin_cur = 0;
  if (!e->d_nan)
    if (int rc = e->d_nan.alloc(e, 1, true)) return rc;
  return stage_slots(e);
}

void ring_maker_join(ngd_engine *e) {
  e->ring_stop = true;
  if (e->ring_maker.joinable()) e->ring_maker.join();
}

int ngd_stage_acquire(ngd_engine *e, double **host_buf, uint64_t *capacity_sites) {
  if (!e || !host_buf || !capacity_sites) return fail(NGD_E_INVALID, "ngd_stage_acquire: null argument");
  if (e->committed) return fail(NGD_E_INVALID, "ngd_stage_acquire: data set already committed");
  HIPCHK(hipSetDevice(e->device));
  int rc = stage_init(e);
  if (rc) return rc;
  const int b = e->pin_cur;
  // the copy out of this buffer, a turn of the ring ago, is done -- and so is the preparation kernel that read its device
  // twin (it follows the copy on the engine's stream, ~30 us): waited for HERE, on the host, so that the copy stream carries
  // no wait of its own ([measured] a stream-side wait on an event costs the copy engine ~50 us of idling per copy)
  HIPCHK(hipEventSynchronize(e->ring[b].k0_done));
  e->pin_lent = b;
  *host_buf = e->ring[b].pin;
  *capacity_sites = e->pin_sites;
  return NGD_OK;
}

int ngd_stage_submit(ngd_engine *e, uint64_t s0, uint64_t n, const ngd_prep *prep) {
  if (!e || !prep) return fail(NGD_E_INVALID, "ngd_stage_submit: null argument");
  if (e->pin_lent < 0) return fail(NGD_E_INVALID, "ngd_stage_submit: no buffer acquired");
  if (prep->call_geno && prep->N_thresh > prep->call_thresh)  // call_geno(), gen_func.cpp:887-888
    return fail(NGD_E_INVALID, "missing data threshold must be smaller than calling genotype threshold!");
  if (n > e->pin_sites || s0 + n > e->g.n_sites || s0 + n < s0)
    return fail(NGD_E_INVALID, "ngd_stage_submit: site range out of bounds");
  HIPCHK(hipSetDevice(e->device));
  // a piece below the in-order prefix rewrites sites that launched eager slices have read -- or are reading still: its
  // preparation kernel would run beside them.  They are waited for and dropped, and none start again in this load.
  // (Checked even once the load is out of order: a piece that jumped ahead left the slices valid, this one does not.)
  if (e->eager_valid && s0 < e->stage_prefix) {
    if (int rc = eager_discard(e)) return rc;
    e->stage_in_order = false;
  }
  const int b = e->pin_lent;
  hipStream_t cs = e->st_copy[0];
  e->n_staged++;
  HIPCHK(hipMemcpyAsync(e->ring[b].draw, e->ring[b].pin, n * e->g.n_ind * 24, hipMemcpyHostToDevice, cs));
  HIPCHK(hipEventRecord(e->ring[b].pin_free, cs));
  HIPCHK(hipStreamWaitEvent(e->st, e->ring[b].pin_free, 0));
  if (int rc = piece_wait_sites(e, s0 + n)) return rc;  // (the part of the images these sites are written to is mapped)
  ngd_launch_prep_layout(e->st, e->g, e->ring[b].draw, s0, n, prep->in_logscale, prep->call_geno, prep->N_thresh,
                         prep->call_thresh, e->sc, e->cfg.pairwise_del, e->PA, e->QB, e->congruent ? e->SM : e->PI, e->mask,
                         e->d_nan);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(e->ring[b].k0_done, e->st));
  if (int rc = eager_advance(e, s0, n, b)) return rc;
  e->pin_lent = -1;
  e->pin_cur = (b + 1) % std::max(1, e->ring_ready.load(std::memory_order_acquire));  // (the buffers that exist by now)
  return NGD_OK;
}

int ngd_upload_raw_sites(ngd_engine *e, const double *raw, uint64_t s0, uint64_t n, const ngd_prep *prep) {
  if (!e || !raw || !prep) return fail(NGD_E_INVALID, "ngd_upload_raw_sites: null argument");
  for (uint64_t done = 0; done < n;) {
    double *buf;
    uint64_t cap;
    int rc = ngd_stage_acquire(e, &buf, &cap);
    if (rc) return rc;
    const uint64_t c = std::min(cap, n - done);
    memcpy(buf, raw + done * e->g.n_ind * 3, c * e->g.n_ind * 24);
    rc = ngd_stage_submit(e, s0 + done, c, prep);
    if (rc) return rc;
    done += c;
  }
  return NGD_OK;
}

// The data set is fixed from here on: what the plain pass needs to leave the unit-sum coordinate out (engine_plans.hip,
// NGD_OPT_UNIT_SKIP) is derived once, as part of the load -- E_i = SUM_s (t0_i(s) - 1) per individual, and the *unit* mark:
// every t0 finite and within 2^-40 of 1 (prepared, normalised input is; values a caller uploads need not be).  One pass
// over the t0 k-groups of the image, a third of it.
static int unit_scan(ngd_engine *e) {
  e->unit_ok = false;
  if (!e->d_unitE) return NGD_OK;
  HIPCHK(hipMemsetAsync(e->d_unitE, 0, (e->g.n_ind + 1) * sizeof(long long), e->st));  // (the last word: the mark's flag)
  int *d_flag = (int *)(e->d_unitE.get() + e->g.n_ind);
  ngd_launch_unit_scan(e->st, e->g, e->PA, e->d_unitE, d_flag);
  HIPCHK(hipGetLastError());
  int flag = 1;
  HIPCHK(hipMemcpyAsync(&flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, e->st));
  HIPCHK(hipStreamSynchronize(e->st));
  e->unit_ok = flag == 0;
  return NGD_OK;
}

int ngd_commit(ngd_engine *e) {
  if (!e) return fail(NGD_E_INVALID, "ngd_commit: null engine");
  HIPCHK(hipSetDevice(e->device));
  if (int rc = piece_join(e)) return rc;
  HIPCHK(hipStreamSynchronize(e->st));
  if (e->d_nan) {
    int flag = 0;
    HIPCHK(hipMemcpy(&flag, e->d_nan, sizeof(int), hipMemcpyDeviceToHost));
    ring_maker_join(e);
    {  // the pipeline is over: its slots go back on a thread of their own (6 x hipHostFree + hipFree are ~30 ms)
      std::vector<RingSlot> slots;
      for (RingSlot &slot : e->ring)
        if (slot.pin || slot.draw) {
          slot.draw.uncount();  // (HERE, not whenever the reaper comes to it)
          slots.push_back(std::move(slot));
        }
      e->pin_sites = 0;
      e->ring_slots = 0;
      e->ring_ready = 0;
      stage_reap(e);
      const int dev = e->device;
      if (!slots.empty())
        e->ring_reaper = std::thread([slots = std::move(slots), dev]() mutable {
          (void)hipSetDevice(dev);
          slots.clear();
        });
    }
    e->pin_cur = 0;
    e->pin_lent = -1;
    if (flag) {  // reported once: a caller that uploads again starts from a clean flag and a fresh pipeline
      HIPCHK(hipMemset(e->d_nan, 0, sizeof(int)));
      if (int rc = eager_discard(e)) return rc;  // (slices of the rejected data: none of them is kept)
      e->stage_prefix = 0;
      e->stage_in_order = true;
      return fail(NGD_E_NAN, "NaN found! Is the file format correct?");
    }
  }
  if (e->staging) {  // upload is over: give the staging buffer back
    if (int rc = e->staging.release()) return rc;
  }
  if (e->QB_res)  // single-image engine: the part of the second image it keeps (stream order: before any pass)
    ngd_launch_qb_range(e->st, e->g, e->sc, e->PA, 0, std::min<uint64_t>(e->qb_res_kg + NGD_KG_TAIL, e->g.n_kg + NGD_KG_TAIL),
                        e->QB_res);
  if (int rc = unit_scan(e)) return rc;
  e->committed = true;
  return NGD_OK;
}

int ngd_synth_fill_range(ngd_engine *e, uint64_t seed, double miss_frac, uint64_t site0) {
  if (!e) return fail(NGD_E_INVALID, "ngd_synth_fill: null engine");
  if (e->committed) return fail(NGD_E_INVALID, "ngd_synth_fill: data set already committed");
  HIPCHK(hipSetDevice(e->device));
  if (int rc = piece_join(e)) return rc;
  ngd_launch_synth(e->st, e->g, seed, miss_frac, site0, e->sc, e->cfg.pairwise_del, e->PA, e->QB,
                   e->congruent ? e->SM : e->PI, e->mask);
  HIPCHK(hipGetLastError());
  return ngd_commit(e);
}

int ngd_synth_fill(ngd_engine *e, uint64_t seed, double miss_frac) { return ngd_synth_fill_range(e, seed, miss_frac, 0); }
