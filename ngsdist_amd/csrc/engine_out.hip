// engine_out.hip -- results on their way out: the streamer of the *_dist calls (chunks leave the device while later
// matrices are still being reduced, the host's threads finish each as it lands), the host-pointer forms, the job driver of
// the tails and what every call that finishes matrices refuses.
#include "ngd_engine.h"

// ---- a job's matrices leaving the device while later ones are still being reduced (ngd_run_job_dist) ----
bool out_trace() {
  static const bool on = getenv("NGD_TRACE_OUT") != nullptr;
  return on;
}
double out_now() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

static int out_event(ngd_engine *e, hipEvent_t *ev) {
  auto &o = e->out;
  if (o.n_used == o.pool.size()) {
    hipEvent_t v;
    HIPCHK(hipEventCreateWithFlags(&v, hipEventDisableTiming));
    o.pool.push_back(v);
  }
  *ev = o.pool[o.n_used++];
  return NGD_OK;
}

// The copies of matrices [queued, m_hi) of d_bsum (--pairwise_del: and d_bcnt) are queued behind whatever the engine's stream
// holds NOW (the first event of a call is the first gate: partials_impl waits for it before it wakes the host's threads):
// chunks of about 8 MiB with an event each, alternating between two copy streams (a chunk's set-up and its event then hide
// behind the other stream's transfer: 49 -> 55 GB/s at cfg 5), tapering towards the job's end -- a chunk is at most a quarter
// of what is left -- because what the host's threads still have to do once the last byte has landed is the last chunk's cells.
// ([measured, round 6] a kernel pushing the results into the pinned buffers 64 KiB at a time with a flag in host memory
// behind every piece -- no events, a smooth arrival -- was no faster, 50 GB/s, and slowed the reductions it ran beside.)
int out_queue(ngd_engine *e, uint32_t m_hi) {
  auto &o = e->out;
  if (!o.on || m_hi <= o.queued) return NGD_OK;
  const uint64_t n_pairs = ngd_n_pairs(e->g.n_ind);
  hipEvent_t gate;
  if (int rc = out_event(e, &gate)) return rc;
  HIPCHK(hipEventRecord(gate, e->st));
  HIPCHK(hipStreamWaitEvent(o.st, gate, 0));
  HIPCHK(hipStreamWaitEvent(o.st2, gate, 0));
  const uint32_t step = (uint32_t)std::min<uint64_t>(1u << 20, std::max<uint64_t>(1, (8ull << 20) / std::max<uint64_t>(1, n_pairs * 8)));
  for (uint32_t a = o.queued, b; a < m_hi; a = b) {
    b = std::min(m_hi, a + std::min(step, std::max(1u, (o.n_mat - a + 3) / 4)));
    hipStream_t st = (o.n_chunk_seq++ & 1) ? o.st2 : o.st;
    HIPCHK(hipMemcpyAsync(o.h_sum + (uint64_t)a * n_pairs, e->d_bsum + (uint64_t)a * n_pairs, (uint64_t)(b - a) * n_pairs * sizeof(double),
                          hipMemcpyDeviceToHost, st));
    if (o.pdel)
      HIPCHK(hipMemcpyAsync(o.h_cnt + (uint64_t)a * n_pairs, e->d_bcnt + (uint64_t)a * n_pairs, (uint64_t)(b - a) * n_pairs * sizeof(uint64_t),
                            hipMemcpyDeviceToHost, st));
    hipEvent_t ev;
    if (int rc = out_event(e, &ev)) return rc;
    HIPCHK(hipEventRecord(ev, st));
    o.chunks.emplace_back(ev, b);
  }
  o.queued = m_hi;
  return NGD_OK;
}

static void out_declare(ngd_engine *e, uint64_t cells) {
  auto &o = e->out;
  std::atomic_thread_fence(std::memory_order_release);
  o.landed = cells;
  if (out_trace()) fprintf(stderr, "[out] %.2f matrices landed +%.3f\n", (double)cells / (double)ngd_n_pairs(e->g.n_ind), out_now() - o.t0);
}

// Declares landed whatever has arrived since the last look (never waits)
int out_advance(ngd_engine *e) {
  auto &o = e->out;
  while (o.n_landed < o.chunks.size()) {
    const hipError_t q = hipEventQuery(o.chunks[o.n_landed].first);
    if (q == hipErrorNotReady) break;
    HIPCHK(q);
    out_declare(e, (uint64_t)o.chunks[o.n_landed].second * ngd_n_pairs(e->g.n_ind));
    o.n_landed++;
  }
  return NGD_OK;
}

// The end of a streamed call, good or bad: the host's threads are let through whatever is left (after a failure: over
// cells nobody will read) and joined.
static int out_join(ngd_engine *e, int rc) {
  auto &o = e->out;
  if (o.finisher.joinable()) {
    std::atomic_thread_fence(std::memory_order_release);
    o.landed = (uint64_t)o.n_mat * ngd_n_pairs(e->g.n_ind);
    o.finisher.join();
    if (!rc && o.finisher_rc) rc = fail(o.finisher_rc, "ngd_run_*_dist: the tail of gen_dist() failed");
  }
  o.on = false;
  return rc;
}

// What has been queued carries sums that a fix-up pass is about to replace
int out_requeue(ngd_engine *e) {
  auto &o = e->out;
  if (!o.on) return NGD_OK;
  HIPCHK(hipStreamSynchronize(o.st));
  HIPCHK(hipStreamSynchronize(o.st2));
  // pieces may have been declared landed already (partials_impl lands what arrives while the last groups are reduced): the
  // host's threads are let through the stale cells and start again from nothing once the matrices have been reduced again
  if (int rc = out_join(e, NGD_OK)) return rc;
  o.on = true;
  o.landed = 0;
  o.n_landed = 0;
  o.queued = 0;
  o.chunks.clear();
  return NGD_OK;
}

void out_start_finisher(ngd_engine *e) {
  auto &o = e->out;
  if (!o.on || o.finisher.joinable()) return;
  o.finisher_rc = 0;
  if (o.tot_sites) o.cnt_mat.assign(o.n_mat, o.tot_sites);
  const uint64_t n_pairs = ngd_n_pairs(e->g.n_ind);
  o.finisher = std::thread([e, n_pairs]() {
    auto &q = e->out;
    q.finisher_rc = ngd_finish_matrices_stream(q.h_sum, q.pdel ? q.h_cnt : nullptr, q.pdel ? nullptr : q.cnt_mat.data(), q.n_mat, n_pairs,
                                               q.evol_model, q.dist, &q.landed);
  });
}

static int out_land_all(ngd_engine *e) {
  auto &o = e->out;
  for (; o.n_landed < o.chunks.size(); o.n_landed++) {
    HIPCHK(hipEventSynchronize(o.chunks[o.n_landed].first));
    out_declare(e, (uint64_t)o.chunks[o.n_landed].second * ngd_n_pairs(e->g.n_ind));
  }
  return NGD_OK;
}

static int out_land(ngd_engine *e) {
  auto &o = e->out;
  int rc = out_queue(e, o.n_mat);
  if (!rc) {
    out_start_finisher(e);
    rc = out_land_all(e);
  }
  rc = out_join(e, rc);
  if (out_trace()) fprintf(stderr, "[out] tail joined +%.3f\n", out_now() - o.t0);
  return rc;
}

int copy_out(ngd_engine *e, uint32_t n_mat, const double *d_sum, const unsigned long long *d_cnt, double *sum,
             uint64_t *cnt) {
  e->n_batch_valid = d_sum == e->d_bsum ? n_mat : 0;
  const uint64_t n = (uint64_t)n_mat * ngd_n_pairs(e->g.n_ind);
  if (sum) HIPCHK(hipMemcpy(sum, d_sum, n * sizeof(double), hipMemcpyDeviceToHost));
  if (cnt) HIPCHK(hipMemcpy(cnt, d_cnt, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return NGD_OK;
}

int batch_buffers(ngd_engine *e, uint32_t n_rep) {
  e->n_batch_valid = 0;  // (the buffers may be freed and grown below; a failed call leaves nothing to fetch)
  HIPCHK(hipSetDevice(e->device));
  const uint64_t need = (uint64_t)n_rep * ngd_n_pairs(e->g.n_ind);
  if (int rc = e->d_bsum.ensure(e, need)) return rc;
  return e->d_bcnt.ensure(e, need);
}

// the host-pointer entry points: into the engine's own result arrays (n_batch = 0: one matrix) or its batch buffers, then out
int run_to_host(ngd_engine *e, const uint64_t *block_maps, const uint32_t *mult, uint32_t n_rep, bool lead_full,
                uint64_t n_blocks, uint64_t block_size, uint32_t n_batch, double *sum, uint64_t *cnt) {
  if (n_rep)
    if (int rc = em_exact_refuse_weighted(e, "a run with a block map or multiplicities, a batch or a job")) return rc;
  if (n_batch)
    if (int rc = batch_buffers(e, n_batch)) return rc;
  double *d_sum = n_batch ? e->d_bsum : e->d_sum;
  unsigned long long *d_cnt = n_batch ? e->d_bcnt : e->d_cnt;
  if (int rc = run_impl(e, block_maps, mult, n_rep, lead_full, n_blocks, block_size, d_sum, d_cnt)) return rc;
  return copy_out(e, n_batch ? n_batch : 1, d_sum, d_cnt, sum, cnt);
}

// the job driver of the tails (ngd_engine.h): ngd_run_job_device into the batch buffers, where the matrices stay
// (ngd_fetch_matrix), then the tail on that one set
int job_tail(ngd_engine *e, const uint64_t *block_maps, uint32_t n_rep, uint64_t n_blocks, uint64_t block_size, const Tail &tail) {
  if (int rc = batch_buffers(e, n_rep + 1)) return rc;
  if (int rc = run_impl(e, block_maps, nullptr, n_rep, n_rep != 0, n_blocks, block_size, e->d_bsum, e->d_bcnt)) return rc;
  e->n_batch_valid = n_rep + 1;
  return tail(0, 1, (uint64_t)n_rep + 1);
}

int finish_refuse(const ngd_engine *e, uint64_t tot_sites, uint64_t evol_model, const std::string &who, const char *no_what) {
  if (tot_sites && e->cfg.pairwise_del)
    return fail(NGD_E_INVALID, who + ": a total number of sites cannot go with pairwise deletion (parse_args.cpp:209-210)");
  if (evol_model > 2) return fail(NGD_E_MODEL, who + ": evolutionary model not supported (ngsDist.cpp:398-399)");
  if (no_what && e->cfg.shard_world > 1)
    return fail(NGD_E_INVALID, who + ": an engine that owns a share of the pairs holds part of every matrix: " + no_what);
  return NGD_OK;
}

// A whole job AND the tail of gen_dist() (ngsDist.cpp:372-401) in one call: the sums (and, --pairwise_del, the counts) leave
// the device chunk by chunk on a stream of their own into pinned memory of the engine's while -- in the per-block-partials
// plan -- later groups of replicates are still being reduced, and the host's threads turn each chunk into distances as it
// lands.  The matrices stay in the engine as after ngd_run_job(..., NULL, NULL) (ngd_fetch_matrix).
int run_dist(ngd_engine *e, const uint64_t *block_maps, const uint32_t *mult, uint32_t n_rep, bool lead_full,
             uint64_t n_blocks, uint64_t block_size, uint64_t tot_sites, uint64_t evol_model, double *dist, const char *who) {
  if (!e || !dist) return fail(NGD_E_INVALID, std::string(who) + ": null argument");
  if (int rc = finish_refuse(e, tot_sites, evol_model, who, nullptr)) return rc;
  if (e->cfg.shard_world > 1)
    return fail(NGD_E_INVALID, std::string(who) + ": an engine that owns a share of the pairs holds part of every matrix -- put the "
                               "shares together first (ngd_run_job_device + the ranks' exchange), then ngd_finish()");
  if (!e->committed) return fail(NGD_E_INVALID, std::string(who) + ": call ngd_commit() first");
  if (n_rep)
    if (int rc = em_exact_refuse_weighted(e, who)) return rc;
  const double t_enter = out_now();
  HIPCHK(hipSetDevice(e->device));
  const uint32_t n_mat = n_rep ? n_rep + (lead_full ? 1u : 0u) : 1u;
  int rc = batch_buffers(e, n_mat);
  if (rc) return rc;
  auto &o = e->out;
  const uint64_t cells = (uint64_t)n_mat * ngd_n_pairs(e->g.n_ind);
  if (!o.st) HIPCHK(hipStreamCreateWithFlags(&o.st, hipStreamNonBlocking));
  if (!o.st2) HIPCHK(hipStreamCreateWithFlags(&o.st2, hipStreamNonBlocking));
  if ((rc = o.h_sum.ensure(cells))) return rc;
  o.pdel = e->cfg.pairwise_del != 0;
  if (o.pdel && (rc = o.h_cnt.ensure(cells))) return rc;
  o.n_mat = n_mat;
  o.queued = 0;
  o.n_used = 0;
  o.n_chunk_seq = 0;
  o.n_landed = 0;
  o.chunks.clear();
  o.landed = 0;
  o.evol_model = evol_model;
  o.tot_sites = tot_sites;
  o.dist = dist;
  o.cnt_mat.assign(n_mat, e->g.n_sites);  // (a plain pass; a job's run_impl writes its matrices' own)
  o.on = true;
  o.t_call = out_now();
  rc = run_impl(e, block_maps, mult, n_rep, n_rep && lead_full, n_blocks, block_size, e->d_bsum, e->d_bcnt);
  rc = rc ? out_join(e, rc) : out_land(e);
  if (!rc) e->n_batch_valid = n_mat;
  if (out_trace()) fprintf(stderr, "[out] call: %.3f ms (setup before it %.3f)\n", out_now() - o.t_call, o.t_call - t_enter);
  return rc;
}
