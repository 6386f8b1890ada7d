// mjhmc_iterate: the call block, the per-iteration kernel arguments, and one function per launch schedule
// (schedule.hpp chooses among them); mjhmc_iterate_download, which brings the samples over while the schedules run.
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <type_traits>
#include <vector>

#include "energies.hpp"  // MMGaussF::kRelayMinL
#include "sampler_internal.hpp"
#include "schedule.hpp"

// The call block (handles.hpp): [Control, kCtlBytes][flf_counts, counts_bytes(cap)][stats, cap x 4 x 8 bytes]
constexpr size_t kCtlBytes = 64;
static_assert(sizeof(Control) <= kCtlBytes, "the failure flag's slot of the call block");
static size_t counts_bytes(int cap) { return (((size_t)cap + 1) * sizeof(int) + 63) / 64 * 64; }
int ensure_call_block(mjhmc_sampler* s, int rows) {
  if (s->call_block && s->stats_cap >= rows) return 0;
  const int cap = std::max(rows, 1024);
  if (s->call_block) {   // (calls end with a stream sync: nothing in flight reads the old block)
    HIPCHK(hipStreamSynchronize(s->stream));
    HIPCHK(hipFree(s->call_block));
    s->call_block = nullptr;
    s->ctl = nullptr;
    s->flf_counts = nullptr;
    s->stats = nullptr;
    s->stats_cap = 0;
  }
  const size_t total = kCtlBytes + counts_bytes(cap) + (size_t)cap * 4 * sizeof(long long);
  HIPCHK(hipMalloc((void**)&s->call_block, total));
  HIPCHK(hipMemsetAsync(s->call_block, 0, total, s->stream));
  s->ctl = (Control*)s->call_block;
  s->flf_counts = (int*)(s->call_block + kCtlBytes);
  s->stats = (long long*)(s->call_block + kCtlBytes + counts_bytes(cap));
  s->stats_cap = cap;
  return 0;
}
// the start of a call: failure flag, counters and the first `rows` tallies zeroed by ONE fill
static int zero_call(mjhmc_sampler* s, int rows) {
  TRY(ensure_call_block(s, rows));
  HIPCHK(hipMemsetAsync(s->call_block, 0, kCtlBytes + counts_bytes(s->stats_cap) + (size_t)rows * 4 * sizeof(long long), s->stream));
  return 0;
}

// The bracket every device schedule puts around its launches.  begin_call: the call block zeroed, then the opening event.
// One HIP-event pair brackets the whole launch sequence of a call (first jump kernel .. last jump kernel, on the
// sampler's stream).  Per-launch event pairs were measured to cost more than they tell: every marker packet opens a
// ~5 us bubble between back-to-back kernels.
static int begin_call(mjhmc_sampler* s, int rows) {
  TRY(zero_call(s, rows));
  if (s->timing_on) HIPCHK(hipEventRecord(s->ev_total[0], s->stream));
  return 0;
}

// end_call: the closing event, then failure flag + cold-list counters + tallies of the call: ONE copy of the head of the
// call block into pinned host memory (a pageable destination makes a small copy a synchronous staged transfer: ~20 us)
// and ONE stream sync.  Until round 6 the call was three fills, two asynchronous copies and -- for the compacted passes --
// a synchronous third.
static int end_call(mjhmc_sampler* s, size_t stats_rows, Control* hc, long long* hs, int* counts = nullptr, int n_counts = 0) {
  if (s->timing_on) HIPCHK(hipEventRecord(s->ev_total[1], s->stream));
  const size_t head = kCtlBytes + counts_bytes(s->stats_cap);
  const size_t need = head + stats_rows * 4 * sizeof(long long);
  if (s->h_pin_cap < need) {
    if (s->h_pin) HIPCHK(hipHostFree(s->h_pin));
    s->h_pin = nullptr;
    s->h_pin_cap = 0;
    HIPCHK(hipHostMalloc((void**)&s->h_pin, need * 2, hipHostMallocDefault));
    s->h_pin_cap = need * 2;
  }
  HIPCHK(hipMemcpyAsync(s->h_pin, s->call_block, need, hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  std::memcpy(hc, s->h_pin, sizeof(Control));
  if (counts) std::memcpy(counts, s->h_pin + kCtlBytes, (size_t)n_counts * sizeof(int));
  std::memcpy(hs, s->h_pin + head, stats_rows * 4 * sizeof(long long));
  return 0;
}

// per-attempt counters of one mjhmc_iterate call from the device tallies hs[attempt][4]
static void fill_iter_stats(const mjhmc_sampler* s, const std::vector<long long>& hs, int attempts, int done, bool failed,
                            mjhmc_iter_stats* per_iter) {
  if (!per_iter) return;
  for (int i = 0; i < attempts; ++i) {
    mjhmc_iter_stats& st = per_iter[i];
    std::memset(&st, 0, sizeof(st));
    clocks_to_stats(s->mode, &hs[4 * i], &st);
    if (s->mode == MJHMC_MODE_MJHMC) st.n_cold = hs[4 * i + 3] & 0xFFFFFFFFLL;   // (the dense kernels: integrated inverse-L trajectories in the high half)
    st.E_evals = s->N + st.n_cold;  // L on all (+ FLF on the cold ones)
    st.dEdX_evals = (int64_t)s->L * (s->N + st.n_cold);
    st.nonfinite = (failed && i == done) ? 1 : 0;
    st.L_used = s->L;
    st.eps_used = s->eps;
    // inverse-L trajectories integrated: all of the cold ones -- the dense kernels skip the F-movers' (dense_pot.hip)
    st.n_flf_run = (s->mode == MJHMC_MODE_MJHMC && s->en->is_dense()) ? (hs[4 * i + 3] >> 32) : st.n_cold;
  }
}

// commit_call: everything after the read-back.  `done` iterations are committed of `attempts` started (the failed one
// included: its RNG tick stays consumed); the buffer parities advance by `parity_steps` -- iterations, or launches for
// the fused schedule -- and the live state is `xlive`.  undo: the input buffers of a single committed iteration survive
// it (mjhmc_rollback); the fused schedule never leaves one.
static int commit_call(mjhmc_sampler* s, const std::vector<long long>& hs, const Control& hc, int done, int attempts,
                       int parity_steps, void* xlive, bool undo, mjhmc_iter_stats* per_iter, int* n_done) {
  fill_iter_stats(s, hs, attempts, done, hc.failed != 0, per_iter);
  s->undo_valid = undo;
  if (undo) {
    s->undo_multipass = false;
    s->undo_X = s->Xcur;
  }
  s->Xcur = xlive;
  s->vcur = (s->vcur + parity_steps) & 1;
  s->scur = (s->scur + parity_steps) & 1;
  s->tick += (uint64_t)attempts;
  if (n_done) *n_done = done;
  s->last_jump_launches = attempts;
  s->timing_pending = s->timing_on;
  return 0;
}

// ... of the schedules that launch iteration by iteration and stop at the first attempt with a non-finite rate
static int commit_iterations(mjhmc_sampler* s, const std::vector<long long>& hs, const Control& hc, int n_iter,
                             const std::vector<void*>& xout, mjhmc_iter_stats* per_iter, int* n_done) {
  const int done = hc.failed ? hc.failed_iter : n_iter;
  return commit_call(s, hs, hc, done, hc.failed ? done + 1 : n_iter, done, done > 0 ? xout[(size_t)done - 1] : s->Xcur,
                     n_iter == 1 && done == 1, per_iter, n_done);
}

static int ab_flags() {
  return (test_env("MJHMC_NO_BLOCK_DECIDE") ? kAbNoBlockDecide : 0) | (test_env("MJHMC_NO_WPP") ? kAbNoWpp : 0) |
         (test_env("MJHMC_NO_QUAD") ? kAbNoQuad : 0) | (test_env("MJHMC_NO_ROWS") ? kAbNoRows : 0) |
         (test_env("MJHMC_NO_RELAY") ? kAbNoRelay : 0) | (test_env("MJHMC_FORCE_RELAY") ? kAbForceRelay : 0);
}

// fused MarkovJumpHMC launches of this sampler run in row form (row_form.hpp: mjhmc_fused_rows_kernel)
static bool fused_rows(const mjhmc_sampler* s) {
  const int kind = s->en->ep.kind;
  // (the mixture's force is a division per coordinate: its row form pays through the relay kernel only -- 0.500 ms against
  // the group form's 0.535 at 32 x 10^6, L = 15, and 0.734 in the one-wave row kernel -- so it takes the row form where the
  // relay runs, launch_fused_rows: from MMGaussF::kRelayMinL leapfrog steps up)
  if (kind == MJHMC_E_MM_GAUSS && s->L < MMGaussF<double>::kRelayMinL && !test_env("MJHMC_FORCE_RELAY")) return false;
  return (kind == MJHMC_E_FUNNEL_NEAL || kind == MJHMC_E_FUNNEL_REF || kind == MJHMC_E_MM_GAUSS) && s->dtype == MJHMC_F64 &&
         s->sh.E == 8 &&
         fused_rows_shape(s->mode, s->sh.logG, ab_flags());
}

// indices of the particles that satisfy a predicate (inverse-L cache cold; moved by R), in arbitrary order.  Each block scans
// kColdChunk particles, collects its hits in LDS and reserves its stretch of the list with ONE global atomic
// (a global atomic per wave serialised on the single counter: 178 us for 10^6 particles, this form ~10 us).
constexpr int kColdChunk = 4096;
template <typename T>
struct ColdCache {  // H_flf is NaN; the scan also writes the copy of H_flf that the inverse-L pass completes
  const T* h;
  T* copy;
  __device__ bool operator()(int64_t p) const {
    const T v = h[p];
    copy[p] = v;
    return v != v;
  }
};
template <class Pred>
__global__ __launch_bounds__(1024) void compact_list_kernel(const Pred pred, int64_t N, const Control* ctl,
                                                            int* __restrict__ list, int* __restrict__ count) {
  __shared__ int hits[kColdChunk];
  __shared__ int n_hits, base;
  if (ctl->failed) return;
  if (threadIdx.x == 0) n_hits = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  for (int k = 0; k < kColdChunk / 1024; ++k) {
    const int64_t p = (int64_t)blockIdx.x * kColdChunk + k * 1024 + threadIdx.x;
    const bool cold = p < N && pred(p);
    const unsigned long long mask = __ballot(cold);
    if (mask) {
      int at = 0;
      if (lane == 0) at = atomicAdd(&n_hits, __popcll(mask));
      at = __shfl(at, 0);
      if (cold) hits[at + __popcll(mask & ((1ull << lane) - 1ull))] = (int)p;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) base = atomicAdd(count, n_hits);
  __syncthreads();
  for (int i = threadIdx.x; i < n_hits; i += 1024) list[base + i] = hits[i];
}

// ---------------------------------------------------------------------------------------------
// mjhmc_iterate_download: samples cross PCIe WHILE the sampler iterates.
// HMCBase.sample / ContinuousTimeHMC.sample (markov_jump_hmc.py:150-173, 293-338) append state.copy().X after every
// iteration; here iteration i writes its X into ring slot ring_slot0 + i and, as soon as its kernels are done, a
// worker thread of the call re-tiles that slot on a second stream into the reference's (ndims, particles) layout and
// brings it to the caller's time-major array (pinned double buffer, host copy threads) -- beside iterations
// i + 1, i + 2, ... on the sampler's own streams.  The launch code marks an iteration by recording an event on every
// stream that runs part of it (dl_mark); the worker never reads a slot whose events have not completed.
// ---------------------------------------------------------------------------------------------
struct DlSession {
  std::vector<std::vector<hipEvent_t>> ev;   // [iteration] the events that complete it
  std::atomic<int> marked{0};                // iterations whose events are recorded
  std::atomic<bool> launched{false};         // the iterate call has returned: nothing more will be marked
  int n_iter = 0, ring_slot0 = 0;
  double* host = nullptr;                    // (D, n_total * N) float64, time-major
  int64_t n_total = 0, k0 = 0;
  std::atomic<int> downloaded{0};            // slots [0, downloaded) are in the host array
  std::vector<char> retiled;                 // [iteration] its slot already sits, in the host layout, in staging slot i (see dl_done)
  std::atomic<bool> cancel{false};           // dl_restart: the worker leaves at its next look
  std::atomic<bool> exited{false};           // the worker has left: nothing of the session is touched from its thread any more
  bool off = false;                          // after dl_restart: the launch code marks nothing, the caller downloads when the call is over
  int rc = 0;
  std::string err;
};

// The parts of a batch on their streams: part k holds particles [k * len, (k + 1) * len), the last part the rest; part 0
// runs on the sampler's own stream.  One part: the whole batch there.
struct Parts {
  int n = 1;
  int64_t len = 0;
  int64_t start(int k) const { return (int64_t)k * len; }
  int64_t count(const mjhmc_sampler* s, int k) const { return k + 1 == n ? s->N - start(k) : len; }
  int64_t npad(const mjhmc_sampler* s, int k) const { return k + 1 == n ? s->Npad - start(k) : len; }
  hipStream_t stream(const mjhmc_sampler* s, int k) const { return k == 0 ? s->stream : s->part_streams[(size_t)k - 1]; }
  int of(int64_t particle) const { return n > 1 ? (int)std::min<int64_t>(particle / len, n - 1) : 0; }
};

// particle-major rows [start, start + ncols) of a state matrix -> columns [start, start + ncols) of the compact (D, N) float64
// matrix `stage`: the reference's layout
static int dl_retile(mjhmc_sampler* s, const void* rows0, int64_t start, int64_t ncols, double* stage, hipStream_t st) {
  return launch_to_dim_major(st, s->dtype, (const char*)rows0 + (size_t)start * row_bytes(s), nullptr, stage, s->D, ncols,
                             s->sh.pitch, s->N, 1, start);
}

// called by the launch code once the kernels completing iterations [i0, i0 + n) of the call are queued
static int dl_mark(mjhmc_sampler* s, int i0, int n, const hipStream_t* streams, int n_streams) {
  DlSession* d = s->dl;
  if (!d || d->off || i0 < d->marked.load(std::memory_order_acquire)) return 0;   // (a re-run after a failure rewrites marked slots with the same values)
  for (int i = i0; i < i0 + n && i < d->n_iter; ++i) {
    for (int k = 0; k < n_streams; ++k) {
      hipEvent_t e = nullptr;
      if (i == i0) {
        HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        HIPCHK(hipEventRecord(e, streams[k]));
      } else {
        e = d->ev[(size_t)i0][(size_t)k];    // iterations of one fused launch complete together
      }
      d->ev[(size_t)i].push_back(e);
    }
  }
  d->marked.store(std::min(i0 + n, d->n_iter), std::memory_order_release);
  return 0;
}

// Iteration j of the call, whose new X is xj, is complete when every stream that ran part of it gets here -- and each of
// them re-tiles its own columns of xj into staging slot j on the way (0.3 ms of a 17 ms C3 iteration): on a stream of
// its own that kernel waited for a workgroup of the NEXT iteration's persistent grid to leave, so every slot crossed
// PCIe one iteration late and two of them after the run had ended.  The worker then only moves bytes (copy engine + host).
static int dl_done(mjhmc_sampler* s, int ring_slot0, int j, const void* xj, const Parts& parts) {
  if (!(s->dl && !s->dl->off && ring_slot0 >= 0 && j >= s->dl->marked.load(std::memory_order_acquire))) return 0;
  hipStream_t sts[kMaxDenseParts];
  const size_t elems = (size_t)s->D * s->N;
  const bool room = s->dl_stage_elems >= (size_t)s->dl->n_iter * elems;
  for (int k = 0; k < parts.n; ++k) {
    sts[k] = parts.stream(s, k);
    if (room) TRY(dl_retile(s, xj, parts.start(k), parts.count(s, k), s->dl_stage + (size_t)j * elems, sts[k]));
  }
  s->dl->retiled[(size_t)j] = room ? 1 : 0;
  return dl_mark(s, j, 1, sts, parts.n);
}

static int dl_download_slot(mjhmc_sampler* s, DlSession* d, int i) {
  const size_t elems = (size_t)s->D * s->N;
  const size_t bytes = elems * sizeof(double), row = (size_t)s->N * sizeof(double);
  const void* src = (const char*)s->ring + (size_t)(d->ring_slot0 + i) * mat_bytes(s);
  const bool retiled = d->retiled[(size_t)i] != 0;
  const double* stage = retiled ? s->dl_stage + (size_t)i * elems : s->dl_stage;
  if (!retiled) TRY(dl_retile(s, src, 0, s->N, s->dl_stage, s->dl_stream));
  // compact (D, N) staging -> row d of the slot lands at host[(d * n_total + k0 + i) * N]; chunks through the pinned pair,
  // each chunk's bytes row by row over the copy threads
  char* host = (char*)d->host;
  const size_t dst_row = (size_t)d->n_total * row, dst_off = (size_t)(d->k0 + i) * row;
  return pipe_chunks(s->dl_stream, s->dl_pin, s->dl_ev, stage, bytes, [=](size_t off, const char* pin, size_t lo, size_t hi) {
    size_t o = lo;
    while (o < hi) {
      const size_t g = off + o, dd = g / row, within = g % row;
      const size_t n = std::min(row - within, hi - o);
      std::memcpy(host + dd * dst_row + dst_off + within, pin + o, n);
      o += n;
    }
  });
}

static void dl_worker_body(mjhmc_sampler* s, DlSession* d) {
  if (hipSetDevice(s->ctx->device) != hipSuccess) {
    d->rc = MJHMC_ERR_HIP;
    d->err = "hipSetDevice failed in the download thread";
    return;
  }
  for (int i = 0; i < d->n_iter; ++i) {
    while (d->marked.load(std::memory_order_acquire) <= i && !d->launched.load(std::memory_order_acquire) &&
           !d->cancel.load(std::memory_order_acquire))
      std::this_thread::sleep_for(std::chrono::microseconds(50));
    if (d->cancel.load(std::memory_order_acquire)) return;
    if (d->marked.load(std::memory_order_acquire) <= i) break;   // a path that marks nothing: the caller downloads afterwards
    for (hipEvent_t e : d->ev[(size_t)i])
      if (hipStreamWaitEvent(s->dl_stream, e, 0) != hipSuccess) {
        d->rc = MJHMC_ERR_HIP;
        d->err = "hipStreamWaitEvent failed in the download thread";
        return;
      }
    const int rc = dl_download_slot(s, d, i);
    if (rc) {
      d->rc = rc;
      d->err = last_error_text();   // (thread-local: hand the message to the calling thread)
      return;
    }
    if (d->cancel.load(std::memory_order_acquire)) return;   // (the slot it has just brought over is about to be rewritten)
    d->downloaded.store(i + 1, std::memory_order_release);
  }
}

static void dl_worker(mjhmc_sampler* s, DlSession* d) {
  dl_worker_body(s, d);
  d->exited.store(true, std::memory_order_release);
}

// the events of a session, each destroyed once (the iterations of a fused launch share theirs)
static void dl_destroy_events(DlSession* d) {
  for (size_t i = 0; i < d->ev.size(); ++i)
    for (hipEvent_t e : d->ev[i]) {
      bool first = true;
      for (size_t j = 0; j < i && first; ++j)
        for (hipEvent_t f : d->ev[j]) first = first && f != e;
      if (first) (void)hipEventDestroy(e);
    }
  for (auto& v : d->ev) v.clear();
}

// A call that is about to be run AGAIN from its first iteration (mjhmc_iterate: a non-finite rate while the parts of a
// dense batch ran freely -- the state is put back and the call re-run on one stream) while samples are being downloaded:
// what the first run marked is void.  A lagging part returned early in the failing iteration and left its columns of the
// ring slots and of the staging slots stale, and the re-run rewrites every slot: the worker must neither have copied nor
// copy any of them.  The worker is told to leave and waited for, its stream drained, the session emptied and switched
// off -- the re-run marks nothing, and mjhmc_iterate_download brings slots [0, done) over when the call has returned.
static int dl_restart(mjhmc_sampler* s) {
  DlSession* d = s->dl;
  if (!d) return 0;
  d->cancel.store(true, std::memory_order_release);
  while (!d->exited.load(std::memory_order_acquire)) std::this_thread::sleep_for(std::chrono::microseconds(50));
  if (s->dl_stream) HIPCHK(hipStreamSynchronize(s->dl_stream));
  dl_destroy_events(d);
  d->marked.store(0, std::memory_order_release);
  d->downloaded.store(0, std::memory_order_release);
  std::fill(d->retiled.begin(), d->retiled.end(), 0);
  d->off = true;
  return 0;
}

// ---------------------------------------------------------------------------------------------
// the argument blocks of an iteration
// ---------------------------------------------------------------------------------------------
// the tile kernels' argument blocks (sampler_args.hpp), apart from the elementwise energies' JumpArgs<T>
template <class A>
struct IsDenseJump : std::false_type {};
template <typename S, typename H, bool POT>
struct IsDenseJump<DenseJumpArgs<S, H, POT>> : std::true_type {};

// part `which` of a split batch: particles [start, start + n), their rows of every per-particle array; of a dense batch
// also their stretch of the lists and their own three rotating counters (iteration i reads slot i % 3, appends to
// (i + 1) % 3, clears (i + 2) % 3)
template <class A>
static A part_args(const A& a, int64_t start, int64_t n, int64_t npad, size_t pitch, int which, int* counters) {
  A h = a;
  h.X_in = a.X_in + (size_t)start * pitch;
  h.V_in = a.V_in + (size_t)start * pitch;
  h.X_out = a.X_out + (size_t)start * pitch;
  h.V_out = a.V_out + (size_t)start * pitch;
  h.EX_in = a.EX_in + start;
  h.EV_in = a.EV_in + start;
  h.Hflf_in = a.Hflf_in + start;
  h.EX_out = a.EX_out + start;
  h.EV_out = a.EV_out + start;
  h.Hflf_out = a.Hflf_out + start;
  h.dwell = a.dwell + start;
  h.dwell_ring = a.dwell_ring + start;
  h.trans = a.trans + start;
  if constexpr (IsDenseJump<A>::value) {
    h.Hspec_in = a.Hspec_in + start;
    h.Hwork = a.Hwork + start;
    h.Hspec_out = a.Hspec_out + start;
    h.cold_list = a.cold_list + start;
    h.next_list = a.next_list + start;
    h.cold_count = counters + 3 * which + a.iter % 3;
    h.next_count = counters + 3 * which + (a.iter + 1) % 3;
    h.zero_count = counters + 3 * which + (a.iter + 2) % 3;
    if constexpr (A::kPot) {
      h.G_in = a.G_in + (size_t)start * pitch;
      h.G_out = a.G_out + (size_t)start * pitch;
    }
  }
  h.N = n;
  h.Npad = npad;
  h.first_pid = a.first_pid + start;
  return h;
}

// The parts of a dense batch on their streams (part 0: the sampler's own)
static int ensure_part_streams(mjhmc_sampler* s, int n_parts) {
  if (!s->ev_fork) {
    HIPCHK(hipEventCreateWithFlags(&s->ev_fork, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&s->ev_join, hipEventDisableTiming));
  }
  while ((int)s->part_streams.size() < n_parts - 1) {
    hipStream_t q;
    hipEvent_t e;
    HIPCHK(hipStreamCreateWithFlags(&q, hipStreamNonBlocking));
    s->part_streams.push_back(q);
    HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    s->part_events.push_back(e);
  }
  return 0;
}

// the state a multi-iteration split call starts from, copied aside / put back (the layout of mjhmc_checkpoint, own buffers)
static int split_state_copy(mjhmc_sampler* s, bool restore) {
  void* live[7];
  size_t sizes[7];
  const int nck = live_state(s, s->en->is_pot(), live, sizes);   // (the only dE/dX-keeping sampler this schedule runs)
  for (int i = 0; i < nck; ++i) {
    if (!s->ick[i]) HIPCHK(hipMalloc(&s->ick[i], sizes[i]));
    if (restore) HIPCHK(hipMemcpyAsync(live[i], s->ick[i], sizes[i], hipMemcpyDeviceToDevice, s->stream));
    else HIPCHK(hipMemcpyAsync(s->ick[i], live[i], sizes[i], hipMemcpyDeviceToDevice, s->stream));
  }
  // (Hspec follows scur and an attempt only writes the other parity, so the call's starting values survive a failed
  // attempt like H_flf's do -- but the halves may have run several iterations: both parities are overwritten)
  if (restore) TRY(drop_spec(s));
  return 0;
}

// The fields every jump block of an iteration shares (JumpArgs<T>, DenseJumpArgs<S, H>): iteration `iter` of the call reads
// X from xin, V of parity vi and the scalars of parity si, writes X to xout and the other parities, records its dwelling
// times in ring slot ring_slot0 + iter (or a scratch vector when nothing is recorded) and its tallies in `stats`.  The
// replay streams, the dense lists and the fused launches' fields are the caller's; the rest is left zero.
template <class A>
static A jump_args(const mjhmc_sampler* s, int iter, int vi, int si, const void* xin, void* xout, int ring_slot0,
                   long long* stats) {
  using S = std::remove_pointer_t<decltype(A::X_out)>;   // the state rows
  using H = std::remove_pointer_t<decltype(A::EX_out)>;  // the per-particle scalars and step parameters
  A a{};
  a.X_in = (const S*)xin;
  a.V_in = (const S*)s->Vbuf[vi];
  a.X_out = (S*)xout;
  a.V_out = (S*)s->Vbuf[vi ^ 1];
  a.EX_in = (const H*)s->EX[si];
  a.EV_in = (const H*)s->EV[si];
  a.Hflf_in = (const H*)s->Hflf[si];
  a.EX_out = (H*)s->EX[si ^ 1];
  a.EV_out = (H*)s->EV[si ^ 1];
  a.Hflf_out = (H*)s->Hflf[si ^ 1];
  a.dwell = s->dwell;
  a.dwell_ring = ring_slot0 >= 0 ? s->dwell_ring + (size_t)(ring_slot0 + iter) * s->Npad : s->dwell_scratch;
  a.trans = s->trans;
  a.ctl = s->ctl;
  a.stats = (unsigned long long*)stats;
  a.N = s->N;
  a.Npad = s->Npad;
  a.first_pid = s->first_pid;
  a.L = s->L;
  a.iter = iter;
  a.mode = s->mode;
  a.eps = (H)s->eps;  // (rounded once from the double expressions)
  a.chalf = (H)(-s->eps / 2.);
  a.r_keep = (H)std::sqrt(1. - s->beta);
  a.r_mix = (H)std::sqrt(s->beta);
  a.p_r = s->p_r;
  a.p_flip = s->p_flip;
  a.key = rng_key(s, s->tick + (uint64_t)iter);
  if constexpr (!IsDenseJump<A>::value) {
    a.D = s->D;
    a.pitch = s->sh.pitch;
    a.CH = s->sh.CH;
    a.logG = s->sh.logG;
    // the fused launch takes the row form exactly where fused_rows() says so: launch_jump_t's fused_rows_shape() sees the
    // lane mapping only, and without kAbNoRows the mixture below its kRelayMinL ran the one-wave row kernel
    a.ab = ab_flags() | (fused_rows(s) ? 0 : kAbNoRows);
  } else if constexpr (A::kPot) {
    a.D = s->D;
  }
  return a;
}

// The two launches of a compacted iteration from its finished jump block: the trajectories (the L proposals and, beside
// them, the inverse-L proposals of the `list`ed cold caches, their H into Hwork) ...
template <typename T>
static TrajArgs<T> traj_args(const JumpArgs<T>& a, T* Hwork, const int* list, const int* count, int n_listed) {
  const int64_t ppb = 256 >> a.logG;   // the list's walkers: sized for a typical list (a few per cent of the batch)
  return TrajArgs<T>{a.X_in, a.V_in, a.X_out, a.V_out, a.EX_out, a.EV_out, Hwork, list, count, a.ctl, a.N, a.D, a.pitch, a.CH,
                     a.logG, a.L, n_listed, (int)std::max<int64_t>(1, std::min<int64_t>((a.N + ppb - 1) / ppb / 8, 2048)),
                     test_env("MJHMC_NO_ROWS") ? 0 : 1, a.eps, a.chalf};
}
// ... and the jump process with a lane per particle, which hands its movers on as the next iteration's list
template <typename T>
static JumpDecideArgs<T> decide_args(const JumpArgs<T>& a, const T* Hwork, int* next_list, int* next_count) {
  return JumpDecideArgs<T>{a.X_in, a.V_in, a.X_out, a.V_out, a.EX_in, a.EV_in, a.EX_out, a.EV_out, a.Hflf_in, Hwork, a.Hflf_out,
                           a.dwell, a.dwell_ring, a.trans, next_list, next_count, a.ctl, a.stats, a.N, a.first_pid, a.D,
                           a.pitch, a.CH, a.logG, a.iter, a.r_keep, a.r_mix, a.p_r, a.key};
}

// the live state sits in one of the ring slots [slot0, slot0 + n) about to be overwritten: move it out first
static int move_out_of_ring(mjhmc_sampler* s, int slot0, int n) {
  const size_t mb = mat_bytes(s);
  const char* lo = (const char*)s->ring + (size_t)slot0 * mb;
  if ((const char*)s->Xcur >= lo && (const char*)s->Xcur < lo + (size_t)n * mb) {
    HIPCHK(hipMemcpyAsync(s->Xbuf[0], s->Xcur, mb, hipMemcpyDeviceToDevice, s->stream));
    s->Xcur = s->Xbuf[0];
  }
  return 0;
}

// where iteration i of a call writes its X: its ring slot, or the ping-pong buffer its input is not in
static void* iteration_out(const mjhmc_sampler* s, int ring_slot0, int i, const void* xin) {
  return ring_slot0 >= 0 ? (void*)((char*)s->ring + (size_t)(ring_slot0 + i) * mat_bytes(s))
                         : (xin != s->Xbuf[0] ? s->Xbuf[0] : s->Xbuf[1]);
}

// test hook MJHMC_DEBUG_POISON="iteration:particle": that particle's kinetic energy (parity si) reads NaN in that iteration
// of the call -> its rates are not finite -> the whole-batch abort of markov_jump_hmc.py:376-389, at a chosen point of a
// multi-iteration call.  The write goes to the stream that runs the particle's part.
static int debug_poison(mjhmc_sampler* s, int iter, int si, const Parts& parts) {
  const char* poison = test_env("MJHMC_DEBUG_POISON");
  int pit = -1;
  long long pp = -1;
  if (!poison || std::sscanf(poison, "%d:%lld", &pit, &pp) != 2 || pit != iter || pp < 0 || pp >= s->N) return 0;
  static const double nan64 = __builtin_nan("");
  static const float nan32 = __builtin_nanf("");
  const hipStream_t pst = parts.stream(s, parts.of(pp));
  if (pst != s->stream && iter == 0) HIPCHK(hipStreamSynchronize(s->stream));  // (the fork to the parts' streams comes later)
  HIPCHK(hipMemcpyAsync((char*)s->EV[si] + (size_t)pp * ssize(s), ssize(s) == 8 ? (const void*)&nan64 : (const void*)&nan32,
                        ssize(s), hipMemcpyHostToDevice, pst));
  return 0;
}

// the replay streams of a call, (n_iter, ...) host arrays or NULL: uploaded iteration by iteration
struct Replay {
  const double* normal;
  const double* exp;
  const double* unif;
  bool any() const { return normal || exp || unif; }
};
static int replay_alloc(mjhmc_sampler* s, const Replay& rp) {
  if (rp.normal && !s->noise) {
    HIPCHK(hipMalloc(&s->noise, mat_bytes(s)));
    HIPCHK(hipMemsetAsync(s->noise, 0, mat_bytes(s), s->stream));
  }
  if (rp.exp && !s->rexp) HIPCHK(hipMalloc((void**)&s->rexp, 3 * s->N * sizeof(double)));
  if (rp.unif && !s->runif) HIPCHK(hipMalloc((void**)&s->runif, (2 * s->N + 1) * sizeof(double)));
  return 0;
}
static int replay_upload(mjhmc_sampler* s, const Replay& rp, int i) {
  if (rp.normal) TRY(upload_matrix(s, rp.normal + (size_t)i * s->D * s->N, s->noise));
  if (rp.exp)
    HIPCHK(hipMemcpyAsync(s->rexp, rp.exp + (size_t)i * 3 * s->N, 3 * s->N * sizeof(double), hipMemcpyHostToDevice, s->stream));
  if (rp.unif)
    HIPCHK(hipMemcpyAsync(s->runif, rp.unif + (size_t)i * (2 * s->N + 1), (2 * s->N + 1) * sizeof(double),
                          hipMemcpyHostToDevice, s->stream));
  return 0;
}

// ---------------------------------------------------------------------------------------------
// the schedules
// ---------------------------------------------------------------------------------------------
// Elementwise energies, counter RNG, n_iter >= 2: launches of up to kMaxFuse FUSED iterations.  A launch reads
// the state buffers of one parity and writes the other, so its input survives it: when some particle meets a
// non-finite rate at iteration f (the reference aborts the WHOLE batch there, markov_jump_hmc.py:376-389) the
// launch that contains f is run again for the iterations before f and the call returns n_done = f.
template <typename T>
static int iterate_fused_t(mjhmc_sampler* s, int n_iter, int ring_slot0, mjhmc_iter_stats* per_iter, int* n_done) {
  const size_t mb = mat_bytes(s);
  const int need = n_iter + kMaxFuse;  // + scratch tallies for the recovery launch

  if (ring_slot0 >= 0) TRY(move_out_of_ring(s, ring_slot0, n_iter));   // (a launch writes several slots while it reads xin)
  void* xin = s->Xcur;
  struct Launch {
    int i0, K, vi, si;
    void* xin;
    void* xout;
  };
  int64_t split_at = 0;  // particles per part
  int n_parts = 3;       // C2: 2 / 3 / 4 / 8 parts measured 0.0803 / 0.0779 / 0.0803 / 0.0782 ms per iteration, unsplit 0.0855
  bool allow_split_now = true;  // (the recovery launch runs on one stream)
  if (ring_slot0 < 0 && !test_env("MJHMC_NO_SPLIT")) {
    if (const char* np = test_env("MJHMC_SPLIT_PARTS")) n_parts = std::max(2, std::min(8, std::atoi(np)));
    const int64_t nslots = s->Npad >> (6 - s->sh.logG);
    if (nslots >= 8 * 4096 && !fused_rows(s)) split_at = (s->Npad / n_parts) / 256 * 256;  // whole workgroups' worth of slots in every part
    if (split_at <= 0 || split_at * (n_parts - 1) >= s->N) split_at = 0;
    if (split_at) TRY(ensure_part_streams(s, n_parts));
  }
  auto launch = [&](const Launch& l, long long* stats) -> int {
    JumpArgs<T> a = jump_args<JumpArgs<T>>(s, l.i0, l.vi, l.si, l.xin, l.xout, ring_slot0, stats);
    a.n_fuse = l.K;
    if (ring_slot0 >= 0) {
      a.xiter = (T*)((char*)s->ring + (size_t)(ring_slot0 + l.i0) * mb);
      a.xiter_stride = mb / sizeof(T);
    }
    if (split_at > 0 && allow_split_now) {
      // several parts on as many streams: a launch is a persistent grid of one slot (here: up to 64 iterations of a
      // particle) per wave and pass, so it ends with a partial pass (C2: 100 000 slots on 4096 resident waves = 24.4
      // passes, 25 paid), and its workgroups all sit in the same phase of their slots at the same time; the parts'
      // workgroups start on the CUs the earlier parts leave and run out of step with them.  The parts meet at the end of
      // every fused launch (once per 64 iterations): the recovery protocol below relies on the inputs of the failing
      // launch being intact, i.e. on no part having started the next launch.
      HIPCHK(hipEventRecord(s->ev_fork, s->stream));
      const Parts parts{n_parts, split_at};
      for (int k = 0; k < n_parts; ++k) {
        const JumpArgs<T> h = part_args(a, parts.start(k), parts.count(s, k), parts.npad(s, k), (size_t)a.pitch, k, nullptr);
        hipStream_t q = parts.stream(s, k);
        if (k > 0) HIPCHK(hipStreamWaitEvent(q, s->ev_fork, 0));
        TRY(with_elementwise_energy(s->en->ep.kind, [&](auto en) { en.jump(h, s->en->ep, s->sh.E, q); }));
        if (k > 0) {
          HIPCHK(hipEventRecord(s->part_events[(size_t)k - 1], q));
          HIPCHK(hipStreamWaitEvent(s->stream, s->part_events[(size_t)k - 1], 0));
        }
      }
    } else {
      TRY(with_elementwise_energy(s->en->ep.kind, [&](auto en) { en.jump(a, s->en->ep, s->sh.E, s->stream); }));
    }
    HIPCHK(hipGetLastError());
    return 0;
  };
  // the last iteration of a launch writes the live state: into its ring slot, or the ping-pong buffer the input is not in
  auto out_of = [&](int i0, int K, void* in) { return iteration_out(s, ring_slot0, i0 + K - 1, in); };

  TRY(debug_poison(s, 0, s->scur, Parts{}));   // (fused launches: iteration 0 only, on the sampler's stream)
  std::vector<Launch> launches;
  TRY(begin_call(s, need));
  for (int i0 = 0; i0 < n_iter; i0 += kMaxFuse) {
    const int j = (int)launches.size();
    Launch l;
    l.i0 = i0;
    l.K = std::min(kMaxFuse, n_iter - i0);
    l.vi = (s->vcur + j) & 1;
    l.si = (s->scur + j) & 1;
    l.xin = xin;
    l.xout = out_of(i0, l.K, xin);
    TRY(launch(l, s->stats + 4 * (size_t)i0));
    launches.push_back(l);
    xin = l.xout;
  }
  Control hc;
  std::vector<long long> hs((size_t)n_iter * 4);
  TRY(end_call(s, (size_t)n_iter, &hc, hs.data()));

  int done = n_iter, attempts = n_iter, committed = (int)launches.size();
  void* xlive = launches.back().xout;
  if (hc.failed) {
    done = 0x7fffffff - hc.inv_iter;
    attempts = done + 1;
    committed = done / kMaxFuse;
    Launch l = launches[(size_t)committed];
    xlive = l.xin;
    l.K = done - l.i0;
    if (l.K > 0) {  // redo the iterations of that launch that precede the failed one (same ticks, same results)
      l.xout = out_of(l.i0, l.K, l.xin);
      long long* redo_stats = s->stats + 4 * (size_t)n_iter;
      HIPCHK(hipMemsetAsync(s->ctl, 0, sizeof(Control), s->stream));
      HIPCHK(hipMemsetAsync(redo_stats, 0, (size_t)kMaxFuse * 4 * sizeof(long long), s->stream));
      allow_split_now = false;
      TRY(launch(l, redo_stats));
      Control rc;
      std::vector<long long> rs((size_t)l.K * 4);
      HIPCHK(hipMemcpyAsync(&rc, s->ctl, sizeof(Control), hipMemcpyDeviceToHost, s->stream));
      HIPCHK(hipMemcpyAsync(rs.data(), redo_stats, rs.size() * sizeof(long long), hipMemcpyDeviceToHost, s->stream));
      HIPCHK(hipStreamSynchronize(s->stream));
      if (rc.failed)  // cannot happen: the same ticks on the same inputs gave finite rates for these iterations before
        return fail(MJHMC_ERR_HIP, "the recovery launch of a fused batch reported a non-finite rate of its own");
      // the tallies of the committed iterations of that launch come from the recovery run: in the failed launch a
      // workgroup that started after the failure may have skipped them
      for (int i = 0; i < l.K; ++i)
        for (int c = 0; c < 4; ++c) hs[(size_t)(l.i0 + i) * 4 + c] = rs[(size_t)i * 4 + c];
      xlive = l.xout;
      ++committed;
    }
  }
  return commit_call(s, hs, hc, done, attempts, committed, xlive, false, per_iter, n_done);
}

// A big dense batch (every sampler mode) is launched as TWO halves on two streams that run FREELY for the whole
// mjhmc_iterate call.
// Every kernel of the dense path is a persistent grid of one workgroup per CU, so a launch ends with a partial round
// (ProductOfT C3: 3125 tiles = 12.2 rounds of 256, then the inverse-L pass of ~250 tiles another partial one: 14 rounds
// where 13.2 would do) and the machine drains at every launch boundary.  Two independent halves fill each other's
// tails and never drain together.  Results cannot depend on the split (per-particle work, RNG keyed by the global
// particle id; tests/test_gpu_dense_parity.py::test_split_launches_equal_single_launches).
// What the halves must NOT do is meet a non-finite rate while one of them is iterations ahead of the other: the
// roll-back contract of mjhmc_iterate is "the state after `done` iterations", and with two state buffers an iteration
// f+1 of the half that ran ahead has overwritten its own state of iteration f-1.  So a multi-iteration call first
// copies the state aside (one device-to-device copy per call, < 0.2 % of it), and if the flag comes up it puts the copy
// back and reports that: mjhmc_iterate runs the call again the single-stream way, which stops at the failing iteration
// exactly as it always did.
// Measured: two free-running samplers of half the batch each gain 7.8 % (C3) / 5.5 % (C5) over one; halves that met at
// every iteration boundary (the first form of this) kept 1.5 % / 4 %: the dispatcher hands free CUs to the pending
// workgroups of the OLDEST dispatch first, a persistent grid of one workgroup per CU shuts out even a one-block memset
// until a workgroup exits, and a boundary at which both halves wait for each other is a drain again.
// (The elementwise compacted passes -- C4 -- were tried as 2 / 3 / 4 free-running parts the same way: 0.2727 ms per
// iteration unsplit, 0.2729 / 0.2744 / 0.310 split: their kernels leave room for each other already.)
static Parts dense_split(const mjhmc_sampler* s, bool allow_split) {
  const int cus = std::max(1, s->ctx->prop.multiProcessorCount);  // of THIS sampler's device
  const int ppt = s->en->is_sic() ? sic_particles_per_tile(s->en->sic_P) : 32;
  const int64_t unit = 64 * (int64_t)ppt;  // whole tiles and whole 64-particle row groups in every part
  const int64_t ntiles = (s->N + ppt - 1) / ppt;
  // A launch is a persistent grid of one workgroup per CU whose items (forward tiles + the inverse-L tiles of the R-movers)
  // take one trajectory time each: alone it ends in a partial round, and at a few hundred tiles that round is most of
  // the launch (C3 at 12 500 particles: 410 items = 1.6 rounds run as 2).  Two parts that never wait for each other fill
  // each other's partial rounds; below ~3/4 of a round of tiles there is nothing to fill.
  // (recording into ring slots changes nothing: iteration i reads slot i - 1 and writes slot i, part by part)
  int want = (allow_split && !test_env("MJHMC_NO_SPLIT") && 4 * ntiles >= 3 * (int64_t)cus) ? 2 : 1;
  if (want > 1)
    if (const char* np = test_env("MJHMC_SPLIT_PARTS")) want = std::max(1, std::min(kMaxDenseParts, std::atoi(np)));
  Parts parts;
  if (want > 1) {
    const int64_t len = (s->Npad / want) / unit * unit;
    if (len > 0 && len * (want - 1) < s->N) parts = Parts{want, len};
  }
  return parts;
}

// Iteration i of a dense batch, xin -> xout: one block of the tile kernels' arguments per part.  S the state rows, H the
// per-particle scalars, POT: ProductOfT; spec_out: where the F-movers' hand-over goes instead (MJHMC_NO_FSPEC), or nullptr
template <typename S, typename H, bool POT>
static void launch_dense_iteration(const mjhmc_sampler* s, const Parts& parts, const Replay& rp, void* spec_out,
                                   int ring_slot0, int i, const void* xin, void* xout) {
  using A = DenseJumpArgs<S, H, POT>;
  const int vi = (s->vcur + i) & 1, si = (s->scur + i) & 1;
  A d = jump_args<A>(s, i, vi, si, xin, xout, ring_slot0, s->stats + 4 * i);
  d.noise = rp.normal ? (const S*)s->noise : nullptr;
  d.rexp = rp.exp ? s->rexp : nullptr;
  d.runif = rp.unif ? s->runif : nullptr;
  if constexpr (A::kPot) {
    d.G_in = (const S*)s->Gbuf[vi];
    d.G_out = (S*)s->Gbuf[vi ^ 1];
  }
  d.Hwork = (H*)s->Hwork;
  d.cold_list = s->cold_list + (size_t)(i & 1) * s->Npad;          // iteration i reads list i & 1 ...
  d.next_list = s->cold_list + (size_t)((i + 1) & 1) * s->Npad;    // ... and writes the next iteration's
  d.Hspec_in = (const H*)s->Hspec[si];
  d.Hspec_out = (H*)(spec_out ? spec_out : s->Hspec[si ^ 1]);
  d.rescan = spec_out ? 1 : 0;
  for (int k = 0; k < parts.n; ++k) {
    A h = part_args(d, parts.start(k), parts.count(s, k), parts.npad(s, k), (size_t)s->sh.pitch, k, s->cold_list + 2 * s->Npad);
    h.ntiles = dense_ntiles(s, h.N, h.Npad);
    // the tile kernel of the energy and the state's type
    if constexpr (!POT) sic_launch_jump(h, s->en->sic_model(), parts.stream(s, k));
    else if constexpr (sizeof(S) == 8) pot64_launch_jump(h, s->en->pot_model(), parts.stream(s, k), s->en->pot_gen());
    else pot_launch_jump(h, s->en->pot_model(), parts.stream(s, k), s->en->pot_gen());
  }
}

// Dense batches: the tile kernels, as free-running parts on their own streams where dense_split says so.  *run_again: a
// non-finite rate came up while several parts ran a multi-iteration call freely -- the state the call started from has
// been put back, nothing is committed, and the caller runs the call again with allow_split = false.
template <typename T>
static int iterate_dense_parts(mjhmc_sampler* s, int n_iter, const Replay& rp, int ring_slot0, mjhmc_iter_stats* per_iter,
                               int* n_done, bool allow_split, bool* run_again) {
  *run_again = false;
  TRY(replay_alloc(s, rp));
  const Parts parts = dense_split(s, allow_split && !rp.any());
  if (parts.n > 1) {
    TRY(ensure_part_streams(s, parts.n));
    if (n_iter > 1) TRY(split_state_copy(s, false));
  }
  // test build, MJHMC_NO_FSPEC=1: nothing is handed on from an F move to the next iteration -- every cold particle's
  // inverse-L proposal is integrated, as the reference does (the A side of test_f_mover_shortcut_is_bit_identical)
  void* spec_out_override = nullptr;
  if (s->mode == MJHMC_MODE_MJHMC && test_env("MJHMC_NO_FSPEC")) {
    if (!s->Hspec_dump) HIPCHK(hipMalloc(&s->Hspec_dump, (size_t)s->Npad * ssize(s)));
    for (int i = 0; i < 2; ++i) HIPCHK(hipMemsetAsync(s->Hspec[i], 0xFF, (size_t)s->Npad * ssize(s), s->stream));
    spec_out_override = s->Hspec_dump;
  }
  // float64 state: the reference's arithmetic, float64 rows streamed through the tile kernel's epilogue (dense_pot64.hip);
  // SparseImageCode's state: bfloat16 (BASELINE.json configs[4]) or float32 (the reference's TensorFlow float32)
  decltype(&launch_dense_iteration<float, float, true>) launch;
  if constexpr (sizeof(T) == 8) launch = launch_dense_iteration<double, double, true>;
  else if (s->en->is_pot()) launch = launch_dense_iteration<float, float, true>;
  else if (s->dtype == MJHMC_BF16) launch = launch_dense_iteration<__bf16, float, false>;
  else launch = launch_dense_iteration<float, float, false>;

  std::vector<void*> xout(n_iter);
  TRY(begin_call(s, n_iter));
  if (ring_slot0 >= 0) TRY(move_out_of_ring(s, ring_slot0, 1));   // (iteration i reads slot i - 1 and writes slot i)
  void* xin = s->Xcur;
  for (int i = 0; i < n_iter; ++i) {
    void* const xo = xout[i] = iteration_out(s, ring_slot0, i, xin);
    TRY(replay_upload(s, rp, i));
    TRY(debug_poison(s, i, (s->scur + i) & 1, parts));
    if (parts.n > 1 && i == 0) {  // the other parts' streams start from everything the first has been given so far
      HIPCHK(hipEventRecord(s->ev_fork, s->stream));
      for (int k = 1; k < parts.n; ++k) HIPCHK(hipStreamWaitEvent(parts.stream(s, k), s->ev_fork, 0));
    }
    launch(s, parts, rp, spec_out_override, ring_slot0, i, xin, xo);
    if (parts.n > 1 && i + 1 == n_iter) {  // the read-back follows every part
      for (int k = 1; k < parts.n; ++k) {
        HIPCHK(hipEventRecord(s->part_events[(size_t)k - 1], parts.stream(s, k)));
        HIPCHK(hipStreamWaitEvent(s->stream, s->part_events[(size_t)k - 1], 0));
      }
    }
    HIPCHK(hipGetLastError());
    TRY(dl_done(s, ring_slot0, i, xo, parts));
    xin = xo;
  }
  Control hc;
  std::vector<long long> hs((size_t)n_iter * 4);
  TRY(end_call(s, (size_t)n_iter, &hc, hs.data()));

  if (hc.failed && parts.n > 1 && n_iter > 1) {
    // a non-finite rate somewhere in the free-running parts: back to the state the call started from; the run on one
    // stream that follows stops at the failing iteration with the state, tallies and RNG position of a call that
    // was never split (nothing of this attempt has been committed: parities, Xcur and the tick are still the call's)
    TRY(split_state_copy(s, true));
    HIPCHK(hipStreamSynchronize(s->stream));
    *run_again = true;
    return 0;
  }
  return commit_iterations(s, hs, hc, n_iter, xout, per_iter, n_done);
}

// The compacted passes of the elementwise energies (step_kernel.hpp, mjhmc_step_kernel): the iteration's trajectories --
// the L proposals and, beside them, the inverse-L proposals of the listed cold caches --, then its jump process with a
// lane per particle, which finishes the movers and hands them on as the next iteration's list (only the first iteration
// of a call scans the cache, and not even that one when the list was `carried` over from the call before).
// (Measured and dropped: the batch as two halves on two free-running streams, 0.2551 ms against 0.2623 for C4 on the
// device but more launches than the host issues in that time; and the halves staggered by half an iteration inside
// ONE launch sequence -- every launch the trajectories of one half beside the jump process of the other --,
// 0.2586 ms: the trajectories keep the vector pipe half busy themselves, there is no idle unit to hide the jump
// process under.  DESIGN.md section 8c.)
template <typename T>
static int iterate_compact_t(mjhmc_sampler* s, int n_iter, int ring_slot0, mjhmc_iter_stats* per_iter, int* n_done,
                             bool carried) {
  if (!s->flf_list) {
    HIPCHK(hipMalloc((void**)&s->flf_list, (size_t)2 * s->Npad * sizeof(int)));   // two lists: iterations alternate
    HIPCHK(hipMalloc(&s->Hpre, (size_t)2 * s->Npad * ssize(s)));
  }
  // (flf_counts: a counter per iteration of the call + the one the last iteration's movers go to -- stats_cap + 1 of them
  // in the call block, zeroed with it)
  std::vector<void*> xout(n_iter);
  TRY(begin_call(s, n_iter));
  if (ring_slot0 >= 0) TRY(move_out_of_ring(s, ring_slot0, 1));   // (iteration i reads slot i - 1 and writes slot i)
  void* xin = s->Xcur;
  // the two lists alternate; a call that follows a committed call of this path starts from the list that call's last
  // jump process left (the host knows its length) instead of scanning H_flf
  const int par0 = carried ? s->list_par : 0;
  for (int i = 0; i < n_iter; ++i) {
    void* const xo = xout[i] = iteration_out(s, ring_slot0, i, xin);
    const int vi = (s->vcur + i) & 1, si = (s->scur + i) & 1;
    TRY(debug_poison(s, i, si, Parts{}));
    const JumpArgs<T> a = jump_args<JumpArgs<T>>(s, i, vi, si, xin, xo, ring_slot0, s->stats + 4 * i);
    const TrajArgs<T> ta = traj_args(a, (T*)s->Hpre, s->flf_list + (size_t)((par0 + i) & 1) * s->Npad,
                                     (carried && i == 0) ? nullptr : s->flf_counts + i, s->list_count);
    const JumpDecideArgs<T> da = decide_args(a, ta.Hwork, s->flf_list + (size_t)((par0 + i + 1) & 1) * s->Npad, s->flf_counts + i + 1);
    if (i == 0 && !carried) {
      const dim3 list_grid((unsigned)((s->N + kColdChunk - 1) / kColdChunk));
      hipLaunchKernelGGL(compact_list_kernel<ColdCache<T>>, list_grid, dim3(1024), 0, s->stream,
                         ColdCache<T>{a.Hflf_in, (T*)s->Hpre + s->Npad}, s->N, s->ctl, s->flf_list, s->flf_counts);
    }
    TRY(with_elementwise_energy(s->en->ep.kind, [&](auto en) {
      en.step(&ta, nullptr, s->en->ep, s->sh.E, s->stream);
      en.step(nullptr, &da, s->en->ep, s->sh.E, s->stream);
    }));
    HIPCHK(hipGetLastError());
    TRY(dl_done(s, ring_slot0, i, xo, Parts{}));
    xin = xo;
  }
  Control hc;
  std::vector<long long> hs((size_t)n_iter * 4);
  std::vector<int> hcnt((size_t)n_iter + 1);   // (+ the list the last iteration's movers went to)
  TRY(end_call(s, (size_t)n_iter, &hc, hs.data(), hcnt.data(), n_iter + 1));
  if (carried) hcnt[0] = s->list_count;
  for (int i = 0; i < n_iter; ++i) hs[4 * (size_t)i + 3] = hcnt[(size_t)i];   // the cold tallies are the list lengths
  if (!hc.failed) {   // the next call's list
    s->list_par = (par0 + n_iter) & 1;
    s->list_count = hcnt[(size_t)n_iter];
    s->list_valid = true;
  }
  return commit_iterations(s, hs, hc, n_iter, xout, per_iter, n_done);
}

// One jump launch per iteration: the elementwise energies outside the other schedules, every replayed call of them, and
// the user-expression energies (float64 only).
template <typename T>
static int iterate_plain_t(mjhmc_sampler* s, int n_iter, const Replay& rp, int ring_slot0, mjhmc_iter_stats* per_iter,
                           int* n_done) {
  TRY(replay_alloc(s, rp));
  std::vector<void*> xout(n_iter);
  TRY(begin_call(s, n_iter));
  if (ring_slot0 >= 0) TRY(move_out_of_ring(s, ring_slot0, 1));   // (iteration i reads slot i - 1 and writes slot i)
  void* xin = s->Xcur;
  const bool user = s->en->is_user();
  for (int i = 0; i < n_iter; ++i) {
    void* const xo = xout[i] = iteration_out(s, ring_slot0, i, xin);
    const int vi = (s->vcur + i) & 1, si = (s->scur + i) & 1;
    TRY(replay_upload(s, rp, i));
    TRY(debug_poison(s, i, si, Parts{}));
    JumpArgs<T> a = jump_args<JumpArgs<T>>(s, i, vi, si, xin, xo, ring_slot0, s->stats + 4 * i);
    a.noise = rp.normal ? (const T*)s->noise : nullptr;
    a.rexp = rp.exp ? s->rexp : nullptr;
    a.runif = rp.unif ? s->runif : nullptr;
    if (user) {
      if constexpr (sizeof(T) == 8) TRY(user_launch_jump(s->en, a, s->stream));
    } else {
      TRY(with_elementwise_energy(s->en->ep.kind, [&](auto en) { en.jump(a, s->en->ep, s->sh.E, s->stream); }));
    }
    HIPCHK(hipGetLastError());
    TRY(dl_done(s, ring_slot0, i, xo, Parts{}));
    xin = xo;
  }
  Control hc;
  std::vector<long long> hs((size_t)n_iter * 4);
  TRY(end_call(s, (size_t)n_iter, &hc, hs.data()));
  return commit_iterations(s, hs, hc, n_iter, xout, per_iter, n_done);
}

template <typename T>
static int run_schedule(mjhmc_sampler* s, Schedule schedule, bool carried, int n_iter, const Replay& rp, int ring_slot0,
                        mjhmc_iter_stats* per_iter, int* n_done) {
  switch (schedule) {
    case Schedule::Fused: return iterate_fused_t<T>(s, n_iter, ring_slot0, per_iter, n_done);
    case Schedule::DenseParts: {
      bool run_again = false;
      TRY(iterate_dense_parts<T>(s, n_iter, rp, ring_slot0, per_iter, n_done, true, &run_again));
      if (!run_again) return 0;
      TRY(dl_restart(s));   // (mjhmc_iterate_download: nothing the first run handed to the download survives it)
      return iterate_dense_parts<T>(s, n_iter, rp, ring_slot0, per_iter, n_done, false, &run_again);
    }
    case Schedule::Compact: return iterate_compact_t<T>(s, n_iter, ring_slot0, per_iter, n_done, carried);
    default: return iterate_plain_t<T>(s, n_iter, rp, ring_slot0, per_iter, n_done);
  }
}

static ScheduleInputs schedule_inputs(const mjhmc_sampler* s, int n_iter, const Replay& rp) {
  const mjhmc_energy* e = s->en;
  ScheduleInputs in;
  in.family = e->is_dense() ? EnergyFamily::Dense
              : e->is_user() ? EnergyFamily::User
              : (e->ep.kind == MJHMC_E_ISO_GAUSS || e->ep.kind == MJHMC_E_DIAG_GAUSS) ? EnergyFamily::Gaussian
              : fused_rows(s) ? EnergyFamily::Rows
                              : EnergyFamily::Other;
  in.wide = s->sh.wide;
  in.pot64_tile = e->is_pot() && !e->pot_big() && !e->lin_tall() && !e->lin_wide() && !s->sh.round32;
  in.N = s->N;
  in.D = s->D;
  in.logG = s->sh.logG;
  in.mjhmc_mode = s->mode == MJHMC_MODE_MJHMC;
  in.L = s->L;
  in.n_iter = n_iter;
  in.replay = rp.any();
  in.no_fuse = test_env("MJHMC_NO_FUSE") != nullptr;
  in.no_compact = test_env("MJHMC_NO_COMPACT") != nullptr;
  if (const char* fb = test_env("MJHMC_FUSE_BELOW")) {
    in.fuse_below_set = true;
    in.fuse_below = std::atoll(fb);
  }
  in.pot64_multipass = test_env("MJHMC_POT64_MULTIPASS") != nullptr;
  return in;
}

extern "C" {

int mjhmc_iterate(mjhmc_sampler* s, int n_iter, const double* replay_normal, const double* replay_exp,
                  const double* replay_unif, int ring_slot0, mjhmc_iter_stats* per_iter, int* n_done) {
  if (!s) return fail(MJHMC_ERR_INVALID, "sampler is NULL");
  if (n_iter < 1) return fail(MJHMC_ERR_INVALID, "n_iter must be >= 1");
  if (s->mode == MJHMC_MODE_CONTROL) {
    if ((replay_normal == nullptr) != (replay_unif == nullptr) || replay_exp)
      return fail(MJHMC_ERR_INVALID, "CONTROL replay takes replay_normal and replay_unif together");
  } else if ((replay_normal == nullptr) != (replay_exp == nullptr) || replay_unif) {
    return fail(MJHMC_ERR_INVALID, "jump-process replay takes replay_normal and replay_exp together");
  }
  if (ring_slot0 >= 0 && (!s->ring || ring_slot0 + n_iter > s->ring_slots))
    return fail(MJHMC_ERR_INVALID, "ring slots out of range (call mjhmc_ring_alloc)");
  if (s->en->is_host())
    return fail(MJHMC_ERR_UNSUPPORTED, "a host-evaluated energy is driven step by step: mjhmc_traj_begin / _step / _finish");
  HIPCHK(hipSetDevice(s->ctx->device));
  const Replay rp{replay_normal, replay_exp, replay_unif};
  const Schedule schedule = select_schedule(schedule_inputs(s, n_iter, rp));
  const bool carried = s->list_valid && !test_env("MJHMC_NO_LIST_CARRY");   // (every schedule consumes it; only the compacted passes renew it)
  s->list_valid = false;
  if (schedule == Schedule::Multipass) {
    const int rc = multipass_iterate(s, n_iter, replay_normal, replay_exp, replay_unif, ring_slot0, per_iter, n_done);
    if (rc == 0) TRY(drop_spec(s));   // (that path neither reads nor writes the F-movers' hand-over: nothing of it is valid afterwards)
    return rc;
  }
  return s->dtype == MJHMC_F64 ? run_schedule<double>(s, schedule, carried, n_iter, rp, ring_slot0, per_iter, n_done)
                               : run_schedule<float>(s, schedule, carried, n_iter, rp, ring_slot0, per_iter, n_done);
}

int mjhmc_iterate_download(mjhmc_sampler* s, int n_iter, int ring_slot0, double* host_out, int64_t n_total, int64_t k0,
                           mjhmc_iter_stats* per_iter, int* n_done) {
  if (!s || !host_out || n_iter < 1) return fail(MJHMC_ERR_INVALID, "bad argument");
  if (ring_slot0 < 0 || !s->ring || ring_slot0 + n_iter > s->ring_slots)
    return fail(MJHMC_ERR_INVALID, "ring slots out of range (call mjhmc_ring_alloc)");
  if (k0 < 0 || k0 + n_iter > n_total) return fail(MJHMC_ERR_INVALID, "time indices [k0, k0 + n_iter) outside the host array");
  HIPCHK(hipSetDevice(s->ctx->device));
  if (!s->dl_stream) {
    // the re-tile kernel of a finished slot should get the first CUs a finishing workgroup of the persistent grids gives up
    int lo = 0, hi = 0;
    HIPCHK(hipDeviceGetStreamPriorityRange(&lo, &hi));
    HIPCHK(hipStreamCreateWithPriority(&s->dl_stream, hipStreamNonBlocking, hi));
  }
  const size_t elems = (size_t)s->D * s->N;
  // staging in the host layout: a slot per iteration of the call where the device has the room (the iterations then
  // re-tile their own output, see dl_done), else one slot the worker re-tiles into
  if (s->dl_stage_elems < (size_t)n_iter * elems) {
    double* big = nullptr;
    if (hipMalloc((void**)&big, (size_t)n_iter * elems * sizeof(double)) == hipSuccess) {
      if (s->dl_stage) HIPCHK(hipFree(s->dl_stage));
      s->dl_stage = big;
      s->dl_stage_elems = (size_t)n_iter * elems;
    } else {
      (void)hipGetLastError();
      if (s->dl_stage_elems < elems) {
        if (s->dl_stage) HIPCHK(hipFree(s->dl_stage));
        s->dl_stage = nullptr;
        s->dl_stage_elems = 0;
        HIPCHK(hipMalloc((void**)&s->dl_stage, elems * sizeof(double)));
        s->dl_stage_elems = elems;
      }
    }
  }
  TRY(ensure_pipe_pair(s->dl_pin, s->dl_ev));
  DlSession d;
  d.ev.resize((size_t)n_iter);
  d.retiled.assign((size_t)n_iter, 0);
  d.n_iter = n_iter;
  d.ring_slot0 = ring_slot0;
  d.host = host_out;
  d.n_total = n_total;
  d.k0 = k0;
  s->dl = &d;
  std::thread worker(dl_worker, s, &d);
  int done = 0;
  const int rc = mjhmc_iterate(s, n_iter, nullptr, nullptr, nullptr, ring_slot0, per_iter, &done);
  d.launched.store(true, std::memory_order_release);
  worker.join();
  s->dl = nullptr;
  int rc2 = d.rc;
  if (rc2) (void)fail(rc2, d.err);
  // what the worker did not bring over (a launch path that marks nothing; a re-run after a failure): plainly, now
  if (!rc && !rc2) {
    HIPCHK(hipStreamSynchronize(s->dl_stream));
    for (int i = d.downloaded.load(); i < done && !rc2; ++i) rc2 = dl_download_slot(s, &d, i);
  }
  dl_destroy_events(&d);
  if (n_done) *n_done = done;
  return rc ? rc : rc2;
}

}  // extern "C"
