// Order-preserving fair sample paths of the jump samplers on a uniform time grid, on the device.
//
// The fair object of a jump sampler is the continuous-time process x_p(t): chain p sits in state k for its holding time
// w_k.  Weighting states by w (estimators.hip, chainstats.hip, histograms.hip) makes pooled statistics fair but loses the
// time order; recording every state once (sample(resample=False)) keeps the order and is biased.  Sampling x_p(t) at
// t_j = j * dt keeps both: an array (ndims, nbatch, n_grid) whose columns follow the target and whose last axis is time --
// what autocor_from_ring (autocor.hip) takes.
//
// Definition (the contract; include/mjhmc_hip.h: mjhmc_timegrid_accumulate).  Per chain p < N a clock T[p] (float64, 0 at
// create) and a cursor j[p] (int32, 0 at create); for the states of ring slots x_slot0 + k, k = 0 .. n - 1 ascending:
//   w  = dwell[w_slot0 + k][p]                       (unit weights: w = 1.0)
//   Tn = T[p] + w                                    one rounded float64 addition
//   while j[p] < n_grid and (double)j[p] * dt < Tn:  one rounded multiplication
//       grid[j[p]][p][:] = x[x_slot0 + k][p][:];  j[p] += 1
//   T[p] = Tn
// Grid point t_j takes the state with T_k <= t_j < T_{k+1}; a state of zero holding time is never emitted, one that spans
// several grid points is emitted for each.  The clock is a sequential sum from the stored value, so grid, T and j do not
// depend on how a run is cut into blocks and are bit-identical from run to run.  There is no floating-point atomic in this
// file.  Rows p >= N of the sample ring, the dwell ring and the grid are neither read nor written.
//
// The grid ring has the sample ring's slot layout and dtype ([Npad][pitch], stored elements copied verbatim), so one
// kernel serves float64, float32 and bfloat16 state: it moves 16-byte chunks and never looks inside them.
//
// Two launches per block, one stream:
//   tg_check_kernel   over the n * N weights: a flag for a weight that is not finite or is negative
//   tg_pass_kernel    the pass; returns at its top when the flag is up, so a refused block changes nothing
// The pass has the access shape of the chain pass (chainstats.hip): lane g owns bytes [16 g, 16 g + 16) of a slot matrix
// (2 / 4 / 8 elements of one chain's row, 1 KB per wave instruction).  It reads its chain's T and j, walks the block's
// slots source-driven -- the chunk of slot k and its weight loaded with kSlotsInFlight slots in flight, then stored to
// every grid slot of the state's range, an execution-masked loop of about one store per state at dt = mean holding time --
// and the lane of the row's first chunk writes T and j once.  Clocks and cursors are double-buffered: the lanes of one row
// may sit in several waves, and the first lane's write must not reach a lane that has not read yet.  The caller swaps the
// buffers after an accepted block.  Every source slot is read at most once (a chain whose grid is full skips the chunks and
// only adds the weights), the writes are exactly the emitted rows.  No LDS, no cross-lane traffic, no atomics.
// HBM bytes of a call: n slots + n dwell vectors read, the emitted rows written, 24 N bytes of clocks and cursors.
#include "timegrid.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../include/mjhmc_hip.h"
#include "handles.hpp"
#include "lagcov.hpp"
#include "ring_rows.hpp"

namespace {

// any weight among w[k * Npad + p], k < n, p < N that is not finite or is negative
__global__ __launch_bounds__(256) void tg_check_kernel(const double* __restrict__ w, int64_t Npad, int64_t N, int n,
                                                       int* __restrict__ bad) {
  int flag = 0;
  for (int k = blockIdx.y; k < n; k += gridDim.y) {
    const double* wk = w + (size_t)k * Npad;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < N; p += (int64_t)gridDim.x * 256) {
      const double v = wk[p];
      if (!(v >= 0.0 && finite_f64(v))) flag = 1;
    }
  }
  if (flag) *bad = 1;
}

// lane g: 16-byte chunk g of every slot = chain g / chunks, chunk g % chunks of its row
__global__ __launch_bounds__(256) void tg_pass_kernel(const uint4* __restrict__ base, const double* __restrict__ w, int64_t Npad,
                                                      int64_t N, int n, int chunks, double dt, int n_grid,
                                                      uint4* __restrict__ grid, const double* __restrict__ T_in,
                                                      const int* __restrict__ j_in, double* __restrict__ T_out,
                                                      int* __restrict__ j_out, const int* __restrict__ bad) {
  if (*bad) return;
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t total = N * chunks;
  if (g >= total) return;
  // (one division per lane; the 32-bit form where the launch allows it)
  const int64_t p = total <= 0xFFFFFFFFll ? (int64_t)((uint32_t)g / (uint32_t)chunks) : g / chunks;
  double t = T_in[p];
  int j = j_in[p];
  const size_t slot_chunks = (size_t)Npad * chunks;
  const uint4* const x0 = base + g;
  const double* const w0 = w ? w + p : nullptr;
  uint4* const g0 = grid + g;
  for (int k0 = 0; k0 < n; k0 += kSlotsInFlight) {
    uint4 q[kSlotsInFlight];
    double wt[kSlotsInFlight];
    const bool open = j < n_grid;   // (a full grid takes no more rows: only the clock goes on)
#pragma unroll
    for (int u = 0; u < kSlotsInFlight; ++u) {
      wt[u] = 1.0;
      q[u] = make_uint4(0u, 0u, 0u, 0u);
      if (k0 + u < n) {
        if (open) q[u] = x0[(size_t)(k0 + u) * slot_chunks];
        if (w0) wt[u] = w0[(size_t)(k0 + u) * Npad];
      }
    }
#pragma unroll
    for (int u = 0; u < kSlotsInFlight; ++u) {
      if (k0 + u < n) {
        const double tn = t + wt[u];
        while (j < n_grid && (double)j * dt < tn) {
          g0[(size_t)j * slot_chunks] = q[u];
          ++j;
        }
        t = tn;
      }
    }
  }
  if (g == p * chunks) {   // (every lane of the row holds the same clock and cursor; the first one's)
    T_out[p] = t;
    j_out[p] = j;
  }
}

// ext[0] = max_p (n_grid - j[p]), ext[1] = max_p j[p]: integers, whatever the order
__global__ __launch_bounds__(256) void tg_extent_kernel(const int* __restrict__ j, int64_t N, int n_grid, int* __restrict__ ext) {
  __shared__ int sm[2][256];
  int lo = n_grid, hi = 0;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < N; p += (int64_t)gridDim.x * 256) {
    const int v = j[p];
    lo = min(lo, v);
    hi = max(hi, v);
  }
  sm[0][threadIdx.x] = lo;
  sm[1][threadIdx.x] = hi;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      sm[0][threadIdx.x] = min(sm[0][threadIdx.x], sm[0][threadIdx.x + o]);
      sm[1][threadIdx.x] = max(sm[1][threadIdx.x], sm[1][threadIdx.x + o]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    atomicMax(&ext[0], n_grid - sm[0][0]);
    atomicMax(&ext[1], sm[1][0]);
  }
}

}  // namespace

int timegrid_accumulate(hipStream_t st, const RingView& r, int n, const double* w, double dt, int n_grid, void* grid,
                        const double* T_in, const int* j_in, double* T_out, int* j_out, int* bad, std::string& err) {
  if (w) {
    const unsigned bx = (unsigned)std::min<int64_t>(1024, (r.N + 255) / 256);
    hipLaunchKernelGGL(tg_check_kernel, dim3(bx, (unsigned)std::min(n, 1024)), dim3(256), 0, st, w, r.Npad, r.N, n, bad);
  }
  const int vec = r.dtype == MJHMC_F64 ? 2 : (r.dtype == MJHMC_F32 ? 4 : 8);
  const int chunks = r.pitch / vec;   // (a row is whole 16-byte chunks: mjhmc_timegrid_create checked)
  const int64_t lanes = r.N * chunks;
  hipLaunchKernelGGL(tg_pass_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, (const uint4*)r.base, w, r.Npad,
                     r.N, n, chunks, dt, n_grid, (uint4*)grid, T_in, j_in, T_out, j_out, bad);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    err = std::string("time-grid pass: ") + hipGetErrorString(e);
    return MJHMC_ERR_HIP;
  }
  return 0;
}

int timegrid_extent(hipStream_t st, const int* j, int64_t N, int n_grid, int* ext, std::string& err) {
  const unsigned bx = (unsigned)std::max<int64_t>(1, std::min<int64_t>(256, (N + 255) / 256));
  hipLaunchKernelGGL(tg_extent_kernel, dim3(bx), dim3(256), 0, st, j, N, n_grid, ext);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    err = std::string("time-grid extent: ") + hipGetErrorString(e);
    return MJHMC_ERR_HIP;
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// The handle of the C ABI (include/mjhmc_hip.h: mjhmc_timegrid_*)
// ---------------------------------------------------------------------------------------------------------------------
struct mjhmc_timegrid {
  mjhmc_sampler* s = nullptr;
  int n_grid = 0;
  double dt = 0.0;
  // the sampler's shape at create: the grid ring has it
  int64_t N = 0, Npad = 0;
  int D = 0, pitch = 0, dtype = 0;
  size_t slot_bytes = 0;
  char* grid = nullptr;                    // [n_grid][Npad][pitch], the state's own type
  double* T[2] = {nullptr, nullptr};       // [Npad] clocks; T[cur] is the current one
  int* j[2] = {nullptr, nullptr};          // [Npad] cursors
  int cur = 0;
  int* flags = nullptr;                    // bad, then the two words of the extent
  int* bad() const { return flags; }
  int* ext() const { return flags + 1; }
  RingView view(int slot0) const { return RingView{grid + (size_t)slot0 * slot_bytes, dtype, Npad, N, D, pitch}; }
};

static void timegrid_free(mjhmc_timegrid* tg) {
  for (void* p : {(void*)tg->grid, (void*)tg->T[0], (void*)tg->T[1], (void*)tg->j[0], (void*)tg->j[1], (void*)tg->flags})
    if (p) (void)hipFree(p);
  delete tg;
}

void timegrid_free_all(mjhmc_sampler* s) {
  for (mjhmc_timegrid* tg : s->timegrids) timegrid_free(tg);
  s->timegrids.clear();
}

static int timegrid_zero(mjhmc_timegrid* tg, bool grid_too) {
  mjhmc_sampler* s = tg->s;
  if (grid_too) HIPCHK(hipMemsetAsync(tg->grid, 0, (size_t)tg->n_grid * tg->slot_bytes, s->stream));
  for (int b = 0; b < 2; ++b) {
    HIPCHK(hipMemsetAsync(tg->T[b], 0, (size_t)tg->Npad * sizeof(double), s->stream));
    HIPCHK(hipMemsetAsync(tg->j[b], 0, (size_t)tg->Npad * sizeof(int), s->stream));
  }
  HIPCHK(hipMemsetAsync(tg->flags, 0, 3 * sizeof(int), s->stream));
  tg->cur = 0;
  return 0;
}

// covered = min_p j[p], max_filled = max_p j[p] (one small launch, two integers back)
static int timegrid_progress(mjhmc_timegrid* tg, int* covered, int* max_filled) {
  mjhmc_sampler* s = tg->s;
  HIPCHK(hipMemsetAsync(tg->ext(), 0, 2 * sizeof(int), s->stream));
  std::string err;
  const int rc = timegrid_extent(s->stream, tg->j[tg->cur], tg->N, tg->n_grid, tg->ext(), err);
  if (rc) return mjhmc_fail(rc, err);
  int h[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(h, tg->ext(), sizeof(h), hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  *covered = tg->n_grid - h[0];
  *max_filled = h[1];
  return 0;
}

static int timegrid_check_slots(const mjhmc_timegrid* tg, int slot0, int n, int limit, const char* what) {
  if (slot0 < 0 || n < 1 || (int64_t)slot0 + n > limit)
    return mjhmc_fail(MJHMC_ERR_INVALID, "grid slots [" + std::to_string(slot0) + ", " + std::to_string((int64_t)slot0 + n) +
                                             ") are outside the " + what + " of " + std::to_string(limit));
  return 0;
}

extern "C" {

int mjhmc_timegrid_create(mjhmc_sampler* s, int n_grid, double dt, mjhmc_timegrid** out) {
  if (!s || !out) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  if (n_grid < 1) return mjhmc_fail(MJHMC_ERR_INVALID, "n_grid must be >= 1, got " + std::to_string(n_grid));
  if (!std::isfinite(dt) || !(dt > 0.0)) return mjhmc_fail(MJHMC_ERR_INVALID, "dt must be finite and positive");
  if (!s->ring) return mjhmc_fail(MJHMC_ERR_INVALID, "the sampler has no sample ring yet (call mjhmc_ring_alloc first)");
  // the pass moves a slot in 16-byte chunks: rows must be whole chunks
  const int vec = s->dtype == MJHMC_F64 ? 2 : (s->dtype == MJHMC_F32 ? 4 : 8);
  if (s->sh.esize * vec != 16 || s->sh.pitch % vec != 0)
    return mjhmc_fail(MJHMC_ERR_UNSUPPORTED, "the sampler's rows are not whole 16-byte chunks of its state type");
  HIPCHK(hipSetDevice(s->ctx->device));
  mjhmc_timegrid* tg = new mjhmc_timegrid();
  tg->s = s;
  tg->n_grid = n_grid;
  tg->dt = dt;
  tg->N = s->N;
  tg->Npad = s->Npad;
  tg->D = s->D;
  tg->pitch = s->sh.pitch;
  tg->dtype = s->dtype;
  tg->slot_bytes = mat_bytes(s);
  const size_t grid_bytes = (size_t)n_grid * tg->slot_bytes;
  hipError_t e = hipMalloc((void**)&tg->grid, grid_bytes);
  for (int b = 0; b < 2; ++b) {
    if (e == hipSuccess) e = hipMalloc((void**)&tg->T[b], (size_t)tg->Npad * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&tg->j[b], (size_t)tg->Npad * sizeof(int));
  }
  if (e == hipSuccess) e = hipMalloc((void**)&tg->flags, 3 * sizeof(int));
  if (e != hipSuccess) {
    const size_t mb = tg->slot_bytes;
    timegrid_free(tg);
    (void)hipGetLastError();
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    char msg[320];
    std::snprintf(msg, sizeof(msg), "a time grid of %d slots x %.3f GB = %.1f GB does not fit the device (%.1f GB free of %.1f GB): "
                  "take fewer grid points or a larger dt -- nothing was allocated",
                  n_grid, mb / 1e9, (double)grid_bytes / 1e9, free_b / 1e9, total_b / 1e9);
    return mjhmc_fail(MJHMC_ERR_HIP, msg);
  }
  // (on the sampler's stream, then synchronised: as mjhmc_ring_alloc zeroes its ring)
  int rc = timegrid_zero(tg, true);
  if (rc == 0 && hipStreamSynchronize(s->stream) != hipSuccess) rc = mjhmc_fail(MJHMC_ERR_HIP, "time grid: zeroing failed");
  if (rc) {
    timegrid_free(tg);
    (void)hipGetLastError();
    return rc;
  }
  s->timegrids.push_back(tg);
  *out = tg;
  return 0;
}

int mjhmc_timegrid_destroy(mjhmc_timegrid* tg) {
  if (!tg) return 0;
  mjhmc_sampler* s = tg->s;
  (void)hipSetDevice(s->ctx->device);
  if (s->stream) (void)hipStreamSynchronize(s->stream);
  s->timegrids.erase(std::remove(s->timegrids.begin(), s->timegrids.end(), tg), s->timegrids.end());
  timegrid_free(tg);
  return 0;
}

int mjhmc_timegrid_reset(mjhmc_timegrid* tg) {
  if (!tg) return mjhmc_fail(MJHMC_ERR_INVALID, "timegrid is NULL");
  HIPCHK(hipSetDevice(tg->s->ctx->device));
  return timegrid_zero(tg, true);
}

int mjhmc_timegrid_accumulate(mjhmc_timegrid* tg, int x_slot0, int n, int w_slot0) {
  if (!tg) return mjhmc_fail(MJHMC_ERR_INVALID, "timegrid is NULL");
  mjhmc_sampler* s = tg->s;
  if (s->N != tg->N || s->Npad != tg->Npad || s->sh.pitch != tg->pitch || s->dtype != tg->dtype)
    return mjhmc_fail(MJHMC_ERR_INVALID, "the sampler's particles, row pitch or state type changed after mjhmc_timegrid_create");
  if (n < 1) return mjhmc_fail(MJHMC_ERR_INVALID, "n must be >= 1");
  if (x_slot0 < 0 || (int64_t)x_slot0 + n > s->ring_slots)
    return mjhmc_fail(MJHMC_ERR_INVALID, "state slots [" + std::to_string(x_slot0) + ", " + std::to_string((int64_t)x_slot0 + n) +
                                             ") are outside the ring of " + std::to_string(s->ring_slots));
  if (w_slot0 < -1 || (w_slot0 >= 0 && (int64_t)w_slot0 + n > s->ring_slots))
    return mjhmc_fail(MJHMC_ERR_INVALID, "dwell slots [" + std::to_string(w_slot0) + ", " + std::to_string((int64_t)w_slot0 + n) +
                                             ") are outside the ring of " + std::to_string(s->ring_slots) +
                                             " (-1 asks for unit weights)");
  HIPCHK(hipSetDevice(s->ctx->device));
  const double* w = w_slot0 >= 0 ? s->dwell_ring + (size_t)w_slot0 * s->Npad : nullptr;
  const RingView src{(const char*)s->ring + (size_t)x_slot0 * tg->slot_bytes, tg->dtype, tg->Npad, tg->N, tg->D, tg->pitch};
  const int in = tg->cur, o = 1 - tg->cur;
  std::string err;
  const int rc = timegrid_accumulate(s->stream, src, n, w, tg->dt, tg->n_grid, tg->grid, tg->T[in], tg->j[in], tg->T[o], tg->j[o],
                                     tg->bad(), err);
  if (rc) return mjhmc_fail(rc, err);
  if (w) {   // (unit weights raise no flag: nothing to wait for)
    int bad = 0;
    HIPCHK(hipMemcpyAsync(&bad, tg->bad(), sizeof(int), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    if (bad) {
      HIPCHK(hipMemsetAsync(tg->bad(), 0, sizeof(int), s->stream));
      return mjhmc_fail(MJHMC_ERR_NONFINITE, "a dwelling time in dwell slots [" + std::to_string(w_slot0) + ", " +
                                                 std::to_string(w_slot0 + n) +
                                                 ") is not finite or is negative (a state whose total jump rate is zero "
                                                 "leaves an infinite one): grid, clocks and cursors are as before the call");
    }
  }
  tg->cur = o;
  return 0;
}

int mjhmc_timegrid_progress(mjhmc_timegrid* tg, int* covered, int* max_filled) {
  if (!tg || !covered || !max_filled) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  HIPCHK(hipSetDevice(tg->s->ctx->device));
  return timegrid_progress(tg, covered, max_filled);
}

int mjhmc_timegrid_read_clocks(mjhmc_timegrid* tg, double* T_host, int32_t* j_host) {
  if (!tg) return mjhmc_fail(MJHMC_ERR_INVALID, "timegrid is NULL");
  mjhmc_sampler* s = tg->s;
  HIPCHK(hipSetDevice(s->ctx->device));
  if (T_host) HIPCHK(hipMemcpyAsync(T_host, tg->T[tg->cur], (size_t)tg->N * sizeof(double), hipMemcpyDeviceToHost, s->stream));
  if (j_host) HIPCHK(hipMemcpyAsync(j_host, tg->j[tg->cur], (size_t)tg->N * sizeof(int), hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  return 0;
}

int mjhmc_timegrid_read(mjhmc_timegrid* tg, int slot0, int n, int stacked, double* host_out) {
  if (!tg || !host_out) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  TRY(timegrid_check_slots(tg, slot0, n, tg->n_grid, "grid"));
  mjhmc_sampler* s = tg->s;
  HIPCHK(hipSetDevice(s->ctx->device));
  const int64_t N = tg->N;
  const size_t total = (size_t)tg->D * N * n;
  TRY(ensure_stage(s, total));
  const char* base = tg->grid + (size_t)slot0 * tg->slot_bytes;
  for (int k = 0; k < n; ++k) {
    const char* slot = base + (size_t)k * tg->slot_bytes;
    if (!stacked)
      TRY(download_cols(s, slot, nullptr, N, host_out, total, (int64_t)n * N, 1, (int64_t)k * N, k == n - 1));
    else
      TRY(download_cols(s, slot, nullptr, N, host_out, total, N * n, n, k, k == n - 1));
  }
  return 0;
}

int mjhmc_timegrid_autocor(mjhmc_timegrid* tg, int slot0, int n, int linear, double* host_out) {
  if (!tg || !host_out) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  mjhmc_sampler* s = tg->s;
  HIPCHK(hipSetDevice(s->ctx->device));
  int covered = 0, max_filled = 0;
  TRY(timegrid_progress(tg, &covered, &max_filled));
  TRY(timegrid_check_slots(tg, slot0, n, covered, "covered grid"));
  std::string err;
  const int rc = autocor_from_ring(s->stream, tg->view(slot0), n, linear, host_out, err);
  return rc ? mjhmc_fail(rc, err) : 0;
}

int mjhmc_grid_lagcov(mjhmc_timegrid* tg, int slot0, int n, int max_lag, const double* shift, double* A_out, double* S_out) {
  if (!tg || !A_out) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  mjhmc_sampler* s = tg->s;
  HIPCHK(hipSetDevice(s->ctx->device));
  int covered = 0, max_filled = 0;
  TRY(timegrid_progress(tg, &covered, &max_filled));
  TRY(timegrid_check_slots(tg, slot0, n, covered, "covered grid"));
  std::string err;
  const int rc = lagcov_from_ring(s->stream, tg->view(slot0), n, max_lag, shift, A_out, S_out, err);
  return rc ? mjhmc_fail(rc, err) : 0;
}

#ifdef MJHMC_TEST_HOOKS
// test build only: the raw bytes of grid slot `slot`, padding rows included ([Npad][pitch] of the state's own type)
int mjhmc_test_timegrid_read_raw(mjhmc_timegrid* tg, int slot, void* host_dst, size_t nbytes) {
  if (!tg || !host_dst || slot < 0 || slot >= tg->n_grid || nbytes != tg->slot_bytes)
    return mjhmc_fail(MJHMC_ERR_INVALID, "bad argument");
  mjhmc_sampler* s = tg->s;
  HIPCHK(hipSetDevice(s->ctx->device));
  HIPCHK(hipMemcpyAsync(host_dst, tg->grid + (size_t)slot * tg->slot_bytes, nbytes, hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  return 0;
}
#endif

}  // extern "C"
