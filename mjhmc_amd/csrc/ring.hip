// The sample ring of a sampler: allocation, the readers (blocks, dwelling times, gathered states, moments,
// autocorrelation, lagged covariance), slot copies, and the test build's slot write.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "autocor.hpp"
#include "lagcov.hpp"
#include "sampler_internal.hpp"

// block-reduced shifted moments of the valid elements of `rows` particle rows
template <typename T>
__global__ void moments_kernel(const T* __restrict__ src, int64_t nrows_pad_per_slot, int64_t nrows_per_slot, int nslots,
                               int D, int pitch, double shift, double* out) {
  double s1 = 0.0, s2 = 0.0;
  const int64_t per_slot = nrows_per_slot * D;
  const int64_t total = per_slot * nslots;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t slot = i / per_slot, rem = i - slot * per_slot;
    const int64_t row = rem / D;
    const int d = (int)(rem - row * D);
    const double v = (double)src[(size_t)(slot * nrows_pad_per_slot + row) * pitch + d] - shift;
    s1 += v;
    s2 += v * v;
  }
  for (int o = 32; o > 0; o >>= 1) {
    s1 += __shfl_xor(s1, o);
    s2 += __shfl_xor(s2, o);
  }
  __shared__ double sm[2][16];
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    sm[0][w] = s1;
    sm[1][w] = s2;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    double t = 0.0;
    for (int k = 0; k < (int)(blockDim.x >> 6); ++k) t += sm[threadIdx.x][k];
    atomicAdd(&out[threadIdx.x], t);
  }
}

// the range check of a reader of ring slots [slot0, slot0 + n), the device made current, and the block as a RingView
static int ring_block(mjhmc_sampler* s, int slot0, int n, RingView* view) {
  if (slot0 < 0 || n < 1 || (int64_t)slot0 + n > s->ring_slots)
    return fail(MJHMC_ERR_INVALID, "ring slots [" + std::to_string(slot0) + ", " + std::to_string((int64_t)slot0 + n) +
                                       ") are outside the ring of " + std::to_string(s->ring_slots));
  HIPCHK(hipSetDevice(s->ctx->device));
  *view = RingView{(const char*)s->ring + (size_t)slot0 * mat_bytes(s), s->dtype, s->Npad, s->N, s->D, s->sh.pitch};
  return 0;
}

extern "C" {

int mjhmc_ring_alloc(mjhmc_sampler* s, int n_slots) {
  if (!s || n_slots < 1) return fail(MJHMC_ERR_INVALID, "bad argument");
  HIPCHK(hipSetDevice(s->ctx->device));
  if (n_slots <= s->ring_slots) return 0;
  HIPCHK(hipStreamSynchronize(s->stream));
  const size_t mb = mat_bytes(s);
  // the NEW ring first: a request the device cannot hold leaves the sampler with the ring it had
  void* ring = nullptr;
  double* dring = nullptr;
  hipError_t e = hipMalloc(&ring, (size_t)n_slots * mb);
  if (e == hipSuccess) e = hipMalloc((void**)&dring, (size_t)n_slots * s->Npad * sizeof(double));
  if (e != hipSuccess) {
    if (ring) (void)hipFree(ring);
    (void)hipGetLastError();
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    char msg[320];
    std::snprintf(msg, sizeof(msg), "a sample ring of %d slots x %.3f GB = %.1f GB does not fit the device (%.1f GB free of %.1f GB): "
                  "record in chunks (mjhmc_iterate_download over a smaller ring) -- the ring the sampler had is kept",
                  n_slots, mb / 1e9, (double)n_slots * mb / 1e9, free_b / 1e9, total_b / 1e9);
    return fail(MJHMC_ERR_HIP, msg);
  }
  // (on the sampler's stream: it does not wait for the null stream, and a memset there can land AFTER the first slots are written)
  HIPCHK(hipMemsetAsync(ring, 0, (size_t)n_slots * mb, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  s->undo_valid = false;
  // the live X may sit in the old ring: park it in a ping-pong buffer before freeing
  if (s->ring && (char*)s->Xcur >= (char*)s->ring && (char*)s->Xcur < (char*)s->ring + (size_t)s->ring_slots * mb) {
    HIPCHK(hipMemcpy(s->Xbuf[0], s->Xcur, mb, hipMemcpyDeviceToDevice));
    s->Xcur = s->Xbuf[0];
  }
  if (s->ring) HIPCHK(hipFree(s->ring));
  if (s->dwell_ring) HIPCHK(hipFree(s->dwell_ring));
  s->ring = ring;
  s->dwell_ring = dring;
  s->ring_slots = n_slots;
  ++s->ring_gen;
  return 0;
}

int mjhmc_ring_slot_bytes(mjhmc_sampler* s, uint64_t* bytes) {
  if (!s || !bytes) return fail(MJHMC_ERR_INVALID, "NULL argument");
  *bytes = (uint64_t)mat_bytes(s) + (uint64_t)s->Npad * sizeof(double);
  return 0;
}

int mjhmc_ring_read_dwell(mjhmc_sampler* s, int slot0, int n, double* host_dst) {
  if (!s || !host_dst) return fail(MJHMC_ERR_INVALID, "NULL argument");
  RingView view;
  TRY(ring_block(s, slot0, n, &view));
  HIPCHK(hipMemcpy2DAsync(host_dst, (size_t)s->N * sizeof(double), s->dwell_ring + (size_t)slot0 * s->Npad,
                          (size_t)s->Npad * sizeof(double), (size_t)s->N * sizeof(double), (size_t)n,
                          hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  return 0;
}

int mjhmc_ring_gather(mjhmc_sampler* s, const int64_t* idx, int64_t n, double* host_out) {
  if (!s || !idx || !host_out || n < 1) return fail(MJHMC_ERR_INVALID, "bad argument");
  HIPCHK(hipSetDevice(s->ctx->device));
  const int64_t pool = (int64_t)s->ring_slots * s->N;
  for (int64_t k = 0; k < n; ++k)
    if (idx[k] < 0 || idx[k] >= pool) return fail(MJHMC_ERR_INVALID, "gather index outside the sample ring");
  std::vector<int64_t> rows((size_t)n);  // pool index (slot * N + p) -> padded row (slot * Npad + p)
  for (int64_t k = 0; k < n; ++k) rows[k] = (idx[k] / s->N) * s->Npad + idx[k] % s->N;
  int64_t* didx = nullptr;
  HIPCHK(hipMalloc((void**)&didx, n * sizeof(int64_t)));
  int rc = 0;
  do {
    if (hipMemcpyAsync(didx, rows.data(), n * sizeof(int64_t), hipMemcpyHostToDevice, s->stream) != hipSuccess) {
      rc = fail(MJHMC_ERR_HIP, "index upload failed");
      break;
    }
    rc = ensure_stage(s, (size_t)s->D * n);
    if (rc) break;
    rc = download_cols(s, s->ring, didx, n, host_out, (size_t)s->D * n, n, 1, 0, true);
  } while (0);
  (void)hipFree(didx);
  return rc;
}

int mjhmc_ring_read(mjhmc_sampler* s, int slot0, int n, int stacked, double* host_out) {
  if (!s || !host_out) return fail(MJHMC_ERR_INVALID, "NULL argument");
  RingView view;
  TRY(ring_block(s, slot0, n, &view));
  const size_t total = (size_t)s->D * s->N * n;
  TRY(ensure_stage(s, total));
  const size_t mb = mat_bytes(s);
  const char* base = (const char*)view.base;
  // slot k: the columns [k N, (k + 1) N) of a row, or -- stacked -- every n-th column from k
  for (int k = 0; k < n; ++k)
    TRY(download_cols(s, base + (size_t)k * mb, nullptr, s->N, host_out, total, (int64_t)n * s->N, stacked ? n : 1,
                      stacked ? k : (int64_t)k * s->N, k == n - 1));
  return 0;
}

int mjhmc_ring_copy(mjhmc_sampler* s, int src_slot, int dst_slot) {
  if (!s) return fail(MJHMC_ERR_INVALID, "sampler is NULL");
  if (src_slot < 0 || dst_slot < 0 || src_slot >= s->ring_slots || dst_slot >= s->ring_slots)
    return fail(MJHMC_ERR_INVALID, "slots out of range");
  if (src_slot == dst_slot) return 0;
  const size_t mb = mat_bytes(s);
  char* dst = (char*)s->ring + (size_t)dst_slot * mb;
  if ((char*)s->Xcur == dst) return fail(MJHMC_ERR_INVALID, "the destination slot holds the live state");
  HIPCHK(hipSetDevice(s->ctx->device));
  if (s->undo_valid && (char*)s->undo_X == dst) s->undo_valid = false;
  HIPCHK(hipMemcpyAsync(dst, (const char*)s->ring + (size_t)src_slot * mb, mb, hipMemcpyDeviceToDevice, s->stream));
  HIPCHK(hipMemcpyAsync(s->dwell_ring + (size_t)dst_slot * s->Npad, s->dwell_ring + (size_t)src_slot * s->Npad,
                        (size_t)s->Npad * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
  return 0;
}

#ifdef MJHMC_TEST_HOOKS
// test build only: a host (ndims, N) float64 block into ring slot `slot`, through the re-tiling every state upload takes
// (synthetic chains with a known answer for the chain-statistics tests)
int mjhmc_test_ring_write(mjhmc_sampler* s, int slot, const double* X) {
  if (!s || !X || slot < 0 || slot >= s->ring_slots) return fail(MJHMC_ERR_INVALID, "bad argument");
  char* dst = (char*)s->ring + (size_t)slot * mat_bytes(s);
  if ((char*)s->Xcur == dst) return fail(MJHMC_ERR_INVALID, "the slot holds the live state");
  HIPCHK(hipSetDevice(s->ctx->device));
  if (s->undo_valid && (char*)s->undo_X == dst) s->undo_valid = false;
  TRY(upload_matrix(s, X, dst));
  HIPCHK(hipStreamSynchronize(s->stream));   // (X is the caller's for the duration of the call only)
  return 0;
}
#endif

int mjhmc_ring_moments(mjhmc_sampler* s, int slot0, int n, double shift, double* sum, double* sumsq) {
  if (!s || !sum || !sumsq) return fail(MJHMC_ERR_INVALID, "NULL argument");
  RingView view;
  TRY(ring_block(s, slot0, n, &view));
  TRY(ensure_stage(s, 2));
  HIPCHK(hipMemsetAsync(s->stage, 0, 2 * sizeof(double), s->stream));
  dispatch_dtype(view.dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(moments_kernel<T>, dim3(1024), dim3(256), 0, s->stream, (const T*)view.base, s->Npad, s->N, n, s->D,
                       s->sh.pitch, shift, s->stage);
  });
  HIPCHK(hipGetLastError());
  double h[2];
  HIPCHK(hipMemcpyAsync(h, s->stage, sizeof(h), hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  *sum = h[0];
  *sumsq = h[1];
  return 0;
}

int mjhmc_ring_autocor(mjhmc_sampler* s, int slot0, int n, int linear, double* host_out) {
  if (!s || !host_out) return fail(MJHMC_ERR_INVALID, "NULL argument");
  RingView view;
  TRY(ring_block(s, slot0, n, &view));
  std::string err;
  const int rc = autocor_from_ring(s->stream, view, n, linear, host_out, err);
  return rc ? fail(rc, err) : 0;
}

int mjhmc_ring_lagcov(mjhmc_sampler* s, int slot0, int n, int max_lag, const double* shift, double* A_out, double* S_out) {
  if (!s || !A_out) return fail(MJHMC_ERR_INVALID, "NULL argument");
  RingView view;
  TRY(ring_block(s, slot0, n, &view));
  std::string err;
  const int rc = lagcov_from_ring(s->stream, view, n, max_lag, shift, A_out, S_out, err);
  return rc ? fail(rc, err) : 0;
}

}  // extern "C"
