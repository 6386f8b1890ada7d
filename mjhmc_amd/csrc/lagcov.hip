// Centred linear lag sums per dimension, on the device.
//
//   u[t][p][d] = (double)x[t][p][d] - c[d]
//   A[k][d]    = sum_{p < N} sum_{t + k < n} u[t][p][d] u[t + k][p][d],  k = 0 .. K <= 256;   S[d] = sum_p sum_t u[t][p][d]
//
// The register form of lag_sums_direct (autocor.hip), kept per dimension instead of pooled.  A thread owns one coordinate d
// of one particle slot of its block; consecutive threads take consecutive coordinates of a state row (coalesced).  With
// dpw = the power of two >= min(D, 64) lanes along d, a block of 256 threads holds PB = 256 / dpw particle slots (D = 2: 128
// particles per block, 32 per wave; D >= 64: one particle per wave and blockIdx.y walks the 64-wide column chunks).
//
// Lags go in BANDS of 32 (k0 = 0, 32, ..), one launch per band.  Within a band a thread walks its particles p = q + PB *
// (blockIdx.x + i * gridDim.x), i ascending, and per particle its series in TILES of 32 time steps, t ascending, with three
// statically indexed register arrays of 32 doubles: the accumulators acc[kk] of lags k0 + kk, carried from particle to
// particle, and the window A = u[T0 - 32 .. T0), B = u[T0 .. T0 + 32) (zeros outside [0, n)).  The leading value
// y = u[T0 + k0 + j] meets the 32 trailing values u[T0 + j - kk]: acc[kk] = fma(win[j + 32 - kk], y, acc[kk]).  In band 0 the
// leading tile IS B and every slot is read once (K <= 31: one read of the n slots); a later band loads its leading values
// as well (8 at a time, k0 steps ahead of the window), so it reads slots [0, n - k0) and [k0, n): at most two reads.
// Leading steps at or beyond n are skipped by a wave-uniform branch: a band costs n * 32 multiply-adds per series.
// S is added from the B tiles of band 0.
//
// Order of addition (a function of N, D, n, K alone: the launch shape below holds no device property):
//   thread: particles ascending, tiles ascending, j ascending, one fma per (j, kk)
//   block:  the PB particle slots of a coordinate meet in LDS, slot 0 first
//   grid:   lagcov_finish adds the per-block partials, block 0 first
// No atomics of any kind in this file.
#include "lagcov.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/mjhmc_hip.h"
#include "ring_source.hpp"   // dispatch_dtype

namespace {

constexpr int kBand = 32;          // lags per band = time steps per tile
constexpr int kLead = 8;           // leading values a later band holds at a time
constexpr int kRows = kBand + 1;   // rows of a block's partial: the band's lags, then S
constexpr int kMaxBlocks = 1024;   // blocks of a band's launch (x * y): two per CU resident at 2 waves / SIMD, twice over

template <typename T, bool FIRST>
__global__ __launch_bounds__(256) void lagcov_pass(const T* __restrict__ ring, size_t slot_elems, int pitch, int D, int64_t N, int n,
                                                   int k0, int dpw_log2, const double* __restrict__ shift,
                                                   double* __restrict__ partial, int Dp) {
  const int tid = threadIdx.x;
  const int dpw = 1 << dpw_log2;
  const int dl = tid & (dpw - 1);
  const int q = tid >> dpw_log2;     // particle slot of the block
  const int PB = 256 >> dpw_log2;
  const int d = blockIdx.y * 64 + dl;   // (gridDim.y == 1 unless dpw == 64)
  const bool d_ok = d < D;
  const double c = (d_ok && shift) ? shift[d] : 0.0;
  double acc[kBand];
#pragma unroll
  for (int kk = 0; kk < kBand; ++kk) acc[kk] = 0.0;
  double s = 0.0;
  for (int64_t pb = (int64_t)blockIdx.x * PB; pb < N; pb += (int64_t)gridDim.x * PB) {
    const int64_t p = pb + q;
    if (!d_ok || p >= N) continue;
    const T* const x = ring + (size_t)p * pitch + d;
    double A[kBand], B[kBand];
#pragma unroll
    for (int i = 0; i < kBand; ++i) A[i] = 0.0;
    for (int T0 = 0; T0 + k0 < n; T0 += kBand) {
#pragma unroll
      for (int i = 0; i < kBand; ++i) B[i] = T0 + i < n ? (double)x[(size_t)(T0 + i) * slot_elems] - c : 0.0;
      if (FIRST) {
#pragma unroll
        for (int i = 0; i < kBand; ++i) s += B[i];
      }
#pragma unroll
      for (int j0 = 0; j0 < kBand; j0 += kLead) {
        double Y[kLead];   // (a later band's leading values, kLead at a time: 16 registers, not 64)
        if (!FIRST) {
#pragma unroll
          for (int j = 0; j < kLead; ++j) Y[j] = T0 + k0 + j0 + j < n ? (double)x[(size_t)(T0 + k0 + j0 + j) * slot_elems] - c : 0.0;
        }
#pragma unroll
        for (int jj = 0; jj < kLead; ++jj) {
          const int j = j0 + jj;
          if (T0 + k0 + j < n) {   // (wave-uniform)
            const double y = FIRST ? B[j] : Y[jj];
#pragma unroll
            for (int kk = 0; kk < kBand; ++kk) {
              const int i = j + kBand - kk;   // the trailing step T0 + j - kk in the window A | B
              acc[kk] = __builtin_fma(i < kBand ? A[i] : B[i - kBand], y, acc[kk]);
            }
          }
        }
      }
#pragma unroll
      for (int i = 0; i < kBand; ++i) A[i] = B[i];
    }
  }
  // the PB particle slots of every coordinate meet in LDS, slot 0 first; 16 lags at a time
  __shared__ double red[16][256];
  double* const mine = partial + (size_t)blockIdx.x * kRows * Dp + blockIdx.y * 64;
#pragma unroll
  for (int g0 = 0; g0 < kBand; g0 += 16) {
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) red[kk][tid] = acc[g0 + kk];
    __syncthreads();
    for (int o = tid; o < 16 * dpw; o += 256) {
      const int kk = o >> dpw_log2, col = o & (dpw - 1);
      double v = red[kk][col];
      for (int qq = 1; qq < PB; ++qq) v += red[kk][(qq << dpw_log2) + col];
      mine[(size_t)(g0 + kk) * Dp + col] = v;
    }
    __syncthreads();
  }
  if (FIRST) {
    red[0][tid] = s;
    __syncthreads();
    if (tid < dpw) {
      double v = red[0][tid];
      for (int qq = 1; qq < PB; ++qq) v += red[0][(qq << dpw_log2) + tid];
      mine[(size_t)kBand * Dp + tid] = v;
    }
  }
}

// A[k0 + kk][d] = sum over blocks, block 0 first, kk < nk; and S[d] from row kBand when S != nullptr
__global__ __launch_bounds__(256) void lagcov_finish(const double* __restrict__ partial, int n_blocks, int Dp, int D, int k0, int nk,
                                                     double* __restrict__ A, double* __restrict__ S) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int rows = nk + (S ? 1 : 0);
  if (idx >= rows * D) return;
  const int kk = idx / D, d = idx - kk * D;
  const int row = kk < nk ? kk : kBand;
  const double* src = partial + (size_t)row * Dp + d;
  double v = 0.0;
  for (int b = 0; b < n_blocks; ++b) v += src[(size_t)b * kRows * Dp];
  if (kk < nk) A[(size_t)(k0 + kk) * D + d] = v;
  else S[d] = v;
}

// host [D][N][n] -> time-major [n][Npad][pitch]
__global__ __launch_bounds__(256) void lagcov_retile(const double* __restrict__ in, int D, int64_t N, int n, int64_t Npad, int pitch,
                                                     double* __restrict__ out) {
  const int64_t total = (int64_t)n * N * D;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
    const int d = (int)(g % D);
    const int64_t r = g / D, p = r % N, t = r / N;
    out[((size_t)t * Npad + p) * pitch + d] = in[((size_t)d * N + p) * n + t];
  }
}

struct DevBuf {
  void* p = nullptr;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
};

#define LCHK(expr)                                                                                      \
  do {                                                                                                  \
    hipError_t e_ = (expr);                                                                             \
    if (e_ != hipSuccess) {                                                                             \
      err = std::string(#expr) + ": " + hipGetErrorString(e_) + " (" + __FILE__ + ":" +                 \
            std::to_string(__LINE__) + ")";                                                             \
      return MJHMC_ERR_HIP;                                                                             \
    }                                                                                                   \
  } while (0)

template <typename T>
void launch_pass(hipStream_t st, dim3 grid, bool first, const RingView& r, int n, int k0, int dpw_log2, const double* shift,
                 double* partial, int Dp) {
  const size_t slot_elems = (size_t)r.Npad * r.pitch;
  if (first)
    hipLaunchKernelGGL((lagcov_pass<T, true>), grid, dim3(256), 0, st, (const T*)r.base, slot_elems, r.pitch, r.D, r.N, n, k0, dpw_log2,
                       shift, partial, Dp);
  else
    hipLaunchKernelGGL((lagcov_pass<T, false>), grid, dim3(256), 0, st, (const T*)r.base, slot_elems, r.pitch, r.D, r.N, n, k0, dpw_log2,
                       shift, partial, Dp);
}

}  // namespace

int lagcov_check(int n, int K, const double* shift, int D, std::string& err) {
  if (n < 1) {
    err = "n must be >= 1, got " + std::to_string(n);
    return MJHMC_ERR_INVALID;
  }
  const int top = std::min(n - 1, kLagcovMaxLag);
  if (K < 0 || K > top) {
    err = "max_lag must be in [0, min(n - 1, 256) = " + std::to_string(top) + "], got " + std::to_string(K);
    return MJHMC_ERR_INVALID;
  }
  if (shift)
    for (int d = 0; d < D; ++d)
      if (!std::isfinite(shift[d])) {
        err = "shift[" + std::to_string(d) + "] is not finite";
        return MJHMC_ERR_INVALID;
      }
  return 0;
}

int lagcov_from_ring(hipStream_t st, const RingView& r, int n, int K, const double* shift, double* A_host, double* S_host,
                     std::string& err) {
  const int rc = lagcov_check(n, K, shift, r.D, err);
  if (rc) return rc;
  if (r.N < 1 || r.D < 1) {
    err = "lag sums need at least one chain and one dimension";
    return MJHMC_ERR_INVALID;
  }
  int dpw_log2 = 0;
  while ((1 << dpw_log2) < std::min(r.D, 64)) ++dpw_log2;
  const int dpw = 1 << dpw_log2, PB = 256 / dpw;
  const int gy = dpw == 64 ? (r.D + 63) / 64 : 1;
  const int Dp = gy * dpw;
  const int gx = (int)std::max<int64_t>(1, std::min<int64_t>((r.N + PB - 1) / PB, std::max(1, kMaxBlocks / gy)));
  const size_t nA = (size_t)(K + 1) * r.D;
  DevBuf partial, out, dshift;
  LCHK(hipMalloc(&partial.p, (size_t)gx * kRows * Dp * sizeof(double)));
  LCHK(hipMalloc(&out.p, (nA + r.D) * sizeof(double)));
  if (shift) {
    LCHK(hipMalloc(&dshift.p, (size_t)r.D * sizeof(double)));
    LCHK(hipMemcpyAsync(dshift.p, shift, (size_t)r.D * sizeof(double), hipMemcpyHostToDevice, st));
  }
  double* const dA = (double*)out.p;
  double* const dS = dA + nA;
  for (int k0 = 0; k0 <= K; k0 += kBand) {
    const bool first = k0 == 0;
    const dim3 grid((unsigned)gx, (unsigned)gy);
    dispatch_dtype(r.dtype, [&](auto tag) {
      launch_pass<typename decltype(tag)::type>(st, grid, first, r, n, k0, dpw_log2, (const double*)dshift.p, (double*)partial.p, Dp);
    });
    LCHK(hipGetLastError());
    const int nk = std::min(kBand, K + 1 - k0);
    const int cells = (nk + (first ? 1 : 0)) * r.D;
    hipLaunchKernelGGL(lagcov_finish, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, (const double*)partial.p, gx, Dp, r.D, k0,
                       nk, dA, first ? dS : (double*)nullptr);
    LCHK(hipGetLastError());
  }
  LCHK(hipMemcpyAsync(A_host, dA, nA * sizeof(double), hipMemcpyDeviceToHost, st));
  if (S_host) LCHK(hipMemcpyAsync(S_host, dS, (size_t)r.D * sizeof(double), hipMemcpyDeviceToHost, st));
  LCHK(hipStreamSynchronize(st));
  return 0;
}

int lagcov_from_host(hipStream_t st, const double* samples, int D, int64_t N, int n, int K, const double* shift, double* A_host,
                     double* S_host, std::string& err) {
  if (D < 1 || N < 1) {
    err = "lag sums need n_dims >= 1 and n_batch >= 1";
    return MJHMC_ERR_INVALID;
  }
  const int rc = lagcov_check(n, K, shift, D, err);
  if (rc) return rc;
  const int64_t Npad = (N + 63) / 64 * 64;
  const int pitch = (D + 1) / 2 * 2 + (D == 1 ? 2 : 0);   // whole 16-byte chunks, and wider than a one-column row
  const size_t in_bytes = (size_t)D * N * n * sizeof(double), view_bytes = (size_t)n * Npad * pitch * sizeof(double);
  DevBuf in, view;
  LCHK(hipMalloc(&in.p, in_bytes));
  LCHK(hipMalloc(&view.p, view_bytes));
  LCHK(hipMemcpyAsync(in.p, samples, in_bytes, hipMemcpyHostToDevice, st));
  LCHK(hipMemsetAsync(view.p, 0xFF, view_bytes, st));   // padding rows and columns: NaN, so that a read of one shows
  const int64_t total = (int64_t)n * N * D;
  hipLaunchKernelGGL(lagcov_retile, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((total + 255) / 256, 4096))), dim3(256), 0, st,
                     (const double*)in.p, D, N, n, Npad, pitch, (double*)view.p);
  LCHK(hipGetLastError());
  const RingView r{view.p, MJHMC_F64, Npad, N, D, pitch};
  return lagcov_from_ring(st, r, n, K, shift, A_host, S_host, err);
}
