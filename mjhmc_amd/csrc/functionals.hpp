// Device functionals: K values g[k] = value_k(S; p) of every recorded state, S[j] = sum_{d < ndims} stat_j(x_d, d; p) --
// the coupled-energy convention of user_expr.hip turned into an observable.  functionals_eval_kernel reads n slots of a
// sample ring (float64, float32 or bfloat16 rows) and writes n slots of a float64 DERIVED ring with the project's row
// layout [Npad][pitchK]; every estimator of the sample ring then runs on the derived ring unchanged.
//
// This header is what hipRTC compiles around the caller's expressions (functionals.hip: functionals_source); it holds
// device code only and includes nothing of the project but ring_rows.hpp, which is of the same kind.  It is compiled by
// rtc_compile (user_expr.hip) with the library's own flags, -ffp-contract=off among them: no product is fused into a sum, so an expression built from + - * /,
// comparisons and ?: rounds operation by operation, as the same NumPy expression does.  Keep that flag for this kernel.
//
// Access shape (ring_rows.hpp: a lane owns 16 bytes of a row, 2 / 4 / 8 elements, widened by RowChunk<DT>); cw = 2^m
// <= 64 column lanes form a row group inside one wave.
//   narrow rows (a row is at most 64 chunks of 16 bytes): one chunk per lane, cw = pow2ceil(chunks); a lane keeps
//     kFnInFlight rows of its row group in flight (kFnInFlight loads issued before the first is used);
//   wide rows: a wave per row, lane l walks chunks l, l + 64, ... in ascending order, kFnInFlight loads at a time.
// A lane adds its elements to J float64 partials in ascending d (padding elements d >= ndims are skipped, not added as
// zeros: a stat need not vanish at 0); the cw partials are then combined by the butterfly t += shfl_xor(t, o), o = 1, 2,
// ... cw / 2, after which every lane of the group holds the same bits (a + b == b + a).  No LDS, no atomics on floats.
// The summation order of a stat is therefore a function of (ndims, dtype, pitch) alone: values are bit-identical from
// run to run and do not depend on how a run is cut into blocks.  All lanes of the group evaluate the K values; lane
// e mod cw stores element e of the derived row, elements K <= e < pitchK as 0.0.
//
// Rows p >= N of the source are never read; rows p >= N of the derived ring are never written (they are zero from
// allocation).  A value of a row p < N that is not finite sets bit k of *bad (an integer atomic).
#pragma once
#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#include <stdint.h>
#endif
#include "ring_rows.hpp"

namespace mjhmc {

constexpr int kFnMaxStats = 8;
constexpr int kFnMaxValues = 16;

struct FunctionalsArgs {
  const void* src;        // first source slot: [n][Npad][pitch] elements of the ring's type
  double* dst;            // first derived slot: [n][Npad][pitchK]
  long long Npad, N;
  int n, D, pitch, chunks;   // chunks = pitch / (elements per 16 bytes)
  int cw, log_cw;            // narrow rows: column lanes of a row group
  int* bad;
};

// the butterfly over the cw lanes of a row group (cw a power of two <= 64, groups aligned inside the wave)
__device__ __forceinline__ double fn_group_sum(double t, int cw) {
  for (int o = 1; o < cw; o <<= 1) t += __shfl_xor(t, o, 64);
  return t;
}

// values of one state from its stats, stored by the lanes of its row group; returns nothing, raises bits of *bad
template <typename F>
__device__ __forceinline__ void fn_finish(const F& f, double* S, int cx, int cw, double* __restrict__ out,
                                          int* __restrict__ bad) {
  constexpr int K = F::K, PK = (K + 1) / 2 * 2;
#pragma unroll
  for (int j = 0; j < F::J; ++j) S[j] = fn_group_sum(S[j], cw);
  double g[PK];
#pragma unroll
  for (int e = 0; e < PK; ++e) g[e] = 0.0;
  f.values(S, g);
  int nf = 0;
#pragma unroll
  for (int k = 0; k < K; ++k)
    if (!finite_f64(g[k])) nf |= 1 << k;
#pragma unroll
  for (int e = 0; e < PK; ++e)
    if ((e & (cw - 1)) == cx) out[e] = g[e];
  if (nf && cx == 0) atomicOr(bad, nf);
}

// F: { static constexpr int J, K; const double* p; void add_stats(double x, int d, double* a) const;
//      void values(const double* S, double* g) const; } -- generated around the caller's expressions
template <int DT, typename F, bool WIDE>
__global__ __launch_bounds__(256) void functionals_eval_kernel(FunctionalsArgs a, F f) {
  constexpr int VEC = RowChunk<DT>::VEC;
  constexpr int JS = F::J > 0 ? F::J : 1;
  constexpr int PK = (F::K + 1) / 2 * 2;
  const int tid = threadIdx.x;
  for (int k = blockIdx.y; k < a.n; k += gridDim.y) {
    const uint4* slot = reinterpret_cast<const uint4*>(a.src) + (size_t)k * a.Npad * a.chunks;
    double* dslot = a.dst + (size_t)k * a.Npad * PK;
    if (!WIDE) {
      const int cx = tid & (a.cw - 1), ry = tid >> a.log_cw, rw = 256 >> a.log_cw;
      const bool active = cx < a.chunks;
      const long long p0 = (long long)blockIdx.x * kFnInFlight * rw + ry;
      uint4 q[kFnInFlight];
#pragma unroll
      for (int u = 0; u < kFnInFlight; ++u) {
        const long long p = p0 + (long long)u * rw;
        q[u] = make_uint4(0u, 0u, 0u, 0u);
        if (active && p < a.N) q[u] = slot[(size_t)p * a.chunks + cx];
      }
#pragma unroll
      for (int u = 0; u < kFnInFlight; ++u) {
        const long long p = p0 + (long long)u * rw;
        if (p >= a.N) continue;   // (uniform over the row group: its lanes share p)
        double S[JS];
#pragma unroll
        for (int j = 0; j < JS; ++j) S[j] = 0.0;
        if (active) {
          double x[VEC];
          RowChunk<DT>::widen(q[u], x);
#pragma unroll
          for (int e = 0; e < VEC; ++e) {
            const int d = cx * VEC + e;
            if (d < a.D) f.add_stats(x[e], d, S);
          }
        }
        fn_finish(f, S, cx, a.cw, dslot + (size_t)p * PK, a.bad);
      }
    } else {
      const int lane = tid & 63, wave = tid >> 6;
      const long long p = (long long)blockIdx.x * 4 + wave;
      if (p >= a.N) continue;     // (uniform over the wave)
      const uint4* row = slot + (size_t)p * a.chunks;
      double S[JS];
#pragma unroll
      for (int j = 0; j < JS; ++j) S[j] = 0.0;
      for (int c0 = lane; c0 < a.chunks; c0 += 64 * kFnInFlight) {
        uint4 q[kFnInFlight];
#pragma unroll
        for (int u = 0; u < kFnInFlight; ++u) {
          const int c = c0 + 64 * u;
          q[u] = make_uint4(0u, 0u, 0u, 0u);
          if (c < a.chunks) q[u] = row[c];
        }
#pragma unroll
        for (int u = 0; u < kFnInFlight; ++u) {
          const int c = c0 + 64 * u;
          if (c < a.chunks) {
            double x[VEC];
            RowChunk<DT>::widen(q[u], x);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
              const int d = c * VEC + e;
              if (d < a.D) f.add_stats(x[e], d, S);
            }
          }
        }
      }
      fn_finish(f, S, lane, 64, dslot + (size_t)p * PK, a.bad);
    }
  }
}

}  // namespace mjhmc
