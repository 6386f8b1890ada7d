// Energy observables: K = 3 values of every recorded state that are NOT sums of per-coordinate terms of x alone --
//     g[0] = E(x)                          the potential energy, as the sampler's own evaluation kernel returns it
//     g[1] = sum_{d < ndims} G_d * G_d     G = dE/dX of the same evaluation
//     g[2] = sum_{d < ndims} x_d * G_d     the virial: E_p[x . grad E] = ndims for every smooth target
// written as a row [E, grad_sq, virial, 0.0] of the DERIVED ring of a mjhmc_functionals (functionals.hip), so that every
// accumulator of the sample ring runs on them unchanged.  E and G come from run_eval (state_io.hip) on the ring slot itself --
// a ring slot has the layout of a state matrix -- into scratch of the handle; energy_observables_kernel below forms the row.
//
// Access shape: that of functionals_eval_kernel (functionals.hpp).  A lane owns 16 bytes of the X row (2 / 4 / 8 elements
// of float64 / float32 / bfloat16) and the matching elements of the G row (float64 or float32: one or two 16-byte loads);
// cw = 2^m <= 64 column lanes form a row group inside one wave.
//   narrow rows (at most 64 chunks): one chunk per lane, kFnInFlight rows of the row group in flight;
//   wide rows: a wave per row, lane l walks chunks l, l + 64, ... in ascending order, kFnInFlight chunks at a time.
// Every element is widened exactly to float64; a lane adds g * g and x * g to its two partials in ascending d, skipping
// d >= ndims; the cw partials are combined by the butterfly t += shfl_xor(t, o), o = 1, 2, ... cw / 2 (fn_group_sum).  The
// library is built with -ffp-contract=off and the pragma below repeats it for this file: no product is fused into a sum.
// No LDS, no atomics on floats.  The summation order is a function of (ndims, state type, pitch) alone: values are
// bit-identical from run to run and independent of how a run is cut into blocks.
//
// Rows p >= N of X, G and E are never read; rows p >= N of the derived ring are never written (zero from allocation).
// A value of a row p < N that is not finite sets bit k of *bad (an integer atomic).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "functionals.hpp"

namespace mjhmc {

constexpr int kEnergyObsValues = 3;   // E, grad_sq, virial
constexpr int kEnergyObsPitch = 4;    // the derived row: the three and a 0.0

struct EnergyObsArgs {
  const void* X;      // one ring slot: [Npad][pitch] elements of the state's type
  const void* G;      // dE/dX of that slot: [Npad][pitch] float64 (float64 state) or float32
  const void* E;      // E of that slot: [Npad] of the gradient's type
  double* dst;        // one derived slot: [Npad][4]
  long long N;
  int D, pitch, chunks;   // chunks = pitch / (state elements per 16 bytes)
  int cw, log_cw;         // narrow rows: column lanes of a row group
  int* bad;
};

// the G elements that match one 16-byte chunk of X: VEC elements of GT (0 float64, 1 float32) = NQ 16-byte loads
template <int DT, int GT>
struct EoGrad {
  static constexpr int VEC = RowChunk<DT>::VEC;
  static constexpr int GVEC = RowChunk<GT>::VEC;
  static_assert(GT == 0 || GT == 1, "dE/dX is float64 or float32");
  static_assert(VEC % GVEC == 0, "a chunk of X must cover whole 16-byte chunks of dE/dX");
  static constexpr int NQ = VEC / GVEC;
  __device__ static __forceinline__ void load(const uint4* __restrict__ grow, int c, uint4* q) {
#pragma unroll
    for (int i = 0; i < NQ; ++i) q[i] = grow[(size_t)c * NQ + i];
  }
  __device__ static __forceinline__ void zero(uint4* q) {
#pragma unroll
    for (int i = 0; i < NQ; ++i) q[i] = make_uint4(0u, 0u, 0u, 0u);
  }
  __device__ static __forceinline__ void widen(const uint4* q, double* g) {
#pragma unroll
    for (int i = 0; i < NQ; ++i) RowChunk<GT>::widen(q[i], g + i * GVEC);
  }
};

template <int GT>
__device__ __forceinline__ double eo_energy(const void* __restrict__ E, long long p) {
  if (GT == 0) return reinterpret_cast<const double*>(E)[p];
  return (double)reinterpret_cast<const float*>(E)[p];
}

#pragma clang fp contract(off)
// chunk c of a row: its elements d < D, in ascending d, into the lane's two partials
template <int DT, int GT>
__device__ __forceinline__ void eo_add_chunk(const uint4& qx, const uint4* qg, int c, int D, double& gs, double& vr) {
  constexpr int VEC = RowChunk<DT>::VEC;
  double x[VEC], g[VEC];
  RowChunk<DT>::widen(qx, x);
  EoGrad<DT, GT>::widen(qg, g);
#pragma unroll
  for (int e = 0; e < VEC; ++e) {
    const int d = c * VEC + e;
    if (d < D) {
      const double gg = g[e] * g[e];
      const double xg = x[e] * g[e];
      gs = gs + gg;
      vr = vr + xg;
    }
  }
}

// the row of one state from the lanes' partials; lane 0 of the row group stores its 32 bytes
__device__ __forceinline__ void eo_finish(double e, double gs, double vr, int cx, int cw, double* __restrict__ out,
                                          int* __restrict__ bad) {
  gs = fn_group_sum(gs, cw);
  vr = fn_group_sum(vr, cw);
  if (cx != 0) return;
  int nf = 0;
  if (!finite_f64(e)) nf |= 1;
  if (!finite_f64(gs)) nf |= 2;
  if (!finite_f64(vr)) nf |= 4;
  double2* o = reinterpret_cast<double2*>(out);
  o[0] = make_double2(e, gs);
  o[1] = make_double2(vr, 0.0);
  if (nf) atomicOr(bad, nf);
}

// DT: the state's type (0 float64, 1 float32, 2 bfloat16); GT: the gradient's and the energy's (0 float64, 1 float32)
template <int DT, int GT, bool WIDE>
__global__ __launch_bounds__(256) void energy_observables_kernel(EnergyObsArgs a) {
  using GR = EoGrad<DT, GT>;
  constexpr int NQ = GR::NQ;
  const int tid = threadIdx.x;
  const uint4* __restrict__ X = reinterpret_cast<const uint4*>(a.X);
  const uint4* __restrict__ G = reinterpret_cast<const uint4*>(a.G);
  if (!WIDE) {
    const int cx = tid & (a.cw - 1), ry = tid >> a.log_cw, rw = 256 >> a.log_cw;
    const bool active = cx < a.chunks;
    const long long p0 = (long long)blockIdx.x * kFnInFlight * rw + ry;
    uint4 qx[kFnInFlight], qg[kFnInFlight][NQ];
    double en[kFnInFlight];
#pragma unroll
    for (int u = 0; u < kFnInFlight; ++u) {
      const long long p = p0 + (long long)u * rw;
      qx[u] = make_uint4(0u, 0u, 0u, 0u);
      GR::zero(qg[u]);
      en[u] = 0.0;
      if (p < a.N) {
        if (active) {
          qx[u] = X[(size_t)p * a.chunks + cx];
          GR::load(G + (size_t)p * a.chunks * NQ, cx, qg[u]);
        }
        if (cx == 0) en[u] = eo_energy<GT>(a.E, p);
      }
    }
#pragma unroll
    for (int u = 0; u < kFnInFlight; ++u) {
      const long long p = p0 + (long long)u * rw;
      if (p >= a.N) continue;   // (uniform over the row group: its lanes share p)
      double gs = 0.0, vr = 0.0;
      if (active) eo_add_chunk<DT, GT>(qx[u], qg[u], cx, a.D, gs, vr);
      eo_finish(en[u], gs, vr, cx, a.cw, a.dst + (size_t)p * kEnergyObsPitch, a.bad);
    }
  } else {
    const int lane = tid & 63, wave = tid >> 6;
    const long long p = (long long)blockIdx.x * 4 + wave;
    if (p >= a.N) return;     // (uniform over the wave)
    const uint4* xrow = X + (size_t)p * a.chunks;
    const uint4* grow = G + (size_t)p * a.chunks * NQ;
    double gs = 0.0, vr = 0.0;
    for (int c0 = lane; c0 < a.chunks; c0 += 64 * kFnInFlight) {
      uint4 qx[kFnInFlight], qg[kFnInFlight][NQ];
#pragma unroll
      for (int u = 0; u < kFnInFlight; ++u) {
        const int c = c0 + 64 * u;
        qx[u] = make_uint4(0u, 0u, 0u, 0u);
        GR::zero(qg[u]);
        if (c < a.chunks) {
          qx[u] = xrow[c];
          GR::load(grow, c, qg[u]);
        }
      }
#pragma unroll
      for (int u = 0; u < kFnInFlight; ++u) {
        const int c = c0 + 64 * u;
        if (c < a.chunks) eo_add_chunk<DT, GT>(qx[u], qg[u], c, a.D, gs, vr);
      }
    }
    const double e = lane == 0 ? eo_energy<GT>(a.E, p) : 0.0;
    eo_finish(e, gs, vr, lane, 64, a.dst + (size_t)p * kEnergyObsPitch, a.bad);
  }
}

// energy_observables.hip: one launch, on `stream`, for one slot.  state_dtype: MJHMC_F64 / _F32 / _BF16 (0 / 1 / 2);
// grad_f32: the gradient and the energy are float32.  Returns false for a pair of types no energy family writes.
bool energy_observables_launch(const EnergyObsArgs& a, int state_dtype, bool grad_f32, bool wide, hipStream_t stream);

}  // namespace mjhmc
