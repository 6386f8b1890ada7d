// How the device statistics read the rows of a ring (the sample ring, a derived ring, a grid ring): float64, float32 or
// bfloat16 elements, every one widened to float64 EXACTLY before anything is computed from it.
//
// The access shape the row passes share (the moment pass of estimators.hip, the histogram pass of histograms.hip, the
// chain pass of chainstats.hip, functionals.hpp, energy_observables.hpp, projections.hpp): a lane owns 16 bytes of a
// row -- one uint4 load, 2 / 4 / 8 elements (RowChunk<DT>::VEC) -- and issues k*InFlight such loads before it uses the
// first.  Rows p >= N are never read.  Each file says how it lays lanes over rows and what it does with the values.
//
// Device code only; includes nothing of the project: hipRTC compiles this header with functionals.hpp,
// energy_observables.hpp and projections.hpp around the caller's expressions.
#pragma once
#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#include <stdint.h>
#endif

namespace mjhmc {

// 16-byte loads a lane issues before it uses the first: over rows (moment and histogram passes), over slots (chain pass),
// over rows or chunks of a row (functionals, energy observables)
constexpr int kRowsInFlight = 4;
constexpr int kSlotsInFlight = 4;
constexpr int kFnInFlight = 4;

// finite: neither NaN nor an infinity (DBL_MAX spelled out: hipRTC has no <cfloat>)
__device__ __forceinline__ bool finite_f64(double v) { return fabs(v) <= 1.7976931348623157e308; }

// the 16 bits of a bfloat16 (in the low half of `bits`) -> float64
__device__ __forceinline__ double bf16_to_f64(unsigned bits) { return (double)__uint_as_float(bits << 16); }

// one stored element, as a kernel holds it in a register (bfloat16 as its 16 bits) -> float64
template <typename T>
struct ElemBits {
  typedef T type;
};
template <>
struct ElemBits<__bf16> {
  typedef unsigned short type;
};
__device__ __forceinline__ double elem_to_f64(double v) { return v; }
__device__ __forceinline__ double elem_to_f64(float v) { return (double)v; }
__device__ __forceinline__ double elem_to_f64(unsigned short v) { return bf16_to_f64(v); }

// 16 bytes of a row -> VEC doubles.  DT: 0 float64, 1 float32, 2 bfloat16 (the MJHMC_* dtype codes)
template <int DT>
struct RowChunk;
template <>
struct RowChunk<0> {
  static constexpr int VEC = 2;
  __device__ static __forceinline__ void widen(const uint4& q, double* v) {
    v[0] = __longlong_as_double((long long)(((unsigned long long)q.y << 32) | (unsigned long long)q.x));
    v[1] = __longlong_as_double((long long)(((unsigned long long)q.w << 32) | (unsigned long long)q.z));
  }
};
template <>
struct RowChunk<1> {
  static constexpr int VEC = 4;
  __device__ static __forceinline__ void widen(const uint4& q, double* v) {
    v[0] = (double)__uint_as_float(q.x);
    v[1] = (double)__uint_as_float(q.y);
    v[2] = (double)__uint_as_float(q.z);
    v[3] = (double)__uint_as_float(q.w);
  }
};
template <>
struct RowChunk<2> {
  static constexpr int VEC = 8;
  __device__ static __forceinline__ void widen(const uint4& q, double* v) {
    const unsigned u[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[2 * j] = bf16_to_f64(u[j] & 0xFFFFu);
      v[2 * j + 1] = bf16_to_f64(u[j] >> 16);
    }
  }
};

// the chunk of the kernels that are templates of the element type
template <typename T>
struct DtypeCode;
template <>
struct DtypeCode<double> {
  static constexpr int value = 0;
};
template <>
struct DtypeCode<float> {
  static constexpr int value = 1;
};
template <>
struct DtypeCode<__bf16> {
  static constexpr int value = 2;
};
template <typename T>
using ChunkOf = RowChunk<DtypeCode<T>::value>;

}  // namespace mjhmc
