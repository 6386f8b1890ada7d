// The hand-written exp family and the arithmetic of the jump process: rates, waiting times, the first minimum.
#pragma once
#ifndef __HIPCC_RTC__  // hipRTC pre-includes the device runtime and has no header search path to it
#include <hip/hip_runtime.h>
#endif

namespace mjhmc {

// exp(h) for |h| < 708 (normal result, no special cases): the library's range reduction and degree-11 polynomial
// without its overflow / underflow / NaN handling.  Measured 0.83 ulp against long double, gated at 2 (tests/test_gpu_device_math.py).
// p = r * p + c with the constant c in a scalar register pair: one VOP3 instruction.  hipcc's own form of a Horner
// step is v_mov x2 (the 64-bit literal into the accumulator VGPR) + v_fmac: three vector instructions.
__device__ __forceinline__ double horner_sc(double r, double p, double c) {
  asm("v_fma_f64 %0, %1, %0, %2" : "+v"(p) : "v"(r), "s"(c));
  return p;
}

template <bool FENCED = true, bool SC = !FENCED>
__device__ __forceinline__ double exp_normal(double h) {
  if constexpr (FENCED) __builtin_amdgcn_sched_barrier(0);  // chain kept compact inside decide(): measured faster
  const double n = __builtin_rint(h * __longlong_as_double(0x3ff71547652b82feLL));        // h / ln 2
  double r = __builtin_fma(n, __longlong_as_double(0xbfe62e42fefa39efLL), h);             // - n ln2 (hi, lo)
  r = __builtin_fma(n, __longlong_as_double(0xbc7abc9e3b39803fLL), r);
  if constexpr (SC) {  // the funnel's force: this chain runs once per leapfrog step (decide()'s form below was
                            // measured faster there as it stands)
    double q = r * __longlong_as_double(0x3e5ade156a5dcb37LL) + __longlong_as_double(0x3e928af3fca7ab0cLL);
    q = horner_sc(r, q, __longlong_as_double(0x3ec71dee623fde64LL));
    q = horner_sc(r, q, __longlong_as_double(0x3efa01997c89e6b0LL));
    q = horner_sc(r, q, __longlong_as_double(0x3f2a01a014761f6eLL));
    q = horner_sc(r, q, __longlong_as_double(0x3f56c16c1852b7b0LL));
    q = horner_sc(r, q, __longlong_as_double(0x3f81111111122322LL));
    q = horner_sc(r, q, __longlong_as_double(0x3fa55555555502a1LL));
    q = horner_sc(r, q, __longlong_as_double(0x3fc5555555555511LL));
    q = horner_sc(r, q, __longlong_as_double(0x3fe000000000000bLL));
    q = __builtin_fma(r, q, 1.0);
    q = __builtin_fma(r, q, 1.0);
    const double yq = __builtin_amdgcn_ldexp(q, (int)n);
    if constexpr (FENCED) __builtin_amdgcn_sched_barrier(0);
    return yq;
  }
  double p = r * __longlong_as_double(0x3e5ade156a5dcb37LL) + __longlong_as_double(0x3e928af3fca7ab0cLL);
  p = __builtin_fma(r, p, __longlong_as_double(0x3ec71dee623fde64LL));
  p = __builtin_fma(r, p, __longlong_as_double(0x3efa01997c89e6b0LL));
  p = __builtin_fma(r, p, __longlong_as_double(0x3f2a01a014761f6eLL));
  p = __builtin_fma(r, p, __longlong_as_double(0x3f56c16c1852b7b0LL));
  p = __builtin_fma(r, p, __longlong_as_double(0x3f81111111122322LL));
  p = __builtin_fma(r, p, __longlong_as_double(0x3fa55555555502a1LL));
  p = __builtin_fma(r, p, __longlong_as_double(0x3fc5555555555511LL));
  p = __builtin_fma(r, p, __longlong_as_double(0x3fe000000000000bLL));
  p = __builtin_fma(r, p, 1.0);
  p = __builtin_fma(r, p, 1.0);
  const double y = __builtin_amdgcn_ldexp(p, (int)n);
  if constexpr (FENCED) __builtin_amdgcn_sched_barrier(0);
  return y;
}
// exp() of the funnel force, branch-free: v_ldexp_f64 rounds into the subnormal range and overflows to inf by itself
// (inf for very negative x_0 is what turns a runaway chain into the non-finite abort), so clamping the argument to
// +-1100 and restoring NaN is all the special handling there is.
__device__ __forceinline__ double exp_any(double h) {
  const double y = exp_normal<false>(__builtin_fmin(__builtin_fmax(h, -1100.0), 1100.0));
  return (h != h) ? h : y;
}
__device__ __forceinline__ float exp_any(float h) { return expf(h); }

// exp(-x) for the funnel force, once per leapfrog step: the argument is clamped to +-1100 (v_ldexp_f64 then rounds into
// the subnormal range / overflows to inf by itself; inf for very negative x_0 is what turns a runaway chain into the
// non-finite abort) and the sign rides on the operand modifiers.  A NaN x_0 needs no care here: it is already in every
// energy term that contains x_0, so the rates are NaN and the attempt aborts whatever this returns.
__device__ __forceinline__ double exp_neg(double x) {
  const double xc = __builtin_fmin(__builtin_fmax(x, -1100.0), 1100.0);
  const double n = __builtin_rint(xc * __longlong_as_double(0xbff71547652b82feLL));       // -x / ln 2
  double r = __builtin_fma(n, __longlong_as_double(0xbfe62e42fefa39efLL), -xc);           // -x - n ln2 (hi, lo)
  r = __builtin_fma(n, __longlong_as_double(0xbc7abc9e3b39803fLL), r);
  double q = r * __longlong_as_double(0x3e5ade156a5dcb37LL) + __longlong_as_double(0x3e928af3fca7ab0cLL);
  q = horner_sc(r, q, __longlong_as_double(0x3ec71dee623fde64LL));
  q = horner_sc(r, q, __longlong_as_double(0x3efa01997c89e6b0LL));
  q = horner_sc(r, q, __longlong_as_double(0x3f2a01a014761f6eLL));
  q = horner_sc(r, q, __longlong_as_double(0x3f56c16c1852b7b0LL));
  q = horner_sc(r, q, __longlong_as_double(0x3f81111111122322LL));
  q = horner_sc(r, q, __longlong_as_double(0x3fa55555555502a1LL));
  q = horner_sc(r, q, __longlong_as_double(0x3fc5555555555511LL));
  q = horner_sc(r, q, __longlong_as_double(0x3fe000000000000bLL));
  q = __builtin_fma(r, q, 1.0);
  q = __builtin_fma(r, q, 1.0);
  return __builtin_amdgcn_ldexp(q, (int)n);
}
__device__ __forceinline__ float exp_neg(float x) { return expf(-x); }

// exp_neg()'s fifteen constants held in VECTOR registers by the caller for the length of a kernel (exp_neg_k: the same
// operations on the same constants, the same bits).  The relay kernel's step loops re-materialised them in scalar registers
// at every leapfrog step -- 30 s_mov_b32 per step: its 106 scalar registers are taken (70 spilled) and the loop's constants
// lost -- where it has vector registers to spare.
struct ExpNegK {
  double k[15];
};
struct NoExpK {};
__device__ __forceinline__ ExpNegK exp_neg_pinned() {
  ExpNegK K;
  const unsigned long long bits[15] = {0xc091300000000000ULL /* -1100 */, 0x4091300000000000ULL /* 1100 */,
                                       0xbff71547652b82feULL, 0xbfe62e42fefa39efULL, 0xbc7abc9e3b39803fULL,
                                       0x3e5ade156a5dcb37ULL, 0x3e928af3fca7ab0cULL, 0x3ec71dee623fde64ULL,
                                       0x3efa01997c89e6b0ULL, 0x3f2a01a014761f6eULL, 0x3f56c16c1852b7b0ULL,
                                       0x3f81111111122322ULL, 0x3fa55555555502a1ULL, 0x3fc5555555555511ULL,
                                       0x3fe000000000000bULL};
#pragma unroll
  for (int i = 0; i < 15; ++i) {
    K.k[i] = __longlong_as_double((long long)bits[i]);
    asm volatile("" : "+v"(K.k[i]));   // opaque: a value in a vector register, not a literal to be re-created at its uses
  }
  return K;
}
__device__ __forceinline__ double exp_neg_k(double x, const ExpNegK& K) {   // exp_neg(), operation for operation
  const double xc = __builtin_fmin(__builtin_fmax(x, K.k[0]), K.k[1]);
  const double n = __builtin_rint(xc * K.k[2]);
  double r = __builtin_fma(n, K.k[3], -xc);
  r = __builtin_fma(n, K.k[4], r);
  double q = r * K.k[5] + K.k[6];
#pragma unroll
  for (int i = 7; i < 15; ++i) q = __builtin_fma(r, q, K.k[i]);
  q = __builtin_fma(r, q, 1.0);
  q = __builtin_fma(r, q, 1.0);
  return __builtin_amdgcn_ldexp(q, (int)n);
}
__device__ __forceinline__ double exp_neg_k(double x, const NoExpK&) { return exp_neg(x); }

// Transition rate exp(dH) ** .5 (markov_jump_hmc.py:341-347).  Where exp(dH) is a normal number the rate is
// evaluated as exp(dH / 2) in one polynomial pass (within 1 ulp of the two-step value).  Where exp(dH)
// overflows (-> inf -> the non-finite abort), is subnormal (its square root then has the reference's coarse
// rounding) or is 0, and for NaN, the literal two-step form runs: thresholds and special values are exactly
// those of the reference expression.
// SC: the polynomial's constants in scalar registers (one particle per wave: the kernel is bound by its vector
// instruction count, and hipcc's own Horner step is three vector instructions)
template <bool SC = false>
__device__ __forceinline__ double jump_rate(double dH) {
  if (!(dH > -708.0 && dH < 709.0)) return sqrt(exp(dH));
  return exp_normal<true, SC>(0.5 * dH);
}

__device__ __forceinline__ double wait_time(double rate, double e, bool& bad) {
  // utils.py:37-48: rate == 0 -> inf; finite -> exponential(scale=1/rate) == (1/rate)*std_exp; else error
  if (rate == 0.0) return __builtin_huge_val();
  if (!isfinite(rate)) {
    bad = true;
    return __builtin_nan("");
  }
  return (1.0 / rate) * e;
}

// np.argmin over rows (first occurrence; a NaN wins as soon as it is met)
__device__ __forceinline__ int first_min3(double a, double b, double c) {
  int k = 0;
  double best = a;
  if (!(best != best)) {
    if (b < best || b != b) {
      k = 1;
      best = b;
    }
  }
  if (!(best != best)) {
    if (c < best || c != c) {
      k = 2;
      best = c;
    }
  }
  return k;
}

}  // namespace mjhmc
