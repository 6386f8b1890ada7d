// The energy functors of the built-in elementwise energies (protocol: lane_group.hpp).
#pragma once
#include "jump_math.hpp"
#include "lane_group.hpp"

namespace mjhmc {

// TestGaussian: E = sum(x^2) / (2 sigma^2), dE/dx = x / sigma^2 (distributions.py:356-362)
template <typename T>
struct IsoGaussF {
  // fused launches (several iterations per launch) exist for this energy; WHEN they are used is the host's decision
  // (schedule.hpp, select_schedule): always for the Gaussian forces, whose single iteration is HBM-bound (measured 1.03-2.7x at
  // every row size), and for the vector-pipe-bound ones only while the batch is small (launch- and latency-bound:
  // funnel 18.7 -> 12.7 us per iteration at 1000 particles; 0.93-0.99x at 10^6, where the compacted passes win)
  static constexpr bool kFuse = true;
  // the force is one multiplication by a constant: the half-kick factor is folded into it,
  // c * (x * inv_s2) -> x * (c * inv_s2)  (identical bits when sigma is a power of two, e.g. the benchmark's 1)
  static constexpr bool kLinearIso = true;
  T inv_s2;      // 1 / sigma^2
  T inv_two_s2;  // 1 / (2 sigma^2)
  using Ctx = NoCtx;
  template <int E>
  using Local = NoLocal<E>;
  template <int E>
  __device__ __forceinline__ Local<E> local(const LaneMap&) const {
    return {};
  }
  template <int E>
  __device__ __forceinline__ Ctx prep(const T (&)[E], const LaneMap&) const {
    return {};
  }
  template <int E>
  __device__ __forceinline__ T grad(T xe, int, int, const Ctx&, const Local<E>&) const {
    return xe * inv_s2;
  }
  // energy = energy_scale(group_sum(energy_lane)): lets the kernels reduce it together with the kinetic energy
  static constexpr bool kLaneEnergy = true;
  template <int E>
  __device__ __forceinline__ T energy_lane(const T (&x)[E], const LaneMap&, const Local<E>&) const {
    T s = 0;
#pragma unroll
    for (int e = 0; e < E; ++e) s = __builtin_fma(x[e], x[e], s);  // padded x are 0; sums are compared at 1e-10, not bitwise
    return s;
  }
  __device__ __forceinline__ T energy_scale(T total) const { return total * inv_two_s2; }
  template <int E>
  __device__ __forceinline__ T energy(const T (&x)[E], const LaneMap& m, const Local<E>& lc) const {
    return energy_scale(group_sum(energy_lane<E>(x, m, lc), m.G));
  }
};

// Gaussian with diagonal J: E = sum x (J x) / 2, dE/dx = Jx/2 + J^T x/2 == j_d x_d exactly
// (distributions.py:268-273)
template <typename T>
struct DiagGaussF {
  static constexpr bool kLinearIso = false;
  static constexpr bool kFuse = true;
  const T* jdiag;  // zero padded to kParamPad elements
  using Ctx = NoCtx;
  template <int E>
  struct Local {
    T j[E];
  };
  template <int E>
  __device__ __forceinline__ Local<E> local(const LaneMap& m) const {
    Local<E> lc;
#pragma unroll
    for (int e = 0; e < E; ++e) lc.j[e] = jdiag[dim_of<T, E>(m, e)];
    return lc;
  }
  template <int E>
  __device__ __forceinline__ Ctx prep(const T (&)[E], const LaneMap&) const {
    return {};
  }
  template <int E>
  __device__ __forceinline__ T grad(T xe, int e, int, const Ctx&, const Local<E>& lc) const {
    return lc.j[e] * xe;
  }
  static constexpr bool kLaneEnergy = true;
  template <int E>
  __device__ __forceinline__ T energy_lane(const T (&x)[E], const LaneMap&, const Local<E>& lc) const {
    T s = 0;
#pragma unroll
    for (int e = 0; e < E; ++e) s = __builtin_fma(x[e], lc.j[e] * x[e], s);
    return s;
  }
  __device__ __forceinline__ T energy_scale(T total) const { return total / T(2); }
  template <int E>
  __device__ __forceinline__ T energy(const T (&x)[E], const LaneMap& m, const Local<E>& lc) const {
    return energy_scale(group_sum(energy_lane<E>(x, m, lc), m.G));
  }
};

// RoughWell: E = sum x^2/(2 s1^2) + cos(2 pi x / s2); dE/dx = x/s1^2 - sin(2 pi x/s2) 2 pi/s2
// (distributions.py:295-304), operation order as written there.
template <typename T>
struct RoughWellF {
  static constexpr bool kLinearIso = false;
  static constexpr bool kFuse = true;
  T s1sq;       // scale1^2
  T two_s1sq;   // 2 scale1^2
  T s2;
  using Ctx = NoCtx;
  template <int E>
  using Local = NoLocal<E>;
  template <int E>
  __device__ __forceinline__ Local<E> local(const LaneMap&) const {
    return {};
  }
  template <int E>
  __device__ __forceinline__ Ctx prep(const T (&)[E], const LaneMap&) const {
    return {};
  }
  template <int E>
  __device__ __forceinline__ T grad(T xe, int, int, const Ctx&, const Local<E>&) const {
    const T pi = T(3.141592653589793);
    const T sn = sin(xe * T(2) * pi / s2);
    return xe / s1sq + -sn * T(2) * pi / s2;
  }
  template <int E>
  __device__ __forceinline__ T energy(const T (&x)[E], const LaneMap& m, const Local<E>&) const {
    const T pi = T(3.141592653589793);
    T s = 0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const T t = (x[e] * x[e]) / two_s1sq + cos(x[e] * T(2) * pi / s2);
      s += (dim_of<T, E>(m, e) < m.D) ? t : T(0);
    }
    return group_sum(s, m.G);
  }
};

// MultimodalGaussian as coded (distributions.py:323-335): separation vector = (2*sep, 0, ..., 0).
template <typename T>
struct MMGaussF {
  static constexpr bool kLinearIso = false;
  static constexpr bool kFuse = true;
  T sep0;  // 2 * separation
  struct Ctx {
    T common;  // exp(sum 4 S X) = exp(4 sep0 x_0)
  };
  template <int E>
  using Local = NoLocal<E>;
  template <int E>
  __device__ __forceinline__ Local<E> local(const LaneMap&) const {
    return {};
  }
  template <int E>
  __device__ __forceinline__ Ctx prep(const T (&x)[E], const LaneMap& m) const {
    const T x0 = group_bcast0(x[0], m);
    return Ctx{(T)exp(T(4) * sep0 * x0)};
  }
  template <int E>
  __device__ __forceinline__ T grad(T xe, int, int d, const Ctx& c, const Local<E>&) const {
    const T s = (d == 0) ? sep0 : T(0);
    return (T(2) * ((xe - s) * c.common + s + xe)) / (c.common + T(1));
  }
  template <int E>
  __device__ __forceinline__ T energy(const T (&x)[E], const LaneMap& m, const Local<E>&) const {
    T a = 0, b = 0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const T s = (dim_of<T, E>(m, e) == 0) ? sep0 : T(0);
      a += (x[e] + s) * (x[e] + s);
      b += (x[e] - s) * (x[e] - s);
    }
    a = group_sum(a, m.G);
    b = group_sum(b, m.G);
    return -(T)log(exp(-a) + exp(-b));
  }
  // the row form (round 6; the protocol of the funnels below): the whole particle in one lane -- exp(4 sep x_0), once per
  // particle and leapfrog step, is paid once per particle instead of once per lane of its group -- and, for the relay of
  // mjhmc_fused_rows_relay_kernel, half a row per lane of a pair.  The same operations in the same order as prep / grad /
  // energy: the same bits (tests/test_gpu_fused.py, tools/fuzz_rows.py).
  static constexpr bool kRowForm = true;
  // (a float64 division per coordinate and step: the relay's saved trajectory outweighs its hand-overs from ~4 steps up --
  // 32 x 10^6, L = 5: 0.288 ms in the relay kernel, 0.308 in the group form; the funnels' break-even is 12 steps)
  static constexpr int kRelayMinL = 4;
  template <int E>
  __device__ __forceinline__ T kick(T ck, T xe, T ve, int e, int d, const Ctx& c) const {
    return __builtin_fma(ck, grad<E>(xe, e, d, c, Local<E>{}), ve);   // kick_fma's form for an energy without a scaled kick
  }
  template <int E, int G, class XK = NoExpK>
  __device__ __forceinline__ Ctx prep_rows(const T (&x)[G][E], const XK& = XK{}) const {
    return Ctx{(T)exp(T(4) * sep0 * x[0][0])};
  }
  template <int E, int G, class XK = NoExpK>
  __device__ __forceinline__ Ctx prep_rows_pair(const T (&xh)[G / 2][E], int, const XK& = XK{}) const {
    return Ctx{(T)exp(T(4) * sep0 * dpp_mov<0xA0>(xh[0][0]))};   // quad_perm [0, 0, 2, 2]: the even lane's x[0][0]
  }
  template <int E, int G>
  __device__ __forceinline__ T energy_rows(const T (&x)[G][E]) const {
    T pa[G], pb[G];
#pragma unroll
    for (int j = 0; j < G; ++j) {
      T a = 0, b = 0;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const T s = (((e / 2) * G + j) * 2 + (e % 2) == 0) ? sep0 : T(0);   // row_dim<G>(j, e) == 0
        a += (x[j][e] + s) * (x[j][e] + s);
        b += (x[j][e] - s) * (x[j][e] - s);
      }
      pa[j] = a;
      pb[j] = b;
    }
    T a, b;
    if constexpr (G == 1) { a = pa[0]; b = pb[0]; }
    else if constexpr (G == 2) { a = pa[0] + pa[1]; b = pb[0] + pb[1]; }
    else { a = (pa[0] + pa[1]) + (pa[2] + pa[3]); b = (pb[0] + pb[1]) + (pb[2] + pb[3]); }   // rows_sum
    return -(T)log(exp(-a) + exp(-b));
  }
  template <int E, int G, class XK = NoExpK>
  __device__ __forceinline__ T energy_pair(const T (&xh)[G / 2][E], int h, const XK& = XK{}) const {
    constexpr int GH = G / 2;
    T pa[GH], pb[GH];
#pragma unroll
    for (int jj = 0; jj < GH; ++jj) {
      T a = 0, b = 0;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const T s = (e == 0 && jj == 0 && h == 0) ? sep0 : T(0);   // dim 0 is the even lane's first coordinate
        a += (xh[jj][e] + s) * (xh[jj][e] + s);
        b += (xh[jj][e] - s) * (xh[jj][e] - s);
      }
      pa[jj] = a;
      pb[jj] = b;
    }
    const T ma = (GH == 1) ? pa[0] : pa[0] + pa[GH - 1], mb = (GH == 1) ? pb[0] : pb[0] + pb[GH - 1];
    const T a = ma + dpp_mov<0xB1>(ma), b = mb + dpp_mov<0xB1>(mb);   // the pair's sums: (p0 + p1) + (p2 + p3), as rows_sum
    return -(T)log(exp(-a) + exp(-b));
  }
};

// group_sum()'s pairing on the G per-lane partial sums of a particle held by ONE lane (the row form): the same bits
template <typename T, int G>
__device__ __forceinline__ T rows_sum(const T (&p)[G]) {
  static_assert(G == 1 || G == 2 || G == 4, "groups inside a quad");
  if constexpr (G == 1) return p[0];
  else if constexpr (G == 2) return p[0] + p[1];
  else return (p[0] + p[1]) + (p[2] + p[3]);
}
// prep() of the two funnels on a whole row: lane j's partial sum exactly as prep() forms it, the partials paired as
// group_sum pairs them, exp(-x0) once per particle (prep() spends the instructions in all G lanes of the group)
template <class Ctx, typename T, int E, int G, class XK = NoExpK>
__device__ __forceinline__ Ctx funnel_prep_rows(const T (&x)[G][E], const XK& xk = XK{}) {
  T part[G];
#pragma unroll
  for (int j = 0; j < G; ++j) {
    T s = (j == 0) ? T(0) : x[j][0] * x[j][0];
#pragma unroll
    for (int e = 1; e < E; ++e) s = __builtin_fma(x[j][e], x[j][e], s);
    part[j] = s;
  }
  Ctx c;
  c.S = rows_sum<T, G>(part);
  c.x0 = x[0][0];
  if constexpr (sizeof(T) == 8) c.ex = exp_neg_k(x[0][0], xk);
  else c.ex = exp_neg(x[0][0]);
  return c;
}

// ... and on HALF a row: the two lanes of a pair hold x[j] for j in [h G/2, (h + 1) G/2), h = 0 (even lane), 1 (odd lane)
// -- the relay of mjhmc_fused_rows_relay_kernel integrates a pooled particle on two lanes.  The partial sums are formed as
// funnel_prep_rows forms them; a pair's sums meet as (p0 + p1) + (p2 + p3) in the even lane and (p2 + p3) + (p0 + p1) in
// the odd one (G = 2: p0 + p1 / p1 + p0) -- the same bits, a floating-point sum does not depend on the order of its TWO terms.
template <class Ctx, typename T, int E, int G, class XK = NoExpK>
__device__ __forceinline__ Ctx funnel_prep_pair(const T (&xh)[G / 2][E], int h, const XK& xk = XK{}) {
  constexpr int GH = G / 2;
  static_assert(G == 2 || G == 4, "a row in two halves");
  T part[GH];
#pragma unroll
  for (int jj = 0; jj < GH; ++jj) {
    T s = xh[jj][0] * xh[jj][0];
    if (jj == 0) s = (h == 0) ? T(0) : s;   // (dim 0 is not part of the sum)
#pragma unroll
    for (int e = 1; e < E; ++e) s = __builtin_fma(xh[jj][e], xh[jj][e], s);
    part[jj] = s;
  }
  const T mine = (GH == 1) ? part[0] : part[0] + part[GH - 1];
  Ctx c;
  c.S = mine + dpp_mov<0xB1>(mine);          // quad_perm [1, 0, 3, 2]: the pair's other lane
  c.x0 = dpp_mov<0xA0>(xh[0][0]);            // quad_perm [0, 0, 2, 2]: the even lane's x[0][0]
  if constexpr (sizeof(T) == 8) c.ex = exp_neg_k(c.x0, xk);
  else c.ex = exp_neg(c.x0);
  return c;
}

// Neal's funnel, x0 ~ N(0, s^2), x_k ~ N(0, e^{x0}) (tf_distributions.py:143-147):
// E = x0^2/(2 s^2) + e^{-x0} sum_k x_k^2 / 2 + (D-1) x0 / 2
template <typename T>
struct FunnelNealF {
  static constexpr bool kLinearIso = false;
  static constexpr bool kFuse = true;
  static constexpr int kWavesRow64 = 3;  // JumpWaves
  T inv_s2;      // 1/scale^2
  T half_dm1;    // (D-1)/2
  struct Ctx {
    T x0, ex, S;  // x_0, exp(-x_0), sum_{k>=1} x_k^2
  };
  template <int E>
  using Local = NoLocal<E>;
  template <int E>
  __device__ __forceinline__ Local<E> local(const LaneMap&) const {
    return {};
  }
  template <int E>
  __device__ __forceinline__ Ctx prep(const T (&x)[E], const LaneMap& m) const {
    T s = (m.j == 0) ? T(0) : x[0] * x[0];  // only (lane 0, element 0) is dim 0
#pragma unroll
    for (int e = 1; e < E; ++e) s = __builtin_fma(x[e], x[e], s);
    Ctx c;
    c.S = group_sum(s, m.G);
    c.x0 = group_bcast0(x[0], m);
    // exp(-x0) in the lane that holds x0, then to its group: the other lanes idle through the ~25 instructions instead of
    // repeating them (same value; C4 runs 8 % higher clocks for it at 2 % less power -- and only 0.4 % faster: the kernel
    // is not bound by its clock)
    T ex0 = T(0);
    if (m.j == 0) ex0 = exp_neg(x[0]);
    c.ex = group_bcast0(ex0, m);
    return c;
  }
  template <int E>
  __device__ __forceinline__ T grad(T xe, int e, int d, const Ctx& c, const Local<E>&) const {
    return (e == 0 && d == 0) ? (c.x0 * inv_s2 - T(0.5) * c.ex * c.S + half_dm1) : xe * c.ex;
  }
  // v += ck * dE/dx as ONE multiply-add per coordinate: the force of x_k is x_k * exp(-x0), and ck * exp(-x0) is shared
  // by the whole particle (counter-RNG trajectories; the replay kernels keep c * (x * ex), the reference's rounding)
  static constexpr bool kScaledKick = true;
  template <int E>
  __device__ __forceinline__ T kick(T ck, T xe, T ve, int e, int d, const Ctx& c) const {
    return (e == 0 && d == 0) ? __builtin_fma(ck, c.x0 * inv_s2 - T(0.5) * c.ex * c.S + half_dm1, ve)
                              : __builtin_fma(xe, ck * c.ex, ve);
  }
  __device__ __forceinline__ T energy_of(const Ctx& c) const {
    return c.x0 * c.x0 * (T(0.5) * inv_s2) + T(0.5) * c.ex * c.S + half_dm1 * c.x0;
  }
  template <int E>
  __device__ __forceinline__ T energy(const T (&x)[E], const LaneMap& m, const Local<E>&) const {
    return energy_of(prep(x, m));
  }
  // the row form (mjhmc_traj_rows_kernel): the whole particle in one lane, x[j] = what lane j of its group would hold
  static constexpr bool kRowForm = true;
  template <int E, int G, class XK = NoExpK>
  __device__ __forceinline__ Ctx prep_rows(const T (&x)[G][E], const XK& xk = XK{}) const {
    return funnel_prep_rows<Ctx, T, E, G, XK>(x, xk);
  }
  template <int E, int G, class XK = NoExpK>
  __device__ __forceinline__ Ctx prep_rows_pair(const T (&xh)[G / 2][E], int h, const XK& xk = XK{}) const {
    return funnel_prep_pair<Ctx, T, E, G, XK>(xh, h, xk);
  }
  template <int E, int G>
  __device__ __forceinline__ T energy_rows(const T (&x)[G][E]) const {
    return energy_of(funnel_prep_rows<Ctx, T, E, G>(x));
  }
  template <int E, int G, class XK = NoExpK>
  __device__ __forceinline__ T energy_pair(const T (&xh)[G / 2][E], int h, const XK& xk = XK{}) const {
    return energy_of(funnel_prep_pair<Ctx, T, E, G, XK>(xh, h, xk));
  }
};

// Funnel exactly as coded (tf_distributions.py:157-165): E = -(D-1) x0^2/s^2 - e^{-x0} sum_k x_k^2
template <typename T>
struct FunnelRefF {
  static constexpr bool kLinearIso = false;
  static constexpr bool kFuse = true;
  static constexpr int kWavesRow64 = 3;  // JumpWaves
  T inv_s2;
  T dm1;  // D-1
  struct Ctx {
    T x0, ex, S;
  };
  template <int E>
  using Local = NoLocal<E>;
  template <int E>
  __device__ __forceinline__ Local<E> local(const LaneMap&) const {
    return {};
  }
  template <int E>
  __device__ __forceinline__ Ctx prep(const T (&x)[E], const LaneMap& m) const {
    T s = (m.j == 0) ? T(0) : x[0] * x[0];  // only (lane 0, element 0) is dim 0
#pragma unroll
    for (int e = 1; e < E; ++e) s = __builtin_fma(x[e], x[e], s);
    Ctx c;
    c.S = group_sum(s, m.G);
    c.x0 = group_bcast0(x[0], m);
    // exp(-x0) in the lane that holds x0, then to its group: the other lanes idle through the ~25 instructions instead of
    // repeating them (same value; C4 runs 8 % higher clocks for it at 2 % less power -- and only 0.4 % faster: the kernel
    // is not bound by its clock)
    T ex0 = T(0);
    if (m.j == 0) ex0 = exp_neg(x[0]);
    c.ex = group_bcast0(ex0, m);
    return c;
  }
  template <int E>
  __device__ __forceinline__ T grad(T xe, int e, int d, const Ctx& c, const Local<E>&) const {
    return (e == 0 && d == 0) ? (T(-2) * dm1 * c.x0 * inv_s2 + c.ex * c.S) : T(-2) * xe * c.ex;
  }
  static constexpr bool kScaledKick = true;
  template <int E>
  __device__ __forceinline__ T kick(T ck, T xe, T ve, int e, int d, const Ctx& c) const {
    return (e == 0 && d == 0) ? __builtin_fma(ck, T(-2) * dm1 * c.x0 * inv_s2 + c.ex * c.S, ve)
                              : __builtin_fma(xe, ck * (T(-2) * c.ex), ve);
  }
  __device__ __forceinline__ T energy_of(const Ctx& c) const { return -(dm1 * c.x0 * c.x0 * inv_s2) - c.ex * c.S; }
  template <int E>
  __device__ __forceinline__ T energy(const T (&x)[E], const LaneMap& m, const Local<E>&) const {
    return energy_of(prep(x, m));
  }
  static constexpr bool kRowForm = true;   // as FunnelNealF
  template <int E, int G, class XK = NoExpK>
  __device__ __forceinline__ Ctx prep_rows(const T (&x)[G][E], const XK& xk = XK{}) const {
    return funnel_prep_rows<Ctx, T, E, G, XK>(x, xk);
  }
  template <int E, int G, class XK = NoExpK>
  __device__ __forceinline__ Ctx prep_rows_pair(const T (&xh)[G / 2][E], int h, const XK& xk = XK{}) const {
    return funnel_prep_pair<Ctx, T, E, G, XK>(xh, h, xk);
  }
  template <int E, int G>
  __device__ __forceinline__ T energy_rows(const T (&x)[G][E]) const {
    return energy_of(funnel_prep_rows<Ctx, T, E, G>(x));
  }
  template <int E, int G, class XK = NoExpK>
  __device__ __forceinline__ T energy_pair(const T (&xh)[G / 2][E], int h, const XK& xk = XK{}) const {
    return energy_of(funnel_prep_pair<Ctx, T, E, G, XK>(xh, h, xk));
  }
};

}  // namespace mjhmc
