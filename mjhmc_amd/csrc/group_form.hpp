// The group form: a particle's row in the registers of its G lanes -- row and stash I/O, the trajectory, the energies of a
// state, the momentum refresh, slot-relative access of the persistent jump kernel.
//
// Floating-point contraction is OFF for this translation unit (see Makefile): the leapfrog
// update is evaluated as the reference writes it (mul, then add), which makes X and V
// bit-identical to the NumPy path for linear forces.
#pragma once
#ifndef __HIPCC_RTC__  // hipRTC pre-includes the device runtime and has no header search path to it
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#include "lane_group.hpp"
#include "philox.hpp"

#ifndef MJHMC_NT
#define MJHMC_NT 1  // streaming (nontemporal) row loads/stores: +1-2 % on C2, state rows are touched once per launch
#endif

namespace mjhmc {

template <typename T, int E>
__device__ __forceinline__ void load_row(const T* row, const LaneMap& m, T (&r)[E]) {
  using V = typename VecOf<T>::type;
  constexpr int VEC = VecOf<T>::n;
#pragma unroll
  for (int c = 0; c < E / VEC; ++c) {
    const int chunk = c * m.G + m.j;
    V v;
    if (chunk < m.CH) {
      v = *reinterpret_cast<const V*>(row + (size_t)chunk * VEC);
    } else {
      if constexpr (VEC == 2) v = V{0, 0};
      else v = V{0, 0, 0, 0};
    }
    if constexpr (VEC == 2) {
      r[c * 2] = v.x;
      r[c * 2 + 1] = v.y;
    } else {
      r[c * 4] = v.x;
      r[c * 4 + 1] = v.y;
      r[c * 4 + 2] = v.z;
      r[c * 4 + 3] = v.w;
    }
  }
}

template <typename T, int E>
__device__ __forceinline__ void store_row(T* row, const LaneMap& m, const T (&r)[E]) {
  using V = typename VecOf<T>::type;
  constexpr int VEC = VecOf<T>::n;
#pragma unroll
  for (int c = 0; c < E / VEC; ++c) {
    const int chunk = c * m.G + m.j;
    if (chunk < m.CH) {
      V v;
      if constexpr (VEC == 2) v = V{r[c * 2], r[c * 2 + 1]};
      else v = V{r[c * 4], r[c * 4 + 1], r[c * 4 + 2], r[c * 4 + 3]};
      *reinterpret_cast<V*>(row + (size_t)chunk * VEC) = v;
    }
  }
}

// per-wave LDS stripe [C][64] of 16-byte chunks
template <typename T, int E>
__device__ __forceinline__ void stash_put(typename VecOf<T>::type (*st)[64], int lane, const T (&r)[E]) {
  using V = typename VecOf<T>::type;
  constexpr int VEC = VecOf<T>::n;
#pragma unroll
  for (int c = 0; c < E / VEC; ++c) {
    if constexpr (VEC == 2) st[c][lane] = V{r[c * 2], r[c * 2 + 1]};
    else st[c][lane] = V{r[c * 4], r[c * 4 + 1], r[c * 4 + 2], r[c * 4 + 3]};
  }
}

template <typename T, int E>
__device__ __forceinline__ void stash_get(typename VecOf<T>::type (*st)[64], int lane, T (&r)[E]) {
  using V = typename VecOf<T>::type;
  constexpr int VEC = VecOf<T>::n;
#pragma unroll
  for (int c = 0; c < E / VEC; ++c) {
    const V q = st[c][lane];
    if constexpr (VEC == 2) {
      r[c * 2] = q.x;
      r[c * 2 + 1] = q.y;
    } else {
      r[c * 4] = q.x;
      r[c * 4 + 1] = q.y;
      r[c * 4 + 2] = q.z;
      r[c * 4 + 3] = q.w;
    }
  }
}

// c * dE/dx_d: the half-kick product of hmc_state.py:88,91
template <class En, typename T, int E, class Ctx, class Lc>
__device__ __forceinline__ T kick_product(const En& en, T c, T xe, int e, int d, const Ctx& ctx, const Lc& lc) {
  if constexpr (En::kLinearIso) return xe * (c * en.inv_s2);
  else return c * en.template grad<E>(xe, e, d, ctx, lc);
}

// v += c * dE/dx_d as one fused multiply-add
template <class En>
struct HasScaledKick {
  template <class U>
  static auto test(int) -> decltype(U::kScaledKick, char());
  template <class U>
  static long test(...);
  static constexpr bool value = sizeof(test<En>(0)) == 1;
};

template <class En, typename T, int E, class Ctx, class Lc>
__device__ __forceinline__ T kick_fma(const En& en, T c, T xe, T ve, int e, int d, const Ctx& ctx, const Lc& lc) {
  if constexpr (En::kLinearIso) return __builtin_fma(xe, c * en.inv_s2, ve);
  else if constexpr (HasScaledKick<En>::value) return en.template kick<E>(c, xe, ve, e, d, ctx);  // force = xe * scale(ctx) for most elements
  else return __builtin_fma(c, en.template grad<E>(xe, e, d, ctx, lc), ve);
}

// M leapfrog steps, in place (hmc_state.py:86-100).
// EXACT = true (the replay kernels, i.e. the golden-vector path): the reference's literal operation order --
// half kicks NOT merged, every product rounded before its sum (the library is built with -ffp-contract=off);
// c*g of the closing kick is reused by the next opening kick (same product).  For forces that are exact
// products this reproduces NumPy's X and V bit for bit.
// EXACT = false (counter-RNG kernels): the same integrator with the two half kicks between consecutive steps
// merged into one (what the reference's compiled variant does, fast/hmc.py:6-98) and every update a single
// fused multiply-add: 2 + grad instead of 5 + grad vector instructions per element and step.  Differs from the
// literal order by rounding only (~1e-16 relative per step, inside the 1e-10 parity bar; the tests compare it
// with the oracle's literal order on the same Philox streams).
template <class En, typename T, int E, bool EXACT>
__device__ __forceinline__ void trajectory(const En& en, const typename En::template Local<E>& lc, const LaneMap& m,
                                           T (&x)[E], T (&v)[E], int L, T eps, T chalf) {
  if constexpr (EXACT) {
    T cg[E];
    {
      const auto ctx = en.prep(x, m);
#pragma unroll
      for (int e = 0; e < E; ++e) cg[e] = kick_product<En, T, E>(en, chalf, x[e], e, dim_of<T, E>(m, e), ctx, lc);
    }
    for (int s = 0; s < L; ++s) {
#pragma unroll
      for (int e = 0; e < E; ++e) {
        v[e] = v[e] + cg[e];
        x[e] = x[e] + eps * v[e];
      }
      const auto ctx = en.prep(x, m);
#pragma unroll
      for (int e = 0; e < E; ++e) {
        cg[e] = kick_product<En, T, E>(en, chalf, x[e], e, dim_of<T, E>(m, e), ctx, lc);
        v[e] = v[e] + cg[e];
      }
    }
  } else {
    if (L <= 0) return;
    {
      const auto ctx = en.prep(x, m);
#pragma unroll
      for (int e = 0; e < E; ++e) v[e] = kick_fma<En, T, E>(en, chalf, x[e], v[e], e, dim_of<T, E>(m, e), ctx, lc);
    }
    const T cfull = chalf + chalf;
    for (int s = 0; s < L; ++s) {
#pragma unroll
      for (int e = 0; e < E; ++e) x[e] = __builtin_fma(eps, v[e], x[e]);
      const auto ctx = en.prep(x, m);
      const T c = (s == L - 1) ? chalf : cfull;  // the closing kick of the trajectory is a half kick
#pragma unroll
      for (int e = 0; e < E; ++e) v[e] = kick_fma<En, T, E>(en, c, x[e], v[e], e, dim_of<T, E>(m, e), ctx, lc);
    }
  }
}

template <typename T, int E>
__device__ __forceinline__ T kinetic(const T (&v)[E], const LaneMap& m) {
  T s = 0;
#pragma unroll
  for (int e = 0; e < E; ++e) s = __builtin_fma(v[e], v[e], s);
  return group_sum(s, m.G) / T(2);  // hmc_state.py:50
}

// EV = kinetic(v) and EX = en.energy(x) of one state, the same bits as the two calls; energies that are a scaled group
// sum (kLaneEnergy) share one reduction ladder with the kinetic energy
template <class En, typename = void>
struct HasLaneEnergy {
  static constexpr bool value = false;
};
template <class En>
struct HasLaneEnergy<En, decltype((void)En::kLaneEnergy)> {
  static constexpr bool value = true;
};
template <class En, typename T, int E, class LC>
__device__ __forceinline__ void state_energies(const En& en, const LC& lc, const LaneMap& m, const T (&x)[E], const T (&v)[E],
                                               T& EX, T& EV) {
  if constexpr (HasLaneEnergy<En>::value) {
    T sv = 0;
#pragma unroll
    for (int e = 0; e < E; ++e) sv = __builtin_fma(v[e], v[e], sv);
    const T sx = en.template energy_lane<E>(x, m, lc);
    T tv, tx;
    group_sum_pair(sv, sx, m.G, tv, tx);
    EV = tv / T(2);
    EX = en.energy_scale(tx);
  } else {
    EV = kinetic<T, E>(v, m);
    EX = en.energy(x, m, lc);
  }
}

// momentum-refresh noise for this lane's dims (hmc_state.py:125): replayed or counter RNG
template <typename T, int E>
__device__ __forceinline__ void refresh_noise(const T* noise_row, const RngKey& key, uint32_t pid, const LaneMap& m,
                                              T (&z)[E]) {
  constexpr int VEC = VecOf<T>::n;
  if (noise_row) {
    load_row<T, E>(noise_row, m, z);
    return;
  }
#pragma unroll
  for (int c = 0; c < E / VEC; ++c) {
    const int chunk = c * m.G + m.j;
#pragma unroll
    for (int h = 0; h < VEC / 2; ++h) {
      const int d = chunk * VEC + 2 * h;
      double z0 = 0.0, z1 = 0.0;
      if (chunk < m.CH && d < m.D) normal_pair(key, pid, (uint32_t)(d >> 1), z0, z1);
      z[c * VEC + 2 * h] = (T)z0;
      z[c * VEC + 2 * h + 1] = (d + 1 < m.D) ? (T)z1 : T(0);
    }
  }
}

// HMCState.R on the stashed momentum, chunk by chunk: v <- v*sqrt(1-beta) + n*sqrt(beta)
// (hmc_state.py:125-126).  The chunk loop is deliberately NOT unrolled: one Box-Muller pair's
// temporaries at a time keeps this rare branch from dictating the kernel's register budget.
template <typename T, int E, bool REPLAY>
__device__ __forceinline__ void refresh_stash(typename VecOf<T>::type (*st)[64], int lane, const T* noise_row,
                                              const RngKey& key, uint32_t pid, const LaneMap& m, T keep, T mix) {
  using V = typename VecOf<T>::type;
  constexpr int VEC = VecOf<T>::n;
#pragma unroll 1
  for (int c = 0; c < E / VEC; ++c) {
    const int chunk = c * m.G + m.j;
    if (chunk >= m.CH) continue;  // stays zero
    const V v0 = st[c][lane];
    V z;
    if constexpr (REPLAY) {
      z = *reinterpret_cast<const V*>(noise_row + (size_t)chunk * VEC);
    } else {
      const int d = chunk * VEC;
      double z0, z1;
      normal_pair(key, pid, (uint32_t)(d >> 1), z0, z1);
      z.x = (T)z0;
      z.y = (d + 1 < m.D) ? (T)z1 : T(0);
      if constexpr (VEC == 4) {
        double z2 = 0.0, z3 = 0.0;
        if (d + 2 < m.D) normal_pair(key, pid, (uint32_t)((d + 2) >> 1), z2, z3);
        z.z = (T)z2;
        z.w = (d + 3 < m.D) ? (T)z3 : T(0);
      }
    }
    V r;
    r.x = v0.x * keep + z.x * mix;
    r.y = v0.y * keep + z.y * mix;
    if constexpr (VEC == 4) {
      r.z = v0.z * keep + z.z * mix;
      r.w = v0.w * keep + z.w * mix;
    }
    st[c][lane] = r;
  }
}

// per-particle scalars travelling with a slot
template <typename T>
struct SlotScalars {
  T EX, EV, Hflf;  // Hflf is NaN <=> the inverse-L cache of this particle is cold
};

// pins the first use of a prefetched value to this program point (otherwise the scheduler may pull
// the use -- and with it a vmcnt wait that drains the whole prefetch -- up to the load)
__device__ __forceinline__ void use_here(double& v) { asm volatile("" : "+v"(v)); }
__device__ __forceinline__ void use_here(float& v) { asm volatile("" : "+v"(v)); }

// Slot-relative row access.  A slot's 64/G particles are one contiguous span, so the address is
// (wave-uniform slot base) + (per-lane constant byte offset) + c * (uniform chunk stride): the
// per-slot address arithmetic is scalar, the vector part never changes.
template <typename T, int E, bool FULLROW>
__device__ __forceinline__ void slot_load(const char* base, uint32_t lane_off, uint32_t chunk_stride, const LaneMap& m,
                                          T (&r)[E]) {
  using V = typename VecOf<T>::type;
  constexpr int VEC = VecOf<T>::n;
#pragma unroll
  for (int c = 0; c < E / VEC; ++c) {
    V v;
    if (FULLROW || c * m.G + m.j < m.CH) {
#if MJHMC_NT
      {
        using NV = T __attribute__((ext_vector_type(VecOf<T>::n)));
        const NV q = __builtin_nontemporal_load(reinterpret_cast<const NV*>(base + lane_off + c * chunk_stride));
        if constexpr (VEC == 2) v = V{q[0], q[1]};
        else v = V{q[0], q[1], q[2], q[3]};
      }
#else
      v = *reinterpret_cast<const V*>(base + lane_off + c * chunk_stride);
#endif
    } else {
      if constexpr (VEC == 2) v = V{0, 0};
      else v = V{0, 0, 0, 0};
    }
    if constexpr (VEC == 2) {
      r[c * 2] = v.x;
      r[c * 2 + 1] = v.y;
    } else {
      r[c * 4] = v.x;
      r[c * 4 + 1] = v.y;
      r[c * 4 + 2] = v.z;
      r[c * 4 + 3] = v.w;
    }
  }
}

template <typename T, int E, bool FULLROW>
__device__ __forceinline__ void slot_store(char* base, uint32_t lane_off, uint32_t chunk_stride, const LaneMap& m,
                                           const T (&r)[E]) {
  using V = typename VecOf<T>::type;
  constexpr int VEC = VecOf<T>::n;
#pragma unroll
  for (int c = 0; c < E / VEC; ++c) {
    if (FULLROW || c * m.G + m.j < m.CH) {
      V v;
      if constexpr (VEC == 2) v = V{r[c * 2], r[c * 2 + 1]};
      else v = V{r[c * 4], r[c * 4 + 1], r[c * 4 + 2], r[c * 4 + 3]};
#if MJHMC_NT
      {
        using NV = T __attribute__((ext_vector_type(VecOf<T>::n)));
        NV q;
        if constexpr (VEC == 2) q = NV{v.x, v.y};
        else q = NV{v.x, v.y, v.z, v.w};
        __builtin_nontemporal_store(q, reinterpret_cast<NV*>(base + lane_off + c * chunk_stride));
      }
#else
      *reinterpret_cast<V*>(base + lane_off + c * chunk_stride) = v;
#endif
    }
  }
}

}  // namespace mjhmc
