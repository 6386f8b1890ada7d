// The lanes of a particle.
//
// Data layout in HBM: particle-major.  Particle p owns `pitch` consecutive elements, so the 64/G
// particles a wavefront works on are ONE contiguous span and every global access is a full
// 16 B/lane, 1 KiB/wave-instruction transaction.  G (power of two, <= 64) lanes share a particle;
// lane j holds chunks j, j+G, j+2G, ... (16-byte chunks) of X and V in registers for the whole
// iteration -- both trajectories run out of registers, reductions are xor-butterflies inside the
// G-lane group, and for G == 64 (ndims >= 256) all per-particle control flow is wave-uniform.
#pragma once
#ifndef __HIPCC_RTC__  // hipRTC pre-includes the device runtime and has no header search path to it
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

namespace mjhmc {

template <typename T>
struct VecOf;
template <>
struct VecOf<double> {
  using type = double2;
  static constexpr int n = 2;
};
template <>
struct VecOf<float> {
  using type = float4;
  static constexpr int n = 4;
};

// which dims a lane owns
struct LaneMap {
  int j;      // lane within the particle group
  int G;      // lanes per particle
  int D;      // true ndims
  int CH;     // 16-byte chunks per particle row (pitch / VEC)
  int lane0;  // wave lane index of the group's lane 0
  int wpp;    // lane mapping known at compile time: 1 = the wavefront is one particle (G == 64), 3 = a quad per particle
              // (G == 4), 6 = half a wavefront per particle (G == 32); 0 = G is a run-time value

  // the whole particle in one lane: decide() with the three clocks in one lane
  static __device__ __forceinline__ LaneMap one_lane() { return LaneMap{0, 1, 1, 1, 0, 0}; }
  // groups of G = 2^k lanes: thread `tid` (of the wave, the workgroup or the grid: groups are aligned), lane `lane` of its wave.
  // (The kernels' instruction schedules follow the order of these arguments: the lane index comes after the row's shape.)
  static __device__ __forceinline__ LaneMap group(int tid, int G, int D, int CH, int lane, int wpp = 0) {
    return LaneMap{tid & (G - 1), G, D, CH, lane & ~(G - 1), wpp};
  }
};

template <typename T, int E>
__device__ __forceinline__ int dim_of(const LaneMap& m, int e) {
  constexpr int VEC = VecOf<T>::n;
  return ((e / VEC) * m.G + m.j) * VEC + (e % VEC);
}

// ---- cross-lane primitives -------------------------------------------------------------------
// Sums inside a G-lane group run on the VALU cross-lane network (DPP quad_perm / row mirrors inside
// a 16-lane row, gfx950's v_permlane16_swap / v_permlane32_swap across rows): no LDS crossbar
// round trips (ds_bpermute), which cost ~100+ cycles of latency per butterfly step.
template <int CTRL>
__device__ __forceinline__ double dpp_mov(double v) {
  // bound_ctrl = true with full row / bank masks: every lane is written, so no zero-initialised destination
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ double swap16_sum(double v) {
  const auto lo = __builtin_amdgcn_permlane16_swap(__double2loint(v), __double2loint(v), false, false);
  const auto hi = __builtin_amdgcn_permlane16_swap(__double2hiint(v), __double2hiint(v), false, false);
  return __hiloint2double(hi[0], lo[0]) + __hiloint2double(hi[1], lo[1]);
}
__device__ __forceinline__ float swap16_sum(float v) {
  const auto r = __builtin_amdgcn_permlane16_swap(__float_as_int(v), __float_as_int(v), false, false);
  return __int_as_float(r[0]) + __int_as_float(r[1]);
}
__device__ __forceinline__ double swap32_sum(double v) {
  const auto lo = __builtin_amdgcn_permlane32_swap(__double2loint(v), __double2loint(v), false, false);
  const auto hi = __builtin_amdgcn_permlane32_swap(__double2hiint(v), __double2hiint(v), false, false);
  return __hiloint2double(hi[0], lo[0]) + __hiloint2double(hi[1], lo[1]);
}
__device__ __forceinline__ float swap32_sum(float v) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_int(v), __float_as_int(v), false, false);
  return __int_as_float(r[0]) + __int_as_float(r[1]);
}

// sum over the lanes of a group (G = 2^k <= 64, groups aligned); every lane gets the same bits.
// (A branch-free form that always runs all six levels and selects zeros was measured: slower, the
// permlane swaps cost more than the wave-uniform branches they replace.)
template <typename T>
__device__ __forceinline__ T group_sum(T v, int G) {
  if (G > 32) v = swap32_sum(v);       // other half of the wave FIRST (the order group_sum_pair reproduces)
  if (G > 1) v += dpp_mov<0xB1>(v);    // quad_perm [1,0,3,2]  : lane ^ 1
  if (G > 2) v += dpp_mov<0x4E>(v);    // quad_perm [2,3,0,1]  : lane ^ 2
  if (G > 4) v += dpp_mov<0x141>(v);   // row_half_mirror      : other quad of the 8
  if (G > 8) v += dpp_mov<0x140>(v);   // row_mirror           : other 8 of the row
  if (G > 16) v = swap16_sum(v);       // other row of the pair
  return v;
}

// v_permlane32_swap on every dword of the pair: afterwards a = [a.lower half | b.lower half], b = [a.upper | b.upper]
__device__ __forceinline__ void swap32_pair(double& a, double& b) {
  const auto lo = __builtin_amdgcn_permlane32_swap(__double2loint(a), __double2loint(b), false, false);
  const auto hi = __builtin_amdgcn_permlane32_swap(__double2hiint(a), __double2hiint(b), false, false);
  a = __hiloint2double(hi[0], lo[0]);
  b = __hiloint2double(hi[1], lo[1]);
}
__device__ __forceinline__ void swap32_pair(float& a, float& b) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_int(a), __float_as_int(b), false, false);
  a = __int_as_float(r[0]);
  b = __int_as_float(r[1]);
}

// group_sum of TWO values at once.  With a wavefront per particle the two reductions share their ladder: one half-wave
// swap leaves a's pair sums in lanes 0..31 and b's in lanes 32..63, five levels reduce both inside their halves, one
// more swap hands each total to the other half -- 24 vector instructions in float64 instead of 44, and bit for bit
// what two group_sum calls return (same pairing at every level).
template <typename T>
__device__ __forceinline__ void group_sum_pair(T a, T b, int G, T& ta, T& tb) {
  if (G == 64) {
    swap32_pair(a, b);  // a = [a_l | b_l], b = [a_{l+32} | b_{l+32}]
    T c = a + b;
    c += dpp_mov<0xB1>(c);
    c += dpp_mov<0x4E>(c);
    c += dpp_mov<0x141>(c);
    c += dpp_mov<0x140>(c);
    c = swap16_sum(c);
    ta = c;
    tb = c;
    swap32_pair(ta, tb);  // ta = [total a | total a], tb = [total b | total b]
  } else {
    ta = group_sum(a, G);
    tb = group_sum(b, G);
  }
}

// value held by lane `r` of the caller's group
__device__ __forceinline__ double readlane_v(double v, int r) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), r), __builtin_amdgcn_readlane(__double2loint(v), r));
}
__device__ __forceinline__ float readlane_v(float v, int r) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), r));
}

template <typename T>
__device__ __forceinline__ T group_lane(T v, const LaneMap& m, int r) {
  if (m.wpp == 1) return readlane_v(v, r);  // v_readlane: no LDS-crossbar round trip
  if (m.wpp == 6) {                         // half a wavefront per particle: both halves' lane r, then this lane's half
    const T lo = readlane_v(v, r), hi = readlane_v(v, 32 + r);
    return m.lane0 ? hi : lo;
  }
  if (m.wpp == 3) {                         // lane r of the quad: one DPP quad_perm broadcast
    switch (r) {
      case 0: return dpp_mov<0x00>(v);
      case 1: return dpp_mov<0x55>(v);
      case 2: return dpp_mov<0xAA>(v);
      default: return dpp_mov<0xFF>(v);
    }
  }
  return __shfl(v, m.lane0 + r);
}

// value of the group's lane 0.  Groups of <= 4 lanes sit inside one quad: a DPP quad_perm broadcast
// (VALU, no LDS crossbar round trip); wider groups go through ds_bpermute.
template <typename T>
__device__ __forceinline__ T group_bcast0(T v, const LaneMap& m) {
  if (m.G == 1) return v;
  if (m.G == 2) return dpp_mov<0xA0>(v);  // quad_perm [0,0,2,2]
  if (m.G == 4) return dpp_mov<0x00>(v);  // quad_perm [0,0,0,0]
  return __shfl(v, m.lane0);
}

// Dense energies (tile kernels): the particles whose inverse-L cache will be cold in the NEXT iteration are known when the
// jump kernel has decided -- every move but L clears the cache (markov_jump_hmc.py:398-412) -- so the lanes that decided
// (one per particle) append them to the next iteration's compacted list right there: one atomic per tile.  Called under
// divergent control flow; `cold` lanes must be active.
__device__ __forceinline__ void append_cold(int* list, int* count, bool cold, int64_t p) {
  const unsigned long long m = __ballot(cold);
  if (m == 0ull) return;
  const int lane = threadIdx.x & 63;
  const int first = __ffsll((long long)m) - 1;
  int base = 0;
  if (lane == first) base = atomicAdd(count, (int)__popcll(m));
  base = __shfl(base, first);
  if (cold) list[base + (int)__popcll(m & ((1ull << lane) - 1ull))] = (int)p;
}

// ------------------------------------------------------------------------------------------
// energy functors.  Protocol (E = elements per lane):
//   Local<E> local<E>(m)              per-lane constants, loaded once per kernel
//   Ctx      prep(x, m)               per-evaluation context (may reduce over the group)
//   T        grad(xe, e, d, ctx, lc)  dE/dx_d for the lane's element e (dim d)
//   T        energy(x, m, lc)         E(x), reduced over the group, valid in every lane
// Padded elements (d >= D) hold x = 0 and must produce grad = 0; energy() masks them.
// ------------------------------------------------------------------------------------------

struct NoCtx {};
template <int E>
struct NoLocal {};

}  // namespace mjhmc
