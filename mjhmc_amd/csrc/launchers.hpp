// Host launchers of the elementwise kernels: the instance selection and the grids, and the macro that defines an energy's
// eight launchers (launcher_decls.hpp) in its translation unit.
#pragma once
#ifndef __HIPCC_RTC__  // host side only
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "jump_kernel.hpp"
#include "launcher_decls.hpp"
#include "row_form.hpp"
#include "step_kernel.hpp"

namespace mjhmc {

// Persistent launch: as many 256-thread blocks as the device keeps resident for this kernel
// (occupancy query, cached per instantiation), never more than there are slots to hand out.
template <class En, typename T, int E, int MODE, bool REPLAY, bool FULLROW, int WPP = 0, bool FUSED = false>
inline void launch_jump_r(const JumpArgs<T>& a, const En& en, hipStream_t st) {
  static int resident_blocks = 0;
  if (resident_blocks == 0) {
    int dev = 0, per_cu = 0, cus = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, mjhmc_jump_kernel<En, T, E, MODE, REPLAY, FULLROW, WPP, FUSED>,
                                                       256, 0);
    resident_blocks = std::max(1, per_cu) * std::max(1, cus);
  }
  const int64_t nslots = a.Npad >> (6 - a.logG);
  const int64_t want = (nslots + 3) / 4;
  const unsigned grid = (unsigned)std::min<int64_t>(want, resident_blocks);
  hipLaunchKernelGGL((mjhmc_jump_kernel<En, T, E, MODE, REPLAY, FULLROW, WPP, FUSED>), dim3(grid), dim3(256), 0, st, a, en);
}

// persistent: as many one-wave workgroups as the device keeps resident (one per SIMD), never more than there are tiles.
// The product's form is the relay kernel (four-wave workgroups, one per CU, the workgroup's cold caches pooled); the
// one-wave form stays as the test build's A/B partner (kAbNoRelay) -- the two must agree bit for bit.
template <class En, typename T, int E, int LOGG, bool FULL>
inline void launch_fused_rows(const JumpArgs<T>& a, const En& en, hipStream_t st) {
  static int resident_blocks = 0, resident_relay = 0;
  if (resident_blocks == 0) {
    int dev = 0, per_cu = 0, per_cu_relay = 0, cus = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, mjhmc_fused_rows_kernel<En, T, E, LOGG, FULL>, 64, 0);
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_relay, mjhmc_fused_rows_relay_kernel<En, T, E, LOGG, FULL>,
                                                       64 * kRelayWaves, 0);
    resident_blocks = std::max(1, per_cu) * std::max(1, cus);
    resident_relay = std::max(1, per_cu_relay) * std::max(1, cus);
  }
  const int64_t tiles = a.Npad >> 6;
  // The relay trades a trajectory per wave and iteration for a quarter of one + four hand-overs through LDS: it wins from
  // ~12 leapfrog steps up (tools/sweep_L.py 32 1000000 funnel, profiles/r06/sweep_L_c4.txt: relay 0.110 + 0.0045 L ms per
  // iteration, one-wave kernel 0.071 + 0.0078 L); shorter trajectories keep the one-wave kernel.  The same bits either way.
  const bool relay = (a.ab & kAbForceRelay) || (!(a.ab & kAbNoRelay) && a.L >= RelayMinL<En>::value);
  if (relay) {
    const unsigned grid = (unsigned)std::min<int64_t>((tiles + kRelayWaves - 1) / kRelayWaves, resident_relay);
    hipLaunchKernelGGL((mjhmc_fused_rows_relay_kernel<En, T, E, LOGG, FULL>), dim3(grid), dim3(64 * kRelayWaves), 0, st, a, en);
    return;
  }
  const unsigned grid = (unsigned)std::min<int64_t>(tiles, resident_blocks);
  hipLaunchKernelGGL((mjhmc_fused_rows_kernel<En, T, E, LOGG, FULL>), dim3(grid), dim3(64), 0, st, a, en);
}

// Replay needs every recorded stream of the mode; it is a test path and exists only in the
// predicated (non-FULLROW) form, as do the control-arm samplers.
template <class En, typename T, int E>
inline void launch_jump_t(const JumpArgs<T>& a, const En& en, hipStream_t st) {
  const bool full = a.CH == (E / VecOf<T>::n) << a.logG;
  const bool replay = a.noise != nullptr;
  if constexpr (En::kFuse) if (a.n_fuse > 0) {  // several iterations per launch (counter RNG only)
    if constexpr (HasRowForm<En>::value && sizeof(T) == 8 && E == 8) {
      if (fused_rows_shape(a.mode, a.logG, a.ab)) {   // a lane per particle (mjhmc_fused_rows_kernel)
        const bool full_row = a.CH == 4 << a.logG;
        if (a.logG == 2 && full_row) launch_fused_rows<En, T, E, 2, true>(a, en, st);
        else if (a.logG == 2) launch_fused_rows<En, T, E, 2, false>(a, en, st);
        else if (full_row) launch_fused_rows<En, T, E, 1, true>(a, en, st);
        else launch_fused_rows<En, T, E, 1, false>(a, en, st);
        return;
      }
    }
    if (a.mode == kModeMJHMC) {
      if (full && a.logG == 6 && !(a.ab & kAbNoBlockDecide)) launch_jump_r<En, T, E, kModeMJHMC, false, true, 5, true>(a, en, st);
      else if (full && a.logG == 5 && !(a.ab & kAbNoBlockDecide)) launch_jump_r<En, T, E, kModeMJHMC, false, true, 6, true>(a, en, st);
      else if (full && a.logG == 6) launch_jump_r<En, T, E, kModeMJHMC, false, true, 1, true>(a, en, st);
      else if (full && a.logG == 2 && !(a.ab & kAbNoQuad)) launch_jump_r<En, T, E, kModeMJHMC, false, true, 3, true>(a, en, st);
      else if (full) launch_jump_r<En, T, E, kModeMJHMC, false, true, 0, true>(a, en, st);
      else launch_jump_r<En, T, E, kModeMJHMC, false, false, 0, true>(a, en, st);
    } else if (a.mode == kModeCT) {
      launch_jump_r<En, T, E, kModeCT, false, false, 0, true>(a, en, st);
    } else {
      launch_jump_r<En, T, E, kModeControl, false, false, 0, true>(a, en, st);
    }
    return;
  }
  if (a.mode == kModeMJHMC) {
    if (replay) launch_jump_r<En, T, E, kModeMJHMC, true, false>(a, en, st);
    else if (full && a.logG == 6 && !(a.ab & kAbNoWpp)) launch_jump_r<En, T, E, kModeMJHMC, false, true, 1>(a, en, st);
    else if (full && a.logG == 2 && !(a.ab & kAbNoQuad)) launch_jump_r<En, T, E, kModeMJHMC, false, true, 3>(a, en, st);
    else if (full) launch_jump_r<En, T, E, kModeMJHMC, false, true>(a, en, st);
    else launch_jump_r<En, T, E, kModeMJHMC, false, false>(a, en, st);
  } else if (a.mode == kModeCT) {
    if (replay) launch_jump_r<En, T, E, kModeCT, true, false>(a, en, st);
    else launch_jump_r<En, T, E, kModeCT, false, false>(a, en, st);
  } else {
    if (replay) launch_jump_r<En, T, E, kModeControl, true, false>(a, en, st);
    else launch_jump_r<En, T, E, kModeControl, false, false>(a, en, st);
  }
}

// trajectories: one workgroup per 256 >> logG particles + the list's walkers in front; jump process: one per 256 x kDecideSub particles
template <class En, typename T, int E>
inline void launch_step_t(const TrajArgs<T>* ta, const JumpDecideArgs<T>* da, const En& en, hipStream_t st) {
  int n_traj = 0, n_decide = 0;
  if (ta) {
    const int64_t ppb = 256 >> ta->logG;
    n_traj = (int)((ta->N + ppb - 1) / ppb) + ta->inv_blocks;
  }
  if (da) n_decide = (int)((da->N + 256 * kDecideSub - 1) / (256 * kDecideSub));
  if constexpr (HasRowForm<En>::value && sizeof(T) == 8 && E == 8) {
    if (ta && !da && ta->rows && (ta->logG == 1 || ta->logG == 2)) {   // a lane per particle, a wavefront per workgroup
      const int64_t fwd = (ta->N + 63) / 64;
      const int n_walk = (int)std::max<int64_t>(1, std::min<int64_t>(fwd / 8, 4096));
      const dim3 grid((unsigned)(fwd + n_walk));
      const bool full = ta->CH == 4 << ta->logG;
      if (ta->logG == 2 && full) hipLaunchKernelGGL((mjhmc_traj_rows_kernel<En, T, E, 2, true>), grid, dim3(64), 0, st, *ta, en, n_walk);
      else if (ta->logG == 2) hipLaunchKernelGGL((mjhmc_traj_rows_kernel<En, T, E, 2, false>), grid, dim3(64), 0, st, *ta, en, n_walk);
      else if (full) hipLaunchKernelGGL((mjhmc_traj_rows_kernel<En, T, E, 1, true>), grid, dim3(64), 0, st, *ta, en, n_walk);
      else hipLaunchKernelGGL((mjhmc_traj_rows_kernel<En, T, E, 1, false>), grid, dim3(64), 0, st, *ta, en, n_walk);
      return;
    }
  }
  const TrajArgs<T> t = ta ? *ta : TrajArgs<T>{};
  const JumpDecideArgs<T> d = da ? *da : JumpDecideArgs<T>{};
  hipLaunchKernelGGL((mjhmc_step_kernel<En, T, E>), dim3((unsigned)(n_traj + n_decide)), dim3(256), 0, st, t, d, en, n_traj,
                     n_decide);
}

template <class En, typename T, int E>
inline void launch_eval_t(const EvalArgs<T>& a, const En& en, hipStream_t st) {
  const int64_t threads = a.N << a.logG;
  const unsigned grid = (unsigned)((threads + 255) / 256);
  hipLaunchKernelGGL((mjhmc_eval_kernel<En, T, E>), dim3(grid), dim3(256), 0, st, a, en);
}

template <class En, typename T, int E>
inline void launch_leap_t(const LeapArgs<T>& a, const En& en, hipStream_t st) {
  const int64_t threads = a.N << a.logG;
  hipLaunchKernelGGL((mjhmc_leap_kernel<En, T, E>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, a, en);
}

// The run-time elements per lane as the kernels' compile-time E: launch(en, integral constant).
// E choices: f64 {2, 8, 16}, f32 {4, 16, 32}  (1, 4, 8 chunks per lane)
template <typename T, class En, class F>
inline void with_elements(int E, const En& en, F&& launch) {
  constexpr int kChunk = 16 / (int)sizeof(T);
  if (E == kChunk) launch(en, std::integral_constant<int, kChunk>{});
  else if (E == 4 * kChunk) launch(en, std::integral_constant<int, 4 * kChunk>{});
  else launch(en, std::integral_constant<int, 8 * kChunk>{});
}
// LAUNCH<const functor type, T, E>(args..., en, st) with the functor MAKE(ep)
#define MJHMC_FOR_E_(T, MAKE, LAUNCH, ...)                            \
  with_elements<T>(E, MAKE(ep), [&](const auto& en, auto e) {         \
    LAUNCH<std::remove_reference_t<decltype(en)>, T, decltype(e)::value>(__VA_ARGS__, en, st); \
  })

#define MJHMC_DEFINE_ENERGY_LAUNCHERS(NAME, MAKE64, MAKE32)                                               \
  void NAME##_jump(const JumpArgs<double>& a, const EnergyParams& ep, int E, hipStream_t st) { MJHMC_FOR_E_(double, MAKE64, launch_jump_t, a); } \
  void NAME##_jump(const JumpArgs<float>& a, const EnergyParams& ep, int E, hipStream_t st) { MJHMC_FOR_E_(float, MAKE32, launch_jump_t, a); }   \
  void NAME##_leap(const LeapArgs<double>& a, const EnergyParams& ep, int E, hipStream_t st) { MJHMC_FOR_E_(double, MAKE64, launch_leap_t, a); } \
  void NAME##_leap(const LeapArgs<float>& a, const EnergyParams& ep, int E, hipStream_t st) { MJHMC_FOR_E_(float, MAKE32, launch_leap_t, a); }   \
  void NAME##_step(const TrajArgs<double>* ta, const JumpDecideArgs<double>* da, const EnergyParams& ep, int E, hipStream_t st) { MJHMC_FOR_E_(double, MAKE64, launch_step_t, ta, da); } \
  void NAME##_step(const TrajArgs<float>* ta, const JumpDecideArgs<float>* da, const EnergyParams& ep, int E, hipStream_t st) { MJHMC_FOR_E_(float, MAKE32, launch_step_t, ta, da); }    \
  void NAME##_eval(const EvalArgs<double>& a, const EnergyParams& ep, int E, hipStream_t st) { MJHMC_FOR_E_(double, MAKE64, launch_eval_t, a); } \
  void NAME##_eval(const EvalArgs<float>& a, const EnergyParams& ep, int E, hipStream_t st) { MJHMC_FOR_E_(float, MAKE32, launch_eval_t, a); }

}  // namespace mjhmc

#endif  // !__HIPCC_RTC__
