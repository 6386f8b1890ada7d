// The launchers of the built-in elementwise energies as the host side sees them: eight overloads per energy, defined by
// MJHMC_DEFINE_ENERGY_LAUNCHERS (launchers.hpp) in the energy's translation unit.
#pragma once
#ifndef __HIPCC_RTC__  // host side only
#include <hip/hip_runtime.h>

#include "sampler_args.hpp"

namespace mjhmc {

#define MJHMC_DECLARE_ENERGY_LAUNCHERS(NAME)                                                       \
  void NAME##_jump(const JumpArgs<double>&, const EnergyParams&, int, hipStream_t);           \
  void NAME##_jump(const JumpArgs<float>&, const EnergyParams&, int, hipStream_t);            \
  void NAME##_leap(const LeapArgs<double>&, const EnergyParams&, int, hipStream_t);           \
  void NAME##_leap(const LeapArgs<float>&, const EnergyParams&, int, hipStream_t);            \
  void NAME##_step(const TrajArgs<double>*, const JumpDecideArgs<double>*, const EnergyParams&, int, hipStream_t); \
  void NAME##_step(const TrajArgs<float>*, const JumpDecideArgs<float>*, const EnergyParams&, int, hipStream_t);  \
  void NAME##_eval(const EvalArgs<double>&, const EnergyParams&, int, hipStream_t);           \
  void NAME##_eval(const EvalArgs<float>&, const EnergyParams&, int, hipStream_t);

MJHMC_DECLARE_ENERGY_LAUNCHERS(iso)
MJHMC_DECLARE_ENERGY_LAUNCHERS(diag)
MJHMC_DECLARE_ENERGY_LAUNCHERS(rough)
MJHMC_DECLARE_ENERGY_LAUNCHERS(mm)
MJHMC_DECLARE_ENERGY_LAUNCHERS(funnel_neal)
MJHMC_DECLARE_ENERGY_LAUNCHERS(funnel_ref)

}  // namespace mjhmc

#endif  // !__HIPCC_RTC__
