// The jump process of one particle: rates, the draws of the three clocks, the first minimum.
#pragma once
#include "jump_math.hpp"
#include "lane_group.hpp"
#include "philox.hpp"
#include "sampler_args.hpp"

namespace mjhmc {

// Rates, waiting-time draws and the first-minimum of one particle (markov_jump_hmc.py:366-396,
// utils.py:15-49).  All lanes of the particle's group enter with the same H values and leave with
// the same (k, dwell, bad).  When the group has >= 4 lanes the independent fp64 transcendental
// chains are evaluated ONCE, lane-parallel -- lane 0 works on the L clock, lane 1 on the R clock /
// the FLF rate, lane 2 on the F clock -- instead of three times in sequence in every lane
// (2 exp + 2 sqrt + 3 log + 3 div + 2 Philox  ->  1 of each), then exchanged inside the group.
// the unit exponential this lane contributes to decide() when the group has >= 4 lanes and the counter RNG is used
// (lane 0: L clock, lane 1: R clock, lanes 2..: F clock).  It depends on (particle id, tick) only, so a caller may
// draw it long before the energies exist (block-level decide: off the critical path between the two barriers).
__device__ __forceinline__ double decide_draw(const RngKey& key, const LaneMap& m, uint32_t pid) {
  const int role = m.j;
  const u32x4 w = philox4x32_10(pid, key.tick_lo, key.tick_hi, role == 1 ? kSlotExpR : kSlotExpLF, key.k0, key.k1);
  const double uA = u53(w.w0, w.w1);
  const double uF = group_lane(u53(w.w2, w.w3), m, 0);
  return neg_log_unit(role >= 2 ? uF : uA);
}

// the unit exponentials of a particle's three clocks in ONE lane (groups of fewer than four lanes): e0 from words 01 and e1
// from words 23 of the L / F slot, e2 from words 01 of the R slot -- or rows 0, 1, 2 of the replayed draws.  The fences keep
// the independent expansions from being interleaved (interleaved they cost ~90 extra VGPRs).
template <typename T, bool REPLAY>
__device__ __forceinline__ void draw_three_clocks(const JumpArgs<T>& a, const RngKey& key, int64_t p, uint32_t pid, double& e0,
                                                  double& e1, double& e2) {
  if constexpr (REPLAY) {
    e0 = a.rexp[p];
    e1 = a.rexp[a.N + p];
    e2 = a.rexp[2 * a.N + p];
  } else {
    const u32x4 w = philox4x32_10(pid, key.tick_lo, key.tick_hi, kSlotExpLF, key.k0, key.k1);
    __builtin_amdgcn_sched_barrier(0);
    const u32x4 q = philox4x32_10(pid, key.tick_lo, key.tick_hi, kSlotExpR, key.k0, key.k1);
    __builtin_amdgcn_sched_barrier(0);
    e0 = neg_log_unit(u53(w.w0, w.w1));
    __builtin_amdgcn_sched_barrier(0);
    e1 = neg_log_unit(u53(w.w2, w.w3));
    __builtin_amdgcn_sched_barrier(0);
    e2 = neg_log_unit(u53(q.w0, q.w1));
    __builtin_amdgcn_sched_barrier(0);
  }
}

template <typename T, bool REPLAY, bool PREDRAWN = false>
__device__ __forceinline__ void decide(const JumpArgs<T>& a, const RngKey& key, const LaneMap& m, T H0, T HL, T Hflf,
                                       int64_t p, uint32_t pid, int& k, double& dwell, bool& bad, double e_pre = 0.0) {
  const double r_rate = a.p_r;
  double dL, dF, dR, l_rate, f_rate;
  if (m.G >= 4) {
    const int role = m.j;  // 0: L clock, 1: R clock (and the FLF rate), 2..: F clock
    const T dH = H0 - ((role == 1) ? Hflf : HL);
    // exp(H1 - H2) ** .5 (markov_jump_hmc.py:341-347)
    const double rate01 = (m.wpp == 1) ? jump_rate<true>((double)dH) : jump_rate<false>((double)dH);
    l_rate = group_lane(rate01, m, 0);
    const double flf_rate = group_lane(rate01, m, 1);
    const double mn = (flf_rate != flf_rate || l_rate != l_rate) ? __builtin_nan("") : fmin(flf_rate, l_rate);
    f_rate = flf_rate - mn;  // :368
    double e;
    if constexpr (PREDRAWN) {
      e = e_pre;
    } else if constexpr (REPLAY) {
      const int row = (role == 0) ? 0 : (role == 1 ? 2 : 1);
      e = a.rexp[(size_t)row * a.N + p];
    } else {
      if (m.wpp == 1) {
        // one particle per wave: the counter, key and slot are wave-uniform, so both Philox calls run
        // on the scalar unit (s_mul_i32 / s_mul_hi_u32) beside the vector work instead of in it
        const uint32_t spid = __builtin_amdgcn_readfirstlane(pid);
        const u32x4 w = philox4x32_10(spid, key.tick_lo, key.tick_hi, kSlotExpLF, key.k0, key.k1);
        const u32x4 q = philox4x32_10(spid, key.tick_lo, key.tick_hi, kSlotExpR, key.k0, key.k1);
        const double uL = u53(w.w0, w.w1), uF = u53(w.w2, w.w3), uR = u53(q.w0, q.w1);
        e = neg_log_unit(role == 0 ? uL : (role == 1 ? uR : uF));
      } else {
        e = decide_draw(key, m, pid);
      }
    }
    const double rate = (role == 0) ? l_rate : (role == 1 ? r_rate : f_rate);
    bool ignore = false;
    const double d = wait_time(rate, e, ignore);
    dL = group_lane(d, m, 0);
    dR = group_lane(d, m, 1);
    dF = group_lane(d, m, 2);
  } else {
    l_rate = jump_rate((double)(H0 - HL));
    __builtin_amdgcn_sched_barrier(0);  // keep the independent expansions from being interleaved:
    const double flf_rate = jump_rate((double)(H0 - Hflf));  // interleaved they cost ~90 extra VGPRs
    __builtin_amdgcn_sched_barrier(0);
    const double mn = (flf_rate != flf_rate || l_rate != l_rate) ? __builtin_nan("") : fmin(flf_rate, l_rate);
    f_rate = flf_rate - mn;
    double eL, eF, eR;
    draw_three_clocks<T, REPLAY>(a, key, p, pid, eL, eF, eR);
    bool ignore = false;
    dL = wait_time(l_rate, eL, ignore);
    __builtin_amdgcn_sched_barrier(0);
    dF = wait_time(f_rate, eF, ignore);
    __builtin_amdgcn_sched_barrier(0);
    dR = wait_time(r_rate, eR, ignore);
    __builtin_amdgcn_sched_barrier(0);
  }
  // draw_from raises on a non-finite rate (utils.py:43-48); rate == 0 is fine (infinite wait)
  bad = !(isfinite(l_rate) && isfinite(f_rate) && isfinite(r_rate));
  k = first_min3(dL, dF, dR);
  dwell = (k == 0) ? dL : (k == 1 ? dF : dR);
}

// ContinuousTimeHMC (markov_jump_hmc.py:251-290): clocks FL (rate sqrt(exp(H0 - H_fl))), F (rate 1),
// R (rate p_r); min_idx is called with [f, fl, r], so ties go F, FL, R.  Returns k: 0 = FL, 1 = F, 2 = R.
template <typename T, bool REPLAY>
__device__ __forceinline__ void decide_ct(const JumpArgs<T>& a, const RngKey& key, const LaneMap& m, T H0, T HL,
                                          int64_t p, uint32_t pid, int& k, double& dwell, bool& bad) {
  const double fl_rate = jump_rate((double)(H0 - HL));
  const double r_rate = a.p_r;
  double dFL, dF, dR;
  if (m.G >= 4) {
    const int role = m.j;  // 0: FL clock, 1: R clock, 2..: F clock
    double e;
    if constexpr (REPLAY) {
      const int row = (role == 0) ? 0 : (role == 1 ? 2 : 1);
      e = a.rexp[(size_t)row * a.N + p];
    } else {
      e = decide_draw(key, m, pid);
    }
    const double rate = (role == 0) ? fl_rate : (role == 1 ? r_rate : 1.0);
    bool ignore = false;
    const double d = wait_time(rate, e, ignore);
    dFL = group_lane(d, m, 0);
    dR = group_lane(d, m, 1);
    dF = group_lane(d, m, 2);
  } else {
    double eFL, eF, eR;
    draw_three_clocks<T, REPLAY>(a, key, p, pid, eFL, eF, eR);
    bool ignore = false;
    dFL = wait_time(fl_rate, eFL, ignore);
    __builtin_amdgcn_sched_barrier(0);
    dF = wait_time(1.0, eF, ignore);
    __builtin_amdgcn_sched_barrier(0);
    dR = wait_time(r_rate, eR, ignore);
    __builtin_amdgcn_sched_barrier(0);
  }
  bad = !(isfinite(fl_rate) && isfinite(r_rate));
  const int kk = first_min3(dF, dFL, dR);  // rows f, fl, r (markov_jump_hmc.py:271)
  k = (kk == 0) ? 1 : (kk == 1 ? 0 : 2);
  dwell = (kk == 0) ? dF : (kk == 1 ? dFL : dR);
}

}  // namespace mjhmc
