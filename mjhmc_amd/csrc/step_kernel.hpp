// The two-launch iteration of a big batch: mjhmc_step_kernel, trajectories beside the jump process.
#pragma once
#include "group_form.hpp"
#include "jump_process.hpp"
#include "sampler_args.hpp"

namespace mjhmc {

// ------------------------------------------------------------------------------------------
// Round 5.  A MarkovJumpHMC iteration of a big batch with several particles per wavefront (C4: 16 particles per wave)
// used to be three launches on one stream -- inverse-L pass over the compacted cold caches (a trajectory's latency on a
// few waves: 32 us of C4's 269), jump kernel, list scan -- with the jump process inside the jump kernel: its ~350
// instructions per wave run on the lanes of the particles' groups between the trajectory and the stores of every slot.
// Now two launches of two KINDS:
//
//   mjhmc_traj_kernel    integrates and nothing else: memory-bound (C4: 1.02 GB in 0.20 ms = 5.1 TB/s).  Leading
//                        workgroups walk the list (the inverse-L proposals, beside the forward slots instead of in front of
//                        them); every other workgroup is one forward slot: load, trajectory, energies, store the end point
//                        AS IF the move were taken.  No LDS, no decision code, no second register set.
//   mjhmc_decide_kernel  the jump process with ONE LANE PER PARTICLE (64 live lanes of a wave instead of 16 groups'
//                        worth): rates, clocks, first minimum, dwelling time, counters (markov_jump_hmc.py:366-415):
//                        vector-pipe-bound.  The workgroup's movers (7 % of C4) are compacted in LDS and finished by lane
//                        groups: pre-move position put back, momentum flipped or redrawn (HMCState.R, with its kinetic
//                        energy); and they ARE the next iteration's list: one atomic per workgroup, no list scan.
//
// The same device functions as the jump kernel (trajectory, state_energies, decide, refresh_stash, kinetic) on the same
// inputs: the same bits (tests/test_gpu_fused.py compares the paths).  C4: 0.269 -> 0.262 ms per iteration, 125 000
// particles 0.057 -> 0.051.  (mjhmc_step_kernel can carry the trajectories of one part of a batch beside the jump process
// of another; iterate.hip does not use that: measured, no gain -- the trajectories keep the vector pipe half busy themselves.)
// ------------------------------------------------------------------------------------------
template <class En, typename T, int E>
__device__ __forceinline__ void traj_block(const TrajArgs<T>& a, const En& en, int vblock) {
  const LaneMap m = LaneMap::group((int)threadIdx.x, 1 << a.logG, a.D, a.CH, (int)(threadIdx.x & 63));
  const auto lc = en.template local<E>(m);
  const int ppb = 256 >> a.logG;  // particles per workgroup
  if (vblock < a.inv_blocks) {
    // inverse-L proposal F L F of the listed particles; only H() of it is ever read (markov_jump_hmc.py:360,367)
    const int n_cold = a.count ? *a.count : a.n_listed;
    for (int64_t first = (int64_t)vblock * ppb; first < n_cold; first += (int64_t)a.inv_blocks * ppb) {
      const int64_t idx = first + (threadIdx.x >> a.logG);
      const bool live = idx < n_cold;
      const int64_t p = a.list[live ? idx : 0];
      T x[E], v[E];
      load_row<T, E>(a.X_in + (size_t)p * a.pitch, m, x);
      load_row<T, E>(a.V_in + (size_t)p * a.pitch, m, v);
#pragma unroll
      for (int e = 0; e < E; ++e) v[e] = -v[e];
      trajectory<En, T, E, false>(en, lc, m, x, v, a.L, a.eps, a.chalf);
      T ex, ev;
      state_energies<En, T, E>(en, lc, m, x, v, ex, ev);
      if (live && m.j == 0) a.Hwork[p] = ex + ev;
    }
    return;
  }
  const int64_t p_raw = (int64_t)(vblock - a.inv_blocks) * ppb + (threadIdx.x >> a.logG);
  const bool alive = p_raw < a.N;
  const int64_t p = alive ? p_raw : a.N - 1;
  T x[E], v[E];
  load_row<T, E>(a.X_in + (size_t)p * a.pitch, m, x);
  load_row<T, E>(a.V_in + (size_t)p * a.pitch, m, v);
  trajectory<En, T, E, false>(en, lc, m, x, v, a.L, a.eps, a.chalf);
  T EXL, EVL;
  state_energies<En, T, E>(en, lc, m, x, v, EXL, EVL);
  if (alive) {
    store_row<T, E>(a.X_out + (size_t)p * a.pitch, m, x);
    store_row<T, E>(a.V_out + (size_t)p * a.pitch, m, v);
    if (m.j == 0) {
      a.EX_out[p] = EXL;
      a.EV_out[p] = EVL;
    }
  }
}

// particles per workgroup of the jump-process launch = 256 x kDecideSub.  A workgroup ends with FOUR global atomics on
// addresses every workgroup of the launch uses -- its movers' place in the next iteration's list (returning), the l / f / r
// tallies -- and same-address atomics are served one after another, ~12 ns each (tools/microbench/atomic_one_address.hip:
// 3 906 workgroups, one counter + three tallies: 55 us per launch; 977 workgroups: 14 us): with 256 particles per
// workgroup they, not the jump process, were most of C4's 0.074 ms launch.  Measured for C4 (10^6 particles), 1 / 2 / 4 / 8
// sub-blocks per workgroup: 74 / 56 / 60 / 65 us (without R-movers 73 / 48 / 46 / 50: more particles per workgroup also
// means their sub-blocks one after the other, and more movers for its lane groups).
constexpr int kDecideSub = 2;

template <typename T, int E>
struct DecideShared {
  typename VecOf<T>::type stash[4][E / VecOf<T>::n][64];
  int movers[256 * kDecideSub];   // this workgroup's movers: particle of the workgroup << 2 | move
  int n_f, n_r, list_base;
  unsigned tally[3];
  int any_bad;
};
template <typename T, int E>
__device__ __forceinline__ void decide_block(const JumpDecideArgs<T>& a, DecideShared<T, E>& sh, int vblock) {
  auto& stash = sh.stash;
  auto& movers = sh.movers;
  int& n_f = sh.n_f;
  int& n_r = sh.n_r;
  int& list_base = sh.list_base;
  auto& tally = sh.tally;
  int& any_bad = sh.any_bad;
  const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
  if (threadIdx.x == 0) {
    n_f = 0;
    n_r = 0;
    any_bad = 0;
  }
  if (threadIdx.x < 3) tally[threadIdx.x] = 0;
  __syncthreads();
  // ---- the jump process, one lane per particle ------------------------------------------------------------------------
#pragma unroll 1
  for (int sb = 0; sb < kDecideSub; ++sb) {
    const int in_wg = sb * 256 + (int)threadIdx.x;
    const int64_t p_raw = (int64_t)vblock * (256 * kDecideSub) + in_wg;
    const bool alive = p_raw < a.N;
    const int64_t p = alive ? p_raw : a.N - 1;
    const T EX0 = a.EX_in[p], EV0 = a.EV_in[p];
    const T H0 = EX0 + EV0;                   // HMCState.H (hmc_state.py:80-84)
    const T HL = a.EX_out[p] + a.EV_out[p];
    T Hflf = a.Hflf_in[p];
    if (!(Hflf == Hflf)) Hflf = a.Hwork[p];   // cold cache: integrated by this iteration's mjhmc_traj_kernel
    JumpArgs<T> ja;
    ja.p_r = a.p_r;
    ja.rexp = nullptr;
    ja.runif = nullptr;
    ja.N = a.N;
    const LaneMap m1 = LaneMap::one_lane();
    int k = 0;
    double dwell = 0.0;
    bool bad = false;
    decide<T, false>(ja, a.key, m1, H0, HL, Hflf, p, (uint32_t)(a.first_pid + p), k, dwell, bad);
    if (alive) {
      a.Hflf_out[p] = (k == 0) ? H0 : (T)__builtin_nan("");   // L: the pre-move state becomes the cached inverse-L state
      a.dwell[p] = dwell;
      a.dwell_ring[p] = dwell;
      a.trans[p] = (uint8_t)k;
      if (k != 0) {                            // F / R keep the position; an R-mover's kinetic energy follows below
        a.EX_out[p] = EX0;
        a.EV_out[p] = EV0;
      }
      if (bad) any_bad = 1;
    }
    const unsigned long long b0 = __ballot(alive && k == 0), b1 = __ballot(alive && k == 1), b2 = __ballot(alive && k == 2);
    if (lane == 0) {
      if (b0) atomicAdd(&tally[0], (unsigned)__popcll(b0));
      if (b1) atomicAdd(&tally[1], (unsigned)__popcll(b1));
      if (b2) atomicAdd(&tally[2], (unsigned)__popcll(b2));
    }
    // the R-movers from the front of the array, the F-movers from its back: the lane groups that redraw a momentum
    // (Philox + Box-Muller: ~1000 instructions) sit together in as few waves as possible
    const unsigned long long below = (1ull << lane) - 1ull;
    if (b2) {
      int at = 0;
      if (lane == 0) at = atomicAdd(&n_r, (int)__popcll(b2));
      at = __shfl(at, 0);
      if (alive && k == 2) movers[at + (int)__popcll(b2 & below)] = (in_wg << 2) | 2;
    }
    if (b1) {
      int at = 0;
      if (lane == 0) at = atomicAdd(&n_f, (int)__popcll(b1));
      at = __shfl(at, 0);
      if (alive && k == 1) movers[256 * kDecideSub - 1 - (at + (int)__popcll(b1 & below))] = (in_wg << 2) | 1;
    }
  }
  __syncthreads();
  const int nr = n_r, nf = n_f, nm = nr + nf;
  if (threadIdx.x == 0) {
    if (any_bad) {  // draw_from's ValueError (utils.py:43-48): the host rolls this attempt back
      a.ctl->failed_iter = a.iter;
      __threadfence();
      a.ctl->failed = 1;
    }
    list_base = nm ? atomicAdd(a.next_count, nm) : 0;
  }
  if (threadIdx.x < 3 && tally[threadIdx.x]) atomicAdd(&a.stats[threadIdx.x], (unsigned long long)tally[threadIdx.x]);
  __syncthreads();
  auto mover = [&](int i) { return movers[i < nr ? i : 256 * kDecideSub - 1 - (i - nr)]; };
  // every move but L clears the cache (markov_jump_hmc.py:409-410): the movers are the next iteration's list
  for (int i = threadIdx.x; i < nm; i += 256) a.next_list[list_base + i] = (int)((int64_t)vblock * (256 * kDecideSub) + (mover(i) >> 2));
  // ---- the movers' successor states, a lane group per mover ------------------------------------------------------------
  const LaneMap m = LaneMap::group((int)threadIdx.x, 1 << a.logG, a.D, a.CH, (int)(threadIdx.x & 63));
  const int ppb = 256 >> a.logG;
  for (int first = 0; first < nm; first += ppb) {
    const int idx = first + (threadIdx.x >> a.logG);
    const bool live = idx < nm;
    const int code = mover(live ? idx : 0);
    const int64_t p = (int64_t)vblock * (256 * kDecideSub) + (code >> 2);
    const int k = code & 3;
    if (__ballot(live) == 0ull) continue;   // (a wave without a mover has nothing to do)
    T x[E], v[E];
    load_row<T, E>(a.X_in + (size_t)p * a.pitch, m, x);
    load_row<T, E>(a.V_in + (size_t)p * a.pitch, m, v);
    const bool r = live && k == 2;
    if (__ballot(r) != 0ull) {  // HMCState.R (hmc_state.py:121-129)
      stash_put<T, E>(stash[wib], lane, v);
      refresh_stash<T, E, false>(stash[wib], lane, nullptr, a.key, (uint32_t)(a.first_pid + p), m, a.r_keep, a.r_mix);
      T vr[E];
      stash_get<T, E>(stash[wib], lane, vr);
      const T evr = kinetic<T, E>(vr, m);
      if (r) {
#pragma unroll
        for (int e = 0; e < E; ++e) v[e] = vr[e];
        if (m.j == 0) a.EV_out[p] = evr;
      }
    }
    if (live && k == 1) {       // HMCState.F
#pragma unroll
      for (int e = 0; e < E; ++e) v[e] = -v[e];
    }
    if (live) {
      store_row<T, E>(a.X_out + (size_t)p * a.pitch, m, x);
      store_row<T, E>(a.V_out + (size_t)p * a.pitch, m, v);
    }
  }
}

// One launch = the trajectories of one half of the batch (TrajArgs) BESIDE the jump process of the other half
// (JumpDecideArgs), their workgroups interleaved four to one -- the ratio of their grids -- so that every CU holds both
// kinds at any time; either side may be absent (n_traj or n_decide zero: the first and the last launch of a call).
template <class En, typename T, int E>
__global__ __launch_bounds__(256) void mjhmc_step_kernel(const TrajArgs<T> ta, const JumpDecideArgs<T> da, const En en,
                                                         int n_traj, int n_decide) {
  __shared__ DecideShared<T, E> sh;
  if ((n_traj ? ta.ctl : da.ctl)->failed) return;
  const int b = blockIdx.x;
  const int groups = min(n_decide, n_traj / 4);      // [4 trajectory workgroups, 1 deciding workgroup] x groups, then the rest
  int role, vb;                                      // role 0: trajectories, 1: jump process
  if (b < 5 * groups) {
    const int g = b / 5, r = b % 5;
    role = r == 4;
    vb = role ? g : 4 * g + r;
  } else {
    const int rest = b - 5 * groups, left_t = n_traj - 4 * groups;
    role = rest >= left_t;
    vb = role ? groups + (rest - left_t) : 4 * groups + rest;
  }
  if (role == 0) traj_block<En, T, E>(ta, en, vb);
  else decide_block<T, E>(da, sh, vb);
}

}  // namespace mjhmc
