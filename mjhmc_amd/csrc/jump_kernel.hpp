// Fused Markov-jump kernel for energies whose gradient is elementwise (optionally coupled through
// a few per-particle scalars).  One launch = one MarkovJumpHMC.sampling_iteration attempt
// (mjhmc/samplers/markov_jump_hmc.py:355-415) for every particle:
//
//   load (X, V) once -> inverse-L proposal (only if the FLF cache is cold; only its H is kept,
//   because the reference reads the FLF state only through H(), :367) -> forward L proposal
//   (mjhmc/samplers/hmc_state.py:86-100) -> transition rates (:341-347) -> waiting-time draws
//   (mjhmc/misc/utils.py:31-49) -> first-minimum (utils.py:15-28) -> write the chosen
//   successor state once.
//
// With it the two stand-alone kernels of the group form: mjhmc_leap_kernel and mjhmc_eval_kernel.  This header is all
// that hipRTC compiles around a user expression (user_expr.hip).
#pragma once
#include "group_form.hpp"
#include "jump_process.hpp"
#include "sampler_args.hpp"

namespace mjhmc {

// REPLAY = true: random numbers come from host-supplied arrays (parity tests against recorded
// reference runs).  It is a compile-time switch because any global load consumed inside the slot
// body forces an in-order vmcnt wait that would also drain the prefetch of the next slot.
// FULLROW = true: every lane's chunks are inside the row (pitch == G * E), no per-chunk predicates.
// MODE: which sampler family's iteration this is (kModeMJHMC / kModeControl / kModeCT).
// WPP = 1: G == 64 (a whole wavefront per particle) is a compile-time fact: the reduction ladder, the group
// exchanges (v_readlane) and the Philox calls (scalar unit) specialise on it.
// WPP = 3: G == 4 (a quad per particle, e.g. ndims 17..32 in float64): two-level DPP reductions without the run-time
// ladder, group exchanges as quad_perm broadcasts instead of ds_bpermute (C4 -3 %, isotropic 32 x 10^6 fused -8 %).
// WPP = 5 (FUSED MJHMC launches, G == 64): as WPP = 1, with the unit exponentials of all the launch's waiting-time
// draws made UP FRONT.  They depend on (particle id, tick) only, and the Philox + log chain behind them is ~130 of
// decide()'s ~190 vector instructions, which a wave-per-particle kernel otherwise spends on three useful lanes.  At the
// top of a slot the wave fills its own stripe of an LDS table [iteration][clock], every quad of lanes working on a
// different iteration -- 16 draws per vector pass instead of one -- and the iterations then run decide() from the
// table (same functions on the same inputs: identical bits); no barrier is involved.
// WPP = 6: the same with half a wavefront per particle (G == 32, two particles per slot).
// FUSED = true: the launch runs a.n_fuse (<= kMaxFuse) consecutive sampling iterations per particle.  The
// chains are independent, so between iterations nothing has to leave the wave: X, V, EX, EV, H_flf stay in
// registers / the LDS stash, HBM sees one read and one write of the state per LAUNCH instead of per
// iteration (plus the ring snapshots when samples are recorded).  Iteration `it` uses RNG tick key.tick + it
// and tallies into stats[4 * it ..]; the first iteration that meets a non-finite rate is reported through
// Control::inv_iter and the host re-runs the launch up to that iteration (the input buffers are untouched).
// waves per SIMD the register allocator is asked to make room for.  Vector-pipe-bound energies whose 8-element
// float64 instance sits a register or two above an occupancy step ask for that step (funnel: 169 -> 168 VGPRs = three
// waves per SIMD instead of two, C4 -3 %); everything else takes the build-wide value.
template <class En, typename T, int E, typename = void>
struct JumpWaves {
  static constexpr int value = MJHMC_JUMP_WAVES;
};
template <class En, typename T, int E>
struct JumpWaves<En, T, E, decltype((void)En::kWavesRow64)> {
  static constexpr int value = (sizeof(T) * E == 64 && sizeof(T) == 8) ? En::kWavesRow64 : MJHMC_JUMP_WAVES;
};
template <class En, typename T, int E, int MODE, bool REPLAY, bool FULLROW, int WPP = 0, bool FUSED = false>
__global__ __launch_bounds__(256, (JumpWaves<En, T, E>::value)) void mjhmc_jump_kernel(const JumpArgs<T> a, const En en) {
  static_assert(!(FUSED && REPLAY), "recorded random numbers are replayed one iteration per launch");
  if (a.ctl->failed) {  // an earlier attempt of this batch was rolled back: do nothing
    // ... unless the failure belongs to THIS fused launch (another workgroup met it first): this workgroup must still run,
    // report an earlier first failure of its own particles if it has one, and flush its tallies of the good iterations
    // (single-iteration launches too: a workgroup that starts after another one of ITS launch has raised the flag -- two
    // processes sharing the GPU delay each other's workgroups by more than a short kernel runs -- must still tally its cold
    // caches: the failed attempt's evaluations count, Distribution.E_count)
    if (!FUSED) {
      if (__hip_atomic_load(&a.ctl->failed_iter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < a.iter) return;
    } else {
      const int first = 0x7fffffff - __hip_atomic_load(&a.ctl->inv_iter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (first < a.iter) return;
    }
  }
  // Persistent waves: wave w handles slots w, w + W, w + 2W, ... (a slot = the 64/G particles one
  // wavefront works on).  The NEXT slot's X, V and scalars are loaded into a second register set
  // before the current slot's trajectories start, so HBM latency hides behind the fp64 work.
  constexpr bool BD = (WPP == 5 || WPP == 6);  // the waiting-time draws of a slot's iterations are made up front (clock table in LDS)
  constexpr int kBdPpw = WPP == 6 ? 2 : 1;     // particles per wave of the block-decide forms
  static_assert(!BD || (FUSED && MODE == kModeMJHMC), "block-level decide exists for fused MJHMC launches");
  const int logG = WPP == 6 ? 5 : ((WPP == 1 || BD) ? 6 : (WPP == 3 ? 2 : a.logG));
  const int G = 1 << logG;
  const int lane = threadIdx.x & 63;
  const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave in block, scalar
  const int ppw = 64 >> logG;
  const int64_t nslots = a.Npad >> (6 - logG);  // rows are padded to a multiple of 64 particles
  const int64_t W = (int64_t)gridDim.x * 4;
  const int64_t wave = (int64_t)blockIdx.x * 4 + wib;
  const int gi = lane >> logG;
  const LaneMap m = LaneMap::group(lane, G, a.D, a.CH, lane, WPP == 6 ? 6 : (BD ? 1 : WPP));
  constexpr int VEC = VecOf<T>::n;
  const uint32_t lane_off = ((uint32_t)gi * a.pitch + m.j * VEC) * (uint32_t)sizeof(T);
  const uint32_t chunk_stride = (uint32_t)(G * VEC * sizeof(T));
  const size_t slot_bytes = (size_t)ppw * a.pitch * sizeof(T);
  const auto lc = en.template local<E>(m);
  unsigned nL = 0, nF = 0, nR = 0, nCold = 0;  // per-lane tallies (group leaders only)
  bool any_bad = false;
  const int n_it = FUSED ? a.n_fuse : 1;
  int first_bad = 0x7fffffff;  // FUSED: first iteration of this lane's particles that met a non-finite rate
  __shared__ unsigned fused_tally[FUSED ? kMaxFuse : 1][4];
  if constexpr (FUSED) {
    fused_tally[threadIdx.x >> 2][threadIdx.x & 3] = 0;  // 256 threads == kMaxFuse * 4
    __syncthreads();
  }
  using Vec = typename VecOf<T>::type;
  constexpr int C = E / VEC;
  __shared__ Vec stash[4][2][C][64];
  Vec(*stash_x)[64] = stash[wib][0];
  Vec(*stash_v)[64] = stash[wib][1];
  __shared__ double bd_e[BD ? kMaxFuse : 1][4 * kBdPpw][3];  // unit exponentials [iteration][particle of the block][L, R, F clock]

  T nx[E], nv[E];
  SlotScalars<T> ns;
  auto fetch = [&](int64_t slot) {
    const int64_t p = slot * ppw + gi;
    ns.EX = a.EX_in[p];  // scalars first: they are the oldest loads, so waiting for them later
    ns.EV = a.EV_in[p];  // never waits for the rows behind them
    ns.Hflf = a.Hflf_in[p];
    slot_load<T, E, FULLROW>((const char*)a.X_in + slot * slot_bytes, lane_off, chunk_stride, m, nx);
    slot_load<T, E, FULLROW>((const char*)a.V_in + slot * slot_bytes, lane_off, chunk_stride, m, nv);
  };
  // FUSED launches spend tens of microseconds per slot: its loads are issued at the top of the slot instead of
  // one slot ahead, which frees the second register set (one more wave per SIMD)
  if (!FUSED && wave < nslots) fetch(wave);

  // (BD: every wave fills the clock table of its OWN slot -- a slot has n_it pairs, enough to keep all sixteen quads of
  // the wave busy -- so the waves of a workgroup need no barrier and walk their slots independently like everyone else)
  const int64_t slot_first = wave;
#pragma unroll 1
  for (int64_t slot0 = slot_first; slot0 < nslots; slot0 += W) {
    const int64_t slot = slot0;
    const int64_t p = slot * ppw + gi;
    const bool alive = p < a.N;
    if constexpr (FUSED) fetch(slot);
    // The slot's pre-move state (x0, v0) is parked in this wave's private LDS stripe (lane-linear
    // 16-byte chunks: conflict-free ds_write_b128 / ds_read_b128, no barrier -- every lane reads
    // back only what it wrote).  Registers then hold just the working trajectory and the
    // prefetched next slot.
    T x[E], v[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      x[e] = nx[e];
      v[e] = nv[e];
    }
    if constexpr (!FUSED) {
      stash_put<T, E>(stash_x, lane, x);
      stash_put<T, E>(stash_v, lane, v);
    }
    T EX0 = ns.EX, EV0 = ns.EV, Hcached = ns.Hflf;
    use_here(EX0);
    use_here(EV0);
    use_here(Hcached);
    if constexpr (!FUSED)
      fetch(slot0 + W < nslots ? slot0 + W : slot0);  // prefetch (unconditional, so waits stay countable): in flight during everything below
    const uint32_t pid = (uint32_t)(a.first_pid + p);
    RngKey key = a.key;
    int k;
    double dwell = 0.0;
    T EXn, EVn, Hc;
    bool tally_cold = false, r_applied = false;
    if constexpr (BD) {
      // this wave's stripe of the table: [iteration][wave * kBdPpw + particle of the slot][clock]; written and read by this
      // wave only (LDS operations of a wave execute in order)
      LaneMap mq = m;   // a quad of lanes per (particle, iteration) pair: lane 0 L clock, 1 R clock, 2 F clock
      mq.j = lane & 3;
      mq.G = 4;
      mq.lane0 = lane & ~3;
      mq.wpp = 3;
      for (int r = lane >> 2; r - (lane >> 2) < kBdPpw * n_it; r += 16) {  // r = kBdPpw * iteration + particle of the slot
        const int it = r / kBdPpw, q = r % kBdPpw;
        RngKey kt = a.key;
        const uint32_t lo = kt.tick_lo + (uint32_t)it;
        kt.tick_hi += lo < kt.tick_lo ? 1u : 0u;
        kt.tick_lo = lo;
        const double e = decide_draw(kt, mq, (uint32_t)(a.first_pid + slot * kBdPpw + q));
        if (it < n_it && (lane & 3) < 3) bd_e[it][kBdPpw * wib + q][lane & 3] = e;
      }
    }
#pragma unroll 1
    for (int it = 0; it < n_it; ++it) {
    if constexpr (FUSED) {
      stash_put<T, E>(stash_x, lane, x);
      stash_put<T, E>(stash_v, lane, v);
    }
    const bool warm = Hcached == Hcached;  // cache_active (hmc_state.py:43-44) is carried as "H_flf is not NaN"
    const T H0 = EX0 + EV0;  // HMCState.H (hmc_state.py:80-84)

    // inverse-L proposal F L F; only H() of it is ever read (markov_jump_hmc.py:360,367)
    T Hflf = Hcached;
    if (MODE == kModeMJHMC && !warm) {
#pragma unroll
      for (int e = 0; e < E; ++e) v[e] = -v[e];
      trajectory<En, T, E, REPLAY>(en, lc, m, x, v, a.L, a.eps, a.chalf);
      T ex, ev;
      state_energies<En, T, E>(en, lc, m, x, v, ex, ev);
      Hflf = ex + ev;
      stash_get<T, E>(stash_x, lane, x);
      stash_get<T, E>(stash_v, lane, v);
    }

    // forward proposal L
    trajectory<En, T, E, REPLAY>(en, lc, m, x, v, a.L, a.eps, a.chalf);
    T EXL, EVL;
    state_energies<En, T, E>(en, lc, m, x, v, EXL, EVL);
    const T HL = EXL + EVL;

    bool bad = false;
    Hc = (T)__builtin_nan("");
    tally_cold = false;
    r_applied = false;
    if constexpr (MODE == kModeMJHMC) {
      if constexpr (BD) {
        // lane 0 of the particle's group: L clock, lane 1: R clock, others: F clock
        const double e_pre = bd_e[it][kBdPpw * wib + (kBdPpw == 2 ? (lane >> 5) : 0)][m.j < 2 ? m.j : 2];
        decide<T, false, true>(a, key, m, H0, HL, Hflf, alive ? p : 0, pid, k, dwell, bad, e_pre);
      } else {
        decide<T, REPLAY>(a, key, m, H0, HL, Hflf, alive ? p : 0, pid, k, dwell, bad);
      }
      tally_cold = !warm;
      // successor state (markov_jump_hmc.py:399-410)
      if (k == 0) {  // L: proposal accepted; the pre-move state becomes the cached inverse-L state
        EXn = EXL;
        EVn = EVL;
        Hc = H0;
      } else if (k == 1) {  // F: flip the momentum; clear_flf_cache (:409-410)
        stash_get<T, E>(stash_x, lane, x);
        stash_get<T, E>(stash_v, lane, v);
#pragma unroll
        for (int e = 0; e < E; ++e) v[e] = -v[e];
        EXn = EX0;
        EVn = EV0;
      } else {  // R: refresh the momentum (hmc_state.py:121-129)
        stash_get<T, E>(stash_x, lane, x);
        if (!REPLAY && a.defer_r) {  // (no caller sets it any more: rounds 1-4 left the refresh to a compacted pass)
          stash_get<T, E>(stash_v, lane, v);
          EVn = EV0;
        } else {
          refresh_stash<T, E, REPLAY>(stash_v, lane, a.noise + (size_t)(alive ? p : 0) * a.pitch, key, pid, m,
                                      a.r_keep, a.r_mix);
          stash_get<T, E>(stash_v, lane, v);
          EVn = kinetic<T, E>(v, m);
        }
        EXn = EX0;
      }
    } else if constexpr (MODE == kModeCT) {
      decide_ct<T, REPLAY>(a, key, m, H0, HL, alive ? p : 0, pid, k, dwell, bad);
      if (k == 0) {  // FL: leap, then flip (markov_jump_hmc.py:258,278)
#pragma unroll
        for (int e = 0; e < E; ++e) v[e] = -v[e];
        EXn = EXL;
        EVn = EVL;
      } else if (k == 1) {  // F
        stash_get<T, E>(stash_x, lane, x);
        stash_get<T, E>(stash_v, lane, v);
#pragma unroll
        for (int e = 0; e < E; ++e) v[e] = -v[e];
        EXn = EX0;
        EVn = EV0;
      } else {  // R (:285-286)
        stash_get<T, E>(stash_x, lane, x);
        refresh_stash<T, E, REPLAY>(stash_v, lane, a.noise + (size_t)(alive ? p : 0) * a.pitch, key, pid, m,
                                    a.r_keep, a.r_mix);
        stash_get<T, E>(stash_v, lane, v);
        EXn = EX0;
        EVn = kinetic<T, E>(v, m);
      }
    } else {
      // Discrete-time control samplers (markov_jump_hmc.py:116-148): propose L then F, accept with
      // min(1, exp(H0 - H1)) (a NaN difference accepts, as `Ediff < 0` is False, :112-113), flip with
      // probability p_flip, then refresh EVERY particle's momentum when the batch-wide gate fires.
      double uacc, uflip, ugate;
      if constexpr (REPLAY) {
        const int64_t pp = alive ? p : 0;
        uacc = a.runif[pp];
        uflip = a.runif[a.N + pp];
        ugate = a.runif[2 * a.N];
      } else {
        const u32x4 q = philox4x32_10(pid, key.tick_lo, key.tick_hi, kSlotExpR, key.k0, key.k1);
        const u32x4 f = philox4x32_10(pid, key.tick_lo, key.tick_hi, kSlotFlip, key.k0, key.k1);
        const u32x4 g = philox4x32_10(0xFFFFFFFFu, key.tick_lo, key.tick_hi, kSlotFlip, key.k0, key.k1);
        uacc = u53(q.w2, q.w3);
        uflip = u53(f.w0, f.w1);
        ugate = u53(g.w2, g.w3);
      }
      const double dH = (double)(H0 - HL);
      const bool accept = !(dH < 0.0) || (uacc < exp(dH));
      const bool flip = uflip < a.p_flip;
      const bool gate = ugate < a.p_r;
      if (accept) {
#pragma unroll
        for (int e = 0; e < E; ++e) v[e] = -v[e];
        EXn = EXL;
        EVn = EVL;
      } else {
        stash_get<T, E>(stash_x, lane, x);
        stash_get<T, E>(stash_v, lane, v);
        EXn = EX0;
        EVn = EV0;
      }
      if (flip) {
#pragma unroll
        for (int e = 0; e < E; ++e) v[e] = -v[e];
      }
      r_applied = gate;
      if (gate) {  // state.R() on the whole batch (:138-141)
        stash_put<T, E>(stash_v, lane, v);
        refresh_stash<T, E, REPLAY>(stash_v, lane, a.noise + (size_t)(alive ? p : 0) * a.pitch, key, pid, m,
                                    a.r_keep, a.r_mix);
        stash_get<T, E>(stash_v, lane, v);
        EVn = kinetic<T, E>(v, m);
      }
      k = (accept ? 1 : 0) | (flip ? 2 : 0);
      // tallies: slot 0 = accepted & flipped (l_count), 1 = flipped only (f_count), 2 = R applied,
      // 3 = accepted only (fl_count)   (markov_jump_hmc.py:143-148)
      tally_cold = (accept && !flip);
    }
    any_bad |= (bad && alive);
    if constexpr (FUSED) {
      // bookkeeping of iteration `it`; the successor state becomes the next iteration's pre-move state
      if (bad && alive) first_bad = min(first_bad, it);
      const bool lead = alive && m.j == 0;
      if constexpr (BD && kBdPpw == 1) {
        // a wavefront per particle: the move is wave-uniform, the tallies are two LDS atomics of lane 0 (the ballots of the
        // general form below cost ~25 vector instructions per iteration to say "one" -- 6 % of C2's iteration)
        if (lead) {
          atomicAdd(&fused_tally[it][k], 1u);
          if (tally_cold) atomicAdd(&fused_tally[it][3], 1u);
        }
      } else {
      unsigned long long b0, b1, b2;
      if constexpr (MODE == kModeControl) {
        b0 = __ballot(lead && k == 3);
        b1 = __ballot(lead && k == 2);
        b2 = __ballot(lead && r_applied);
      } else {
        b0 = __ballot(lead && k == 0);
        b1 = __ballot(lead && k == 1);
        b2 = __ballot(lead && k == 2);
      }
      const unsigned long long b3 = __ballot(lead && tally_cold);
      if (lane == 0) {
        if (b0) atomicAdd(&fused_tally[it][0], (unsigned)__popcll(b0));
        if (b1) atomicAdd(&fused_tally[it][1], (unsigned)__popcll(b1));
        if (b2) atomicAdd(&fused_tally[it][2], (unsigned)__popcll(b2));
        if (b3) atomicAdd(&fused_tally[it][3], (unsigned)__popcll(b3));
      }
      }
      if (a.xiter) {  // sample ring: X and the dwelling times after every iteration
        slot_store<T, E, FULLROW>((char*)(a.xiter + (size_t)it * a.xiter_stride) + slot * slot_bytes, lane_off,
                                  chunk_stride, m, x);
        a.dwell_ring[(size_t)it * a.Npad + p] = dwell;
      }
      EX0 = EXn;
      EV0 = EVn;
      Hcached = Hc;
      key.tick_hi += (key.tick_lo == 0xFFFFFFFFu) ? 1u : 0u;
      key.tick_lo += 1u;
    }
    }  // fused iterations

    // Stores are unconditional on purpose: rows beyond N are padding (allocated, never read back),
    // and every lane of a group writes the same scalar to the same address.  With no store behind
    // a branch the compiler can COUNT them, so the wait for the prefetched loads at the loop end is
    // vmcnt(#stores) instead of vmcnt(0) -- the wave never sits waiting for HBM write acks.
    if (!FUSED || !a.xiter)
      slot_store<T, E, FULLROW>((char*)a.X_out + slot * slot_bytes, lane_off, chunk_stride, m, x);
    slot_store<T, E, FULLROW>((char*)a.V_out + slot * slot_bytes, lane_off, chunk_stride, m, v);
    a.EX_out[p] = EXn;
    a.EV_out[p] = EVn;
    a.Hflf_out[p] = Hc;
    a.dwell[p] = dwell;
    if constexpr (!FUSED) a.dwell_ring[p] = dwell;
    a.trans[p] = (uint8_t)k;
    if (!FUSED && alive && m.j == 0) {
      if constexpr (MODE == kModeControl) {
        nL += (k == 3);
        nF += (k == 2);
        nR += r_applied ? 1u : 0u;
      } else {
        nL += (k == 0);
        nF += (k == 1);
        nR += (k == 2);
      }
      nCold += tally_cold ? 1u : 0u;
    }
  }
  if constexpr (FUSED) {
    for (int o = 32; o > 0; o >>= 1) first_bad = min(first_bad, __shfl_xor(first_bad, o));
    if (first_bad != 0x7fffffff && lane == 0) {
      a.ctl->failed = 1;
      atomicMax(&a.ctl->inv_iter, 0x7fffffff - (a.iter + first_bad));
    }
    __syncthreads();
    const int it = threadIdx.x >> 2, c = threadIdx.x & 3;
    if (it < n_it) {
      const unsigned t = fused_tally[it][c];
      if (t) atomicAdd(&a.stats[4 * it + c], (unsigned long long)t);
    }
    return;
  }
  if (any_bad) {  // draw_from's ValueError (utils.py:43-48): the host rolls this attempt back
    a.ctl->failed_iter = a.iter;   // (first: whoever sees the flag sees which launch raised it)
    __threadfence();
    a.ctl->failed = 1;
  }

  // integer bookkeeping: l/f/r counts and the number of cold inverse-L caches of this attempt
  // (markov_jump_hmc.py:413-415; Distribution.E_count / dEdX_count, distributions.py:62-75)
  __shared__ unsigned tally[4][4];
  for (int o = 32; o > 0; o >>= 1) {
    nL += __shfl_xor(nL, o);
    nF += __shfl_xor(nF, o);
    nR += __shfl_xor(nR, o);
    nCold += __shfl_xor(nCold, o);
  }
  if (lane == 0) {
    tally[wib][0] = nL;
    tally[wib][1] = nF;
    tally[wib][2] = nR;
    tally[wib][3] = nCold;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const unsigned long long t =
        (unsigned long long)tally[0][threadIdx.x] + tally[1][threadIdx.x] + tally[2][threadIdx.x] + tally[3][threadIdx.x];
    if (t) atomicAdd(&a.stats[threadIdx.x], t);
  }
}

// ------------------------------------------------------------------------------------------
// HMCState.leapfrog / HMCState.L as an operator on caller-supplied states (hmc_state.py:86-100): the reference's
// literal operation order (the EXACT trajectory), then EV, EX and dE/dX of the end point.
// ------------------------------------------------------------------------------------------
template <class En, typename T, int E>
__global__ __launch_bounds__(256) void mjhmc_leap_kernel(const LeapArgs<T> a, const En en) {
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int G = 1 << a.logG;
  const int64_t p_raw = tid >> a.logG;
  const bool alive = p_raw < a.N;
  const int64_t p = alive ? p_raw : a.N - 1;
  const LaneMap m = LaneMap::group((int)tid, G, a.D, a.CH, (int)(threadIdx.x & 63));
  T x[E], v[E];
  load_row<T, E>(a.X + (size_t)p * a.pitch, m, x);
  load_row<T, E>(a.V + (size_t)p * a.pitch, m, v);
  const auto lc = en.template local<E>(m);
  trajectory<En, T, E, true>(en, lc, m, x, v, a.L, a.eps, a.chalf);
  if (alive) {
    store_row<T, E>(a.X_out + (size_t)p * a.pitch, m, x);
    store_row<T, E>(a.V_out + (size_t)p * a.pitch, m, v);
  }
  if (a.G) {
    T g[E];
    const auto ctx = en.prep(x, m);
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int d = dim_of<T, E>(m, e);
      g[e] = (d < a.D) ? en.template grad<E>(x[e], e, d, ctx, lc) : T(0);
    }
    if (alive) store_row<T, E>(a.G + (size_t)p * a.pitch, m, g);
  }
  if (a.EX) {
    const T ex = en.energy(x, m, lc);
    if (alive && m.j == 0) a.EX[p] = ex;
  }
  if (a.EV) {
    const T ev = kinetic<T, E>(v, m);
    if (alive && m.j == 0) a.EV[p] = ev;
  }
}

// ------------------------------------------------------------------------------------------
// evaluation kernel: E(X), dEdX(X), optionally kinetic energy / generated initial momentum
// (HMCState.__init__, hmc_state.py:24-39; Distribution.E/dEdX, distributions.py:62-81)
// ------------------------------------------------------------------------------------------

template <class En, typename T, int E>
__global__ __launch_bounds__(256) void mjhmc_eval_kernel(const EvalArgs<T> a, const En en) {
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int G = 1 << a.logG;
  const int64_t p_raw = tid >> a.logG;
  const bool alive = p_raw < a.N;
  const int64_t p = alive ? p_raw : a.N - 1;
  const LaneMap m = LaneMap::group((int)tid, G, a.D, a.CH, (int)(threadIdx.x & 63));
  T x[E];
  load_row<T, E>(a.X + (size_t)p * a.pitch, m, x);
  const auto lc = en.template local<E>(m);
  if (a.G) {
    T g[E];
    const auto ctx = en.prep(x, m);
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int d = dim_of<T, E>(m, e);
      g[e] = (d < a.D) ? en.template grad<E>(x[e], e, d, ctx, lc) : T(0);
    }
    if (alive) store_row<T, E>(a.G + (size_t)p * a.pitch, m, g);
  }
  if (a.E) {
    const T ex = en.energy(x, m, lc);
    if (alive && m.j == 0) a.E[p] = ex;
  }
  if (a.EV) {
    T v[E];
    if (a.V_out) {
      refresh_noise<T, E>(nullptr, a.key, (uint32_t)(a.first_pid + p), m, v);
      if (alive) store_row<T, E>(a.V_out + (size_t)p * a.pitch, m, v);
    } else {
      load_row<T, E>(a.V + (size_t)p * a.pitch, m, v);
    }
    const T ev = kinetic<T, E>(v, m);
    if (alive && m.j == 0) a.EV[p] = ev;
  }
}

}  // namespace mjhmc
