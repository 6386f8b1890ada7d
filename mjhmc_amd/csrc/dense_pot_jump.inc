// Body of a float32-state tile kernel, included INSIDE the kernel definition (dense_pot.hip; linear_energy.hip for the
// kernels of a linear-model energy): the jump kernel, one sampling_iteration attempt for a tile of 32 particles.
// MODE = kModeMJHMC (markov_jump_hmc.py:355-415), kModeCT (ContinuousTimeHMC, :251-290) or kModeControl (HMCBase /
// HMC / ControlHMC, :116-148 -- the comparison arm of the reference's ProductOfT experiments,
// search/control_poe_36/mjhmc_objective.py:14).
// In scope: template parameters NB (and REPLAY, MODE), the arguments `a` and `mdl`, the experts `xp`.
  __shared__ Shared<NB> sh;
  if (a.ctl->failed) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 31, h = lane >> 5;
  // MJHMC: the inverse-L tiles of this iteration's list are the first items of the launch
  const int ncold = MODE == kModeMJHMC ? *a.cold_count : 0;
  const int64_t nft = (ncold + kP - 1) / kP;
  if ((int64_t)blockIdx.x >= nft + a.ntiles) return;
  if (MODE == kModeMJHMC && blockIdx.x == 0 && threadIdx.x == 0) {
    *a.zero_count = 0;   // the list two iterations back is consumed: its counter is free for the next iteration's appends
    if (ncold) atomicAdd(&a.stats[3], (unsigned long long)ncold << 32);   // integrated here: the high half of the cold tally
  }
  unsigned n0 = 0, n1 = 0, n2 = 0, n3 = 0;  // tallies (meaning per mode: fill_iter_stats in iterate.hip)
  bool any_bad = false;
  AReg<NB> ar;
  areg_load<NB>(mdl, w, c, h, ar);
  stage_bias<NB>(mdl, sh);
  for (int64_t item = blockIdx.x; item < nft + a.ntiles; item += gridDim.x) {
    const bool inverse = item < nft;   // (uniform over the workgroup)
    int64_t p;
    if (inverse) {
      const int64_t slot = item * kP + c;
      p = a.cold_list[slot < ncold ? slot : ncold - 1];  // pad the last tile with a repeat
    } else {
      p = (item - nft) * kP + c;
    }
    const bool alive = p < a.N;
    Tile<NB> x, v, g;
    tile_load<NB>(a.X_in, p, w, h, x);
    tile_load<NB>(a.V_in, p, w, h, v);
    tile_load<NB>(a.G_in, p, w, h, g);
    if (inverse) {
#pragma unroll
      for (int r = 0; r < NB; ++r) v.b[r] = -v.b[r];
    }
    float EXL = 0.f;
    pot_trajectory<NB>(mdl, xp, ar, sh, w, c, h, lane, x, v, g, a.L, a.eps, a.chalf, &EXL);
    const float EVL = pot_kinetic<NB>(sh, w, c, h, v);
    const float HL = EXL + EVL;
    if (inverse) {
      if (w == 0 && h == 0) a.Hwork[p] = HL;
      __syncthreads();
      continue;
    }

    // rates / acceptance, waiting times, first minimum: lanes 0..31 of wave 0, one particle each
    if (w == 0 && h == 0) {
      const uint32_t pid = (uint32_t)(a.first_pid + (alive ? p : 0));
      const float EX0 = a.EX_in[p], EV0 = a.EV_in[p];
      const float H0 = EX0 + EV0;
      // H of the inverse-L proposal: cached; or the L proposal of the iteration in which the particle flipped; or being
      // integrated by an inverse-L item of this very launch -- then the particle is left pending for pot_fix_kernel
      float Hflf = MODE == kModeMJHMC ? a.Hflf_in[p] : 0.f;
      const bool cold = !(Hflf == Hflf);
      bool pending = false;
      if (cold) {
        Hflf = a.Hspec_in[p];
        pending = !(Hflf == Hflf);
      }
      double best = 0.0;
      bool bad = false, gate = false;
      int k = 0;
      if (!pending) {
        if constexpr (MODE == kModeMJHMC)
          k = dense_decide<REPLAY>(H0, HL, Hflf, a.p_r, pid, alive ? p : 0, a.N, a.rexp, a.key, best, bad);
        else if constexpr (MODE == kModeCT)
          k = dense_decide_ct<REPLAY>(H0, HL, a.p_r, pid, alive ? p : 0, a.N, a.rexp, a.key, best, bad);
        else
          k = dense_control<REPLAY>(H0, HL, a.p_r, a.p_flip, pid, alive ? p : 0, a.N, a.runif, a.key, gate);
        any_bad |= (bad && alive);
        // every move but L clears the cache; of those only the R-movers need their inverse-L proposal integrated
        if constexpr (MODE == kModeMJHMC) append_cold(a.next_list, a.next_count, alive && k == 2, p);
        a.dwell[p] = best;
        a.dwell_ring[p] = best;
        a.trans[p] = (uint8_t)k;
      }
      sh.move[c] = k | (gate ? 4 : 0);
      if (alive) {
        if constexpr (MODE == kModeControl) {  // l_count, f_count, R applied, fl_count (markov_jump_hmc.py:143-148)
          n0 += (k == 3);
          n1 += (k == 2);
          n2 += gate ? 1u : 0u;
          n3 += (k == 1);
        } else if (!pending) {
          n0 += (k == 0);
          n1 += (k == 1);
          n2 += (k == 2);
        }
        if constexpr (MODE == kModeMJHMC) n3 += cold;   // the reference integrates F L F for every one of these
      }
      // scalars of the successors that keep or take whole states; a refreshed kinetic energy is filled in below
      const bool took_L = MODE == kModeControl ? (k & 1) : (k == 0);
      a.EX_out[p] = took_L ? EXL : EX0;
      a.EV_out[p] = took_L ? EVL : EV0;
      if (!pending) {
        a.Hflf_out[p] = (MODE == kModeMJHMC && k == 0) ? H0 : __builtin_nanf("");
        if constexpr (MODE == kModeMJHMC) a.Hspec_out[p] = (k == 1) ? HL : __builtin_nanf("");
      }
    }
    __syncthreads();
    pot_finish<NB, REPLAY, MODE, false>(a, sh, p, alive, w, c, h, x, v, g);
    __syncthreads();
  }
  if (any_bad) {
    a.ctl->failed = 1;
    a.ctl->failed_iter = a.iter;
  }
  __shared__ unsigned tally[4];
  if (threadIdx.x < 4) tally[threadIdx.x] = 0;
  __syncthreads();
  if (n0) atomicAdd(&tally[0], n0);
  if (n1) atomicAdd(&tally[1], n1);
  if (n2) atomicAdd(&tally[2], n2);
  if (n3) atomicAdd(&tally[3], n3);
  __syncthreads();
  if (threadIdx.x < 4 && tally[threadIdx.x]) atomicAdd(&a.stats[threadIdx.x], (unsigned long long)tally[threadIdx.x]);
