// Body of the float64-state jump kernel, included INSIDE the kernel definition (dense_pot64.hip; linear_energy.hip for the
// kernels of a linear-model energy): one sampling_iteration attempt for a tile of 32 particles (MODE as in
// dense_pot_jump.inc).  In scope: template parameters NB, REPLAY, MODE, the arguments `a` and `mdl`, the experts `xp`.
  __shared__ Shared64<NB> sh;
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
  // tallies (meaning per mode: fill_iter_stats in iterate.hip) and the failure flag live in LDS, not in registers that would be
  // live across every GEMM loop and streamed pass of the kernel: [0..3] counts, [4] some particle met a non-finite rate
  __shared__ unsigned tally[5];
  if (threadIdx.x < 5) tally[threadIdx.x] = 0;
  AReg64<NB> ar;
  areg_load<NB>(mdl, w, c, h, ar);
  stage_bias<NB>(mdl, sh.s);
  for (int64_t item = blockIdx.x; item < nft + a.ntiles; item += gridDim.x) {
    const bool inverse = item < nft;   // (uniform over the workgroup)
    [[maybe_unused]] const int istamp_item = (int)(item / gridDim.x) & 15;   // (the timing build's POT_ISTAMP)
    auto column_of = [&](int64_t it) -> int64_t {
      if (it < nft) {
        const int64_t slot = it * kP + c;
        return a.cold_list[slot < ncold ? slot : ncold - 1];  // pad the last tile with a repeat
      }
      return (it - nft) * kP + c;
    };
    // (everything that is not needed during the trajectory -- the scalars of the decision, the output rows' addresses --
    // is fetched / formed after it: the kernel sits at its 512-register budget, and what is live across the GEMM loops
    // and the per-step passes decides whether those spill; tools/check_isa.sh gates both.  That includes the column's own
    // index: it is looked up again behind the trajectory, through an item number the compiler cannot see through)
    Tile<NB> g;
    VTile<NB> v, x;
    float exl = 0.f;
    double EVL;
    {
      const int64_t p = column_of(item);
      POT_ISTAMP(0);
      staged_start<NB>(sh.s, a.X_in, a.V_in, a.G_in, p, w, c, h, g, v, x, inverse);
      POT_ISTAMP(1);
      EVL = pot64_trajectory<NB>(mdl, xp, ar, sh, w, c, h, lane, g, v, x, a.L, a.eps, a.chalf, &exl);
      POT_ISTAMP(2);
    }
    int64_t item_again = item;
    asm volatile("" : "+s"(item_again));
    const int64_t p = column_of(item_again);
    const bool alive = p < a.N;
    const size_t roff = (size_t)p * (128 * NB) + 32 * NB * w + 4 * NB * h;
    // the end point's position: into the output rows -- an inverse-L item's is wanted by nobody and is dropped (its last
    // list tile is padded with a repeated column: two lanes' rows would be the same row)
    if (!inverse) staged_end_x<NB>(sh.s, a.X_out, p, w, c, h, x);
    POT_ISTAMP(3);
    const double EXL = (double)exl;
    const double HL = EXL + EVL;
    if (inverse) {
      if (w == 0 && h == 0) a.Hwork[p] = HL;
      __syncthreads();
      POT_ISTAMP(4);
      continue;
    }

    if constexpr (MODE == kModeMJHMC) {
      // the jump process itself -- rates, clocks, first minimum, the successor of a move that is not L -- belongs to
      // pot64_decide_kernel, which runs when this launch's inverse-L items are done too: here the end point of L is
      // written as if taken (position: by the last drift), with its energies
      if (w == 0 && h == 0) {
        a.EX_out[p] = EXL;
        a.EV_out[p] = EVL;
      }
      staged_end_vg<NB>(sh.s, a.V_out, a.G_out, p, w, c, h, v, g);
      POT_ISTAMP(4);
      continue;
    }

    // the discrete-time and continuous-time control samplers decide here: lanes 0..31 of wave 0, one particle each
    if (w == 0 && h == 0) {
      const int64_t pp = alive ? p : 0;
      const uint32_t pid = (uint32_t)(a.first_pid + pp);
      const double EX0 = a.EX_in[p], EV0 = a.EV_in[p];
      const double H0 = EX0 + EV0;
      double best = 0.0;
      bool bad = false, gate = false;
      const int k = pot64_decide<REPLAY, MODE>(a, H0, HL, 0.0, pp, pid, best, bad, gate);
      if (bad && alive) tally[4] = 1;
      a.dwell[p] = best;
      a.dwell_ring[p] = best;
      a.trans[p] = (uint8_t)k;
      sh.s.move[c] = k | (gate ? 4 : 0);
      {
        // one LDS atomic per tally and tile (the 32 deciding lanes of wave 0)
        unsigned long long b0, b1, b2, b3 = 0ull;
        if constexpr (MODE == kModeControl) {  // l_count, f_count, R applied, fl_count (markov_jump_hmc.py:143-148)
          b0 = __ballot(alive && k == 3);
          b1 = __ballot(alive && k == 2);
          b2 = __ballot(alive && gate);
          b3 = __ballot(alive && k == 1);
        } else {
          b0 = __ballot(alive && k == 0);
          b1 = __ballot(alive && k == 1);
          b2 = __ballot(alive && k == 2);
        }
        if (c == 0) {
          if (b0) atomicAdd(&tally[0], (unsigned)__popcll(b0));
          if (b1) atomicAdd(&tally[1], (unsigned)__popcll(b1));
          if (b2) atomicAdd(&tally[2], (unsigned)__popcll(b2));
          if (b3) atomicAdd(&tally[3], (unsigned)__popcll(b3));
        }
      }
      // scalars of the successors that keep or take whole states; a refreshed kinetic energy is filled in below
      const bool took_L = MODE == kModeControl ? (k & 1) : (k == 0);
      a.EX_out[p] = took_L ? EXL : EX0;
      a.EV_out[p] = took_L ? EVL : EV0;
      a.Hflf_out[p] = __builtin_nan("");
    }
    __syncthreads();
    pot64_finish<NB, REPLAY, MODE, false>(a, sh, p, alive, roff, w, c, h, v, g);
    __syncthreads();
    POT_ISTAMP(4);
  }
  __syncthreads();
  if (threadIdx.x == 0 && tally[4]) {
    a.ctl->failed = 1;
    a.ctl->failed_iter = a.iter;
  }
  if (threadIdx.x < 4 && tally[threadIdx.x]) atomicAdd(&a.stats[threadIdx.x], (unsigned long long)tally[threadIdx.x]);
