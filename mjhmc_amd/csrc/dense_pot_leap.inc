// Body of a float32-state tile kernel, included INSIDE the kernel definition (dense_pot.hip; linear_energy.hip for the
// kernels of a linear-model energy): HMCState.leapfrog / HMCState.L on caller-supplied states
// (hmc_state.py:86-100; figures/poe_fig.py:59 assigns and integrates states of a ProductOfT sampler): dE/dX at the start
// point, L steps, energies of the end point.
// In scope: template parameters NB (and REPLAY, MODE), the arguments `a` and `mdl`, the experts `xp`.
  __shared__ Shared<NB> sh;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 31, h = lane >> 5;
  AReg<NB> ar;
  areg_load<NB>(mdl, w, c, h, ar);
  stage_bias<NB>(mdl, sh);
  for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int64_t p = tile * kP + c;
    Tile<NB> x, v, g;
    tile_load<NB>(a.X, p, w, h, x);
    tile_load<NB>(a.V, p, w, h, v);
    float ex = 0.f;
    pot_gradient<NB>(mdl, xp, ar, sh, w, c, h, lane, x, g, true, &ex);
    __syncthreads();
    pot_trajectory<NB>(mdl, xp, ar, sh, w, c, h, lane, x, v, g, a.L, a.eps, a.chalf, &ex);
    const float ev = pot_kinetic<NB>(sh, w, c, h, v);
    tile_store<NB>(a.X_out, p, w, h, x);
    tile_store<NB>(a.V_out, p, w, h, v);
    if (a.G) tile_store<NB>(a.G, p, w, h, g);
    if (w == 0 && h == 0) {
      if (a.EX) a.EX[p] = ex;
      if (a.EV) a.EV[p] = ev;
    }
    __syncthreads();
  }
