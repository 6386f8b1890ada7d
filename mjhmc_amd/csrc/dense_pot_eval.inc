// Body of a float32-state tile kernel, included INSIDE the kernel definition (dense_pot.hip; linear_energy.hip for the
// kernels of a linear-model energy): evaluation: E(X), dEdX(X), optional kinetic energy / generated momentum (HMCState.__init__).
// In scope: template parameters NB (and REPLAY, MODE), the arguments `a` and `mdl`, the experts `xp`.
  __shared__ Shared<NB> sh;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 31, h = lane >> 5;
  AReg<NB> ar;
  areg_load<NB>(mdl, w, c, h, ar);
  stage_bias<NB>(mdl, sh);
  for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int64_t p = tile * kP + c;
    Tile<NB> x, g;
    tile_load<NB>(a.X, p, w, h, x);
    float ex = 0.f;
    pot_gradient<NB>(mdl, xp, ar, sh, w, c, h, lane, x, g, true, &ex);
    if (a.G) tile_store<NB>(a.G, p, w, h, g);
    if (a.E && w == 0 && h == 0) a.E[p] = ex;
    if (a.EV) {
      Tile<NB> v;
      if (a.V_gen) {
        pot_normals<NB>(a.key, (uint32_t)(a.first_pid + (p < a.N ? p : 0)), w, h, a.D, v);
        tile_store<NB>(a.V_gen, p, w, h, v);
      } else {
        tile_load<NB>(a.V, p, w, h, v);
      }
      const float ev = pot_kinetic<NB>(sh, w, c, h, v);
      if (w == 0 && h == 0) a.EV[p] = ev;
    }
    __syncthreads();
  }
