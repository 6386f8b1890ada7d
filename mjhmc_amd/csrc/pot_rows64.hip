// ProductOfT as the reference runs it (distributions.py:408-415 with hmc_state.py:29-38): float64 HMCState arrays around
// a float32 force -- the inputs are downcast (allow_input_downcast=True), E and dE/dX come back as float32.  The force is
// the float32 matrix-core evaluation of dense_pot.hip on a float32 copy of the rows (the blocked evaluation beyond 512
// dims, the fused kernel of a tall linear model); this unit holds the float64 rows around it on the multi-pass engine
// (multipass.hip): the one-off evaluation, and the trajectory in one fused row pass per leapfrog step.
#include <hip/hip_runtime.h>

#include "multipass.hpp"

namespace {

__global__ void hk_narrow(const double* __restrict__ src, float* __restrict__ dst, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = (float)src[i];
}
__global__ void hk_widen(const float* __restrict__ src, double* __restrict__ dst, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = (double)src[i];
}

// One leapfrog step of ProductOfT's float64-state path in ONE pass over the rows: [closing half kick of the previous
// step] + opening half kick + drift + the float32 copy the force kernel reads.  Same operations in the same order as the
// separate passes (every product rounded before its sum; two half kicks stay two roundings), 2 GB instead of 4.5 GB of
// HBM traffic per step at 512 x 100 000.
template <bool G32>
__global__ void hk_pot_kick_drift(double* __restrict__ X, double* __restrict__ V, const void* __restrict__ Gsrc,
                                  float* __restrict__ X32, double c, double eps, int closing, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double g = G32 ? (double)((const float*)Gsrc)[i] : ((const double*)Gsrc)[i];
  double v = V[i];
  if (closing) v = v + c * g;
  v = v + c * g;
  const double x = X[i] + eps * v;
  V[i] = v;
  X[i] = x;
  X32[i] = (float)x;
}
// closing half kick from the float32 force; the stored dE/dX in float64
__global__ void hk_pot_close(double* __restrict__ V, const float* __restrict__ G32, double* __restrict__ G64, double c, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double g = (double)G32[i];
  V[i] = V[i] + c * g;
  G64[i] = g;
}

// the float32 force on rows buf[0] ([rows_pad][pitch] float32) -> dE/dX rows buf[1] (or none) and E buf[2] (or none): the
// tile kernel's evaluation up to 512 dims, the blocked evaluation (buf[3]: its u rows) beyond, the fused kernel of a tall or
// wide linear model
void pot_force32(mjhmc_sampler* s, float* const* buf, bool want_G, bool want_E, int64_t rows_pad, int64_t nrows) {
  if (s->en->pot_big()) {
    pot_big_eval(s->en->pot_big_model(), buf[0], want_G ? buf[1] : nullptr, want_E ? buf[2] : nullptr, buf[3], rows_pad, s->stream);
    return;
  }
  if (s->en->lin_tall()) {   // the fused block-by-block kernel of a tall linear model (no u rows: buf[3] is not used)
    lin_tall_eval(s->en, buf[0], want_G ? buf[1] : nullptr, want_E ? buf[2] : nullptr, rows_pad, nrows, s->stream);
    return;
  }
  if (s->en->lin_wide()) {   // the fused kernel of a wide linear model: rows of pitch 512 ND, dE/dX rows that need no zeroing
    lin_wide_eval(s->en, buf[0], want_G ? buf[1] : nullptr, want_E ? buf[2] : nullptr, rows_pad, nrows, s->stream);
    return;
  }
  PotEvalArgs a;
  a.X = buf[0];
  a.G = want_G ? buf[1] : nullptr;
  a.E = want_E ? buf[2] : nullptr;
  a.EV = nullptr;
  a.V = nullptr;
  a.V_gen = nullptr;
  a.N = nrows;
  a.ntiles = rows_pad / 32;
  a.first_pid = 0;
  a.D = s->D;
  a.key = RngKey{0u, 0u, 0u, 0u};
  pot_launch_eval(a, s->en->pot_model(), s->stream, s->en->pot_gen());
}

}  // namespace

int PotRows32::ensure(size_t cap_rows, int pitch, bool big) {
  if (buf[0]) return 0;
  HIPCHK(hipMalloc((void**)&buf[0], cap_rows * pitch * sizeof(float)));
  HIPCHK(hipMalloc((void**)&buf[1], cap_rows * pitch * sizeof(float)));
  HIPCHK(hipMalloc((void**)&buf[2], cap_rows * sizeof(float)));
  if (big) HIPCHK(hipMalloc((void**)&buf[3], cap_rows * pitch * sizeof(float)));
  return 0;
}

void PotRows32::release() {
  for (float*& b : buf) {
    if (b) (void)hipFree(b);
    b = nullptr;
  }
}

// the float32 copy of float64 rows the float32 force reads (pot_eval_rows_f64), for the other readers of a float64 slot
void pot_narrow_rows32(const double* src, float* dst, int64_t n, hipStream_t st) {
  hipLaunchKernelGGL(hk_narrow, grid1(n), dim3(256), 0, st, src, dst, n);
}

// E and dE/dX of float64 rows X through the float32 force: in the workspace's float32 rows when they hold rows_pad rows,
// in a set of its own otherwise (a sampler without workspace, mjhmc_eval / mjhmc_leapfrog of more rows), which the call
// waits for and releases on every way out
int pot_eval_rows_f64(mjhmc_sampler* s, const double* X, double* G, double* E, int64_t nrows) {
  const int pitch = s->sh.pitch;
  const int64_t rows_pad = (nrows + 63) / 64 * 64, ne = rows_pad * pitch;
  const bool own = !(s->prop && rows_pad <= 2 * s->Npad);
  PotRows32 one_off;
  PotRows32& rows = own ? one_off : s->prop->pot32;
  TRY(rows.ensure(own ? (size_t)rows_pad : (size_t)2 * s->Npad, pitch, s->en->pot_big()));
  float* const* buf = rows.buf;
  HIPCHK(hipMemsetAsync(buf[0], 0, (size_t)ne * sizeof(float), s->stream));  // rows beyond nrows: zeros, never NaN garbage
  hipLaunchKernelGGL(hk_narrow, grid1(nrows * pitch), dim3(256), 0, s->stream, X, buf[0], nrows * pitch);
  pot_force32(s, buf, G != nullptr, E != nullptr, rows_pad, nrows);
  if (G) hipLaunchKernelGGL(hk_widen, grid1(nrows * pitch), dim3(256), 0, s->stream, (const float*)buf[1], G, nrows * pitch);
  if (E) hipLaunchKernelGGL(hk_widen, grid1(nrows), dim3(256), 0, s->stream, (const float*)buf[2], E, nrows);
  HIPCHK(hipGetLastError());
  if (own) HIPCHK(hipStreamSynchronize(s->stream));
  return 0;
}

// the L leapfrog steps of ProductOfT's float64-state path on the proposal columns: per step one fused row pass
// (hk_pot_kick_drift) and one float32 matrix-core force evaluation (pot_launch_eval); the first step's force is the stored
// float64 dE/dX, the later ones the float32 output of the previous evaluation, exactly as the separate passes use them
int pot_trajectory_f64(mjhmc_sampler* s) {
  ProposalRows* t = s->prop;
  const int pitch = s->sh.pitch;
  const int64_t n = t->n_cols, rows_pad = (n + 63) / 64 * 64, ne = n * pitch;
  TRY(t->pot32.ensure((size_t)2 * s->Npad, pitch, s->en->pot_big()));
  float* const* buf = t->pot32.buf;
  HIPCHK(hipMemsetAsync(buf[0], 0, (size_t)rows_pad * pitch * sizeof(float), s->stream));  // rows beyond n: zeros
  const double c = -s->eps / 2.;
  for (int l = 0; l < s->L; ++l) {
    if (l == 0)
      hipLaunchKernelGGL(hk_pot_kick_drift<false>, grid1(ne), dim3(256), 0, s->stream, t->X, t->V, (const void*)t->G, buf[0], c,
                         s->eps, 0, ne);
    else
      hipLaunchKernelGGL(hk_pot_kick_drift<true>, grid1(ne), dim3(256), 0, s->stream, t->X, t->V, (const void*)buf[1], buf[0], c,
                         s->eps, 1, ne);
    pot_force32(s, buf, true, l == s->L - 1, rows_pad, n);
    t->steps += 1;
  }
  hipLaunchKernelGGL(hk_pot_close, grid1(ne), dim3(256), 0, s->stream, t->V, (const float*)buf[1], t->G, c, ne);
  hipLaunchKernelGGL(hk_widen, grid1(n), dim3(256), 0, s->stream, (const float*)buf[2], t->E, n);
  HIPCHK(hipGetLastError());
  return 0;
}
