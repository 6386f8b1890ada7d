// Wide samplers: the built-in elementwise energies with ndims beyond the register-resident kernels (Shape::wide), on the
// multi-pass engine (multipass.hip) -- their E and dE/dX on rows of any length, and the one-off operators of state_io.hip
// (evaluation, leapfrog) for such rows.  hk_energy_grad is a second implementation of the six energies of energies.hpp:
// its sums run in its own order (one wavefront per row), and the tests hold its bits.
#include <hip/hip_runtime.h>

#include "multipass.hpp"

namespace {

struct WideEnergy {
  int kind;
  double a, b, c;        // the functor constants of energies.hpp (IsoGaussF, RoughWellF, MMGaussF, FunnelNealF, FunnelRefF)
  const double* jdiag;   // DIAG_GAUSS
};

__device__ __forceinline__ double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__global__ void hk_energy_grad(const double* __restrict__ X, double* __restrict__ G, double* __restrict__ E, int64_t nrows,
                               int D, int pitch, const WideEnergy w) {
  const int64_t r = blockIdx.x;
  if (r >= nrows) return;
  const int lane = threadIdx.x;
  const double* x = X + r * pitch;
  double* g = G ? G + r * pitch : nullptr;
  const double pi = 3.141592653589793;
  double e = 0.0;
  switch (w.kind) {
    case MJHMC_E_ISO_GAUSS: {  // a = 1/sigma^2, b = 1/(2 sigma^2)
      double s = 0.0;
      for (int d = lane; d < D; d += 64) {
        const double xv = x[d];
        s = __builtin_fma(xv, xv, s);
        if (g) g[d] = xv * w.a;
      }
      e = wave_sum(s) * w.b;
      break;
    }
    case MJHMC_E_DIAG_GAUSS: {
      double s = 0.0;
      for (int d = lane; d < D; d += 64) {
        const double xv = x[d], j = w.jdiag[d];
        s = __builtin_fma(xv, j * xv, s);
        if (g) g[d] = j * xv;
      }
      e = wave_sum(s) / 2.0;
      break;
    }
    case MJHMC_E_ROUGH_WELL: {  // a = s1^2, b = 2 s1^2, c = s2 (distributions.py:295-304, operation order as written there)
      double s = 0.0;
      for (int d = lane; d < D; d += 64) {
        const double xv = x[d];
        s += (xv * xv) / w.b + cos(xv * 2.0 * pi / w.c);
        if (g) g[d] = xv / w.a + -sin(xv * 2.0 * pi / w.c) * 2.0 * pi / w.c;
      }
      e = wave_sum(s);
      break;
    }
    case MJHMC_E_MM_GAUSS: {  // a = 2 * separation (distributions.py:323-335)
      const double common = exp(4.0 * w.a * x[0]);
      double sa = 0.0, sb = 0.0;
      for (int d = lane; d < D; d += 64) {
        const double xv = x[d], sp = d == 0 ? w.a : 0.0;
        sa += (xv + sp) * (xv + sp);
        sb += (xv - sp) * (xv - sp);
        if (g) g[d] = (2.0 * ((xv - sp) * common + sp + xv)) / (common + 1.0);
      }
      e = -log(exp(-wave_sum(sa)) + exp(-wave_sum(sb)));
      break;
    }
    case MJHMC_E_FUNNEL_NEAL:    // a = 1/scale^2, b = (D-1)/2 (tf_distributions.py:143-147)
    case MJHMC_E_FUNNEL_REF: {   // a = 1/scale^2, b = D-1     (tf_distributions.py:157-165, as coded)
      const double x0 = x[0], ex = exp(-x0);
      double s = 0.0;
      for (int d = lane; d < D; d += 64) {
        const double xv = x[d];
        if (d > 0) s = __builtin_fma(xv, xv, s);
      }
      const double S = wave_sum(s);
      const bool neal = w.kind == MJHMC_E_FUNNEL_NEAL;
      if (g)
        for (int d = lane; d < D; d += 64) {
          if (d == 0) g[0] = neal ? (x0 * w.a - 0.5 * ex * S + w.b) : (-2.0 * w.b * x0 * w.a + ex * S);
          else g[d] = neal ? x[d] * ex : -2.0 * x[d] * ex;
        }
      e = neal ? (x0 * x0 * (0.5 * w.a) + 0.5 * ex * S + w.b * x0) : (-(w.b * x0 * x0 * w.a) - ex * S);
      break;
    }
    default: break;
  }
  if (E && lane == 0) E[r] = e;
}

int wide_energy_of(const mjhmc_energy* en, WideEnergy* w) {
  const EnergyParams& ep = en->ep;
  w->kind = ep.kind;
  w->a = w->b = w->c = 0.0;
  w->jdiag = (const double*)ep.dev_f64;
  switch (ep.kind) {
    case MJHMC_E_ISO_GAUSS: w->a = 1.0 / (ep.p[0] * ep.p[0]); w->b = 1.0 / (2.0 * (ep.p[0] * ep.p[0])); return 0;
    case MJHMC_E_DIAG_GAUSS: return 0;
    case MJHMC_E_ROUGH_WELL: w->a = ep.p[0] * ep.p[0]; w->b = 2.0 * (ep.p[0] * ep.p[0]); w->c = ep.p[1]; return 0;
    case MJHMC_E_MM_GAUSS: w->a = 2.0 * ep.p[0]; return 0;
    case MJHMC_E_FUNNEL_NEAL: w->a = 1.0 / (ep.p[0] * ep.p[0]); w->b = 0.5 * (ep.ndims - 1); return 0;
    case MJHMC_E_FUNNEL_REF: w->a = 1.0 / (ep.p[0] * ep.p[0]); w->b = (double)(ep.ndims - 1); return 0;
    default: return mjhmc_fail(MJHMC_ERR_UNSUPPORTED, "ndims too large for this energy's register-resident kernels, and it has no multi-pass form");
  }
}

}  // namespace

int wide_eval_rows(mjhmc_sampler* s, const double* X, double* G, double* E, int64_t nrows) {
  if (s->en->is_pot()) return pot_eval_rows_f64(s, X, G, E, nrows);
  WideEnergy w;
  TRY(wide_energy_of(s->en, &w));
  hipLaunchKernelGGL(hk_energy_grad, dim3((unsigned)nrows), dim3(64), 0, s->stream, X, G, E, nrows, s->D, s->sh.pitch, w);
  HIPCHK(hipGetLastError());
  return 0;
}

// run_eval of state_io.hip for a host energy or a wide sampler: the kinetic energy of V (or the tick-0 momentum) always; E and
// dE/dX from the device kernel for a wide sampler, the caller's (mjhmc_host_set_energy) for a host energy
int wide_run_eval(mjhmc_sampler* s, const void* X, void* Gout, void* Eout, const void* V, void* Vgen, void* EVout) {
  if (!s->en->is_host() && X && (Gout || Eout)) TRY(wide_eval_rows(s, (const double*)X, (double*)Gout, (double*)Eout, s->N));
  return host_run_eval(s, V, Vgen, EVout);
}

// mjhmc_leapfrog for a wide shape: n_steps of hmc_state.py:86-100 on rows X, V (device), literal operation order
int wide_leapfrog(mjhmc_sampler* w, const double* X, const double* V, double* Xo, double* Vo, double* G, double* EX,
                  double* EV, double eps, int n_steps) {
  const int64_t ne = w->Npad * w->sh.pitch, nv = w->N * w->sh.pitch;
  double* g = G;
  if (!g) HIPCHK(hipMalloc((void**)&g, (size_t)ne * sizeof(double)));
  auto body = [&]() -> int {
    HIPCHK(hipMemcpyAsync(Xo, X, (size_t)ne * sizeof(double), hipMemcpyDeviceToDevice, w->stream));
    HIPCHK(hipMemcpyAsync(Vo, V, (size_t)ne * sizeof(double), hipMemcpyDeviceToDevice, w->stream));
    TRY(wide_eval_rows(w, Xo, g, EX, w->N));
    const double c = -eps / 2.;
    for (int l = 0; l < n_steps; ++l) {
      rows_axpy(w->stream, Vo, g, c, nv);
      rows_axpy(w->stream, Xo, Vo, eps, nv);
      TRY(wide_eval_rows(w, Xo, g, EX, w->N));
      rows_axpy(w->stream, Vo, g, c, nv);
    }
    if (w->sh.round32) {   // float32-valued state: the end point is rounded, its energies and dE/dX are those of what is handed out
      TRY(round_rows32(w, Xo));
      TRY(round_rows32(w, Vo));
      TRY(wide_eval_rows(w, Xo, g, EX, w->N));
    }
    if (EV) rows_kinetic(w->stream, Vo, EV, w->N, w->D, w->sh.pitch);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(w->stream));
    return 0;
  };
  const int rc = body();
  if (!G && g) (void)hipFree(g);
  return rc;
}
