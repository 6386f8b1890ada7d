// Kernel Stein discrepancy of a recorded ensemble (include/mjhmc_hip.h: mjhmc_stein_*; kernels and the definition in
// stein.hpp).  The handle owns what one evaluation needs -- dE/dX and E of ONE slot in the layout and types the energy
// family writes (as the energy observables' scratch, functionals.hip), one (S, Sd) partial per tile of pairs, the four
// results and the flag word -- and evaluate is: the sampler's own evaluation kernels on the slot (state_io.hip:
// sampler_eval_rows), the pair kernel, the finish kernel, one read-back; all on the sampler's stream.
//   float64 state  -> float64 dE/dX   (elementwise and user-expression energies, the wide / multi-pass path, ProductOfT
//                                      and linear models with float64 state)
//   float32 state  -> float32 dE/dX   (elementwise energies, ProductOfT and linear models, SparseImageCode)
//   bfloat16 state -> float32 dE/dX   (SparseImageCode: [Npad][ndims], pitch == ndims)
#include "stein.hpp"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <string>

#include "../../include/mjhmc_hip.h"
#include "handles.hpp"

struct mjhmc_stein {
  mjhmc_sampler* s = nullptr;
  double c = 0;
  uint64_t src_gen = 0;     // the sampler's ring at create
  void* G = nullptr;        // [Npad][pitch] float64 (float64 state) or float32
  void* E = nullptr;        // [Npad] of the same type
  double* part = nullptr;   // [tiles(N)][2]
  char* res = nullptr;      // {double out[4]; int bad;}: what one evaluation reads back
};

namespace {

struct SteinResult {
  double out[4];
  int bad;
};

long long stein_tiles(long long n) {
  const long long nt = (n + mjhmc::kSteinTile - 1) / mjhmc::kSteinTile;
  return nt * (nt + 1) / 2;
}

void stein_free(mjhmc_stein* k) {
  for (void* p : {k->G, k->E, (void*)k->part, (void*)k->res})
    if (p) (void)hipFree(p);
  delete k;
}

}  // namespace

namespace mjhmc {

bool stein_launch(const SteinArgs& a, int state_dtype, bool grad_f32, hipStream_t stream) {
  const dim3 grid((unsigned)a.n_tiles), block(256);
  if (state_dtype == 0 && !grad_f32) hipLaunchKernelGGL((stein_pair_kernel<0, 0>), grid, block, 0, stream, a);
  else if (state_dtype == 1 && grad_f32) hipLaunchKernelGGL((stein_pair_kernel<1, 1>), grid, block, 0, stream, a);
  else if (state_dtype == 2 && grad_f32) hipLaunchKernelGGL((stein_pair_kernel<2, 1>), grid, block, 0, stream, a);
  else return false;
  hipLaunchKernelGGL(stein_finish_kernel, dim3(1), block, 0, stream, a);
  return true;
}

}  // namespace mjhmc

void stein_free_all(mjhmc_sampler* s) {
  for (mjhmc_stein* k : s->steins) stein_free(k);
  s->steins.clear();
}

extern "C" {

int mjhmc_stein_create(mjhmc_sampler* s, double c, mjhmc_stein** out) {
  if (!s || !out) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  if (!std::isfinite(c) || !(c > 0)) return mjhmc_fail(MJHMC_ERR_INVALID, "the kernel scale c must be finite and > 0");
  if (s->en->is_host())
    return mjhmc_fail(MJHMC_ERR_UNSUPPORTED,
                      "a host-evaluated energy has no device evaluation: the caller's callables are the only evaluation of "
                      "dE/dX, so the Stein discrepancy of its states is the caller's to form");
  if (!s->ring) return mjhmc_fail(MJHMC_ERR_INVALID, "the sampler has no sample ring yet (call mjhmc_ring_alloc first)");
  // the kernel loads four elements of a row at once: rows must be whole 16-byte chunks of the state's type
  const int vec = s->dtype == MJHMC_F64 ? 2 : (s->dtype == MJHMC_F32 ? 4 : 8);
  if (s->sh.esize * vec != 16 || s->sh.pitch % vec != 0)
    return mjhmc_fail(MJHMC_ERR_UNSUPPORTED, "the sampler's rows are not whole 16-byte chunks of its state type");
  const long long tiles = stein_tiles(s->N);
  if (tiles > 0x7FFFFFFFll) return mjhmc_fail(MJHMC_ERR_UNSUPPORTED, "too many particles for one launch of the Stein pair pass");
  HIPCHK(hipSetDevice(s->ctx->device));
  mjhmc_stein* k = new mjhmc_stein();
  k->s = s;
  k->c = c;
  k->src_gen = s->ring_gen;
  // dE/dX has the state's row pitch in every family and is float64 exactly where the state is (functionals.hip)
  const size_t gsize = s->dtype == MJHMC_F64 ? 8 : 4;
  const size_t gbytes = (size_t)s->Npad * s->sh.pitch * gsize, ebytes = (size_t)s->Npad * gsize;
  hipError_t e = hipMalloc(&k->G, gbytes);
  if (e == hipSuccess) e = hipMalloc(&k->E, ebytes);
  if (e == hipSuccess) e = hipMalloc((void**)&k->part, (size_t)tiles * 2 * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&k->res, sizeof(SteinResult));
  if (e == hipSuccess) e = hipMemsetAsync(k->G, 0, gbytes, s->stream);
  if (e == hipSuccess) e = hipMemsetAsync(k->E, 0, ebytes, s->stream);
  if (e == hipSuccess) e = hipMemsetAsync(k->res, 0, sizeof(SteinResult), s->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
  if (e != hipSuccess) {
    stein_free(k);
    (void)hipGetLastError();
    return mjhmc_fail(MJHMC_ERR_HIP, std::string("stein: ") + hipGetErrorString(e));
  }
  s->steins.push_back(k);
  *out = k;
  return 0;
}

int mjhmc_stein_evaluate(mjhmc_stein* k, int x_slot, int w_slot, int64_t n_use, double out[4]) {
  if (!k || !out) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  mjhmc_sampler* s = k->s;
  if (k->src_gen != s->ring_gen)
    return mjhmc_fail(MJHMC_ERR_INVALID, "the sample ring was re-allocated after mjhmc_stein_create: create a new one");
  if (x_slot < 0 || x_slot >= s->ring_slots)
    return mjhmc_fail(MJHMC_ERR_INVALID, "state slot " + std::to_string(x_slot) + " is outside the ring of " +
                                             std::to_string(s->ring_slots));
  if (w_slot < -1 || w_slot >= s->ring_slots)
    return mjhmc_fail(MJHMC_ERR_INVALID, "dwell slot " + std::to_string(w_slot) + " is outside the ring of " +
                                             std::to_string(s->ring_slots));
  if (n_use < 1 || n_use > s->N)
    return mjhmc_fail(MJHMC_ERR_INVALID, "n_use must be in [1, " + std::to_string(s->N) + "], got " + std::to_string(n_use));
  HIPCHK(hipSetDevice(s->ctx->device));
  const char* X = (const char*)s->ring + (size_t)x_slot * mat_bytes(s);
  HIPCHK(hipMemsetAsync(k->res, 0, sizeof(SteinResult), s->stream));
  TRY(sampler_eval_rows(s, X, k->G, k->E));
  mjhmc::SteinArgs a;
  a.X = X;
  a.G = k->G;
  a.w = w_slot >= 0 ? s->dwell_ring + (size_t)w_slot * s->Npad : nullptr;
  a.part = k->part;
  a.out = reinterpret_cast<double*>(k->res);
  a.bad = reinterpret_cast<int*>(k->res + offsetof(SteinResult, bad));
  a.n_use = n_use;
  a.n_tiles = stein_tiles(n_use);
  a.D = s->D;
  a.pitch = s->sh.pitch;
  a.c2 = k->c * k->c;
  a.nd = (double)s->D;
  if (!mjhmc::stein_launch(a, s->dtype, s->dtype != MJHMC_F64, s->stream))
    return mjhmc_fail(MJHMC_ERR_UNSUPPORTED, "no Stein pair kernel for this state type");
  HIPCHK(hipGetLastError());
  SteinResult r;
  HIPCHK(hipMemcpyAsync(&r, k->res, sizeof(SteinResult), hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  if (r.bad == mjhmc::kSteinBadSum)
    return mjhmc_fail(MJHMC_ERR_NONFINITE, "the pair sums of slot " + std::to_string(x_slot) +
                                               " overflow float64 although every weight, state and gradient is finite");
  if (r.bad) {
    const char* what = (r.bad & mjhmc::kSteinBadWeight) ? "a weight" : (r.bad & mjhmc::kSteinBadState) ? "a state" : "a gradient (dE/dX)";
    std::string where = (r.bad & mjhmc::kSteinBadWeight) ? " in dwell slot " + std::to_string(w_slot) : " in slot " + std::to_string(x_slot);
    return mjhmc_fail(MJHMC_ERR_NONFINITE, std::string(what) + " among the first " + std::to_string(n_use) + " particles" + where +
                                               " is not finite: the Stein discrepancy of this ensemble is not defined");
  }
  for (int i = 0; i < 4; ++i) out[i] = r.out[i];
  return 0;
}

int mjhmc_stein_destroy(mjhmc_stein* k) {
  if (!k) return 0;
  mjhmc_sampler* s = k->s;
  (void)hipSetDevice(s->ctx->device);
  if (s->stream) (void)hipStreamSynchronize(s->stream);
  s->steins.erase(std::remove(s->steins.begin(), s->steins.end(), k), s->steins.end());
  stein_free(k);
  return 0;
}

}  // extern "C"
