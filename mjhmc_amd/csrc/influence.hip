// Data-row influence of a linear-model energy (include/mjhmc_hip.h: mjhmc_influence_*): the
// D x K cross moments of the state with ONE value t_j = h(u_j, j) per expert, from which Cov(x_d, t_j) is formed on the
// host -- with t the pointwise log-likelihood, the first-order effect of deleting data row j on the posterior mean and the
// infinitesimal-jackknife covariance.  For the experts [j0, j1) the handle keeps, in float64 on the device,
//     W = sum w     Sx[d] = sum w (x_d - cx_d)     S2x[d] = sum w (x_d - cx_d)^2
//     St[j] = sum w (t_j - ct_j)     S2t[j] = sum w (t_j - ct_j)^2     Cxt[d][j] = sum w x_d (t_j - ct_j)
// x enters the cross sum about 0, as the gradient does in crossmoments.hip: with ct near the mean of t the sum has nothing
// large to cancel whatever the offset of x.
//
// The experts are walked in PANELS: panel i is block b0 + i of the model's P = 128 NB experts (b0 = j0 / P), of which the
// columns [lo_i, hi_i) lie inside [j0, j1).  Per recorded slot, in stream order on the sampler's stream:
//   1. a float64 slot is narrowed to the handle's float32 rows (pot_narrow_rows32, what its force is given); a float32
//      slot is read in place;
//   2. the moment pass of estimators.hip on the sample-ring slot about cx: W, Sx, S2x -- once per slot;
//   3. per panel, in ascending order:
//      a. the generated kernel (dense_lin_values.hpp): T[p][j - block] = the value, 0 where w == 0, p >= N or j outside;
//      b. the moment pass on T seen as a one-slot float32 ring of hi_i columns about ct: St, S2t of the panel;
//      c. the cross pass of crossmoments.hip, g = the sample-ring slot, b = the columns [lo_i, hi_i) of T, cb = ct:
//         the panel's D x (hi_i - lo_i) piece of Cxt.  (xcov_kernel pairs a float64 g with a float64 b only: for float64
//         state T is widened exactly to a float64 panel first.)
// Both passes are the library's own, unchanged: one fixed order of sums, no floating-point atomic; every slot is added to the
// totals separately and in slot order, so nothing depends on how a run is cut into calls.  Scratch is the panel and the
// passes' partials: a function of (N, D, P), not of K.  Cxt is stored panel by panel, [D][hi_i - lo_i] each, once.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/mjhmc_hip.h"
#include "crossmoments.hpp"
#include "dense_lin_values.hpp"
#include "estimators.hpp"
#include "handles.hpp"
#include "ring_rows.hpp"
#include "ring_source.hpp"

namespace {

// flags[0] = 1 when one of the n * N weights of the call is negative or not finite
__global__ __launch_bounds__(256) void inf_check_weights_kernel(const double* __restrict__ w, int64_t Npad, int64_t N, int n,
                                                                int* __restrict__ flags) {
  const int64_t total = (int64_t)n * N, stride = (int64_t)gridDim.x * 256;
  int badw = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const int64_t k = i / N, p = i - k * N;
    const double v = w[(size_t)k * Npad + p];
    if (!(v >= 0.0) || !mjhmc::finite_f64(v)) badw = 1;
  }
  if (badw) flags[0] = 1;
}

// the float32 panel widened exactly: what the cross pass pairs with a float64 state
__global__ __launch_bounds__(256) void inf_widen_kernel(const float* __restrict__ src, double* __restrict__ dst, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) dst[i] = (double)src[i];
}

struct Panel {
  int blk;        // the model's block
  int lo, hi;     // its columns inside [j0, j1)
  size_t coff;    // where its [D][hi - lo] piece of Cxt starts
  CrossPlan plan;
};

// one expression: no ';' outside it, something inside it
int checked_value(const char* value, std::string* out) {
  const std::string all(value);
  const size_t a = all.find_first_not_of(" \t\n"), b = all.find_last_not_of(" \t\n");
  if (a == std::string::npos) return mjhmc_fail(MJHMC_ERR_INVALID, "the value expression is empty");
  if (all.find(';') != std::string::npos)
    return mjhmc_fail(MJHMC_ERR_INVALID, "the influence pass takes ONE value expression per pass (no ';'): more than one value is "
                                         "more than one handle");
  *out = all.substr(a, b - a + 1);
  return 0;
}

}  // namespace

struct mjhmc_influence : RingAccumulator {
  using RingAccumulator::RingAccumulator;
  int D = 0, K = 0, P = 0;         // dims, the model's experts, the panel's side
  int j0 = 0, j1 = 0, b0 = 0;      // the experts asked for; the block of the first panel
  int ntiles = 0;
  std::vector<Panel> panels;
  hipModule_t module = nullptr;
  hipFunction_t fn = nullptr;
  float* X32 = nullptr;            // [Npad][P]: the float32 rows of a float64 slot
  float* T = nullptr;              // [Npad][P]: the panel
  double* T64 = nullptr;           // [Npad][P]: the panel widened, float64 state only
  EstimatorPlan xplan, tplan;      // the moment passes over the sample-ring slot and over the panel
  double* accx = nullptr;          // [1 + 2 D]: W, Sx, S2x
  double* acct = nullptr;          // [panels][1 + 2 P]: per panel W (not read), St, S2t of its columns [0, hi)
  double* Cxt = nullptr;           // the panels' pieces, [D][hi - lo] each
  double* cx = nullptr;            // [D]
  double* ct = nullptr;            // [panels][P]: entry j - b0 P
  double* mpart_x = nullptr;
  double* mpart_t = nullptr;
  double* xpart = nullptr;
  size_t scratch_bytes = 0;
  bool poisoned = false;           // a value that is not finite went into the sums: reset first
  // (`bad` holds two flags: [0] a refused weight, what the two passes obey; [1] the lowest expert of a value that is not
  // finite, kLvNoBad when there is none)
  size_t acct_elems() const { return panels.size() * (1 + 2 * (size_t)P); }
  size_t cxt_elems() const { return (size_t)D * (size_t)(j1 - j0); }
  ~mjhmc_influence() override {
    free_device({X32, T, T64, accx, acct, Cxt, cx, ct, mpart_x, mpart_t, xpart});
    if (module) (void)hipModuleUnload(module);
  }
};

namespace {

hipError_t inf_clear_flags(mjhmc_influence* h) {
  const int flags[2] = {0, mjhmc::kLvNoBad};
  hipError_t e = hipMemcpyAsync(h->bad, flags, sizeof(flags), hipMemcpyHostToDevice, h->s->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->s->stream);   // (flags is on this stack)
  return e;
}

hipError_t inf_zero_sums(mjhmc_influence* h) {
  hipStream_t st = h->s->stream;
  hipError_t e = hipMemsetAsync(h->accx, 0, (1 + 2 * (size_t)h->D) * sizeof(double), st);
  if (e == hipSuccess) e = hipMemsetAsync(h->acct, 0, h->acct_elems() * sizeof(double), st);
  if (e == hipSuccess) e = hipMemsetAsync(h->Cxt, 0, h->cxt_elems() * sizeof(double), st);
  if (e == hipSuccess) e = inf_clear_flags(h);
  return e;
}

}  // namespace

extern "C" {

int mjhmc_influence_check(int ndims, int64_t nexperts, const char* value, const char* include_dir) {
  if (!value || !include_dir) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  if (ndims < 1 || nexperts < 1) return mjhmc_fail(MJHMC_ERR_INVALID, "a linear model has ndims >= 1 and nexperts >= 1");
  if (ndims > kPotDim || nexperts > kLinTallMaxExperts)
    return mjhmc_fail(MJHMC_ERR_UNSUPPORTED, "linear models take at most 512 dims and 1048576 (2^20) experts (got " +
                                                 std::to_string(ndims) + " x " + std::to_string(nexperts) + ")");
  std::string v, err;
  TRY(checked_value(value, &v));
  const RtcCode* code = nullptr;
  const int rc = linear_values_compile(v, linear_pointwise_dim(ndims, nexperts), include_dir, &err, &code);
  return rc ? mjhmc_fail(rc, err) : 0;
}

int mjhmc_influence_create(mjhmc_sampler* s, const char* value, int64_t j0, int64_t j1, const char* include_dir,
                           mjhmc_influence** out) {
  if (!s || !value || !include_dir || !out) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  const mjhmc_energy* e = s->en;
  if (e->ep.kind != MJHMC_E_LINEAR_EXPR || !e->lin)
    return mjhmc_fail(MJHMC_ERR_UNSUPPORTED, std::string("the influence of a data row is that of an expert of a linear-model energy "
                                                         "(MJHMC_E_LINEAR_EXPR): the sampler's energy is MJHMC_E_") +
                                                 energy_kind_name(e->ep.kind) + ", which has no experts u = W x + b to report on");
  if (e->lin->grouped())
    return mjhmc_fail(MJHMC_ERR_UNSUPPORTED, "the influence of a data row of a grouped linear model (mjhmc_energy_create_linear_grouped) "
                                             "are not formed: its experts are stored in a permuted order and the terms of a group "
                                             "are coupled through its log-sum-exp, while this pass reports per expert in the "
                                             "caller's order");
  if (e->lin_wide())
    return mjhmc_fail(MJHMC_ERR_UNSUPPORTED, "the influence of a data row of a wide linear model (mjhmc_energy_create_linear_wide) is not formed: "
                                             "the per-expert passes take models of at most 512 dims, stored in one chunk of "
                                             "dims per block of experts");
  if (s->dtype != MJHMC_F64 && s->dtype != MJHMC_F32)
    return mjhmc_fail(MJHMC_ERR_UNSUPPORTED, "linear models run with float32 or float64 state");
  if (!s->ring) return acc_no_ring(nullptr);
  std::string v;
  TRY(checked_value(value, &v));
  const int K = e->lin->gen.lin.K;
  if (j0 < 0 || j1 > K || j0 >= j1)
    return mjhmc_fail(MJHMC_ERR_INVALID, "the experts [" + std::to_string(j0) + ", " + std::to_string(j1) +
                                             ") are not a range 0 <= j0 < j1 <= K of the model's K = " + std::to_string(K));
  const int P = e->pot_dim;
  if (s->sh.pitch != P) return mjhmc_fail(MJHMC_ERR_UNSUPPORTED, "the sampler's rows do not have the model's padded pitch");
  HIPCHK(hipSetDevice(s->ctx->device));
  std::string err;
  const RtcCode* code = nullptr;
  const int rc = linear_values_compile(v, P, include_dir, &err, &code);
  if (rc) return mjhmc_fail(rc, err);
  const RingSource src = ring_source(s, nullptr);
  mjhmc_influence* h = new mjhmc_influence("influence", "influence handle", s, nullptr, src);
  h->D = s->D;
  h->K = K;
  h->P = P;
  h->j0 = (int)j0;
  h->j1 = (int)j1;
  h->b0 = (int)j0 / P;
  h->ntiles = (int)((s->N + mjhmc::kP - 1) / mjhmc::kP);
  size_t coff = 0;
  for (int blk = h->b0; blk * P < h->j1; ++blk) {
    Panel pn;
    pn.blk = blk;
    pn.lo = std::max(h->j0, blk * P) - blk * P;
    pn.hi = std::min(h->j1, (blk + 1) * P) - blk * P;
    pn.coff = coff;
    pn.plan = cross_plan(s->N, h->D, pn.hi - pn.lo);
    coff += (size_t)h->D * (pn.hi - pn.lo);
    h->panels.push_back(pn);
  }
  h->xplan = estimator_plan(ring_source_view(s, src, 0), false);
  h->tplan = estimator_plan(RingView{nullptr, MJHMC_F32, s->Npad, s->N, P, P}, false);
  // the partials of the cross pass for every width a panel can have: a function of (N, D, P) alone
  size_t xpart_elems = 0;
  for (int wd = 64; wd <= P; wd += 64) xpart_elems = std::max(xpart_elems, cross_plan(s->N, h->D, wd).partial_elems);
  const size_t panel_elems = (size_t)s->Npad * P;
  const bool f64 = s->dtype == MJHMC_F64;
  h->scratch_bytes = panel_elems * sizeof(float) * (f64 ? 2 : 1) + (f64 ? panel_elems * sizeof(double) : 0) +
                     (xpart_elems + h->xplan.moment_partial_elems + h->tplan.moment_partial_elems) * sizeof(double);
  hipError_t he = hipModuleLoadData(&h->module, code->code.data());
  if (he == hipSuccess) he = hipModuleGetFunction(&h->fn, h->module, code->lowered[0].c_str());
  if (he == hipSuccess && f64) he = hipMalloc((void**)&h->X32, panel_elems * sizeof(float));
  if (he == hipSuccess && f64) he = hipMalloc((void**)&h->T64, panel_elems * sizeof(double));
  if (he == hipSuccess) he = hipMalloc((void**)&h->T, panel_elems * sizeof(float));
  if (he == hipSuccess) he = hipMalloc((void**)&h->accx, (1 + 2 * (size_t)h->D) * sizeof(double));
  if (he == hipSuccess) he = hipMalloc((void**)&h->cx, (size_t)h->D * sizeof(double));
  if (he == hipSuccess) he = hipMalloc((void**)&h->ct, h->panels.size() * P * sizeof(double));
  if (he == hipSuccess) he = hipMalloc((void**)&h->mpart_x, h->xplan.moment_partial_elems * sizeof(double));
  if (he == hipSuccess) he = hipMalloc((void**)&h->mpart_t, h->tplan.moment_partial_elems * sizeof(double));
  if (he == hipSuccess) he = hipMalloc((void**)&h->xpart, xpart_elems * sizeof(double));
  if (he == hipSuccess) he = hipMalloc((void**)&h->bad, 2 * sizeof(int));
  if (he != hipSuccess) {
    delete h;
    (void)hipGetLastError();
    return mjhmc_fail(MJHMC_ERR_HIP, std::string("influence buffers: ") + hipGetErrorString(he));
  }
  // the totals: the only allocation that grows with the experts asked for
  const size_t tot_bytes = (h->cxt_elems() + h->acct_elems()) * sizeof(double);
  he = hipMalloc((void**)&h->Cxt, h->cxt_elems() * sizeof(double));
  if (he == hipSuccess) he = hipMalloc((void**)&h->acct, h->acct_elems() * sizeof(double));
  if (he != hipSuccess) {
    delete h;
    (void)hipGetLastError();
    return mjhmc_fail(MJHMC_ERR_HIP, "the influence totals of " + std::to_string(s->D) + " dims x " + std::to_string(j1 - j0) +
                                         " experts need " + std::to_string(tot_bytes) + " bytes of device memory: the allocation "
                                         "failed (" + hipGetErrorString(he) + "); take the experts in ranges");
  }
  he = hipMemsetAsync(h->T, 0, panel_elems * sizeof(float), s->stream);
  if (he == hipSuccess) he = hipMemsetAsync(h->cx, 0, (size_t)h->D * sizeof(double), s->stream);
  if (he == hipSuccess) he = hipMemsetAsync(h->ct, 0, h->panels.size() * P * sizeof(double), s->stream);
  if (he == hipSuccess) he = inf_zero_sums(h);
  if (he != hipSuccess) {
    delete h;
    (void)hipGetLastError();
    return mjhmc_fail(MJHMC_ERR_HIP, std::string("influence buffers: ") + hipGetErrorString(he));
  }
  return acc_created(h, out);
}

int mjhmc_influence_destroy(mjhmc_influence* h) { return acc_destroy(h); }

int mjhmc_influence_info(mjhmc_influence* h, int* ndims, int64_t* j0, int64_t* j1, int* panel_experts, int64_t* scratch_bytes) {
  if (!h || !ndims || !j0 || !j1 || !panel_experts || !scratch_bytes) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  *ndims = h->D;
  *j0 = h->j0;
  *j1 = h->j1;
  *panel_experts = h->P;
  *scratch_bytes = (int64_t)h->scratch_bytes;
  return 0;
}

int mjhmc_influence_reset(mjhmc_influence* h) {
  if (!h) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  HIPCHK(hipSetDevice(h->s->ctx->device));
  HIPCHK(inf_zero_sums(h));
  h->n_states = 0;
  h->poisoned = false;
  return 0;
}

int mjhmc_influence_set_shift(mjhmc_influence* h, const double* cx, const double* ct) {
  if (!h) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  if (h->n_states != 0 || h->poisoned)
    return mjhmc_fail(MJHMC_ERR_INVALID, "the shifts belong to the sums already accumulated: mjhmc_influence_reset first");
  mjhmc_sampler* s = h->s;
  HIPCHK(hipSetDevice(s->ctx->device));
  const size_t nt = h->panels.size() * (size_t)h->P;
  std::vector<double> hx((size_t)h->D, 0.0), ht(nt, 0.0);
  if (cx)
    for (int d = 0; d < h->D; ++d) {
      if (!std::isfinite(cx[d])) return mjhmc_fail(MJHMC_ERR_INVALID, "state shift entry " + std::to_string(d) + " is not finite");
      hx[(size_t)d] = cx[d];
    }
  if (ct)
    for (int j = h->j0; j < h->j1; ++j) {
      if (!std::isfinite(ct[j - h->j0]))
        return mjhmc_fail(MJHMC_ERR_INVALID, "value shift entry " + std::to_string(j - h->j0) + " is not finite");
      ht[(size_t)(j - h->b0 * h->P)] = ct[j - h->j0];
    }
  HIPCHK(hipMemcpyAsync(h->cx, hx.data(), hx.size() * sizeof(double), hipMemcpyHostToDevice, s->stream));
  HIPCHK(hipMemcpyAsync(h->ct, ht.data(), ht.size() * sizeof(double), hipMemcpyHostToDevice, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));   // (the vectors are this call's)
  return 0;
}

int mjhmc_influence_accumulate(mjhmc_influence* h, int x_slot0, int w_slot0, int n) {
  if (!h) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  mjhmc_sampler* s = h->s;
  if (h->poisoned)
    return mjhmc_fail(MJHMC_ERR_INVALID, "the sums hold a value that is not finite (an earlier mjhmc_influence_accumulate said "
                                         "which): mjhmc_influence_reset first");
  RingSource src;
  TRY(acc_begin(h, x_slot0, w_slot0, n, &src));
  HIPCHK(hipSetDevice(s->ctx->device));
  if (w_slot0 >= 0)
    hipLaunchKernelGGL(inf_check_weights_kernel, dim3((unsigned)std::min<int64_t>(1024, ((int64_t)n * s->N + 255) / 256)), dim3(256),
                       0, s->stream, acc_weights(h, w_slot0), s->Npad, s->N, n, h->bad);
  const mjhmc_energy* e = s->en;
  const int P = h->P;
  const int nblk = e->lin_tall() ? e->lin->tall_nblk : 1;
  const mjhmc::LinTallModel tm{e->pot[0], e->pot[1], e->pot[2], nblk, s->D, h->K};
  const mjhmc::PotLinear lin = e->lin->gen.lin;
  const unsigned grid = (unsigned)std::min<int64_t>(h->ntiles, std::max(1, s->ctx->prop.multiProcessorCount));
  const int64_t panel_elems = s->Npad * (int64_t)P;
  const bool f64 = s->dtype == MJHMC_F64;
  std::string err;
  int rc = 0;
  for (int k = 0; k < n && !rc; ++k) {
    const RingView xview = ring_source_view(s, src, x_slot0 + k);
    const double* w = w_slot0 >= 0 ? acc_weights(h, w_slot0 + k) : nullptr;
    mjhmc::LvArgs a;
    if (f64) {
      pot_narrow_rows32((const double*)xview.base, h->X32, panel_elems, s->stream);
      a.X = h->X32;
    } else {
      a.X = (const float*)xview.base;
    }
    a.w = w;
    a.T = h->T;
    a.flags = h->bad + 1;
    a.N = s->N;
    a.ntiles = h->ntiles;
    a.jlo = h->j0;
    a.jhi = h->j1;
    rc = estimator_moments(s->stream, xview, 1, w, h->cx, h->xplan, h->mpart_x, h->accx, h->bad, err);
    for (size_t i = 0; i < h->panels.size() && !rc; ++i) {
      const Panel& pn = h->panels[i];
      a.blk = pn.blk;
      void* params[] = {(void*)&a, (void*)&tm, (void*)&lin};
      const hipError_t le = hipModuleLaunchKernel(h->fn, grid, 1, 1, 256, 1, 1, 0, s->stream, params, nullptr);
      if (le != hipSuccess) {
        err = std::string("values kernel: ") + hipGetErrorString(le);
        rc = MJHMC_ERR_HIP;
        break;
      }
      if (f64)
        hipLaunchKernelGGL(inf_widen_kernel, dim3((unsigned)std::min<int64_t>(4096, (panel_elems + 255) / 256)), dim3(256), 0,
                           s->stream, h->T, h->T64, panel_elems);
      const double* ct = h->ct + i * (size_t)P;
      const RingView tview{h->T, MJHMC_F32, s->Npad, s->N, pn.hi, P};
      const RingView bview = f64 ? RingView{h->T64 + pn.lo, MJHMC_F64, s->Npad, s->N, pn.hi - pn.lo, P}
                                 : RingView{h->T + pn.lo, MJHMC_F32, s->Npad, s->N, pn.hi - pn.lo, P};
      rc = estimator_moments(s->stream, tview, 1, w, ct, h->tplan, h->mpart_t, h->acct + i * (1 + 2 * (size_t)P), h->bad, err);
      if (!rc) rc = cross_cov(s->stream, xview, bview, w, ct + pn.lo, pn.plan, h->xpart, h->Cxt + pn.coff, h->bad, err);
    }
  }
  if (rc) {
    h->poisoned = true;   // (part of the call may be in the sums)
    return mjhmc_fail(rc, err);
  }
  HIPCHK(hipGetLastError());
  int flags[2] = {0, mjhmc::kLvNoBad};
  HIPCHK(hipMemcpyAsync(flags, h->bad, sizeof(flags), hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  if (flags[0] || flags[1] != mjhmc::kLvNoBad) HIPCHK(inf_clear_flags(h));
  if (flags[0])   // (every fold of the call saw the flag: nothing was added)
    return mjhmc_fail(MJHMC_ERR_NONFINITE, "a weight in dwell slots [" + std::to_string(w_slot0) + ", " + std::to_string(w_slot0 + n) +
                                               ") is negative or not finite: nothing of this call was added");
  if (flags[1] != mjhmc::kLvNoBad) {
    h->poisoned = true;
    return mjhmc_fail(MJHMC_ERR_NONFINITE, "the value at expert " + std::to_string(flags[1]) +
                                               " is not finite for a particle of positive weight in state slots [" +
                                               std::to_string(x_slot0) + ", " + std::to_string(x_slot0 + n) +
                                               "): the sums hold it -- mjhmc_influence_reset before any further call");
  }
  h->n_states += (int64_t)n * s->N;
  return 0;
}

int mjhmc_influence_read(mjhmc_influence* h, double* W, double* Sx, double* S2x, double* St, double* S2t, int64_t* n_states) {
  if (!h || !W || !Sx || !S2x || !St || !S2t || !n_states) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  mjhmc_sampler* s = h->s;
  HIPCHK(hipSetDevice(s->ctx->device));
  const size_t D = (size_t)h->D, stride = 1 + 2 * (size_t)h->P;
  std::vector<double> hx(1 + 2 * D), ht(h->acct_elems());
  HIPCHK(hipMemcpyAsync(hx.data(), h->accx, hx.size() * sizeof(double), hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipMemcpyAsync(ht.data(), h->acct, ht.size() * sizeof(double), hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  *W = hx[0];   // (the sample ring's own moment pass: bit for bit the W of an estimator on the same slots, slot by slot)
  std::copy(hx.begin() + 1, hx.begin() + 1 + D, Sx);
  std::copy(hx.begin() + 1 + D, hx.end(), S2x);
  size_t o = 0;
  for (size_t i = 0; i < h->panels.size(); ++i) {
    const Panel& pn = h->panels[i];
    const double* acc = ht.data() + i * stride;   // [0] W, then S1[hi], S2[hi]
    for (int c = pn.lo; c < pn.hi; ++c, ++o) {
      St[o] = acc[1 + c];
      S2t[o] = acc[1 + pn.hi + c];
    }
  }
  *n_states = h->n_states;
  return 0;
}

int mjhmc_influence_read_cross(mjhmc_influence* h, int64_t ja, int64_t jb, double* Cxt_out) {
  if (!h || !Cxt_out) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  if (ja < h->j0 || jb > h->j1 || ja >= jb)
    return mjhmc_fail(MJHMC_ERR_INVALID, "the columns [" + std::to_string(ja) + ", " + std::to_string(jb) +
                                             ") are not a range inside the handle's experts [" + std::to_string(h->j0) + ", " +
                                             std::to_string(h->j1) + ")");
  mjhmc_sampler* s = h->s;
  HIPCHK(hipSetDevice(s->ctx->device));
  HIPCHK(hipStreamSynchronize(s->stream));
  const size_t out_cols = (size_t)(jb - ja);
  for (const Panel& pn : h->panels) {
    const int64_t base = (int64_t)pn.blk * h->P;
    const int64_t a = std::max<int64_t>(ja, base + pn.lo), b = std::min<int64_t>(jb, base + pn.hi);
    if (a >= b) continue;
    const size_t wd = (size_t)(pn.hi - pn.lo);
    HIPCHK(hipMemcpy2D(Cxt_out + (a - ja), out_cols * sizeof(double), h->Cxt + pn.coff + (size_t)(a - base - pn.lo),
                       wd * sizeof(double), (size_t)(b - a) * sizeof(double), (size_t)h->D, hipMemcpyDeviceToHost));
  }
  return 0;
}

}  // extern "C"
