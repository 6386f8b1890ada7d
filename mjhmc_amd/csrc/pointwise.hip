// Per-expert statistics of a linear-model energy over blocks of the sample ring (include/mjhmc_hip.h: mjhmc_pointwise_*;
// the kernel and the order of its sums in dense_lin_pointwise.hpp).
//
// Per recorded slot, in stream order on the sampler's stream:
//   1. a float64 slot is narrowed to the handle's float32 rows (the multi-pass path's own narrowing, pot_rows64.hip); a
//      float32 slot is read in place -- either way [Npad][P] float32 with the rows beyond the batch zero, what the float32
//      force is given;
//   2. the generated kernel over the items (strip, block of experts): one partial (S1, S2, mx, se) per strip, value and
//      expert, and the strip's sum of weights;
//   3. the fold of this file: per expert the strips in ascending order into the slot's sum, the slot's sum onto the
//      running totals.
// The running totals exist twice.  A call folds its slots onto a COPY of the totals and the copy becomes the totals when
// the call's one read-back shows no flag: a refused call (a weight that is negative or not finite, a value that is not
// finite) has added nothing.  Every slot goes onto the totals separately and in slot order, so the sums do not depend on
// how a run is cut into calls.
// A grouped model's handle (mjhmc_pointwise_create_grouped; the kernel in dense_lin_group_pointwise.hpp, DESIGN.md section
// 3.3o) is the same handle with columns in place of experts: G C of them when a value is per member, G otherwise, the
// grouped blocks alone as its items.  The kernel writes the columns a value has; the partials are set empty once, at
// creation, so the columns G .. G C - 1 of a per-group value stay (0, 0, -inf, 0) through every fold.
#include "dense_lin_group_pointwise.hpp"
#include "dense_lin_pointwise.hpp"

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/mjhmc_hip.h"
#include "handles.hpp"
#include "ring_source.hpp"

namespace {

// totals: [0] W, [1] unused, then S1, S2, mx, se as [4][M][K]
constexpr size_t kPwTotHead = 2;

__global__ __launch_bounds__(256) void pw_init_kernel(double* __restrict__ tot, size_t MK) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < kPwTotHead) tot[i] = 0.0;
  if (i < 4 * MK) tot[kPwTotHead + i] = (i >= 2 * MK && i < 3 * MK) ? -__builtin_huge_val() : 0.0;
}

// every strip's partials [4 M][KP] empty: (0, 0, -inf, 0)
__global__ __launch_bounds__(256) void pw_part_empty_kernel(double* __restrict__ part, size_t total, size_t MKP) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const size_t r = i % (4 * MKP);
  part[i] = (r >= 2 * MKP && r < 3 * MKP) ? -__builtin_huge_val() : 0.0;
}

// flags[0] = 1 when one of the n * N weights of the call is negative or not finite
__global__ __launch_bounds__(256) void pw_check_weights_kernel(const double* __restrict__ w, int64_t Npad, int64_t N, int n,
                                                               int* __restrict__ flags) {
  const int64_t total = (int64_t)n * N, stride = (int64_t)gridDim.x * 256;
  int badw = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const int64_t k = i / N, p = i - k * N;
    const double v = w[(size_t)k * Npad + p];
    if (!(v >= 0.0) || !mjhmc::pw_finite(v)) badw = 1;
  }
  if (badw) flags[0] = 1;
}

// one thread per expert j < K: the strips of one slot in ascending order from (0, 0, -inf, 0), then onto the totals;
// thread 0 does the same for the sum of weights
__global__ __launch_bounds__(256) void pw_fold_kernel(const double* __restrict__ part, const double* __restrict__ partW, int nstrips,
                                                      int M, unsigned lme, size_t KP, int K, double* __restrict__ tot) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j == 0) {
    double ws = 0.0;
    for (int s = 0; s < nstrips; ++s) ws = ws + partW[s];
    tot[0] = tot[0] + ws;
  }
  if (j >= K) return;
  const size_t MK = (size_t)M * K;
  double* T = tot + kPwTotHead;
  for (int m = 0; m < M; ++m) {
    double s1 = 0.0, s2 = 0.0, mx = -__builtin_huge_val(), se = 0.0;
    for (int s = 0; s < nstrips; ++s) {
      const double* p = part + (size_t)s * (4 * M) * KP + j;
      s1 = s1 + p[(size_t)(0 * M + m) * KP];
      s2 = s2 + p[(size_t)(1 * M + m) * KP];
      if ((lme >> m) & 1u) mjhmc::pw_lme_merge(mx, se, p[(size_t)(2 * M + m) * KP], p[(size_t)(3 * M + m) * KP]);
    }
    const size_t o = (size_t)m * K + j;
    T[o] = T[o] + s1;
    T[MK + o] = T[MK + o] + s2;
    if ((lme >> m) & 1u) mjhmc::pw_lme_merge(T[2 * MK + o], T[3 * MK + o], mx, se);
  }
}

// "a; b ;c" -> {"a", "b", "c"} (surrounding blanks dropped); false for an empty piece
bool split_values(const char* values, std::vector<std::string>* out) {
  const std::string all(values);
  size_t at = 0;
  while (true) {
    const size_t semi = all.find(';', at);
    std::string piece = all.substr(at, semi == std::string::npos ? std::string::npos : semi - at);
    const size_t a = piece.find_first_not_of(" \t\n"), b = piece.find_last_not_of(" \t\n");
    if (a == std::string::npos) return false;
    out->push_back(piece.substr(a, b - a + 1));
    if (semi == std::string::npos) return true;
    at = semi + 1;
  }
}

int checked_values(const char* values, std::vector<std::string>* out) {
  if (!split_values(values, out))
    return mjhmc_fail(MJHMC_ERR_INVALID, "a value expression is empty (the values are ';'-separated, 1 to 4 of them)");
  if (out->size() > (size_t)mjhmc::kPwMaxValues)
    return mjhmc_fail(MJHMC_ERR_INVALID, "the pointwise pass takes 1 to 4 value expressions, got " + std::to_string(out->size()));
  return 0;
}

int checked_mask(const char* what, unsigned mask, int M) {
  if (mask >> M)
    return mjhmc_fail(MJHMC_ERR_INVALID, std::string("the ") + what + " mask " + std::to_string(mask) + " has bits beyond the " +
                                             std::to_string(M) + " values");
  return 0;
}

}  // namespace

struct mjhmc_pointwise : RingAccumulator {
  using RingAccumulator::RingAccumulator;
  int M = 0, K = 0, P = 0, nblk = 0;   // values, experts (columns), the blocks' side and count
  bool grouped = false;                // a grouped model's handle: columns are groups or members, nblk its grouped blocks
  size_t KP = 0;                       // the column pitch of `part`: nblk P, or K for a grouped model
  unsigned lme = 0;
  int ntiles = 0, nstrips = 0;
  hipModule_t module = nullptr;
  hipFunction_t fn = nullptr;
  float* X32 = nullptr;                // [Npad][P]: the float32 rows of a float64 slot
  double* part = nullptr;              // [nstrips][4 M][KP]
  double* partW = nullptr;             // [nstrips]
  double* tot[2] = {nullptr, nullptr}; // the totals and the copy a call works on
  int cur = 0;
  // (`bad` holds two flags: [0] a refused weight, [1] the lowest (m << 20) | j of a value that is not finite)
  size_t tot_elems() const { return kPwTotHead + 4 * (size_t)M * K; }
  ~mjhmc_pointwise() override {
    free_device({X32, part, partW, tot[0], tot[1]});
    if (module) (void)hipModuleUnload(module);
  }
};

namespace {

hipError_t pw_clear_flags(mjhmc_pointwise* h) {
  const int flags[2] = {0, mjhmc::kPwNoBad};
  hipError_t e = hipMemcpyAsync(h->bad, flags, sizeof(flags), hipMemcpyHostToDevice, h->s->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->s->stream);   // (flags is on this stack)
  return e;
}

hipError_t pw_zero_sums(mjhmc_pointwise* h) {
  const size_t MK = (size_t)h->M * h->K;
  const size_t n = std::max<size_t>(4 * MK, kPwTotHead);
  hipLaunchKernelGGL(pw_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->s->stream, h->tot[h->cur], MK);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = pw_clear_flags(h);
  return e;
}

// the handle of M values over `cols` columns in nblk blocks of P around the compiled kernel, its buffers and empty sums
int pw_new_handle(mjhmc_sampler* s, const RtcCode& code, int M, unsigned lme_mask, int P, int nblk, int cols, bool grouped,
                  mjhmc_pointwise** out) {
  const RingSource src = ring_source(s, nullptr);
  mjhmc_pointwise* h = new mjhmc_pointwise("pointwise", "pointwise handle", s, nullptr, src);
  h->M = M;
  h->lme = lme_mask;
  h->P = P;
  h->nblk = nblk;
  h->K = cols;
  h->grouped = grouped;
  h->KP = grouped ? (size_t)cols : (size_t)nblk * P;
  h->ntiles = (int)((s->N + mjhmc::kP - 1) / mjhmc::kP);
  h->nstrips = (h->ntiles + mjhmc::kPwStripTiles - 1) / mjhmc::kPwStripTiles;
  const size_t MKP = (size_t)M * h->KP, part_elems = (size_t)h->nstrips * 4 * MKP;
  hipError_t he = hipModuleLoadData(&h->module, code.code.data());
  if (he == hipSuccess) he = hipModuleGetFunction(&h->fn, h->module, code.lowered[0].c_str());
  if (he == hipSuccess && s->dtype == MJHMC_F64) he = hipMalloc((void**)&h->X32, (size_t)s->Npad * P * sizeof(float));
  if (he == hipSuccess) he = hipMalloc((void**)&h->part, part_elems * sizeof(double));
  if (he == hipSuccess) he = hipMalloc((void**)&h->partW, (size_t)h->nstrips * sizeof(double));
  if (he == hipSuccess) he = hipMalloc((void**)&h->tot[0], h->tot_elems() * sizeof(double));
  if (he == hipSuccess) he = hipMalloc((void**)&h->tot[1], h->tot_elems() * sizeof(double));
  if (he == hipSuccess) he = hipMalloc((void**)&h->bad, 2 * sizeof(int));
  if (he == hipSuccess && grouped) {   // (a per-group value's kernel leaves the columns behind its G untouched)
    hipLaunchKernelGGL(pw_part_empty_kernel, dim3((unsigned)((part_elems + 255) / 256)), dim3(256), 0, s->stream, h->part, part_elems, MKP);
    he = hipGetLastError();
  }
  if (he == hipSuccess) he = pw_zero_sums(h);
  if (he != hipSuccess) {
    delete h;
    (void)hipGetLastError();
    return mjhmc_fail(MJHMC_ERR_HIP, std::string("pointwise buffers: ") + hipGetErrorString(he));
  }
  return acc_created(h, out);
}

}  // namespace

extern "C" {

int mjhmc_pointwise_check(int ndims, int64_t nexperts, const char* values, const char* include_dir) {
  if (!values || !include_dir) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  if (ndims < 1 || nexperts < 1) return mjhmc_fail(MJHMC_ERR_INVALID, "a linear model has ndims >= 1 and nexperts >= 1");
  if (ndims > kPotDim || nexperts > kLinTallMaxExperts)
    return mjhmc_fail(MJHMC_ERR_UNSUPPORTED, "linear models take at most 512 dims and 1048576 (2^20) experts (got " +
                                                 std::to_string(ndims) + " x " + std::to_string(nexperts) + ")");
  std::vector<std::string> v;
  TRY(checked_values(values, &v));
  std::string err;
  const RtcCode* code = nullptr;
  const int rc = linear_pointwise_compile(v, linear_pointwise_dim(ndims, nexperts), include_dir, &err, &code);
  return rc ? mjhmc_fail(rc, err) : 0;
}

int mjhmc_pointwise_create(mjhmc_sampler* s, const char* values, unsigned lme_mask, const char* include_dir, mjhmc_pointwise** out) {
  if (!s || !values || !include_dir || !out) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  const mjhmc_energy* e = s->en;
  if (e->ep.kind != MJHMC_E_LINEAR_EXPR || !e->lin)
    return mjhmc_fail(MJHMC_ERR_UNSUPPORTED, std::string("the pointwise statistics are those of the experts of a linear-model energy "
                                                         "(MJHMC_E_LINEAR_EXPR): the sampler's energy is MJHMC_E_") +
                                                 energy_kind_name(e->ep.kind) + ", which has no experts u = W x + b to report on");
  if (e->lin->grouped())
    return mjhmc_fail(MJHMC_ERR_UNSUPPORTED, "the pointwise statistics of a grouped linear model (mjhmc_energy_create_linear_grouped) "
                                             "are not formed: its experts are stored in a permuted order and the terms of a group "
                                             "are coupled through its log-sum-exp, while this pass reports per expert in the "
                                             "caller's order (its per-row pass is mjhmc_pointwise_create_grouped)");
  if (e->lin_wide())
    return mjhmc_fail(MJHMC_ERR_UNSUPPORTED, "the pointwise statistics of a wide linear model (mjhmc_energy_create_linear_wide) are not formed: "
                                             "the per-expert passes take models of at most 512 dims, stored in one chunk of "
                                             "dims per block of experts");
  if (s->dtype != MJHMC_F64 && s->dtype != MJHMC_F32)
    return mjhmc_fail(MJHMC_ERR_UNSUPPORTED, "linear models run with float32 or float64 state");
  if (!s->ring) return acc_no_ring(nullptr);
  std::vector<std::string> v;
  TRY(checked_values(values, &v));
  const int M = (int)v.size();
  TRY(checked_mask("log-mean-exp", lme_mask, M));
  const int P = e->pot_dim;
  if (s->sh.pitch != P) return mjhmc_fail(MJHMC_ERR_UNSUPPORTED, "the sampler's rows do not have the model's padded pitch");
  HIPCHK(hipSetDevice(s->ctx->device));
  std::string err;
  const RtcCode* code = nullptr;
  const int rc = linear_pointwise_compile(v, P, include_dir, &err, &code);
  if (rc) return mjhmc_fail(rc, err);
  return pw_new_handle(s, *code, M, lme_mask, P, e->lin_tall() ? e->lin->tall_nblk : 1, e->lin->gen.lin.K, false, out);
}

int mjhmc_pointwise_grouped_check(int ndims, int64_t nexperts, int group_size, int64_t n_groups, const char* values,
                                  unsigned member_mask, const char* include_dir) {
  if (!values || !include_dir) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  TRY(linear_grouped_check_args(ndims, nexperts, group_size, n_groups, "", "", ""));
  std::vector<std::string> v;
  TRY(checked_values(values, &v));
  TRY(checked_mask("per-member", member_mask, (int)v.size()));
  std::string err;
  const RtcCode* code = nullptr;
  const int rc = linear_group_pointwise_compile(v, tall_pad(ndims), group_size, member_mask, include_dir, &err, &code);
  return rc ? mjhmc_fail(rc, err) : 0;
}

int mjhmc_pointwise_create_grouped(mjhmc_sampler* s, const char* values, unsigned lme_mask, unsigned member_mask,
                                   const char* include_dir, mjhmc_pointwise** out) {
  if (!s || !values || !include_dir || !out) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  const mjhmc_energy* e = s->en;
  if (e->ep.kind != MJHMC_E_LINEAR_EXPR || !e->lin || !e->lin->grouped())
    return mjhmc_fail(MJHMC_ERR_UNSUPPORTED,
                      std::string("the per-group statistics are those of the groups of a grouped linear model "
                                  "(mjhmc_energy_create_linear_grouped): the sampler's energy is ") +
                          (e->ep.kind == MJHMC_E_LINEAR_EXPR && e->lin
                               ? "a linear model without groups, whose per-expert pass is mjhmc_pointwise_create"
                               : std::string("MJHMC_E_") + energy_kind_name(e->ep.kind) +
                                     ", which has no groups of experts to report on (mjhmc_pointwise_create is the pass of "
                                     "the linear models without groups)"));
  if (s->dtype != MJHMC_F64 && s->dtype != MJHMC_F32)
    return mjhmc_fail(MJHMC_ERR_UNSUPPORTED, "linear models run with float32 or float64 state");
  if (!s->ring) return acc_no_ring(nullptr);
  std::vector<std::string> v;
  TRY(checked_values(values, &v));
  const int M = (int)v.size();
  TRY(checked_mask("log-mean-exp", lme_mask, M));
  TRY(checked_mask("per-member", member_mask, M));
  const int P = e->pot_dim;
  if (s->sh.pitch != P) return mjhmc_fail(MJHMC_ERR_UNSUPPORTED, "the sampler's rows do not have the model's padded pitch");
  HIPCHK(hipSetDevice(s->ctx->device));
  std::string err;
  const RtcCode* code = nullptr;
  const int rc = linear_group_pointwise_compile(v, P, e->lin->grp_C, member_mask, include_dir, &err, &code);
  if (rc) return mjhmc_fail(rc, err);
  const int cols = member_mask ? e->lin->grp_G * e->lin->grp_C : e->lin->grp_G;
  return pw_new_handle(s, *code, M, lme_mask, P, e->lin->grp_nbg, cols, true, out);
}

int mjhmc_pointwise_destroy(mjhmc_pointwise* h) { return acc_destroy(h); }

int mjhmc_pointwise_info(mjhmc_pointwise* h, int* n_values, int64_t* nexperts, int* strip_tiles) {
  if (!h || !n_values || !nexperts || !strip_tiles) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  *n_values = h->M;
  *nexperts = h->K;
  *strip_tiles = mjhmc::kPwStripTiles;
  return 0;
}

int mjhmc_pointwise_reset(mjhmc_pointwise* h) {
  if (!h) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  HIPCHK(hipSetDevice(h->s->ctx->device));
  HIPCHK(pw_zero_sums(h));
  h->n_states = 0;
  return 0;
}

int mjhmc_pointwise_accumulate(mjhmc_pointwise* h, int x_slot0, int w_slot0, int n) {
  if (!h) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  mjhmc_sampler* s = h->s;
  RingSource src;
  TRY(acc_begin(h, x_slot0, w_slot0, n, &src));
  HIPCHK(hipSetDevice(s->ctx->device));
  double* work = h->tot[1 - h->cur];
  HIPCHK(hipMemcpyAsync(work, h->tot[h->cur], h->tot_elems() * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
  if (w_slot0 >= 0)
    hipLaunchKernelGGL(pw_check_weights_kernel, dim3((unsigned)std::min<int64_t>(1024, ((int64_t)n * s->N + 255) / 256)), dim3(256),
                       0, s->stream, acc_weights(h, w_slot0), s->Npad, s->N, n, h->bad);
  const mjhmc_energy* e = s->en;
  // lin_pointwise_kernel or lin_group_pointwise_kernel: the same arguments around the kernel's own model
  const mjhmc::LinTallModel tm{e->pot[0], e->pot[1], e->pot[2], h->nblk, s->D, h->K};
  const mjhmc::LinGroupedModel gm{e->pot[0], e->pot[1], e->pot[2], e->lin->grp_nbg, e->lin->grp_nbp, s->D, e->lin->tall_K, e->lin->grp_G};
  const mjhmc::PotLinear lin = e->lin->gen.lin;
  const size_t KP = h->KP;
  const int64_t nitems = (int64_t)h->nstrips * h->nblk;
  const unsigned grid = (unsigned)std::min<int64_t>(nitems, std::max(1, s->ctx->prop.multiProcessorCount));
  for (int k = 0; k < n; ++k) {
    const char* X = src.base + (size_t)(x_slot0 + k) * src.slot_bytes;
    mjhmc::PwArgs a;
    if (s->dtype == MJHMC_F64) {
      pot_narrow_rows32((const double*)X, h->X32, s->Npad * (int64_t)h->P, s->stream);
      a.X = h->X32;
    } else {
      a.X = (const float*)X;
    }
    a.w = w_slot0 >= 0 ? acc_weights(h, w_slot0 + k) : nullptr;
    a.part = h->part;
    a.partW = h->partW;
    a.flags = h->bad + 1;
    a.N = s->N;
    a.ntiles = h->ntiles;
    a.nstrips = h->nstrips;
    a.lme = h->lme;
    void* params[] = {(void*)&a, h->grouped ? (void*)&gm : (void*)&tm, (void*)&lin};
    HIPCHK(hipModuleLaunchKernel(h->fn, grid, 1, 1, 256, 1, 1, 0, s->stream, params, nullptr));
    hipLaunchKernelGGL(pw_fold_kernel, dim3((unsigned)((h->K + 255) / 256)), dim3(256), 0, s->stream, h->part, h->partW,
                       h->nstrips, h->M, h->lme, KP, h->K, work);
  }
  HIPCHK(hipGetLastError());
  int flags[2] = {0, mjhmc::kPwNoBad};
  HIPCHK(hipMemcpyAsync(flags, h->bad, sizeof(flags), hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  if (flags[0] || flags[1] != mjhmc::kPwNoBad) {
    HIPCHK(pw_clear_flags(h));   // (the totals are untouched: the call worked on their copy)
    if (flags[0])
      return mjhmc_fail(MJHMC_ERR_NONFINITE, "a weight in dwell slots [" + std::to_string(w_slot0) + ", " + std::to_string(w_slot0 + n) +
                                                 ") is negative or not finite: nothing of this block was added");
    return mjhmc_fail(MJHMC_ERR_NONFINITE, "value " + std::to_string(flags[1] >> mjhmc::kPwExpertBits) + " at expert " +
                                               std::to_string(flags[1] & ((1 << mjhmc::kPwExpertBits) - 1)) +
                                               " is not finite for a particle of positive weight in state slots [" +
                                               std::to_string(x_slot0) + ", " + std::to_string(x_slot0 + n) +
                                               "): nothing of this block was added");
  }
  h->cur = 1 - h->cur;
  h->n_states += (int64_t)n * s->N;
  return 0;
}

int mjhmc_pointwise_read(mjhmc_pointwise* h, double* W, double* S1, double* S2, double* lme_max, double* lme_sum, int64_t* n_states) {
  if (!h || !W || !S1 || !S2 || !lme_max || !lme_sum || !n_states) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  mjhmc_sampler* s = h->s;
  HIPCHK(hipSetDevice(s->ctx->device));
  const size_t MK = (size_t)h->M * h->K, bytes = MK * sizeof(double);
  const double* T = h->tot[h->cur];
  HIPCHK(hipMemcpyAsync(W, T, sizeof(double), hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipMemcpyAsync(S1, T + kPwTotHead, bytes, hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipMemcpyAsync(S2, T + kPwTotHead + MK, bytes, hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipMemcpyAsync(lme_max, T + kPwTotHead + 2 * MK, bytes, hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipMemcpyAsync(lme_sum, T + kPwTotHead + 3 * MK, bytes, hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  *n_states = h->n_states;
  return 0;
}

}  // extern "C"
