// Device functionals (include/mjhmc_hip.h: mjhmc_functionals_*): statistics of caller expressions g(x) without the
// samples ever reaching the host.  The caller states
//     S[j] = sum_{d < ndims} stat_j(x_d, d; p)   j < J <= 8        g[k] = value_k(S; p)   k < K, 1 <= K <= 16
// as C expressions (`x` the coordinate widened exactly to float64, `d` its index, `p[m]` float64 parameters); this file
// generates a functor around them, compiles functionals_eval_kernel (functionals.hpp) for it with hipRTC -- through
// rtc_compile, i.e. with the library's own flags, -ffp-contract=off among them -- and owns the DERIVED ring the kernel
// writes: float64 rows [Npad][pitchK], pitchK = pick_shape(K, MJHMC_F64).pitch, the layout of every sample ring.  The
// accumulator handles (estimators.hip, chainstats.hip, histograms.hip) read either ring through RingSource
// (ring_source.hpp), so moments, covariance, R-hat / ESS and histograms of g need no kernel of their own.
//
// A second kind of handle (mjhmc_functionals_create_energy) fills the same derived ring with the ENERGY OBSERVABLES
// [E, grad_sq, virial] of every recorded state: no expressions and no hipRTC -- per slot the sampler's own evaluation
// (state_io.hip: sampler_eval_rows) into scratch of the handle, then energy_observables_kernel (energy_observables.hpp).
//
// A third kind (mjhmc_functionals_create_linear) fills it with LINEAR PROJECTIONS g = link(A x + b) of every recorded state:
// K <= 512 caller-chosen directions through the small-GEMM kernel of projections.hpp -- the library's own instantiation for
// the identity link, a hipRTC build around the caller's link expression otherwise (projections.hip).
#include "functionals.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/mjhmc_hip.h"
#include "energy_observables.hpp"
#include "handles.hpp"
#include "projections.hpp"
#include "ring_source.hpp"
#include "user_expr.hpp"

struct mjhmc_functionals {
  mjhmc_sampler* s = nullptr;
  int J = 0, K = 0, pitchK = 0;
  uint64_t src_gen = 0;         // the sampler's ring at create: the kernel's geometry is that ring's
  hipModule_t module = nullptr;
  hipFunction_t fn = nullptr;
  double* dparams = nullptr;
  int* bad = nullptr;
  double* ring = nullptr;       // [ring_slots][Npad][pitchK]
  int ring_slots = 0;
  uint64_t ring_gen = 0;        // counts the (re-)allocations of the derived ring
  int chunks = 0, cw = 1, log_cw = 0;
  bool wide = false;
  // the energy observables: no module; E and dE/dX of ONE slot, in the layout and types the energy family writes
  bool energy = false;
  void* eo_G = nullptr;         // [Npad][pitch] float64 (float64 state) or float32
  void* eo_E = nullptr;         // [Npad] of the same type
  // the linear projections: device copies of A (transposed, zero-padded) and b; module / fn only with a link expression
  bool linear = false;
  double* lin_At = nullptr;     // [Dpad][Kpad], At[d][k] = A[k][d]
  double* lin_b = nullptr;      // [Kpad]
  int lin_Kpad = 0;
  size_t slot_bytes() const { return (size_t)s->Npad * pitchK * sizeof(double); }
};

namespace {

std::vector<std::string> split_exprs(const char* text) {
  std::vector<std::string> out;
  std::string cur;
  for (const char* c = text ? text : ""; *c; ++c) {
    if (*c == ';') {
      out.push_back(cur);
      cur.clear();
    } else {
      cur.push_back(*c);
    }
  }
  bool blank = true;
  for (char ch : cur) blank = blank && (ch == ' ' || ch == '\t' || ch == '\n');
  if (!blank) out.push_back(cur);
  return out;
}

// the translation unit handed to hipRTC
std::string functionals_source(const std::vector<std::string>& stats, const std::vector<std::string>& values) {
  const int J = (int)stats.size(), K = (int)values.size();
  std::string s;
  s += "#include \"functionals.hpp\"\n";
  s += "namespace mjhmc {\n";
  s += "// S[j] = sum_d stat_j(x_d, d; p), g[k] = value_k(S; p): the caller's expressions\n";
  s += "struct UserFunctionals {\n";
  s += "  static constexpr int J = " + std::to_string(J) + ", K = " + std::to_string(K) + ";\n";
  s += "  const double* p;  // parameters, device memory\n";
  for (int j = 0; j < J; ++j)
    s += "  __device__ __forceinline__ double stat" + std::to_string(j) +
         "(double x, int d) const { (void)x; (void)d; return (double)(" + stats[(size_t)j] + "); }\n";
  s += "  __device__ __forceinline__ void add_stats(double x, int d, double* a) const {\n";
  s += "    (void)x; (void)d; (void)a;\n";
  for (int j = 0; j < J; ++j) s += "    a[" + std::to_string(j) + "] += stat" + std::to_string(j) + "(x, d);\n";
  s += "  }\n";
  for (int k = 0; k < K; ++k)
    s += "  __device__ __forceinline__ double value" + std::to_string(k) + "(const double* S) const { (void)S; return (double)(" +
         values[(size_t)k] + "); }\n";
  s += "  __device__ __forceinline__ void values(const double* S, double* g) const {\n";
  for (int k = 0; k < K; ++k) s += "    g[" + std::to_string(k) + "] = value" + std::to_string(k) + "(S);\n";
  s += "  }\n";
  s += "};\n";
  s += "}  // namespace mjhmc\n";
  return s;
}

// one compile per (source, instantiation) and process: a driver call creates a functionals per run
int functionals_compile(const std::string& src, int dt, bool wide, const std::string& include_dir, const RtcCode** out,
                        std::string* err) {
  const std::string name = "mjhmc::functionals_eval_kernel<" + std::to_string(dt) + ", mjhmc::UserFunctionals, " +
                           (wide ? "true" : "false") + ">";
  return rtc_compile_cached(src, "mjhmc_functionals.hip", {name}, include_dir, "the functional expressions do not compile", out, err);
}

int check_counts(int J, int K) {
  if (J > mjhmc::kFnMaxStats)
    return mjhmc_fail(MJHMC_ERR_INVALID, "functionals take at most " + std::to_string(mjhmc::kFnMaxStats) + " stats (J = " +
                                             std::to_string(J) + ")");
  if (K < 1 || K > mjhmc::kFnMaxValues)
    return mjhmc_fail(MJHMC_ERR_INVALID, "the number of values K must be in [1, " + std::to_string(mjhmc::kFnMaxValues) +
                                             "], got " + std::to_string(K));
  return 0;
}

// lane map of a ring row of `pitch` elements of `vec` per 16 bytes (functionals.hpp)
void row_geometry(int pitch, int vec, int* chunks, int* cw, int* log_cw, bool* wide) {
  *chunks = pitch / vec;
  *wide = *chunks > 64;
  int c = 1, l = 0;
  while (c < *chunks && c < 64) {
    c <<= 1;
    ++l;
  }
  *cw = c;
  *log_cw = l;
}

void functionals_free(mjhmc_functionals* f) {
  mjhmc_sampler* s = f->s;
  accumulators_free_owned(s, f);
  for (void* p : {(void*)f->dparams, (void*)f->bad, (void*)f->ring, f->eo_G, f->eo_E, (void*)f->lin_At, (void*)f->lin_b})
    if (p) (void)hipFree(p);
  if (f->module) (void)hipModuleUnload(f->module);
  delete f;
}

// the three values of slots [x_slot0, x_slot0 + n): per slot the evaluation launches of the energy family (one for the
// elementwise, expression, ProductOfT float32-state and SparseImageCode kernels; narrow + force + widen passes on the
// float64-state ProductOfT path) and ONE launch of energy_observables_kernel, all on the sampler's stream; the scratch is
// reused slot after slot in stream order.  One flag read-back (one synchronisation) for the block.
const char* const kEnergyObsNames[3] = {"E", "grad_sq", "virial"};

// one slot: the evaluation into the scratch (eval), the reduction of slot and scratch into the derived slot (reduce)
int energy_slot(mjhmc_functionals* f, int x_slot, int out_slot, bool eval, bool reduce) {
  mjhmc_sampler* s = f->s;
  const char* X = (const char*)s->ring + (size_t)x_slot * mat_bytes(s);
  if (eval) TRY(sampler_eval_rows(s, X, f->eo_G, f->eo_E));
  if (!reduce) return 0;
  mjhmc::EnergyObsArgs a;
  a.X = X;
  a.G = f->eo_G;
  a.E = f->eo_E;
  a.dst = f->ring + (size_t)out_slot * s->Npad * f->pitchK;
  a.N = s->N;
  a.D = s->D;
  a.pitch = s->sh.pitch;
  a.chunks = f->chunks;
  a.cw = f->cw;
  a.log_cw = f->log_cw;
  a.bad = f->bad;
  if (!mjhmc::energy_observables_launch(a, s->dtype, s->dtype != MJHMC_F64, f->wide, s->stream))
    return mjhmc_fail(MJHMC_ERR_UNSUPPORTED, "no energy-observables kernel for this state type");
  HIPCHK(hipGetLastError());
  return 0;
}

int energy_evaluate(mjhmc_functionals* f, int x_slot0, int n, int out_slot0) {
  mjhmc_sampler* s = f->s;
  const int64_t rows_per_block = f->wide ? 4 : (int64_t)mjhmc::kFnInFlight * (256 >> f->log_cw);
  if ((s->N + rows_per_block - 1) / rows_per_block > 0x7FFFFFFFll)
    return mjhmc_fail(MJHMC_ERR_UNSUPPORTED, "too many particles for one launch of the energy-observables pass");
  for (int t = 0; t < n; ++t) TRY(energy_slot(f, x_slot0 + t, out_slot0 + t, true, true));
  int bad = 0;
  HIPCHK(hipMemcpyAsync(&bad, f->bad, sizeof(int), hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  if (bad) {
    HIPCHK(hipMemsetAsync(f->bad, 0, sizeof(int), s->stream));
    int k = 0;
    while (!((bad >> k) & 1)) ++k;
    return mjhmc_fail(MJHMC_ERR_NONFINITE, "value " + std::to_string(k) + " (" + kEnergyObsNames[k] +
                                               ") of the energy observables is not finite for a state in slots [" +
                                               std::to_string(x_slot0) + ", " + std::to_string(x_slot0 + n) +
                                               "): do not accumulate derived slots [" + std::to_string(out_slot0) + ", " +
                                               std::to_string(out_slot0 + n) + ")");
  }
  return 0;
}

// the projections of slots [x_slot0, x_slot0 + n): ONE launch of projections_kernel on the sampler's stream (blockIdx.y
// strides over the slots) and one flag read-back
int linear_evaluate(mjhmc_functionals* f, int x_slot0, int n, int out_slot0) {
  mjhmc_sampler* s = f->s;
  mjhmc::ProjArgs a;
  a.src = (const char*)s->ring + (size_t)x_slot0 * mat_bytes(s);
  a.dst = f->ring + (size_t)out_slot0 * s->Npad * f->pitchK;
  a.At = f->lin_At;
  a.b = f->lin_b;
  a.Npad = s->Npad;
  a.N = s->N;
  a.n = n;
  a.D = s->D;
  a.chunks = f->chunks;
  a.K = f->K;
  a.pitchK = f->pitchK;
  a.Kpad = f->lin_Kpad;
  a.bad = f->bad;
  const int64_t gx = (s->N + mjhmc::kProjRows - 1) / mjhmc::kProjRows;
  if (gx > 0x7FFFFFFFll) return mjhmc_fail(MJHMC_ERR_UNSUPPORTED, "too many particles for one launch of the projections pass");
  if (f->fn) {
    struct {
      const double* p;
    } link{f->dparams};
    void* params[] = {&a, &link};
    HIPCHK(hipModuleLaunchKernel(f->fn, (unsigned)gx, (unsigned)std::min(n, 1024), 1, 256, 1, 1, 0, s->stream, params, nullptr));
  } else {
    if (!mjhmc::projections_launch(a, s->dtype, s->stream))
      return mjhmc_fail(MJHMC_ERR_UNSUPPORTED, "no projections kernel for this state type");
    HIPCHK(hipGetLastError());
  }
  int bad = mjhmc::kProjNoBad;
  HIPCHK(hipMemcpyAsync(&bad, f->bad, sizeof(int), hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  if (bad != mjhmc::kProjNoBad) {
    const int no_bad = mjhmc::kProjNoBad;
    HIPCHK(hipMemcpyAsync(f->bad, &no_bad, sizeof(int), hipMemcpyHostToDevice, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return mjhmc_fail(MJHMC_ERR_NONFINITE, "value " + std::to_string(bad) + " of the projections is not finite for a state in slots [" +
                                               std::to_string(x_slot0) + ", " + std::to_string(x_slot0 + n) +
                                               "): do not accumulate derived slots [" + std::to_string(out_slot0) + ", " +
                                               std::to_string(out_slot0 + n) + ")");
  }
  return 0;
}

// the first entry of v[0 .. n) that is not finite, or -1
int64_t first_nonfinite(const double* v, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) return (int64_t)i;
  return -1;
}

}  // namespace

RingSource functionals_ring_source(const mjhmc_functionals* f) {
  RingSource r;
  r.base = (const char*)f->ring;
  r.slot_bytes = f->slot_bytes();
  r.slots = f->ring_slots;
  r.dtype = MJHMC_F64;
  r.D = f->K;
  r.pitch = f->pitchK;
  r.esize = 8;
  r.gen = f->ring_gen;
  r.owner = f;
  return r;
}

mjhmc_sampler* functionals_sampler(const mjhmc_functionals* f) { return f->s; }

void functionals_free_all(mjhmc_sampler* s) {
  // (each takes its handles out of the sampler's list)
  for (mjhmc_functionals* f : s->functionals) functionals_free(f);
  s->functionals.clear();
}

extern "C" {

int mjhmc_functionals_check(int ndims, const char* stats, const char* values, const char* include_dir) {
  if (!values || !include_dir) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  if (ndims < 1) return mjhmc_fail(MJHMC_ERR_INVALID, "ndims must be >= 1");
  const std::vector<std::string> st = split_exprs(stats), va = split_exprs(values);
  TRY(check_counts((int)st.size(), (int)va.size()));
  Shape sh;
  TRY(pick_shape(ndims, MJHMC_F64, &sh));
  int chunks, cw, log_cw;
  bool wide;
  row_geometry(sh.pitch, 2, &chunks, &cw, &log_cw, &wide);
  const RtcCode* c = nullptr;
  std::string err;
  const int rc = functionals_compile(functionals_source(st, va), MJHMC_F64, wide, include_dir, &c, &err);
  return rc ? mjhmc_fail(rc, err) : 0;
}

int mjhmc_functionals_create(mjhmc_sampler* s, const char* stats, const char* values, const double* params, size_t nparams,
                             const char* include_dir, mjhmc_functionals** out) {
  if (!s || !values || !include_dir || !out) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  if (nparams && !params) return mjhmc_fail(MJHMC_ERR_INVALID, "params is NULL");
  const std::vector<std::string> st = split_exprs(stats), va = split_exprs(values);
  TRY(check_counts((int)st.size(), (int)va.size()));
  if (!s->ring) return mjhmc_fail(MJHMC_ERR_INVALID, "the sampler has no sample ring yet (call mjhmc_ring_alloc first)");
  // the kernel addresses a row in 16-byte chunks of the state's own type: rows must be whole chunks of it
  const int vec = s->dtype == MJHMC_F64 ? 2 : (s->dtype == MJHMC_F32 ? 4 : 8);
  if (s->sh.esize * vec != 16 || s->sh.pitch % vec != 0)
    return mjhmc_fail(MJHMC_ERR_UNSUPPORTED, "the sampler's rows are not whole 16-byte chunks of its state type");
  Shape shK;
  TRY(pick_shape((int)va.size(), MJHMC_F64, &shK));
  if (shK.pitch != ((int)va.size() + 1) / 2 * 2) return mjhmc_fail(MJHMC_ERR_UNSUPPORTED, "unexpected row pitch of the derived ring");
  HIPCHK(hipSetDevice(s->ctx->device));
  int chunks, cw, log_cw;
  bool wide;
  row_geometry(s->sh.pitch, vec, &chunks, &cw, &log_cw, &wide);
  const RtcCode* c = nullptr;
  std::string err;
  const int rc = functionals_compile(functionals_source(st, va), s->dtype, wide, include_dir, &c, &err);
  if (rc) return mjhmc_fail(rc, err);
  mjhmc_functionals* f = new mjhmc_functionals();
  f->s = s;
  f->J = (int)st.size();
  f->K = (int)va.size();
  f->pitchK = shK.pitch;
  f->src_gen = s->ring_gen;
  f->chunks = chunks;
  f->cw = cw;
  f->log_cw = log_cw;
  f->wide = wide;
  hipError_t e = hipModuleLoadData(&f->module, c->code.data());
  if (e == hipSuccess) e = hipModuleGetFunction(&f->fn, f->module, c->lowered[0].c_str());
  if (e == hipSuccess) e = hipMalloc((void**)&f->dparams, (nparams ? nparams : 1) * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&f->bad, sizeof(int));
  if (e == hipSuccess && nparams)
    e = hipMemcpyAsync(f->dparams, params, nparams * sizeof(double), hipMemcpyHostToDevice, s->stream);
  if (e == hipSuccess) e = hipMemsetAsync(f->bad, 0, sizeof(int), s->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(s->stream);   // (params is the caller's for the duration of the call only)
  if (e != hipSuccess) {
    functionals_free(f);
    (void)hipGetLastError();
    return mjhmc_fail(MJHMC_ERR_HIP, std::string("functionals: ") + hipGetErrorString(e));
  }
  s->functionals.push_back(f);
  *out = f;
  return 0;
}

int mjhmc_functionals_create_energy(mjhmc_sampler* s, mjhmc_functionals** out) {
  if (!s || !out) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  if (s->en->is_host())
    return mjhmc_fail(MJHMC_ERR_UNSUPPORTED,
                      "a host-evaluated energy has no device evaluation: the caller's callables are the only evaluation of E "
                      "and dE/dX, so the energy observables of its states are the caller's to form");
  if (!s->ring) return mjhmc_fail(MJHMC_ERR_INVALID, "the sampler has no sample ring yet (call mjhmc_ring_alloc first)");
  const int vec = s->dtype == MJHMC_F64 ? 2 : (s->dtype == MJHMC_F32 ? 4 : 8);
  if (s->sh.esize * vec != 16 || s->sh.pitch % vec != 0)
    return mjhmc_fail(MJHMC_ERR_UNSUPPORTED, "the sampler's rows are not whole 16-byte chunks of its state type");
  Shape shK;
  TRY(pick_shape(mjhmc::kEnergyObsValues, MJHMC_F64, &shK));
  if (shK.pitch != mjhmc::kEnergyObsPitch) return mjhmc_fail(MJHMC_ERR_UNSUPPORTED, "unexpected row pitch of the derived ring");
  HIPCHK(hipSetDevice(s->ctx->device));
  mjhmc_functionals* f = new mjhmc_functionals();
  f->s = s;
  f->energy = true;
  f->K = mjhmc::kEnergyObsValues;
  f->pitchK = shK.pitch;
  f->src_gen = s->ring_gen;
  row_geometry(s->sh.pitch, vec, &f->chunks, &f->cw, &f->log_cw, &f->wide);
  // dE/dX has the state's row pitch in every family (SparseImageCode: [Npad][ndims] float32, pitch == ndims) and is
  // float64 exactly where the state is; E is a scalar of the same type per row.  Rows p >= N: zero, and never read.
  const size_t gsize = s->dtype == MJHMC_F64 ? 8 : 4;
  const size_t gbytes = (size_t)s->Npad * s->sh.pitch * gsize, ebytes = (size_t)s->Npad * gsize;
  hipError_t e = hipMalloc(&f->eo_G, gbytes);
  if (e == hipSuccess) e = hipMalloc(&f->eo_E, ebytes);
  if (e == hipSuccess) e = hipMalloc((void**)&f->bad, sizeof(int));
  if (e == hipSuccess) e = hipMemsetAsync(f->eo_G, 0, gbytes, s->stream);
  if (e == hipSuccess) e = hipMemsetAsync(f->eo_E, 0, ebytes, s->stream);
  if (e == hipSuccess) e = hipMemsetAsync(f->bad, 0, sizeof(int), s->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
  if (e != hipSuccess) {
    functionals_free(f);
    (void)hipGetLastError();
    return mjhmc_fail(MJHMC_ERR_HIP, std::string("energy observables: ") + hipGetErrorString(e));
  }
  s->functionals.push_back(f);
  *out = f;
  return 0;
}

int mjhmc_functionals_create_linear(mjhmc_sampler* s, int n_values, const double* A, const double* b, const char* link_expr,
                                    const double* params, size_t nparams, const char* include_dir, mjhmc_functionals** out) {
  if (!s || !A || !out) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  if (link_expr && !include_dir) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  if (nparams && !params) return mjhmc_fail(MJHMC_ERR_INVALID, "params is NULL");
  const int K = n_values;
  if (K < 1 || K > mjhmc::kProjMaxValues)
    return mjhmc_fail(MJHMC_ERR_INVALID, "the number of values K must be in [1, " + std::to_string(mjhmc::kProjMaxValues) +
                                             "], got " + std::to_string(K));
  if (!s->ring) return mjhmc_fail(MJHMC_ERR_INVALID, "the sampler has no sample ring yet (call mjhmc_ring_alloc first)");
  const int D = s->D;
  int64_t at = first_nonfinite(A, (size_t)K * D);
  if (at >= 0)
    return mjhmc_fail(MJHMC_ERR_INVALID, "A[" + std::to_string(at / D) + "][" + std::to_string(at % D) + "] is not finite");
  if (b && (at = first_nonfinite(b, (size_t)K)) >= 0) return mjhmc_fail(MJHMC_ERR_INVALID, "b[" + std::to_string(at) + "] is not finite");
  if ((at = first_nonfinite(params, nparams)) >= 0) return mjhmc_fail(MJHMC_ERR_INVALID, "p[" + std::to_string(at) + "] is not finite");
  const int vec = s->dtype == MJHMC_F64 ? 2 : (s->dtype == MJHMC_F32 ? 4 : 8);
  if (s->sh.esize * vec != 16 || s->sh.pitch % vec != 0)
    return mjhmc_fail(MJHMC_ERR_UNSUPPORTED, "the sampler's rows are not whole 16-byte chunks of its state type");
  Shape shK;
  TRY(pick_shape(K, MJHMC_F64, &shK));
  if (shK.pitch != (K + 1) / 2 * 2) return mjhmc_fail(MJHMC_ERR_UNSUPPORTED, "unexpected row pitch of the derived ring");
  HIPCHK(hipSetDevice(s->ctx->device));
  const RtcCode* link = nullptr;   // (none: the identity, in the library)
  if (link_expr) {
    std::string err;
    const int rc = mjhmc::projections_link_compile(link_expr, s->dtype, K, include_dir, &link, &err);
    if (rc) return mjhmc_fail(rc, err);
  }
  // A transposed and zero-padded to whole tiles and d chunks (projections.hpp: ProjArgs), b padded with zeros
  const int Kpad = (K + 63) / 64 * 64, Dpad = (D + 63) / 64 * 64;
  std::vector<double> At((size_t)Dpad * Kpad, 0.0), bp((size_t)Kpad, 0.0);
  for (int k = 0; k < K; ++k) {
    for (int d = 0; d < D; ++d) At[(size_t)d * Kpad + k] = A[(size_t)k * D + d];
    if (b) bp[(size_t)k] = b[k];
  }
  mjhmc_functionals* f = new mjhmc_functionals();
  f->s = s;
  f->linear = true;
  f->K = K;
  f->pitchK = shK.pitch;
  f->lin_Kpad = Kpad;
  f->src_gen = s->ring_gen;
  row_geometry(s->sh.pitch, vec, &f->chunks, &f->cw, &f->log_cw, &f->wide);
  const int no_bad = mjhmc::kProjNoBad;
  hipError_t e = hipSuccess;
  if (link) {
    e = hipModuleLoadData(&f->module, link->code.data());
    if (e == hipSuccess) e = hipModuleGetFunction(&f->fn, f->module, link->lowered[0].c_str());
  }
  if (e == hipSuccess) e = hipMalloc((void**)&f->lin_At, At.size() * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&f->lin_b, bp.size() * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&f->dparams, (nparams ? nparams : 1) * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&f->bad, sizeof(int));
  if (e == hipSuccess) e = hipMemcpyAsync(f->lin_At, At.data(), At.size() * sizeof(double), hipMemcpyHostToDevice, s->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(f->lin_b, bp.data(), bp.size() * sizeof(double), hipMemcpyHostToDevice, s->stream);
  if (e == hipSuccess && nparams)
    e = hipMemcpyAsync(f->dparams, params, nparams * sizeof(double), hipMemcpyHostToDevice, s->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(f->bad, &no_bad, sizeof(int), hipMemcpyHostToDevice, s->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(s->stream);   // (the host copies live for the duration of the call only)
  if (e != hipSuccess) {
    functionals_free(f);
    (void)hipGetLastError();
    return mjhmc_fail(MJHMC_ERR_HIP, std::string("projections: ") + hipGetErrorString(e));
  }
  s->functionals.push_back(f);
  *out = f;
  return 0;
}

int mjhmc_functionals_destroy(mjhmc_functionals* f) {
  if (!f) return 0;
  mjhmc_sampler* s = f->s;
  (void)hipSetDevice(s->ctx->device);
  if (s->stream) (void)hipStreamSynchronize(s->stream);
  s->functionals.erase(std::remove(s->functionals.begin(), s->functionals.end(), f), s->functionals.end());
  functionals_free(f);
  return 0;
}

int mjhmc_functionals_info(mjhmc_functionals* f, int* n_values, uint64_t* slot_bytes) {
  if (!f || !n_values || !slot_bytes) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  *n_values = f->K;
  *slot_bytes = (uint64_t)f->slot_bytes();
  return 0;
}

int mjhmc_functionals_ring_alloc(mjhmc_functionals* f, int n_slots) {
  if (!f) return mjhmc_fail(MJHMC_ERR_INVALID, "functionals is NULL");
  if (n_slots < 1) return mjhmc_fail(MJHMC_ERR_INVALID, "n_slots must be >= 1");
  mjhmc_sampler* s = f->s;
  HIPCHK(hipSetDevice(s->ctx->device));
  if (n_slots <= f->ring_slots) return 0;
  HIPCHK(hipStreamSynchronize(s->stream));
  const size_t bytes = (size_t)n_slots * f->slot_bytes();
  // the NEW ring first: a request the device cannot hold leaves the ring there was
  double* ring = nullptr;
  const hipError_t e = hipMalloc((void**)&ring, bytes);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    char msg[256];
    std::snprintf(msg, sizeof(msg), "a derived ring of %d slots x %.3f GB does not fit the device (%s): the ring there was is kept",
                  n_slots, f->slot_bytes() / 1e9, hipGetErrorString(e));
    return mjhmc_fail(MJHMC_ERR_HIP, msg);
  }
  // rows p >= N stay zero for the life of the ring: the kernel never writes them
  HIPCHK(hipMemsetAsync(ring, 0, bytes, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  if (f->ring) HIPCHK(hipFree(f->ring));
  f->ring = ring;
  f->ring_slots = n_slots;
  ++f->ring_gen;
  return 0;
}

int mjhmc_functionals_evaluate(mjhmc_functionals* f, int x_slot0, int n, int out_slot0) {
  if (!f) return mjhmc_fail(MJHMC_ERR_INVALID, "functionals is NULL");
  mjhmc_sampler* s = f->s;
  if (f->src_gen != s->ring_gen)
    return mjhmc_fail(MJHMC_ERR_INVALID, "the sample ring was re-allocated after mjhmc_functionals_create: create a new one");
  if (!f->ring) return mjhmc_fail(MJHMC_ERR_INVALID, "the functionals have no derived ring yet (call mjhmc_functionals_ring_alloc first)");
  if (n < 1) return mjhmc_fail(MJHMC_ERR_INVALID, "n must be >= 1");
  if (x_slot0 < 0 || (int64_t)x_slot0 + n > s->ring_slots)
    return mjhmc_fail(MJHMC_ERR_INVALID, "state slots [" + std::to_string(x_slot0) + ", " + std::to_string((int64_t)x_slot0 + n) +
                                             ") are outside the ring of " + std::to_string(s->ring_slots));
  if (out_slot0 < 0 || (int64_t)out_slot0 + n > f->ring_slots)
    return mjhmc_fail(MJHMC_ERR_INVALID, "derived slots [" + std::to_string(out_slot0) + ", " + std::to_string((int64_t)out_slot0 + n) +
                                             ") are outside the derived ring of " + std::to_string(f->ring_slots));
  HIPCHK(hipSetDevice(s->ctx->device));
  if (f->energy) return energy_evaluate(f, x_slot0, n, out_slot0);
  if (f->linear) return linear_evaluate(f, x_slot0, n, out_slot0);
  mjhmc::FunctionalsArgs a;
  a.src = (const char*)s->ring + (size_t)x_slot0 * mat_bytes(s);
  a.dst = f->ring + (size_t)out_slot0 * s->Npad * f->pitchK;
  a.Npad = s->Npad;
  a.N = s->N;
  a.n = n;
  a.D = s->D;
  a.pitch = s->sh.pitch;
  a.chunks = f->chunks;
  a.cw = f->cw;
  a.log_cw = f->log_cw;
  a.bad = f->bad;
  struct {
    const double* p;
  } fn{f->dparams};
  void* params[] = {&a, &fn};
  const int64_t rows_per_block = f->wide ? 4 : (int64_t)mjhmc::kFnInFlight * (256 >> f->log_cw);
  const int64_t gx = (s->N + rows_per_block - 1) / rows_per_block;
  if (gx > 0x7FFFFFFFll) return mjhmc_fail(MJHMC_ERR_UNSUPPORTED, "too many particles for one launch of the functionals pass");
  HIPCHK(hipModuleLaunchKernel(f->fn, (unsigned)gx, (unsigned)std::min(n, 1024), 1, 256, 1, 1, 0, s->stream, params, nullptr));
  int bad = 0;
  HIPCHK(hipMemcpyAsync(&bad, f->bad, sizeof(int), hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  if (bad) {
    HIPCHK(hipMemsetAsync(f->bad, 0, sizeof(int), s->stream));
    int k = 0;
    while (!((bad >> k) & 1)) ++k;
    return mjhmc_fail(MJHMC_ERR_NONFINITE, "value " + std::to_string(k) + " of the functionals is not finite for a state in slots [" +
                                               std::to_string(x_slot0) + ", " + std::to_string(x_slot0 + n) +
                                               "): do not accumulate derived slots [" + std::to_string(out_slot0) + ", " +
                                               std::to_string(out_slot0 + n) + ")");
  }
  return 0;
}

int mjhmc_functionals_read(mjhmc_functionals* f, int slot0, int n, double* host_out) {
  if (!f || !host_out) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  if (slot0 < 0 || n < 1 || (int64_t)slot0 + n > f->ring_slots) return mjhmc_fail(MJHMC_ERR_INVALID, "slots out of range");
  mjhmc_sampler* s = f->s;
  HIPCHK(hipSetDevice(s->ctx->device));
  // (a test and inspection path: the rows come over as they are and are re-tiled here)
  std::vector<double> rows((size_t)s->Npad * f->pitchK);
  for (int t = 0; t < n; ++t) {
    TRY(copy_to_host(s, f->ring + (size_t)(slot0 + t) * s->Npad * f->pitchK, rows.data(), rows.size() * sizeof(double)));
    for (int k = 0; k < f->K; ++k)
      for (int64_t p = 0; p < s->N; ++p) host_out[((size_t)k * n + t) * s->N + p] = rows[(size_t)p * f->pitchK + k];
  }
  return 0;
}

#ifdef MJHMC_TEST_HOOKS
// test build only (tools/energy_observables_bench.py): ONE half of the energy observables' work on slots [x_slot0, x_slot0
// + n), so that the two can be timed apart -- part 0 the evaluation launches into the scratch, part 1 the reduction kernel
// on the slot and whatever the scratch holds; no flag read-back, synchronised at the end
int mjhmc_test_energy_observables_part(mjhmc_functionals* f, int x_slot0, int n, int out_slot0, int part) {
  if (!f || !f->energy || !f->ring || n < 1 || x_slot0 < 0 || out_slot0 < 0 || (part != 0 && part != 1))
    return mjhmc_fail(MJHMC_ERR_INVALID, "bad argument");
  mjhmc_sampler* s = f->s;
  if (f->src_gen != s->ring_gen || (int64_t)x_slot0 + n > s->ring_slots || (int64_t)out_slot0 + n > f->ring_slots)
    return mjhmc_fail(MJHMC_ERR_INVALID, "bad argument");
  HIPCHK(hipSetDevice(s->ctx->device));
  for (int t = 0; t < n; ++t) TRY(energy_slot(f, x_slot0 + t, out_slot0 + t, part == 0, part == 1));
  HIPCHK(hipMemsetAsync(f->bad, 0, sizeof(int), s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  return 0;
}
#endif

}  // extern "C"
