// C ABI of libmjhmc_hip.so (include/mjhmc_hip.h): error plumbing, the ctx / energy / sampler handles, hyper-parameters,
// checkpoint / restore / rollback, the RNG tick, and the ctx-level utilities.  The launch schedules are iterate.hip's,
// state transfer and evaluation state_io.hip's, the sample ring ring.hip's.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <functional>
#include <vector>

#include "autocor.hpp"
#include "lagcov.hpp"
#include "sampler_internal.hpp"

// ---------------------------------------------------------------------------------------------
// error plumbing
// ---------------------------------------------------------------------------------------------
static thread_local std::string g_err;

int mjhmc_fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
const std::string& last_error_text() { return g_err; }

// lanes-per-particle / elements-per-lane selection (see lane_group.hpp header comment)

int pick_shape(int D, int dtype, Shape* out) {
  const int esize = dtype == MJHMC_F64 ? 8 : 4;
  const int VEC = 16 / esize;
  Shape s;
  s.esize = esize;
  s.pitch = (D + VEC - 1) / VEC * VEC;
  s.CH = s.pitch / VEC;
  int C, G;
  if (s.CH <= 1) {
    C = 1;
    G = 1;
  } else {
    C = 4;
    if (const char* force = test_env("MJHMC_CHUNKS_PER_LANE")) {  // perf experiments
      const int f = std::atoi(force);
      C = f == 8 ? 8 : (f == 1 ? 1 : 4);
    }
    G = pow2ceil((s.CH + C - 1) / C);
    if (G > 64) {
      C = 8;
      G = pow2ceil((s.CH + 7) / 8);
    }
    if (G > 64) {
      // more dims than 64 lanes x 16 elements hold: float64 samplers of the built-in elementwise energies take the
      // multi-pass path (multipass.hip: state in HBM between the substeps); others have no such form
      // (float32 state: the same path on float64 storage, the state rounded to float32 wherever it is written)
      s.esize = 8;
      s.pitch = (D + 1) / 2 * 2;
      s.CH = s.pitch / 2;
      s.E = 0;
      s.logG = 0;
      s.wide = true;
      s.round32 = dtype != MJHMC_F64;
      *out = s;
      return 0;
    }
  }
  s.E = C * VEC;
  s.logG = ilog2(G);
  *out = s;
  return 0;
}

int check_state_dtype(const mjhmc_energy* e, int dtype) {
  if (dtype != MJHMC_F64 && dtype != MJHMC_F32 && dtype != MJHMC_BF16)
    return fail(MJHMC_ERR_INVALID, "dtype must be F64, F32 or BF16");
  if (dtype == MJHMC_BF16 && !e->is_sic()) return fail(MJHMC_ERR_UNSUPPORTED, "BF16 state: SPARSE_CODE only");
  if (e->is_sic() && dtype == MJHMC_F64)
    return fail(MJHMC_ERR_UNSUPPORTED, "SPARSE_CODE runs with BF16 state (the benchmark's) or F32 state (the reference's)");
  if (e->is_user() && dtype != MJHMC_F64) return fail(MJHMC_ERR_UNSUPPORTED, "user-expression energies run in float64");
  if (e->is_host() && dtype != MJHMC_F64) return fail(MJHMC_ERR_UNSUPPORTED, "host-evaluated energies run in float64");
  return 0;
}

int shape_for(const mjhmc_energy* e, int* dtype, Shape* sh) {
  if (e->is_pot()) {
    if (*dtype != MJHMC_F64 && *dtype != MJHMC_F32) return fail(MJHMC_ERR_UNSUPPORTED, "PRODUCT_OF_T and LINEAR_EXPR run with float32 or float64 state");
    if (*dtype == MJHMC_F64 || e->pot_big() || e->lin_tall() || e->lin_wide()) {
      // the reference's own arithmetic: float64 HMCState arrays around the float32 force (distributions.py:408-415,
      // hmc_state.py:29-38); ndims > 512, tall and wide linear models: their force evaluation exists on the multi-pass path only
      *sh = Shape{0, 0, e->pot_dim, e->pot_dim / 2, 8, true};
      sh->round32 = *dtype != MJHMC_F64;
    } else {
      *sh = Shape{0, 0, e->pot_dim, e->pot_dim / 4, 4};
    }
  } else if (e->is_sic()) {
    if (*dtype != MJHMC_BF16 && *dtype != MJHMC_F32)
      return fail(MJHMC_ERR_UNSUPPORTED, "SPARSE_CODE runs with BF16 state (the benchmark's) or F32 state (the reference's)");
    // a particle row = n_patches x n_coeffs elements of the state's type (the matrix-core operands are bf16 either way)
    *sh = *dtype == MJHMC_BF16 ? Shape{0, 0, e->ep.ndims, e->ep.ndims / 8, 2} : Shape{0, 0, e->ep.ndims, e->ep.ndims / 4, 4};
  } else {
    TRY(pick_shape(e->ep.ndims, *dtype, sh));
  }
  if (sh->round32) *dtype = MJHMC_F64;
  return 0;
}

// (sampler_internal.hpp says when)
int drop_spec(mjhmc_sampler* s) {
  if (!s->Hspec[0]) return 0;
  HIPCHK(hipSetDevice(s->ctx->device));
  HIPCHK(hipMemsetAsync(s->Hspec[s->scur], 0xFF, (size_t)s->Npad * ssize(s), s->stream));
  return 0;
}

int live_state(const mjhmc_sampler* s, bool with_dEdX, void* ptrs[7], size_t sizes[7]) {
  const size_t mb = mat_bytes(s), vb = (size_t)s->Npad * ssize(s), db = (size_t)s->Npad * sizeof(double);
  void* const p[7] = {s->Xcur, s->Vbuf[s->vcur], s->EX[s->scur], s->EV[s->scur], s->Hflf[s->scur], s->dwell, s->Gbuf[s->vcur]};
  const size_t b[7] = {mb, mb, vb, vb, vb, db, mb};
  std::copy(p, p + 7, ptrs);
  std::copy(b, b + 7, sizes);
  return with_dEdX ? 7 : 6;
}

// mjhmc_draw_from / mjhmc_min_idx: the jump process's helpers on caller arrays (mjhmc/misc/utils.py:15-50)
__global__ void draw_from_kernel(const double* __restrict__ rates, const double* __restrict__ e, int64_t n,
                                 double* __restrict__ out, long long* first_bad) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  bool bad = false;
  out[i] = wait_time(rates[i], e[i], bad);
  if (bad) atomicMin(first_bad, (long long)i);
}
__global__ void min_idx_kernel(const double* __restrict__ draws, int k, int64_t n, int32_t* __restrict__ which) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  int w = 0;
  double best = draws[j];
  for (int r = 1; r < k; ++r) {   // np.argmin: the first minimum; the first NaN wins outright
    const double d = draws[(size_t)r * n + j];
    if (!(best != best) && (d < best || d != d)) {
      w = r;
      best = d;
    }
  }
  which[j] = w;
}

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
// the end of a create that failed after the handle existed: the failure's message survives the destroy
static int destroy_keeping_error(mjhmc_energy* e, int rc) {
  const std::string keep = g_err;
  mjhmc_energy_destroy(e);
  g_err = keep;
  return rc;
}

extern "C" {

const char* mjhmc_last_error(void) { return g_err.c_str(); }
int mjhmc_abi_version(void) { return MJHMC_ABI_VERSION; }

int mjhmc_ctx_create(int device, mjhmc_ctx** out) {
  if (!out) return fail(MJHMC_ERR_INVALID, "out is NULL");
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return fail(MJHMC_ERR_NO_DEVICE, "no HIP device visible");
  if (device < 0 || device >= n) return fail(MJHMC_ERR_INVALID, "device index out of range");
  HIPCHK(hipSetDevice(device));
  mjhmc_ctx* c = new mjhmc_ctx();
  c->device = device;
  HIPCHK(hipGetDeviceProperties(&c->prop, device));
  *out = c;
  return 0;
}

int mjhmc_ctx_destroy(mjhmc_ctx* ctx) {
  delete ctx;
  return 0;
}

int mjhmc_ctx_info(mjhmc_ctx* ctx, char* name, size_t name_cap, int* n_cu, uint64_t* hbm_bytes) {
  if (!ctx) return fail(MJHMC_ERR_INVALID, "ctx is NULL");
  if (name && name_cap) {
    // ... and its PCI address, e.g. "[0000:75:00.0]": how a caller finds the device's sysfs / SMI entry
    std::snprintf(name, name_cap, "%s (%s) [%04x:%02x:%02x.0]", ctx->prop.name, ctx->prop.gcnArchName, ctx->prop.pciDomainID,
                  ctx->prop.pciBusID, ctx->prop.pciDeviceID);
  }
  if (n_cu) *n_cu = ctx->prop.multiProcessorCount;
  if (hbm_bytes) *hbm_bytes = (uint64_t)ctx->prop.totalGlobalMem;
  return 0;
}

int mjhmc_energy_create(mjhmc_ctx* ctx, int kind, int ndims, const double* params, size_t nparams,
                        mjhmc_energy** out) {
  if (!ctx || !out) return fail(MJHMC_ERR_INVALID, "ctx/out is NULL");
  if (ndims < 1) return fail(MJHMC_ERR_INVALID, "ndims must be >= 1");
  if (nparams && !params) return fail(MJHMC_ERR_INVALID, "params is NULL");
  HIPCHK(hipSetDevice(ctx->device));
  mjhmc_energy* e = new mjhmc_energy();
  e->ctx = ctx;
  e->params.assign(params, params + nparams);
  std::memset(&e->ep, 0, sizeof(e->ep));
  e->ep.kind = kind;
  e->ep.ndims = ndims;
  auto need = [&](size_t n) { return nparams == n; };
  int rc = 0;
  switch (kind) {
    case MJHMC_E_ISO_GAUSS:
      if (!need(1) || !(params[0] > 0)) rc = fail(MJHMC_ERR_INVALID, "ISO_GAUSS expects {sigma > 0}");
      else e->ep.p[0] = params[0];
      break;
    case MJHMC_E_ROUGH_WELL:
      if (!need(2)) rc = fail(MJHMC_ERR_INVALID, "ROUGH_WELL expects {scale1, scale2}");
      else {
        e->ep.p[0] = params[0];
        e->ep.p[1] = params[1];
      }
      break;
    case MJHMC_E_MM_GAUSS:
    case MJHMC_E_FUNNEL_NEAL:
    case MJHMC_E_FUNNEL_REF:
      if (!need(1)) rc = fail(MJHMC_ERR_INVALID, "expects one scalar parameter");
      else e->ep.p[0] = params[0];
      break;
    case MJHMC_E_DIAG_GAUSS: {
      if (!need((size_t)ndims)) {
        rc = fail(MJHMC_ERR_INVALID, "DIAG_GAUSS expects ndims diagonal entries");
        break;
      }
      const size_t npad = std::max<size_t>(kParamPad, (size_t)ndims);  // (more than kParamPad dims: the multi-pass path)
      std::vector<double> h64(npad, 0.0);
      std::vector<float> h32(npad, 0.f);
      for (int i = 0; i < ndims; ++i) {
        h64[i] = params[i];
        h32[i] = (float)params[i];
      }
      if (hipMalloc(&e->dev64, npad * sizeof(double)) != hipSuccess ||
          hipMalloc(&e->dev32, npad * sizeof(float)) != hipSuccess ||
          hipMemcpy(e->dev64, h64.data(), npad * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
          hipMemcpy(e->dev32, h32.data(), npad * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
        rc = fail(MJHMC_ERR_HIP, "allocating DIAG_GAUSS parameters failed");
      e->ep.dev_f64 = e->dev64;
      e->ep.dev_f32 = e->dev32;
      break;
    }
    case MJHMC_E_PRODUCT_OF_T: {
      // params = {nbasis, W[D*nbasis] row-major, nu[nbasis], b[nbasis]}  (distributions.py:379-406)
      const int K = nparams ? (int)params[0] : 0;
      if (K != ndims || nparams != (size_t)1 + (size_t)ndims * K + 2 * (size_t)K) {
        rc = fail(MJHMC_ERR_INVALID, "PRODUCT_OF_T expects {nbasis == ndims, W[D*K], nu[K], b[K]}");
        break;
      }
      const double* W = params + 1;
      const double* nu = W + (size_t)ndims * K;
      const double* b = nu + K;
      // up to 512 dims: the register-resident tile kernels; beyond: 512 x 512 blocks for the multi-pass path (pot_big_eval)
      const int DIM = ndims <= 128 ? 128 : (ndims <= 256 ? 256 : (ndims + 511) / 512 * 512);
      const int nb = DIM / 512;   // (>= 2: blocked storage)
      e->pot_dim = DIM;
      const size_t M = (size_t)DIM * DIM;
      std::vector<float> w1(M, 0.f), w2t(M, 0.f), cb(DIM, 0.f), al(DIM, 0.f);
      for (int j = 0; j < K; ++j) {
        // parameters are float32 in the reference (theano.shared(np.array(.., dtype='float32')), :398-406)
        const double nuj = (double)(float)nu[j];
        cb[j] = (float)((double)(float)b[j] / nuj);
        al[j] = (float)((nuj + 1.0) / 2.0);
        for (int d = 0; d < ndims; ++d) {
          const double wdj = (double)(float)W[(size_t)d * K + j];
          if (nb < 2) {
            w1[(size_t)d * DIM + j] = (float)(wdj / nuj);
            w2t[(size_t)j * DIM + d] = (float)(wdj * (nuj + 1.0) / nuj);
          } else {   // W1b[db][jb][d % 512][j % 512], W2Tb[jb][db][j % 512][d % 512]
            const size_t db = (size_t)d / 512, jb = (size_t)j / 512, dl = (size_t)d % 512, jl = (size_t)j % 512;
            w1[((db * nb + jb) * 512 + dl) * 512 + jl] = (float)(wdj / nuj);
            w2t[((jb * nb + db) * 512 + jl) * 512 + dl] = (float)(wdj * (nuj + 1.0) / nuj);
          }
        }
      }
      const void* src[4] = {w1.data(), w2t.data(), cb.data(), al.data()};
      const size_t bytes[4] = {M * 4, M * 4, (size_t)DIM * 4, (size_t)DIM * 4};
      for (int i = 0; i < 4 && !rc; ++i) {
        if (hipMalloc((void**)&e->pot[i], bytes[i]) != hipSuccess ||
            hipMemcpy(e->pot[i], src[i], bytes[i], hipMemcpyHostToDevice) != hipSuccess)
          rc = fail(MJHMC_ERR_HIP, "allocating PRODUCT_OF_T parameters failed");
      }
      break;
    }
    case MJHMC_E_SPARSE_CODE: {
      // params = {n_patches, img, n_coeffs, lambda, cauchy, B[img*n_coeffs] (img, n_coeffs) row-major, Y[n_patches*img]}
      if (nparams < 5) {
        rc = fail(MJHMC_ERR_INVALID, "SPARSE_CODE expects {n_patches, img, n_coeffs, lambda, cauchy, B, Y}");
        break;
      }
      const int P = (int)params[0], I = (int)params[1], C = (int)params[2];
      if (P < 1 || P > 32 || I != kSicImg || !sic_coeffs_supported(C) || ndims != P * C) {
        rc = fail(MJHMC_ERR_UNSUPPORTED,
                  "SPARSE_CODE device kernel is built for img_size=256, n_coeffs=1024 or 512, 1 <= n_patches <= 32");
        break;
      }
      e->sic_P = P;
      e->sic_nc = C;
      if (nparams != (size_t)5 + (size_t)I * C + (size_t)P * I) {
        rc = fail(MJHMC_ERR_INVALID, "SPARSE_CODE parameter vector has the wrong length");
        break;
      }
      e->sic_lambda = (float)params[3];
      e->sic_cauchy = params[4] != 0.0 ? 1 : 0;
      const double* B = params + 5;
      const double* Y = B + (size_t)I * C;
      auto bf16_of = [](double v) -> uint16_t {  // round-to-nearest-even float32 -> bfloat16
        float f = (float)v;
        uint32_t u;
        std::memcpy(&u, &f, 4);
        if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((u >> 16) | 0x40);
        u += 0x7FFFu + ((u >> 16) & 1u);
        return (uint16_t)(u >> 16);
      };
      const int NB = C / 256;  // 32-row blocks per wave (8 waves share the C coefficient rows)
      std::vector<uint16_t> a1((size_t)(C / 16) * 2 * I * 8), a2((size_t)16 * 2 * C * 8);
      for (int ks = 0; ks < C / 16; ++ks)
        for (int h = 0; h < 2; ++h)
          for (int i = 0; i < I; ++i)
            for (int j = 0; j < 8; ++j) {
              const int ws = ks / (2 * NB), b = (ks >> 1) % NB, sx = ks & 1;
              const int c = 32 * NB * ws + 32 * b + 16 * sx + 8 * (j >> 2) + 4 * h + (j & 3);
              a1[(((size_t)ks * 2 + h) * I + i) * 8 + j] = bf16_of(B[(size_t)i * C + c]);
            }
      for (int ks = 0; ks < 16; ++ks)
        for (int h = 0; h < 2; ++h)
          for (int c = 0; c < C; ++c)
            for (int j = 0; j < 8; ++j) {
              const int ws = ks >> 1, sx = ks & 1;
              const int i = 32 * ws + 16 * sx + 8 * (j >> 2) + 4 * h + (j & 3);
              a2[(((size_t)ks * 2 + h) * C + c) * 8 + j] = bf16_of(B[(size_t)i * C + c]);
            }
      std::vector<float> yv((size_t)P * I);
      for (size_t i = 0; i < yv.size(); ++i) yv[i] = (float)Y[i];
      const void* src[3] = {a1.data(), a2.data(), yv.data()};
      const size_t bytes[3] = {a1.size() * 2, a2.size() * 2, yv.size() * 4};
      // the two fragment orders of the dictionary are kept in kSicCopies identical copies (workgroups of an XCD
      // alternate between them): every CU streams the same 1 MB per leapfrog step out of its XCD's L2, and spreading
      // that over two sets of lines was measured faster than all CUs hitting one
      e->sic_copies = kSicCopies;
      if (const char* cp = test_env("MJHMC_SIC_COPIES")) e->sic_copies = std::max(1, std::min(4, std::atoi(cp)));
      for (int i = 0; i < 3 && !rc; ++i) {
        const int reps = i < 2 ? e->sic_copies : 1;
        if (hipMalloc(&e->sic[i], bytes[i] * reps) != hipSuccess) rc = fail(MJHMC_ERR_HIP, "allocating SPARSE_CODE parameters failed");
        for (int r = 0; r < reps && !rc; ++r)
          if (hipMemcpy((char*)e->sic[i] + (size_t)r * bytes[i], src[i], bytes[i], hipMemcpyHostToDevice) != hipSuccess)
            rc = fail(MJHMC_ERR_HIP, "uploading SPARSE_CODE parameters failed");
      }
      break;
    }
    case MJHMC_E_HOST:  // no device form: the caller evaluates E and dE/dX (host_energy.hip)
      if (nparams) rc = fail(MJHMC_ERR_INVALID, "HOST takes no parameters");
      break;
    default:
      rc = fail(MJHMC_ERR_UNSUPPORTED, "energy kind not implemented in this build");
  }
  if (rc) return destroy_keeping_error(e, rc);
  *out = e;
  return 0;
}

int mjhmc_energy_create_expr_coupled(mjhmc_ctx* ctx, int ndims, const char* stat_exprs, const char* energy_expr,
                                     const char* energy0_expr, const char* grad_expr, const double* params, size_t nparams,
                                     const char* include_dir, mjhmc_energy** out) {
  if (!ctx || !out || !energy_expr || !grad_expr || !include_dir) return fail(MJHMC_ERR_INVALID, "NULL argument");
  if (ndims < 1) return fail(MJHMC_ERR_INVALID, "ndims must be >= 1");
  if (nparams && !params) return fail(MJHMC_ERR_INVALID, "params is NULL");
  HIPCHK(hipSetDevice(ctx->device));
  Shape sh;
  TRY(pick_shape(ndims, MJHMC_F64, &sh));
  mjhmc_energy* e = new mjhmc_energy();
  e->ctx = ctx;
  if (nparams) e->params.assign(params, params + nparams);
  std::memset(&e->ep, 0, sizeof(e->ep));
  e->ep.kind = MJHMC_E_USER_EXPR;
  e->ep.ndims = ndims;
  const int rc = user_energy_build(e, energy_expr, grad_expr, stat_exprs, energy0_expr, include_dir, params, nparams, sh.E);
  if (rc) return destroy_keeping_error(e, rc);
  *out = e;
  return 0;
}

int mjhmc_energy_create_expr(mjhmc_ctx* ctx, int ndims, const char* energy_expr, const char* grad_expr,
                             const double* params, size_t nparams, const char* include_dir, mjhmc_energy** out) {
  return mjhmc_energy_create_expr_coupled(ctx, ndims, nullptr, energy_expr, nullptr, grad_expr, params, nparams, include_dir, out);
}

int mjhmc_expr_check_coupled(int ndims, const char* stat_exprs, const char* energy_expr, const char* energy0_expr,
                             const char* grad_expr, const char* include_dir) {
  if (!energy_expr || !grad_expr || !include_dir) return fail(MJHMC_ERR_INVALID, "NULL argument");
  if (ndims < 1) return fail(MJHMC_ERR_INVALID, "ndims must be >= 1");
  Shape sh;
  TRY(pick_shape(ndims, MJHMC_F64, &sh));
  std::vector<char> code;
  std::vector<std::string> lowered;
  std::string err;
  const int rc = user_expr_compile(user_expr_source(energy_expr, grad_expr, stat_exprs ? stat_exprs : "", energy0_expr ? energy0_expr : ""),
                                   include_dir, sh.E, &code, &lowered, &err);
  return rc ? fail(rc, err) : 0;
}

int mjhmc_expr_check(int ndims, const char* energy_expr, const char* grad_expr, const char* include_dir) {
  return mjhmc_expr_check_coupled(ndims, nullptr, energy_expr, nullptr, grad_expr, include_dir);
}

// What the mjhmc_energy_create_linear* entry points share; each entry point keeps its own order of checks (sizes before ctx for
// the tall, grouped and wide forms, after it for the square one).
static int linear_check_model(const double* W, const double* b, const double* params, size_t nparams, const double* expert_params,
                              int n_expert_rows) {
  if (!W || !b) return fail(MJHMC_ERR_INVALID, "W or b is NULL");
  if (nparams && !params) return fail(MJHMC_ERR_INVALID, "params is NULL");
  if (n_expert_rows < 0 || n_expert_rows > 4 || (n_expert_rows && !expert_params))
    return fail(MJHMC_ERR_INVALID, "LINEAR_EXPR takes 0 to 4 per-expert parameter rows");
  return 0;
}

static int linear_check_finite(int ndims, int64_t nexperts, const double* W, const double* b) {
  for (size_t i = 0, n = (size_t)nexperts * ndims; i < n; ++i)
    if (!std::isfinite(W[i])) return fail(MJHMC_ERR_INVALID, "W has a non-finite entry (row " + std::to_string(i / ndims) + ")");
  for (int64_t j = 0; j < nexperts; ++j)
    if (!std::isfinite(b[j])) return fail(MJHMC_ERR_INVALID, "b has a non-finite entry (" + std::to_string(j) + ")");
  return 0;
}

// a new MJHMC_E_LINEAR_EXPR energy on ctx's device, built by `build`; destroyed again, keeping the message, if that fails
static int linear_energy_shell(mjhmc_ctx* ctx, int ndims, mjhmc_energy** out, const std::function<int(mjhmc_energy*)>& build) {
  HIPCHK(hipSetDevice(ctx->device));
  mjhmc_energy* e = new mjhmc_energy();
  e->ctx = ctx;
  std::memset(&e->ep, 0, sizeof(e->ep));
  e->ep.kind = MJHMC_E_LINEAR_EXPR;
  e->ep.ndims = ndims;
  const int rc = build(e);
  if (rc) return destroy_keeping_error(e, rc);
  *out = e;
  return 0;
}

int mjhmc_energy_create_linear(mjhmc_ctx* ctx, int ndims, int nexperts, const double* W, const double* b,
                               const char* energy_expr, const char* grad_expr, const double* params, size_t nparams,
                               const double* expert_params, int n_expert_rows, const char* include_dir, mjhmc_energy** out) {
  if (!ctx || !out) return fail(MJHMC_ERR_INVALID, "NULL argument");
  TRY(linear_check_args(ndims, nexperts, energy_expr, grad_expr, include_dir));
  TRY(linear_check_model(W, b, params, nparams, expert_params, n_expert_rows));
  return linear_energy_shell(ctx, ndims, out, [&](mjhmc_energy* e) {
    return linear_energy_build(e, nexperts, W, b, energy_expr, grad_expr, params, nparams, expert_params, n_expert_rows, include_dir);
  });
}

int mjhmc_linear_check(int ndims, int nexperts, const char* energy_expr, const char* grad_expr, const char* include_dir) {
  TRY(linear_check_args(ndims, nexperts, energy_expr, grad_expr, include_dir));
  std::string err;
  const RtcCode* c = nullptr;
  const int rc = linear_compile(energy_expr, grad_expr, linear_dim(ndims, nexperts), include_dir, &err, &c);
  return rc ? fail(rc, err) : 0;
}

int mjhmc_energy_create_linear_tall(mjhmc_ctx* ctx, int ndims, int64_t nexperts, const double* W, const double* b,
                                    const char* energy_expr, const char* grad_expr, const double* params, size_t nparams,
                                    const double* expert_params, int n_expert_rows, const char* include_dir, mjhmc_energy** out) {
  TRY(linear_tall_check_args(ndims, nexperts, energy_expr, grad_expr, include_dir));
  if (!ctx || !out) return fail(MJHMC_ERR_INVALID, "NULL argument");
  TRY(linear_check_model(W, b, params, nparams, expert_params, n_expert_rows));
  TRY(linear_check_finite(ndims, nexperts, W, b));
  return linear_energy_shell(ctx, ndims, out, [&](mjhmc_energy* e) {
    return linear_tall_energy_build(e, nexperts, W, b, energy_expr, grad_expr, params, nparams, expert_params, n_expert_rows,
                                    include_dir);
  });
}

int mjhmc_linear_tall_check(int ndims, int64_t nexperts, const char* energy_expr, const char* grad_expr, const char* include_dir) {
  TRY(linear_tall_check_args(ndims, nexperts, energy_expr, grad_expr, include_dir));
  std::string err;
  const RtcCode* c = nullptr;
  const int rc = linear_tall_compile(energy_expr, grad_expr, tall_pad(ndims), include_dir, &err, &c);
  return rc ? fail(rc, err) : 0;
}

int mjhmc_energy_create_linear_wide(mjhmc_ctx* ctx, int ndims, int64_t nexperts, const double* W, const double* b,
                                    const char* energy_expr, const char* grad_expr, const double* params, size_t nparams,
                                    const double* expert_params, int n_expert_rows, const char* include_dir, mjhmc_energy** out) {
  TRY(linear_wide_check_args(ndims, nexperts, energy_expr, grad_expr, include_dir));
  if (!ctx || !out) return fail(MJHMC_ERR_INVALID, "NULL argument");
  TRY(linear_check_model(W, b, params, nparams, expert_params, n_expert_rows));
  TRY(linear_check_finite(ndims, nexperts, W, b));
  return linear_energy_shell(ctx, ndims, out, [&](mjhmc_energy* e) {
    return linear_wide_energy_build(e, nexperts, W, b, energy_expr, grad_expr, params, nparams, expert_params, n_expert_rows,
                                    include_dir);
  });
}

int mjhmc_linear_wide_check(int ndims, int64_t nexperts, const char* energy_expr, const char* grad_expr, const char* include_dir) {
  TRY(linear_wide_check_args(ndims, nexperts, energy_expr, grad_expr, include_dir));
  std::string err;
  const RtcCode* c = nullptr;
  const int rc = linear_wide_compile(energy_expr, grad_expr, include_dir, &err, &c);
  return rc ? fail(rc, err) : 0;
}

int mjhmc_energy_create_linear_grouped(mjhmc_ctx* ctx, int ndims, int64_t nexperts, const double* W, const double* b,
                                       int group_size, int64_t n_groups, const char* energy_expr, const char* grad_expr,
                                       const double* params, size_t nparams, const double* expert_params, int n_expert_rows,
                                       const char* include_dir, mjhmc_energy** out) {
  TRY(linear_grouped_check_args(ndims, nexperts, group_size, n_groups, energy_expr, grad_expr, include_dir));
  if (!ctx || !out) return fail(MJHMC_ERR_INVALID, "NULL argument");
  TRY(linear_check_model(W, b, params, nparams, expert_params, n_expert_rows));
  TRY(linear_check_finite(ndims, nexperts, W, b));
  return linear_energy_shell(ctx, ndims, out, [&](mjhmc_energy* e) {
    return linear_grouped_energy_build(e, nexperts, W, b, group_size, n_groups, energy_expr, grad_expr, params, nparams,
                                       expert_params, n_expert_rows, include_dir);
  });
}

int mjhmc_linear_grouped_check(int ndims, int64_t nexperts, int group_size, int64_t n_groups, const char* energy_expr,
                               const char* grad_expr, const char* include_dir) {
  TRY(linear_grouped_check_args(ndims, nexperts, group_size, n_groups, energy_expr, grad_expr, include_dir));
  std::string err;
  const RtcCode* c = nullptr;
  const int dim = linear_grouped_layout(ndims, nexperts, group_size, n_groups).P;
  const int rc = linear_grouped_compile(energy_expr, grad_expr, dim, group_size, include_dir, &err, &c);
  return rc ? fail(rc, err) : 0;
}

int mjhmc_linear_grouped_layout(int ndims, int64_t nexperts, int group_size, int64_t n_groups, int64_t* slot_to_expert,
                                int64_t* n_slots) {
  if (!n_slots) return fail(MJHMC_ERR_INVALID, "NULL argument");
  TRY(linear_grouped_check_args(ndims, nexperts, group_size, n_groups, "", "", ""));
  const LinGroupedLayout L = linear_grouped_layout(ndims, nexperts, group_size, n_groups);
  *n_slots = L.nslots;
  if (slot_to_expert)
    for (int64_t s = 0; s < L.nslots; ++s) slot_to_expert[s] = linear_grouped_slot_expert(L, nexperts, group_size, n_groups, s);
  return 0;
}

int mjhmc_energy_destroy(mjhmc_energy* e) {
  if (!e) return 0;
  user_energy_free(e);
  linear_energy_free(e);
  if (e->dev64) (void)hipFree(e->dev64);
  if (e->dev32) (void)hipFree(e->dev32);
  for (float* q : e->pot)
    if (q) (void)hipFree(q);
  for (void* q : e->sic)
    if (q) (void)hipFree(q);
  delete e;
  return 0;
}

int mjhmc_sampler_destroy(mjhmc_sampler* s) {
  if (!s) return 0;
  (void)hipSetDevice(s->ctx->device);
  if (s->stream) (void)hipStreamSynchronize(s->stream);
  functionals_free_all(s);   // (and the handles created on them)
  accumulators_free_all(s);
  timegrid_free_all(s);
  stein_free_all(s);
  void* ptrs[] = {s->flf_list, s->call_block, s->Hpre, s->Hwork, s->cold_list, s->Hspec[0], s->Hspec[1], s->Hspec_dump, s->Gbuf[0], s->Gbuf[1], s->Xbuf[0], s->Xbuf[1], s->Vbuf[0],  s->Vbuf[1], s->EX[0],     s->EX[1],  s->EV[0],
                  s->EV[1],   s->Hflf[0], s->Hflf[1],  s->dwell,  s->dwell_scratch,  s->trans,
                  s->ring,     s->dwell_ring, s->stage,  s->noise,  s->rexp,
                  s->runif,   s->scratch,  s->ck[0],    s->ck[1],    s->ck[2],   s->ck[3],  s->ck[4],
                  s->ck[5],   s->ck[6]};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  for (auto& e : s->ev_total)
    if (e) (void)hipEventDestroy(e);
  for (auto& e : s->ev_k) (void)hipEventDestroy(e);
  for (auto& e : s->part_events) (void)hipEventDestroy(e);
  for (auto& q : s->part_streams) (void)hipStreamDestroy(q);
  if (s->ev_join) (void)hipEventDestroy(s->ev_join);
  if (s->ev_fork) (void)hipEventDestroy(s->ev_fork);
  for (void* q : s->ick)
    if (q) (void)hipFree(q);
  if (s->h_pin) (void)hipHostFree(s->h_pin);
  if (s->dl_stage) (void)hipFree(s->dl_stage);
  for (int i = 0; i < 2; ++i) {
    if (s->dl_pin[i]) (void)hipHostFree(s->dl_pin[i]);
    if (s->dl_ev[i]) (void)hipEventDestroy(s->dl_ev[i]);
  }
  if (s->dl_stream) (void)hipStreamDestroy(s->dl_stream);
  for (int i = 0; i < 2; ++i) {
    if (s->pipe_pin[i]) (void)hipHostFree(s->pipe_pin[i]);
    if (s->pipe_ev[i]) (void)hipEventDestroy(s->pipe_ev[i]);
  }
  proposal_rows_free(s);
  if (s->stream) (void)hipStreamDestroy(s->stream);
  delete s;
  return 0;
}

int mjhmc_sampler_create(mjhmc_ctx* ctx, mjhmc_energy* e, int64_t nparticles, int64_t first_particle_id, int dtype,
                         const double* Xinit, const double* Vinit, uint64_t seed, int mode, mjhmc_sampler** out) {
  if (!ctx || !e || !out || !Xinit) return fail(MJHMC_ERR_INVALID, "NULL argument");
  if (nparticles < 1) return fail(MJHMC_ERR_INVALID, "nparticles must be >= 1");
  TRY(check_state_dtype(e, dtype));
  if (mode < MJHMC_MODE_MJHMC || mode > MJHMC_MODE_CTHMC) return fail(MJHMC_ERR_INVALID, "unknown sampler mode");
  if (first_particle_id < 0 || first_particle_id + nparticles > 0xFFFFFFFFLL)
    return fail(MJHMC_ERR_INVALID, "global particle ids must fit 32 bits");
  HIPCHK(hipSetDevice(ctx->device));
  mjhmc_sampler* s = new mjhmc_sampler();
  s->ctx = ctx;
  s->en = e;
  s->N = nparticles;
  s->Npad = (nparticles + 63) / 64 * 64;
  s->first_pid = first_particle_id;
  s->D = e->ep.ndims;
  s->dtype = dtype;
  s->mode = mode;
  s->seed = seed;
  int rc = shape_for(e, &s->dtype, &s->sh);
  if (rc) {
    delete s;
    return rc;
  }
  dtype = s->dtype;   // (the storage dtype)
  auto build = [&]() -> int {
    HIPCHK(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
    const size_t mb = mat_bytes(s);
    for (int i = 0; i < 2; ++i) {
      HIPCHK(hipMalloc(&s->Xbuf[i], mb));
      HIPCHK(hipMalloc(&s->Vbuf[i], mb));
      HIPCHK(hipMemsetAsync(s->Xbuf[i], 0, mb, s->stream));
      HIPCHK(hipMemsetAsync(s->Vbuf[i], 0, mb, s->stream));
      if (e->is_pot() || ((e->is_host() || s->sh.wide) && i == 0)) {  // these keep dE/dX as part of the state, like HMCState.dEdX
        HIPCHK(hipMalloc(&s->Gbuf[i], mb));
        HIPCHK(hipMemsetAsync(s->Gbuf[i], 0, mb, s->stream));
      }
      if (e->is_dense()) {
        if (!s->Hwork) {
          HIPCHK(hipMalloc((void**)&s->Hwork, s->Npad * ssize(s)));  // float32, or float64 for ProductOfT's float64 state
          HIPCHK(hipMemsetAsync(s->Hwork, 0, s->Npad * ssize(s), s->stream));   // (padding rows read it and ignore it)
          HIPCHK(hipMalloc((void**)&s->cold_list, (2 * s->Npad + 3 * kMaxDenseParts) * sizeof(int)));  // two lists (iterations alternate) + [part][3] counters
        }
        HIPCHK(hipMalloc(&s->Hspec[i], s->Npad * ssize(s)));
        HIPCHK(hipMemsetAsync(s->Hspec[i], 0xFF, s->Npad * ssize(s), s->stream));   // NaN: nothing handed on
      }
      HIPCHK(hipMalloc(&s->EX[i], s->Npad * ssize(s)));
      HIPCHK(hipMalloc(&s->EV[i], s->Npad * ssize(s)));
      HIPCHK(hipMalloc(&s->Hflf[i], s->Npad * ssize(s)));
      HIPCHK(hipMemsetAsync(s->EX[i], 0, s->Npad * ssize(s), s->stream));
      HIPCHK(hipMemsetAsync(s->EV[i], 0, s->Npad * ssize(s), s->stream));
      HIPCHK(hipMemsetAsync(s->Hflf[i], 0xFF, s->Npad * ssize(s), s->stream));  // all-ones = NaN = cold
    }
    HIPCHK(hipMalloc((void**)&s->dwell, s->Npad * sizeof(double)));
    HIPCHK(hipMemsetAsync(s->dwell, 0, s->Npad * sizeof(double), s->stream));
    HIPCHK(hipMalloc((void**)&s->dwell_scratch, s->Npad * sizeof(double)));
    HIPCHK(hipMalloc((void**)&s->trans, s->Npad));
    HIPCHK(hipMemsetAsync(s->trans, 0, s->Npad, s->stream));
    TRY(ensure_call_block(s, 1024));   // everything mjhmc_iterate needs is created here, so a timed call never allocates
    HIPCHK(hipEventCreate(&s->ev_total[0]));
    HIPCHK(hipEventCreate(&s->ev_total[1]));
    // a state matrix big enough for the pipelined host copies: their pinned buffers now, not inside the first read
    if ((size_t)s->D * s->N * sizeof(double) >= 2 * kPipeChunk) TRY(ensure_pipe_pair(s->pipe_pin, s->pipe_ev));
    s->Xcur = s->Xbuf[0];
    TRY(upload_matrix(s, Xinit, s->Xcur));
    if (s->sh.round32) TRY(round_rows32(s, s->Xcur));
    if (Vinit) {
      TRY(upload_matrix(s, Vinit, s->Vbuf[0]));
      if (s->sh.round32) TRY(round_rows32(s, s->Vbuf[0]));
      TRY(run_eval(s, s->Xcur, s->Gbuf[0], s->EX[0], s->Vbuf[0], nullptr, s->EV[0]));
    } else {
      TRY(run_eval(s, s->Xcur, s->Gbuf[0], s->EX[0], nullptr, s->Vbuf[0], s->EV[0]));
      if (s->sh.round32) {   // the generated momentum is stored in float32 too: its kinetic energy is that of what is stored
        TRY(round_rows32(s, s->Vbuf[0]));
        TRY(run_eval(s, nullptr, nullptr, nullptr, s->Vbuf[0], nullptr, s->EV[0]));
      }
    }
    HIPCHK(hipStreamSynchronize(s->stream));
    return 0;
  };
  rc = build();
  if (rc) {
    std::string keep = g_err;
    mjhmc_sampler_destroy(s);
    g_err = keep;
    return rc;
  }
  *out = s;
  return 0;
}

int mjhmc_set_hparams(mjhmc_sampler* s, double epsilon, int num_leapfrog_steps, double p_r, double beta,
                      double p_flip) {
  if (!s) return fail(MJHMC_ERR_INVALID, "sampler is NULL");
  if (num_leapfrog_steps < 0) return fail(MJHMC_ERR_INVALID, "num_leapfrog_steps must be >= 0");
  if (epsilon != s->eps || num_leapfrog_steps != s->L) TRY(drop_spec(s));
  s->eps = epsilon;
  s->L = num_leapfrog_steps;
  s->p_r = p_r;
  s->beta = beta;
  s->p_flip = p_flip;
  return 0;
}

// ProductOfT keeps dE/dX of the current state (HMCState.dEdX) and the jump kernel does not recompute it: it is part of
// the state a rollback must put back; so it is for the other samplers that store it
static bool keeps_dEdX(const mjhmc_sampler* s) { return s->en->is_pot() || s->en->is_host() || s->sh.wide; }

int mjhmc_checkpoint(mjhmc_sampler* s) {
  if (!s) return fail(MJHMC_ERR_INVALID, "sampler is NULL");
  HIPCHK(hipSetDevice(s->ctx->device));
  void* src[7];
  size_t sizes[7];
  const int nck = live_state(s, keeps_dEdX(s), src, sizes);
  for (int i = 0; i < nck; ++i) {
    if (!s->ck[i]) HIPCHK(hipMalloc(&s->ck[i], sizes[i]));
    HIPCHK(hipMemcpyAsync(s->ck[i], src[i], sizes[i], hipMemcpyDeviceToDevice, s->stream));
  }
  s->ck_tick = s->tick;
  s->ck_valid = true;
  return 0;
}

int mjhmc_restore(mjhmc_sampler* s) {
  if (!s) return fail(MJHMC_ERR_INVALID, "sampler is NULL");
  if (!s->ck_valid) return fail(MJHMC_ERR_INVALID, "no checkpoint taken");
  HIPCHK(hipSetDevice(s->ctx->device));
  s->Xcur = s->Xbuf[0];
  void* dst[7];
  size_t sizes[7];
  const int nck = live_state(s, keeps_dEdX(s), dst, sizes);
  for (int i = 0; i < nck; ++i) HIPCHK(hipMemcpyAsync(dst[i], s->ck[i], sizes[i], hipMemcpyDeviceToDevice, s->stream));
  TRY(drop_spec(s));
  s->list_valid = false;
  s->tick = s->ck_tick;
  s->undo_valid = false;
  HIPCHK(hipStreamSynchronize(s->stream));
  return 0;
}

int mjhmc_rollback(mjhmc_sampler* s) {
  if (!s) return fail(MJHMC_ERR_INVALID, "sampler is NULL");
  if (!s->undo_valid) return fail(MJHMC_ERR_INVALID, "nothing to roll back: the last call was not a committed single iteration");
  // an iteration reads one buffer parity and writes the other: flipping the parities back IS the pre-move state
  // (X, V, EX, EV, H_flf and, for ProductOfT, dE/dX); dwell / trans hold the rolled-back attempt's values until
  // the retry overwrites them.  The RNG tick stays consumed, like the reference's already-drawn numbers.
  s->undo_valid = false;
  s->list_valid = false;   // (the carried list is the rolled-back successor's)
  if (s->undo_multipass) return multipass_rollback(s);   // committed in place: the pre-move state is copied back
  s->Xcur = s->undo_X;
  s->vcur ^= 1;
  s->scur ^= 1;
  return 0;
}

int mjhmc_get_tick(mjhmc_sampler* s, uint64_t* tick) {
  if (!s || !tick) return fail(MJHMC_ERR_INVALID, "NULL argument");
  *tick = s->tick;
  return 0;
}

int mjhmc_set_tick(mjhmc_sampler* s, uint64_t tick) {
  if (!s) return fail(MJHMC_ERR_INVALID, "sampler is NULL");
  s->tick = tick;
  s->undo_valid = false;
  return 0;
}

int mjhmc_advance_tick(mjhmc_sampler* s, int64_t n) {
  if (!s || n < 0) return fail(MJHMC_ERR_INVALID, "bad argument");
  s->tick += (uint64_t)n;
  return 0;
}

int mjhmc_reset_flf_cache(mjhmc_sampler* s) {
  if (!s) return fail(MJHMC_ERR_INVALID, "sampler is NULL");
  HIPCHK(hipSetDevice(s->ctx->device));
  HIPCHK(hipMemsetAsync(s->Hflf[s->scur], 0xFF, s->Npad * ssize(s), s->stream));
  s->list_valid = false;
  return drop_spec(s);
}


int mjhmc_mem_info(mjhmc_ctx* ctx, uint64_t* free_bytes, uint64_t* total_bytes) {
  if (!ctx || !free_bytes || !total_bytes) return fail(MJHMC_ERR_INVALID, "NULL argument");
  HIPCHK(hipSetDevice(ctx->device));
  size_t f = 0, t = 0;
  HIPCHK(hipMemGetInfo(&f, &t));
  *free_bytes = f;
  *total_bytes = t;
  return 0;
}

int mjhmc_draw_from(mjhmc_ctx* ctx, const double* rates, const double* unit_exp, int64_t n, double* out,
                    int64_t* first_bad) {
  if (!ctx || !rates || !unit_exp || !out || n < 0) return fail(MJHMC_ERR_INVALID, "bad argument");
  if (first_bad) *first_bad = -1;
  if (n == 0) return 0;
  HIPCHK(hipSetDevice(ctx->device));
  double *d_r = nullptr, *d_e = nullptr, *d_o = nullptr;
  long long* d_bad = nullptr;
  const size_t bytes = (size_t)n * sizeof(double);
  const long long none = 0x7fffffffffffffffLL;
  long long bad = none;
  hipError_t rc = hipMalloc(&d_r, 3 * bytes + sizeof(long long));
  if (rc != hipSuccess) return fail(MJHMC_ERR_HIP, hipGetErrorString(rc));
  d_e = d_r + n;
  d_o = d_e + n;
  d_bad = reinterpret_cast<long long*>(d_o + n);
  rc = hipMemcpy(d_r, rates, bytes, hipMemcpyHostToDevice);
  if (rc == hipSuccess) rc = hipMemcpy(d_e, unit_exp, bytes, hipMemcpyHostToDevice);
  if (rc == hipSuccess) rc = hipMemcpy(d_bad, &none, sizeof(long long), hipMemcpyHostToDevice);
  if (rc == hipSuccess) {
    hipLaunchKernelGGL(draw_from_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d_r, d_e, n, d_o, d_bad);
    rc = hipGetLastError();
  }
  if (rc == hipSuccess) rc = hipMemcpy(out, d_o, bytes, hipMemcpyDeviceToHost);
  if (rc == hipSuccess) rc = hipMemcpy(&bad, d_bad, sizeof(long long), hipMemcpyDeviceToHost);
  (void)hipFree(d_r);
  if (rc != hipSuccess) return fail(MJHMC_ERR_HIP, hipGetErrorString(rc));
  if (bad != none) {
    if (first_bad) *first_bad = (int64_t)bad;
    return fail(MJHMC_ERR_NONFINITE, "Infinite rate (mjhmc/misc/utils.py:43-48)");
  }
  return 0;
}

int mjhmc_min_idx(mjhmc_ctx* ctx, const double* draws, int k, int64_t n, int32_t* which) {
  if (!ctx || !draws || !which || k < 1 || n < 0) return fail(MJHMC_ERR_INVALID, "bad argument");
  if (n == 0) return 0;
  HIPCHK(hipSetDevice(ctx->device));
  double* d_d = nullptr;
  const size_t bytes = (size_t)k * (size_t)n * sizeof(double);
  hipError_t rc = hipMalloc(&d_d, bytes + (size_t)n * sizeof(int32_t));
  if (rc != hipSuccess) return fail(MJHMC_ERR_HIP, hipGetErrorString(rc));
  int32_t* d_w = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(d_d) + bytes);
  rc = hipMemcpy(d_d, draws, bytes, hipMemcpyHostToDevice);
  if (rc == hipSuccess) {
    hipLaunchKernelGGL(min_idx_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d_d, k, n, d_w);
    rc = hipGetLastError();
  }
  if (rc == hipSuccess) rc = hipMemcpy(which, d_w, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost);
  (void)hipFree(d_d);
  if (rc != hipSuccess) return fail(MJHMC_ERR_HIP, hipGetErrorString(rc));
  return 0;
}

int mjhmc_autocor(mjhmc_ctx* ctx, const double* samples, int64_t n_series, int n_samples, int linear,
                  double* host_out) {
  if (!ctx || !samples || !host_out) return fail(MJHMC_ERR_INVALID, "NULL argument");
  HIPCHK(hipSetDevice(ctx->device));
  std::string err;
  const int rc = autocor_from_host(nullptr, samples, n_series, n_samples, linear, host_out, err);
  return rc ? fail(rc, err) : 0;
}

int mjhmc_lagcov(mjhmc_ctx* ctx, const double* samples, int n_dims, int64_t n_batch, int n_samples, int max_lag,
                 const double* shift, double* A_out, double* S_out) {
  if (!ctx || !samples || !A_out) return fail(MJHMC_ERR_INVALID, "NULL argument");
  HIPCHK(hipSetDevice(ctx->device));
  std::string err;
  const int rc = lagcov_from_host(nullptr, samples, n_dims, n_batch, n_samples, max_lag, shift, A_out, S_out, err);
  return rc ? fail(rc, err) : 0;
}

int mjhmc_last_timing(mjhmc_sampler* s, double* total_ms, double* jump_kernel_ms, int* n_jump_launches) {
  if (!s) return fail(MJHMC_ERR_INVALID, "sampler is NULL");
  if (s->timing_pending) {
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, s->ev_total[0], s->ev_total[1]));
    s->last_total_ms = s->last_jump_ms = ms;
    s->timing_pending = false;
  }
  if (total_ms) *total_ms = s->last_total_ms;
  if (jump_kernel_ms) *jump_kernel_ms = s->last_jump_ms;
  if (n_jump_launches) *n_jump_launches = s->last_jump_launches;
  return 0;
}

int mjhmc_set_timing(mjhmc_sampler* s, int on) {
  if (!s) return fail(MJHMC_ERR_INVALID, "sampler is NULL");
  s->timing_on = on != 0;
  if (!s->timing_on) s->timing_pending = false;
  return 0;
}

int mjhmc_sync(mjhmc_sampler* s) {
  if (!s) return fail(MJHMC_ERR_INVALID, "sampler is NULL");
  HIPCHK(hipSetDevice(s->ctx->device));
  HIPCHK(hipStreamSynchronize(s->stream));
  return 0;
}

}  // extern "C"
