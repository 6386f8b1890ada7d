// Linear-model energies:
//
//     E(x) = sum_{j<K} f(u_j, j),   u = W x + b,   dE/dx = W^T f'(u)        (W: K x D, 1 <= D, K <= 512)
//
// with f and f' C expressions of `u` (float), `j` (int), `p[k]` (shared float parameters) and `q[m]` (per-expert parameter
// row m at expert j, m < 4).  This is the ProductOfT tile kernel's force with its elementwise stage replaced: the first
// GEMM forms u (W1 = W^T, cb = b), the caller's f' gives phi(u), the second GEMM applies W (W2T = W).  The model is
// padded to P = 128, 256 or 512 rows in both dimensions like ProductOfT's; experts j >= K are masked (LinearExperts,
// dense_pot_kernels.hpp), the state rows d >= D are zero as everywhere.  The kernels are the built-in ones' own text (the
// fragments dense_pot_{eval,jump,leap}.inc and dense_pot64_jump.inc), compiled with hipRTC around the generated functor
// for the one NB the model needs: float32-state jump kernels x 3 modes x replay, the float64-state ones likewise, eval
// and leap -- 14 kernels.  The cold-list, fix and decide kernels take no model and are the library's own.  Everything
// else (dE/dX storage, call blocks, parts, the multi-pass path at L = 0, state operations) is ProductOfT's: is_pot().
// Models with more experts than 512 (K <= 2^20, D <= 512) are the second half of this file: one fused kernel over expert
// blocks (dense_lin_tall.hpp) as the force of the multi-pass path.  Grouped models (a log-sum-exp
// over groups of experts: softmax regression) are the third part: the tall form with a permuted layout and a kernel of its
// own (dense_lin_grouped.hpp).  Models with more dims than 512 (D <= 4096, K <= 2^20) are the fourth:
// the tall form's blocks with a dim chunk index, one fused kernel over expert blocks x dim chunks (dense_lin_wide.hpp,
// DESIGN.md section 3.6e).
// What the forms share stands once: every compile is "source, name expressions, rtc_compile_cached" (user_expr.hpp: one
// cache for the process), every builder loads its module through linear_module_load and puts its model on the device through
// linear_model_upload (slots in blocks of P and a slot -> expert map: one block and the identity for the square form, the
// identity for the tall one, linear_grouped_slot_expert for the grouped one).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "dense_lin_grouped.hpp"   // LinGroupedModel (the kernel itself is compiled by hipRTC)
#include "handles.hpp"
#include "linear_energy.hpp"

namespace {

// E = sum_j f(u_j, j), dE/dx = W^T f'(u): the caller's expressions as a functor (shared by both generated sources)
std::string user_functor_source(const std::string& energy_expr, const std::string& grad_expr) {
  std::string s;
  s += "// E = sum_j f(u_j, j), dE/dx = W^T f'(u): the caller's expressions (u float, j int, p[k], q[m])\n";
  s += "struct LinUserF {\n";
  s += "  static __device__ __forceinline__ float f(float u, int j, const float* __restrict__ p, LinQ q) {\n";
  s += "    (void)u; (void)j; (void)p; (void)q;\n";
  s += "    return (float)(" + energy_expr + ");\n  }\n";
  s += "  static __device__ __forceinline__ float fp(float u, int j, const float* __restrict__ p, LinQ q) {\n";
  s += "    (void)u; (void)j; (void)p; (void)q;\n";
  s += "    return (float)(" + grad_expr + ");\n  }\n";
  s += "};\n";
  return s;
}

std::string linear_source(const std::string& energy_expr, const std::string& grad_expr) {
  std::string s;
  s += "#include \"dense_pot_kernels.hpp\"\n";
  s += "#include \"dense_pot64_kernels.hpp\"\n";
  s += "namespace mjhmc {\n";
  s += user_functor_source(energy_expr, grad_expr);
  s += "using LinXP = LinearExperts<LinUserF>;\n";
  s += "template <int NB>\n__global__ __launch_bounds__(256, 1) void lin_eval_kernel(const PotEvalArgs a, const PotModel mdl, const PotLinear lin) {\n";
  s += "  const LinXP xp{lin};\n#include \"dense_pot_eval.inc\"\n}\n";
  s += "template <int NB, bool REPLAY, int MODE>\n__global__ __launch_bounds__(256, 1) void lin_jump_kernel(const PotJumpArgs a, const PotModel mdl, const PotLinear lin) {\n";
  s += "  const LinXP xp{lin};\n#include \"dense_pot_jump.inc\"\n}\n";
  s += "template <int NB>\n__global__ __launch_bounds__(256, 1) void lin_leap_kernel(const PotLeapArgs a, const PotModel mdl, const PotLinear lin) {\n";
  s += "  const LinXP xp{lin};\n#include \"dense_pot_leap.inc\"\n}\n";
  s += "template <int NB, bool REPLAY, int MODE>\n__global__ __launch_bounds__(256, 1) void lin64_jump_kernel(const Pot64JumpArgs a, const PotModel mdl, const PotLinear lin) {\n";
  s += "  const LinXP xp{lin};\n#include \"dense_pot64_jump.inc\"\n}\n";
  s += "}  // namespace mjhmc\n";
  return s;
}

// [0, 6): float32-state jump kernels (mode * 2 + replay), [6, 12): float64-state ones, 12: eval, 13: leap
std::vector<std::string> linear_kernel_names(int NB) {
  const std::string nb = std::to_string(NB);
  std::vector<std::string> n;
  for (const char* k : {"lin_jump_kernel", "lin64_jump_kernel"})
    for (int mode = 0; mode < 3; ++mode)
      for (int replay = 0; replay < 2; ++replay)
        n.push_back(std::string("mjhmc::") + k + "<" + nb + ", " + (replay ? "true" : "false") + ", " + std::to_string(mode) + ">");
  n.push_back("mjhmc::lin_eval_kernel<" + nb + ">");
  n.push_back("mjhmc::lin_leap_kernel<" + nb + ">");
  return n;
}

// A tall model's one kernel (dense_lin_tall.hpp): a source of its own, so a tall model compiles this and nothing else
std::string linear_tall_source(const std::string& energy_expr, const std::string& grad_expr) {
  std::string s;
  s += "#include \"dense_lin_tall.hpp\"\n";
  s += "namespace mjhmc {\n";
  s += user_functor_source(energy_expr, grad_expr);
  s += "template <int NB>\n__global__ __launch_bounds__(256, 1) void lin_tall_eval_kernel(const PotEvalArgs a, const LinTallModel tm, const PotLinear lin) {\n";
  s += "  __shared__ Shared<NB> sh;\n  lin_tall_eval_tiles<NB, LinUserF>(a, tm, lin, sh);\n}\n";
  s += "}  // namespace mjhmc\n";
  return s;
}

// A wide model's one kernel (dense_lin_wide.hpp; always the NB = 4 tile code): a source and a cache key of its own
std::string linear_wide_source(const std::string& energy_expr, const std::string& grad_expr) {
  std::string s;
  s += "#include \"dense_lin_wide.hpp\"\n";
  s += "namespace mjhmc {\n";
  s += user_functor_source(energy_expr, grad_expr);
  s += "__global__ __launch_bounds__(256, 1) void lin_wide_eval_kernel(const PotEvalArgs a, const LinWideModel wm, const PotLinear lin) {\n";
  s += "  __shared__ Shared<4> sh;\n  lin_wide_eval_tiles<LinUserF>(a, wm, lin, sh);\n}\n";
  s += "}  // namespace mjhmc\n";
  return s;
}

// The per-expert statistics pass (dense_lin_pointwise.hpp): the caller's M value expressions as a
// functor, and the one kernel around it -- a source of its own, compiled when a pointwise handle is created and never
// when an energy is
std::string linear_pointwise_source(const std::vector<std::string>& values) {
  std::string s;
  s += "#include \"dense_lin_pointwise.hpp\"\n";
  s += "namespace mjhmc {\n";
  s += "// the caller's value expressions h_m(u, j; p, q) (u float, j int, p[k], q[m])\n";
  s += "struct PwUserH {\n";
  s += "  static constexpr int kM = " + std::to_string(values.size()) + ";\n";
  s += "  template <int MI>\n";
  s += "  static __device__ __forceinline__ float h(float u, int j, const float* __restrict__ p, LinQ q) {\n";
  s += "    (void)u; (void)j; (void)p; (void)q;\n";
  for (size_t m = 0; m < values.size(); ++m)
    s += std::string(m ? "    else " : "    ") + "if constexpr (MI == " + std::to_string(m) + ") return (float)(" + values[m] + ");\n";
  s += "    else return 0.f;\n  }\n";
  s += "};\n";
  s += "template <int NB>\n__global__ __launch_bounds__(256, 1) void lin_pointwise_kernel(const PwArgs a, const LinTallModel tm, const PotLinear lin) {\n";
  s += "  __shared__ Shared<NB> sh;\n  __shared__ double wts[kP];\n  lin_pointwise_items<NB, PwUserH>(a, tm, lin, sh, wts);\n}\n";
  s += "}  // namespace mjhmc\n";
  return s;
}

// The values of one block of experts, stored (dense_lin_values.hpp): ONE value expression as a
// functor and the one kernel around it -- a source and a cache key of its own, compiled when an influence handle is created
std::string linear_values_source(const std::string& value) {
  std::string s;
  s += "#include \"dense_lin_values.hpp\"\n";
  s += "namespace mjhmc {\n";
  s += "// the caller's value expression h(u, j; p, q) (u float, j int, p[k], q[m])\n";
  s += "struct LvUserH {\n";
  s += "  static __device__ __forceinline__ float h(float u, int j, const float* __restrict__ p, LinQ q) {\n";
  s += "    (void)u; (void)j; (void)p; (void)q;\n";
  s += "    return (float)(" + value + ");\n  }\n";
  s += "};\n";
  s += "template <int NB>\n__global__ __launch_bounds__(256, 1) void lin_values_kernel(const LvArgs a, const LinTallModel tm, const PotLinear lin) {\n";
  s += "  __shared__ Shared<NB> sh;\n  __shared__ double wts[kP];\n  lin_values_tiles<NB, LvUserH>(a, tm, lin, sh, wts);\n}\n";
  s += "}  // namespace mjhmc\n";
  return s;
}

int resident_cus() {
  int dev = 0, cus = 0;
  (void)hipGetDevice(&dev);
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  return cus > 1 ? cus : 1;
}

}  // namespace

int linear_dim(int ndims, int nexperts) {
  const int m = ndims > nexperts ? ndims : nexperts;
  return m <= 128 ? 128 : (m <= 256 ? 256 : (m <= kPotDim ? kPotDim : 0));
}

int linear_check_args(int ndims, int nexperts, const char* energy_expr, const char* grad_expr, const char* include_dir) {
  if (!energy_expr || !grad_expr || !include_dir) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  if (ndims < 1 || nexperts < 1) return mjhmc_fail(MJHMC_ERR_INVALID, "LINEAR_EXPR needs ndims >= 1 and nexperts >= 1");
  if (!linear_dim(ndims, nexperts))
    return mjhmc_fail(MJHMC_ERR_UNSUPPORTED, "LINEAR_EXPR runs on the register-resident tile kernels: ndims and nexperts must "
                                             "be at most 512 (got " + std::to_string(ndims) + " x " + std::to_string(nexperts) +
                                             "); there is no blocked form for wider models");
  return 0;
}

int tall_pad(int ndims) { return ndims <= 128 ? 128 : (ndims <= 256 ? 256 : kPotDim); }

namespace {

const char* const kEnergyWords = "the energy expressions do not compile";

// the compiled code as e->lin's module, and its kernels by lowered name: fns in the order of the name expressions
int linear_module_load(LinearEnergy* l, const RtcCode& c, const std::vector<hipFunction_t*>& fns) {
  HIPCHK(hipModuleLoadData(&l->module, c.code.data()));
  for (size_t k = 0; k < fns.size(); ++k) HIPCHK(hipModuleGetFunction(fns[k], l->module, c.lowered[k].c_str()));
  return 0;
}

// The model on the device, float32, in the blocked layout: S slots in blocks of P, slot blk P + local holding the caller's
// expert j = expert(slot), -1 for padding (zero), and the dims in ND chunks of P (the state rows' pitch is P ND; one chunk
// for every form but the wide one):
//     W1b[blk][dc][dl][local] = W2Tb[blk][dc][local][dl] = W[j][P dc + dl]
//     (u = cb[blk] + sum_dc W1b[blk][dc]^T x_dc; dE/dx_dc += W2Tb[blk][dc]^T phi(u))
// cb = b and the per-expert rows q[m] (rows of S floats) in slot order, the shared parameters behind them.  One block, one
// chunk and the identity map are a <= 512 model in ProductOfT's own layout.  `form` words the allocation failure ("a tall").
int linear_model_upload(mjhmc_energy* e, int P, size_t S, int K, const double* W, const double* b, const double* params,
                        size_t nparams, const double* expert_params, int n_expert_rows,
                        const std::function<int64_t(int64_t)>& expert, const char* form, int ND = 1) {
  const int D = e->ep.ndims;
  LinearEnergy* l = e->lin;
  e->pot_dim = P * ND;
  const size_t M = (size_t)P * P, mat_bytes = S * P * ND * sizeof(float), nrows = (size_t)4 * S + (nparams ? nparams : 1);
  std::vector<float> w1(S * P * ND, 0.f), w2t(S * P * ND, 0.f), cb(S, 0.f), rows(nrows, 0.f);
  for (size_t slot = 0; slot < S; ++slot) {
    const int64_t j = expert((int64_t)slot);
    if (j < 0) continue;
    const size_t blk = slot / P, jl = slot % P;
    cb[slot] = (float)b[j];
    for (int d = 0; d < D; ++d) {
      const float w = (float)W[(size_t)j * D + d];
      const size_t m = (blk * ND + (size_t)(d / P)) * M, dl = (size_t)(d % P);
      w1[m + dl * P + jl] = w;
      w2t[m + jl * P + dl] = w;
    }
    for (int m = 0; m < n_expert_rows; ++m) rows[(size_t)m * S + slot] = (float)expert_params[(size_t)m * K + j];
  }
  for (size_t k = 0; k < nparams; ++k) rows[(size_t)4 * S + k] = (float)params[k];
  const void* src[3] = {w1.data(), w2t.data(), cb.data()};
  const size_t bytes[3] = {mat_bytes, mat_bytes, S * sizeof(float)};
  for (int i = 0; i < 3; ++i) {
    if (hipMalloc((void**)&e->pot[i], bytes[i]) != hipSuccess) {
      (void)hipGetLastError();
      e->pot[i] = nullptr;
      return mjhmc_fail(MJHMC_ERR_HIP, std::string(form) + " LINEAR_EXPR model of " + std::to_string(D) + " dims x " + std::to_string(K) +
                                       " experts needs " + std::to_string(2 * mat_bytes) + " bytes of device memory for its matrices (" +
                                       std::to_string(S / P * ND) + " blocks of " + std::to_string(P) + " x " + std::to_string(P) +
                                       ", twice): the allocation failed");
    }
    HIPCHK(hipMemcpy(e->pot[i], src[i], bytes[i], hipMemcpyHostToDevice));
  }
  HIPCHK(hipMalloc((void**)&l->rows, nrows * sizeof(float)));
  HIPCHK(hipMemcpy(l->rows, rows.data(), nrows * sizeof(float), hipMemcpyHostToDevice));
  l->gen.lin = PotLinear{l->rows, l->rows + (size_t)4 * S, K, (int)S};
  return 0;
}

}  // namespace

int linear_compile(const std::string& energy_expr, const std::string& grad_expr, int dim, const std::string& include_dir,
                   std::string* err, const RtcCode** out) {
  return rtc_compile_cached(linear_source(energy_expr, grad_expr), "mjhmc_linear_energy.hip", linear_kernel_names(dim / 128),
                            include_dir, kEnergyWords, out, err);
}

int linear_energy_build(mjhmc_energy* e, int nexperts, const double* W, const double* b, const char* energy_expr,
                        const char* grad_expr, const double* params, size_t nparams, const double* expert_params,
                        int n_expert_rows, const char* include_dir) {
  const int D = e->ep.ndims, K = nexperts, DIM = linear_dim(D, K);
  LinearEnergy* l = e->lin = new LinearEnergy();
  const RtcCode* c = nullptr;
  std::string err;
  const int rc = linear_compile(energy_expr, grad_expr, DIM, include_dir, &err, &c);
  if (rc) return mjhmc_fail(rc, err);
  std::vector<hipFunction_t*> fns;   // the order of linear_kernel_names
  for (int k = 0; k < 12; ++k) fns.push_back(k < 6 ? &l->gen.jump32[k / 2][k % 2] : &l->gen.jump64[(k - 6) / 2][k % 2]);
  fns.push_back(&l->gen.eval);
  fns.push_back(&l->gen.leap);
  TRY(linear_module_load(l, *c, fns));
  e->pot_rows = D > K ? D : K;
  // ProductOfT's layout (W1 = W^T: u = W1^T x + cb; W2T = W: dE/dx = W2T^T phi(u)): one block of DIM slots
  return linear_model_upload(e, DIM, (size_t)DIM, K, W, b, params, nparams, expert_params, n_expert_rows,
                             [K](int64_t slot) { return slot < K ? slot : -1; }, "a");
}

void linear_energy_free(mjhmc_energy* e) {
  if (!e->lin) return;
  if (e->lin->rows) (void)hipFree(e->lin->rows);
  if (e->lin->module) (void)hipModuleUnload(e->lin->module);
  delete e->lin;
  e->lin = nullptr;
}

// ---------------------------------------------------------------------------------------------------------------------
// Tall models: 1 <= D <= 512, 1 <= K <= 2^20.  P = the pad of D alone; the experts in
// nblk = ceil(K / P) blocks, each stored like a <= 512 model's W1 / W2T / cb, and one generated kernel that walks them
// (dense_lin_tall.hpp).  The energy keeps the kind MJHMC_E_LINEAR_EXPR and is_pot(); its samplers run the multi-pass path
// (lin_tall(), handles.hpp), whose float32 force this kernel is.
// ---------------------------------------------------------------------------------------------------------------------
int linear_tall_check_args(int ndims, int64_t nexperts, const char* energy_expr, const char* grad_expr, const char* include_dir) {
  if (!energy_expr || !grad_expr || !include_dir) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  if (ndims < 1 || nexperts < 1) return mjhmc_fail(MJHMC_ERR_INVALID, "LINEAR_EXPR needs ndims >= 1 and nexperts >= 1");
  if (ndims > kPotDim)
    return mjhmc_fail(MJHMC_ERR_UNSUPPORTED, "a tall LINEAR_EXPR model takes at most 512 dims (got " + std::to_string(ndims) +
                                             "): its expert blocks are the tile kernels' 512 x 512 at the most");
  if (nexperts > kLinTallMaxExperts)
    return mjhmc_fail(MJHMC_ERR_UNSUPPORTED, "a tall LINEAR_EXPR model takes at most 1048576 (2^20) experts (got " +
                                             std::to_string(nexperts) + ")");
  return 0;
}

int linear_tall_compile(const std::string& energy_expr, const std::string& grad_expr, int dim, const std::string& include_dir,
                        std::string* err, const RtcCode** out) {
  return rtc_compile_cached(linear_tall_source(energy_expr, grad_expr), "mjhmc_linear_tall.hip",
                            {"mjhmc::lin_tall_eval_kernel<" + std::to_string(dim / 128) + ">"}, include_dir, kEnergyWords, out, err);
}

int linear_tall_energy_build(mjhmc_energy* e, int64_t nexperts, const double* W, const double* b, const char* energy_expr,
                             const char* grad_expr, const double* params, size_t nparams, const double* expert_params,
                             int n_expert_rows, const char* include_dir) {
  const int D = e->ep.ndims, K = (int)nexperts, P = tall_pad(D), nblk = (K + P - 1) / P;
  LinearEnergy* l = e->lin = new LinearEnergy();
  const RtcCode* c = nullptr;
  std::string err;
  const int rc = linear_tall_compile(energy_expr, grad_expr, P, include_dir, &err, &c);
  if (rc) return mjhmc_fail(rc, err);
  TRY(linear_module_load(l, *c, {&l->tall}));
  l->tall_nblk = nblk;
  l->tall_K = K;
  e->pot_rows = D;
  return linear_model_upload(e, P, (size_t)nblk * P, K, W, b, params, nparams, expert_params, n_expert_rows,
                             [K](int64_t slot) { return slot < K ? slot : -1; }, "a tall");
}

void lin_tall_eval(const mjhmc_energy* e, const float* X32, float* G32, float* E32, int64_t rows_pad, int64_t nrows, hipStream_t st) {
  PotEvalArgs a;
  a.X = X32;
  a.G = G32;
  a.E = E32;
  a.EV = nullptr;
  a.V = nullptr;
  a.V_gen = nullptr;
  a.N = nrows;
  a.ntiles = rows_pad / 32;
  a.first_pid = 0;
  a.D = e->ep.ndims;
  a.key = RngKey{0u, 0u, 0u, 0u};
  const PotLinear lin = e->lin->gen.lin;
  const unsigned grid = (unsigned)std::min<int64_t>(a.ntiles, resident_cus());
  // lin_tall_eval_kernel or lin_grouped_eval_kernel (dense_lin_grouped.hpp): the same arguments around the kernel's own model
  const LinTallModel tm{e->pot[0], e->pot[1], e->pot[2], e->lin->tall_nblk, e->ep.ndims, e->lin->tall_K};
  const LinGroupedModel gm{e->pot[0], e->pot[1], e->pot[2], e->lin->grp_nbg, e->lin->grp_nbp, e->ep.ndims, e->lin->tall_K, e->lin->grp_G};
  void* params[] = {(void*)&a, e->lin->grouped() ? (void*)&gm : (void*)&tm, (void*)&lin};
  (void)hipModuleLaunchKernel(e->lin->tall, grid, 1, 1, 256, 1, 1, 0, st, params, nullptr);
}

// ---------------------------------------------------------------------------------------------------------------------
// Wide models: 1 <= D <= 4096, 1 <= K <= 2^20.  Always blocks of 512: the experts in
// nblk = ceil(K / 512) blocks, the dims in ND = ceil(D / 512) chunks, and one generated kernel that walks them
// (dense_lin_wide.hpp).  The energy keeps the kind MJHMC_E_LINEAR_EXPR and is_pot(); its samplers run the multi-pass path
// (lin_wide(), handles.hpp) on rows of pitch 512 ND, whose float32 force this kernel is.
// ---------------------------------------------------------------------------------------------------------------------
int linear_wide_check_args(int ndims, int64_t nexperts, const char* energy_expr, const char* grad_expr, const char* include_dir) {
  if (!energy_expr || !grad_expr || !include_dir) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  if (ndims < 1 || nexperts < 1) return mjhmc_fail(MJHMC_ERR_INVALID, "LINEAR_EXPR needs ndims >= 1 and nexperts >= 1");
  if (ndims > kLinWideMaxDims)
    return mjhmc_fail(MJHMC_ERR_UNSUPPORTED, "a wide LINEAR_EXPR model takes at most 4096 dims (got " + std::to_string(ndims) +
                                             "): 8 chunks of the tile kernels' 512");
  if (nexperts > kLinTallMaxExperts)
    return mjhmc_fail(MJHMC_ERR_UNSUPPORTED, "a wide LINEAR_EXPR model takes at most 1048576 (2^20) experts (got " +
                                             std::to_string(nexperts) + ")");
  return 0;
}

int linear_wide_compile(const std::string& energy_expr, const std::string& grad_expr, const std::string& include_dir,
                        std::string* err, const RtcCode** out) {
  return rtc_compile_cached(linear_wide_source(energy_expr, grad_expr), "mjhmc_linear_wide.hip", {"mjhmc::lin_wide_eval_kernel"},
                            include_dir, kEnergyWords, out, err);
}

int linear_wide_energy_build(mjhmc_energy* e, int64_t nexperts, const double* W, const double* b, const char* energy_expr,
                             const char* grad_expr, const double* params, size_t nparams, const double* expert_params,
                             int n_expert_rows, const char* include_dir) {
  const int D = e->ep.ndims, K = (int)nexperts, P = kPotDim, nblk = (K + P - 1) / P, ND = (D + P - 1) / P;
  LinearEnergy* l = e->lin = new LinearEnergy();
  const RtcCode* c = nullptr;
  std::string err;
  const int rc = linear_wide_compile(energy_expr, grad_expr, include_dir, &err, &c);
  if (rc) return mjhmc_fail(rc, err);
  TRY(linear_module_load(l, *c, {&l->wide}));
  l->tall_nblk = nblk;
  l->tall_K = K;
  l->wide_nd = ND;
  e->pot_rows = D;
  return linear_model_upload(e, P, (size_t)nblk * P, K, W, b, params, nparams, expert_params, n_expert_rows,
                             [K](int64_t slot) { return slot < K ? slot : -1; }, "a wide", ND);
}

void lin_wide_eval(const mjhmc_energy* e, const float* X32, float* G32, float* E32, int64_t rows_pad, int64_t nrows, hipStream_t st) {
  PotEvalArgs a;
  a.X = X32;
  a.G = G32;
  a.E = E32;
  a.EV = nullptr;
  a.V = nullptr;
  a.V_gen = nullptr;
  a.N = nrows;
  a.ntiles = rows_pad / 32;
  a.first_pid = 0;
  a.D = e->ep.ndims;
  a.key = RngKey{0u, 0u, 0u, 0u};
  const PotLinear lin = e->lin->gen.lin;
  const unsigned grid = (unsigned)std::min<int64_t>(a.ntiles, resident_cus());
  const LinWideModel wm{e->pot[0], e->pot[1], e->pot[2], e->lin->tall_nblk, e->lin->wide_nd, e->ep.ndims, e->lin->tall_K};
  void* params[] = {(void*)&a, (void*)&wm, (void*)&lin};
  (void)hipModuleLaunchKernel(e->lin->wide, grid, 1, 1, 256, 1, 1, 0, st, params, nullptr);
}

// ---------------------------------------------------------------------------------------------------------------------
// Grouped models: the tall form plus sum_g LSE_c u_{gC+c} over the first G groups of C experts.
// The layout: blocks of P = the pad of D; a lane type (w, h) of a block holds 16 NB slots, slot s = NB q + r at local
// column 32 NB w + NB acc_row(q, h) + r, and takes Gl = floor(16 NB / C) whole groups, group gl in slots [C gl, C gl + C);
// a block takes the 8 Gl groups (8 blk + 2 w + h) Gl + gl.  The plain experts follow in blocks of their own, in caller
// order.  The energy is lin_tall() (the multi-pass path, lin_tall_eval above) with its own kernel.
// ---------------------------------------------------------------------------------------------------------------------
namespace {

std::string linear_grouped_source(const std::string& energy_expr, const std::string& grad_expr, int group_size) {
  std::string s;
  s += "#include \"dense_lin_grouped.hpp\"\n";
  s += "namespace mjhmc {\n";
  s += user_functor_source(energy_expr, grad_expr);
  s += "constexpr int kGroupSize = " + std::to_string(group_size) + ";   // members per group: the register loops are unrolled over it\n";
  s += "template <int NB>\n__global__ __launch_bounds__(256, 1) void lin_grouped_eval_kernel(const PotEvalArgs a, const LinGroupedModel gm, const PotLinear lin) {\n";
  s += "  __shared__ Shared<NB> sh;\n  lin_grouped_eval_tiles<NB, kGroupSize, LinUserF>(a, gm, lin, sh);\n}\n";
  s += "}  // namespace mjhmc\n";
  return s;
}

}  // namespace

LinGroupedLayout linear_grouped_layout(int ndims, int64_t nexperts, int group_size, int64_t n_groups) {
  LinGroupedLayout L;
  L.P = tall_pad(ndims);
  L.Gl = 16 * (L.P / 128) / group_size;
  const int64_t per_block = 8 * L.Gl, plain = nexperts - n_groups * group_size;
  L.nbg = (int)((n_groups + per_block - 1) / per_block);
  L.nbp = (int)((plain + L.P - 1) / L.P);
  L.nslots = (int64_t)(L.nbg + L.nbp) * L.P;
  return L;
}

int64_t linear_grouped_slot_expert(const LinGroupedLayout& L, int64_t nexperts, int group_size, int64_t n_groups, int64_t slot) {
  const int NB = L.P / 128;
  const int64_t blk = slot / L.P, local = slot % L.P;
  if (blk >= L.nbg) {
    const int64_t j = n_groups * group_size + (blk - L.nbg) * L.P + local;
    return j < nexperts ? j : -1;
  }
  const int w = (int)local / (32 * NB), row = (int)local % (32 * NB) / NB, r = (int)local % NB;
  const int h = (row >> 2) & 1, q = (row & 3) + 4 * (row >> 3);   // row = acc_row(q, h) = (q & 3) + 8 (q >> 2) + 4 h
  const int s = NB * q + r, gl = s / group_size, c = s % group_size;
  if (gl >= L.Gl) return -1;
  const int64_t g = (8 * blk + 2 * w + h) * L.Gl + gl;
  return g < n_groups ? g * group_size + c : -1;
}

int linear_grouped_check_args(int ndims, int64_t nexperts, int group_size, int64_t n_groups, const char* energy_expr,
                              const char* grad_expr, const char* include_dir) {
  if (!energy_expr || !grad_expr || !include_dir) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  if (ndims < 1 || nexperts < 1) return mjhmc_fail(MJHMC_ERR_INVALID, "LINEAR_EXPR needs ndims >= 1 and nexperts >= 1");
  if (group_size < 2)
    return mjhmc_fail(MJHMC_ERR_INVALID, "a grouped LINEAR_EXPR model needs group_size >= 2 (got " + std::to_string(group_size) + ")");
  if (n_groups < 1)
    return mjhmc_fail(MJHMC_ERR_INVALID, "a grouped LINEAR_EXPR model needs n_groups >= 1 (got " + std::to_string(n_groups) + ")");
  if (group_size > kLinGroupMax)
    return mjhmc_fail(MJHMC_ERR_UNSUPPORTED, "a grouped LINEAR_EXPR model takes groups of at most 16 experts (got group_size = " +
                                             std::to_string(group_size) + "): a group lies in one lane's 16 registers per block");
  if (nexperts > kLinTallMaxExperts || n_groups > kLinTallMaxExperts || n_groups * group_size > nexperts)
    return nexperts > kLinTallMaxExperts || n_groups > kLinTallMaxExperts
               ? mjhmc_fail(MJHMC_ERR_UNSUPPORTED, "a grouped LINEAR_EXPR model takes at most 1048576 (2^20) slots (got " +
                                                       std::to_string(nexperts) + " experts, " + std::to_string(n_groups) + " groups)")
               : mjhmc_fail(MJHMC_ERR_INVALID, "the " + std::to_string(n_groups) + " groups of " + std::to_string(group_size) +
                                                   " are more than the model's " + std::to_string(nexperts) + " experts");
  if (ndims > kPotDim)
    return mjhmc_fail(MJHMC_ERR_UNSUPPORTED, "a grouped LINEAR_EXPR model takes at most 512 dims (got " + std::to_string(ndims) +
                                             "): its expert blocks are the tile kernels' 512 x 512 at the most");
  const LinGroupedLayout L = linear_grouped_layout(ndims, nexperts, group_size, n_groups);
  if (L.nslots > kLinTallMaxExperts)
    return mjhmc_fail(MJHMC_ERR_UNSUPPORTED, "a grouped LINEAR_EXPR model takes at most 1048576 (2^20) slots (these " +
                                             std::to_string(n_groups) + " groups of " + std::to_string(group_size) + " and " +
                                             std::to_string(nexperts - n_groups * group_size) + " plain experts need " +
                                             std::to_string(L.nslots) + " in blocks of " + std::to_string(L.P) + ")");
  return 0;
}

// The per-group statistics pass of a grouped model (dense_lin_group_pointwise.hpp): the caller's M
// value expressions as a functor -- they see lse, sm and c beside what a pointwise value sees -- with the group size and
// the values' kinds as constants of the source, and the one kernel around it
namespace {

std::string linear_group_pointwise_source(const std::vector<std::string>& values, int group_size, unsigned member_mask) {
  std::string s;
  s += "#include \"dense_lin_group_pointwise.hpp\"\n";
  s += "namespace mjhmc {\n";
  s += "constexpr int kGroupSize = " + std::to_string(group_size) + ";   // members per group: the register loops are unrolled over it\n";
  s += "// the caller's value expressions h_m(u, j; p, q; lse, sm, c) (u, lse, sm float; j, c int; p[k], q[m])\n";
  s += "struct GpUserH {\n";
  s += "  static constexpr int kM = " + std::to_string(values.size()) + ";\n";
  s += "  static constexpr unsigned kMemberMask = " + std::to_string(member_mask) + "u;   // bit m: value m is per member\n";
  s += "  template <int MI>\n";
  s += "  static __device__ __forceinline__ float h(float u, int j, const float* __restrict__ p, LinQ q, float lse, float sm, int c) {\n";
  s += "    (void)u; (void)j; (void)p; (void)q; (void)lse; (void)sm; (void)c;\n";
  for (size_t m = 0; m < values.size(); ++m)
    s += std::string(m ? "    else " : "    ") + "if constexpr (MI == " + std::to_string(m) + ") return (float)(" + values[m] + ");\n";
  s += "    else return 0.f;\n  }\n";
  s += "};\n";
  s += "template <int NB>\n__global__ __launch_bounds__(256, 1) void lin_group_pointwise_kernel(const PwArgs a, const LinGroupedModel gm, const PotLinear lin) {\n";
  s += "  __shared__ Shared<NB> sh;\n  __shared__ double wts[kP];\n  lin_group_pointwise_items<NB, kGroupSize, GpUserH>(a, gm, lin, sh, wts);\n}\n";
  s += "}  // namespace mjhmc\n";
  return s;
}

}  // namespace

int linear_group_pointwise_compile(const std::vector<std::string>& values, int dim, int group_size, unsigned member_mask,
                                   const std::string& include_dir, std::string* err, const RtcCode** out) {
  return rtc_compile_cached(linear_group_pointwise_source(values, group_size, member_mask), "mjhmc_linear_group_pointwise.hip",
                            {"mjhmc::lin_group_pointwise_kernel<" + std::to_string(dim / 128) + ">"}, include_dir,
                            "the value expressions do not compile", out, err);
}

int linear_grouped_compile(const std::string& energy_expr, const std::string& grad_expr, int dim, int group_size,
                           const std::string& include_dir, std::string* err, const RtcCode** out) {
  return rtc_compile_cached(linear_grouped_source(energy_expr, grad_expr, group_size), "mjhmc_linear_grouped.hip",
                            {"mjhmc::lin_grouped_eval_kernel<" + std::to_string(dim / 128) + ">"}, include_dir, kEnergyWords, out, err);
}

int linear_grouped_energy_build(mjhmc_energy* e, int64_t nexperts, const double* W, const double* b, int group_size,
                                int64_t n_groups, const char* energy_expr, const char* grad_expr, const double* params,
                                size_t nparams, const double* expert_params, int n_expert_rows, const char* include_dir) {
  const int D = e->ep.ndims, K = (int)nexperts;
  const LinGroupedLayout L = linear_grouped_layout(D, nexperts, group_size, n_groups);
  LinearEnergy* l = e->lin = new LinearEnergy();
  const RtcCode* c = nullptr;
  std::string err;
  const int rc = linear_grouped_compile(energy_expr, grad_expr, L.P, group_size, include_dir, &err, &c);
  if (rc) return mjhmc_fail(rc, err);
  TRY(linear_module_load(l, *c, {&l->tall}));
  l->tall_nblk = L.nbg + L.nbp;
  l->tall_K = K;
  l->grp_C = group_size;
  l->grp_G = (int)n_groups;
  l->grp_nbg = L.nbg;
  l->grp_nbp = L.nbp;
  e->pot_rows = D;
  return linear_model_upload(e, L.P, (size_t)L.nslots, K, W, b, params, nparams, expert_params, n_expert_rows,
                             [&](int64_t slot) { return linear_grouped_slot_expert(L, nexperts, group_size, n_groups, slot); },
                             "a grouped");
}

// ---------------------------------------------------------------------------------------------------------------------
// The per-expert statistics pass of a linear model, square or tall (dense_lin_pointwise.hpp, pointwise.hip)
// ---------------------------------------------------------------------------------------------------------------------
int linear_pointwise_dim(int ndims, int64_t nexperts) {
  return nexperts > kPotDim ? tall_pad(ndims) : linear_dim(ndims, (int)nexperts);
}

int linear_pointwise_compile(const std::vector<std::string>& values, int dim, const std::string& include_dir,
                             std::string* err, const RtcCode** out) {
  return rtc_compile_cached(linear_pointwise_source(values), "mjhmc_linear_pointwise.hip",
                            {"mjhmc::lin_pointwise_kernel<" + std::to_string(dim / 128) + ">"}, include_dir,
                            "the value expressions do not compile", out, err);
}

// ---------------------------------------------------------------------------------------------------------------------
// The values of one block of experts, stored: the first half of the influence pass (dense_lin_values.hpp, influence.hip)
// ---------------------------------------------------------------------------------------------------------------------
int linear_values_compile(const std::string& value, int dim, const std::string& include_dir, std::string* err,
                          const RtcCode** out) {
  return rtc_compile_cached(linear_values_source(value), "mjhmc_linear_values.hip",
                            {"mjhmc::lin_values_kernel<" + std::to_string(dim / 128) + ">"}, include_dir,
                            "the value expression does not compile", out, err);
}
