// Linear-model energies E(x) = sum_{j<K} f(u_j, j), u = W x + b (MJHMC_E_LINEAR_EXPR, linear_energy.hip): the ProductOfT
// tile kernels compiled with hipRTC around a caller's f and f'.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "dense_pot.hpp"

struct mjhmc_energy;
struct RtcCode;   // user_expr.hpp: a cached hipRTC compile, {code, lowered names}

struct LinearEnergy {
  hipModule_t module = nullptr;
  mjhmc::PotGenerated gen;   // the module's kernels and the experts' device arguments
  float* rows = nullptr;     // [4][dim] per-expert rows, then the shared parameters (gen.lin.q, gen.lin.p)
  // a tall model (more than 512 experts): its one kernel, lin_tall_eval_kernel, and its block count; the
  // tile kernels of `gen` are then absent (gen.lin alone is used) and the sampler runs the multi-pass path
  hipFunction_t tall = nullptr;
  int tall_nblk = 0, tall_K = 0;
  // a grouped model: `tall` is lin_grouped_eval_kernel, the blocks are grp_nbg grouped ones and then
  // grp_nbp plain ones (tall_nblk in all), grp_C members per group (0: not grouped), grp_G groups
  int grp_C = 0, grp_G = 0, grp_nbg = 0, grp_nbp = 0;
  bool grouped() const { return grp_C != 0; }
  // a wide model (more than 512 dims allowed): its one kernel, lin_wide_eval_kernel, over tall_nblk blocks
  // of 512 experts x wide_nd chunks of 512 dims (tall_K experts); `tall` and the tile kernels of `gen` are then absent
  hipFunction_t wide = nullptr;
  int wide_nd = 0;
};

constexpr int64_t kLinTallMaxExperts = (int64_t)1 << 20;

// the padded dimension of a (D, K) model: 128, 256 or 512; 0 beyond the tile kernels
int linear_dim(int ndims, int nexperts);
// argument checks shared by creation and the device-free check (records the message, returns the error code)
int linear_check_args(int ndims, int nexperts, const char* energy_expr, const char* grad_expr, const char* include_dir);
// the hipRTC compile of the 14 kernels for one padded dimension (every compile here: rtc_compile_cached, user_expr.hpp)
int linear_compile(const std::string& energy_expr, const std::string& grad_expr, int dim, const std::string& include_dir,
                   std::string* err, const RtcCode** out);
int linear_energy_build(mjhmc_energy* e, int nexperts, const double* W, const double* b, const char* energy_expr,
                        const char* grad_expr, const double* params, size_t nparams, const double* expert_params,
                        int n_expert_rows, const char* include_dir);
void linear_energy_free(mjhmc_energy* e);

// Tall models: 1 <= ndims <= 512, 1 <= nexperts <= 2^20 (kLinTallMaxExperts), experts in blocks of the pad of ndims
int tall_pad(int ndims);   // 128, 256 or 512
int linear_tall_check_args(int ndims, int64_t nexperts, const char* energy_expr, const char* grad_expr, const char* include_dir);
// the hipRTC compile of lin_tall_eval_kernel<dim / 128>: its own small source, its own cache key
int linear_tall_compile(const std::string& energy_expr, const std::string& grad_expr, int dim, const std::string& include_dir,
                        std::string* err, const RtcCode** out);
int linear_tall_energy_build(mjhmc_energy* e, int64_t nexperts, const double* W, const double* b, const char* energy_expr,
                             const char* grad_expr, const double* params, size_t nparams, const double* expert_params,
                             int n_expert_rows, const char* include_dir);
// E (or none) and dE/dX (or none) of float32 rows X32 [rows_pad][pad of ndims] (rows_pad a multiple of 32) on `st`
void lin_tall_eval(const mjhmc_energy* e, const float* X32, float* G32, float* E32, int64_t rows_pad, int64_t nrows, hipStream_t st);

// Wide models: 1 <= ndims <= 4096 (kLinWideMaxDims), 1 <= nexperts <= 2^20, experts in blocks of 512, dims
// in chunks of 512 (ndims <= 512: one chunk)
constexpr int kLinWideMaxDims = 4096;
int linear_wide_check_args(int ndims, int64_t nexperts, const char* energy_expr, const char* grad_expr, const char* include_dir);
// the hipRTC compile of lin_wide_eval_kernel: its own small source, its own cache key
int linear_wide_compile(const std::string& energy_expr, const std::string& grad_expr, const std::string& include_dir,
                        std::string* err, const RtcCode** out);
int linear_wide_energy_build(mjhmc_energy* e, int64_t nexperts, const double* W, const double* b, const char* energy_expr,
                             const char* grad_expr, const double* params, size_t nparams, const double* expert_params,
                             int n_expert_rows, const char* include_dir);
// E (or none) and dE/dX (or none) of float32 rows X32 [rows_pad][e->pot_dim] (rows_pad a multiple of 32) on `st`; G32 needs
// no zeroing
void lin_wide_eval(const mjhmc_energy* e, const float* X32, float* G32, float* E32, int64_t rows_pad, int64_t nrows, hipStream_t st);

// Grouped models: the first n_groups * group_size experts are groups under a log-sum-exp, stored so that
// a group lies in one lane's registers (dense_lin_grouped.hpp); 2 <= group_size <= 16, at most 2^20 slots
constexpr int kLinGroupMax = 16;
struct LinGroupedLayout {
  int P, Gl, nbg, nbp;   // the pad of ndims, groups per lane type, grouped blocks, plain blocks
  int64_t nslots;        // (nbg + nbp) P
};
LinGroupedLayout linear_grouped_layout(int ndims, int64_t nexperts, int group_size, int64_t n_groups);
// the caller's expert of a slot, -1 for padding
int64_t linear_grouped_slot_expert(const LinGroupedLayout& L, int64_t nexperts, int group_size, int64_t n_groups, int64_t slot);
int linear_grouped_check_args(int ndims, int64_t nexperts, int group_size, int64_t n_groups, const char* energy_expr,
                              const char* grad_expr, const char* include_dir);
// the hipRTC compile of lin_grouped_eval_kernel<dim / 128> with the group size a constant of the source
int linear_grouped_compile(const std::string& energy_expr, const std::string& grad_expr, int dim, int group_size,
                           const std::string& include_dir, std::string* err, const RtcCode** out);
int linear_grouped_energy_build(mjhmc_energy* e, int64_t nexperts, const double* W, const double* b, int group_size,
                                int64_t n_groups, const char* energy_expr, const char* grad_expr, const double* params,
                                size_t nparams, const double* expert_params, int n_expert_rows, const char* include_dir);

// The per-group statistics pass of a grouped model (dense_lin_group_pointwise.hpp, pointwise.hip): the hipRTC compile of
// lin_group_pointwise_kernel<dim / 128> around 1 .. 4 value expressions, dim = linear_grouped_layout's P; the group size and
// the values' kinds (bit m of member_mask: value m is per member) are constants of the source and so of the cache key
int linear_group_pointwise_compile(const std::vector<std::string>& values, int dim, int group_size, unsigned member_mask,
                                   const std::string& include_dir, std::string* err, const RtcCode** out);

// The per-expert statistics pass (dense_lin_pointwise.hpp, pointwise.hip): the padded dimension of the blocks a model of
// (ndims, nexperts) is stored in (the tall layout beyond 512 experts, the square one otherwise; 0: no such model), and the
// hipRTC compile of lin_pointwise_kernel<dim / 128> around 1 .. 4 value expressions (which of them keep a log-mean-exp is
// a launch argument) -- its own source and cache key: creating an energy compiles none of it
int linear_pointwise_dim(int ndims, int64_t nexperts);
int linear_pointwise_compile(const std::vector<std::string>& values, int dim, const std::string& include_dir,
                             std::string* err, const RtcCode** out);

// The values of one block of experts, stored (dense_lin_values.hpp, influence.hip): the hipRTC compile of
// lin_values_kernel<dim / 128> around ONE value expression, dim from linear_pointwise_dim -- its own source and cache key
int linear_values_compile(const std::string& value, int dim, const std::string& include_dir, std::string* err,
                          const RtcCode** out);
