// Linear-model energies E(x) = sum_{j<K} f(u_j, j), u = W x + b (MJHMC_E_LINEAR_EXPR, linear_energy.hip): the ProductOfT
// tile kernels compiled with hipRTC around a caller's f and f'.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "dense_pot.hpp"

struct mjhmc_energy;

struct LinearEnergy {
  hipModule_t module = nullptr;
  mjhmc::PotGenerated gen;   // the module's kernels and the experts' device arguments
  float* rows = nullptr;     // [4][dim] per-expert rows, then the shared parameters (gen.lin.q, gen.lin.p)
};

// the padded dimension of a (D, K) model: 128, 256 or 512; 0 beyond the tile kernels
int linear_dim(int ndims, int nexperts);
// argument checks shared by creation and the device-free check (records the message, returns the error code)
int linear_check_args(int ndims, int nexperts, const char* energy_expr, const char* grad_expr, const char* include_dir);
// the hipRTC compile of the 14 kernels for one padded dimension; code objects are cached per process by source
int linear_compile(const std::string& energy_expr, const std::string& grad_expr, int dim, const std::string& include_dir,
                   std::string* err, const std::vector<char>** code, const std::vector<std::string>** lowered);
int linear_energy_build(mjhmc_energy* e, int nexperts, const double* W, const double* b, const char* energy_expr,
                        const char* grad_expr, const double* params, size_t nparams, const double* expert_params,
                        int n_expert_rows, const char* include_dir);
void linear_energy_free(mjhmc_energy* e);
