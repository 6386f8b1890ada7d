// Centred linear lag sums per dimension along the time axis of a ring (lagcov.hip): what the integrated autocorrelation
// time and the effective sample size of every coordinate are made of (mjhmc/misc/autocor.py:177-211 computes the pooled,
// uncentred lag products on the host).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "autocor.hpp"   // RingView

constexpr int kLagcovMaxLag = 256;

// n consecutive slots of `r` (r.base = the first), shift: D float64 on the HOST or nullptr (zeros), 0 <= K <= min(n - 1, 256):
//   u[t][p][d] = (double)x[t][p][d] - shift[d]                              one rounded subtraction
//   A[k][d]    = sum_{p < N} sum_{t = 0}^{n - 1 - k} u[t][p][d] u[t + k][p][d]   k = 0 .. K   -> A_host[(K + 1) * D], C order
//   S[d]       = sum_{p < N} sum_{t < n} u[t][p][d]                                           -> S_host[D], nullable
// Linear (not circular), unnormalised.  Rows p >= N and columns d >= D are not read.  No floating-point atomics: the order
// of addition is a function of (N, D, n, K) alone.  Synchronises `st`.
int lagcov_from_ring(hipStream_t st, const RingView& r, int n, int K, const double* shift, double* A_host, double* S_host,
                     std::string& err);
// the same for a host array [n_dims][n_batch][n_samples] (C order), re-tiled on the device into a temporary time-major
// float64 view whose padding rows and columns hold NaN
int lagcov_from_host(hipStream_t st, const double* samples, int D, int64_t N, int n, int K, const double* shift, double* A_host,
                     double* S_host, std::string& err);
// the argument checks the entry points share: n, K and the shift (D host doubles or nullptr)
int lagcov_check(int n, int K, const double* shift, int D, std::string& err);
