// Weighted sufficient statistics of blocks of ring slots (estimators.hip): per-dimension first and second moments and
// the dense covariance, dwell-time weighted for the jump samplers.  The sums stay on the device between calls.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "autocor.hpp"   // RingView

// launch geometry of the two passes for one ring shape; a function of (N, D, pitch, dtype) alone, so that two runs on
// one device fold the same partial sums in the same order
struct EstimatorPlan {
  // moment pass: a workgroup is CW column lanes (16 bytes of a row each) x 256 / CW row lanes
  int vec = 2, cw = 1, log_cw = 0, gx = 1, gy = 1;
  size_t moment_partial_elems = 0;   // [gx][2][pitch] sums + [gx] weights
  // covariance pass: 64 x 64 output blocks (4 x 4 MFMA tiles) with I <= J, the contraction split over `splits` waves
  int nb = 0, pairs = 0, splits = 0;
  size_t cov_partial_elems = 0;      // [pairs][splits][16 tiles][4 registers][64 lanes]
};

constexpr int kEstimatorMaxCovDims = 512;

EstimatorPlan estimator_plan(const RingView& r, bool want_cov);

// acc[0] += W, acc[1 + d] += S1_d, acc[1 + D + d] += S2_d over n slots of `r` (r.base = the first slot), weights
// w[k * Npad + p] (device; nullptr = 1), shift c[D] (device).  A non-finite weight sets *bad and leaves acc as it was.
int estimator_moments(hipStream_t st, const RingView& r, int n, const double* w, const double* c,
                      const EstimatorPlan& plan, double* partial, double* acc, int* bad, std::string& err);
// C[d * D + e] += sum w (x_d - c_d)(x_e - c_e), both triangles (bit-identical mirror images); D <= kEstimatorMaxCovDims.
// Reads *bad (set by estimator_moments on the same block, same stream) and adds nothing when it is set.
int estimator_cov(hipStream_t st, const RingView& r, int n, const double* w, const double* c, const EstimatorPlan& plan,
                  double* partial, double* C, const int* bad, std::string& err);
