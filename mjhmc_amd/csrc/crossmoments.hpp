// Weighted cross moments of dE/dX with the rows of a ring (crossmoments.hip): what the first-order zero-variance control
// variates are made of.  For ONE recorded slot, its gradient matrix G[p][d] (d < D; float64 or float32, as the energy
// family writes it), the matching slot B[p][k] of a ring (k < K; the sample ring in its own type, or a float64 derived
// ring), weights w_p and a shift cb[K]:
//     Cgb[d][k] += sum_{p < N} w_p * G[p][d] * (B[p][k] - cb[k])
// every element widened to float64 exactly (ring_rows.hpp), every product and sum float64, no contraction
// (-ffp-contract=off), no floating-point atomics.  The gradient is taken about 0: E_p[dE/dX] = 0 is its known mean.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "autocor.hpp"   // RingView

// launch geometry of the cross pass; a function of (N, D, K) alone, so that two runs fold the same partial sums in the
// same order
struct CrossPlan {
  int nbg = 0, nbk = 0;        // 64-wide blocks over the D gradient columns and the K ring columns
  int blocks = 0, splits = 0;  // nbg * nbk output blocks (the full rectangle), the contraction split over `splits` waves
  size_t partial_elems = 0;    // [blocks][splits][16 tiles][4 registers][64 lanes]
};

CrossPlan cross_plan(int64_t N, int D, int K);

// Cgb[d * K + k] += sum_p w_p g_pd (b_pk - cb_k) over the one slot `g` (r.base = the gradient matrix, D columns) and the
// one slot `b` (K columns) of the same particles; w[p] (device; nullptr = 1), cb[K] (device).  D, K <=
// kEstimatorMaxCovDims.  Reads *bad on the same stream and adds nothing when it is set.
int cross_cov(hipStream_t st, const RingView& g, const RingView& b, const double* w, const double* cb, const CrossPlan& plan,
              double* partial, double* Cgb, const int* bad, std::string& err);
