// Per-chain weighted sums of blocks of ring slots (chainstats.hip): for every particle (= chain) its own sum of weights
// and first and second moments per dimension, kept on the device between calls, and their fold over the chains into the
// sums R-hat and the multi-chain effective sample size are made of.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "autocor.hpp"   // RingView

// launch geometry of the fold for one ring shape; a function of (N, pitch) alone, so that two runs on one device add the
// same partial sums in the same order
struct ChainFoldPlan {
  // a workgroup is cw column lanes (one accumulator column each) x rw = 256 / cw row lanes; gy workgroups cover a row,
  // gx workgroups share the chains: row lane ry of workgroup bx takes chains bx * rw + ry, + gx * rw, ...
  int cw = 1, log_cw = 0, gx = 1, gy = 1;
  size_t partial_elems = 0;   // [gx][3][pitch] sums of m, m^2, v + [gx] sums of a0
  // additions a term passes through on its way into a folded sum: the row lane's own chains, the row lanes of the
  // workgroup, the workgroups of one finish lane, the 16 finish lanes (what the tests' error bound is made of)
  int64_t depth(int64_t N) const {
    const int64_t rw = 256 >> log_cw;
    return (N + (int64_t)gx * rw - 1) / ((int64_t)gx * rw) + rw + (gx + 15) / 16 + 16;
  }
};

ChainFoldPlan chain_fold_plan(const RingView& r);

// a0[p] += sum_k w, a1[p * pitch + d] += sum_k w (x_d - c_d), a2[...] += sum_k w (x_d - c_d)^2 over the n slots of `r`
// (r.base = the first slot), for every chain p < N; weights w[k * Npad + p] (device; nullptr = 1), shift c[D] (device).
// With weights, a check of the block's n * N weights runs first: a non-finite one sets *bad and the sums stay as they were.
int chain_accumulate(hipStream_t st, const RingView& r, int n, const double* w, const double* c, double* a0, double* a1,
                     double* a2, int* bad, std::string& err);
// out[0] = sum_p a0_p, out[1 + d] = sum_p m_pd, out[1 + D + d] = sum_p m_pd^2, out[1 + 2 D + d] = sum_p v_pd  (device)
int chain_fold(hipStream_t st, const RingView& r, const ChainFoldPlan& plan, const double* a0, const double* a1,
               const double* a2, double* partial, double* out, std::string& err);
