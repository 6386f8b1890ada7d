// Argument blocks of the ProductOfT MFMA kernels (dense_pot.hip).
#pragma once
#ifndef __HIPCC_RTC__  // hipRTC pre-includes the device runtime (linear_energy.hip)
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#include "jump_math.hpp"
#include "jump_process.hpp"  // decide<double> / decide_ct<double> of the float64-state kernels
#include "lane_group.hpp"
#include "philox.hpp"
#include "sampler_args.hpp"  // Control, the dense argument blocks

namespace mjhmc {

constexpr int kPotDim = 512;  // largest ndims == nbasis of the register-resident tile kernels (rows are zero padded to 128, 256 or 512);
                              // beyond it: blocked evaluation on the multi-pass path (PotBigModel, pot_big_eval)

// device-resident model, float32, padded to 512 x 512
struct PotModel {
  const float* W1;     // [d][j] = W[d][j] / nu_j              (first GEMM:  u = W1^T x + cb)
  const float* W2T;    // [j][d] = W[d][j] * (nu_j + 1) / nu_j  (second GEMM: dE/dx = W2T^T phi(u))
  const float* cb;     // [j]    = b_j / nu_j
  const float* alpha;  // [j]    = (nu_j + 1) / 2   (0 for padded experts)
  int dim;             // padded dimension: 128, 256 or 512
  int ndims;           // true ndims == nbasis (rows at or beyond it are zero padding)
};

// the tile kernels' argument blocks (sampler_args.hpp: DenseJumpArgs): float32 state rows, and the reference's
// arithmetic (dense_pot64.hip) with float64 state rows around the float32 force
using PotJumpArgs = DenseJumpArgs<float, float, true>;
using Pot64JumpArgs = DenseJumpArgs<double, double, true>;
using PotLeapArgs = DenseLeapArgs<float, true>;
using PotEvalArgs = DenseEvalArgs<float, true>;

// The experts of a linear-model energy (MJHMC_E_LINEAR_EXPR: E = sum_j f(u_j, j), u = W x + b; dense_pot_kernels.hpp
// LinearExperts), the third argument of its generated kernels
struct PotLinear {
  const float* q;   // [4][stride] per-expert parameter rows (q[m] at expert j: q[m * stride + j])
  const float* p;   // shared parameters
  int K;            // experts; j >= K is padding
  int stride;       // the padded dimension
};

// A tall linear-model energy (more experts than the tile kernels hold; dense_lin_tall.hpp): the experts in
// nblk blocks of P = the pad of D (128, 256 or 512), each block laid out like a <= 512 model's matrices, zero padded
struct LinTallModel {
  const float* W1b;    // [blk][d][j] = W[blk P + j][d]   (first GEMM of the block:  u = W1b[blk]^T x + cb[blk])
  const float* W2Tb;   // [blk][j][d] = W[blk P + j][d]   (second GEMM: dE/dx += W2Tb[blk]^T phi(u))
  const float* cb;     // [nblk P]    = b
  int nblk, D, K;
};

// A wide linear-model energy (more dims than the tile kernels hold; dense_lin_wide.hpp): the tall layout's
// blocks of 512 experts with a dim chunk index added -- ND = Dpad / 512 chunks of 512 dims, every (block, chunk) a
// 512 x 512 matrix laid out like a <= 512 model's, zero padded (compare PotBigModel)
struct LinWideModel {
  const float* W1w;    // [jb][dc][d][j] = W[512 jb + j][512 dc + d]   (u += W1w[jb][dc]^T x_dc, from cb[jb])
  const float* W2Tw;   // [jb][dc][j][d] = W[512 jb + j][512 dc + d]   (dE/dx_dc += W2Tw[jb][dc]^T phi(u))
  const float* cb;     // [512 nblk]     = b
  int nblk, ND, D, K;
};

// Rates, waiting times and first minimum of ONE particle, evaluated serially by one lane (the dense
// kernels run it on 32 lanes of one wave, one particle each; ~1e3 instructions against ~1e6 cycles of
// trajectory).  markov_jump_hmc.py:366-396, utils.py:15-49.  Returns k (0 L, 1 F, 2 R).
template <bool REPLAY>
__device__ __forceinline__ int dense_decide(float H0, float HL, float Hflf, double p_r, uint32_t pid, int64_t p,
                                            int64_t N, const double* rexp, const RngKey& key, double& dwell, bool& bad) {
  const double l_rate = sqrt(exp((double)(H0 - HL)));
  const double flf_rate = sqrt(exp((double)(H0 - Hflf)));
  const double mn = (flf_rate != flf_rate || l_rate != l_rate) ? __builtin_nan("") : fmin(flf_rate, l_rate);
  const double f_rate = flf_rate - mn;
  const double r_rate = p_r;
  double eL, eF, eR;
  if constexpr (REPLAY) {
    eL = rexp[p];
    eF = rexp[N + p];
    eR = rexp[2 * N + p];
  } else {
    const u32x4 wq = philox4x32_10(pid, key.tick_lo, key.tick_hi, kSlotExpLF, key.k0, key.k1);
    const u32x4 qq = philox4x32_10(pid, key.tick_lo, key.tick_hi, kSlotExpR, key.k0, key.k1);
    eL = -log(u53(wq.w0, wq.w1));
    eF = -log(u53(wq.w2, wq.w3));
    eR = -log(u53(qq.w0, qq.w1));
  }
  bad = !(isfinite(l_rate) && isfinite(f_rate) && isfinite(r_rate));
  const double dL = l_rate == 0.0 ? __builtin_huge_val() : (1.0 / l_rate) * eL;
  const double dF = f_rate == 0.0 ? __builtin_huge_val() : (1.0 / f_rate) * eF;
  const double dR = r_rate == 0.0 ? __builtin_huge_val() : (1.0 / r_rate) * eR;
  int k = 0;
  double best = dL;
  if (!(best != best) && (dF < best || dF != dF)) {
    k = 1;
    best = dF;
  }
  if (!(best != best) && (dR < best || dR != dR)) {
    k = 2;
    best = dR;
  }
  dwell = best;
  return k;
}

// ContinuousTimeHMC (markov_jump_hmc.py:251-290): clocks FL (rate sqrt(exp(H0 - H_fl))), F (rate 1), R (rate p_r);
// min_idx is called with [f, fl, r], so ties go F, FL, R.  Returns k: 0 = FL, 1 = F, 2 = R.
template <bool REPLAY>
__device__ __forceinline__ int dense_decide_ct(float H0, float HL, double p_r, uint32_t pid, int64_t p, int64_t N,
                                               const double* rexp, const RngKey& key, double& dwell, bool& bad) {
  const double fl_rate = sqrt(exp((double)(H0 - HL)));
  const double r_rate = p_r;
  double eFL, eF, eR;
  if constexpr (REPLAY) {
    eFL = rexp[p];
    eF = rexp[N + p];
    eR = rexp[2 * N + p];
  } else {
    const u32x4 wq = philox4x32_10(pid, key.tick_lo, key.tick_hi, kSlotExpLF, key.k0, key.k1);
    const u32x4 qq = philox4x32_10(pid, key.tick_lo, key.tick_hi, kSlotExpR, key.k0, key.k1);
    eFL = -log(u53(wq.w0, wq.w1));
    eF = -log(u53(wq.w2, wq.w3));
    eR = -log(u53(qq.w0, qq.w1));
  }
  bad = !(isfinite(fl_rate) && isfinite(r_rate));
  const double dFL = fl_rate == 0.0 ? __builtin_huge_val() : (1.0 / fl_rate) * eFL;
  const double dF = eF;  // rate 1
  const double dR = r_rate == 0.0 ? __builtin_huge_val() : (1.0 / r_rate) * eR;
  int kk = 0;  // rows f, fl, r (markov_jump_hmc.py:271)
  double best = dF;
  if (!(best != best) && (dFL < best || dFL != dFL)) {
    kk = 1;
    best = dFL;
  }
  if (!(best != best) && (dR < best || dR != dR)) {
    kk = 2;
    best = dR;
  }
  dwell = best;
  return kk == 0 ? 1 : (kk == 1 ? 0 : 2);
}

// Discrete-time control samplers (markov_jump_hmc.py:116-148): accept the L F proposal with min(1, exp(H0 - H1)) (a NaN
// difference accepts, as `Ediff < 0` is False, :112-113), flip with probability p_flip; `gate`: the batch-wide
// momentum refresh fires this iteration.  Returns k = accepted | flipped << 1.
template <bool REPLAY>
__device__ __forceinline__ int dense_control(float H0, float HL, double p_r, double p_flip, uint32_t pid, int64_t p,
                                             int64_t N, const double* runif, const RngKey& key, bool& gate) {
  double uacc, uflip, ugate;
  if constexpr (REPLAY) {
    uacc = runif[p];
    uflip = runif[N + p];
    ugate = runif[2 * N];
  } else {
    const u32x4 q = philox4x32_10(pid, key.tick_lo, key.tick_hi, kSlotExpR, key.k0, key.k1);
    const u32x4 f = philox4x32_10(pid, key.tick_lo, key.tick_hi, kSlotFlip, key.k0, key.k1);
    const u32x4 g = philox4x32_10(0xFFFFFFFFu, key.tick_lo, key.tick_hi, kSlotFlip, key.k0, key.k1);
    uacc = u53(q.w2, q.w3);
    uflip = u53(f.w0, f.w1);
    ugate = u53(g.w2, g.w3);
  }
  const double dH = (double)(H0 - HL);
  const bool accept = !(dH < 0.0) || (uacc < exp(dH));
  const bool flip = uflip < p_flip;
  gate = ugate < p_r;
  return (accept ? 1 : 0) | (flip ? 2 : 0);
}

// float32 Box-Muller on two uniforms of u53() rounded to float32 (u2 may round to 1.0: the angle 2 pi)
__device__ __forceinline__ void box_muller_f32(float u1, float u2, float& z0, float& z1) {
  const float r = sqrtf(-2.0f * logf(u1 > 0.f ? u1 : 1e-38f));
  float s, c;
  sincospif(2.0f * u2, &s, &c);
  z0 = r * c;
  z1 = r * s;
}

// float32 Box-Muller pair from the same Philox words as normal_pair (the float64 version costs ~4x
// the instructions; for float32 / bfloat16 state its extra digits are rounded away anyway)
__device__ __forceinline__ void normal_pair_f32(const RngKey& k, uint32_t pid, uint32_t pair, float& z0, float& z1) {
  const u32x4 w = philox4x32_10(pid, k.tick_lo, k.tick_hi, pair, k.k0, k.k1);
  const float u1 = (float)u53(w.w0, w.w1);
  const float u2 = (float)u53(w.w2, w.w3);
  box_muller_f32(u1, u2, z0, z1);
}

// ndims == nbasis > 512 (the reference takes any square size, distributions.py:379-406): the pre-scaled matrices as
// 512 x 512 BLOCKS, each laid out like a whole 512-dim model's matrix, so that the tile kernels' GEMM runs on them as is
struct PotBigModel {
  const float* W1b;    // [db][jb][512][512]: block (db, jb) of W[d][j] / nu_j
  const float* W2Tb;   // [jb][db][512][512]: block (jb, db) of (W[d][j] (nu_j + 1) / nu_j)^T
  const float* cb;     // [dim]
  const float* alpha;  // [dim]
  int dim;             // ndims rounded up to a multiple of 512
  int ndims;
};
#ifndef __HIPCC_RTC__  // (host entry points: not in the hipRTC translation units of linear_energy.hip)
// E (or nullptr) and dE/dX (or nullptr) of rows X32 [rows_pad][dim] (float32, rows_pad a multiple of 32); U: scratch of
// the same shape.  2 (dim / 512)^2 block-GEMM launches + one elementwise pass.
void pot_big_eval(const PotBigModel& m, const float* X32, float* G32, float* E32, float* U, int64_t rows_pad, hipStream_t st);

// The hipRTC-built kernels of one linear-model energy (linear_energy.hip, one NB): the entry points below launch them, with
// the same grids and the same cold-list / fix / decide kernels, in place of ProductOfT's own when `gen` is given
struct PotGenerated {
  hipFunction_t jump32[3][2] = {};   // dense_pot_jump.inc   [mode][replay]
  hipFunction_t jump64[3][2] = {};   // dense_pot64_jump.inc [mode][replay]
  hipFunction_t eval = nullptr, leap = nullptr;
  PotLinear lin{};
};

void pot_launch_jump(const PotJumpArgs& a, const PotModel& mdl, hipStream_t st, const PotGenerated* gen = nullptr);
void pot_launch_eval(const PotEvalArgs& a, const PotModel& mdl, hipStream_t st, const PotGenerated* gen = nullptr);
void pot_launch_leap(const PotLeapArgs& a, const PotModel& mdl, hipStream_t st, const PotGenerated* gen = nullptr);
void pot64_launch_jump(const Pot64JumpArgs& a, const PotModel& mdl, hipStream_t st, const PotGenerated* gen = nullptr);
// a generated kernel on (args, model, experts): the signature of linear_energy.hip's wrappers
template <class A>
inline void pot_launch_generated(hipFunction_t f, unsigned grid, hipStream_t st, const A& a, const PotModel& mdl, const PotLinear& lin) {
  void* params[] = {(void*)&a, (void*)&mdl, (void*)&lin};
  (void)hipModuleLaunchKernel(f, grid, 1, 1, 256, 1, 1, 0, st, params, nullptr);
}
#endif

}  // namespace mjhmc
