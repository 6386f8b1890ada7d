// Grouped linear-model energies: the tall form with a log-sum-exp over groups of experts,
//
//     E(x) = sum_{j<K} f(u_j, j) + sum_{g<G} LSE_{c<C} u_{gC+c},   u = W x + b
//     dE/dx = W^T phi,   phi_j = f'(u_j, j) + [j < G C] softmax_g(u)_c
//
// -- multinomial logistic (softmax) regression: G data rows of C classes, then plain experts (a prior).  The first G C
// experts are G groups of C consecutive experts, 2 <= C <= 16.  The host (linear_energy.hip) stores the experts of a block
// of P = 128 NB so that the C members of a group are C consecutive slots of ONE lane's 16 NB accumulator registers: the
// max, the sum of exponentials and the softmax between GEMM 1 and GEMM 2 are then an unrolled loop over registers with
// static indices -- no cross-lane traffic, no LDS, no barrier beyond the tall kernel's two per block, and u never reaches
// memory.  Grouped blocks come first; the plain experts follow in blocks of their own, laid out and evaluated exactly as
// a tall model's (LinearTallExperts, dense_lin_tall.hpp), through the family's block step (lin_block, dense_lin_tall.hpp).
#pragma once
#ifndef __HIPCC_RTC__  // hipRTC pre-includes the device runtime (linear_energy.hip)
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#include "dense_lin_tall.hpp"

namespace mjhmc {

// The blocks of a grouped model, nbg grouped ones and then nbp plain ones, contiguous and each laid out like a <= 512
// model's matrices.  Slot (blk, local) of a grouped block, local = 32 NB w + NB acc_row(q, h) + r, is slot s = NB q + r of
// lane type (w, h); the lane type holds the Gl = floor(16 NB / C) groups (8 blk + 2 w + h) Gl + gl, gl < Gl, group gl in
// its slots [C gl, C gl + C); the slots from C Gl on, and the groups at or beyond G, are padding (zero columns, masked).
struct LinGroupedModel {
  const float* W1b;    // [blk][d][slot] (first GEMM of the block:  u = W1b[blk]^T x + cb[blk])
  const float* W2Tb;   // [blk][slot][d] (second GEMM: dE/dx += W2Tb[blk]^T phi(u))
  const float* cb;     // [(nbg + nbp) P]
  int nbg, nbp;        // grouped blocks, plain blocks
  int D, K, G;         // dims, experts (G C grouped ones first), groups
};

template <int NB>
__device__ __forceinline__ float slot_get(const Tile<NB>& u, int s) { return u.b[s % NB][s / NB]; }

// The experts of one grouped block.  The caller's f / f' see the caller's expert index j = g C + c; the q[m] rows are
// stored in slot order (rows of lin.stride floats).  The group term in float32, contraction off, one order: m = fmaxf over
// c ascending, t_c = expf(u_c - m), s = t_0 + ... + t_{C-1} ascending, the term m + logf(s), the softmax t_c / s.
template <class F, int C>
struct LinearGroupedExperts {
  PotLinear lin;
  int blk, G;
  template <int NB>
  __device__ __forceinline__ float group_max(const Tile<NB>& u, int gl) const {
    float m = slot_get<NB>(u, C * gl);
#pragma unroll
    for (int c = 1; c < C; ++c) m = fmaxf(m, slot_get<NB>(u, C * gl + c));
    return m;
  }
  template <int NB>
  __device__ __forceinline__ float energy_sum(const Tile<NB>& u, int w, int h) const {
    constexpr int Gl = 16 * NB / C, P = 128 * NB;
    const int g0 = (8 * blk + 2 * w + h) * Gl, slot0 = blk * P + 32 * NB * w;
    float es = 0.f;
#pragma unroll
    for (int gl = 0; gl < Gl; ++gl) {
      const bool live = g0 + gl < G;
      const float m = group_max<NB>(u, gl);
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float t = expf(slot_get<NB>(u, C * gl + c) - m);
        s = c ? s + t : t;
      }
      const float lse = m + logf(s);
      es += live ? lse : 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const int sl = C * gl + c, j = (g0 + gl) * C + c;
        const float e = F::f(slot_get<NB>(u, sl), j, lin.p, LinQ{lin.q, lin.stride, slot0 + NB * acc_row(sl / NB, h) + sl % NB});
        es += live ? e : 0.f;
      }
    }
    return es;
  }
  template <int NB>
  __device__ __forceinline__ void phi(Tile<NB>& u, int w, int h) const {
    constexpr int Gl = 16 * NB / C, P = 128 * NB;
    const int g0 = (8 * blk + 2 * w + h) * Gl, slot0 = blk * P + 32 * NB * w;
#pragma unroll
    for (int gl = 0; gl < Gl; ++gl) {
      const bool live = g0 + gl < G;
      const float m = group_max<NB>(u, gl);
      float t[C];
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        t[c] = expf(slot_get<NB>(u, C * gl + c) - m);
        s = c ? s + t[c] : t[c];
      }
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const int sl = C * gl + c, j = (g0 + gl) * C + c;
        const float g = F::fp(slot_get<NB>(u, sl), j, lin.p, LinQ{lin.q, lin.stride, slot0 + NB * acc_row(sl / NB, h) + sl % NB}) + t[c] / s;
        u.b[sl % NB][sl / NB] = live ? g : 0.f;
      }
    }
#pragma unroll
    for (int sl = C * Gl; sl < 16 * NB; ++sl) u.b[sl % NB][sl / NB] = 0.f;   // the lane's padding slots
  }
};

// E(X), dE/dX(X) of rows a.X ([32 ntiles][P] float32, rows beyond the batch zero), as lin_tall_eval_tiles: x published once
// per tile, then the grouped blocks and the plain blocks in storage order, dE/dx accumulating in the same registers.  One
// order of additions whatever the grid: the result depends on the model and the row alone.
template <int NB, int C, class F>
__device__ __forceinline__ void lin_grouped_eval_tiles(const PotEvalArgs& a, const LinGroupedModel& gm, const PotLinear& lin, Shared<NB>& sh) {
  static_assert(C >= 2 && C <= 16, "a group has 2 to 16 members");
  constexpr int P = 128 * NB;
  constexpr size_t MB = (size_t)P * P;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 31, h = lane >> 5;
  const int nblk = gm.nbg + gm.nbp, GC = gm.G * C;
  // the plain experts' caller index j = G C + (their position): the q rows are in slot order, nbg P - G C >= 0 further on
  const PotLinear plin{lin.q + ((size_t)gm.nbg * P - (size_t)GC), lin.p, gm.K, lin.stride};
  AReg<NB> ar;
  if constexpr (NB > 1) areg_load<NB>(PotModel{gm.W1b, gm.W2Tb, gm.cb, nullptr, P, P}, w, c, h, ar);
  for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int64_t p = tile * kP + c;
    Tile<NB> g;
    {
      Tile<NB> x;
      tile_load<NB>(a.X, p, w, h, x);
      publish<NB>(sh.pub[0][w], lane, x);   // (the last reads of the previous tile's image lie before its closing barriers)
    }
#pragma unroll
    for (int r = 0; r < NB; ++r)
#pragma unroll
      for (int q = 0; q < 16; ++q) g.b[r][q] = 0.f;
    float es = 0.f;
#pragma unroll 1
    for (int blk = 0; blk < gm.nbg; ++blk) {
      // (NB = 1 skips k-row groups at or beyond PotModel::ndims: a permuted block may use any of its P columns)
      const PotModel mdl{gm.W1b + blk * MB, gm.W2Tb + blk * MB, gm.cb + (size_t)blk * P, nullptr, P, P};
      const LinearGroupedExperts<F, C> xp{lin, blk, gm.G};
      const int nxt = blk + 1 < nblk ? blk + 1 : 0;          // (the last block hands on block 0's W1: the next tile's)
      lin_block<NB>(mdl, xp, gm.W1b + nxt * MB, ar, sh, w, c, h, lane, a.E != nullptr, es, g);
    }
#pragma unroll 1
    for (int pb = 0; pb < gm.nbp; ++pb) {
      const int blk = gm.nbg + pb;
      const int left = gm.K - GC - pb * P;                   // plain experts of this block (> 0; >= P: a full block)
      const int kexp = left < P ? left : P;
      const PotModel mdl{gm.W1b + blk * MB, gm.W2Tb + blk * MB, gm.cb + (size_t)blk * P, nullptr, P, gm.D > kexp ? gm.D : kexp};
      const LinearTallExperts<F> xp{plin, GC + pb * P};
      const int nxt = blk + 1 < nblk ? blk + 1 : 0;
      lin_block<NB>(mdl, xp, gm.W1b + nxt * MB, ar, sh, w, c, h, lane, a.E != nullptr, es, g);
    }
    if (a.E) {
      const float part = half_sum(es);
      if (h == 0) sh.red[0][w][c] = part;
      __syncthreads();
      if (w == 0 && h == 0) a.E[p] = sh.red[0][0][c] + sh.red[0][1][c] + sh.red[0][2][c] + sh.red[0][3][c];
    }
    if (a.G) tile_store<NB>(a.G, p, w, h, g);
    __syncthreads();
  }
}

}  // namespace mjhmc
