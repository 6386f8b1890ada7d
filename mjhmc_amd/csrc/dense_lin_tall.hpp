// Tall linear-model energies: E(x) = sum_{j<K} f(u_j, j), u = W x + b with MORE experts than the
// tile kernels' 512 -- W: K x D, D <= 512, K <= 2^20.  The experts are cut into nblk = ceil(K / P) blocks of P = 128 NB
// (the pad of D alone), every block a square P x P model laid out like a <= 512 model's W1 / W2T / cb, and ONE kernel walks
// the blocks per tile of 32 particles: u never leaves the registers (as an N x K matrix in HBM it would be 26 GB at
// N = 10^5, K = 65 536) and dE/dx accumulates over the blocks in the same accumulator registers.  Built from the tile
// kernels' own parts (dense_pot_tile.hpp) and compiled with hipRTC around the caller's f / f' (linear_energy.hip).
#pragma once
#ifndef __HIPCC_RTC__  // hipRTC pre-includes the device runtime (linear_energy.hip)
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#include "dense_pot.hpp"
#include "dense_pot_kernels.hpp"
#include "dense_pot_tile.hpp"

namespace mjhmc {

// LinearExperts for one block of a tall model: the local expert of the tile layout is expert j0 + local of the model --
// that is the j the caller's expressions see, the entry of the q[m] rows they read (rows of lin.stride = nblk P floats)
// and what the mask j < lin.K tests.
template <class F>
struct LinearTallExperts {
  PotLinear lin;
  int j0;
  template <int NB>
  __device__ __forceinline__ float energy_sum(const Tile<NB>& u, int w, int h) const {
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q)
#pragma unroll
      for (int r = 0; r < NB; ++r) {
        const int j = j0 + 32 * NB * w + NB * acc_row(q, h) + r;
        const float e = F::f(u.b[r][q], j, lin.p, LinQ{lin.q, lin.stride, j});
        s += j < lin.K ? e : 0.f;
      }
    return s;
  }
  template <int NB>
  __device__ __forceinline__ void phi(Tile<NB>& u, int w, int h) const {
#pragma unroll
    for (int q = 0; q < 16; ++q)
#pragma unroll
      for (int r = 0; r < NB; ++r) {
        const int j = j0 + 32 * NB * w + NB * acc_row(q, h) + r;
        const float g = F::fp(u.b[r][q], j, lin.p, LinQ{lin.q, lin.stride, j});
        u.b[r][q] = j < lin.K ? g : 0.f;
      }
  }
};

// One block step with the block's experts XP (LinearTallExperts here, LinearGroupedExperts in dense_lin_grouped.hpp):
// cb -> LDS, u = cb + W1^T x (GEMM 1), the lane's energy terms into a running float, phi(u) published, g += W2T^T phi(u)
// (GEMM 2, g never zeroed between blocks).  `next` is the matrix whose chunk 0 leaves in ar (NB > 1).  The grouped kernel's
// two loops call it.  lin_tall_eval_tiles below holds the same step as text of its own: as a callee the step compiles to
// other code there (tools/isa_equal.py --rtc: up to 28 registers fewer at NB = 1, but 4 more and a few more instructions
// for some expressions at NB = 2 and 4), and a listing that is higher anywhere is not taken without need.
template <int NB, class XP>
__device__ __forceinline__ void lin_block(const PotModel& mdl, const XP& xp, const float* next, AReg<NB>& ar, Shared<NB>& sh,
                                          int w, int c, int h, int lane, bool want_E, float& es, Tile<NB>& g) {
  constexpr int P = 128 * NB;
  // sh.cb was last read in front of the previous block's GEMM 1, and every wave has passed a barrier since
  for (int i = threadIdx.x; i < P; i += 256) sh.cb[i] = mdl.cb[i];
  if constexpr (NB == 1) areg_load<1>(mdl, w, c, h, ar);     // both matrices of the block, register resident
  __syncthreads();   // cb and (first block) x visible; the previous block's GEMM 2 has read its phi(u) image
  Tile<NB> u;
  rowvec_load<NB>(sh.cb, w, h, u);
  if constexpr (NB == 1) gemm_any<1, false>(mdl, ar, sh.pub[0], w, c, h, lane, u);
  else gemm_dim<NB>(mdl.W1, mdl.W2T, sh.pub[0], w, c, h, lane, ar.a0, u);
  if (want_E) es += xp.template energy_sum<NB>(u, w, h);
  xp.template phi<NB>(u, w, h);
  publish<NB>(sh.pub[1][w], lane, u);
  __syncthreads();
  if constexpr (NB == 1) gemm_any<1, true>(mdl, ar, sh.pub[1], w, c, h, lane, g);
  else gemm_dim<NB>(mdl.W2T, next, sh.pub[1], w, c, h, lane, ar.a0, g);
}

// The evaluation E(X), dE/dX(X) of rows a.X ([32 ntiles][P] float32, rows beyond the batch zero).  Per tile: x is published
// once; per block: cb -> LDS, u = cb + W1[blk]^T x (GEMM 1), the lane's energy terms into a running float, phi(u) published,
// g += W2T[blk]^T phi(u) (GEMM 2, never zeroed between blocks).  The GEMMs alternate W1[0], W2T[0], W1[1], ...: gemm_dim
// hands chunk 0 of the next matrix across the epilogue as in the tile kernels.  One order of additions whatever the grid:
// the result depends on the model and the row alone.
template <int NB, class F>
__device__ __forceinline__ void lin_tall_eval_tiles(const PotEvalArgs& a, const LinTallModel& tm, const PotLinear& lin, Shared<NB>& sh) {
  constexpr int P = 128 * NB;
  constexpr size_t MB = (size_t)P * P;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 31, h = lane >> 5;
  AReg<NB> ar;
  if constexpr (NB > 1) areg_load<NB>(PotModel{tm.W1b, tm.W2Tb, tm.cb, nullptr, P, P}, w, c, h, ar);
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
    for (int blk = 0; blk < tm.nblk; ++blk) {
      const int left = tm.K - blk * P;                          // experts of this block (> 0; >= P: a full block)
      const int kexp = left < P ? left : P;
      const PotModel mdl{tm.W1b + blk * MB, tm.W2Tb + blk * MB, tm.cb + (size_t)blk * P, nullptr, P, tm.D > kexp ? tm.D : kexp};
      const LinearTallExperts<F> xp{lin, blk * P};
      // sh.cb was last read in front of the previous block's GEMM 1, and every wave has passed a barrier since
      for (int i = threadIdx.x; i < P; i += 256) sh.cb[i] = mdl.cb[i];
      if constexpr (NB == 1) areg_load<1>(mdl, w, c, h, ar);     // both matrices of the block, register resident
      __syncthreads();   // cb and (first block) x visible; the previous block's GEMM 2 has read its phi(u) image
      Tile<NB> u;
      rowvec_load<NB>(sh.cb, w, h, u);
      if constexpr (NB == 1) gemm_any<1, false>(mdl, ar, sh.pub[0], w, c, h, lane, u);
      else gemm_dim<NB>(mdl.W1, mdl.W2T, sh.pub[0], w, c, h, lane, ar.a0, u);
      if (a.E) es += xp.template energy_sum<NB>(u, w, h);
      xp.template phi<NB>(u, w, h);
      publish<NB>(sh.pub[1][w], lane, u);
      __syncthreads();
      if constexpr (NB == 1) {
        gemm_any<1, true>(mdl, ar, sh.pub[1], w, c, h, lane, g);
      } else {
        const int nxt = blk + 1 < tm.nblk ? blk + 1 : 0;       // (the last block hands on block 0's W1: the next tile's)
        gemm_dim<NB>(mdl.W2T, tm.W1b + nxt * MB, sh.pub[1], w, c, h, lane, ar.a0, g);
      }
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
