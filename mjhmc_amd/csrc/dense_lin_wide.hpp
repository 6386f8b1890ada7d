// Wide linear-model energies: E(x) = sum_{j<K} f(u_j, j), u = W x + b with MORE dims than the tile
// kernels' 512 -- W: K x D, D <= 4096, K <= 2^20.  The dims are cut into ND = Dpad / 512 chunks (Dpad: D rounded up to a
// multiple of 512), the experts into nblk = ceil(K / 512) blocks, every (block, chunk) a 512 x 512 matrix laid out like a
// <= 512 model's W1 / W2T, and ONE kernel walks them per tile of 32 particles.  Per expert block: u = cb + sum over the dim
// chunks of W1w[jb][dc]^T x_dc in the accumulator registers (x_dc published chunk by chunk), the energy terms, phi(u)
// published, and then per dim chunk g_dc += W2Tw[jb][dc]^T phi(u).  u and phi(u) never leave the chip; dE/dx is ND tiles
// wide, more than the register file holds, and lives in the tile's own G rows between the expert blocks: only the owning
// workgroup touches them, each lane reads back exactly the elements it stored, so there is no race, no atomic, and no
// zeroing of G before the launch (block 0 starts every chunk from zero).  One order of additions whatever the grid.  Built
// from the tile kernels' own parts (dense_pot_tile.hpp, LinearTallExperts of dense_lin_tall.hpp) at NB = 4 and compiled with
// hipRTC around the caller's f / f' (linear_energy.hip).  One chunk (D <= 512) performs the tall kernel's operations in the
// tall kernel's order: the same bits.
#pragma once
#ifndef __HIPCC_RTC__  // hipRTC pre-includes the device runtime (linear_energy.hip)
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#include "dense_lin_tall.hpp"

namespace mjhmc {

// tile_load / tile_store (dense_pot_tile.hpp) on rows of another pitch, from column col0 on: chunk col0 / (128 NB) of the
// rows of particle `p` in a particle-major [*, pitch] matrix
template <int NB>
__device__ __forceinline__ void tile_load_at(const float* base, int pitch, int col0, int64_t p, int w, int h, Tile<NB>& t) {
  using V = typename VecN<NB>::type;
  const float* row = base + (size_t)p * pitch + col0 + 32 * NB * w;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const V v = *reinterpret_cast<const V*>(row + NB * acc_row(q, h));
#pragma unroll
    for (int r = 0; r < NB; ++r) t.b[r][q] = vget<NB>(v, r);
  }
}

template <int NB>
__device__ __forceinline__ void tile_store_at(float* base, int pitch, int col0, int64_t p, int w, int h, const Tile<NB>& t) {
  using V = typename VecN<NB>::type;
  float* row = base + (size_t)p * pitch + col0 + 32 * NB * w;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    V v;
#pragma unroll
    for (int r = 0; r < NB; ++r) vset<NB>(v, r, t.b[r][q]);
    *reinterpret_cast<V*>(row + NB * acc_row(q, h)) = v;
  }
}

// The evaluation E(X), dE/dX(X) of rows a.X ([32 ntiles][512 ND] float32, rows beyond the batch and dims beyond D zero).
// The GEMMs walk W1w[jb][0 .. ND-1], W2Tw[jb][0 .. ND-1], W1w[jb+1][0], ...: gemm_dim hands chunk 0 of the next matrix of
// that walk across the epilogue as in the tile kernels (an energy-only call skips the W2Tw matrices; the last hand-over goes
// to block 0, the next tile's first matrix).
template <class F>
__device__ __forceinline__ void lin_wide_eval_tiles(const PotEvalArgs& a, const LinWideModel& wm, const PotLinear& lin, Shared<4>& sh) {
  constexpr int NB = 4, P = 128 * NB;
  constexpr size_t MB = (size_t)P * P;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 31, h = lane >> 5;
  const int ND = wm.ND, pitch = P * ND;
  const bool want_G = a.G != nullptr;
  AReg<NB> ar;
  areg_load<NB>(PotModel{wm.W1w, wm.W2Tw, wm.cb, nullptr, P, P}, w, c, h, ar);
  for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int64_t p = tile * kP + c;
    float es = 0.f;
#pragma unroll 1
    for (int jb = 0; jb < wm.nblk; ++jb) {
      const float* W1 = wm.W1w + (size_t)jb * ND * MB;
      const float* W2T = wm.W2Tw + (size_t)jb * ND * MB;
      const float* W1next = wm.W1w + (size_t)(jb + 1 < wm.nblk ? jb + 1 : 0) * ND * MB;
      const LinearTallExperts<F> xp{lin, jb * P};
      // phase 1: u = cb + sum_dc W1w[jb][dc]^T x_dc, ascending dc
      Tile<NB> u;
#pragma unroll 1
      for (int dc = 0; dc < ND; ++dc) {
        {
          Tile<NB> x;
          tile_load_at<NB>(a.X, pitch, P * dc, p, w, h, x);
          __syncthreads();   // the previous GEMM on the x image (the previous chunk's, block's or tile's) has read it
          publish<NB>(sh.pub[0][w], lane, x);
        }
        // sh.cb was last read behind the previous block's second barrier: an energy-only call of one chunk has no other
        // barrier between that read and this write than the one above
        if (dc == 0)
          for (int i = threadIdx.x; i < P; i += 256) sh.cb[i] = wm.cb[(size_t)jb * P + i];
        __syncthreads();     // x_dc and (dc == 0) cb visible
        if (dc == 0) rowvec_load<NB>(sh.cb, w, h, u);
        const float* next = dc + 1 < ND ? W1 + (size_t)(dc + 1) * MB : (want_G ? W2T : W1next);
        gemm_dim<NB>(W1 + (size_t)dc * MB, next, sh.pub[0], w, c, h, lane, ar.a0, u);
      }
      if (a.E) es += xp.template energy_sum<NB>(u, w, h);
      if (!want_G) continue;
      // phase 2: per dim chunk g_dc (zero at block 0, else what the previous block left in the G rows) += W2Tw[jb][dc]^T phi(u)
      xp.template phi<NB>(u, w, h);
      publish<NB>(sh.pub[1][w], lane, u);   // (the previous block's last GEMM on this image lies before phase 1's barriers)
      __syncthreads();
#pragma unroll 1
      for (int dc = 0; dc < ND; ++dc) {
        Tile<NB> g;
        if (jb == 0) {
#pragma unroll
          for (int r = 0; r < NB; ++r)
#pragma unroll
            for (int q = 0; q < 16; ++q) g.b[r][q] = 0.f;
        } else {
          tile_load_at<NB>(a.G, pitch, P * dc, p, w, h, g);
        }
        const float* next = dc + 1 < ND ? W2T + (size_t)(dc + 1) * MB : W1next;
        gemm_dim<NB>(W2T + (size_t)dc * MB, next, sh.pub[1], w, c, h, lane, ar.a0, g);
        tile_store_at<NB>(a.G, pitch, P * dc, p, w, h, g);
      }
    }
    if (a.E) {
      const float part = half_sum(es);
      if (h == 0) sh.red[0][w][c] = part;
      __syncthreads();
      if (w == 0 && h == 0) a.E[p] = sh.red[0][0][c] + sh.red[0][1][c] + sh.red[0][2][c] + sh.red[0][3][c];
    }
    __syncthreads();   // (sh.red is written again by the next tile only behind further barriers; this closes the tile as the tall kernel does)
  }
}

}  // namespace mjhmc
