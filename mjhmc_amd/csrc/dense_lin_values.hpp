// The values of ONE block of experts of a linear-model energy at every particle of one ring slot, stored (DESIGN.md
// section 3.3n): the piece between GEMM 1 of the tall force (dense_lin_tall.hpp), which forms u = W x + b block by block and
// keeps it on the chip, and the cross pass of crossmoments.hip, which contracts two per-particle matrices over the
// particles.  For the block blk of P = 128 NB experts, one value expression h(u, j; p, q) and the particles p of the slot:
//     T[p][j - blk P] = (float)h(u_j(x_p), j)        w_p > 0 and jlo <= j < jhi
//                     = 0.0f                          w_p == 0, p >= N, or j outside [jlo, jhi)   (jhi <= K)
// -- SELECTED, never multiplied: the passes that read T form w (t - ct) and (w x)(t - ct), and 0 * NaN must not form.
// T is the PANEL, [32 ntiles][P] float32: the N x K matrix of values is never stored, one panel is.
//
// Work item = tile of 32 particles, tiles strided over the grid.  Per workgroup the block's b -> sh.cb and its W1 rows
// (NB = 1: all of them, register resident; NB > 1: chunk 0, handed from GEMM to GEMM by gemm_dim) once; per tile x and the
// weights published, u = cb + W1^T x (GEMM 1 alone, as dense_lin_pointwise.hpp), h(u) published as float32 into the image
// phi(u) would take (sh.pub[1]) and stored from there: the image holds 32 NB groups of four experts (one float4 per
// particle); thread (g, sub) = (tid % (32 NB), tid / (32 NB)) owns group g and stores it for the particles sub, sub + 8 / NB,
// ... -- consecutive lanes write consecutive experts of a row (NB = 1: one float4 each, 512 contiguous bytes per row).
// A value that is not finite at w > 0 inside [jlo, jhi) lowers *flags to its expert j (an integer atomic: the lowest expert
// wins whatever the schedule).  Nothing is summed here: every element of T is written by exactly one thread.
#pragma once
#ifndef __HIPCC_RTC__  // hipRTC pre-includes the device runtime (linear_energy.hip)
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#include "dense_pot.hpp"
#include "dense_pot_kernels.hpp"
#include "dense_pot_tile.hpp"

namespace mjhmc {

constexpr int kLvNoBad = 0x7FFFFFFF;   // *flags when every value is finite

struct LvArgs {
  const float* X;     // [32 ntiles][P] float32 rows of one slot, rows beyond the batch zero
  const double* w;    // [>= N] weights, or nullptr for unit weights
  float* T;           // [32 ntiles][P] the panel
  int* flags;         // [1]: the lowest expert j of a value that is not finite
  int64_t N;
  int ntiles;         // ceil(N / 32)
  int blk;            // the block of experts [blk P, (blk + 1) P)
  int jlo, jhi;       // the experts asked for: jlo <= j < jhi <= K (others store 0)
};

#pragma clang fp contract(off)

__device__ __forceinline__ bool lv_finite(float v) { return fabsf(v) <= 3.4028234663852886e38f; }

// H::h(u, j, p, q): the caller's expression (linear_energy.hip)
template <int NB, class H>
__device__ __forceinline__ void lin_values_tiles(const LvArgs& a, const LinTallModel& tm, const PotLinear& lin, Shared<NB>& sh,
                                                 double* wts /* [32] LDS */) {
  constexpr int P = 128 * NB, NG = 32 * NB, SPLIT = 256 / NG;
  constexpr size_t MB = (size_t)P * P;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 31, h = lane >> 5;
  const int g = tid % NG, sub = tid / NG;
  // group g = ((w' NB + r) 4 + q4) 2 + h' of the image: its four experts are rows 8 q4 + 4 h' + qq of wave w', block r
  const int e0 = 32 * NB * ((g >> 3) / NB) + NB * (8 * ((g >> 1) & 3) + 4 * (g & 1)) + ((g >> 3) % NB);
  const int j0 = a.blk * P;
  const float* W1 = tm.W1b + (size_t)a.blk * MB;
  // GEMM 1 alone, ndims = P: NB = 1 walks every k-row group (the rows beyond D are zero), as the pointwise kernel
  const PotModel mdl{W1, W1, tm.cb + (size_t)a.blk * P, nullptr, P, P};
  bool jin[4];
#pragma unroll
  for (int qq = 0; qq < 4; ++qq) {
    const int j = j0 + e0 + NB * qq;
    jin[qq] = j >= a.jlo && j < a.jhi;
  }
  for (int i = tid; i < P; i += 256) sh.cb[i] = mdl.cb[i];
  AReg<NB> ar;
  if constexpr (NB == 1) {
    const float* m1 = W1 + (size_t)(4 * h) * 128 + 32 * w + c;
#pragma unroll
    for (int chunk = 0; chunk < 4; ++chunk) a_chunk_load<1>(m1, chunk, ar.w1[chunk]);
  } else {
    a_chunk_load<NB>(W1 + (size_t)(4 * NB * h) * P + 32 * NB * w + NB * c, 0, ar.a0);
  }
  int bad = kLvNoBad;
#pragma unroll 1
  for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int64_t p = (int64_t)tile * kP + c;
    {
      Tile<NB> x;
      tile_load<NB>(a.X, p, w, h, x);
      publish<NB>(sh.pub[0][w], lane, x);
    }
    if (tid < kP) {
      const int64_t pp = (int64_t)tile * kP + tid;
      wts[tid] = pp < a.N ? (a.w ? a.w[pp] : 1.0) : 0.0;
    }
    __syncthreads();   // x, the weights and (first tile) cb visible
    {
      Tile<NB> u;
      rowvec_load<NB>(sh.cb, w, h, u);
      if constexpr (NB == 1) gemm_any<1, false>(mdl, ar, sh.pub[0], w, c, h, lane, u);
      else gemm_dim<NB>(W1, W1, sh.pub[0], w, c, h, lane, ar.a0, u);   // (hands on chunk 0 of the same block: the next tile's)
#pragma unroll
      for (int q = 0; q < 16; ++q)
#pragma unroll
        for (int r = 0; r < NB; ++r) {
          const int j = j0 + 32 * NB * w + NB * acc_row(q, h) + r;
          u.b[r][q] = H::h(u.b[r][q], j, lin.p, LinQ{lin.q, lin.stride, j});
        }
      publish<NB>(sh.pub[1][w], lane, u);
    }
    __syncthreads();
    const f32x4* img = &sh.pub[1][0].v[0][0][0] + (g >> 1) * 64 + (g & 1) * 32;
#pragma unroll 1
    for (int cc = sub; cc < kP; cc += SPLIT) {
      const f32x4 t4 = img[cc];
      const bool on = wts[cc] > 0.0;
      float* row = a.T + ((size_t)tile * kP + cc) * P + e0;
      f32x4 o;
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) {
        const bool live = on && jin[qq];
        if (live && !lv_finite(t4[qq])) {
          const int j = j0 + e0 + NB * qq;
          bad = j < bad ? j : bad;
        }
        o[qq] = live ? t4[qq] : 0.0f;
      }
      if constexpr (NB == 1) {
        *reinterpret_cast<f32x4*>(row) = o;
      } else {
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) row[NB * qq] = o[qq];
      }
    }
    __syncthreads();   // both images and the weights are read: the next tile may take them
  }
  if (bad != kLvNoBad) atomicMin(a.flags, bad);
}

}  // namespace mjhmc
