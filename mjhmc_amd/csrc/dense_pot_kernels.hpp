// What the float32-state tile kernels share beyond dense_pot_tile.hpp: the experts of a linear-model energy and the
// finish of a move.  The kernels' bodies are the fragments dense_pot_{eval,jump,leap}.inc, included inside the kernel
// definitions -- ProductOfT's in dense_pot.hip (experts: PotExperts), a linear-model energy's in the hipRTC translation
// unit of linear_energy.hip (experts: LinearExperts<F>).  (As device functions called from thin kernels the bodies
// compiled to different instruction schedules for ProductOfT; inside the kernel they are the original text: DESIGN.md 3.6b.)
#pragma once
#ifndef __HIPCC_RTC__  // hipRTC pre-includes the device runtime (linear_energy.hip)
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#include "dense_pot.hpp"
#include "dense_pot_tile.hpp"

namespace mjhmc {

// Per-expert parameter rows at expert j: q[m] is row m's entry j (rows of `stride` floats)
struct LinQ {
  const float* q;
  int stride, j;
  __device__ __forceinline__ float operator[](int m) const { return q[(size_t)m * stride + j]; }
};

// A caller's experts: F::f(u, j, p, q) (the energy term) and F::fp(u, j, p, q) (its derivative, phi), p the shared
// parameters, q the per-expert rows at j (the functor linear_energy.hip generates).  Experts at or beyond lin.K are
// padding: their terms and their phi are masked to exactly 0 by a select -- f(0) need not be 0 (softplus: log 2) and
// f'(0) need not be finite (u / fabs(u)), and the padded matrix rows are zero either way.
template <class F>
struct LinearExperts {
  static constexpr bool kProductOfT = false;
  PotLinear lin;
  template <int NB>
  __device__ __forceinline__ float energy_sum(const Tile<NB>& u, int w, int h) const {
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q)
#pragma unroll
      for (int r = 0; r < NB; ++r) {
        const int j = 32 * NB * w + NB * acc_row(q, h) + r;
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
        const int j = 32 * NB * w + NB * acc_row(q, h) + r;
        const float g = F::fp(u.b[r][q], j, lin.p, LinQ{lin.q, lin.stride, j});
        u.b[r][q] = j < lin.K ? g : 0.f;
      }
  }
};

// The successor's rows once the moves of a tile's columns stand in sh.move.  FIX = false (jump kernel): x, v, g hold the
// end point of L.  FIX = true (pot_fix_kernel): columns that keep the end point are finished already (their rows hold
// it); only the others are touched.
template <int NB, bool REPLAY, int MODE, bool FIX, class SH>
__device__ __forceinline__ void pot_finish(const PotJumpArgs& a, SH& sh, int64_t p, bool alive, int w, int c, int h,
                                           Tile<NB>& x, Tile<NB>& v, Tile<NB>& g) {
  const int mv = sh.move[c];
  const int k = mv & 3;
  bool refresh;  // this column's momentum is redrawn (HMCState.R)
  bool touch = true;
  if constexpr (MODE == kModeControl) {
    if (!(k & 1)) {  // rejected: back to the pre-move state
      tile_load<NB>(a.X_in, p, w, h, x);
      tile_load<NB>(a.G_in, p, w, h, g);
      tile_load<NB>(a.V_in, p, w, h, v);
    } else {  // accepted L F: flip
#pragma unroll
      for (int r = 0; r < NB; ++r) v.b[r] = -v.b[r];
    }
    if (k & 2) {
#pragma unroll
      for (int r = 0; r < NB; ++r) v.b[r] = -v.b[r];
    }
    refresh = (mv & 4) != 0;  // batch-wide (markov_jump_hmc.py:138-141)
  } else {
    const bool keep_L = (k == 0);
    if constexpr (FIX) touch = !keep_L;
    if (!keep_L) {  // F / R keep the position (and its gradient)
      tile_load<NB>(a.X_in, p, w, h, x);
      tile_load<NB>(a.G_in, p, w, h, g);
      tile_load<NB>(a.V_in, p, w, h, v);
    }
    if ((MODE == kModeCT && k == 0) || k == 1) {  // CT's FL move ends with a flip (:258,278); F flips
#pragma unroll
      for (int r = 0; r < NB; ++r) v.b[r] = -v.b[r];
    }
    refresh = (k == 2);
  }
  const bool tile_refreshes = __ballot(refresh) != 0ull;
  if constexpr (REPLAY) {
    if (refresh) {  // HMCState.R (hmc_state.py:121-129) with the recorded normals
      Tile<NB> z;
      tile_load<NB>(a.noise, alive ? p : 0, w, h, z);
#pragma unroll
      for (int r = 0; r < NB; ++r) v.b[r] = v.b[r] * a.r_keep + z.b[r] * a.r_mix;
    }
  } else {
    // column by column (the set is the same in every wave: it comes from sh.move), the whole workgroup drawing
    unsigned cols = (unsigned)(__ballot(refresh) & 0xFFFFFFFFull);
    while (cols) {
      const int c0 = __ffs((int)cols) - 1;
      cols &= cols - 1;
      const int64_t p0 = __shfl((long long)p, c0);
      column_normals<NB, float>(a.key, (uint32_t)(a.first_pid + (p0 < a.N ? p0 : 0)), a.D, sh.zn);
      __syncthreads();
      if (c == c0) {
        using V = typename VecN<NB>::type;
        const float* zrow = sh.zn + 32 * NB * w;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const V z = *reinterpret_cast<const V*>(zrow + NB * acc_row(q, h));
#pragma unroll
          for (int r = 0; r < NB; ++r) v.b[r][q] = v.b[r][q] * a.r_keep + vget<NB>(z, r) * a.r_mix;
        }
      }
      __syncthreads();
    }
  }
  if (tile_refreshes) {  // all waves take part in the reduction; only refreshed columns use the result
    const float evr = pot_kinetic<NB>(sh, w, c, h, v);
    if (refresh && w == 0 && h == 0) a.EV_out[p] = evr;
  }
  if (touch) {
    tile_store<NB>(a.X_out, p, w, h, x);
    tile_store<NB>(a.V_out, p, w, h, v);
    tile_store<NB>(a.G_out, p, w, h, g);
  }
}

}  // namespace mjhmc
