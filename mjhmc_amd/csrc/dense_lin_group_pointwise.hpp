// Per-group ("per data row") statistics of a grouped linear-model energy over a recorded ensemble (DESIGN.md section
// 3.3o): the TRANSPOSE of lin_grouped_eval_kernel (dense_lin_grouped.hpp), as dense_lin_pointwise.hpp is the transpose of
// the tall kernel -- and that pass itself (pw_items: the same items, tile loop, reduction, store and fold) with the values
// of a block formed here.  After GEMM 1 a lane holds all C logits of its Gl = floor(16 NB / C) groups in registers, so per
// group, in float32 with contraction off and exactly as the energy forms them (LinearGroupedExperts),
//     m = fmaxf over c ascending,  t_c = expf(u_c - m),  s = t_0 + ... + t_{C-1} ascending,  lse = m + logf(s),  sm_c = t_c / s
// are a register loop with static indices: no cross-lane traffic, no LDS and no barrier beyond the pass's own.  A value is
// h_m(u, j; p, q; lse, sm, c) at member c of group g (j = g C + c, the caller's index), of one of two kinds:
//   * per member: one number per grouped expert, column j = g C + c;
//   * per group:  the float32 sum of h_m over the members in ascending c (s = c ? s + t : t), column g.  It travels in the
//     image entry of member 0's slot; the entries of the other members are dead for that value.
// Only the nbg grouped blocks are walked: the plain experts behind the groups are not reported on.
//
// The column of an image entry is arithmetic (linear_grouped_layout's rule, no table).  Reduction thread g of the image
// owns the entries qq < 4 of lane type (w', h') = ((g >> 3) / NB, g & 1), accumulator slots s = NB (4 ((g >> 1) & 3) + qq)
// + (g >> 3) % NB; slot s is member s % C of the lane type's group gl = s / C, which is the model's group
// (8 blk + 2 w' + h') Gl + gl.  Padding slots (gl >= Gl) and groups at or beyond G have the column kPwDead: in no sum, in no
// check, never stored.
#pragma once
#ifndef __HIPCC_RTC__  // hipRTC pre-includes the device runtime (linear_energy.hip)
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#include "dense_lin_grouped.hpp"
#include "dense_lin_pointwise.hpp"

namespace mjhmc {

#pragma clang fp contract(off)

// The grouped block `blk` as pw_items sees it.  H: kM values, kMemberMask (bit m: value m is per member),
// h<MI>(u, j, p, q, lse, sm, c) the caller's expressions (linear_energy.hip).
template <int NB, int C, class H>
struct GpBlock {
  static constexpr int kM = H::kM, Gl = 16 * NB / C, P = 128 * NB;
  const PotLinear& lin;
  int G;
  int blk;
  int jm[4], jg[4];   // the thread's four columns of a per-member value, of a per-group value

  template <int MI>
  static constexpr bool member() { return (H::kMemberMask >> MI) & 1u; }

  __device__ __forceinline__ void set(int blk_, int g) {
    blk = blk_;
    const int g0 = (8 * blk + 2 * ((g >> 3) / NB) + (g & 1)) * Gl;
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) {
      const int s = NB * (4 * ((g >> 1) & 3) + qq) + (g >> 3) % NB;
      const int gl = s / C, c = s - gl * C;
      const bool live = gl < Gl && g0 + gl < G;
      jm[qq] = live ? (g0 + gl) * C + c : kPwDead;
      jg[qq] = live && c == 0 ? g0 + gl : kPwDead;
    }
  }

  // value MI of the lane's groups into the image, reduced; then the values after it
  template <int MI>
  __device__ __forceinline__ void value(const Tile<NB>& u, Shared<NB>& sh, const double* wts, int w, int h, int lane, int g, int sub,
                                        unsigned lme, PwAcc<kM>& acc, int& bad) const {
    {
      const LinearGroupedExperts<H, C> xp{lin, blk, G};   // (the energy's own max; its f / f' are not asked for)
      const int g0 = (8 * blk + 2 * w + h) * Gl, slot0 = blk * P + 32 * NB * w;
      Tile<NB> v;
#pragma unroll
      for (int gl = 0; gl < Gl; ++gl) {
        // (groups at or beyond G are not masked here: their columns are dead, their q rows and logits zero)
        const float m = xp.template group_max<NB>(u, gl);
        float t[C];
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
          t[c] = expf(slot_get<NB>(u, C * gl + c) - m);
          s = c ? s + t[c] : t[c];
        }
        const float lse = m + logf(s);
        float gs = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const int sl = C * gl + c, j = (g0 + gl) * C + c;
          const float val = H::template h<MI>(slot_get<NB>(u, sl), j, lin.p, LinQ{lin.q, lin.stride, slot0 + NB * acc_row(sl / NB, h) + sl % NB},
                                              lse, t[c] / s, c);
          if constexpr (member<MI>()) {
            v.b[sl % NB][sl / NB] = val;
          } else {
            gs = c ? gs + val : val;
            v.b[sl % NB][sl / NB] = 0.f;
          }
        }
        if constexpr (!member<MI>()) v.b[(C * gl) % NB][(C * gl) / NB] = gs;
      }
#pragma unroll
      for (int sl = C * Gl; sl < 16 * NB; ++sl) v.b[sl % NB][sl / NB] = 0.f;   // the lane's padding slots
      publish<NB>(sh.pub[1][w], lane, v);
    }
    pw_reduce<NB, kM, MI>(sh, wts, g, sub, member<MI>() ? jm : jg, member<MI>() ? G * C : G, lme, acc, bad);
    if constexpr (MI + 1 < kM) value<MI + 1>(u, sh, wts, w, h, lane, g, sub, lme, acc, bad);
  }
  __device__ __forceinline__ void values(const Tile<NB>& u, Shared<NB>& sh, const double* wts, int w, int h, int lane, int g, int sub,
                                         unsigned lme, PwAcc<kM>& acc, int& bad) const {
    value<0>(u, sh, wts, w, h, lane, g, sub, lme, acc, bad);
  }

  template <int MI>
  __device__ __forceinline__ void store_from(const PwArgs& a, double* red, size_t KP, int strip, int g, int sub, PwAcc<kM>& acc) const {
    pw_store_one<NB, kM, MI>(a, member<MI>() ? G * C : G, red, KP, strip, g, sub, member<MI>() ? jm : jg, acc);
    if constexpr (MI + 1 < kM) store_from<MI + 1>(a, red, KP, strip, g, sub, acc);
  }
  __device__ __forceinline__ void store(const PwArgs& a, double* red, size_t KP, int strip, int g, int sub, PwAcc<kM>& acc) const {
    store_from<0>(a, red, KP, strip, g, sub, acc);
  }
};

// a.part is [nstrips][4 M][KP], KP = G C when a value is per member and G otherwise; a per-group value fills its first G
// columns and the kernel never writes the rest (pointwise.hip keeps them empty)
template <int NB, int C, class H>
__device__ __forceinline__ void lin_group_pointwise_items(const PwArgs& a, const LinGroupedModel& gm, const PotLinear& lin,
                                                          Shared<NB>& sh, double* wts /* [32] LDS */) {
  static_assert(C >= 2 && C <= 16, "a group has 2 to 16 members");
  GpBlock<NB, C, H> bv{lin, gm.G};
  const size_t KP = H::kMemberMask ? (size_t)gm.G * C : (size_t)gm.G;
  pw_items<NB>(a, gm.W1b, gm.cb, gm.nbg, KP, bv, sh, wts);
}

}  // namespace mjhmc
