// The float64-state tile kernel's building blocks (the reference's arithmetic: float64 register tiles integrated in the epilogue
// around the float32 force; dense_pot64.hip has the design), the trajectory templated on the experts of the force
// (dense_pot_tile.hpp).  The kernel's body is the fragment dense_pot64_jump.inc, included inside the kernel definition:
// ProductOfT's pot64_jump_kernel in dense_pot64.hip, a linear-model energy's in linear_energy.hip's hipRTC unit.
#pragma once
#ifndef __HIPCC_RTC__  // hipRTC pre-includes the device runtime (linear_energy.hip)
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#include "dense_pot.hpp"
#include "dense_pot_tile.hpp"
#include "group_form.hpp"  // use_here

namespace mjhmc {

template <int NB>
struct DVecN;
template <>
struct DVecN<1> {
  using type = double;
};
template <>
struct DVecN<2> {
  using type = __attribute__((ext_vector_type(2))) double;
};
template <>
struct DVecN<4> {
  using type = __attribute__((ext_vector_type(4))) double;
};
template <int NB>
__device__ __forceinline__ double dget(const typename DVecN<NB>::type& v, int r) {
  if constexpr (NB == 1) return v;
  else return v[r];
}
template <int NB>
__device__ __forceinline__ void dset(typename DVecN<NB>::type& v, int r, double x) {
  if constexpr (NB == 1) v = x;
  else v[r] = x;
}

// A lane's elements of particle row `row` ([*][DIM] float64): register index q <-> NB consecutive doubles at
// row + 32 NB w + NB acc_row(q, h).  The (w, h) part is folded into the lane's base pointer, the q part is an
// immediate offset of the load.
template <int NB>
__device__ __forceinline__ int q_off(int q) { return NB * ((q & 3) + 8 * (q >> 2)); }
template <int NB>
__device__ __forceinline__ const double* lane_row(const double* base, int64_t p, int w, int h) {
  return base + (size_t)p * (128 * NB) + 32 * NB * w + 4 * NB * h;
}
template <int NB>
__device__ __forceinline__ double* lane_row(double* base, int64_t p, int w, int h) {
  return base + (size_t)p * (128 * NB) + 32 * NB * w + 4 * NB * h;
}
template <int NB>
__device__ __forceinline__ typename DVecN<NB>::type dv_load(const double* lrow, int q) {
  return *reinterpret_cast<const typename DVecN<NB>::type*>(lrow + q_off<NB>(q));
}
template <int NB>
__device__ __forceinline__ void dv_store(double* lrow, int q, const typename DVecN<NB>::type& v) {
  *reinterpret_cast<typename DVecN<NB>::type*>(lrow + q_off<NB>(q)) = v;
}

// A rows per register set of the GEMMs (dense_pot_tile.hpp): NB = 4 runs the half-depth form, gemm_dim_half -- its 64
// registers are what lets the position live in registers; NB = 1, 2 have registers to spare and keep whole chunks
template <int NB>
constexpr int kA64 = NB == 4 ? 8 : 16;
template <int NB>
using AReg64 = AReg<NB, kA64<NB>>;

constexpr int kPark = 8;   // momentum elements per lane that sit out the GEMM loops in LDS (see pot64_trajectory)
template <int NB>
struct Shared64 {
  Shared<NB> s;
  double red64[4][kP];
  double zn[128 * NB];   // the float64 standard normals of one refreshing column (column_normals)
  f32x4 park[kPark / 2][256];
};

using uvec4 = __attribute__((ext_vector_type(4))) unsigned;
using f64x2 = __attribute__((ext_vector_type(2))) double;

// The particle rows at the two ends of a trajectory, staged through the B-operand images (Shared<NB>::pub: 32 KB x NB,
// exactly the tile's 32 rows of DIM float64), which are idle there.  Read in the lanes' own accumulator layout a wave
// instruction touches 64 rows 4 KB apart (64 cache lines: ~64 cycles of the address pipe); staged, every wave
// instruction moves a contiguous 1 KB (512 B at NB = 1) of ONE row, and the lanes take or leave their elements in LDS.
// LDS image: row-major, piece (16 B; 8 at NB = 1) k of row c at c * 1024 NB + (k ^ (c & 15)) * PB -- the XOR spreads the
// 32 rows' elements of one register index over the banks (row starts are bank-aligned).
template <int NB>
struct PieceOf {
  using type = uvec4;
};
template <>
struct PieceOf<1> {
  using type = unsigned long long;
};
// A lane constant the compiler must form where it is used.  The staging addresses below are functions of the thread
// index alone: hoisted out of the kernel's item loop they are ~45 values held across every trajectory, and the kernel has
// no register for them (they went to scratch, each reload awaited on its own in front of its LDS access); formed in place
// they are two vector instructions per piece.
__device__ __forceinline__ int here(int lane_const) {
  asm volatile("" : "+v"(lane_const));
  return lane_const;
}
template <int NB>
struct Stage {
  using P = typename PieceOf<NB>::type;
  static constexpr int PB = sizeof(P);               // piece bytes
  static constexpr int RB = 1024 * NB;               // row bytes
  static constexpr int RP = RB / PB;                 // pieces per row: a multiple of 64 (a wave instruction: one row)
  static constexpr int K = 32 * RP / 256;            // pieces per thread and array: 16 (NB = 1, 2), 32 (NB = 4)
  static constexpr int KB = K < 16 ? K : 16;         // requests in flight per thread
};
__device__ __forceinline__ unsigned stage_addr(int row, int piece, int pb, int rb) {
  return (unsigned)(row * rb + ((piece ^ (row & 15)) * pb));
}
// rows [p(c)] of `rows` ([*][DIM] float64; p: this lane's column's particle, columns = lanes 0..31) -> LDS image
template <int NB>
__device__ __forceinline__ void stage_rows_in(const double* rows, int64_t p, char* img) {
  using S = Stage<NB>;
  using P = typename S::P;
  const int t = here(threadIdx.x);
#pragma unroll 1
  for (int i0 = 0; i0 < S::K; i0 += S::KB) {
    P buf[S::KB];
#pragma unroll
    for (int i = 0; i < S::KB; ++i) {
      const int k = (i0 + i) * 256 + t, row = k / S::RP, piece = k % S::RP;   // (row: uniform over the wave)
      const int64_t pr = __shfl((long long)p, row);
      buf[i] = *reinterpret_cast<const P*>(reinterpret_cast<const char*>(rows) + (size_t)pr * S::RB + (size_t)piece * S::PB);
    }
#pragma unroll
    for (int i = 0; i < S::KB; ++i) {
      const int k = (i0 + i) * 256 + t, row = k / S::RP, piece = k % S::RP;
      *reinterpret_cast<P*>(img + stage_addr(row, piece, S::PB, S::RB)) = buf[i];
    }
  }
}
// LDS image -> rows [p(c)] of `rows`
template <int NB>
__device__ __forceinline__ void stage_rows_out(double* rows, int64_t p, const char* img) {
  using S = Stage<NB>;
  using P = typename S::P;
  const int t = here(threadIdx.x);
#pragma unroll 1
  for (int i0 = 0; i0 < S::K; i0 += S::KB) {
#pragma unroll
    for (int i = 0; i < S::KB; ++i) {
      const int k = (i0 + i) * 256 + t, row = k / S::RP, piece = k % S::RP;
      const int64_t pr = __shfl((long long)p, row);
      *reinterpret_cast<P*>(reinterpret_cast<char*>(rows) + (size_t)pr * S::RB + (size_t)piece * S::PB) =
          *reinterpret_cast<const P*>(img + stage_addr(row, piece, S::PB, S::RB));
    }
  }
}
// this lane's NB doubles of register index q in the LDS image (its column's row, the accumulator layout's elements)
template <int NB>
__device__ __forceinline__ typename DVecN<NB>::type stage_get(const char* img, int w, int c, int h, int q) {
  using S = Stage<NB>;
  const int first = (8 * NB * (32 * w + acc_row(q, h))) / S::PB;
  if constexpr (NB == 4) {
    const f64x2 lo = *reinterpret_cast<const f64x2*>(img + stage_addr(c, first, S::PB, S::RB));
    const f64x2 hi = *reinterpret_cast<const f64x2*>(img + stage_addr(c, first + 1, S::PB, S::RB));
    typename DVecN<4>::type v;
    v[0] = lo[0];
    v[1] = lo[1];
    v[2] = hi[0];
    v[3] = hi[1];
    return v;
  } else {
    return *reinterpret_cast<const typename DVecN<NB>::type*>(img + stage_addr(c, first, S::PB, S::RB));
  }
}
template <int NB>
__device__ __forceinline__ void stage_put(char* img, int w, int c, int h, int q, const typename DVecN<NB>::type& v) {
  using S = Stage<NB>;
  const int first = (8 * NB * (32 * w + acc_row(q, h))) / S::PB;
  if constexpr (NB == 4) {
    f64x2 lo, hi;
    lo[0] = v[0];
    lo[1] = v[1];
    hi[0] = v[2];
    hi[1] = v[3];
    *reinterpret_cast<f64x2*>(img + stage_addr(c, first, S::PB, S::RB)) = lo;
    *reinterpret_cast<f64x2*>(img + stage_addr(c, first + 1, S::PB, S::RB)) = hi;
  } else {
    *reinterpret_cast<typename DVecN<NB>::type*>(img + stage_addr(c, first, S::PB, S::RB)) = v;
  }
}
template <int NB>
__device__ __forceinline__ char* stage_image(Shared<NB>& s) {
  static_assert(sizeof(s.pub) == 32 * Stage<NB>::RB, "the staging image is the two B-operand images");
  return reinterpret_cast<char*>(&s.pub[0][0]);
}

// the wave's elements of a float64 state array in registers for the whole trajectory (accumulator layout: 2 x 16 NB
// registers): the momentum and the position
template <int NB>
struct VTile {
  double b[NB][16];
};

// One kick / drift pass over this wave's elements of the tile, in registers alone:
//   NKICK = 1: v = v + c g                          (the first step of a trajectory: v holds [-]V_in, staged_start)
//   NKICK = 2: v = (v + c g) + c g                  (closing half kick of a step, opening one of the next)
//   x = x + eps v ;  float32(x) -> this lane's slot of the X image of GEMM 1
// (the last drift's x is the end point: staged_end_x takes it to the rows)
// Every product is rounded before its sum (the library is built with -ffp-contract=off): NumPy's V += c * g.
// (A form that streamed the position through a per-workgroup working copy in memory, 128 KB in and out per step at
// NB = 4, took ~6 000 cycles per pass: DESIGN.md 3.4b.)
// DONE: elements q < DONE (a multiple of four) of blocks 0 .. NB - 2 have had their pass already (StepTail)
template <int NB, int NKICK, int DONE = 0>
__device__ __forceinline__ void kick_drift_pass(const Tile<NB>& g, VTile<NB>& v, VTile<NB>& x, double c, double eps,
                                                PubWave<NB>* pub0, int w, int lane) {
#pragma unroll
  for (int q4 = 0; q4 < 4; ++q4) {
    f32x4 px[NB];
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) {
      const int q = 4 * q4 + qq;
#pragma unroll
      for (int r = 0; r < NB; ++r) {
        if (r < NB - 1 && q < DONE) continue;
        const double t = c * (double)g.b[r][q];
        double vv = v.b[r][q];
        vv = vv + t;
        if constexpr (NKICK == 2) vv = vv + t;
        v.b[r][q] = vv;
        const double xx = x.b[r][q] + eps * vv;
        x.b[r][q] = xx;
        px[r][qq] = (float)xx;
      }
    }
#pragma unroll
    for (int r = 0; r < NB; ++r)
      if (!(r < NB - 1 && 4 * q4 < DONE)) pub0[w].v[r][q4][lane] = px[r];
    __builtin_amdgcn_sched_barrier(0);   // chunk by chunk: what is live beside the tiles stays one chunk's temporaries
  }
}

// The middle steps' pass under GEMM 2's last MFMAs (dense_pot_tile.hpp: half_mfma_tail, NoTail): block rb's dE/dX is
// final while blocks rb + 1 .. NB - 1 still accumulate, so its elements are kicked, drifted, rounded and written to the X
// image between their MFMAs -- kPass elements per gap, the same operations on the same values as kick_drift_pass<NB, 2>.
// Block NB - 1 (whose parked momentum is in LDS meanwhile) and what the gaps do not hold stay behind the GEMM:
// kick_drift_pass<NB, 2, kDone>.  kPhi: the same for phi under GEMM 1.
template <bool B>
struct Flag {   // a compile-time switch passed as an argument
  static constexpr bool value = B;
};

template <int NB>
struct StepTail {
  static constexpr bool kOn = true, kFill = true;
  static constexpr int kPhi = 1, kPass = 1;
  static constexpr int kDone = 8 * kPass;
  VTile<NB>& v;
  VTile<NB>& x;
  double c, eps;
  PubWave<NB>& pubw;  // this wave's X image
  int lane;
  f32x4& px;          // the quad being collected
  __device__ __forceinline__ void pass_slice(const Tile<NB>& g, int rb, int j) const {
#pragma unroll
    for (int e = 0; e < kPass; ++e) {
      const int q = kPass * j + e;
      const double t = c * (double)g.b[rb][q];
      double vv = v.b[rb][q];
      vv = vv + t;
      vv = vv + t;
      v.b[rb][q] = vv;
      const double xx = x.b[rb][q] + eps * vv;
      x.b[rb][q] = xx;
      px[q & 3] = (float)xx;
      if ((q & 3) == 3) pubw.v[rb][q >> 2][lane] = px;
    }
  }
};

// The closing half kick of the trajectory, v += c g, and this lane's part of sum(v^2)
template <int NB>
__device__ __forceinline__ double closing_kick(const Tile<NB>& g, VTile<NB>& v, double c) {
  double s = 0.0;
#pragma unroll
  for (int q = 0; q < 16; ++q)
#pragma unroll
    for (int r = 0; r < NB; ++r) {
      const double vv = v.b[r][q] + c * (double)g.b[r][q];
      v.b[r][q] = vv;
      s = s + vv * vv;
    }
  return s;
}

// sum over the tile's 4 waves x 2 lane halves of a per-lane partial; every lane of column c gets the total.
// One barrier pair.
template <int NB, class SH>
__device__ __forceinline__ double column_sum(SH& sh, int w, int c, int h, double part) {
  const double both = swap32_sum(part);
  if (h == 0) sh.red64[w][c] = both;
  __syncthreads();
  const double tot = sh.red64[0][c] + sh.red64[1][c] + sh.red64[2][c] + sh.red64[3][c];
  __syncthreads();
  return tot;
}

// The start of a trajectory: the tile's rows (p: this lane's column's particle) through the staging image -- X into
// x, the stored dE/dX (float64 rows holding float32 values) into g, [-]V into v (neg: the F of F L F).
// Barriers: the image is free on entry (the caller's last read of it stands behind a barrier) and on return.
template <int NB>
__device__ __forceinline__ void staged_start(Shared<NB>& s, const double* xin, const double* vin, const double* gin, int64_t p,
                                             int w, int c, int h, Tile<NB>& g, VTile<NB>& v, VTile<NB>& x, bool neg) {
  char* img = stage_image<NB>(s);
  c = here(c), w = here(w), h = here(h);
  stage_rows_in<NB>(xin, p, img);
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const typename DVecN<NB>::type xx = stage_get<NB>(img, w, c, h, q);
#pragma unroll
    for (int r = 0; r < NB; ++r) x.b[r][q] = dget<NB>(xx, r);
  }
  __syncthreads();
  stage_rows_in<NB>(gin, p, img);
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const typename DVecN<NB>::type gg = stage_get<NB>(img, w, c, h, q);
#pragma unroll
    for (int r = 0; r < NB; ++r) g.b[r][q] = (float)dget<NB>(gg, r);
  }
  __syncthreads();
  stage_rows_in<NB>(vin, p, img);
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const typename DVecN<NB>::type vv = stage_get<NB>(img, w, c, h, q);
#pragma unroll
    for (int r = 0; r < NB; ++r) v.b[r][q] = neg ? -dget<NB>(vv, r) : dget<NB>(vv, r);   // (uniform: an inverse-L item)
  }
  __syncthreads();
}

// Rows out through the staging image: the end point's position (the tile the last drift left), its momentum, its
// dE/dX.  Barriers as staged_start's.
template <int NB>
__device__ __forceinline__ void staged_end_x(Shared<NB>& s, double* xout, int64_t p, int w, int c, int h, const VTile<NB>& x) {
  char* img = stage_image<NB>(s);
  c = here(c), w = here(w), h = here(h);
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    typename DVecN<NB>::type xx;
#pragma unroll
    for (int r = 0; r < NB; ++r) dset<NB>(xx, r, x.b[r][q]);
    stage_put<NB>(img, w, c, h, q, xx);
  }
  __syncthreads();
  stage_rows_out<NB>(xout, p, img);
  __syncthreads();
}
template <int NB>
__device__ __forceinline__ void staged_end_vg(Shared<NB>& s, double* vout, double* gout, int64_t p, int w, int c, int h,
                                              const VTile<NB>& v, const Tile<NB>& g) {
  using DV = typename DVecN<NB>::type;
  char* img = stage_image<NB>(s);
  c = here(c), w = here(w), h = here(h);
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    DV vv;
#pragma unroll
    for (int r = 0; r < NB; ++r) dset<NB>(vv, r, v.b[r][q]);
    stage_put<NB>(img, w, c, h, q, vv);
  }
  __syncthreads();
  stage_rows_out<NB>(vout, p, img);
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    DV gg;
#pragma unroll
    for (int r = 0; r < NB; ++r) dset<NB>(gg, r, (double)g.b[r][q]);
    stage_put<NB>(img, w, c, h, q, gg);
  }
  __syncthreads();
  stage_rows_out<NB>(gout, p, img);
  __syncthreads();
}

// L >= 1 leapfrog steps (hmc_state.py:86-100) from the position in x, the momentum in v and the stored dE/dX in g
// (staged_start).  On return the end point's position is in x (staged_end_x takes it to the rows), its momentum in v,
// g holds its dE/dX (float32), *ex its energy (float32, from the last gradient's u), and the return value is its
// kinetic energy sum(V^2) / 2 (all lanes of column c).
template <int NB, class XP>
__device__ __forceinline__ double pot64_trajectory(const PotModel& mdl, const XP& xp, AReg64<NB>& ar, Shared64<NB>& sh, int w, int c, int h,
                                                   int lane, Tile<NB>& g, VTile<NB>& v, VTile<NB>& x, int L, double eps,
                                                   double chalf, float* ex) {
  PubWave<NB>* pub0 = sh.s.pub[0];   // the X images of the four waves (this wave's: pub0[w])
  constexpr bool kTail = XP::kProductOfT && NB == 4 && kA64<NB> == 8;   // per-step vector work under the GEMMs' tails
  kick_drift_pass<NB, 1>(g, v, x, chalf, eps, pub0, w, lane);
  if constexpr (kTail) {
    // The middle steps and the last one apart: the last gradient has no pass behind it and wants the energy.  (One loop
    // with the work under the tails behind a branch on the step number per MFMA gap: 140 spilled registers.)
    // TAIL: a middle step's gradient, phi and the pass of the finished blocks under the GEMMs' last MFMAs (StepTail).
    // The momentum elements of kPark sit it out in LDS, as below.
    auto gradient = [&](auto tail, [[maybe_unused]] int stamp_slot) {
      POT_STAMP(0);
#pragma unroll
      for (int k = 0; k < kPark / 2; ++k) {
        f64x2 two;
        two[0] = v.b[NB - 1][15 - 2 * k];
        two[1] = v.b[NB - 1][14 - 2 * k];
        sh.park[k][threadIdx.x] = __builtin_bit_cast(f32x4, two);
      }
      if constexpr (decltype(tail)::value) {
        f32x4 px;
        pot_gradient_published<NB>(mdl, xp, ar, sh.s, w, c, h, lane, g, false, ex, stamp_slot,
                                   StepTail<NB>{v, x, chalf, eps, pub0[w], lane, px});
      } else {
        pot_gradient_published<NB>(mdl, xp, ar, sh.s, w, c, h, lane, g, true, ex, stamp_slot, BlockTail());
      }
#pragma unroll
      for (int k = 0; k < kPark / 2; ++k) {
        const f64x2 two = __builtin_bit_cast(f64x2, sh.park[k][threadIdx.x]);
        v.b[NB - 1][15 - 2 * k] = two[0];
        v.b[NB - 1][14 - 2 * k] = two[1];
      }
#pragma unroll
      for (int r = 0; r < NB; ++r)
#pragma unroll
        for (int q = 0; q < 16; ++q) use_here(v.b[r][q]);
      POT_STAMP(6);
    };
    for (int s = 0; s < L - 1; ++s) {
      gradient(Flag<true>{}, s);
      kick_drift_pass<NB, 2, StepTail<NB>::kDone>(g, v, x, chalf, eps, pub0, w, lane);
      [[maybe_unused]] const int stamp_slot = s;
      POT_STAMP(7);
    }
    gradient(Flag<false>{}, L - 1);
  } else {
  for (int s = 0; s < L; ++s) {
    [[maybe_unused]] const int stamp_slot = s;
    POT_STAMP(0);
    // Neither the momentum nor the position (2 x 32 NB registers) is touched by the gradient, whose GEMM loops run at
    // the register budget.  A few momentum elements sit the gradient out in LDS (lane-linear, conflict-free): without
    // them the allocator keeps as many values in scratch across the whole trajectory (the bench instance: 33 spilled
    // registers, a step 700 cycles longer, nearly all of it in GEMM 2: 70 140 against 69 480; with them: none).
    if constexpr (NB == 4) {
#pragma unroll
      for (int k = 0; k < kPark / 2; ++k) {
        f64x2 two;
        two[0] = v.b[NB - 1][15 - 2 * k];
        two[1] = v.b[NB - 1][14 - 2 * k];
        sh.park[k][threadIdx.x] = __builtin_bit_cast(f32x4, two);
      }
    }
    pot_gradient_published<NB>(mdl, xp, ar, sh.s, w, c, h, lane, g, s == L - 1, ex, s);
    if constexpr (NB == 4) {
#pragma unroll
      for (int k = 0; k < kPark / 2; ++k) {
        const f64x2 two = __builtin_bit_cast(f64x2, sh.park[k][threadIdx.x]);
        v.b[NB - 1][15 - 2 * k] = two[0];
        v.b[NB - 1][14 - 2 * k] = two[1];
      }
      // (whatever the allocator still keeps of the momentum in scratch across the GEMM loops comes back HERE, in front of
      // the pass, not inside it)
#pragma unroll
      for (int r = 0; r < NB; ++r)
#pragma unroll
        for (int q = 0; q < 16; ++q) use_here(v.b[r][q]);
    }
    POT_STAMP(6);
    if (s < L - 1) kick_drift_pass<NB, 2>(g, v, x, chalf, eps, pub0, w, lane);
    POT_STAMP(7);
  }
  }
  const double part = closing_kick<NB>(g, v, chalf);
  return column_sum<NB>(sh, w, c, h, part) / 2.0;
}


// what the kernel that only DECIDES and finishes the moves needs of Shared64 (pot64_decide_kernel)
template <int NB>
struct Finish64Shared {
  struct {
    int move[kP];
  } s;
  double red64[4][kP];
  double zn[128 * NB];
};

// The successor's rows once the moves of a tile's columns stand in sh.s.move.  FIX = false (jump kernel): the end point's
// position is in the output rows, its momentum in v, its dE/dX in g.  FIX = true (pot64_decide_kernel): columns that keep the
// end point are finished already (v, g unused); only the others are touched.  roff: this lane's elements of its column's row.
template <int NB, bool REPLAY, int MODE, bool FIX, class SH>
__device__ __forceinline__ void pot64_finish(const Pot64JumpArgs& a, SH& sh, int64_t p, bool alive, size_t roff, int w, int c,
                                             int h, const VTile<NB>& v, const Tile<NB>& g) {
  using DV = typename DVecN<NB>::type;
  const double* xin = a.X_in + roff;
  const double* vin = a.V_in + roff;
  const double* gin = a.G_in + roff;
  double* xo = a.X_out + roff;
  double* vo = a.V_out + roff;
  double* go = a.G_out + roff;
  const int mv = sh.s.move[c];
  const int k = mv & 3;
  bool take, flip, refresh;  // keep the end point of L; negate the successor's momentum; redraw it (HMCState.R)
  if constexpr (MODE == kModeControl) {
    const bool accept = k & 1, fl = k & 2;
    take = accept;
    flip = accept != fl;      // accepted: L F, then possibly F again; rejected: possibly F (markov_jump_hmc.py:116-141)
    refresh = (mv & 4) != 0;  // batch-wide (:138-141)
  } else {
    take = k == 0;
    flip = (MODE == kModeCT && k == 0) || k == 1;  // CT's FL move ends with a flip (:258,278); F flips
    refresh = k == 2;
  }
  // the successor's rows.  A kept end point: position already in the output rows, momentum from the registers
  // (negated where the move ends with a flip), dE/dX from the accumulator; everything else: the pre-move position and
  // dE/dX, and in the second loop its momentum, flipped / refreshed
  const bool tile_refreshes = __ballot(refresh) != 0ull;
  if (!FIX || !take) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      DV gg;
      if (take) {
        if constexpr (!FIX) {
          DV vv;
#pragma unroll
          for (int r = 0; r < NB; ++r) {
            dset<NB>(vv, r, flip ? -v.b[r][q] : v.b[r][q]);
            dset<NB>(gg, r, (double)g.b[r][q]);
          }
          dv_store<NB>(vo, q, vv);
        }
      } else {
        gg = dv_load<NB>(gin, q);
        dv_store<NB>(xo, q, dv_load<NB>(xin, q));
      }
      dv_store<NB>(go, q, gg);
    }
  }
  double s2 = 0.0;
  if (!take || (REPLAY && refresh)) {
    const double* vsrc = take ? (const double*)vo : vin;   // (a kept end point's momentum is flipped already)
    const bool fl2 = flip && !take;
    const double* nrow = REPLAY ? lane_row<NB>(a.noise, alive ? p : 0, w, h) : nullptr;
#pragma unroll 1
    for (int q = 0; q < 16; ++q) {
      DV vv = dv_load<NB>(vsrc, q);
      if (fl2) vv = -vv;
      if constexpr (REPLAY) {
        if (refresh) {  // HMCState.R (hmc_state.py:121-129) with the recorded normals
          const DV z = dv_load<NB>(nrow, q);
#pragma unroll
          for (int r = 0; r < NB; ++r) {
            const double t = dget<NB>(vv, r) * a.r_keep + dget<NB>(z, r) * a.r_mix;
            dset<NB>(vv, r, t);
            s2 = s2 + t * t;
          }
        }
      }
      dv_store<NB>(vo, q, vv);
    }
  }
  if constexpr (!REPLAY) {
    // HMCState.R, column by column (the set is the same in every wave: it comes from sh.move), the whole workgroup
    // drawing the column's normals (column_normals); the column's momentum is in the output rows by now
    unsigned cols = (unsigned)(__ballot(refresh) & 0xFFFFFFFFull);
    while (cols) {
      const int c0 = __ffs((int)cols) - 1;
      cols &= cols - 1;
      const int64_t p0 = __shfl((long long)p, c0);
      column_normals<NB, double>(a.key, (uint32_t)(a.first_pid + (p0 < a.N ? p0 : 0)), a.D, sh.zn);
      __syncthreads();
      if (c == c0) {
        const double* zrow = sh.zn + 32 * NB * w + 4 * NB * h;
#pragma unroll 1
        for (int q = 0; q < 16; ++q) {
          DV vv = dv_load<NB>(vo, q);
          const DV z = *reinterpret_cast<const DV*>(zrow + q_off<NB>(q));
#pragma unroll
          for (int r = 0; r < NB; ++r) {
            const double t = dget<NB>(vv, r) * a.r_keep + dget<NB>(z, r) * a.r_mix;
            dset<NB>(vv, r, t);
            s2 = s2 + t * t;
          }
          dv_store<NB>(vo, q, vv);
        }
      }
      __syncthreads();
    }
  }
  if (tile_refreshes) {  // all waves take part in the reduction; only refreshed columns use the result
    const double evr = column_sum<NB>(sh, w, c, h, s2) / 2.0;
    if (refresh && w == 0 && h == 0) a.EV_out[p] = evr;
  }
}

// rates / acceptance, waiting times, first minimum of ONE particle by one lane, with the device functions of the
// elementwise kernels in their one-lane-per-particle forms (as hk_decide of the multi-pass path)
template <bool REPLAY, int MODE>
__device__ __forceinline__ int pot64_decide(const Pot64JumpArgs& a, double H0, double HL, double Hflf, int64_t pp, uint32_t pid,
                                            double& best, bool& bad, bool& gate) {
  JumpArgs<double> ja;
  ja.p_r = a.p_r;
  ja.p_flip = a.p_flip;
  ja.rexp = a.rexp;
  ja.runif = a.runif;
  ja.N = a.N;
  const LaneMap m = LaneMap::one_lane();
  int k = 0;
  if constexpr (MODE == kModeMJHMC) {
    decide<double, REPLAY>(ja, a.key, m, H0, HL, Hflf, pp, pid, k, best, bad);
  } else if constexpr (MODE == kModeCT) {
    decide_ct<double, REPLAY>(ja, a.key, m, H0, HL, pp, pid, k, best, bad);
  } else {
    double uacc, uflip, ugate;
    if constexpr (REPLAY) {
      uacc = a.runif[pp];
      uflip = a.runif[a.N + pp];
      ugate = a.runif[2 * a.N];
    } else {
      const u32x4 q = philox4x32_10(pid, a.key.tick_lo, a.key.tick_hi, kSlotExpR, a.key.k0, a.key.k1);
      const u32x4 f = philox4x32_10(pid, a.key.tick_lo, a.key.tick_hi, kSlotFlip, a.key.k0, a.key.k1);
      const u32x4 gq = philox4x32_10(0xFFFFFFFFu, a.key.tick_lo, a.key.tick_hi, kSlotFlip, a.key.k0, a.key.k1);
      uacc = u53(q.w2, q.w3);
      uflip = u53(f.w0, f.w1);
      ugate = u53(gq.w2, gq.w3);
    }
    const double dH = H0 - HL;
    const bool accept = !(dH < 0.0) || (uacc < exp(dH));
    const bool flip = uflip < a.p_flip;
    gate = ugate < a.p_r;
    k = (accept ? 1 : 0) | (flip ? 2 : 0);
  }
  return k;
}


}  // namespace mjhmc
