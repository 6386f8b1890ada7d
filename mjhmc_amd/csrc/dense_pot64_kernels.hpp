// The float64-state tile kernel's building blocks (the reference's arithmetic: float64 rows streamed through the epilogue
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

constexpr int kPark = 8;   // momentum elements per lane that sit out the GEMM loops in LDS (see pot64_trajectory)
template <int NB>
struct Shared64 {
  Shared<NB> s;
  double red64[4][kP];
  double zn[128 * NB];   // the float64 standard normals of one refreshing column (column_normals)
  f32x4 park[kPark / 2][256];
};

// The wave's working copy of its X and V elements between the passes of a trajectory, in the workgroup's scratch
// (2 x 32 x DIM float64): LANE-LINEAR pieces [wave][array][piece][lane] of 16 bytes (8 at NB = 1), so every access of the
// per-step passes is 64 lanes x 16 B = 1 KB contiguous.  In the particle-major rows themselves a wave instruction
// touches 64 different 128-byte lines (lane = particle, 4 KB apart): the address pipe takes ~64 cycles per instruction
// and, with 128 of them per wave and step, a first form that integrated in the rows spent 40 000 cycles per step there
// (C3 21.3 ms instead of 16.6).  Rows are touched once per trajectory, read and written through LDS (staged_start,
// staged_end_x, staged_end_vg).
// Accesses go through a buffer resource: scalar base + the lane's constant offset + a scalar piece offset.
template <int NB>
struct Work {
  static constexpr int PB = NB == 1 ? 8 : 16;        // piece bytes
  static constexpr int PQ = NB * 8 / PB;             // pieces per register index
  static constexpr unsigned kArea = 16u * PQ * 64u * PB;  // one wave's X (or V) elements: 8192 NB bytes
  __amdgpu_buffer_rsrc_t rs;
  unsigned voff;   // the lane's piece inside the wave's area: w * kArea + lane * PB (vector register)
  static constexpr unsigned xb = 0;   // X areas of the four waves, then (kept for a momentum working copy) the V areas
  static constexpr unsigned vb = 4 * kArea;
};
template <int NB>
__device__ __forceinline__ Work<NB> work_of(double* scratch, unsigned wg, int w, int lane) {
  Work<NB> k;
  char* base = (char*)scratch + (size_t)wg * (8 * Work<NB>::kArea);
  k.rs = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, 8 * Work<NB>::kArea, 0x00020000);
  // (the wave index is threadIdx-derived: a vector value to the compiler.  In the scalar offset of a buffer access it
  // would force a readfirstlane loop around every load and store)
  k.voff = (unsigned)w * Work<NB>::kArea + (unsigned)lane * Work<NB>::PB;
  return k;
}
using uvec4 = __attribute__((ext_vector_type(4))) unsigned;
using uvec2 = __attribute__((ext_vector_type(2))) unsigned;
using f64x2 = __attribute__((ext_vector_type(2))) double;
template <int NB>
__device__ __forceinline__ typename DVecN<NB>::type wk_load(const Work<NB>& k, unsigned area, int q) {
  if constexpr (NB == 1) {
    return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(k.rs, k.voff, area + (unsigned)q * 512u, 0));
  } else if constexpr (NB == 2) {
    return __builtin_bit_cast(f64x2, __builtin_amdgcn_raw_buffer_load_b128(k.rs, k.voff, area + (unsigned)q * 1024u, 0));
  } else {
    const f64x2 lo = __builtin_bit_cast(f64x2, __builtin_amdgcn_raw_buffer_load_b128(k.rs, k.voff, area + (unsigned)q * 2048u, 0));
    const f64x2 hi = __builtin_bit_cast(f64x2, __builtin_amdgcn_raw_buffer_load_b128(k.rs, k.voff, area + (unsigned)q * 2048u + 1024u, 0));
    typename DVecN<4>::type v;
    v[0] = lo[0];
    v[1] = lo[1];
    v[2] = hi[0];
    v[3] = hi[1];
    return v;
  }
}
template <int NB>
__device__ __forceinline__ void wk_store(const Work<NB>& k, unsigned area, int q, const typename DVecN<NB>::type& v) {
  if constexpr (NB == 1) {
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(uvec2, v), k.rs, k.voff, area + (unsigned)q * 512u, 0);
  } else if constexpr (NB == 2) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(uvec4, v), k.rs, k.voff, area + (unsigned)q * 1024u, 0);
  } else {
    f64x2 lo, hi;
    lo[0] = v[0];
    lo[1] = v[1];
    hi[0] = v[2];
    hi[1] = v[3];
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(uvec4, lo), k.rs, k.voff, area + (unsigned)q * 2048u, 0);
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(uvec4, hi), k.rs, k.voff, area + (unsigned)q * 2048u + 1024u, 0);
  }
}

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
  const int t = threadIdx.x;
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
  const int t = threadIdx.x;
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

// the wave's momentum elements, float64, in registers for the whole trajectory (accumulator layout: 2 x 16 NB registers)
template <int NB>
struct VTile {
  double b[NB][16];
};

// One kick / drift pass over this wave's elements of the tile.  The momentum stays in registers; the position is
// streamed through registers from the working copy in four chunks of four register indices (double buffered: chunk
// n + 1 is in flight while chunk n is worked on).
//   NKICK = 1: v = v + c g                          (the first step of a trajectory: v holds [-]V_in, staged_start)
//   NKICK = 2: v = (v + c g) + c g                  (closing half kick of a step, opening one of the next)
//   x = X + eps v ;  store x to the working copy ;  float32(x) -> the X image of GEMM 1
// (the last drift's X is the end point: the caller takes it from the working copy, staged_end_x)
// Every product is rounded before its sum (the library is built with -ffp-contract=off): NumPy's V += c * g.
template <int NB, int NKICK>
__device__ __forceinline__ void kick_drift_pass(const Work<NB>& wk, const Tile<NB>& g, VTile<NB>& v, double c, double eps,
                                                PubWave<NB>* pub0, int w, int lane) {
  using DV = typename DVecN<NB>::type;
  DV xa[4], xb[4];
  auto load4 = [&](int q4, DV(&x)[4]) {
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) x[qq] = wk_load<NB>(wk, wk.xb, 4 * q4 + qq);
  };
  // the momentum first: it needs no memory, so it runs while the X loads are in flight
  auto kick4 = [&](int q4) {
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) {
      const int q = 4 * q4 + qq;
#pragma unroll
      for (int r = 0; r < NB; ++r) {
        const double t = c * (double)g.b[r][q];
        double vv = v.b[r][q];
        vv = vv + t;
        if constexpr (NKICK == 2) vv = vv + t;
        v.b[r][q] = vv;
      }
    }
  };
  auto drift4 = [&](int q4, DV(&x)[4]) {
    f32x4 px[NB];
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) {
      const int q = 4 * q4 + qq;
#pragma unroll
      for (int r = 0; r < NB; ++r) {
        const double xx = dget<NB>(x[qq], r) + eps * v.b[r][q];
        dset<NB>(x[qq], r, xx);
        px[r][qq] = (float)xx;
      }
      wk_store<NB>(wk, wk.xb, q, x[qq]);
    }
    if constexpr (NB == 4) {
      // this lane's slot of the X image, formed from the working copy's lane offset (which every load and store of the
      // pass holds in a register anyway): voff = w * 32 KB + lane * 16 -> w * 16 KB + lane * 16.  As a loop-invariant
      // address it was one more value held -- in scratch -- across the GEMM loops, and its reload in front of the first
      // publish of a pass stood behind an s_waitcnt vmcnt(0) that drained the pass's loads.
      unsigned off = ((wk.voff >> 1) & 0xFFFFC000u) | (wk.voff & 0x3FFu);
      asm volatile("" : "+v"(off));
      char* img = reinterpret_cast<char*>(pub0) + off;
#pragma unroll
      for (int r = 0; r < NB; ++r) *reinterpret_cast<f32x4*>(img + (size_t)(r * 4 + q4) * 1024) = px[r];
    } else {
#pragma unroll
      for (int r = 0; r < NB; ++r) pub0[w].v[r][q4][lane] = px[r];
    }
  };
  // (Measured: all four kick4 first, in the shadow of the first X loads, then the drifts -- more registers live across
  // the pass, 119 -> 283 spilled, C3 in this arithmetic 17.6 -> 18.7 ms.)
  load4(0, xa);
  load4(1, xb);
  __builtin_amdgcn_sched_barrier(0);
  kick4(0);
  drift4(0, xa);
  __builtin_amdgcn_sched_barrier(0);
  load4(2, xa);
  __builtin_amdgcn_sched_barrier(0);
  kick4(1);
  drift4(1, xb);
  __builtin_amdgcn_sched_barrier(0);
  load4(3, xb);
  __builtin_amdgcn_sched_barrier(0);
  kick4(2);
  drift4(2, xa);
  __builtin_amdgcn_sched_barrier(0);
  kick4(3);
  drift4(3, xb);
}

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

// The start of a trajectory: the tile's rows (p: this lane's column's particle) through the staging image -- X into the
// working copy, the stored dE/dX (float64 rows holding float32 values) into g, [-]V into v (neg: the F of F L F).
// Barriers: the image is free on entry (the caller's last read of it stands behind a barrier) and on return.
template <int NB>
__device__ __forceinline__ void staged_start(Shared<NB>& s, const Work<NB>& wk, const double* xin, const double* vin,
                                             const double* gin, int64_t p, int w, int c, int h, Tile<NB>& g, VTile<NB>& v,
                                             bool neg) {
  char* img = stage_image<NB>(s);
  stage_rows_in<NB>(xin, p, img);
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 16; ++q) wk_store<NB>(wk, wk.xb, q, stage_get<NB>(img, w, c, h, q));
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

// Rows out through the staging image: the end point's position (from the working copy, where the last drift left it),
// its momentum, its dE/dX.  Barriers as staged_start's.
template <int NB>
__device__ __forceinline__ void staged_end_x(Shared<NB>& s, const Work<NB>& wk, double* xout, int64_t p, int w, int c, int h) {
  char* img = stage_image<NB>(s);
#pragma unroll
  for (int q = 0; q < 16; ++q) stage_put<NB>(img, w, c, h, q, wk_load<NB>(wk, wk.xb, q));
  __syncthreads();
  stage_rows_out<NB>(xout, p, img);
  __syncthreads();
}
template <int NB>
__device__ __forceinline__ void staged_end_vg(Shared<NB>& s, double* vout, double* gout, int64_t p, int w, int c, int h,
                                              const VTile<NB>& v, const Tile<NB>& g) {
  using DV = typename DVecN<NB>::type;
  char* img = stage_image<NB>(s);
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

// L >= 1 leapfrog steps (hmc_state.py:86-100) from the position in the working copy, the momentum in v and the stored
// dE/dX in g (staged_start).  On return the end point's position is in the working copy (staged_end_x takes it to the
// rows), its momentum in v, g holds its dE/dX (float32), *ex its energy (float32, from the last gradient's u), and the
// return value is its kinetic energy sum(V^2) / 2 (all lanes of column c).
template <int NB, class XP>
__device__ __forceinline__ double pot64_trajectory(const PotModel& mdl, const XP& xp, AReg<NB>& ar, Shared64<NB>& sh, int w, int c, int h,
                                                   int lane, const Work<NB>& wk, Tile<NB>& g, VTile<NB>& v, int L, double eps,
                                                   double chalf, float* ex) {
  PubWave<NB>* pub0 = sh.s.pub[0];   // the X images of the four waves (this wave's: pub0[w])
  kick_drift_pass<NB, 1>(wk, g, v, chalf, eps, pub0, w, lane);
  for (int s = 0; s < L; ++s) {
    [[maybe_unused]] const int stamp_slot = s;
    POT_STAMP(0);
    // The momentum (32 NB registers) is not touched by the gradient, whose GEMM loops run at the register budget: the
    // allocator spills a few of its elements across them and reloads them inside the streamed pass, where a scratch
    // reload is a counted load whose wait drains the pass's own loads.  A few elements sit the gradient out in LDS
    // instead (lane-linear, conflict-free; an LDS wait drains nothing).
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
      // the pass's loads, not between them)
#pragma unroll
      for (int r = 0; r < NB; ++r)
#pragma unroll
        for (int q = 0; q < 16; ++q) use_here(v.b[r][q]);
    }
    POT_STAMP(6);
    if (s < L - 1) kick_drift_pass<NB, 2>(wk, g, v, chalf, eps, pub0, w, lane);
    POT_STAMP(7);
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
