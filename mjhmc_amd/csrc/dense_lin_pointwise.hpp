// Per-expert statistics of a linear-model energy over a recorded ensemble: the TRANSPOSE of the
// tall force kernel (dense_lin_tall.hpp).  Both form u = W x + b on fp32 MFMA block of experts by block of experts; the
// force sums over experts per particle, this pass sums over particles per expert.  Per expert j < K, value m < M and the
// particles p < N of one ring slot, with t = (double)h_m(u_j, j; p, q) widened exactly and w the particle's weight:
//     S1 += w t      S2 += (w t) t      (mx, se): mx = max t over w > 0, se = sum w exp(t - mx)   [where the mask asks]
// u never leaves the chip: GEMM 1 of the tile kernels (dense_pot_tile.hpp) leaves it in the accumulator registers, the
// caller's values go through the LDS image the force's phi(u) would take (sh.pub[1]) and are summed from there.
//
// Work item = (strip of kPwStripTiles tiles of 32 particles, block of P = 128 NB experts).  Within an item:
//   * the block's b -> sh.cb and its W1 rows (NB = 1: all of them, register resident; NB > 1: chunk 0, handed from GEMM to
//     GEMM by gemm_dim) once; then the strip's tiles in ascending order;
//   * per tile: x published, u = cb + W1^T x, and per value m: h_m(u) published (float32), barrier, the
//     reduction below, barrier;
//   * reduction over a tile's 32 particles: the image holds 32 NB groups of four experts (one float4 per particle); thread
//     (g, sub) = (tid % (32 NB), tid / (32 NB)) owns group g and the 4 NB particles [4 NB sub, 4 NB (sub + 1)) of every
//     tile, reads them in the fixed order c = 4 NB sub + ((i + g) mod 4 NB), i = 0, 1, ... (the rotation spreads a wave's
//     ds_read_b128 over the banks) and keeps 4 x (S1, S2, mx, se) per value in float64 registers across the strip:
//     16 M doubles per thread, whatever NB.  A particle of weight 0 (and every row p >= N) is SELECTED out, never
//     multiplied: its value may be anything;
//   * after the last tile the 8 / NB particle subsets of a group are combined through LDS in ascending sub and the sums of
//     the experts j < K go to part[strip][4 M][nblk P].  Item (strip, 0) also writes the strip's sum of weights.
// A value that is not finite at a particle with w > 0 lowers *flags to (m << 20) | j (an integer atomic: the lowest
// value index and expert win whatever the schedule).  No floating-point atomic: the order of every addition is a
// function of (N, K, D) alone.  The fold over strips and slots is pointwise.hip's.
#pragma once
#ifndef __HIPCC_RTC__  // hipRTC pre-includes the device runtime (linear_energy.hip)
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#include "dense_pot.hpp"
#include "dense_pot_kernels.hpp"
#include "dense_pot_tile.hpp"

namespace mjhmc {

constexpr int kPwStripTiles = 32;          // tiles of 32 particles per strip: a constant of the order of additions
constexpr int kPwMaxValues = 4;
constexpr int kPwNoBad = 0x7FFFFFFF;       // *flags when every value is finite
constexpr int kPwExpertBits = 20;          // *flags = (m << 20) | j; j < 2^20 (kLinTallMaxExperts)
constexpr int kPwDead = 0x7FFFFFFF;        // the column of an entry that belongs to no column: below no K

struct PwArgs {
  const float* X;     // [32 ntiles][P] float32 rows of one slot, rows beyond the batch zero
  const double* w;    // [>= N] weights, or nullptr for unit weights
  double* part;       // [nstrips][4 M][nblk P]: S1[M], S2[M], mx[M], se[M] of every strip
  double* partW;      // [nstrips] sum of the strip's weights
  int* flags;         // [1]: the lowest (m << 20) | j of a value that is not finite
  int64_t N;
  int ntiles, nstrips;   // ntiles = ceil(N / 32), nstrips = ceil(ntiles / kPwStripTiles)
  unsigned lme;          // bit m: value m keeps (mx, se) (a launch argument: one compile serves every mask)
};

#pragma clang fp contract(off)

__device__ __forceinline__ bool pw_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

// (mx, se) with one more term of weight w > 0 and finite t when `use`, unchanged otherwise -- by selects, no branch: a new
// maximum rescales se.  mx = -inf (nothing yet) gives d = +inf and e = 0: se = 0 * 0 + w.  Not used: d = 0, e = 1 and
// se + 0 * 1.  -inf - (-inf) cannot form: t is finite where it is used.
__device__ __forceinline__ void pw_lme_add(double& mx, double& se, double t, double w, bool use) {
  const double d = use ? t - mx : 0.0;
  const double we = use ? w : 0.0;
  const double e = exp(-fabs(d));
  const bool up = d > 0.0;
  se = up ? se * e + we : se + we * e;
  mx = up ? t : mx;
}

// (mx, se) <- merged with (mx2, se2); two empty pairs stay (-inf, 0) without a subtraction
__device__ __forceinline__ void pw_lme_merge(double& mx, double& se, double mx2, double se2) {
  const double m = mx2 > mx ? mx2 : mx;
  if (m < -1.7976931348623157e308) return;
  se = se * exp(mx - m) + se2 * exp(mx2 - m);
  mx = m;
}

template <int M>
struct PwAcc {
  double s1[M][4], s2[M][4], mx[M][4], se[M][4];
};

// The image of value MI (sh.pub[1], published by the caller) summed over the tile's 32 particles into acc, between two
// barriers of its own.  jq: the column of each of the thread's four entries; an entry whose column is not below K (a
// padded expert; kPwDead) is dead -- in no sum, in no check, never stored.
template <int NB, int M, int MI>
__device__ __forceinline__ void pw_reduce(Shared<NB>& sh, const double* wts, int g, int sub, const int (&jq)[4], int K, unsigned lme,
                                          PwAcc<M>& acc, int& bad) {
  constexpr int PS = 4 * NB;   // particles of a subset
  __syncthreads();
  const f32x4* img = &sh.pub[1][0].v[0][0][0] + (g >> 1) * 64 + (g & 1) * 32 + sub * PS;
  const int rot = g & (PS - 1);
  const bool keep = (lme >> MI) & 1u;   // (wave-uniform)
#pragma unroll 1
  for (int i = 0; i < PS; ++i) {
    const int cc = (i + rot) & (PS - 1);
    const f32x4 t4 = img[cc];
    const double wp = wts[sub * PS + cc];
    const bool on = wp > 0.0;
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) {
      const double t = (double)t4[qq];
      const bool live = on && jq[qq] < K, fin = pw_finite(t);
      if (live && !fin) {
        const int code = (MI << kPwExpertBits) | jq[qq];
        bad = code < bad ? code : bad;
      }
      const bool use = live && fin;
      const double wt = wp * t;
      acc.s1[MI][qq] = acc.s1[MI][qq] + (use ? wt : 0.0);
      acc.s2[MI][qq] = acc.s2[MI][qq] + (use ? wt * t : 0.0);
      if (keep) pw_lme_add(acc.mx[MI][qq], acc.se[MI][qq], t, wp, use);
    }
  }
  __syncthreads();   // the image is read: the next value (or the next tile's) may take it
}

// value MI of the tile whose u sits in the accumulator registers, and the values after it
template <int NB, class H, int MI>
struct PwValue {
  static __device__ __forceinline__ void run(const Tile<NB>& u, const PotLinear& lin, Shared<NB>& sh, const double* wts, int j0,
                                            int w, int h, int lane, int g, int sub, const int (&jq)[4], unsigned lme, PwAcc<H::kM>& acc, int& bad) {
    {
      Tile<NB> v;
#pragma unroll
      for (int q = 0; q < 16; ++q)
#pragma unroll
        for (int r = 0; r < NB; ++r) {
          const int j = j0 + 32 * NB * w + NB * acc_row(q, h) + r;
          // (padded experts j >= K are not masked here -- 16 NB loop-invariant predicates would sit in scalar registers
          // across the strip: the reduction never reads their entries into a sum, and nothing stores them)
          v.b[r][q] = H::template h<MI>(u.b[r][q], j, lin.p, LinQ{lin.q, lin.stride, j});
        }
      publish<NB>(sh.pub[1][w], lane, v);
    }
    pw_reduce<NB, H::kM, MI>(sh, wts, g, sub, jq, lin.K, lme, acc, bad);
    if constexpr (MI + 1 < H::kM) PwValue<NB, H, MI + 1>::run(u, lin, sh, wts, j0, w, h, lane, g, sub, jq, lme, acc, bad);
  }
};

// the particle subsets of value MI combined in ascending sub through red[16][256] (LDS), the columns jq < K stored
template <int NB, int M, int MI>
__device__ __forceinline__ void pw_store_one(const PwArgs& a, int K, double* red, size_t KP, int strip, int g, int sub,
                                             const int (&jq)[4], PwAcc<M>& acc) {
  constexpr int NG = 32 * NB, SPLIT = 256 / NG;
  const int tid = threadIdx.x;
#pragma unroll
  for (int qq = 0; qq < 4; ++qq) {
    red[(0 + qq) * 256 + tid] = acc.s1[MI][qq];
    red[(4 + qq) * 256 + tid] = acc.s2[MI][qq];
    red[(8 + qq) * 256 + tid] = acc.mx[MI][qq];
    red[(12 + qq) * 256 + tid] = acc.se[MI][qq];
  }
  __syncthreads();
  if (sub == 0) {
    double* out = a.part + (size_t)strip * (4 * M) * KP;
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) {
      double s1 = acc.s1[MI][qq], s2 = acc.s2[MI][qq], mx = acc.mx[MI][qq], se = acc.se[MI][qq];
      for (int o = 1; o < SPLIT; ++o) {
        const int t = g + o * NG;
        s1 = s1 + red[(0 + qq) * 256 + t];
        s2 = s2 + red[(4 + qq) * 256 + t];
        if ((a.lme >> MI) & 1u) pw_lme_merge(mx, se, red[(8 + qq) * 256 + t], red[(12 + qq) * 256 + t]);
      }
      if (jq[qq] < K) {
        out[(size_t)(0 * M + MI) * KP + jq[qq]] = s1;
        out[(size_t)(1 * M + MI) * KP + jq[qq]] = s2;
        out[(size_t)(2 * M + MI) * KP + jq[qq]] = mx;
        out[(size_t)(3 * M + MI) * KP + jq[qq]] = se;
      }
    }
  }
  __syncthreads();
}

template <int NB, class H, int MI>
struct PwStore {
  static __device__ __forceinline__ void run(const PwArgs& a, const PotLinear& lin, double* red, size_t KP, int strip, int g, int sub,
                                            const int (&jq)[4], PwAcc<H::kM>& acc) {
    pw_store_one<NB, H::kM, MI>(a, lin.K, red, KP, strip, g, sub, jq, acc);
    if constexpr (MI + 1 < H::kM) PwStore<NB, H, MI + 1>::run(a, lin, red, KP, strip, g, sub, jq, acc);
  }
};

// The experts of one block as this pass sees them -- B: kM values; set(blk, g) the columns of reduction thread g's four
// entries; values(u, ...) every value published and reduced; store(...) the strip's sums.  Here the block of a square or
// tall model: expert j0 + local in the caller's order, every value per expert (H: kM values, h<MI>(u, j, p, q) the
// caller's expressions, linear_energy.hip).  The grouped model's is GpBlock (dense_lin_group_pointwise.hpp).
template <int NB, class H>
struct PwTallBlock {
  static constexpr int kM = H::kM;
  const PotLinear& lin;
  int j0;
  int jq[4];
  __device__ __forceinline__ void set(int blk, int g) {
    // group g = ((w' NB + r) 4 + q4) 2 + h' of the image: its four experts are rows 8 q4 + 4 h' + qq of wave w', block r
    const int e0 = 32 * NB * ((g >> 3) / NB) + NB * (8 * ((g >> 1) & 3) + 4 * (g & 1)) + ((g >> 3) % NB);
    j0 = blk * (128 * NB);
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) jq[qq] = j0 + e0 + NB * qq;
  }
  __device__ __forceinline__ void values(const Tile<NB>& u, Shared<NB>& sh, const double* wts, int w, int h, int lane, int g, int sub,
                                         unsigned lme, PwAcc<kM>& acc, int& bad) const {
    PwValue<NB, H, 0>::run(u, lin, sh, wts, j0, w, h, lane, g, sub, jq, lme, acc, bad);
  }
  __device__ __forceinline__ void store(const PwArgs& a, double* red, size_t KP, int strip, int g, int sub, PwAcc<kM>& acc) const {
    PwStore<NB, H, 0>::run(a, lin, red, KP, strip, g, sub, jq, acc);
  }
};

// the items (strip, block) over nblk blocks stored at W1b / cbb like a tall model's; KP: the column pitch of a.part
template <int NB, class B>
__device__ __forceinline__ void pw_items(const PwArgs& a, const float* W1b, const float* cbb, int nblk, size_t KP, B& bv, Shared<NB>& sh,
                                         double* wts /* [32] LDS */) {
  constexpr int P = 128 * NB, M = B::kM, NG = 32 * NB;
  constexpr size_t MB = (size_t)P * P;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 31, h = lane >> 5;
  const int g = tid % NG, sub = tid / NG;
  const int nitems = a.nstrips * nblk;
  int bad = kPwNoBad;
  for (int item = blockIdx.x; item < nitems; item += gridDim.x) {
    const int strip = item / nblk, blk = item - strip * nblk;
    const float* W1 = W1b + (size_t)blk * MB;
    // GEMM 1 alone.  ndims = P: NB = 1's skip of the k-row groups beyond D (gemm_any) is folded away -- its 16 predicates are
    // loop invariant here and would hold 32 scalar registers across the strip (30 - 35 of them spilled)
    const PotModel mdl{W1, W1, cbb + (size_t)blk * P, nullptr, P, P};
    bv.set(blk, g);
    // (the previous item's last LDS reads lie before its closing barrier)
    for (int i = tid; i < P; i += 256) sh.cb[i] = mdl.cb[i];
    AReg<NB> ar;
    if constexpr (NB == 1) {
      const float* m1 = W1 + (size_t)(4 * h) * 128 + 32 * w + c;
#pragma unroll
      for (int chunk = 0; chunk < 4; ++chunk) a_chunk_load<1>(m1, chunk, ar.w1[chunk]);
    } else {
      a_chunk_load<NB>(W1 + (size_t)(4 * NB * h) * P + 32 * NB * w + NB * c, 0, ar.a0);
    }
    PwAcc<M> acc;
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) {
        acc.s1[m][qq] = acc.s2[m][qq] = acc.se[m][qq] = 0.0;
        acc.mx[m][qq] = -__builtin_huge_val();
      }
    const int t0 = strip * kPwStripTiles;
    const int t1 = t0 + kPwStripTiles < a.ntiles ? t0 + kPwStripTiles : a.ntiles;
#pragma unroll 1
    for (int tile = t0; tile < t1; ++tile) {
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
      Tile<NB> u;
      rowvec_load<NB>(sh.cb, w, h, u);
      if constexpr (NB == 1) gemm_any<1, false>(mdl, ar, sh.pub[0], w, c, h, lane, u);
      else gemm_dim<NB>(W1, W1, sh.pub[0], w, c, h, lane, ar.a0, u);   // (hands on chunk 0 of the same block: the next tile's)
      bv.values(u, sh, wts, w, h, lane, g, sub, a.lme, acc, bad);
    }
    // both images are free behind the last value's closing barrier: 16 x 256 doubles = 32 KB <= sizeof(sh.pub)
    bv.store(a, reinterpret_cast<double*>(&sh.pub[0][0]), KP, strip, g, sub, acc);
    if (blk == 0 && w == 0) {   // the strip's weights: lane l takes p = 32 t0 + l + 64 i, then the butterfly
      double s = 0.0;
      for (int i = 0; i < kPwStripTiles / 2; ++i) {
        const int64_t pp = (int64_t)t0 * kP + lane + 64 * i;
        const double wv = pp < a.N ? (a.w ? a.w[pp] : 1.0) : 0.0;
        s = s + (wv > 0.0 ? wv : 0.0);
      }
      for (int o = 1; o < 64; o <<= 1) s = s + __shfl_xor(s, o, 64);
      if (lane == 0) a.partW[strip] = s;
    }
  }
  if (bad != kPwNoBad) atomicMin(a.flags, bad);
}

template <int NB, class H>
__device__ __forceinline__ void lin_pointwise_items(const PwArgs& a, const LinTallModel& tm, const PotLinear& lin, Shared<NB>& sh,
                                                    double* wts /* [32] LDS */) {
  PwTallBlock<NB, H> bv{lin};
  pw_items<NB>(a, tm.W1b, tm.cb, tm.nblk, (size_t)tm.nblk * (128 * NB), bv, sh, wts);
}

}  // namespace mjhmc
