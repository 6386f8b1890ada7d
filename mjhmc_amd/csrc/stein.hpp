// Kernel Stein discrepancy of one recorded ensemble against exp(-E) (include/mjhmc_hip.h: mjhmc_stein_*).  For the
// particles p < n_use of one ring slot, weights w_p, G = dE/dX at the states, the IMQ base kernel with exponent -1/2,
//     k(x,y) = (c^2 + |x-y|^2)^(-1/2),
// and, per pair, r2 = sum_d (x_d-y_d)^2, dd = sum_d (Gx_d-Gy_d)(x_d-y_d), gg = sum_d Gx_d*Gy_d, q = c^2 + r2, t = 1/sqrt(q):
//     k_p(x,y) = gg*t - t^3*dd + ndims*t^3 - 3*t^5*r2
//     W = sum w_p     W2 = sum w_p^2     S = sum_{i,j} w_i w_j k_p(x_i,x_j)     Sd = sum_i w_i^2 k_p(x_i,x_i)
//
// stein_pair_kernel: the O(n_use^2 * ndims) pass, in the DIFFERENCE form (the Gram form |x|^2+|y|^2-2x.y cancels for the
// nearby states an ensemble of short chains consists of, and float64 MFMA runs at the float64 vector rate on gfx950).
//   * a workgroup of 256 threads owns the 64 x 64 tile (I, J), I <= J, of pairs i = 64 I + r, j = 64 J + s; thread
//     (ty, tx) = (tid / 16, tid % 16) owns the 4 x 4 pairs r = ty + 16 a, s = tx + 16 b: 48 float64 accumulators.
//   * the d axis is walked in chunks of kSteinChunk = 16; X and G of both row sets are staged through LDS ALREADY WIDENED
//     to float64 (exactly), d-major: sm[m][d][row], 4 x 16 x 64 x 8 B = 32 KiB.  Staging: thread t holds row t % 64 and the
//     four dimensions 4 (t / 64) .. + 3 of the chunk, so a wave's ds_write_b64 covers 64 consecutive doubles (no two lanes
//     of a 16-lane store group on one bank); the next chunk's global loads are issued before the current chunk's arithmetic.
//     Reading: one d per step; the 16 tx lanes of a ty read 16 consecutive doubles (128 B of the 256-B bank row), the other
//     16 lanes of the 32-lane ds_read_b64 group read the SAME addresses (broadcast), and the row reads are two adjacent
//     doubles per group: no bank conflict under the (a/4) mod 64 rule.  The 16-row interleave is what makes this so.
//   * per (pair, d), in ascending d:  dx = xi - xj;  dg = gi - gj;  r2 += dx*dx;  dd += dg*dx;  gg += gi*gj  -- every
//     product rounded before its sum (-ffp-contract=off, repeated by the pragma below): 2 subtractions, 3 products, 3 sums.
//     Elements d >= ndims are staged as 0.0 and the last chunk stops at ndims.
//   * epilogue per pair, 11 roundings:  q = c2 + r2;  s = sqrt(q);  t = 1/s;  t2 = t*t;  t3 = t2*t;  t5 = t3*t2;
//         k = ((gg*t - t3*dd) + nd*t3) - (3*t5)*r2      [gg*t, t3*dd, nd*t3, 3*t5, (3 t5)*r2: 5 products; 3 sums]
//     then v = (w_i*w_j)*k: 2 more.  (c2 = c*c is rounded once on the host; nd = (double)ndims is exact.)
//   * pairs with i >= n_use or j >= n_use are SELECTED out (v = 0.0 by ?:, never a product with zero); rows >= n_use are
//     never loaded either: they may hold NaN, and their gradient usually does.
//   * reduction, no floating-point atomic: the thread adds its 16 v in the order (a, b) = (0,0), (0,1), ... (3,3) from 0.0
//     [16 additions]; the wave's butterfly t += shfl_xor(t, o), o = 1, 2, ... 32 [6]; wave totals through LDS, thread 0
//     adds waves 0, 1, 2, 3 in order [3]; an off-diagonal tile counts twice (x 2.0, exact).  A diagonal tile computes the
//     full square once and the same reduction of the pairs with i == j gives its Sd.  One (S, Sd) per tile into part[].
//   * tile index T = J (J + 1) / 2 + I (64-bit); the grid is one workgroup per tile.
//   * rows of a diagonal tile see every particle p < n_use once: a state or gradient element d < ndims of such a row that
//     is not finite raises bit 1 / bit 2 of *bad (an integer atomic).
// stein_finish_kernel: ONE workgroup of 256 threads.  Thread t adds part[t], part[t + 256], ... in ascending order from
// 0.0 [ceil(n_tiles / 256) additions], then the butterfly [6] and the four wave totals in order [3]; the same for w_p and
// w_p * w_p over p < n_use, p = t, t + 256, ...  A weight that is not finite raises bit 0 of *bad, a sum that is not finite
// although every input is (overflow) bit 3.  out = {W, W2, S, Sd}.
// Longest chain of additions behind S: 16 + 6 + 3 + ceil(n_tiles / 256) + 6 + 3.
// The order of every addition is a function of (ndims, n_use, types, pitch) alone: bit-identical from run to run and
// independent of how the run is cut into blocks.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ring_rows.hpp"

namespace mjhmc {

constexpr int kSteinTile = 64;      // particles per tile side
constexpr int kSteinChunk = 16;     // dimensions staged per step
constexpr int kSteinBadWeight = 1, kSteinBadState = 2, kSteinBadGrad = 4, kSteinBadSum = 8;

struct SteinArgs {
  const void* X;      // one ring slot: [Npad][pitch] elements of the state's type
  const void* G;      // dE/dX of that slot: [Npad][pitch] float64 (float64 state) or float32
  const double* w;    // [Npad] weights, or nullptr for unit weights
  double* part;       // [n_tiles][2]: (S, Sd) of every tile
  double* out;        // [4]: W, W2, S, Sd
  int* bad;
  long long n_use, n_tiles;
  int D, pitch;
  double c2, nd;      // c * c, (double)ndims
};

// four consecutive elements d0 .. d0 + 3 of a row, widened exactly; elements d >= D are 0.0 and nothing at or beyond the
// pitch is read.  DT: 0 float64 (pitch even, d0 a multiple of 4: two 16-byte loads), 1 float32 (pitch a multiple of 4: one
// 16-byte load), 2 bfloat16 (pitch a multiple of 8: one 8-byte load)
template <int DT>
__device__ __forceinline__ void stein_load4(const void* __restrict__ base, long long row, int pitch, int d0, int D, double* v) {
  v[0] = v[1] = v[2] = v[3] = 0.0;
  if (DT == 0) {
    const double* r = reinterpret_cast<const double*>(base) + (size_t)row * pitch;
    if (d0 < D) {
      const double2 q = *reinterpret_cast<const double2*>(r + d0);
      v[0] = q.x;
      if (d0 + 1 < D) v[1] = q.y;
    }
    if (d0 + 2 < D) {
      const double2 q = *reinterpret_cast<const double2*>(r + d0 + 2);
      v[2] = q.x;
      if (d0 + 3 < D) v[3] = q.y;
    }
  } else if (DT == 1) {
    const float* r = reinterpret_cast<const float*>(base) + (size_t)row * pitch;
    if (d0 < D) {
      const float4 q = *reinterpret_cast<const float4*>(r + d0);
      v[0] = (double)q.x;
      if (d0 + 1 < D) v[1] = (double)q.y;
      if (d0 + 2 < D) v[2] = (double)q.z;
      if (d0 + 3 < D) v[3] = (double)q.w;
    }
  } else {
    const unsigned short* r = reinterpret_cast<const unsigned short*>(base) + (size_t)row * pitch;
    if (d0 < D) {
      const uint2 q = *reinterpret_cast<const uint2*>(r + d0);
      v[0] = bf16_to_f64(q.x & 0xFFFFu);
      if (d0 + 1 < D) v[1] = bf16_to_f64(q.x >> 16);
      if (d0 + 2 < D) v[2] = bf16_to_f64(q.y & 0xFFFFu);
      if (d0 + 3 < D) v[3] = bf16_to_f64(q.y >> 16);
    }
  }
}

#pragma clang fp contract(off)
// wave butterfly, then the four wave totals through LDS, added in order; every thread passes its value and gets the total
__device__ __forceinline__ double stein_block_sum(double t, double* __restrict__ red /* [4] LDS */) {
  for (int o = 1; o < 64; o <<= 1) t = t + __shfl_xor(t, o, 64);
  __syncthreads();   // (red may still be read from a previous sum)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = t;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// tile index -> (I, J), I <= J, T = J (J + 1) / 2 + I
__device__ __forceinline__ void stein_tile_of(long long T, long long* I, long long* J) {
  long long j = (long long)((sqrt(8.0 * (double)T + 1.0) - 1.0) * 0.5);
  while (j * (j + 1) / 2 > T) --j;
  while ((j + 1) * (j + 2) / 2 <= T) ++j;
  *J = j;
  *I = T - j * (j + 1) / 2;
}

// DT: the state's type (0 float64, 1 float32, 2 bfloat16); GT: the gradient's (0 float64, 1 float32)
template <int DT, int GT>
__global__ __launch_bounds__(256) void stein_pair_kernel(SteinArgs a) {
  __shared__ double sm[4][kSteinChunk][kSteinTile];   // XI, GI, XJ, GJ of the chunk, d-major
  __shared__ double red[4];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  long long I, J;
  stein_tile_of((long long)blockIdx.x, &I, &J);
  const bool diag = I == J;
  // staging: this thread's row of either set and its four dimensions of the chunk
  const int srow = tid & 63, sq = tid >> 6;
  const long long pi = I * kSteinTile + srow, pj = J * kSteinTile + srow;
  const bool li = pi < a.n_use, lj = pj < a.n_use;
  double nx[4][4];   // the next chunk: XI, GI, XJ, GJ
  auto fetch = [&](int c0) {
    const int d0 = c0 + 4 * sq;
#pragma unroll
    for (int m = 0; m < 4; ++m) nx[m][0] = nx[m][1] = nx[m][2] = nx[m][3] = 0.0;
    if (li) {
      stein_load4<DT>(a.X, pi, a.pitch, d0, a.D, nx[0]);
      stein_load4<GT>(a.G, pi, a.pitch, d0, a.D, nx[1]);
    }
    if (lj) {
      stein_load4<DT>(a.X, pj, a.pitch, d0, a.D, nx[2]);
      stein_load4<GT>(a.G, pj, a.pitch, d0, a.D, nx[3]);
    }
  };
  int nf = 0;
  double r2[4][4], dd[4][4], gg[4][4];
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v) r2[u][v] = dd[u][v] = gg[u][v] = 0.0;
  fetch(0);
  for (int c0 = 0; c0 < a.D; c0 += kSteinChunk) {
    __syncthreads();   // the previous chunk has been read
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int e = 0; e < 4; ++e) sm[m][4 * sq + e][srow] = nx[m][e];
    if (diag) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (!finite_f64(nx[0][e])) nf |= kSteinBadState;
        if (!finite_f64(nx[1][e])) nf |= kSteinBadGrad;
      }
    }
    __syncthreads();
    if (c0 + kSteinChunk < a.D) fetch(c0 + kSteinChunk);
    const int dn = a.D - c0 < kSteinChunk ? a.D - c0 : kSteinChunk;
    for (int d = 0; d < dn; ++d) {
      double xi[4], gi[4], xj[4], gj[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        xi[u] = sm[0][d][ty + 16 * u];
        gi[u] = sm[1][d][ty + 16 * u];
        xj[u] = sm[2][d][tx + 16 * u];
        gj[u] = sm[3][d][tx + 16 * u];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const double dx = xi[u] - xj[v];
          const double dg = gi[u] - gj[v];
          r2[u][v] = r2[u][v] + dx * dx;
          dd[u][v] = dd[u][v] + dg * dx;
          gg[u][v] = gg[u][v] + gi[u] * gj[v];
        }
    }
  }
  // epilogue
  double wi[4], wj[4];
  bool vi[4], vj[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const long long i = I * kSteinTile + ty + 16 * u, j = J * kSteinTile + tx + 16 * u;
    vi[u] = i < a.n_use;
    vj[u] = j < a.n_use;
    wi[u] = (vi[u] && a.w) ? a.w[i] : 1.0;
    wj[u] = (vj[u] && a.w) ? a.w[j] : 1.0;
  }
  double s = 0.0, sd = 0.0;
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const double q = a.c2 + r2[u][v];
      const double sq_ = sqrt(q);
      const double t = 1.0 / sq_;
      const double t2 = t * t;
      const double t3 = t2 * t;
      const double t5 = t3 * t2;
      const double k = ((gg[u][v] * t - t3 * dd[u][v]) + a.nd * t3) - (3.0 * t5) * r2[u][v];
      const double val = (wi[u] * wj[v]) * k;
      const bool on = vi[u] && vj[v];
      s = s + (on ? val : 0.0);
      sd = sd + ((on && diag && ty == tx && u == v) ? val : 0.0);
    }
  s = stein_block_sum(s, red);
  sd = stein_block_sum(sd, red);
  if (tid == 0) {
    a.part[2 * (size_t)blockIdx.x] = diag ? s : 2.0 * s;
    a.part[2 * (size_t)blockIdx.x + 1] = sd;
  }
  if (nf) atomicOr(a.bad, nf);
}

__global__ __launch_bounds__(256) void stein_finish_kernel(SteinArgs a) {
  __shared__ double red[4];
  const int tid = threadIdx.x;
  double s = 0.0, sd = 0.0, w1 = 0.0, w2 = 0.0;
  for (long long T = tid; T < a.n_tiles; T += 256) {
    s = s + a.part[2 * (size_t)T];
    sd = sd + a.part[2 * (size_t)T + 1];
  }
  int nf = 0;
  for (long long p = tid; p < a.n_use; p += 256) {
    const double w = a.w ? a.w[p] : 1.0;
    if (!finite_f64(w)) nf |= kSteinBadWeight;
    w1 = w1 + w;
    w2 = w2 + w * w;
  }
  s = stein_block_sum(s, red);
  sd = stein_block_sum(sd, red);
  w1 = stein_block_sum(w1, red);
  w2 = stein_block_sum(w2, red);
  if (tid == 0) {
    if (!finite_f64(s) || !finite_f64(sd) || !finite_f64(w2)) nf |= kSteinBadSum;
    a.out[0] = w1;
    a.out[1] = w2;
    a.out[2] = s;
    a.out[3] = sd;
  }
  if (nf) atomicOr(a.bad, nf);
}

// stein.hip: the pair kernel and the finish kernel on `stream`.  state_dtype: MJHMC_F64 / _F32 / _BF16 (0 / 1 / 2);
// grad_f32: the gradient is float32.  Returns false for a pair of types no energy family writes.
bool stein_launch(const SteinArgs& a, int state_dtype, bool grad_f32, hipStream_t stream);

}  // namespace mjhmc
