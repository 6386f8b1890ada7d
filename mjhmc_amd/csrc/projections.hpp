// Linear projections of the recorded states: K values of every state that are affine read-outs of it,
//     u[p][k] = b[k] + sum_{d < ndims} A[k][d] * x[p][d]        g[p][k] = link(u[p][k], k; params)   (identity: g = u)
// written as rows of the DERIVED ring of a mjhmc_functionals (functionals.hip), so that every accumulator of the sample
// ring runs on them unchanged.  projections_kernel below is a small GEMM over ring slots: n slots x N particles x K
// values, the rows float64, float32 or bfloat16 and widened exactly with RowChunk<DT> (ring_rows.hpp).
//
// This header is also what hipRTC compiles around a caller's link expression (projections.hip: link_source): device code
// only, nothing of the project but functionals.hpp.  It is compiled with the library's own flags, -ffp-contract=off among
// them, and the pragma below repeats it for this file: no product is fused into a sum.
//
// Arithmetic contract.  An accumulator starts at b[k] (0.0 where no b was given) and adds the products A[k][d] * x[p][d] in
// ascending d, each product rounded before its sum; padding elements d >= ndims are skipped, not added as zeros.  No value
// is split over lanes, waves or workgroups, and there are no atomics on floats: a value is a function of (A, b, x) alone --
// bit-identical from run to run, for every block, state type and tile configuration, and equal to the NumPy loop
// `u = b.copy(); for d: u = u + A[:, d, None] * X[d]` bit for bit.  The price is two float64 instructions per (p, k, d)
// where a fused multiply-add would take one.
//
// Shape.  A workgroup of 256 threads owns a tile of 64 rows x TK values, TK = 16 * KV: lane (tx = tid & 15, ty = tid >> 4)
// keeps the 4 x KV accumulators of rows 4 ty .. 4 ty + 3 and values KV tx .. KV tx + KV - 1.  KV = 4 (64 values) is the
// general tile; KV = 1 (16 values) serves K <= 16, where three quarters of the wide tile would be padding.  The d loop
// goes in chunks of DC = 8 * VEC elements (128 bytes of a row: 16 / 32 / 64 elements of float64 / float32 / bfloat16):
//   * the X chunk is loaded with 16-byte loads, 8 consecutive lanes on the 128 bytes of one row, widened and stored
//     TRANSPOSED in LDS, Xs[dd][row] with rows padded to 66 doubles; the A chunk is a straight 16-byte copy from the
//     handle's device copy of A, which is kept transposed and zero-padded ([Dpad][Kpad]), into As[dd][k];
//   * the loads of chunk s + 1 are issued into registers before the arithmetic of chunk s and written to LDS after it
//     (two barriers per chunk), so they are in flight under 2 * 4 * KV * DC float64 instructions per lane;
//   * per dd a lane reads its 4 x values and KV a values from LDS (16-byte reads; the lanes of a wave read 4 distinct x
//     addresses and 16 distinct a addresses, conflict-free) and issues 4 KV multiplies and 4 KV adds.
// blockIdx.x is the row tile, blockIdx.y strides over slots; K > TK loops over value tiles inside the workgroup, re-reading
// the same 64 rows per value tile (ceil(K / 64) reads of a slot, all but the first out of L2: a tile's rows are 64 * pitch *
// esize bytes, 256 KiB at 512 float64).  Rows p >= N are neither read nor written; elements K <= e < pitchK are stored as
// 0.0.  The lowest value index of a row p < N whose value is not finite goes to *bad through an integer atomicMin.
#pragma once
#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

struct RtcCode;   // user_expr.hpp
#endif

#include "functionals.hpp"

namespace mjhmc {

constexpr int kProjMaxValues = 512;
constexpr int kProjRows = 64;            // rows of a tile
constexpr int kProjRowPad = 2;           // Xs rows: 66 doubles (16-byte reads stay aligned, row stride off the power of two)
constexpr int kProjNoBad = 0x7FFFFFFF;   // *bad when every value is finite

struct ProjArgs {
  const void* src;        // first source slot: [n][Npad][pitch] elements of the ring's type
  double* dst;            // first derived slot: [n][Npad][pitchK]
  const double* At;       // [Dpad][Kpad]: At[d][k] = A[k][d], zero where d >= D or k >= K; Dpad, Kpad multiples of 64
  const double* b;        // [Kpad], zero where k >= K (and everywhere when no b was given)
  long long Npad, N;
  int n, D, chunks;       // chunks = pitch / (elements per 16 bytes)
  int K, pitchK, Kpad;
  int* bad;
};

// the identity link: g = u
struct ProjIdentity {
  const double* p;
  __device__ __forceinline__ double apply(double u, int) const { return u; }
};

// values per lane of the tile that serves K values (the tile holds 16 * KV)
__host__ __device__ constexpr int proj_lane_values(int K) { return K <= 16 ? 1 : 4; }

#pragma clang fp contract(off)
// DT: the state's type (0 float64, 1 float32, 2 bfloat16); KV: values per lane (1 or 4);
// L: { const double* p; double apply(double u, int k) const; } -- ProjIdentity, or generated around the caller's expression
template <int DT, int KV, typename L>
__global__ __launch_bounds__(256) void projections_kernel(ProjArgs a, L link) {
  constexpr int VEC = RowChunk<DT>::VEC;
  constexpr int DC = 8 * VEC;                       // elements of a d chunk: 128 bytes of a row
  constexpr int TK = 16 * KV;
  constexpr int XS = kProjRows + kProjRowPad;
  constexpr int NA = (DC * TK / 2 + 255) / 256;     // 16-byte loads of the A chunk per lane
  static_assert(KV == 1 || KV == 4, "a lane owns 1 or 4 values");
  __shared__ __attribute__((aligned(16))) double Xs[DC * XS];
  __shared__ __attribute__((aligned(16))) double As[DC * TK];
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;
  const int lc = tid & 7, lr = tid >> 3;            // staging: chunk of the 128 bytes, row (and row + 32)
  const long long p0 = (long long)blockIdx.x * kProjRows;
  const int nsteps = (a.D + DC - 1) / DC;
  const double2* __restrict__ At2 = reinterpret_cast<const double2*>(a.At);

  for (int slot = blockIdx.y; slot < a.n; slot += gridDim.y) {
    const uint4* __restrict__ X = reinterpret_cast<const uint4*>(a.src) + (size_t)slot * a.Npad * a.chunks;
    double* __restrict__ out = a.dst + (size_t)slot * a.Npad * a.pitchK;
    for (int k0 = 0; k0 < a.K; k0 += TK) {
      double acc[4][KV];
#pragma unroll
      for (int j = 0; j < KV; ++j) {
        const double bk = a.b[k0 + tx * KV + j];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i][j] = bk;
      }
      uint4 qx[2];
      double2 qa[NA];
      // chunk `step` of the tile's rows and of A into registers (rows p >= N and chunks past the row: zeros, never used
      // in a sum that is kept -- rows p >= N are not stored, elements d >= D are not added)
      auto stage_load = [&](int step) {
        const int c = step * 8 + lc;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const long long p = p0 + lr + 32 * h;
          qx[h] = make_uint4(0u, 0u, 0u, 0u);
          if (p < a.N && c < a.chunks) qx[h] = X[(size_t)p * a.chunks + c];
        }
#pragma unroll
        for (int i = 0; i < NA; ++i) {
          const int idx = tid + 256 * i;            // double2 index within the [DC][TK] chunk
          qa[i] = make_double2(0.0, 0.0);
          if (idx < DC * TK / 2) {
            const int dd = idx / (TK / 2), kk = idx % (TK / 2);
            qa[i] = At2[((size_t)(step * DC + dd) * a.Kpad + k0) / 2 + kk];
          }
        }
      };
      auto stage_store = [&]() {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          double v[VEC];
          RowChunk<DT>::widen(qx[h], v);
#pragma unroll
          for (int e = 0; e < VEC; ++e) Xs[(lc * VEC + e) * XS + lr + 32 * h] = v[e];
        }
#pragma unroll
        for (int i = 0; i < NA; ++i) {
          const int idx = tid + 256 * i;
          if (idx < DC * TK / 2) reinterpret_cast<double2*>(As)[idx] = qa[i];
        }
      };
      auto add_element = [&](int dd) {
        const double2 x01 = *reinterpret_cast<const double2*>(&Xs[dd * XS + ty * 4]);
        const double2 x23 = *reinterpret_cast<const double2*>(&Xs[dd * XS + ty * 4 + 2]);
        const double x[4] = {x01.x, x01.y, x23.x, x23.y};
        double av[KV];
        if constexpr (KV == 4) {
          const double2 a01 = *reinterpret_cast<const double2*>(&As[dd * TK + tx * KV]);
          const double2 a23 = *reinterpret_cast<const double2*>(&As[dd * TK + tx * KV + 2]);
          av[0] = a01.x;
          av[1] = a01.y;
          av[KV - 2] = a23.x;
          av[KV - 1] = a23.y;
        } else {
          av[0] = As[dd * TK + tx];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < KV; ++j) {
            const double prod = av[j] * x[i];
            acc[i][j] = acc[i][j] + prod;
          }
      };

      stage_load(0);
      for (int step = 0; step < nsteps; ++step) {
        __syncthreads();                            // the previous chunk's reads of Xs / As are done
        stage_store();
        __syncthreads();
        if (step + 1 < nsteps) stage_load(step + 1);
        const int left = a.D - step * DC;           // elements d < D of this chunk (uniform)
        if (left >= DC) {
#pragma unroll 8
          for (int dd = 0; dd < DC; ++dd) add_element(dd);
        } else {
          for (int dd = 0; dd < left; ++dd) add_element(dd);
        }
      }

      // the link, the flag and the store: element e of a row is value e for e < K and 0.0 for K <= e < pitchK
      int badk = kProjNoBad;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long long p = p0 + ty * 4 + i;
        if (p >= a.N) continue;
        double g[KV];
#pragma unroll
        for (int j = 0; j < KV; ++j) {
          const int k = k0 + tx * KV + j;
          g[j] = 0.0;
          if (k < a.K) {
            g[j] = link.apply(acc[i][j], k);
            if (!finite_f64(g[j]) && k < badk) badk = k;
          }
        }
        double* row = out + (size_t)p * a.pitchK + k0 + tx * KV;
        if constexpr (KV == 4) {
          // (pitchK and k0 + 4 tx are even: a pair is inside the row or outside it as a whole)
          if (k0 + tx * KV < a.pitchK) *reinterpret_cast<double2*>(row) = make_double2(g[0], g[1]);
          if (k0 + tx * KV + 2 < a.pitchK) *reinterpret_cast<double2*>(row + 2) = make_double2(g[KV - 2], g[KV - 1]);
        } else {
          if (k0 + tx < a.pitchK) row[0] = g[0];
        }
      }
      if (badk != kProjNoBad) atomicMin(a.bad, badk);
    }
  }
}

#ifndef __HIPCC_RTC__
// projections.hip: one launch on `stream` for the n slots of `a`, identity link.  state_dtype: MJHMC_F64 / _F32 / _BF16
// (0 / 1 / 2); the tile is chosen from a.K (proj_lane_values).  Returns false for a state type there is no kernel for.
bool projections_launch(const ProjArgs& a, int state_dtype, hipStream_t stream);
// the code object and the lowered kernel name of projections_kernel<state_dtype, proj_lane_values(K), link> for the C
// expression `link` of u, k and p[m], compiled with hipRTC once per process and (expression, instantiation)
// (rtc_compile_cached, user_expr.hpp); 0 or an MJHMC_ERR_* code with *err the message (MJHMC_ERR_INVALID: the compiler's log)
int projections_link_compile(const std::string& link, int state_dtype, int K, const std::string& include_dir, const ::RtcCode** out,
                             std::string* err);
#endif

}  // namespace mjhmc
