// Cell labels of the recorded states: which of M centres a state is nearest to (its Voronoi cell), or "outside".
// occ_label_kernel below is the distance twin of projections_kernel (projections.hpp): n slots x N particles x M centres,
// the rows float64, float32 or bfloat16 and widened exactly with RowChunk<DT> (ring_rows.hpp).  The contract -- labels,
// tables, refusals -- is stated at the top of occupancy.hip.
//
// Arithmetic.  For a row x and centre m the accumulator d2 starts at 0.0 and takes, for d ascending below K,
//     t = x[d] - c[m][d];  sq = t * t;  d2 = d2 + sq
// every operation rounded: three float64 instructions per (p, m, d).  The library is built with -ffp-contract=off and the
// pragma below repeats it for this file: no square is fused into a sum.  Padding elements d >= K are skipped, not added as
// zeros.  No distance is split over lanes, waves or workgroups: a label is a function of (x, centres, r2) alone.
//
// Shape: that of projections_kernel.  A workgroup of 256 threads owns a tile of 64 rows x TK centres, TK = 16 * KV: lane
// (tx = tid & 15, ty = tid >> 4) keeps the 4 x KV distances of rows 4 ty .. 4 ty + 3 and centres KV tx .. KV tx + KV - 1.
// KV = 4 (64 centres, all there can be) is the general tile; KV = 1 serves M <= 16.  The d loop goes in chunks of DC = 8 *
// VEC elements (128 bytes of a row): the X chunk is loaded with 16-byte loads, widened and stored TRANSPOSED in LDS,
// Xs[dd][row] with rows padded to 66 doubles; the centre chunk is a straight 16-byte copy from the handle's device copy,
// which is kept transposed and zero-padded ([Dpad][64]), into Cs[dd][m]; the loads of chunk s + 1 are issued into registers
// before the arithmetic of chunk s and written to LDS after it (two barriers per chunk).
//
// What differs from projections_kernel: nothing is stored per (p, m).  After the d loop a lane takes the best of its own KV
// centres in ascending m -- `d2 < best`, strictly, from best = +inf, label = M, so that a NaN or infinite distance is never
// chosen -- and skips m >= M BY INDEX: the zero columns of the padded tile hold the distance to the origin and must never
// win.  The 16 lanes that share a row (one DPP row of a wave) then reduce (best, label) lexicographically in four DPP
// steps (occ_take_min) -- the smaller distance, at equal distances the smaller index -- after which every one of them
// holds the row's label; the radius test follows and lane tx = 0 stores the four bytes of its four rows as one 32-bit word.
// Rows p >= N are loaded as zeros and their bytes (inside the [n][Npad] label scratch) are written but never read.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ring_rows.hpp"

namespace mjhmc {

constexpr int kOccMaxCentres = 64;
constexpr int kOccRows = 64;      // rows of a tile
constexpr int kOccRowPad = 2;     // Xs rows: 66 doubles (16-byte reads stay aligned, row stride off the power of two)

struct OccLabelArgs {
  const void* src;        // first source slot: [n][Npad][pitch] elements of the ring's type
  uint8_t* labels;        // [n][Npad]
  const double* Ct;       // [Dpad][64]: Ct[d][m] = c[m][d], zero where d >= K or m >= M; Dpad a multiple of 64
  const double* r2;       // [64]: squared radius of centre m, +inf for none
  long long Npad, N;
  int n, D, chunks;       // chunks = pitch / (elements per 16 bytes)
  int M;
};

// centres per lane of the tile that serves M centres (the tile holds 16 * KV)
__host__ __device__ constexpr int occ_lane_centres(int M) { return M <= 16 ? 1 : 4; }

// The cross-lane step of the 16 lanes that share a row: DPP moves inside a row of 16 lanes (no LDS traffic).  The pairs
// (best, label) are totally ordered and the smaller of two is taken on both sides, so the partners need not be an xor
// butterfly: lane ^ 1 and lane ^ 2 make the four lanes of a quad agree, row_half_mirror (lane 7 - i of each 8) the two quads
// of a half, row_mirror (lane 15 - i) the two halves.  All 256 lanes of the workgroup are active where this runs.
constexpr int kDppQuadXor1 = 0xB1;         // quad_perm:[1,0,3,2]
constexpr int kDppQuadXor2 = 0x4E;         // quad_perm:[2,3,0,1]
constexpr int kDppRowHalfMirror = 0x141;
constexpr int kDppRowMirror = 0x140;

template <int CTRL>
__device__ __forceinline__ void occ_take_min(double& best, int& label) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(best), CTRL, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(best), CTRL, 0xF, 0xF, false);
  const int ol = __builtin_amdgcn_update_dpp(0, label, CTRL, 0xF, 0xF, false);
  const double ob = __hiloint2double(hi, lo);
  if (ob < best || (ob == best && ol < label)) {
    best = ob;
    label = ol;
  }
}

#pragma clang fp contract(off)
// DT: the state's type (0 float64, 1 float32, 2 bfloat16); KV: centres per lane (1 or 4)
template <int DT, int KV>
__global__ __launch_bounds__(256) void occ_label_kernel(OccLabelArgs a) {
  constexpr int VEC = RowChunk<DT>::VEC;
  constexpr int DC = 8 * VEC;                       // elements of a d chunk: 128 bytes of a row
  constexpr int TK = 16 * KV;
  constexpr int XS = kOccRows + kOccRowPad;
  constexpr int NA = (DC * TK / 2 + 255) / 256;     // 16-byte loads of the centre chunk per lane
  static_assert(KV == 1 || KV == 4, "a lane owns 1 or 4 centres");
  __shared__ __attribute__((aligned(16))) double Xs[DC * XS];
  __shared__ __attribute__((aligned(16))) double Cs[DC * TK];
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;
  const int lc = tid & 7, lr = tid >> 3;            // staging: chunk of the 128 bytes, row (and row + 32)
  const long long p0 = (long long)blockIdx.x * kOccRows;
  const int nsteps = (a.D + DC - 1) / DC;
  const double2* __restrict__ Ct2 = reinterpret_cast<const double2*>(a.Ct);
  const double inf = __longlong_as_double(0x7FF0000000000000ll);

  for (int slot = blockIdx.y; slot < a.n; slot += gridDim.y) {
    const uint4* __restrict__ X = reinterpret_cast<const uint4*>(a.src) + (size_t)slot * a.Npad * a.chunks;
    double acc[4][KV];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < KV; ++j) acc[i][j] = 0.0;
    uint4 qx[2];
    double2 qc[NA];
    // chunk `step` of the tile's rows and of the centres into registers (rows p >= N and chunks past the row: zeros)
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
        const int idx = tid + 256 * i;              // double2 index within the [DC][TK] chunk
        qc[i] = make_double2(0.0, 0.0);
        if (idx < DC * TK / 2) {
          const int dd = idx / (TK / 2), kk = idx % (TK / 2);
          qc[i] = Ct2[((size_t)(step * DC + dd) * kOccMaxCentres) / 2 + kk];
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
        if (idx < DC * TK / 2) reinterpret_cast<double2*>(Cs)[idx] = qc[i];
      }
    };
    auto add_element = [&](int dd) {
      const double2 x01 = *reinterpret_cast<const double2*>(&Xs[dd * XS + ty * 4]);
      const double2 x23 = *reinterpret_cast<const double2*>(&Xs[dd * XS + ty * 4 + 2]);
      const double x[4] = {x01.x, x01.y, x23.x, x23.y};
      double cv[KV];
      if constexpr (KV == 4) {
        const double2 c01 = *reinterpret_cast<const double2*>(&Cs[dd * TK + tx * KV]);
        const double2 c23 = *reinterpret_cast<const double2*>(&Cs[dd * TK + tx * KV + 2]);
        cv[0] = c01.x;
        cv[1] = c01.y;
        cv[KV - 2] = c23.x;
        cv[KV - 1] = c23.y;
      } else {
        cv[0] = Cs[dd * TK + tx];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < KV; ++j) {
          const double t = x[i] - cv[j];
          const double sq = t * t;
          acc[i][j] = acc[i][j] + sq;
        }
    };

    stage_load(0);
    for (int step = 0; step < nsteps; ++step) {
      __syncthreads();                              // the previous chunk's reads of Xs / Cs are done
      stage_store();
      __syncthreads();
      if (step + 1 < nsteps) stage_load(step + 1);
      const int left = a.D - step * DC;             // elements d < D of this chunk (uniform)
      if (left >= DC) {
#pragma unroll 8
        for (int dd = 0; dd < DC; ++dd) add_element(dd);
      } else {
        for (int dd = 0; dd < left; ++dd) add_element(dd);
      }
    }

    // the lane's best centre per row, the 16 lanes' best, the radius, the byte
    uint32_t word = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      double best = inf;
      int label = a.M;
#pragma unroll
      for (int j = 0; j < KV; ++j) {
        const int m = tx * KV + j;
        if (m < a.M && acc[i][j] < best) {
          best = acc[i][j];
          label = m;
        }
      }
      occ_take_min<kDppQuadXor1>(best, label);
      occ_take_min<kDppQuadXor2>(best, label);
      occ_take_min<kDppRowHalfMirror>(best, label);
      occ_take_min<kDppRowMirror>(best, label);
      if (label < a.M && !(best <= a.r2[label])) label = a.M;
      word |= (uint32_t)label << (8 * i);
    }
    // (Npad and p0 are multiples of 64, 4 ty of 4: the word is aligned and inside the slot's Npad bytes)
    if (tx == 0) *reinterpret_cast<uint32_t*>(a.labels + (size_t)slot * a.Npad + p0 + ty * 4) = word;
  }
}

// occupancy.hip: one launch on `stream` for the n slots of `a`.  state_dtype: MJHMC_F64 / _F32 / _BF16 (0 / 1 / 2); the tile
// is chosen from a.M (occ_lane_centres).  Returns false for a state type there is no kernel for.
bool occ_label_launch(const OccLabelArgs& a, int state_dtype, hipStream_t stream);

}  // namespace mjhmc
