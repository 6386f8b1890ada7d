// Dwell-time-weighted mean, variance and covariance from the sample ring, on the device.
//
// For a block of n recorded states x[k][p][:] (ring slot x_slot0 + k, particle p < N) and weights w[k][p]
//   W    = sum w          S1_d = sum w (x_d - c_d)        S2_d = sum w (x_d - c_d)^2
//   C_de = sum w (x_d - c_d)(x_e - c_e)
// with a caller-given shift c; every ring element (float64, float32, bfloat16) is widened to float64 exactly and all
// products and sums are float64.  Padding particles (N <= p < Npad) are never read.
//
// Which dwell goes with which state.  Every jump kernel writes the holding time it draws in the iteration that fills ring
// slot s to dwell-ring slot s: iterate.hip jump_args() sets a.dwell_ring = s->dwell_ring + (ring_slot0 + iter) * Npad, the
// fused kernels add `it * Npad` to the pointer of their first iteration (jump_kernel.hpp, row_form.hpp: a.dwell_ring[it * Npad + p]),
// the dense kernels store `best` through it, and the host-energy / multi-pass path does the same
// (multipass.hip: c.dwell_ring = s->dwell_ring + ring_slot * Npad).  The draw uses the rates OUT of the state the
// iteration starts from, so it is the time the particle spent in the state of slot s - 1: the holding time of the state
// in slot s sits in dwell slot s + 1.  The kernels here take the two slot offsets separately and the sampler-level driver
// passes w_slot0 = x_slot0 + 1.  (Read from the sources named above, all five writers; the definition test then checks
// the pairing numerically against ring_read / ring_read_dwell.)
//
// Moment pass: HBM-bound, one read of the block.  A lane owns 16 bytes of a row (ring_rows.hpp) and walks the
// particles with a stride, kRowsInFlight loads issued before the first is used; float64 partial sums per lane, summed over the row lanes of the workgroup through LDS, one
// partial vector per workgroup in a scratch buffer, and a second small kernel that adds the workgroups' partials in
// index order to the running sums.  No floating-point atomics: the result does not depend on the schedule.
//
// Covariance pass (D <= 512): C = Xc^T diag(w) Xc is a rank-k update whose contraction axis is the particle axis, the row
// axis of the particle-major layout.  v_mfma_f64_16x16x4_f64: lane l supplies A[row l & 15][k = l >> 4] and
// B[k = l >> 4][col l & 15], one double each, and receives D[row (l >> 4) + 4 r][col l & 15] in register r.  A wave owns a
// 64 x 64 block of C (4 x 4 tiles, 128 accumulator registers), takes every `splits`-th group of four particles, loads
// four A and four B values per lane (A scaled by w and both shifted by c on the way in) and issues up to 16 MFMAs on
// them: each loaded value feeds four MFMAs from registers, which is the reason to use the matrix instruction here -- its
// float64 rate equals the vector rate on gfx950.  Only blocks and tiles with d_tile <= e_tile are computed; the fold
// kernel adds the waves' partial tiles in index order and writes both triangles from the same sum.
#include "estimators.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/mjhmc_hip.h"
#include "handles.hpp"
#include "ring_rows.hpp"
#include "ring_source.hpp"

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

// partial[(bx * 2 + m) * pitch + col] = the workgroup's sum of w (x - c)^(m + 1), partial_w[bx] = its sum of w
template <typename T>
__global__ __launch_bounds__(256) void est_moments_kernel(const T* __restrict__ base, const double* __restrict__ w,
                                                          const double* __restrict__ c, int64_t Npad, int64_t N, int n, int D,
                                                          int pitch, int cw, int log_cw, double* __restrict__ partial,
                                                          double* __restrict__ partial_w, int* __restrict__ bad) {
  constexpr int VEC = ChunkOf<T>::VEC;
  __shared__ double sm[256][2 * VEC + 1];
  const int tid = threadIdx.x;
  const int cx = tid & (cw - 1), ry = tid >> log_cw, rw = 256 >> log_cw;
  const int col0 = (blockIdx.y * cw + cx) * VEC;
  const bool active = col0 < pitch;
  double cs[VEC], s1[VEC], s2[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    cs[j] = (active && col0 + j < D) ? c[col0 + j] : 0.0;
    s1[j] = 0.0;
    s2[j] = 0.0;
  }
  double wsum = 0.0;
  int nonfinite = 0;
  const int64_t stride = (int64_t)gridDim.x * rw;
  for (int k = 0; k < n; ++k) {
    const T* slot = base + (size_t)k * Npad * pitch + col0;
    const double* wk = w ? w + (size_t)k * Npad : nullptr;
    for (int64_t p0 = (int64_t)blockIdx.x * rw + ry; p0 < N; p0 += stride * kRowsInFlight) {
      double x[kRowsInFlight][VEC], wt[kRowsInFlight];
#pragma unroll
      for (int u = 0; u < kRowsInFlight; ++u) {
        const int64_t p = p0 + u * stride;
        wt[u] = 0.0;
        if (p < N) {
          wt[u] = wk ? wk[p] : 1.0;
          if (active) ChunkOf<T>::widen(*reinterpret_cast<const uint4*>(slot + (size_t)p * pitch), x[u]);
        }
      }
#pragma unroll
      for (int u = 0; u < kRowsInFlight; ++u) {
        const int64_t p = p0 + u * stride;
        if (p < N) {
          if (!finite_f64(wt[u])) nonfinite = 1;
          wsum += wt[u];
          if (active) {
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
              const double d = x[u][j] - cs[j];
              const double wd = wt[u] * d;
              s1[j] += wd;
              s2[j] += wd * d;
            }
          }
        }
      }
    }
  }
  if (nonfinite) *bad = 1;
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    sm[tid][j] = s1[j];
    sm[tid][VEC + j] = s2[j];
  }
  sm[tid][2 * VEC] = wsum;
  __syncthreads();
  // the row lanes of a column, in index order
  for (int o = tid; o < cw * 2 * VEC; o += 256) {
    const int cxo = o / (2 * VEC), j = o - cxo * 2 * VEC;
    double t = 0.0;
    for (int r = 0; r < rw; ++r) t += sm[r * cw + cxo][j];
    const int col = (blockIdx.y * cw + cxo) * VEC + (j < VEC ? j : j - VEC);
    if (col < pitch) partial[((size_t)blockIdx.x * 2 + (j < VEC ? 0 : 1)) * pitch + col] = t;
  }
  if (blockIdx.y == 0 && tid == 0) {
    double t = 0.0;
    for (int r = 0; r < rw; ++r) t += sm[r * cw][2 * VEC];   // (every column lane of a row holds the same sum; lane 0's)
    partial_w[blockIdx.x] = t;
  }
}

// acc[0] += sum_b partial_w[b]; acc[1 + m * D + d] += sum_b partial[(b * 2 + m) * pitch + d].  A workgroup is 16 outputs x
// 16 lanes over b: lane q adds b = q, q + 16, ... in index order (16 consecutive doubles per load across the outputs),
// then the 16 lane sums are added in index order -- a fixed order for a given gx.
__global__ __launch_bounds__(256) void est_fold_moments_kernel(const double* __restrict__ partial,
                                                               const double* __restrict__ partial_w, int gx, int D, int pitch,
                                                               double* __restrict__ acc, const int* __restrict__ bad) {
  __shared__ double sm[16][17];
  const int o = threadIdx.x & 15, q = threadIdx.x >> 4;
  const int j = blockIdx.x * 16 + o;
  double t = 0.0;
  if (j <= 2 * D) {
    if (j == 0) {
#pragma unroll 8
      for (int b = q; b < gx; b += 16) t += partial_w[b];
    } else {
      const int m = (j - 1) / D, d = (j - 1) - m * D;
      const double* col = partial + (size_t)m * pitch + d;
#pragma unroll 8
      for (int b = q; b < gx; b += 16) t += col[(size_t)b * 2 * pitch];
    }
  }
  sm[q][o] = t;
  __syncthreads();
  if (q == 0 && j <= 2 * D && !*bad) {
    double s = 0.0;
    for (int r = 0; r < 16; ++r) s += sm[r][o];
    acc[j] += s;
  }
}

// (The wave-uniform run-time predicates around the MFMAs cost accumulator copies between AGPRs and VGPRs, 256 of the ~365
// vector instructions of a step; the compile-time form that removes them needs 300 VGPRs, one wave per SIMD, and ran at
// half the speed -- profiles/r07/estimators.md.)
// one wave = one (block pair, split): partial[((pair * splits + split) * 16 + ti * 4 + tj) * 256 + r * 64 + lane]
template <typename T>
__global__ __launch_bounds__(256) void est_cov_kernel(const T* __restrict__ base, const double* __restrict__ w,
                                                      const double* __restrict__ c, int64_t Npad, int64_t N, int n, int D,
                                                      int pitch, int nb, int splits, double* __restrict__ partial) {
  typedef typename ElemBits<T>::type Bits;   // (bfloat16 is loaded as its 16 bits)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int split = blockIdx.y * 4 + wave;
  // blockIdx.x -> (I, J), I <= J < nb, row-major over the upper triangle
  int I = 0, rest = blockIdx.x;
  while (rest >= nb - I) {
    rest -= nb - I;
    ++I;
  }
  const int J = I + rest;
  const bool diag = I == J;
  const int lr = lane & 15, lk = lane >> 4;
  int colA[4], colB[4];
  double cA[4], cB[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    colA[t] = I * 64 + t * 16 + lr;
    colB[t] = J * 64 + t * 16 + lr;
    cA[t] = colA[t] < D ? c[colA[t]] : 0.0;
    cB[t] = colB[t] < D ? c[colB[t]] : 0.0;
  }
  // (wave-uniform) tiles that exist and are needed
  bool tileA[4], tileB[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    tileA[t] = I * 64 + t * 16 < D;
    tileB[t] = J * 64 + t * 16 < D;
  }
  f64x4 acc[4][4];
#pragma unroll
  for (int ti = 0; ti < 4; ++ti)
#pragma unroll
    for (int tj = 0; tj < 4; ++tj) acc[ti][tj] = f64x4{0.0, 0.0, 0.0, 0.0};

  const int64_t nst = (N + 3) / 4;                         // groups of four particles per slot
  const int64_t mine = split < nst ? (nst - split + splits - 1) / splits : 0;   // this wave's groups per slot
  const int64_t total = mine * n;

  double xa[4], xb[4], wt;
  int fk = 0;          // slot and group (within the slot) of the next fetch: slots outermost, as the moment pass
  int64_t fst = split;
  auto fetch = [&](double* a, double* b, double& wgt) {
    const int64_t p = fst * 4 + lk;
    const bool live = p < N;
    wgt = live ? (w ? w[(size_t)fk * Npad + p] : 1.0) : 0.0;
    const Bits* row = reinterpret_cast<const Bits*>(base) + ((size_t)fk * Npad + (live ? p : 0)) * pitch;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      a[t] = (live && colA[t] < D) ? elem_to_f64(row[colA[t]]) : cA[t];
      if (!diag) b[t] = (live && colB[t] < D) ? elem_to_f64(row[colB[t]]) : cB[t];
    }
    fst += splits;
    if (fst >= nst) {
      fst = split;
      ++fk;
    }
  };
  if (total > 0) fetch(xa, xb, wt);
  for (int64_t i = 0; i < total; ++i) {
    double na[4], nb_[4], nw = 0.0;
#pragma unroll
    for (int t = 0; t < 4; ++t) na[t] = nb_[t] = 0.0;
    if (i + 1 < total) fetch(na, nb_, nw);
    double a[4], b[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const double da = xa[t] - cA[t];
      a[t] = wt * da;
      b[t] = diag ? da : xb[t] - cB[t];
    }
#pragma unroll
    for (int ti = 0; ti < 4; ++ti)
#pragma unroll
      for (int tj = 0; tj < 4; ++tj)
        if (tileA[ti] && tileB[tj] && (!diag || ti <= tj))
          acc[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ti], b[tj], acc[ti][tj], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      xa[t] = na[t];
      xb[t] = nb_[t];
    }
    wt = nw;
  }
  double* out = partial + ((size_t)blockIdx.x * splits + split) * 4096;
#pragma unroll
  for (int ti = 0; ti < 4; ++ti)
#pragma unroll
    for (int tj = 0; tj < 4; ++tj)
      if (tileA[ti] && tileB[tj] && (!diag || ti <= tj)) {
#pragma unroll
        for (int r = 0; r < 4; ++r) out[(ti * 4 + tj) * 256 + r * 64 + lane] = acc[ti][tj][r];
      }
}

// one thread per element of a block pair's 64 x 64 partial: the splits in index order, then both triangles of C
__global__ __launch_bounds__(256) void est_fold_cov_kernel(const double* __restrict__ partial, int nb, int pairs, int splits,
                                                           int D, double* __restrict__ C, const int* __restrict__ bad) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= (int64_t)pairs * 4096 || *bad) return;
  const int pair = (int)(g >> 12), o = (int)(g & 4095);
  int I = 0, rest = pair;
  while (rest >= nb - I) {
    rest -= nb - I;
    ++I;
  }
  const int J = I + rest;
  const int tile = o >> 8, r = (o >> 6) & 3, lane = o & 63;
  const int ti = tile >> 2, tj = tile & 3;
  const int gi = I * 4 + ti, gj = J * 4 + tj;
  const int d = gi * 16 + (lane >> 4) + 4 * r, e = gj * 16 + (lane & 15);
  if (gi > gj || d >= D || e >= D || (gi == gj && d > e)) return;
  double t = 0.0;
  for (int s = 0; s < splits; ++s) t += partial[((size_t)pair * splits + s) * 4096 + o];
  const double v = C[(size_t)d * D + e] + t;
  C[(size_t)d * D + e] = v;
  C[(size_t)e * D + d] = v;
}

}  // namespace

EstimatorPlan estimator_plan(const RingView& r, bool want_cov) {
  EstimatorPlan pl;
  pl.vec = r.dtype == MJHMC_F64 ? 2 : (r.dtype == MJHMC_F32 ? 4 : 8);
  const int chunks = (r.pitch + pl.vec - 1) / pl.vec;
  pl.cw = std::min(256, pow2ceil(chunks));
  pl.log_cw = ilog2(pl.cw);
  pl.gy = (chunks + pl.cw - 1) / pl.cw;
  const int rw = 256 / pl.cw;
  // about four workgroups per compute unit, each with at least kRowsInFlight rows per row lane
  const int64_t want = std::max<int64_t>(1, 1024 / pl.gy);
  const int64_t have = (r.N + (int64_t)rw * kRowsInFlight - 1) / ((int64_t)rw * kRowsInFlight);
  pl.gx = (int)std::max<int64_t>(1, std::min(want, have));
  pl.moment_partial_elems = (size_t)pl.gx * 2 * r.pitch + pl.gx;
  if (want_cov && r.D <= kEstimatorMaxCovDims) {
    pl.nb = (r.D + 63) / 64;
    pl.pairs = pl.nb * (pl.nb + 1) / 2;
    const int64_t groups = (r.N + 3) / 4;
    // two waves per SIMD over the device (2048), at least 16 groups of four particles per wave, a multiple of 4 waves
    int64_t sp = std::max<int64_t>(1, 2048 / pl.pairs);
    sp = std::min(sp, std::max<int64_t>(1, groups / 16));
    pl.splits = (int)((sp + 3) / 4 * 4);
    pl.cov_partial_elems = (size_t)pl.pairs * pl.splits * 4096;
  }
  return pl;
}

int estimator_moments(hipStream_t st, const RingView& r, int n, const double* w, const double* c, const EstimatorPlan& pl,
                      double* partial, double* acc, int* bad, std::string& err) {
  double* partial_w = partial + (size_t)pl.gx * 2 * r.pitch;
  const dim3 grid(pl.gx, pl.gy), block(256);
  dispatch_dtype(r.dtype, [&](auto tag) {
    typedef typename decltype(tag)::type T;
    hipLaunchKernelGGL(est_moments_kernel<T>, grid, block, 0, st, (const T*)r.base, w, c, r.Npad, r.N, n, r.D, r.pitch, pl.cw,
                       pl.log_cw, partial, partial_w, bad);
  });
  hipLaunchKernelGGL(est_fold_moments_kernel, dim3((2 * r.D + 1 + 15) / 16), dim3(256), 0, st, partial, partial_w, pl.gx,
                     r.D, r.pitch, acc, bad);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    err = std::string("moment pass: ") + hipGetErrorString(e);
    return MJHMC_ERR_HIP;
  }
  return 0;
}

int estimator_cov(hipStream_t st, const RingView& r, int n, const double* w, const double* c, const EstimatorPlan& pl,
                  double* partial, double* C, const int* bad, std::string& err) {
  if (r.D > kEstimatorMaxCovDims || pl.pairs < 1) {
    err = "the covariance pass takes at most " + std::to_string(kEstimatorMaxCovDims) + " dims (this ring has " +
          std::to_string(r.D) + "): first and second moments only";
    return MJHMC_ERR_INVALID;
  }
  const dim3 grid(pl.pairs, pl.splits / 4), block(256);
  dispatch_dtype(r.dtype, [&](auto tag) {
    typedef typename decltype(tag)::type T;
    hipLaunchKernelGGL(est_cov_kernel<T>, grid, block, 0, st, (const T*)r.base, w, c, r.Npad, r.N, n, r.D, r.pitch, pl.nb,
                       pl.splits, partial);
  });
  hipLaunchKernelGGL(est_fold_cov_kernel, dim3((unsigned)(((size_t)pl.pairs * 4096 + 255) / 256)), dim3(256), 0, st, partial,
                     pl.nb, pl.pairs, pl.splits, r.D, C, bad);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    err = std::string("covariance pass: ") + hipGetErrorString(e);
    return MJHMC_ERR_HIP;
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// The accumulator handle of the C ABI (include/mjhmc_hip.h: mjhmc_estimator_*)
// ---------------------------------------------------------------------------------------------------------------------
struct mjhmc_estimator : RingAccumulator {
  using RingAccumulator::RingAccumulator;
  int D = 0;                  // dimensions of a state of that ring
  bool want_cov = false;
  EstimatorPlan plan;
  double* acc = nullptr;      // [1 + 2 D]: W, S1, S2
  double* C = nullptr;        // [D][D]
  double* shift = nullptr;    // [D]
  double* mpart = nullptr;
  double* cpart = nullptr;
  ~mjhmc_estimator() override { free_device({acc, C, shift, mpart, cpart}); }
};

static int estimator_create_on_source(mjhmc_sampler* s, const mjhmc_functionals* fn, int want_cov, mjhmc_estimator** out) {
  const RingSource src = ring_source(s, fn);
  if (!src.base) return acc_no_ring(fn);
  if (want_cov && src.D > kEstimatorMaxCovDims)
    return mjhmc_fail(MJHMC_ERR_INVALID, "the covariance pass takes at most " + std::to_string(kEstimatorMaxCovDims) +
                                             " dims (ndims = " + std::to_string(src.D) + "): ask for the moments only");
  HIPCHK(hipSetDevice(s->ctx->device));
  mjhmc_estimator* est = new mjhmc_estimator("estimator", "estimator", s, fn, src);
  est->D = src.D;
  est->want_cov = want_cov != 0;
  est->plan = estimator_plan(ring_source_view(s, src, 0), est->want_cov);
  const size_t D = (size_t)src.D;
  hipError_t e = hipMalloc((void**)&est->acc, (1 + 2 * D) * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&est->shift, D * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&est->mpart, est->plan.moment_partial_elems * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&est->bad, sizeof(int));
  if (e == hipSuccess && est->want_cov) e = hipMalloc((void**)&est->C, D * D * sizeof(double));
  if (e == hipSuccess && est->want_cov) e = hipMalloc((void**)&est->cpart, est->plan.cov_partial_elems * sizeof(double));
  if (e == hipSuccess) e = hipMemsetAsync(est->acc, 0, (1 + 2 * D) * sizeof(double), s->stream);
  if (e == hipSuccess) e = hipMemsetAsync(est->shift, 0, D * sizeof(double), s->stream);
  if (e == hipSuccess) e = hipMemsetAsync(est->bad, 0, sizeof(int), s->stream);
  if (e == hipSuccess && est->want_cov) e = hipMemsetAsync(est->C, 0, D * D * sizeof(double), s->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
  if (e != hipSuccess) {
    delete est;
    (void)hipGetLastError();
    return mjhmc_fail(MJHMC_ERR_HIP, std::string("estimator buffers: ") + hipGetErrorString(e));
  }
  return acc_created(est, out);
}

extern "C" {

int mjhmc_estimator_create(mjhmc_sampler* s, int want_cov, mjhmc_estimator** out) {
  if (!s || !out) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  return estimator_create_on_source(s, nullptr, want_cov, out);
}

int mjhmc_estimator_create_on(mjhmc_functionals* f, int want_cov, mjhmc_estimator** out) {
  if (!f || !out) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  return estimator_create_on_source(functionals_sampler(f), f, want_cov, out);
}

int mjhmc_estimator_destroy(mjhmc_estimator* est) { return acc_destroy(est); }

int mjhmc_estimator_reset(mjhmc_estimator* est) {
  if (!est) return mjhmc_fail(MJHMC_ERR_INVALID, "estimator is NULL");
  mjhmc_sampler* s = est->s;
  HIPCHK(hipSetDevice(s->ctx->device));
  const size_t D = (size_t)est->D;
  HIPCHK(hipMemsetAsync(est->acc, 0, (1 + 2 * D) * sizeof(double), s->stream));
  if (est->want_cov) HIPCHK(hipMemsetAsync(est->C, 0, D * D * sizeof(double), s->stream));
  HIPCHK(hipMemsetAsync(est->bad, 0, sizeof(int), s->stream));
  est->n_states = 0;
  return 0;
}

int mjhmc_estimator_set_shift(mjhmc_estimator* est, const double* c) {
  if (!est) return mjhmc_fail(MJHMC_ERR_INVALID, "estimator is NULL");
  if (est->n_states != 0)
    return mjhmc_fail(MJHMC_ERR_INVALID, "the shift belongs to the sums already accumulated: mjhmc_estimator_reset first");
  mjhmc_sampler* s = est->s;
  HIPCHK(hipSetDevice(s->ctx->device));
  const size_t bytes = (size_t)est->D * sizeof(double);
  if (c) {
    for (int d = 0; d < est->D; ++d)
      if (!std::isfinite(c[d])) return mjhmc_fail(MJHMC_ERR_INVALID, "shift entry " + std::to_string(d) + " is not finite");
    HIPCHK(hipMemcpyAsync(est->shift, c, bytes, hipMemcpyHostToDevice, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));   // (c is the caller's for the duration of the call only)
  } else {
    HIPCHK(hipMemsetAsync(est->shift, 0, bytes, s->stream));
  }
  return 0;
}

int mjhmc_estimator_accumulate(mjhmc_estimator* est, int x_slot0, int w_slot0, int n) {
  if (!est) return mjhmc_fail(MJHMC_ERR_INVALID, "estimator is NULL");
  mjhmc_sampler* s = est->s;
  RingSource src;
  TRY(acc_begin(est, x_slot0, w_slot0, n, &src));
  HIPCHK(hipSetDevice(s->ctx->device));
  const RingView view = ring_source_view(s, src, x_slot0);
  const double* w = acc_weights(est, w_slot0);
  std::string err;
  int rc = estimator_moments(s->stream, view, n, w, est->shift, est->plan, est->mpart, est->acc, est->bad, err);
  if (!rc && est->want_cov) rc = estimator_cov(s->stream, view, n, w, est->shift, est->plan, est->cpart, est->C, est->bad, err);
  if (rc) return mjhmc_fail(rc, err);
  return acc_end(est, n, [&](int) { return acc_nonfinite_dwell(w_slot0, n); });
}

int mjhmc_estimator_read(mjhmc_estimator* est, double* W, double* S1, double* S2, double* C, int64_t* n_states) {
  if (!est || !W || !S1 || !S2 || !n_states) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  if (C && !est->want_cov) return mjhmc_fail(MJHMC_ERR_INVALID, "this estimator was created without the covariance");
  mjhmc_sampler* s = est->s;
  HIPCHK(hipSetDevice(s->ctx->device));
  const size_t D = (size_t)est->D;
  std::vector<double> h(1 + 2 * D);
  HIPCHK(hipMemcpyAsync(h.data(), est->acc, h.size() * sizeof(double), hipMemcpyDeviceToHost, s->stream));
  if (C) HIPCHK(hipMemcpyAsync(C, est->C, D * D * sizeof(double), hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  *W = h[0];
  std::copy(h.begin() + 1, h.begin() + 1 + D, S1);
  std::copy(h.begin() + 1 + D, h.end(), S2);
  *n_states = est->n_states;
  return 0;
}

#ifdef MJHMC_TEST_HOOKS
// test build only: one entry of the dwell ring (what a zero total rate would leave there)
int mjhmc_test_ring_write_dwell(mjhmc_sampler* s, int slot, int64_t particle, double value) {
  if (!s || slot < 0 || slot >= s->ring_slots || particle < 0 || particle >= s->N)
    return mjhmc_fail(MJHMC_ERR_INVALID, "bad argument");
  HIPCHK(hipSetDevice(s->ctx->device));
  HIPCHK(hipMemcpyAsync(s->dwell_ring + (size_t)slot * s->Npad + particle, &value, sizeof(double), hipMemcpyHostToDevice,
                        s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  return 0;
}
#endif

}  // extern "C"
