// Device control variates (include/mjhmc_hip.h: mjhmc_crossmoments_*): the sums from which f - beta^T g, g = dE/dX,
// beta = Cov(g,g)^-1 Cov(g,f), is formed on the host -- the first-order zero-variance control variates of Mira, Solgi and
// Imparato (2013); E_p[g] = 0 for every target p = exp(-E) / Z that vanishes at infinity.
//
// Per recorded slot, in stream order on the sampler's stream:
//   1. the sampler's own evaluation kernels on the sample-ring slot (state_io.hip: sampler_eval_rows) into the handle's gradient
//      matrix G and energy vector, in the layout and types the energy family writes (as stein.hip);
//   2. the moment and covariance passes of estimators.hip on G seen as a one-slot ring, about 0: W, Sg, S2g, Cgg;
//   3. the moment pass on the matching slot of the handle's RingSource (sample ring or derived ring), about cb: Sb, S2b;
//   4. the cross pass of this file: Cgb.
// Every slot is added to the running totals separately, so the sums do not depend on how a run is cut into calls.
//
// Cross pass (D, K <= 512): Cgb = G^T diag(w) (B - cb) is a rank-N update whose contraction axis is the particle axis, as
// the covariance pass of estimators.hip, and the kernel is modelled on est_cov_kernel (read its header comment first):
// v_mfma_f64_16x16x4_f64, a wave owns a 64 x 64 block of the output (4 x 4 tiles, 128 accumulator registers), takes every
// `splits`-th group of four particles, forms A = w * G and B - cb on the way in and issues the next group's loads before
// the current group's MFMAs.  What differs: the block grid is the full rectangle ceil(D / 64) x ceil(K / 64) (no
// triangle, no diagonal shortcut), and A and B have their own base pointers, element types and pitches.  Tiles past D or
// K are skipped by the same wave-uniform run-time predicates (the compile-time form ran at half the speed there).
// Partials go to a scratch buffer and the fold kernel adds the splits in index order.  Rows p >= N are never read; a
// dead lane of a partial group of four supplies w = 0 and zeros, so it adds nothing.
#include "crossmoments.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "../../include/mjhmc_hip.h"
#include "estimators.hpp"
#include "handles.hpp"
#include "ring_rows.hpp"
#include "ring_source.hpp"

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

// one wave = one (block, split): partial[((block * splits + split) * 16 + ti * 4 + tj) * 256 + r * 64 + lane]
template <typename TG, typename TB>
__global__ __launch_bounds__(256) void xcov_kernel(const TG* __restrict__ G, const TB* __restrict__ B,
                                                   const double* __restrict__ w, const double* __restrict__ cb, int64_t N, int D,
                                                   int K, int pitchG, int pitchB, int nbk, int splits,
                                                   double* __restrict__ partial) {
  typedef typename ElemBits<TG>::type BitsG;
  typedef typename ElemBits<TB>::type BitsB;   // (bfloat16 is loaded as its 16 bits)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int split = blockIdx.y * 4 + wave;
  const int I = blockIdx.x / nbk, J = blockIdx.x - I * nbk;   // row-major over the rectangle
  const int lr = lane & 15, lk = lane >> 4;
  int colA[4], colB[4];
  double cB[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    colA[t] = I * 64 + t * 16 + lr;
    colB[t] = J * 64 + t * 16 + lr;
    cB[t] = colB[t] < K ? cb[colB[t]] : 0.0;
  }
  // (wave-uniform) tiles that exist
  bool tileA[4], tileB[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    tileA[t] = I * 64 + t * 16 < D;
    tileB[t] = J * 64 + t * 16 < K;
  }
  f64x4 acc[4][4];
#pragma unroll
  for (int ti = 0; ti < 4; ++ti)
#pragma unroll
    for (int tj = 0; tj < 4; ++tj) acc[ti][tj] = f64x4{0.0, 0.0, 0.0, 0.0};

  const int64_t nst = (N + 3) / 4;                                              // groups of four particles
  const int64_t mine = split < nst ? (nst - split + splits - 1) / splits : 0;   // this wave's groups

  double xa[4], xb[4], wt;
  int64_t fst = split;   // group of the next fetch
  auto fetch = [&](double* a, double* b, double& wgt) {
    const int64_t p = fst * 4 + lk;
    const bool live = p < N;
    wgt = live ? (w ? w[p] : 1.0) : 0.0;
    const BitsG* rowG = reinterpret_cast<const BitsG*>(G) + (size_t)(live ? p : 0) * pitchG;
    const BitsB* rowB = reinterpret_cast<const BitsB*>(B) + (size_t)(live ? p : 0) * pitchB;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      a[t] = (live && colA[t] < D) ? elem_to_f64(rowG[colA[t]]) : 0.0;
      b[t] = (live && colB[t] < K) ? elem_to_f64(rowB[colB[t]]) : cB[t];
    }
    fst += splits;
  };
  if (mine > 0) fetch(xa, xb, wt);
  for (int64_t i = 0; i < mine; ++i) {
    double na[4], nb_[4], nw = 0.0;
#pragma unroll
    for (int t = 0; t < 4; ++t) na[t] = nb_[t] = 0.0;
    if (i + 1 < mine) fetch(na, nb_, nw);
    double a[4], b[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      a[t] = wt * xa[t];
      b[t] = xb[t] - cB[t];
    }
#pragma unroll
    for (int ti = 0; ti < 4; ++ti)
#pragma unroll
      for (int tj = 0; tj < 4; ++tj)
        if (tileA[ti] && tileB[tj]) acc[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ti], b[tj], acc[ti][tj], 0, 0, 0);
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
      if (tileA[ti] && tileB[tj]) {
#pragma unroll
        for (int r = 0; r < 4; ++r) out[(ti * 4 + tj) * 256 + r * 64 + lane] = acc[ti][tj][r];
      }
}

// one thread per element of a block's 64 x 64 partial: the splits in index order, added to Cgb[d][k]
__global__ __launch_bounds__(256) void xcov_fold_kernel(const double* __restrict__ partial, int nbk, int blocks, int splits, int D,
                                                        int K, double* __restrict__ Cgb, const int* __restrict__ bad) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= (int64_t)blocks * 4096 || *bad) return;
  const int blk = (int)(g >> 12), o = (int)(g & 4095);
  const int I = blk / nbk, J = blk - I * nbk;
  const int tile = o >> 8, r = (o >> 6) & 3, lane = o & 63;
  const int ti = tile >> 2, tj = tile & 3;
  const int d = (I * 4 + ti) * 16 + (lane >> 4) + 4 * r, k = (J * 4 + tj) * 16 + (lane & 15);
  if (d >= D || k >= K) return;   // (an element inside D x K lies in a tile the waves wrote)
  double t = 0.0;
  for (int s = 0; s < splits; ++s) t += partial[((size_t)blk * splits + s) * 4096 + o];
  Cgb[(size_t)d * K + k] += t;
}

// flags[0] = 1 when one of the n * N weights of the call is not finite (what the moment pass raises per block, here for
// the whole call ahead of its first slot: the folds of every slot then add nothing)
__global__ __launch_bounds__(256) void xcov_check_weights_kernel(const double* __restrict__ w, int64_t Npad, int64_t N, int n,
                                                                 int* __restrict__ flags) {
  const int64_t total = (int64_t)n * N, stride = (int64_t)gridDim.x * 256;
  int nonfinite = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const int64_t k = i / N, p = i - k * N;
    if (!finite_f64(w[(size_t)k * Npad + p])) nonfinite = 1;
  }
  if (nonfinite) flags[0] = 1;
}

// flags[1] = min(flags[1], slot * 4 + what) for a value of a row p < N that is not finite: what = 0 a state element, 1 an
// element of dE/dX, 2 an energy.  (An integer atomic: the lowest code wins whatever the schedule.)
template <typename TX, typename TG>
__global__ __launch_bounds__(256) void xcov_check_slot_kernel(const TX* __restrict__ X, const TG* __restrict__ G,
                                                              const TG* __restrict__ E, int64_t N, int D, int pitch, int slot,
                                                              int* __restrict__ flags) {
  typedef typename ElemBits<TX>::type BitsX;
  const int64_t total = N * pitch, stride = (int64_t)gridDim.x * 256;
  int what = 3;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const int64_t p = i / pitch;
    const int d = (int)(i - p * pitch);
    if (d >= D) continue;
    if (!finite_f64(elem_to_f64(reinterpret_cast<const BitsX*>(X)[i]))) what = 0;
    if (what > 1 && !finite_f64((double)G[i])) what = 1;
    if (d == 0 && what > 2 && !finite_f64((double)E[p])) what = 2;
  }
  if (what < 3) atomicMin(flags + 1, slot * 4 + what);
}

constexpr int kNoBadSlot = INT_MAX;

}  // namespace

CrossPlan cross_plan(int64_t N, int D, int K) {
  CrossPlan pl;
  pl.nbg = (D + 63) / 64;
  pl.nbk = (K + 63) / 64;
  pl.blocks = pl.nbg * pl.nbk;
  const int64_t groups = (N + 3) / 4;
  // as the covariance pass: two waves per SIMD over the device (2048), at least 16 groups of four particles per wave, a
  // multiple of 4 waves
  int64_t sp = std::max<int64_t>(1, 2048 / pl.blocks);
  sp = std::min(sp, std::max<int64_t>(1, groups / 16));
  pl.splits = (int)((sp + 3) / 4 * 4);
  pl.partial_elems = (size_t)pl.blocks * pl.splits * 4096;
  return pl;
}

int cross_cov(hipStream_t st, const RingView& g, const RingView& b, const double* w, const double* cb, const CrossPlan& pl,
              double* partial, double* Cgb, const int* bad, std::string& err) {
  if (g.D > kEstimatorMaxCovDims || b.D > kEstimatorMaxCovDims || pl.blocks < 1) {
    err = "the cross pass takes at most " + std::to_string(kEstimatorMaxCovDims) + " x " + std::to_string(kEstimatorMaxCovDims) +
          " values (this one has " + std::to_string(g.D) + " x " + std::to_string(b.D) + ")";
    return MJHMC_ERR_INVALID;
  }
  if (g.N != b.N || (g.dtype != MJHMC_F64 && g.dtype != MJHMC_F32) || (g.dtype == MJHMC_F64 && b.dtype != MJHMC_F64)) {
    err = "no cross-moment kernel for this pair of gradient and ring types";
    return MJHMC_ERR_UNSUPPORTED;
  }
  const dim3 grid(pl.blocks, pl.splits / 4), block(256);
  if (g.dtype == MJHMC_F64) {
    hipLaunchKernelGGL((xcov_kernel<double, double>), grid, block, 0, st, (const double*)g.base, (const double*)b.base, w, cb, g.N,
                       g.D, b.D, g.pitch, b.pitch, pl.nbk, pl.splits, partial);
  } else {
    dispatch_dtype(b.dtype, [&](auto tag) {
      typedef typename decltype(tag)::type TB;
      hipLaunchKernelGGL((xcov_kernel<float, TB>), grid, block, 0, st, (const float*)g.base, (const TB*)b.base, w, cb, g.N, g.D,
                         b.D, g.pitch, b.pitch, pl.nbk, pl.splits, partial);
    });
  }
  hipLaunchKernelGGL(xcov_fold_kernel, dim3((unsigned)(((size_t)pl.blocks * 4096 + 255) / 256)), dim3(256), 0, st, partial, pl.nbk,
                     pl.blocks, pl.splits, g.D, b.D, Cgb, bad);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    err = std::string("cross pass: ") + hipGetErrorString(e);
    return MJHMC_ERR_HIP;
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// The accumulator handle of the C ABI (include/mjhmc_hip.h: mjhmc_crossmoments_*)
// ---------------------------------------------------------------------------------------------------------------------
struct mjhmc_crossmoments : RingAccumulator {
  using RingAccumulator::RingAccumulator;
  int D = 0, K = 0;             // dimensions of a state (of dE/dX) and of a row of the source ring
  uint64_t sample_gen = 0;      // the sampler's sample ring at create (the gradient is evaluated from it whatever the source)
  int gdtype = MJHMC_F64;       // float64 dE/dX exactly where the state is float64 (stein.hip)
  void* G = nullptr;            // [Npad][pitch] dE/dX of one slot
  void* E = nullptr;            // [Npad] its energies, of the same type
  EstimatorPlan gplan, bplan;   // the passes over G (moments + covariance) and over the source (moments)
  CrossPlan xplan;
  double* accg = nullptr;       // [1 + 2 D]: W as the pass over G adds it (not read), Sg, S2g
  double* accb = nullptr;       // [1 + 2 K]: W, Sb, S2b
  double* Cgg = nullptr;        // [D][D]
  double* Cgb = nullptr;        // [D][K]
  double* shift = nullptr;      // [K] cb
  double* zero = nullptr;       // [D] the shift of the gradient sums: its known mean
  double* mpart_g = nullptr;
  double* mpart_b = nullptr;
  double* cpart = nullptr;
  double* xpart = nullptr;
  bool poisoned = false;        // a non-finite state, gradient or energy went into the sums: reset first
  // (`bad` holds two flags: [0] a non-finite weight, what the estimator passes raise and obey; [1] the lowest
  // slot * 4 + what of a non-finite value, kNoBadSlot when there is none)
  ~mjhmc_crossmoments() override {
    free_device({G, E, accg, accb, Cgg, Cgb, shift, zero, mpart_g, mpart_b, cpart, xpart});
  }
  RingView grad_view() const { return RingView{G, gdtype, s->Npad, s->N, D, s->sh.pitch}; }
};

namespace {

hipError_t cross_zero_sums(mjhmc_crossmoments* h) {
  mjhmc_sampler* s = h->s;
  const size_t D = (size_t)h->D, K = (size_t)h->K;
  const int flags[2] = {0, kNoBadSlot};
  hipError_t e = hipMemsetAsync(h->accg, 0, (1 + 2 * D) * sizeof(double), s->stream);
  if (e == hipSuccess) e = hipMemsetAsync(h->accb, 0, (1 + 2 * K) * sizeof(double), s->stream);
  if (e == hipSuccess) e = hipMemsetAsync(h->Cgg, 0, D * D * sizeof(double), s->stream);
  if (e == hipSuccess) e = hipMemsetAsync(h->Cgb, 0, D * K * sizeof(double), s->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(h->bad, flags, sizeof(flags), hipMemcpyHostToDevice, s->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(s->stream);   // (flags is on this stack)
  return e;
}

int cross_create_on_source(mjhmc_sampler* s, const mjhmc_functionals* fn, mjhmc_crossmoments** out) {
  if (s->en->is_host())
    return mjhmc_fail(MJHMC_ERR_UNSUPPORTED,
                      "a host-evaluated energy has no device evaluation: the caller's callables are the only evaluation of "
                      "dE/dX, so the control variates of its states are the caller's to form");
  if (s->sh.wide)
    return mjhmc_fail(MJHMC_ERR_UNSUPPORTED,
                      "a sampler on the wide (multi-pass) path -- rows beyond the register-resident kernels, or ProductOfT and "
                      "linear-model energies with float64 state -- has no single-launch evaluation of dE/dX here: the control "
                      "variates of its states are not formed (float32 state runs the tile kernels)");
  if (!s->ring) return acc_no_ring(nullptr);
  const RingSource src = ring_source(s, fn);
  if (!src.base) return acc_no_ring(fn);
  if (s->D > kEstimatorMaxCovDims || src.D > kEstimatorMaxCovDims)
    return mjhmc_fail(MJHMC_ERR_INVALID, "the cross moments take at most " + std::to_string(kEstimatorMaxCovDims) +
                                             " dims and " + std::to_string(kEstimatorMaxCovDims) + " values (ndims = " +
                                             std::to_string(s->D) + ", K = " + std::to_string(src.D) + ")");
  // the passes load 16 bytes of a row at once: rows must be whole 16-byte chunks of the state's type
  const int vec = s->dtype == MJHMC_F64 ? 2 : (s->dtype == MJHMC_F32 ? 4 : 8);
  if (s->sh.esize * vec != 16 || s->sh.pitch % vec != 0)
    return mjhmc_fail(MJHMC_ERR_UNSUPPORTED, "the sampler's rows are not whole 16-byte chunks of its state type");
  HIPCHK(hipSetDevice(s->ctx->device));
  mjhmc_crossmoments* h = new mjhmc_crossmoments("crossmoments", "cross-moment handle", s, fn, src);
  h->D = s->D;
  h->K = src.D;
  h->sample_gen = s->ring_gen;
  h->gdtype = s->dtype == MJHMC_F64 ? MJHMC_F64 : MJHMC_F32;
  h->gplan = estimator_plan(RingView{nullptr, h->gdtype, s->Npad, s->N, h->D, s->sh.pitch}, true);
  h->bplan = estimator_plan(ring_source_view(s, src, 0), false);
  h->xplan = cross_plan(s->N, h->D, h->K);
  const size_t D = (size_t)h->D, K = (size_t)h->K;
  // dE/dX has the state's row pitch in every family (stein.hip, functionals.hip)
  const size_t gsize = h->gdtype == MJHMC_F64 ? 8 : 4;
  const size_t gbytes = (size_t)s->Npad * s->sh.pitch * gsize, ebytes = (size_t)s->Npad * gsize;
  hipError_t e = hipMalloc(&h->G, gbytes);
  if (e == hipSuccess) e = hipMalloc(&h->E, ebytes);
  if (e == hipSuccess) e = hipMalloc((void**)&h->accg, (1 + 2 * D) * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&h->accb, (1 + 2 * K) * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&h->Cgg, D * D * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&h->Cgb, D * K * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&h->shift, K * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&h->zero, D * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&h->mpart_g, h->gplan.moment_partial_elems * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&h->mpart_b, h->bplan.moment_partial_elems * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&h->cpart, h->gplan.cov_partial_elems * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&h->xpart, h->xplan.partial_elems * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&h->bad, 2 * sizeof(int));
  if (e == hipSuccess) e = hipMemsetAsync(h->G, 0, gbytes, s->stream);
  if (e == hipSuccess) e = hipMemsetAsync(h->E, 0, ebytes, s->stream);
  if (e == hipSuccess) e = hipMemsetAsync(h->shift, 0, K * sizeof(double), s->stream);
  if (e == hipSuccess) e = hipMemsetAsync(h->zero, 0, D * sizeof(double), s->stream);
  if (e == hipSuccess) e = cross_zero_sums(h);
  if (e != hipSuccess) {
    delete h;
    (void)hipGetLastError();
    return mjhmc_fail(MJHMC_ERR_HIP, std::string("cross-moment buffers: ") + hipGetErrorString(e));
  }
  return acc_created(h, out);
}

}  // namespace

extern "C" {

int mjhmc_crossmoments_create(mjhmc_sampler* s, mjhmc_crossmoments** out) {
  if (!s || !out) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  return cross_create_on_source(s, nullptr, out);
}

int mjhmc_crossmoments_create_on(mjhmc_functionals* f, mjhmc_crossmoments** out) {
  if (!f || !out) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  return cross_create_on_source(functionals_sampler(f), f, out);
}

int mjhmc_crossmoments_destroy(mjhmc_crossmoments* h) { return acc_destroy(h); }

int mjhmc_crossmoments_info(mjhmc_crossmoments* h, int* ndims, int* n_values) {
  if (!h || !ndims || !n_values) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  *ndims = h->D;
  *n_values = h->K;
  return 0;
}

int mjhmc_crossmoments_reset(mjhmc_crossmoments* h) {
  if (!h) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  HIPCHK(hipSetDevice(h->s->ctx->device));
  HIPCHK(cross_zero_sums(h));
  h->n_states = 0;
  h->poisoned = false;
  return 0;
}

int mjhmc_crossmoments_set_shift(mjhmc_crossmoments* h, const double* cb) {
  if (!h) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  if (h->n_states != 0 || h->poisoned)
    return mjhmc_fail(MJHMC_ERR_INVALID, "the shift belongs to the sums already accumulated: mjhmc_crossmoments_reset first");
  mjhmc_sampler* s = h->s;
  HIPCHK(hipSetDevice(s->ctx->device));
  const size_t bytes = (size_t)h->K * sizeof(double);
  if (cb) {
    for (int k = 0; k < h->K; ++k)
      if (!std::isfinite(cb[k])) return mjhmc_fail(MJHMC_ERR_INVALID, "shift entry " + std::to_string(k) + " is not finite");
    HIPCHK(hipMemcpyAsync(h->shift, cb, bytes, hipMemcpyHostToDevice, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));   // (cb is the caller's for the duration of the call only)
  } else {
    HIPCHK(hipMemsetAsync(h->shift, 0, bytes, s->stream));
  }
  return 0;
}

int mjhmc_crossmoments_accumulate(mjhmc_crossmoments* h, int x_slot0, int w_slot0, int n) {
  if (!h) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  mjhmc_sampler* s = h->s;
  if (h->poisoned)
    return mjhmc_fail(MJHMC_ERR_INVALID, "the sums hold a value that is not finite (an earlier mjhmc_crossmoments_accumulate "
                                         "said which): mjhmc_crossmoments_reset first");
  RingSource src;
  TRY(acc_begin(h, x_slot0, w_slot0, n, &src));
  if (h->sample_gen != s->ring_gen)
    return mjhmc_fail(MJHMC_ERR_INVALID, "the sample ring was re-allocated after mjhmc_crossmoments_create: create a new "
                                         "cross-moment handle");
  if ((int64_t)x_slot0 + n > s->ring_slots)
    return mjhmc_fail(MJHMC_ERR_INVALID, "state slots [" + std::to_string(x_slot0) + ", " + std::to_string((int64_t)x_slot0 + n) +
                                             ") are outside the sample ring of " + std::to_string(s->ring_slots));
  HIPCHK(hipSetDevice(s->ctx->device));
  const int64_t check_blocks = std::min<int64_t>(1024, (s->N * s->sh.pitch + 255) / 256);
  if (w_slot0 >= 0)
    hipLaunchKernelGGL(xcov_check_weights_kernel, dim3((unsigned)std::min<int64_t>(1024, ((int64_t)n * s->N + 255) / 256)),
                       dim3(256), 0, s->stream, acc_weights(h, w_slot0), s->Npad, s->N, n, h->bad);
  const RingView gview = h->grad_view();
  std::string err;
  int rc = 0;
  for (int j = 0; j < n && !rc; ++j) {
    const char* X = (const char*)s->ring + (size_t)(x_slot0 + j) * mat_bytes(s);
    rc = sampler_eval_rows(s, X, h->G, h->E);
    if (rc) {
      h->poisoned = j > 0;   // (earlier slots of this call are in the sums; the call is not)
      return rc;
    }
    dispatch_dtype(s->dtype, [&](auto tag) {
      typedef typename decltype(tag)::type TX;
      if (h->gdtype == MJHMC_F64)
        hipLaunchKernelGGL((xcov_check_slot_kernel<TX, double>), dim3((unsigned)check_blocks), dim3(256), 0, s->stream,
                           (const TX*)X, (const double*)h->G, (const double*)h->E, s->N, h->D, s->sh.pitch, x_slot0 + j, h->bad);
      else
        hipLaunchKernelGGL((xcov_check_slot_kernel<TX, float>), dim3((unsigned)check_blocks), dim3(256), 0, s->stream,
                           (const TX*)X, (const float*)h->G, (const float*)h->E, s->N, h->D, s->sh.pitch, x_slot0 + j, h->bad);
    });
    const double* w = w_slot0 >= 0 ? acc_weights(h, w_slot0 + j) : nullptr;
    const RingView bview = ring_source_view(s, src, x_slot0 + j);
    rc = estimator_moments(s->stream, gview, 1, w, h->zero, h->gplan, h->mpart_g, h->accg, h->bad, err);
    if (!rc) rc = estimator_cov(s->stream, gview, 1, w, h->zero, h->gplan, h->cpart, h->Cgg, h->bad, err);
    if (!rc) rc = estimator_moments(s->stream, bview, 1, w, h->shift, h->bplan, h->mpart_b, h->accb, h->bad, err);
    if (!rc) rc = cross_cov(s->stream, gview, bview, w, h->shift, h->xplan, h->xpart, h->Cgb, h->bad, err);
  }
  if (rc) {
    h->poisoned = true;   // (part of the call may be in the sums)
    return mjhmc_fail(rc, err);
  }
  int flags[2] = {0, kNoBadSlot};
  HIPCHK(hipMemcpyAsync(flags, h->bad, sizeof(flags), hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  if (flags[0] || flags[1] != kNoBadSlot) {
    const int clear[2] = {0, kNoBadSlot};
    HIPCHK(hipMemcpyAsync(h->bad, clear, sizeof(clear), hipMemcpyHostToDevice, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
  }
  if (flags[0]) return acc_nonfinite_dwell(w_slot0, n);   // (every fold of the call saw the flag: nothing was added)
  if (flags[1] != kNoBadSlot) {
    static const char* const what[3] = {"a state", "a gradient (dE/dX)", "an energy"};
    h->poisoned = true;
    return mjhmc_fail(MJHMC_ERR_NONFINITE, std::string(what[flags[1] & 3]) + " of slot " + std::to_string(flags[1] >> 2) +
                                               " is not finite: the control variates of this run are not defined, and the "
                                               "sums hold it -- mjhmc_crossmoments_reset before any further call");
  }
  h->n_states += (int64_t)n * s->N;
  return 0;
}

int mjhmc_crossmoments_read(mjhmc_crossmoments* h, double* W, double* Sg, double* S2g, double* Sb, double* S2b, double* Cgg,
                            double* Cgb, int64_t* n_states) {
  if (!h || !W || !Sg || !S2g || !Sb || !S2b || !Cgg || !Cgb || !n_states) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  mjhmc_sampler* s = h->s;
  HIPCHK(hipSetDevice(s->ctx->device));
  const size_t D = (size_t)h->D, K = (size_t)h->K;
  std::vector<double> hg(1 + 2 * D), hb(1 + 2 * K);
  HIPCHK(hipMemcpyAsync(hg.data(), h->accg, hg.size() * sizeof(double), hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipMemcpyAsync(hb.data(), h->accb, hb.size() * sizeof(double), hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipMemcpyAsync(Cgg, h->Cgg, D * D * sizeof(double), hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipMemcpyAsync(Cgb, h->Cgb, D * K * sizeof(double), hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  *W = hb[0];   // (the ring's own moment pass: bit for bit the W of an estimator on the same slots)
  std::copy(hg.begin() + 1, hg.begin() + 1 + D, Sg);
  std::copy(hg.begin() + 1 + D, hg.end(), S2g);
  std::copy(hb.begin() + 1, hb.begin() + 1 + K, Sb);
  std::copy(hb.begin() + 1 + K, hb.end(), S2b);
  *n_states = h->n_states;
  return 0;
}

}  // extern "C"
