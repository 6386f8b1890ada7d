// Dwell-weighted marginal histograms from the sample ring, on the device.
//
// Definition (the contract; include/mjhmc_hip.h: mjhmc_histogram_accumulate).  B bins per dimension between lo_d and
// hi_d, inv_d = B / (hi_d - lo_d) computed by the host in float64, one quantum q (a power of two).  For a state element x
// (float64, float32 or bfloat16 in the ring, widened exactly to float64) and its weight w:
//   t = (x - lo_d) * inv_d                 two rounded float64 operations (built with -ffp-contract=off)
//   bin = 0 if !(t >= 0)  (NaN too);  B + 1 if t >= B;  1 + (int)t otherwise
//   u = rint(w / q)                        nearest-even, exact division; an unsigned 64-bit integer
//   count[d][bin] += 1;  mass[d][bin] += u;       uint64 [D][B + 2]
// and once per state W_units += u.  All sums are integers: they do not depend on the order of addition, so the tables
// are bit-identical from run to run and whatever the blocks, shards add exactly, and integer atomics (LDS and global)
// are allowed.  There is no floating-point atomic in this file.  |q mass - sum w| <= 0.5 q count, bin by bin.
// States and weights pair as in mjhmc_estimator_accumulate (estimators.hip): slots x_slot0 + k and dwell slots w_slot0 + k,
// or unit weights.  Rows p >= N and the dwell ring's padding entries are never read.
//
// Three launches per block, one stream:
//   hist_check_kernel   over the n * N weights: a flag for a weight that is not finite or negative, a flag for w / q >=
//                       2^53, and the workgroup's sum of units (clamped at 2^63) as one partial
//   hist_decide_kernel  one workgroup: adds the partials (clamped), raises the third flag when W_units would reach 2^63,
//                       otherwise -- and only when no flag is up -- commits W_units += the block's units
//   hist_kernel         the pass; returns at its top when a flag is up, so a refused block adds nothing
//
// The pass reads the block once with the access shape of the moment pass (ring_rows.hpp: a lane owns 16 bytes of a row):
// a workgroup is cw column lanes x 256 / cw row lanes, rows are strided over the workgroups of a strip and kRowsInFlight
// loads are issued before the first is used.  A workgroup covers a strip of dimensions whose
// private tables -- mass u64 [strip][B + 2], then count u32 [strip][B + 2] -- live in LDS; the strip is the largest power
// of two whose tables fit kLdsBudget (32 KB: four to five workgroups per compute unit), so 32 dimensions at B = 64, 8 at
// B = 256, 2 at B = 1024.  Binning is one ds_add_u32 and, for weighted blocks, one ds_add_u64 per element, neither
// returning a value; unit-weight blocks skip the second and the flush takes mass = count * rint(1 / q).  Lanes of one
// wave instruction that hit the same bin of the same dimension are serialised by the LDS; which lanes share a dimension
// is fixed by the layout (64 / cw row lanes per dimension and wave), how often they share a bin is the data's: a marginal
// spread over B bins with span 8 puts about 40 / B of its mass into its central bin.
// At the end every workgroup adds its non-zero bins to the global tables with global u64 integer atomics.
// A strip narrower than a lane's 16 bytes (bfloat16 at B >= 512, float32 at B = 1024) makes the lanes of neighbouring
// strips load the same 16 bytes and bin their own part of them.
#include "histograms.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/mjhmc_hip.h"
#include "handles.hpp"
#include "ring_rows.hpp"
#include "ring_source.hpp"

namespace {

typedef unsigned long long u64;

constexpr size_t kLdsBudget = 32768;      // bytes of LDS tables per workgroup
constexpr int kCheckMaxGy = 64;           // slots the weight check spreads over workgroups
constexpr u64 kUnitsLimit = 1ull << 63;   // W_units stays below this
constexpr double kTwo53 = 9007199254740992.0;

__device__ inline u64 add_clamped(u64 a, u64 b) {   // a, b <= 2^63
  const u64 s = a + b;
  return (s >= kUnitsLimit || s < a) ? kUnitsLimit : s;
}

// partial[by * gridDim.x + bx] = the workgroup's sum of rint(w * inv_q) over its share of w[k * Npad + p], k < n, p < N
__global__ __launch_bounds__(256) void hist_check_kernel(const double* __restrict__ w, int64_t Npad, int64_t N, int n,
                                                         double inv_q, u64* __restrict__ partial, int* __restrict__ bad) {
  __shared__ u64 sm[256];
  u64 s = 0;
  int flags = 0;
  for (int k = blockIdx.y; k < n; k += gridDim.y) {
    const double* wk = w + (size_t)k * Npad;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < N; p += (int64_t)gridDim.x * 256) {
      const double v = wk[p];
      if (!(v >= 0.0 && finite_f64(v))) {
        flags |= kHistBadNonfinite;
      } else {
        const double r = v * inv_q;   // (= v / q exactly: q is a power of two)
        if (!(r < kTwo53))
          flags |= kHistBadTooLarge;
        else
          s = add_clamped(s, (u64)rint(r));
      }
    }
  }
  if (flags) atomicOr(bad, flags);
  sm[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sm[threadIdx.x] = add_clamped(sm[threadIdx.x], sm[threadIdx.x + o]);
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = sm[0];
}

// block units = extra + sum of n_partial partials (clamped at 2^63); W_units += them unless a flag is up or the sum would
// reach 2^63, which raises kHistBadTotal
__global__ __launch_bounds__(256) void hist_decide_kernel(const u64* __restrict__ partial, int n_partial, u64 extra,
                                                          u64* __restrict__ W_units, int* __restrict__ bad) {
  __shared__ u64 sm[256];
  u64 s = 0;
  for (int i = threadIdx.x; i < n_partial; i += 256) s = add_clamped(s, partial[i]);
  sm[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sm[threadIdx.x] = add_clamped(sm[threadIdx.x], sm[threadIdx.x + o]);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const u64 total = add_clamped(add_clamped(sm[0], extra), *W_units);
    if (total >= kUnitsLimit)
      *bad = *bad | kHistBadTotal;
    else if (!*bad)
      *W_units = total;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void hist_kernel(const T* __restrict__ base, const double* __restrict__ w,
                                                   const double* __restrict__ lo, const double* __restrict__ inv, double inv_q,
                                                   int64_t Npad, int64_t N, int n, int D, int pitch, int B, int strip, int cw,
                                                   int log_cw, u64* __restrict__ gcount, u64* __restrict__ gmass,
                                                   const int* __restrict__ bad) {
  constexpr int VEC = ChunkOf<T>::VEC;
  extern __shared__ u64 hist_lds[];
  if (*bad) return;
  const int nb = B + 2, cells = strip * nb;
  u64* const lmass = hist_lds;
  uint32_t* const lcount = reinterpret_cast<uint32_t*>(hist_lds + cells);
  const int tid = threadIdx.x;
  for (int i = tid; i < cells; i += 256) {
    lmass[i] = 0;
    lcount[i] = 0;
  }
  __syncthreads();
  const int cx = tid & (cw - 1), ry = tid >> log_cw, rw = 256 >> log_cw;
  const int strip0 = blockIdx.y * strip;
  const int col0 = (strip0 / VEC + cx) * VEC;           // the lane's 16 bytes of a row
  const bool active = col0 < pitch;
  // the lane's elements that belong to this strip (all of them unless the strip is narrower than the 16 bytes)
  bool mine[VEC];
  double los[VEC], invs[VEC];
  int cell0[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    const int col = col0 + j;
    mine[j] = active && col >= strip0 && col < strip0 + strip && col < D;
    los[j] = mine[j] ? lo[col] : 0.0;
    invs[j] = mine[j] ? inv[col] : 0.0;
    cell0[j] = (col - strip0) * nb;
  }
  const double Bd = (double)B;
  const int64_t stride = (int64_t)gridDim.x * rw;
  for (int k = 0; k < n; ++k) {
    const T* slot = base + (size_t)k * Npad * pitch + col0;
    const double* wk = w ? w + (size_t)k * Npad : nullptr;
    for (int64_t p0 = (int64_t)blockIdx.x * rw + ry; p0 < N; p0 += stride * kRowsInFlight) {
      uint4 q[kRowsInFlight];
      double wt[kRowsInFlight];
#pragma unroll
      for (int u = 0; u < kRowsInFlight; ++u) {
        const int64_t p = p0 + u * stride;
        wt[u] = 1.0;
        if (p < N && active) {
          q[u] = *reinterpret_cast<const uint4*>(slot + (size_t)p * pitch);
          if (wk) wt[u] = wk[p];
        }
      }
#pragma unroll
      for (int u = 0; u < kRowsInFlight; ++u) {
        const int64_t p = p0 + u * stride;
        if (p < N && active) {
          double x[VEC];
          ChunkOf<T>::widen(q[u], x);
          const u64 units = wk ? (u64)rint(wt[u] * inv_q) : 0;   // (the check passed: 0 <= w / q < 2^53)
#pragma unroll
          for (int j = 0; j < VEC; ++j) {
            if (mine[j]) {
              const double d = x[j] - los[j];
              const double t = d * invs[j];
              const int bin = !(t >= 0.0) ? 0 : (t >= Bd ? B + 1 : 1 + (int)t);
              atomicAdd(&lcount[cell0[j] + bin], 1u);
              if (wk) atomicAdd(&lmass[cell0[j] + bin], units);
            }
          }
        }
      }
    }
  }
  __syncthreads();
  const u64 unit = (u64)rint(inv_q);   // a unit weight's units
  for (int i = tid; i < cells; i += 256) {
    const uint32_t c = lcount[i];
    if (c) {
      const int dl = i / nb, b = i - dl * nb;
      const size_t g = (size_t)(strip0 + dl) * nb + b;   // (strip0 + dl < D: only such cells were touched)
      atomicAdd(&gcount[g], (u64)c);
      atomicAdd(&gmass[g], w ? lmass[i] : (u64)c * unit);
    }
  }
}

int pow2floor_i(int64_t v) {
  int p = 1;
  while ((int64_t)p * 2 <= v) p <<= 1;
  return p;
}

}  // namespace

HistogramPlan histogram_plan(const RingView& r, int bins) {
  HistogramPlan pl;
  pl.vec = r.dtype == MJHMC_F64 ? 2 : (r.dtype == MJHMC_F32 ? 4 : 8);
  pl.bins = bins;
  const size_t per_dim = (size_t)(bins + 2) * (sizeof(u64) + sizeof(uint32_t));
  pl.strip = pow2floor_i(std::max<int64_t>(1, (int64_t)(kLdsBudget / per_dim)));   // (B = 1024: 12 312 bytes per dimension, 2)
  pl.strip = std::min(pl.strip, std::min(256 * pl.vec, pow2ceil(r.D)));
  pl.cw = std::max(1, pl.strip / pl.vec);
  pl.log_cw = ilog2(pl.cw);
  pl.gy = (r.D + pl.strip - 1) / pl.strip;
  const int rw = 256 / pl.cw;
  // about four workgroups per compute unit, each with at least kRowsInFlight rows per row lane
  const int64_t want = std::max<int64_t>(1, 1024 / pl.gy);
  const int64_t have = (r.N + (int64_t)rw * kRowsInFlight - 1) / ((int64_t)rw * kRowsInFlight);
  pl.gx = (int)std::max<int64_t>(1, std::min(want, have));
  histogram_check_grid(r.N, &pl.check_gx, &pl.check_gy);
  pl.lds_bytes = (size_t)pl.strip * per_dim;
  return pl;
}

void histogram_check_grid(int64_t N, int* check_gx, int* check_gy) {
  *check_gx = (int)std::max<int64_t>(1, std::min<int64_t>(256, (N + 255) / 256));
  *check_gy = kCheckMaxGy;
}

void histogram_weight_pass(hipStream_t st, const double* w, int64_t Npad, int64_t N, int n, double inv_q, int check_gx,
                           int check_gy, u64* partial, u64* W_units, int* bad) {
  int n_partial = 0;
  u64 extra = 0;
  if (w) {
    const int gy = std::min(n, check_gy);
    n_partial = check_gx * gy;
    hipLaunchKernelGGL(hist_check_kernel, dim3(check_gx, gy), dim3(256), 0, st, w, Npad, N, n, inv_q, partial, bad);
  } else {
    // unit weights: n * N states of rint(1 / q) units each (the caller refused 1 / q >= 2^53)
    const u64 unit = (u64)rint(inv_q), states = (u64)n * (u64)N;
    extra = (unit && states > (kUnitsLimit - 1) / unit) ? kUnitsLimit : unit * states;
  }
  hipLaunchKernelGGL(hist_decide_kernel, dim3(1), dim3(256), 0, st, partial, n_partial, extra, W_units, bad);
}

int histogram_refusal(int bad, int w_slot0, int n) {
  const std::string where = "dwell slots [" + std::to_string(w_slot0) + ", " + std::to_string(w_slot0 + n) + ")";
  if (bad & kHistBadNonfinite)
    return mjhmc_fail(MJHMC_ERR_NONFINITE, "a dwelling time in " + where +
                                               " is not finite or is negative (a state whose total jump rate is zero "
                                               "leaves an infinite one): nothing of this block was added");
  if (bad & kHistBadTooLarge)
    return mjhmc_fail(MJHMC_ERR_INVALID, "a weight in " + where +
                                             " is 2^53 quanta or more (w / quantum must stay below 2^53: take a larger "
                                             "quantum): nothing of this block was added");
  return mjhmc_fail(MJHMC_ERR_INVALID, "this block would take the total weight to 2^63 quanta or beyond (take a larger "
                                       "quantum): nothing of this block was added");
}

int histogram_accumulate(hipStream_t st, const RingView& r, int n, const double* w, const double* lo, const double* inv,
                         double inv_q, const HistogramPlan& pl, u64* partial, u64* count, u64* mass, u64* W_units, int* bad,
                         std::string& err) {
  if (r.N >= (1ll << 32)) {
    err = "the histogram pass counts a workgroup's states per bin in 32 bits: fewer than 2^32 particles";
    return MJHMC_ERR_UNSUPPORTED;
  }
  histogram_weight_pass(st, w, r.Npad, r.N, n, inv_q, pl.check_gx, pl.check_gy, partial, W_units, bad);
  // a workgroup's count of a bin is 32 bits wide: at most 2^32 - 1 states per launch of the pass
  const int per_launch = (int)std::max<int64_t>(1, std::min<int64_t>(n, 0xFFFFFFFFll / r.N));
  const dim3 grid(pl.gx, pl.gy), block(256);
  const size_t slot_bytes = (size_t)r.Npad * r.pitch * (16 / pl.vec);
  for (int k0 = 0; k0 < n; k0 += per_launch) {
    const int nk = std::min(per_launch, n - k0);
    const char* base = (const char*)r.base + (size_t)k0 * slot_bytes;
    const double* wk = w ? w + (size_t)k0 * r.Npad : nullptr;
    dispatch_dtype(r.dtype, [&](auto tag) {
      typedef typename decltype(tag)::type T;
      hipLaunchKernelGGL(hist_kernel<T>, grid, block, pl.lds_bytes, st, (const T*)base, wk, lo, inv, inv_q, r.Npad, r.N, nk, r.D,
                         r.pitch, pl.bins, pl.strip, pl.cw, pl.log_cw, count, mass, bad);
    });
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    err = std::string("histogram pass: ") + hipGetErrorString(e);
    return MJHMC_ERR_HIP;
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// The accumulator handle of the C ABI (include/mjhmc_hip.h: mjhmc_histogram_*)
// ---------------------------------------------------------------------------------------------------------------------
struct mjhmc_histogram : RingAccumulator {
  using RingAccumulator::RingAccumulator;
  int D = 0;                  // dimensions of a state of that ring
  HistogramPlan plan;
  double inv_q = 1.0;
  double* range = nullptr;    // [2][D]: lo, inv
  u64* tables = nullptr;      // count [D][B + 2], mass [D][B + 2], W_units
  u64* partial = nullptr;     // the weight check's per-workgroup units
  ~mjhmc_histogram() override { free_device({range, tables, partial}); }
  size_t cells() const { return (size_t)D * (plan.bins + 2); }
  u64* count() const { return tables; }
  u64* mass() const { return tables + cells(); }
  u64* W_units() const { return tables + 2 * cells(); }
  size_t table_bytes() const { return (2 * cells() + 1) * sizeof(u64); }
};

// have: the sampler or the functionals handle was given (s itself is looked at only after the argument checks that need none)
static int histogram_create_on_source(bool have, mjhmc_sampler* s, const mjhmc_functionals* fn, int n_bins, const double* lo,
                                      const double* hi, double quantum, mjhmc_histogram** out) {
  if (n_bins < 1 || n_bins > kHistogramMaxBins)
    return mjhmc_fail(MJHMC_ERR_INVALID, "n_bins must be in [1, " + std::to_string(kHistogramMaxBins) + "], got " +
                                             std::to_string(n_bins));
  int exp2 = 0;
  if (!(quantum > 0.0) || !std::isfinite(quantum) || std::frexp(quantum, &exp2) != 0.5)
    return mjhmc_fail(MJHMC_ERR_INVALID, "the quantum must be a positive power of two");
  const double inv_q = 1.0 / quantum;   // exact, unless it leaves the normal range
  if (!std::isnormal(inv_q) || !std::isnormal(quantum))
    return mjhmc_fail(MJHMC_ERR_INVALID, "the quantum must be a positive power of two whose inverse is a normal float64");
  if (!have || !lo || !hi || !out) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  if (fn) s = functionals_sampler(fn);
  const RingSource src = ring_source(s, fn);
  const int D = src.D;
  std::vector<double> range(2 * (size_t)D);
  for (int d = 0; d < D; ++d) {
    if (!std::isfinite(lo[d]) || !std::isfinite(hi[d]))
      return mjhmc_fail(MJHMC_ERR_INVALID, "the range of dimension " + std::to_string(d) + " is not finite");
    if (!(lo[d] < hi[d])) return mjhmc_fail(MJHMC_ERR_INVALID, "dimension " + std::to_string(d) + ": lo must be below hi");
    const double inv = (double)n_bins / (hi[d] - lo[d]);
    if (!std::isfinite(inv) || !(inv > 0.0))
      return mjhmc_fail(MJHMC_ERR_INVALID, "dimension " + std::to_string(d) + ": n_bins / (hi - lo) is not a finite positive float64");
    range[d] = lo[d];
    range[(size_t)D + d] = inv;
  }
  if (!src.base) return acc_no_ring(fn);
  // the pass addresses a row in 16-byte chunks of the state's own type: rows must be whole chunks of it
  const int vec = src.dtype == MJHMC_F64 ? 2 : (src.dtype == MJHMC_F32 ? 4 : 8);
  if (src.esize * vec != 16 || src.pitch % vec != 0)
    return mjhmc_fail(MJHMC_ERR_UNSUPPORTED, "the sampler's rows are not whole 16-byte chunks of its state type");
  HIPCHK(hipSetDevice(s->ctx->device));
  mjhmc_histogram* h = new mjhmc_histogram("histogram", "histogram", s, fn, src);
  h->D = D;
  h->inv_q = inv_q;
  h->plan = histogram_plan(ring_source_view(s, src, 0), n_bins);
  const size_t partial_bytes = (size_t)h->plan.check_gx * h->plan.check_gy * sizeof(u64);
  hipError_t e = hipMalloc((void**)&h->range, range.size() * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&h->tables, h->table_bytes());
  if (e == hipSuccess) e = hipMalloc((void**)&h->partial, partial_bytes);
  if (e == hipSuccess) e = hipMalloc((void**)&h->bad, sizeof(int));
  if (e == hipSuccess) e = hipMemcpyAsync(h->range, range.data(), range.size() * sizeof(double), hipMemcpyHostToDevice, s->stream);
  if (e == hipSuccess) e = hipMemsetAsync(h->tables, 0, h->table_bytes(), s->stream);
  if (e == hipSuccess) e = hipMemsetAsync(h->partial, 0, partial_bytes, s->stream);
  if (e == hipSuccess) e = hipMemsetAsync(h->bad, 0, sizeof(int), s->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(s->stream);   // (range is this call's)
  if (e != hipSuccess) {
    delete h;
    (void)hipGetLastError();
    return mjhmc_fail(MJHMC_ERR_HIP, std::string("histogram buffers: ") + hipGetErrorString(e));
  }
  return acc_created(h, out);
}

extern "C" {

int mjhmc_histogram_create(mjhmc_sampler* s, int n_bins, const double* lo, const double* hi, double quantum,
                           mjhmc_histogram** out) {
  return histogram_create_on_source(s != nullptr, s, nullptr, n_bins, lo, hi, quantum, out);
}

int mjhmc_histogram_create_on(mjhmc_functionals* f, int n_bins, const double* lo, const double* hi, double quantum,
                              mjhmc_histogram** out) {
  return histogram_create_on_source(f != nullptr, nullptr, f, n_bins, lo, hi, quantum, out);
}

int mjhmc_histogram_destroy(mjhmc_histogram* h) { return acc_destroy(h); }

int mjhmc_histogram_reset(mjhmc_histogram* h) {
  if (!h) return mjhmc_fail(MJHMC_ERR_INVALID, "histogram is NULL");
  mjhmc_sampler* s = h->s;
  HIPCHK(hipSetDevice(s->ctx->device));
  HIPCHK(hipMemsetAsync(h->tables, 0, h->table_bytes(), s->stream));
  HIPCHK(hipMemsetAsync(h->bad, 0, sizeof(int), s->stream));
  h->n_states = 0;
  return 0;
}

int mjhmc_histogram_accumulate(mjhmc_histogram* h, int x_slot0, int w_slot0, int n) {
  if (!h) return mjhmc_fail(MJHMC_ERR_INVALID, "histogram is NULL");
  mjhmc_sampler* s = h->s;
  RingSource src;
  TRY(acc_begin(h, x_slot0, w_slot0, n, &src));
  if (w_slot0 < 0 && !(h->inv_q < kTwo53))
    return mjhmc_fail(MJHMC_ERR_INVALID, "a unit weight is 2^53 quanta or more: w / quantum must stay below 2^53");
  HIPCHK(hipSetDevice(s->ctx->device));
  const double* w = acc_weights(h, w_slot0);
  std::string err;
  const int rc = histogram_accumulate(s->stream, ring_source_view(s, src, x_slot0), n, w, h->range, h->range + h->D, h->inv_q, h->plan,
                                      h->partial, h->count(), h->mass(), h->W_units(), h->bad, err);
  if (rc) return mjhmc_fail(rc, err);
  return acc_end(h, n, [&](int bad) { return histogram_refusal(bad, w_slot0, n); });
}

int mjhmc_histogram_read(mjhmc_histogram* h, uint64_t* count, uint64_t* mass, uint64_t* W_units, int64_t* n_states) {
  if (!h || !count || !mass || !W_units || !n_states) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  mjhmc_sampler* s = h->s;
  HIPCHK(hipSetDevice(s->ctx->device));
  const size_t bytes = h->cells() * sizeof(u64);
  u64 W = 0;
  HIPCHK(hipMemcpyAsync(count, h->count(), bytes, hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipMemcpyAsync(mass, h->mass(), bytes, hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipMemcpyAsync(&W, h->W_units(), sizeof(u64), hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  *W_units = W;
  *n_states = h->n_states;
  return 0;
}

#ifdef MJHMC_TEST_HOOKS
// test build only: every byte of the padding rows (N <= p < Npad) of ring slot `slot` and of its dwell-ring padding
// entries set to `byte` -- garbage nobody may read (0xFF: NaN in every state type and as a weight)
int mjhmc_test_ring_fill_padding(mjhmc_sampler* s, int slot, int byte) {
  if (!s || slot < 0 || slot >= s->ring_slots) return mjhmc_fail(MJHMC_ERR_INVALID, "bad argument");
  HIPCHK(hipSetDevice(s->ctx->device));
  const size_t pad = (size_t)(s->Npad - s->N);
  if (pad) {
    HIPCHK(hipMemsetAsync((char*)s->ring + (size_t)slot * mat_bytes(s) + (size_t)s->N * row_bytes(s), byte, pad * row_bytes(s),
                          s->stream));
    HIPCHK(hipMemsetAsync(s->dwell_ring + (size_t)slot * s->Npad + s->N, byte, pad * sizeof(double), s->stream));
  }
  HIPCHK(hipStreamSynchronize(s->stream));
  return 0;
}
#endif

}  // extern "C"
