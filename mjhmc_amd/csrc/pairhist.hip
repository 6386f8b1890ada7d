// Dwell-weighted joint histograms of pairs of state dimensions from the sample ring, on the device.
//
// Definition (the contract; include/mjhmc_hip.h: mjhmc_pairhist_accumulate) -- the 1-D contract of histograms.hip, taken
// per axis.  P pairs (i_p, j_p), B bins per axis between lo[p][a] and hi[p][a] (a = 0: the i axis, a = 1: the j axis),
// inv[p][a] = B / (hi - lo) computed by the host in float64, one quantum q (a power of two).  For a state (float64,
// float32 or bfloat16 in the ring, widened exactly to float64) and its weight w:
//   t_a = (x_a - lo[p][a]) * inv[p][a]      two rounded float64 operations (built with -ffp-contract=off)
//   b_a = 0 if !(t_a >= 0)  (NaN too);  B + 1 if t_a >= B;  1 + (int)t_a otherwise
//   u = rint(w / q)                         nearest-even, exact division; an unsigned 64-bit integer
//   count[p][b_1][b_0] += 1;  mass[p][b_1][b_0] += u        uint64 [P][B + 2][B + 2], the i axis fastest
// and once per state W_units += u.  All sums are integers: the tables are bit-identical from run to run and whatever the
// blocks, shards add exactly, and integer atomics (LDS and global) are allowed.  There is no floating-point atomic in
// this file.  Rows p >= N and the dwell ring's padding entries are never read.
//
// The weight check and the decision are those of the 1-D pass (histograms.hpp: histogram_weight_pass), then one launch of
// the pair pass, which returns at its top when a flag is up: a refused block adds nothing.
//
// The pass: a lane owns a row (a particle) and walks the block's slots, kStatesInFlight of them at a time -- their
// weights once per state, then per pair of the workgroup's group the two elements of each of those states by their own
// type, all issued before the first is used.  These are scattered element loads: a pair touches at most two cache
// lines of a row, so the pass never fetches more lines than a full pass over the ring would, and of a 4 KB row a small
// fraction.  Two forms share the binning code (pairhist_cell), chosen by (B, P) alone (pairhist_plan):
//   LDS form     while a pair's tables fit kPairhistLdsBudget (B <= 71): a workgroup owns a group of pairs, each with
//                private tables in LDS -- mass u64 [group][B + 2][B + 2], then count u32 [group][B + 2][B + 2].  Binning is
//                one ds_add_u32 and, for weighted blocks, one ds_add_u64, neither returning a value; unit-weight blocks
//                skip the second and the flush takes mass = count * rint(1 / q).  At the end the workgroup adds its
//                non-zero cells to the global tables with global u64 atomics.  The 32-bit count limits a launch to
//                2^32 - 1 states: longer blocks are split into launches, as in the 1-D pass.
//   global form  above that B: one pair per workgroup row, every state two global u64 atomics (count, mass) into the
//                pair's table (16 900 cells at B = 128).
// Lanes of one wave instruction that hit the same cell are serialised by the LDS (or by the memory side): how often
// is the data's -- a joint spread over B x B cells collides far less than a marginal over B.
#include "pairhist.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/mjhmc_hip.h"
#include "handles.hpp"
#include "histograms.hpp"
#include "ring_rows.hpp"
#include "ring_source.hpp"

namespace {

typedef unsigned long long u64;

constexpr int kStatesInFlight = 4;        // states of a row whose loads a lane issues before it uses the first
constexpr double kTwo53 = 9007199254740992.0;

__device__ inline int pairhist_bin(double x, double lo, double inv, int B, double Bd) {
  const double d = x - lo;
  const double t = d * inv;
  return !(t >= 0.0) ? 0 : (t >= Bd ? B + 1 : 1 + (int)t);
}

// the cell of a state in a pair's table, the i axis fastest
__device__ inline int pairhist_cell(double xi, double xj, double lo0, double inv0, double lo1, double inv1, int B, double Bd) {
  return pairhist_bin(xj, lo1, inv1, B, Bd) * (B + 2) + pairhist_bin(xi, lo0, inv0, B, Bd);
}

template <typename S, bool LDS>
__global__ __launch_bounds__(256) void pairhist_kernel(const S* __restrict__ base, const double* __restrict__ w,
                                                       const int32_t* __restrict__ pairs, const double* __restrict__ range,
                                                       double inv_q, int64_t Npad, int64_t N, int n, int pitch, int B, int P,
                                                       int group, u64* __restrict__ gcount, u64* __restrict__ gmass,
                                                       const int* __restrict__ bad) {
  extern __shared__ u64 pairhist_lds[];
  if (*bad) return;
  const int nb = B + 2, cells = nb * nb;
  const int g0 = blockIdx.y * group, ng = min(group, P - g0);   // this workgroup's pairs g0 .. g0 + ng - 1
  u64* const lmass = pairhist_lds;
  uint32_t* const lcount = reinterpret_cast<uint32_t*>(pairhist_lds + (size_t)group * cells);
  const int tid = threadIdx.x;
  if (LDS) {
    for (int i = tid; i < ng * cells; i += 256) {
      lmass[i] = 0;
      lcount[i] = 0;
    }
    __syncthreads();
  }
  const double Bd = (double)B;
  const u64 unit = (u64)rint(inv_q);   // a unit weight's units
  const size_t slot_stride = (size_t)Npad * pitch;
  for (int64_t p = (int64_t)blockIdx.x * 256 + tid; p < N; p += (int64_t)gridDim.x * 256) {
    const S* row = base + (size_t)p * pitch;
    for (int k0 = 0; k0 < n; k0 += kStatesInFlight) {
      // (a short last batch loads slot n - 1 again in its spare places, so that no load is conditional, and bins it once)
      double wt[kStatesInFlight];
#pragma unroll
      for (int u = 0; u < kStatesInFlight; ++u) wt[u] = w ? w[(size_t)min(k0 + u, n - 1) * Npad + p] : 1.0;
      for (int g = 0; g < ng; ++g) {
        const int i = pairs[2 * (g0 + g)], j = pairs[2 * (g0 + g) + 1];
        const double* rg = range + 4 * (size_t)(g0 + g);
        const double lo0 = rg[0], inv0 = rg[1], lo1 = rg[2], inv1 = rg[3];
        S xi[kStatesInFlight], xj[kStatesInFlight];
#pragma unroll
        for (int u = 0; u < kStatesInFlight; ++u) {
          const S* x = row + (size_t)min(k0 + u, n - 1) * slot_stride;
          xi[u] = x[i];
          xj[u] = x[j];
        }
#pragma unroll
        for (int u = 0; u < kStatesInFlight; ++u) {
          if (k0 + u < n) {
            const int c = pairhist_cell(elem_to_f64(xi[u]), elem_to_f64(xj[u]), lo0, inv0, lo1, inv1, B, Bd);
            const u64 units = w ? (u64)rint(wt[u] * inv_q) : unit;   // (the check passed: 0 <= w / q < 2^53)
            if (LDS) {
              atomicAdd(&lcount[g * cells + c], 1u);
              if (w) atomicAdd(&lmass[g * cells + c], units);
            } else {
              const size_t at = (size_t)(g0 + g) * cells + c;
              atomicAdd(&gcount[at], (u64)1);
              atomicAdd(&gmass[at], units);
            }
          }
        }
      }
    }
  }
  if (LDS) {
    __syncthreads();
    for (int i = tid; i < ng * cells; i += 256) {
      const uint32_t c = lcount[i];
      if (c) {
        const size_t at = (size_t)g0 * cells + i;   // (pair g0 + i / cells, cell i % cells: the tables are contiguous)
        atomicAdd(&gcount[at], (u64)c);
        atomicAdd(&gmass[at], w ? lmass[i] : (u64)c * unit);
      }
    }
  }
}

}  // namespace

PairhistPlan pairhist_plan(int64_t N, int bins, int n_pairs) {
  PairhistPlan pl;
  pl.bins = bins;
  pl.n_pairs = n_pairs;
  pl.cells = (bins + 2) * (bins + 2);
  const size_t per_pair = (size_t)pl.cells * (sizeof(u64) + sizeof(uint32_t));
  const int fit = (int)(kPairhistLdsBudget / per_pair);
  pl.lds = fit >= 1;
  pl.group = pl.lds ? std::min(n_pairs, std::min(kPairhistMaxGroup, fit)) : 1;
  pl.gy = (n_pairs + pl.group - 1) / pl.group;
  pl.lds_bytes = pl.lds ? (size_t)pl.group * per_pair : 0;
  // a lane per row; about four workgroups per compute unit when there are rows enough
  const int64_t want = std::max<int64_t>(1, 1024 / pl.gy);
  const int64_t have = (N + 255) / 256;
  pl.gx = (int)std::max<int64_t>(1, std::min(want, have));
  histogram_check_grid(N, &pl.check_gx, &pl.check_gy);
  return pl;
}

int pairhist_accumulate(hipStream_t st, const RingView& r, int n, const double* w, const int32_t* pairs, const double* range,
                        double inv_q, const PairhistPlan& pl, u64* partial, u64* count, u64* mass, u64* W_units, int* bad,
                        std::string& err) {
  if (r.N >= (1ll << 32)) {
    err = "the pair-histogram pass counts a workgroup's states per cell in 32 bits: fewer than 2^32 particles";
    return MJHMC_ERR_UNSUPPORTED;
  }
  histogram_weight_pass(st, w, r.Npad, r.N, n, inv_q, pl.check_gx, pl.check_gy, partial, W_units, bad);
  // a workgroup's count of a cell is 32 bits wide: at most 2^32 - 1 states per launch of the pass
  const int per_launch = (int)std::max<int64_t>(1, std::min<int64_t>(n, 0xFFFFFFFFll / r.N));
  const dim3 grid(pl.gx, pl.gy), block(256);
  const size_t esize = r.dtype == MJHMC_F64 ? 8 : (r.dtype == MJHMC_F32 ? 4 : 2);
  const size_t slot_bytes = (size_t)r.Npad * r.pitch * esize;
  for (int k0 = 0; k0 < n; k0 += per_launch) {
    const int nk = std::min(per_launch, n - k0);
    const char* base = (const char*)r.base + (size_t)k0 * slot_bytes;
    const double* wk = w ? w + (size_t)k0 * r.Npad : nullptr;
    dispatch_dtype(r.dtype, [&](auto tag) {
      typedef typename ElemBits<typename decltype(tag)::type>::type S;   // (bfloat16 is loaded as its 16 bits)
      const auto kernel = pl.lds ? pairhist_kernel<S, true> : pairhist_kernel<S, false>;
      hipLaunchKernelGGL(kernel, grid, block, pl.lds_bytes, st, (const S*)base, wk, pairs, range, inv_q, r.Npad, r.N, nk,
                         r.pitch, pl.bins, pl.n_pairs, pl.group, count, mass, bad);
    });
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    err = std::string("pair-histogram pass: ") + hipGetErrorString(e);
    return MJHMC_ERR_HIP;
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// The accumulator handle of the C ABI (include/mjhmc_hip.h: mjhmc_pairhist_*)
// ---------------------------------------------------------------------------------------------------------------------
struct mjhmc_pairhist : RingAccumulator {   // (ring_gen: the pairs were checked against that ring's dimensions)
  using RingAccumulator::RingAccumulator;
  PairhistPlan plan;
  double inv_q = 1.0;
  int32_t* pairs = nullptr;   // [P][2]
  double* range = nullptr;    // [P][4]: lo_i, inv_i, lo_j, inv_j
  u64* tables = nullptr;      // count [P][B + 2][B + 2], mass [P][B + 2][B + 2], W_units
  u64* partial = nullptr;     // the weight check's per-workgroup units
  ~mjhmc_pairhist() override { free_device({pairs, range, tables, partial}); }
  size_t cells() const { return (size_t)plan.n_pairs * plan.cells; }
  u64* count() const { return tables; }
  u64* mass() const { return tables + cells(); }
  u64* W_units() const { return tables + 2 * cells(); }
  size_t table_bytes() const { return (2 * cells() + 1) * sizeof(u64); }
};

// have: the sampler or the functionals handle was given (s itself is looked at only after the argument checks that need none)
static int pairhist_create_on_source(bool have, mjhmc_sampler* s, const mjhmc_functionals* fn, int n_pairs, const int32_t* pairs,
                                     int n_bins, const double* lo, const double* hi, double quantum, mjhmc_pairhist** out) {
  if (n_pairs < 1 || n_pairs > kPairhistMaxPairs)
    return mjhmc_fail(MJHMC_ERR_INVALID, "n_pairs must be in [1, " + std::to_string(kPairhistMaxPairs) + "], got " +
                                             std::to_string(n_pairs));
  if (n_bins < 1 || n_bins > kPairhistMaxBins)
    return mjhmc_fail(MJHMC_ERR_INVALID, "n_bins must be in [1, " + std::to_string(kPairhistMaxBins) + "] per axis, got " +
                                             std::to_string(n_bins));
  int exp2 = 0;
  if (!(quantum > 0.0) || !std::isfinite(quantum) || std::frexp(quantum, &exp2) != 0.5)
    return mjhmc_fail(MJHMC_ERR_INVALID, "the quantum must be a positive power of two");
  const double inv_q = 1.0 / quantum;   // exact, unless it leaves the normal range
  if (!std::isnormal(inv_q) || !std::isnormal(quantum))
    return mjhmc_fail(MJHMC_ERR_INVALID, "the quantum must be a positive power of two whose inverse is a normal float64");
  if (!have || !pairs || !lo || !hi || !out) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  if (fn) s = functionals_sampler(fn);
  const RingSource src = ring_source(s, fn);
  const int D = src.D;
  std::vector<double> range(4 * (size_t)n_pairs);
  for (int p = 0; p < n_pairs; ++p) {
    for (int a = 0; a < 2; ++a) {
      const std::string where = "pair " + std::to_string(p) + ", axis " + std::to_string(a);
      const int d = pairs[2 * p + a];
      if (d < 0 || d >= D)
        return mjhmc_fail(MJHMC_ERR_INVALID, where + ": dimension index " + std::to_string(d) + " is outside [0, " +
                                                 std::to_string(D) + ")");
      const double l = lo[2 * p + a], h = hi[2 * p + a];
      if (!std::isfinite(l) || !std::isfinite(h)) return mjhmc_fail(MJHMC_ERR_INVALID, "the range of " + where + " is not finite");
      if (!(l < h)) return mjhmc_fail(MJHMC_ERR_INVALID, where + ": lo must be below hi");
      const double inv = (double)n_bins / (h - l);
      if (!std::isfinite(inv) || !(inv > 0.0))
        return mjhmc_fail(MJHMC_ERR_INVALID, where + ": n_bins / (hi - lo) is not a finite positive float64");
      range[4 * (size_t)p + 2 * a] = l;
      range[4 * (size_t)p + 2 * a + 1] = inv;
    }
  }
  if (!src.base) return acc_no_ring(fn);
  // the pass loads single elements of the state's own type
  if (src.esize != (src.dtype == MJHMC_F64 ? 8 : (src.dtype == MJHMC_F32 ? 4 : 2)) || src.pitch < D)
    return mjhmc_fail(MJHMC_ERR_UNSUPPORTED, "the ring's rows do not store elements of its state type");
  if (s->N >= (1ll << 32))
    return mjhmc_fail(MJHMC_ERR_UNSUPPORTED, "the pair-histogram pass counts a workgroup's states per cell in 32 bits: fewer than 2^32 particles");
  HIPCHK(hipSetDevice(s->ctx->device));
  mjhmc_pairhist* h = new mjhmc_pairhist("pairhist", "pair histogram", s, fn, src);
  h->inv_q = inv_q;
  h->plan = pairhist_plan(s->N, n_bins, n_pairs);
  const size_t partial_bytes = (size_t)h->plan.check_gx * h->plan.check_gy * sizeof(u64);
  const size_t pair_bytes = 2 * (size_t)n_pairs * sizeof(int32_t);
  hipError_t e = hipMalloc((void**)&h->pairs, pair_bytes);
  if (e == hipSuccess) e = hipMalloc((void**)&h->range, range.size() * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&h->tables, h->table_bytes());
  if (e == hipSuccess) e = hipMalloc((void**)&h->partial, partial_bytes);
  if (e == hipSuccess) e = hipMalloc((void**)&h->bad, sizeof(int));
  if (e == hipSuccess) e = hipMemcpyAsync(h->pairs, pairs, pair_bytes, hipMemcpyHostToDevice, s->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(h->range, range.data(), range.size() * sizeof(double), hipMemcpyHostToDevice, s->stream);
  if (e == hipSuccess) e = hipMemsetAsync(h->tables, 0, h->table_bytes(), s->stream);
  if (e == hipSuccess) e = hipMemsetAsync(h->partial, 0, partial_bytes, s->stream);
  if (e == hipSuccess) e = hipMemsetAsync(h->bad, 0, sizeof(int), s->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(s->stream);   // (pairs and range are this call's)
  if (e != hipSuccess) {
    delete h;
    (void)hipGetLastError();
    return mjhmc_fail(MJHMC_ERR_HIP, std::string("pair-histogram buffers: ") + hipGetErrorString(e));
  }
  return acc_created(h, out);
}

extern "C" {

int mjhmc_pairhist_create(mjhmc_sampler* s, int n_pairs, const int32_t* pairs, int n_bins, const double* lo, const double* hi,
                          double quantum, mjhmc_pairhist** out) {
  return pairhist_create_on_source(s != nullptr, s, nullptr, n_pairs, pairs, n_bins, lo, hi, quantum, out);
}

int mjhmc_pairhist_create_on(mjhmc_functionals* f, int n_pairs, const int32_t* pairs, int n_bins, const double* lo,
                             const double* hi, double quantum, mjhmc_pairhist** out) {
  return pairhist_create_on_source(f != nullptr, nullptr, f, n_pairs, pairs, n_bins, lo, hi, quantum, out);
}

int mjhmc_pairhist_destroy(mjhmc_pairhist* h) { return acc_destroy(h); }

int mjhmc_pairhist_reset(mjhmc_pairhist* h) {
  if (!h) return mjhmc_fail(MJHMC_ERR_INVALID, "pair histogram is NULL");
  mjhmc_sampler* s = h->s;
  HIPCHK(hipSetDevice(s->ctx->device));
  HIPCHK(hipMemsetAsync(h->tables, 0, h->table_bytes(), s->stream));
  HIPCHK(hipMemsetAsync(h->bad, 0, sizeof(int), s->stream));
  h->n_states = 0;
  return 0;
}

int mjhmc_pairhist_accumulate(mjhmc_pairhist* h, int x_slot0, int w_slot0, int n) {
  if (!h) return mjhmc_fail(MJHMC_ERR_INVALID, "pair histogram is NULL");
  mjhmc_sampler* s = h->s;
  RingSource src;
  TRY(acc_begin(h, x_slot0, w_slot0, n, &src));
  if (w_slot0 < 0 && !(h->inv_q < kTwo53))
    return mjhmc_fail(MJHMC_ERR_INVALID, "a unit weight is 2^53 quanta or more: w / quantum must stay below 2^53");
  HIPCHK(hipSetDevice(s->ctx->device));
  const double* w = acc_weights(h, w_slot0);
  std::string err;
  const int rc = pairhist_accumulate(s->stream, ring_source_view(s, src, x_slot0), n, w, h->pairs, h->range, h->inv_q, h->plan,
                                     h->partial, h->count(), h->mass(), h->W_units(), h->bad, err);
  if (rc) return mjhmc_fail(rc, err);
  return acc_end(h, n, [&](int bad) { return histogram_refusal(bad, w_slot0, n); });
}

int mjhmc_pairhist_read(mjhmc_pairhist* h, uint64_t* count, uint64_t* mass, uint64_t* W_units, int64_t* n_states) {
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

}  // extern "C"
