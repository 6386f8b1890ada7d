// Per-chain convergence statistics from the sample ring, on the device: the sums behind R-hat (plain and split) and the
// multi-chain effective sample size.
//
// The pooled estimator (estimators.hip) adds over particles first; what it cannot say is whether the chains agree with
// each other.  Here every particle p < N (= chain) keeps its own sums, per part h (part = which half of the run):
//   a0[h][p] = sum_k w        a1[h][p][d] = sum_k w (x_d - c_d)        a2[h][p][d] = sum_k w (x_d - c_d)^2
// for states x[k][p][:] of ring slots x_slot0 + k, weights w[k][p] of dwell slots w_slot0 + k (or 1) and a shift c: the
// conventions, and the slot / dwell pairing, of mjhmc_estimator_accumulate.  a1 and a2 have the ring's own row layout
// ([Npad][pitch] float64), so one index serves the state and both accumulators.
//
// Chain pass: one launch per accumulate, HBM-bound.  A slot is a contiguous [Npad][pitch] matrix and a lane owns 16 bytes
// of it (ring_rows.hpp; 2 / 4 / 8 elements of one chain's row): lane g of the launch takes bytes [16 g, 16 g + 16) of
// every slot of the block, so a wave instruction reads 1 KB of consecutive memory.  The lane reads the stored sums of its elements into
// registers, walks the block's slots for them (kSlotsInFlight loads issued before the first is used) and writes the
// sums back once.  No cross-lane reduction, no atomics, no LDS.  The operation order per element is part of the contract:
//   t = x - c;  u = w * t;  a1 = a1 + u;  a2 = a2 + u * t;     k ascending, from the stored a1, a2;  a0 = a0 + w
// (built with -ffp-contract=off: five roundings, no fused multiply-add).  The sums are therefore bit-identical to that
// sequence of float64 operations on the host and do not depend on how a run is cut into blocks.
// HBM bytes of a call: n slots + n dwell vectors read, the part's a0, a1, a2 read and written once.
// Rows p >= N are never read and their accumulators are never written (zero from create on, and no fold reads them).
//
// Non-finite weights: a check over the n * N weights of the block (the dwell ring's padding entries p >= N are never
// written by anyone and are not looked at) runs first on the same stream and raises a device flag; the chain pass reads
// the flag at its top and writes nothing when it is set.
//
// Fold: per chain m = a1 / a0, v = a2 / a0 - m * m, and the sums over p < N of a0, m, m^2 and v: per-workgroup partials
// in a scratch buffer, then a second small kernel that adds them in index order.  The order is a function of the ring's
// shape alone (ChainFoldPlan), no floating-point atomics: bit-identical from run to run on one device.
#include "chainstats.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../include/mjhmc_hip.h"
#include "handles.hpp"
#include "ring_rows.hpp"
#include "ring_source.hpp"

namespace {

// any non-finite weight among w[k * Npad + p], k < n, p < N
__global__ __launch_bounds__(256) void cs_check_kernel(const double* __restrict__ w, int64_t Npad, int64_t N, int n,
                                                       int* __restrict__ bad) {
  int nonfinite = 0;
  for (int k = blockIdx.y; k < n; k += gridDim.y) {
    const double* wk = w + (size_t)k * Npad;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < N; p += (int64_t)gridDim.x * 256)
      if (!finite_f64(wk[p])) nonfinite = 1;
  }
  if (nonfinite) *bad = 1;
}

// lane g: elements [g * VEC, g * VEC + VEC) of every slot = chain g / chunks, columns (g % chunks) * VEC ...
template <typename T>
__global__ __launch_bounds__(256) void cs_chain_kernel(const T* __restrict__ base, const double* __restrict__ w,
                                                       const double* __restrict__ c, int64_t Npad, int64_t N, int n, int D,
                                                       int pitch, int chunks, double* __restrict__ a0,
                                                       double* __restrict__ a1, double* __restrict__ a2,
                                                       const int* __restrict__ bad) {
  constexpr int VEC = ChunkOf<T>::VEC;
  if (*bad) return;
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t total = N * chunks;
  if (g >= total) return;
  // (one division per lane; the 32-bit form where the launch allows it)
  const int64_t p = total <= 0xFFFFFFFFll ? (int64_t)((uint32_t)g / (uint32_t)chunks) : g / chunks;
  const int cx = (int)(g - p * chunks);
  const int col0 = cx * VEC;
  double cs[VEC], s1[VEC], s2[VEC];
  double2* const o1 = reinterpret_cast<double2*>(a1 + (size_t)g * VEC);
  double2* const o2 = reinterpret_cast<double2*>(a2 + (size_t)g * VEC);
#pragma unroll
  for (int j = 0; j < VEC; j += 2) {
    const double2 q1 = o1[j / 2], q2 = o2[j / 2];
    s1[j] = q1.x;
    s1[j + 1] = q1.y;
    s2[j] = q2.x;
    s2[j + 1] = q2.y;
    cs[j] = col0 + j < D ? c[col0 + j] : 0.0;
    cs[j + 1] = col0 + j + 1 < D ? c[col0 + j + 1] : 0.0;
  }
  double s0 = a0[p];
  const size_t slot_elems = (size_t)Npad * pitch;
  const T* const x0 = base + (size_t)g * VEC;
  const double* const w0 = w ? w + p : nullptr;
  for (int k0 = 0; k0 < n; k0 += kSlotsInFlight) {
    uint4 q[kSlotsInFlight];
    double wt[kSlotsInFlight];
#pragma unroll
    for (int u = 0; u < kSlotsInFlight; ++u) {
      wt[u] = 1.0;
      if (k0 + u < n) {
        q[u] = *reinterpret_cast<const uint4*>(x0 + (size_t)(k0 + u) * slot_elems);
        if (w0) wt[u] = w0[(size_t)(k0 + u) * Npad];
      }
    }
#pragma unroll
    for (int u = 0; u < kSlotsInFlight; ++u) {
      if (k0 + u < n) {
        double x[VEC];
        ChunkOf<T>::widen(q[u], x);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          const double t = x[j] - cs[j];
          const double wd = wt[u] * t;
          s1[j] = s1[j] + wd;
          s2[j] = s2[j] + wd * t;
        }
        s0 = s0 + wt[u];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < VEC; j += 2) {
    o1[j / 2] = make_double2(s1[j], s1[j + 1]);
    o2[j / 2] = make_double2(s2[j], s2[j + 1]);
  }
  if (cx == 0) a0[p] = s0;   // (every lane of the row holds the same sum; the first one's)
}

// partial[(bx * 3 + j) * pitch + col] = the workgroup's sum over its chains of m, m^2, v (j = 0, 1, 2);
// partial_w[bx] = its sum of a0
__global__ __launch_bounds__(256) void cs_fold_kernel(const double* __restrict__ a0, const double* __restrict__ a1,
                                                      const double* __restrict__ a2, int64_t N, int D, int pitch, int cw,
                                                      int log_cw, double* __restrict__ partial,
                                                      double* __restrict__ partial_w) {
  __shared__ double sm[256][5];
  const int tid = threadIdx.x;
  const int cx = tid & (cw - 1), ry = tid >> log_cw, rw = 256 >> log_cw;
  const int col = blockIdx.y * cw + cx;
  const bool active = col < D;
  double tm = 0.0, tq = 0.0, tv = 0.0, tw = 0.0;
  const int64_t stride = (int64_t)gridDim.x * rw;
#pragma unroll 4
  for (int64_t p = (int64_t)blockIdx.x * rw + ry; p < N; p += stride) {
    const double wp = a0[p];
    tw += wp;
    if (active) {
      const double m = a1[(size_t)p * pitch + col] / wp;
      const double mm = m * m;
      const double v = a2[(size_t)p * pitch + col] / wp - mm;
      tm += m;
      tq += mm;
      tv += v;
    }
  }
  sm[tid][0] = tm;
  sm[tid][1] = tq;
  sm[tid][2] = tv;
  sm[tid][3] = tw;
  __syncthreads();
  // the row lanes of a column, in index order
  for (int o = tid; o < cw * 3; o += 256) {
    const int cxo = o / 3, j = o - cxo * 3;
    double t = 0.0;
    for (int r = 0; r < rw; ++r) t += sm[r * cw + cxo][j];
    const int colo = blockIdx.y * cw + cxo;
    if (colo < D) partial[((size_t)blockIdx.x * 3 + j) * pitch + colo] = t;
  }
  if (blockIdx.y == 0 && tid == 0) {
    double t = 0.0;
    for (int r = 0; r < rw; ++r) t += sm[r * cw][3];
    partial_w[blockIdx.x] = t;
  }
}

// out[0] = sum_b partial_w[b]; out[1 + j * D + d] = sum_b partial[(b * 3 + j) * pitch + d].  A workgroup is 16 outputs x
// 16 lanes over b: lane q adds b = q, q + 16, ... in index order, then the 16 lane sums are added in index order -- a
// fixed order for a given gx.
__global__ __launch_bounds__(256) void cs_fold_finish_kernel(const double* __restrict__ partial,
                                                             const double* __restrict__ partial_w, int gx, int D, int pitch,
                                                             double* __restrict__ out) {
  __shared__ double sm[16][17];
  const int o = threadIdx.x & 15, q = threadIdx.x >> 4;
  const int i = blockIdx.x * 16 + o;
  double t = 0.0;
  if (i <= 3 * D) {
    if (i == 0) {
      for (int b = q; b < gx; b += 16) t += partial_w[b];
    } else {
      const int j = (i - 1) / D, d = (i - 1) - j * D;
      const double* col = partial + (size_t)j * pitch + d;
      for (int b = q; b < gx; b += 16) t += col[(size_t)b * 3 * pitch];
    }
  }
  sm[q][o] = t;
  __syncthreads();
  if (q == 0 && i <= 3 * D) {
    double s = 0.0;
    for (int r = 0; r < 16; ++r) s += sm[r][o];
    out[i] = s;
  }
}

// src [N][pitch] float64 rows -> dst (D, N) row-major (the host layout of every array of the reference)
__global__ void cs_to_dim_major(const double* __restrict__ src, double* __restrict__ dst, int D, int64_t N, int pitch) {
  __shared__ double tile[32][33];
  const int64_t p0 = (int64_t)blockIdx.x * 32;
  const int d0 = blockIdx.y * 32;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int pp = threadIdx.y + 8 * i;
    const int64_t p = p0 + pp;
    const int d = d0 + threadIdx.x;
    if (d < D && p < N) tile[pp][threadIdx.x] = src[(size_t)p * pitch + d];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int dd = threadIdx.y + 8 * i;
    const int d = d0 + dd;
    const int64_t p = p0 + threadIdx.x;
    if (d < D && p < N) dst[(size_t)d * N + p] = tile[threadIdx.x][dd];
  }
}

}  // namespace

ChainFoldPlan chain_fold_plan(const RingView& r) {
  ChainFoldPlan pl;
  pl.cw = std::min(256, pow2ceil(r.D));
  pl.log_cw = ilog2(pl.cw);
  pl.gy = (r.D + pl.cw - 1) / pl.cw;
  const int rw = 256 / pl.cw;
  // about four workgroups per compute unit, each row lane with at least four chains
  const int64_t want = std::max<int64_t>(1, 1024 / pl.gy);
  const int64_t have = (r.N + (int64_t)rw * 4 - 1) / ((int64_t)rw * 4);
  pl.gx = (int)std::max<int64_t>(1, std::min(want, have));
  pl.partial_elems = (size_t)pl.gx * 3 * r.pitch + pl.gx;
  return pl;
}

int chain_accumulate(hipStream_t st, const RingView& r, int n, const double* w, const double* c, double* a0, double* a1,
                     double* a2, int* bad, std::string& err) {
  if (w) {
    const unsigned bx = (unsigned)std::min<int64_t>(1024, (r.N + 255) / 256);
    hipLaunchKernelGGL(cs_check_kernel, dim3(bx, (unsigned)std::min(n, 1024)), dim3(256), 0, st, w, r.Npad, r.N, n, bad);
  }
  const int vec = r.dtype == MJHMC_F64 ? 2 : (r.dtype == MJHMC_F32 ? 4 : 8);
  const int chunks = r.pitch / vec;   // (a row is whole 16-byte chunks: pick_shape, shape_for)
  const int64_t lanes = r.N * chunks;
  const dim3 grid((unsigned)((lanes + 255) / 256)), block(256);
  dispatch_dtype(r.dtype, [&](auto tag) {
    typedef typename decltype(tag)::type T;
    hipLaunchKernelGGL(cs_chain_kernel<T>, grid, block, 0, st, (const T*)r.base, w, c, r.Npad, r.N, n, r.D, r.pitch, chunks,
                       a0, a1, a2, bad);
  });
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    err = std::string("chain pass: ") + hipGetErrorString(e);
    return MJHMC_ERR_HIP;
  }
  return 0;
}

int chain_fold(hipStream_t st, const RingView& r, const ChainFoldPlan& pl, const double* a0, const double* a1,
               const double* a2, double* partial, double* out, std::string& err) {
  double* partial_w = partial + (size_t)pl.gx * 3 * r.pitch;
  hipLaunchKernelGGL(cs_fold_kernel, dim3(pl.gx, pl.gy), dim3(256), 0, st, a0, a1, a2, r.N, r.D, r.pitch, pl.cw, pl.log_cw,
                     partial, partial_w);
  hipLaunchKernelGGL(cs_fold_finish_kernel, dim3((3 * r.D + 1 + 15) / 16), dim3(256), 0, st, partial, partial_w, pl.gx, r.D,
                     r.pitch, out);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    err = std::string("chain fold: ") + hipGetErrorString(e);
    return MJHMC_ERR_HIP;
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// The accumulator handle of the C ABI (include/mjhmc_hip.h: mjhmc_chainstats_*)
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kChainMaxParts = 2;

struct mjhmc_chainstats : RingAccumulator {   // (ring_gen: the sums have that ring's row layout)
  using RingAccumulator::RingAccumulator;
  int D = 0, pitch = 0;       // dimensions and row pitch of a state of that ring
  int n_parts = 1;
  ChainFoldPlan plan;
  double* acc = nullptr;      // [n_parts] x { a0 [Npad], a1 [Npad][pitch], a2 [Npad][pitch] }
  double* shift = nullptr;    // [D]
  double* fpart = nullptr;    // the fold's per-workgroup partials
  double* fout = nullptr;     // [1 + 3 D]
  ~mjhmc_chainstats() override { free_device({acc, shift, fpart, fout}); }
  int64_t n_slots[kChainMaxParts] = {0, 0};   // states per chain added to each part
  size_t part_elems() const { return (size_t)(2 * pitch + 1) * s->Npad; }
  double* a0(int h) const { return acc + (size_t)h * part_elems(); }
  double* a1(int h) const { return a0(h) + s->Npad; }
  double* a2(int h) const { return a1(h) + (size_t)s->Npad * pitch; }
};

static int chain_check_part(const mjhmc_chainstats* cs, int part) {
  if (!cs) return mjhmc_fail(MJHMC_ERR_INVALID, "chainstats is NULL");
  if (part < 0 || part >= cs->n_parts)
    return mjhmc_fail(MJHMC_ERR_INVALID, "part " + std::to_string(part) + " is outside [0, " + std::to_string(cs->n_parts) + ")");
  return 0;
}

static int chainstats_create_on_source(mjhmc_sampler* s, const mjhmc_functionals* fn, int n_parts, mjhmc_chainstats** out) {
  if (n_parts < 1 || n_parts > kChainMaxParts) return mjhmc_fail(MJHMC_ERR_INVALID, "n_parts must be 1 or 2");
  const RingSource src = ring_source(s, fn);
  if (!src.base) return acc_no_ring(fn);
  // the chain pass addresses a slot in 16-byte chunks of the state's own type: rows must be whole chunks of it
  const int vec = src.dtype == MJHMC_F64 ? 2 : (src.dtype == MJHMC_F32 ? 4 : 8);
  if (src.esize * vec != 16 || src.pitch % vec != 0)
    return mjhmc_fail(MJHMC_ERR_UNSUPPORTED, "the sampler's rows are not whole 16-byte chunks of its state type");
  HIPCHK(hipSetDevice(s->ctx->device));
  mjhmc_chainstats* cs = new mjhmc_chainstats("chainstats", "one", s, fn, src);
  cs->D = src.D;
  cs->pitch = src.pitch;
  cs->n_parts = n_parts;
  cs->plan = chain_fold_plan(ring_source_view(s, src, 0));
  const size_t D = (size_t)src.D, acc_bytes = (size_t)n_parts * cs->part_elems() * sizeof(double);
  hipError_t e = hipMalloc((void**)&cs->acc, acc_bytes);
  if (e == hipSuccess) e = hipMalloc((void**)&cs->shift, D * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&cs->fpart, cs->plan.partial_elems * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&cs->fout, (1 + 3 * D) * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&cs->bad, sizeof(int));
  if (e == hipSuccess) e = hipMemsetAsync(cs->acc, 0, acc_bytes, s->stream);
  if (e == hipSuccess) e = hipMemsetAsync(cs->shift, 0, D * sizeof(double), s->stream);
  if (e == hipSuccess) e = hipMemsetAsync(cs->bad, 0, sizeof(int), s->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
  if (e != hipSuccess) {
    delete cs;
    (void)hipGetLastError();
    char msg[256];
    std::snprintf(msg, sizeof(msg), "chain statistics buffers (%.3f GB of per-chain sums): %s", acc_bytes / 1e9,
                  hipGetErrorString(e));
    return mjhmc_fail(MJHMC_ERR_HIP, msg);
  }
  return acc_created(cs, out);
}

extern "C" {

int mjhmc_chainstats_create(mjhmc_sampler* s, int n_parts, mjhmc_chainstats** out) {
  if (!s || !out) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  return chainstats_create_on_source(s, nullptr, n_parts, out);
}

int mjhmc_chainstats_create_on(mjhmc_functionals* f, int n_parts, mjhmc_chainstats** out) {
  if (!f || !out) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  return chainstats_create_on_source(functionals_sampler(f), f, n_parts, out);
}

int mjhmc_chainstats_destroy(mjhmc_chainstats* cs) { return acc_destroy(cs); }

int mjhmc_chainstats_reset(mjhmc_chainstats* cs) {
  if (!cs) return mjhmc_fail(MJHMC_ERR_INVALID, "chainstats is NULL");
  mjhmc_sampler* s = cs->s;
  HIPCHK(hipSetDevice(s->ctx->device));
  HIPCHK(hipMemsetAsync(cs->acc, 0, (size_t)cs->n_parts * cs->part_elems() * sizeof(double), s->stream));
  HIPCHK(hipMemsetAsync(cs->bad, 0, sizeof(int), s->stream));
  for (int64_t& k : cs->n_slots) k = 0;
  return 0;
}

int mjhmc_chainstats_set_shift(mjhmc_chainstats* cs, const double* c) {
  if (!cs) return mjhmc_fail(MJHMC_ERR_INVALID, "chainstats is NULL");
  for (int64_t k : cs->n_slots)
    if (k != 0)
      return mjhmc_fail(MJHMC_ERR_INVALID, "the shift belongs to the sums already accumulated: mjhmc_chainstats_reset first");
  mjhmc_sampler* s = cs->s;
  HIPCHK(hipSetDevice(s->ctx->device));
  const size_t bytes = (size_t)cs->D * sizeof(double);
  if (c) {
    for (int d = 0; d < cs->D; ++d)
      if (!std::isfinite(c[d])) return mjhmc_fail(MJHMC_ERR_INVALID, "shift entry " + std::to_string(d) + " is not finite");
    HIPCHK(hipMemcpyAsync(cs->shift, c, bytes, hipMemcpyHostToDevice, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));   // (c is the caller's for the duration of the call only)
  } else {
    HIPCHK(hipMemsetAsync(cs->shift, 0, bytes, s->stream));
  }
  return 0;
}

int mjhmc_chainstats_accumulate(mjhmc_chainstats* cs, int part, int x_slot0, int w_slot0, int n) {
  TRY(chain_check_part(cs, part));
  mjhmc_sampler* s = cs->s;
  RingSource src;
  TRY(acc_begin(cs, x_slot0, w_slot0, n, &src));
  HIPCHK(hipSetDevice(s->ctx->device));
  const double* w = acc_weights(cs, w_slot0);
  std::string err;
  const int rc = chain_accumulate(s->stream, ring_source_view(s, src, x_slot0), n, w, cs->shift, cs->a0(part), cs->a1(part),
                                  cs->a2(part), cs->bad, err);
  if (rc) return mjhmc_fail(rc, err);
  if (w) {   // (unit weights raise no flag: nothing to wait for)
    int bad = 0;
    TRY(acc_take_flag(cs, &bad));
    if (bad) return acc_nonfinite_dwell(w_slot0, n);
  }
  cs->n_slots[part] += n;
  return 0;
}

int mjhmc_chainstats_read(mjhmc_chainstats* cs, int part, int64_t* n_chains, int64_t* n_states_per_chain, double* Sw,
                          double* Sm, double* Sq, double* Sv) {
  TRY(chain_check_part(cs, part));
  if (!n_chains || !n_states_per_chain || !Sw || !Sm || !Sq || !Sv) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  if (cs->n_slots[part] == 0)
    return mjhmc_fail(MJHMC_ERR_INVALID, "nothing has been added to part " + std::to_string(part) + " yet");
  mjhmc_sampler* s = cs->s;
  HIPCHK(hipSetDevice(s->ctx->device));
  std::string err;
  // (the fold reads the per-chain sums, not the ring: the view gives it N, D and the pitch)
  const int rc = chain_fold(s->stream, ring_source_view(s, ring_source(s, cs->fn), 0), cs->plan, cs->a0(part), cs->a1(part), cs->a2(part), cs->fpart,
                            cs->fout, err);
  if (rc) return mjhmc_fail(rc, err);
  const size_t D = (size_t)cs->D;
  std::vector<double> h(1 + 3 * D);
  HIPCHK(hipMemcpyAsync(h.data(), cs->fout, h.size() * sizeof(double), hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  *n_chains = s->N;
  *n_states_per_chain = cs->n_slots[part];
  *Sw = h[0];
  std::copy(h.begin() + 1, h.begin() + 1 + D, Sm);
  std::copy(h.begin() + 1 + D, h.begin() + 1 + 2 * D, Sq);
  std::copy(h.begin() + 1 + 2 * D, h.end(), Sv);
  return 0;
}

int mjhmc_chainstats_read_chains(mjhmc_chainstats* cs, int part, double* a0, double* a1, double* a2) {
  TRY(chain_check_part(cs, part));
  mjhmc_sampler* s = cs->s;
  HIPCHK(hipSetDevice(s->ctx->device));
  if (a0) TRY(copy_to_host(s, cs->a0(part), a0, (size_t)s->N * sizeof(double)));
  const size_t elems = (size_t)cs->D * s->N;
  double* const host[2] = {a1, a2};
  const double* const dev[2] = {cs->a1(part), cs->a2(part)};
  for (int m = 0; m < 2; ++m) {
    if (!host[m]) continue;
    TRY(ensure_stage(s, elems));
    const dim3 grid((unsigned)((s->N + 31) / 32), (unsigned)((cs->D + 31) / 32)), block(32, 8);
    hipLaunchKernelGGL(cs_to_dim_major, grid, block, 0, s->stream, dev[m], s->stage, cs->D, s->N, cs->pitch);
    HIPCHK(hipGetLastError());
    TRY(copy_to_host(s, s->stage, host[m], elems * sizeof(double)));
  }
  return 0;
}

}  // extern "C"
