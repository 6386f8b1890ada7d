// Cell occupancy and transition counts of the recorded chains, on the device: how much time the ensemble spends in each
// region of the state space and how often a chain moves from one to another, without downloading a trajectory.
//
// Definition (the contract; include/mjhmc_hip.h: mjhmc_occupancy_accumulate).  M centres c[m] of K = D coordinates, 1 <= M <=
// 64, an optional squared radius r2[m] (+inf: none) and one quantum q (a power of two).  The cells are the Voronoi cells of
// the centres -- with radii, their intersections with the balls (core sets) -- plus cell M, "outside".
//
// Label of a state row x (float64, float32 or bfloat16 in the ring, widened exactly to float64).  For m ascending:
//   d2_m = 0.0;  for d ascending below K:  t = x_d - c[m][d];  d2_m = d2_m + t * t      every operation rounded (built with
//                                                                   -ffp-contract=off; padding elements are skipped)
//   best = +inf, label = M;  m replaces the label only when d2_m < best, strictly: the lowest index wins ties, and a NaN or
//   infinite distance is never chosen, so a row that is not finite lands outside with no special case
//   with radii: label = M unless best <= r2[label]
// A label is a function of (x, centres, r2) alone and equals the NumPy loop `d2 = d2 + (X[d] - C[:, d, None])**2` bit for bit.
//
// Tables, all uint64, indexed by cell in [0, M].  u = rint(w / q), nearest-even, the division exact:
//   count[a], mass[a]            states in cell a and their units, over every state of every chain
//   trans[a][b]                  pairs (state s, state s + 1) of one chain with labels a, b, pairs that straddle two
//                                linked blocks included
//   from_count[a], from_mass[a]  count / mass restricted to the states that have a successor; from_count[a] is the row sum
//                                of trans
//   W_units                      the sum of units
// and per chain p: switches[p], the transitions with a != b (the outside cell is a cell), and visited[p], a 64-bit mask of
// the cells < M seen.  mjhmc_occupancy_read tallies them with integer atomics: chains_by_switches (17 entries: 0 .. 15 and
// >= 16) and chains_by_cells (M + 1 entries: the chains that saw exactly c distinct cells).
// Everything is an integer sum plus a per-chain carry -- the label and the units of the chain's last state -- so the tables
// are bit-identical from run to run and for every cut of a run into linked blocks.  There is no floating-point atomic in
// this file; LDS and global integer atomics are used.  States and weights pair as in mjhmc_histogram_accumulate, whose
// weight check, decision and refusals are used as they are (histograms.hpp): a refused block adds nothing and leaves the
// carry as it was.
//
// Four launches per block, one stream:
//   hist_check_kernel, hist_decide_kernel   the weight logic of histograms.hip (histogram_weight_pass): flags, W_units
//   occ_label_kernel<DT, KV>   (occupancy.hpp) the block's labels, uint8 [n][Npad], into the handle's scratch; it reads no
//                              flag and changes nothing but the scratch
//   occ_count_kernel           one lane per chain walks the block's n labels in slot order, from the chain's carried
//                              (label, units) when the block is linked; a workgroup keeps count, mass, from_count, from_mass
//                              and trans in LDS ((M + 1)^2 + 4 (M + 1) u64: 35 880 bytes at M = 64), adds with ds_add_u64
//                              and flushes its non-zero entries with global u64 atomics; switches, visited and the carry
//                              are plain vector stores.  It returns at its top when a flag is up.
#include "occupancy.hpp"

#include <cmath>
#include <vector>

#include "../../include/mjhmc_hip.h"
#include "handles.hpp"
#include "histograms.hpp"
#include "ring_source.hpp"

namespace mjhmc {

namespace {

template <int DT>
void label_launch(const OccLabelArgs& a, dim3 grid, hipStream_t stream) {
  if (occ_lane_centres(a.M) == 1)
    hipLaunchKernelGGL((occ_label_kernel<DT, 1>), grid, dim3(256), 0, stream, a);
  else
    hipLaunchKernelGGL((occ_label_kernel<DT, 4>), grid, dim3(256), 0, stream, a);
}

}  // namespace

bool occ_label_launch(const OccLabelArgs& a, int state_dtype, hipStream_t stream) {
  const dim3 grid((unsigned)((a.N + kOccRows - 1) / kOccRows), (unsigned)(a.n < 1024 ? a.n : 1024));
  if (state_dtype == 0) label_launch<0>(a, grid, stream);
  else if (state_dtype == 1) label_launch<1>(a, grid, stream);
  else if (state_dtype == 2) label_launch<2>(a, grid, stream);
  else return false;
  return true;
}

}  // namespace mjhmc

namespace {

typedef unsigned long long u64;

constexpr double kTwo53 = 9007199254740992.0;
constexpr int kOccSwitchBins = 17;   // chains_by_switches: 0 .. 15 and >= 16
constexpr int kOccInFlight = 4;      // labels and weights a lane loads before it uses the first

struct OccCountArgs {
  const uint8_t* labels;   // [n][Npad]
  const double* w;         // [n][Npad], or nullptr: unit weights
  double inv_q;
  long long Npad, N;
  int n, M, linked;
  uint8_t* carry_label;    // [Npad] the label and
  u64* carry_units;        // [Npad] the units of the chain's last state
  uint32_t* switches;      // [Npad]
  u64* visited;            // [Npad]
  u64* tables;             // count, mass, from_count, from_mass [M + 1] each, trans [M + 1][M + 1]
  const int* bad;
};

__global__ __launch_bounds__(256) void occ_count_kernel(OccCountArgs a) {
  extern __shared__ u64 occ_lds[];
  if (*a.bad) return;
  const int C = a.M + 1, cells = 4 * C + C * C;
  const int tid = threadIdx.x;
  for (int i = tid; i < cells; i += 256) occ_lds[i] = 0;
  __syncthreads();
  u64* const lcount = occ_lds;
  u64* const lmass = occ_lds + C;
  u64* const lfrom_count = occ_lds + 2 * C;
  u64* const lfrom_mass = occ_lds + 3 * C;
  u64* const ltrans = occ_lds + 4 * C;
  const long long p = (long long)blockIdx.x * 256 + tid;
  if (p < a.N) {
    int prev = -1;
    u64 prev_units = 0;
    if (a.linked) {
      prev = a.carry_label[p];
      prev_units = a.carry_units[p];
    }
    uint32_t sw = a.switches[p];
    u64 vis = a.visited[p];
    const u64 unit = (u64)rint(a.inv_q);   // a unit weight's units
    for (int k0 = 0; k0 < a.n; k0 += kOccInFlight) {
      int lab[kOccInFlight];
      double wt[kOccInFlight];
#pragma unroll
      for (int u = 0; u < kOccInFlight; ++u) {
        const int k = k0 + u;
        lab[u] = 0;
        wt[u] = 0.0;
        if (k < a.n) {
          lab[u] = a.labels[(size_t)k * a.Npad + p];
          if (a.w) wt[u] = a.w[(size_t)k * a.Npad + p];
        }
      }
#pragma unroll
      for (int u = 0; u < kOccInFlight; ++u) {
        if (k0 + u >= a.n) break;
        const int b = lab[u];
        const u64 units = a.w ? (u64)rint(wt[u] * a.inv_q) : unit;   // (the check passed: 0 <= w / q < 2^53)
        atomicAdd(&lcount[b], 1ull);
        atomicAdd(&lmass[b], units);
        if (prev >= 0) {
          atomicAdd(&lfrom_count[prev], 1ull);
          atomicAdd(&lfrom_mass[prev], prev_units);
          atomicAdd(&ltrans[prev * C + b], 1ull);
          sw += prev != b;
        }
        if (b < a.M) vis |= 1ull << b;
        prev = b;
        prev_units = units;
      }
    }
    a.carry_label[p] = (uint8_t)prev;
    a.carry_units[p] = prev_units;
    a.switches[p] = sw;
    a.visited[p] = vis;
  }
  __syncthreads();
  for (int i = tid; i < cells; i += 256) {
    const u64 v = occ_lds[i];
    if (v) atomicAdd(&a.tables[i], v);
  }
}

// by_switches[min(switches[p], 16)] += 1 and by_cells[popcount(visited[p])] += 1 over the chains p < N
__global__ __launch_bounds__(256) void occ_tally_kernel(const uint32_t* __restrict__ switches, const u64* __restrict__ visited,
                                                        long long N, int M, u64* __restrict__ by_switches,
                                                        u64* __restrict__ by_cells) {
  __shared__ uint32_t sm[kOccSwitchBins + mjhmc::kOccMaxCentres + 1];
  const int tid = threadIdx.x, cells = kOccSwitchBins + M + 1;
  for (int i = tid; i < cells; i += 256) sm[i] = 0;
  __syncthreads();
  for (long long p = (long long)blockIdx.x * 256 + tid; p < N; p += (long long)gridDim.x * 256) {
    const uint32_t sw = switches[p];
    atomicAdd(&sm[sw < 16u ? sw : 16u], 1u);
    atomicAdd(&sm[kOccSwitchBins + __popcll(visited[p])], 1u);
  }
  __syncthreads();
  for (int i = tid; i < cells; i += 256) {
    const uint32_t c = sm[i];
    if (c) atomicAdd(i < kOccSwitchBins ? &by_switches[i] : &by_cells[i - kOccSwitchBins], (u64)c);
  }
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
// The accumulator handle of the C ABI (include/mjhmc_hip.h: mjhmc_occupancy_*)
// ---------------------------------------------------------------------------------------------------------------------
struct mjhmc_occupancy : RingAccumulator {
  using RingAccumulator::RingAccumulator;
  int M = 0, D = 0;
  double inv_q = 1.0;
  int check_gx = 1, check_gy = 1;
  int label_slots = 0;        // slots the label scratch holds (the ring's, at create)
  int last_n = 0;             // slots of the last block labelled
  bool has_carry = false;     // a block was added since create / reset
  double* centres = nullptr;  // Ct [Dpad][64], then r2 [64]
  size_t ct_elems = 0;
  uint8_t* labels = nullptr;  // [label_slots][Npad]
  u64* tables = nullptr;      // count, mass, from_count, from_mass [M + 1], trans [M + 1][M + 1], W_units; then the tallies of a
                              // read: chains_by_switches [17], chains_by_cells [M + 1]
  u64* partial = nullptr;     // the weight check's per-workgroup units
  u64* chain64 = nullptr;     // carry_units [Npad], visited [Npad]
  uint32_t* switches = nullptr;   // [Npad]
  uint8_t* carry_label = nullptr; // [Npad]
  ~mjhmc_occupancy() override { free_device({centres, labels, tables, partial, chain64, switches, carry_label}); }
  int C() const { return M + 1; }
  size_t cells() const { return 4 * (size_t)C() + (size_t)C() * C(); }   // without W_units
  u64* W_units() const { return tables + cells(); }
  u64* tallies() const { return tables + cells() + 1; }
  size_t tally_cells() const { return (size_t)kOccSwitchBins + C(); }
  size_t table_bytes() const { return (cells() + 1 + tally_cells()) * sizeof(u64); }
  u64* carry_units() const { return chain64; }
  u64* visited() const { return chain64 + s->Npad; }
};

// what reset zeroes: the tables and the per-chain state (the label scratch and the carry need none: has_carry says
// whether the carry means anything)
static hipError_t occupancy_zero(mjhmc_occupancy* h) {
  mjhmc_sampler* s = h->s;
  hipError_t e = hipMemsetAsync(h->tables, 0, h->table_bytes(), s->stream);
  if (e == hipSuccess) e = hipMemsetAsync(h->chain64, 0, 2 * (size_t)s->Npad * sizeof(u64), s->stream);
  if (e == hipSuccess) e = hipMemsetAsync(h->switches, 0, (size_t)s->Npad * sizeof(uint32_t), s->stream);
  if (e == hipSuccess) e = hipMemsetAsync(h->carry_label, 0, (size_t)s->Npad, s->stream);
  if (e == hipSuccess) e = hipMemsetAsync(h->bad, 0, sizeof(int), s->stream);
  h->n_states = 0;
  h->has_carry = false;
  return e;
}

// the label pass of a block into the handle's scratch; false: no kernel for the ring's state type
static bool occupancy_launch_labels(mjhmc_occupancy* h, const RingView& r, int n) {
  const int vec = r.dtype == MJHMC_F64 ? 2 : (r.dtype == MJHMC_F32 ? 4 : 8);
  const mjhmc::OccLabelArgs la{r.base, h->labels, h->centres, h->centres + h->ct_elems, r.Npad, r.N, n, r.D, r.pitch / vec, h->M};
  h->last_n = n;
  return mjhmc::occ_label_launch(la, r.dtype, h->s->stream);
}

// the count pass over the n slots of labels in the scratch
static void occupancy_launch_count(mjhmc_occupancy* h, const RingView& r, const double* w, int n, int linked) {
  const OccCountArgs ca{h->labels, w, h->inv_q, r.Npad, r.N, n, h->M, linked, h->carry_label, h->carry_units(), h->switches,
                        h->visited(), h->tables, h->bad};
  hipLaunchKernelGGL(occ_count_kernel, dim3((unsigned)((r.N + 255) / 256)), dim3(256), h->cells() * sizeof(u64), h->s->stream, ca);
}

// have: the sampler or the functionals handle was given (s itself is looked at only after the argument checks that need none)
static int occupancy_create_on_source(bool have, mjhmc_sampler* s, const mjhmc_functionals* fn, int n_centres, int n_dims,
                                      const double* centres, const double* r2, double quantum, mjhmc_occupancy** out) {
  using mjhmc::kOccMaxCentres;
  if (n_centres < 1 || n_centres > kOccMaxCentres)
    return mjhmc_fail(MJHMC_ERR_INVALID, "the number of centres M must be in [1, " + std::to_string(kOccMaxCentres) + "], got " +
                                             std::to_string(n_centres));
  int exp2 = 0;
  if (!(quantum > 0.0) || !std::isfinite(quantum) || std::frexp(quantum, &exp2) != 0.5)
    return mjhmc_fail(MJHMC_ERR_INVALID, "the quantum must be a positive power of two");
  const double inv_q = 1.0 / quantum;   // exact, unless it leaves the normal range
  if (!std::isnormal(inv_q) || !std::isnormal(quantum))
    return mjhmc_fail(MJHMC_ERR_INVALID, "the quantum must be a positive power of two whose inverse is a normal float64");
  if (!have || !centres || !out) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  if (n_dims < 1) return mjhmc_fail(MJHMC_ERR_INVALID, "the centres must have at least one coordinate");
  const int M = n_centres;
  for (int m = 0; m < M; ++m) {
    for (int d = 0; d < n_dims; ++d)
      if (!std::isfinite(centres[(size_t)m * n_dims + d]))
        return mjhmc_fail(MJHMC_ERR_INVALID, "coordinate " + std::to_string(d) + " of centre " + std::to_string(m) + " is not finite");
    if (r2 && !(r2[m] >= 0.0))
      return mjhmc_fail(MJHMC_ERR_INVALID, "the squared radius of centre " + std::to_string(m) + " is negative or NaN");
  }
  if (fn) s = functionals_sampler(fn);
  const RingSource src = ring_source(s, fn);
  const int D = src.D;
  if (n_dims != D)
    return mjhmc_fail(MJHMC_ERR_INVALID, "the centres have " + std::to_string(n_dims) + " coordinates, a state of the " + src.name() +
                                             " has " + std::to_string(D));
  if (!src.base) return acc_no_ring(fn);
  // the label pass addresses a row in 16-byte chunks of the state's own type: rows must be whole chunks of it
  const int vec = src.dtype == MJHMC_F64 ? 2 : (src.dtype == MJHMC_F32 ? 4 : 8);
  if (src.esize * vec != 16 || src.pitch % vec != 0)
    return mjhmc_fail(MJHMC_ERR_UNSUPPORTED, "the sampler's rows are not whole 16-byte chunks of its state type");
  // centres transposed and zero-padded, then the squared radii
  const size_t Dpad = ((size_t)D + 63) / 64 * 64;
  std::vector<double> ct(Dpad * kOccMaxCentres + kOccMaxCentres, 0.0);
  for (int m = 0; m < M; ++m)
    for (int d = 0; d < D; ++d) ct[(size_t)d * kOccMaxCentres + m] = centres[(size_t)m * D + d];
  for (int m = 0; m < kOccMaxCentres; ++m) ct[Dpad * kOccMaxCentres + m] = (r2 && m < M) ? r2[m] : HUGE_VAL;
  HIPCHK(hipSetDevice(s->ctx->device));
  mjhmc_occupancy* h = new mjhmc_occupancy("occupancy", "occupancy accumulator", s, fn, src);
  h->M = M;
  h->D = D;
  h->inv_q = inv_q;
  h->ct_elems = Dpad * kOccMaxCentres;
  h->label_slots = src.slots;
  histogram_check_grid(s->N, &h->check_gx, &h->check_gy);
  const size_t partial_bytes = (size_t)h->check_gx * h->check_gy * sizeof(u64);
  const size_t Npad = (size_t)s->Npad;
  hipError_t e = hipMalloc((void**)&h->centres, ct.size() * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&h->labels, (size_t)h->label_slots * Npad);
  if (e == hipSuccess) e = hipMalloc((void**)&h->tables, h->table_bytes());
  if (e == hipSuccess) e = hipMalloc((void**)&h->partial, partial_bytes);
  if (e == hipSuccess) e = hipMalloc((void**)&h->chain64, 2 * Npad * sizeof(u64));
  if (e == hipSuccess) e = hipMalloc((void**)&h->switches, Npad * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMalloc((void**)&h->carry_label, Npad);
  if (e == hipSuccess) e = hipMalloc((void**)&h->bad, sizeof(int));
  if (e == hipSuccess) e = hipMemcpyAsync(h->centres, ct.data(), ct.size() * sizeof(double), hipMemcpyHostToDevice, s->stream);
  if (e == hipSuccess) e = hipMemsetAsync(h->labels, 0, (size_t)h->label_slots * Npad, s->stream);
  if (e == hipSuccess) e = hipMemsetAsync(h->partial, 0, partial_bytes, s->stream);
  if (e == hipSuccess) e = occupancy_zero(h);
  if (e == hipSuccess) e = hipStreamSynchronize(s->stream);   // (ct is this call's)
  if (e != hipSuccess) {
    delete h;
    (void)hipGetLastError();
    return mjhmc_fail(MJHMC_ERR_HIP, std::string("occupancy buffers: ") + hipGetErrorString(e));
  }
  return acc_created(h, out);
}

extern "C" {

int mjhmc_occupancy_create(mjhmc_sampler* s, int n_centres, int n_dims, const double* centres, const double* r2, double quantum,
                           mjhmc_occupancy** out) {
  return occupancy_create_on_source(s != nullptr, s, nullptr, n_centres, n_dims, centres, r2, quantum, out);
}

int mjhmc_occupancy_create_on(mjhmc_functionals* f, int n_centres, int n_dims, const double* centres, const double* r2,
                              double quantum, mjhmc_occupancy** out) {
  return occupancy_create_on_source(f != nullptr, nullptr, f, n_centres, n_dims, centres, r2, quantum, out);
}

int mjhmc_occupancy_destroy(mjhmc_occupancy* h) { return acc_destroy(h); }

int mjhmc_occupancy_info(mjhmc_occupancy* h, int* n_centres, int* n_dims, int* label_slots) {
  if (!h || !n_centres || !n_dims || !label_slots) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  *n_centres = h->M;
  *n_dims = h->D;
  *label_slots = h->label_slots;
  return 0;
}

int mjhmc_occupancy_reset(mjhmc_occupancy* h) {
  if (!h) return mjhmc_fail(MJHMC_ERR_INVALID, "occupancy accumulator is NULL");
  HIPCHK(hipSetDevice(h->s->ctx->device));
  HIPCHK(occupancy_zero(h));
  return 0;
}

int mjhmc_occupancy_accumulate(mjhmc_occupancy* h, int x_slot0, int w_slot0, int n, int linked) {
  if (!h) return mjhmc_fail(MJHMC_ERR_INVALID, "occupancy accumulator is NULL");
  mjhmc_sampler* s = h->s;
  RingSource src;
  TRY(acc_begin(h, x_slot0, w_slot0, n, &src));
  if (linked != 0 && linked != 1) return mjhmc_fail(MJHMC_ERR_INVALID, "linked must be 0 or 1, got " + std::to_string(linked));
  if (linked && !h->has_carry)
    return mjhmc_fail(MJHMC_ERR_INVALID, "linked = 1, but no block was added since create or reset: there is no state to follow");
  if (w_slot0 < 0 && !(h->inv_q < kTwo53))
    return mjhmc_fail(MJHMC_ERR_INVALID, "a unit weight is 2^53 quanta or more: w / quantum must stay below 2^53");
  HIPCHK(hipSetDevice(s->ctx->device));
  const double* w = acc_weights(h, w_slot0);
  const RingView r = ring_source_view(s, src, x_slot0);
  histogram_weight_pass(s->stream, w, r.Npad, r.N, n, h->inv_q, h->check_gx, h->check_gy, h->partial, h->W_units(), h->bad);
  if (!occupancy_launch_labels(h, r, n)) return mjhmc_fail(MJHMC_ERR_UNSUPPORTED, "there is no label kernel for the ring's state type");
  occupancy_launch_count(h, r, w, n, linked);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mjhmc_fail(MJHMC_ERR_HIP, std::string("occupancy pass: ") + hipGetErrorString(e));
  TRY(acc_end(h, n, [&](int bad) { return histogram_refusal(bad, w_slot0, n); }));
  h->has_carry = true;
  return 0;
}

int mjhmc_occupancy_read(mjhmc_occupancy* h, uint64_t* count, uint64_t* mass, uint64_t* from_count, uint64_t* from_mass,
                         uint64_t* trans, uint64_t* W_units, uint64_t* chains_by_switches, uint64_t* chains_by_cells,
                         uint32_t* switches, uint64_t* visited, int64_t* n_states) {
  if (!h || !count || !mass || !from_count || !from_mass || !trans || !W_units || !chains_by_switches || !chains_by_cells ||
      !n_states)
    return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  mjhmc_sampler* s = h->s;
  HIPCHK(hipSetDevice(s->ctx->device));
  const size_t C = (size_t)h->C();
  HIPCHK(hipMemsetAsync(h->tallies(), 0, h->tally_cells() * sizeof(u64), s->stream));
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(1024, (s->N + 255) / 256));
  hipLaunchKernelGGL(occ_tally_kernel, dim3(grid), dim3(256), 0, s->stream, h->switches, h->visited(), (long long)s->N, h->M,
                     h->tallies(), h->tallies() + kOccSwitchBins);
  HIPCHK(hipGetLastError());
  std::vector<u64> host(h->table_bytes() / sizeof(u64));
  HIPCHK(hipMemcpyAsync(host.data(), h->tables, h->table_bytes(), hipMemcpyDeviceToHost, s->stream));
  if (switches) HIPCHK(hipMemcpyAsync(switches, h->switches, (size_t)s->N * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
  if (visited) HIPCHK(hipMemcpyAsync(visited, h->visited(), (size_t)s->N * sizeof(u64), hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  const u64* t = host.data();
  std::copy(t, t + C, count);
  std::copy(t + C, t + 2 * C, mass);
  std::copy(t + 2 * C, t + 3 * C, from_count);
  std::copy(t + 3 * C, t + 4 * C, from_mass);
  std::copy(t + 4 * C, t + 4 * C + C * C, trans);
  *W_units = t[h->cells()];
  std::copy(t + h->cells() + 1, t + h->cells() + 1 + kOccSwitchBins, chains_by_switches);
  std::copy(t + h->cells() + 1 + kOccSwitchBins, t + h->cells() + 1 + kOccSwitchBins + C, chains_by_cells);
  *n_states = h->n_states;
  return 0;
}

int mjhmc_occupancy_read_labels(mjhmc_occupancy* h, int n, uint8_t* labels) {
  if (!h || !labels) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  if (n < 1 || n > h->last_n)
    return mjhmc_fail(MJHMC_ERR_INVALID, "n must be in [1, " + std::to_string(h->last_n) + "], the slots of the last block, got " +
                                             std::to_string(n));
  mjhmc_sampler* s = h->s;
  HIPCHK(hipSetDevice(s->ctx->device));
  HIPCHK(hipMemcpy2DAsync(labels, (size_t)s->N, h->labels, (size_t)s->Npad, (size_t)s->N, (size_t)n, hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  return 0;
}

#ifdef MJHMC_TEST_HOOKS
// test build only (tools/occupancy_bench.py): ONE of the two passes of a block, so that they can be timed apart -- part 0
// the label pass into the scratch, part 1 the count pass over the n slots of labels the scratch holds (unlinked; the
// weights are not checked: the caller's are valid); no flag read-back, synchronised at the end
int mjhmc_test_occupancy_part(mjhmc_occupancy* h, int x_slot0, int w_slot0, int n, int part) {
  if (!h || (part != 0 && part != 1)) return mjhmc_fail(MJHMC_ERR_INVALID, "bad argument");
  mjhmc_sampler* s = h->s;
  RingSource src;
  TRY(acc_begin(h, x_slot0, w_slot0, n, &src));
  if (part == 1 && n > h->last_n) return mjhmc_fail(MJHMC_ERR_INVALID, "the scratch holds fewer slots of labels");
  HIPCHK(hipSetDevice(s->ctx->device));
  const RingView r = ring_source_view(s, src, x_slot0);
  if (part == 0) {
    if (!occupancy_launch_labels(h, r, n)) return mjhmc_fail(MJHMC_ERR_UNSUPPORTED, "no label kernel for the ring's state type");
  } else {
    occupancy_launch_count(h, r, acc_weights(h, w_slot0), n, 0);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(s->stream));
  return 0;
}

// test build only: every byte of the padding ELEMENTS (ndims <= d < pitch) of all Npad rows of ring slot `slot` set to
// `byte` -- garbage no label may depend on (0xFF: NaN in every state type)
int mjhmc_test_ring_fill_element_padding(mjhmc_sampler* s, int slot, int byte) {
  if (!s || slot < 0 || slot >= s->ring_slots) return mjhmc_fail(MJHMC_ERR_INVALID, "bad argument");
  HIPCHK(hipSetDevice(s->ctx->device));
  const size_t used = (size_t)s->D * s->sh.esize;
  if (row_bytes(s) > used)
    HIPCHK(hipMemset2DAsync((char*)s->ring + (size_t)slot * mat_bytes(s) + used, row_bytes(s), byte, row_bytes(s) - used,
                            (size_t)s->Npad, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  return 0;
}
#endif

}  // extern "C"
