// The multi-pass sampler: the particle state and the proposal columns live in HBM between the substeps of an iteration,
// and every substep is a plain kernel over rows -- kick, drift, an energy evaluation, the jump decision (rates, waiting
// times, first minimum: the same device functions the elementwise kernels call), the commit (successor selection,
// momentum refresh, counters, dwelling times, the sample ring).  The leapfrog arithmetic is in the reference's literal
// operation order (hmc_state.py:86-100).
//
// Three kinds of sampler run on it.  Host energies drive it from outside, one call per leapfrog step, with the caller's
// E and dE/dX (host_energy.hip: the protocol, and the layout of the proposal columns).  With the gradient from a device
// kernel instead of a call-back it serves the built-in elementwise energies when ndims exceeds what the register-resident
// jump kernel holds (> 1024 float64 dims: 64 lanes x 16 elements) -- `wide` samplers (Shape::wide, wide_energy.hip),
// driven by multipass_iterate from mjhmc_iterate.  The reference accepts any ndims (hmc_state.py:86-100 are plain array
// operations); so does the engine, on this slower path.  And it is the float64-state ProductOfT path of pot_rows64.hip:
// what runs where the tile kernels do not, and their bit-for-bit twin in the tests.
#include <hip/hip_runtime.h>

#include <array>
#include <cmath>
#include <cstring>
#include <vector>

#include "jump_process.hpp"  // decide / decide_ct in their one-lane forms
#include "multipass.hpp"
#include "sampler_internal.hpp"

namespace {

__global__ void hk_copy_rows(double* __restrict__ dst, const double* __restrict__ src, const int* __restrict__ idx,
                             int64_t nrows, int pitch, double sign) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nrows * pitch) return;
  const int64_t r = i / pitch;
  const int d = (int)(i - r * pitch);
  const int64_t sr = idx ? idx[r] : r;
  dst[i] = sign * src[sr * pitch + d];
}

// y += a * x, product rounded before the sum (the library is built with -ffp-contract=off): NumPy's V += c * g
__global__ void hk_axpy(double* __restrict__ y, const double* __restrict__ x, double a, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = y[i] + a * x[i];
}

// (D, n) float64 row-major in `stage`  ->  rows [n][pitch]
__global__ void hk_to_rows(const double* __restrict__ stage, double* __restrict__ dst, int D, int64_t n, int pitch) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * D) return;
  const int d = (int)(i / n);
  const int64_t r = i - (int64_t)d * n;
  dst[r * pitch + d] = stage[i];
}

// out[r] = sum_d V[r][d]^2 / 2 : one wavefront per row (np.sum(V * V, axis=0) / 2., hmc_state.py:74-78)
__global__ void hk_kinetic(const double* __restrict__ V, double* __restrict__ out, int64_t nrows, int D, int pitch) {
  const int64_t r = blockIdx.x;
  if (r >= nrows) return;
  double s = 0.0;
  for (int d = threadIdx.x; d < D; d += 64) {
    const double v = V[r * pitch + d];
    s += v * v;
  }
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (threadIdx.x == 0) out[r] = s / 2.0;
}

// tick-0 normals: the initial momentum (hmc_state.py:24-26), as mjhmc_eval_kernel draws it
__global__ void hk_gen_v(double* __restrict__ V, RngKey key, int64_t first_pid, int64_t N, int D, int pitch) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int pairs = (D + 1) / 2;
  if (i >= N * pairs) return;
  const int64_t p = i / pairs;
  const int pr = (int)(i - p * pairs);
  double z0, z1;
  normal_pair(key, (uint32_t)(first_pid + p), (uint32_t)pr, z0, z1);
  V[p * pitch + 2 * pr] = z0;
  if (2 * pr + 1 < D) V[p * pitch + 2 * pr + 1] = z1;
}

struct DecideArgs {
  const double* EX;
  const double* EV;
  const double* Hflf;
  const double* E;    // proposals
  const double* EVw;
  const int* coldpos;
  int* kmove;
  double* dtmp;
  double* hnew;
  const double* rexp;
  const double* runif;
  Control* ctl;
  int64_t N, Npad, first_pid;
  double p_r, p_flip;
  int mode;
  RngKey key;
};

// one thread per particle: the jump decision, with the device functions of the elementwise kernels (one lane per
// particle: their serial forms)
template <bool REPLAY>
__global__ void hk_decide(const DecideArgs a) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.N) return;
  const uint32_t pid = (uint32_t)(a.first_pid + p);
  const double EX0 = a.EX[p], EV0 = a.EV[p];
  const double H0 = EX0 + EV0;
  const double EXL = a.E[p], EVL = a.EVw[p];
  const double HL = EXL + EVL;
  JumpArgs<double> ja;
  ja.p_r = a.p_r;
  ja.p_flip = a.p_flip;
  ja.rexp = a.rexp;
  ja.runif = a.runif;
  ja.N = a.N;
  const LaneMap m = LaneMap::one_lane();
  int k = 0;
  double dwell = 0.0;
  bool bad = false;
  double EXn = EX0, EVn = EV0, Hc = __builtin_nan("");
  if (a.mode == kModeMJHMC) {
    const double hc = a.Hflf[p];
    double Hf = hc;
    if (!(hc == hc)) {
      const int j = a.coldpos[p];
      Hf = a.E[a.N + j] + a.EVw[a.N + j];
    }
    decide<double, REPLAY>(ja, a.key, m, H0, HL, Hf, p, pid, k, dwell, bad);
    if (k == 0) {  // L accepted: the pre-move state becomes the cached inverse-L state (markov_jump_hmc.py:399-404)
      EXn = EXL;
      EVn = EVL;
      Hc = H0;
    }
  } else if (a.mode == kModeCT) {
    decide_ct<double, REPLAY>(ja, a.key, m, H0, HL, p, pid, k, dwell, bad);
    if (k == 0) {
      EXn = EXL;
      EVn = EVL;
    }
  } else {  // markov_jump_hmc.py:116-148
    double uacc, uflip, ugate;
    if constexpr (REPLAY) {
      uacc = a.runif[p];
      uflip = a.runif[a.N + p];
      ugate = a.runif[2 * a.N];
    } else {
      const u32x4 q = philox4x32_10(pid, a.key.tick_lo, a.key.tick_hi, kSlotExpR, a.key.k0, a.key.k1);
      const u32x4 f = philox4x32_10(pid, a.key.tick_lo, a.key.tick_hi, kSlotFlip, a.key.k0, a.key.k1);
      const u32x4 g = philox4x32_10(0xFFFFFFFFu, a.key.tick_lo, a.key.tick_hi, kSlotFlip, a.key.k0, a.key.k1);
      uacc = u53(q.w2, q.w3);
      uflip = u53(f.w0, f.w1);
      ugate = u53(g.w2, g.w3);
    }
    const double dH = H0 - HL;
    const bool accept = !(dH < 0.0) || (uacc < exp(dH));
    const bool flip = uflip < a.p_flip;
    const bool gate = ugate < a.p_r;
    k = (accept ? 1 : 0) | (flip ? 2 : 0) | (gate ? 4 : 0);
    if (accept) {
      EXn = EXL;
      EVn = EVL;
    }
  }
  if (bad) a.ctl->failed = 1;
  a.kmove[p] = k;
  a.dtmp[p] = dwell;
  a.hnew[p] = EXn;
  a.hnew[a.Npad + p] = EVn;
  a.hnew[2 * a.Npad + p] = Hc;
}

struct CommitArgs {
  double* X;
  double* V;
  double* G;
  double* EXs;
  double* EVs;
  double* Hflf;
  double* TX;     // in: the proposal's end point; out: the pre-move rows (what mjhmc_rollback puts back)
  double* TV;
  double* TG;
  const int* kmove;
  const double* dtmp;
  double* hnew;   // in: EX, EV, H_flf of the successor; out: the pre-move values
  const double* noise;  // replay normals (rows) or nullptr
  double* dwell;
  double* dwell_ring;
  uint8_t* trans;
  double* ring_slot;  // X snapshot target or nullptr
  unsigned long long* stats;
  int64_t N, Npad, first_pid;
  int D, pitch, mode;
  int round32;    // the state is float32-valued (Shape::round32): successors are rounded as they are written
  double r_keep, r_mix;
  RngKey key;
};

// one wavefront per particle: successor state (markov_jump_hmc.py:399-410 / 138-141 / 277-286), momentum refresh
// (hmc_state.py:121-129), bookkeeping
template <bool REPLAY>
__global__ void hk_commit(const CommitArgs a) {
  const int64_t p = blockIdx.x;
  if (p >= a.N) return;
  const int lane = threadIdx.x;
  const int km = a.kmove[p];
  const uint32_t pid = (uint32_t)(a.first_pid + p);
  double* x = a.X + p * a.pitch;
  double* v = a.V + p * a.pitch;
  double* g = a.G + p * a.pitch;
  bool take = false, flip_old = false, flip_new = false, refresh = false;
  int n0 = 0, n1 = 0, n2 = 0, n3 = 0, k = km;
  if (a.mode == kModeMJHMC) {
    take = km == 0;
    flip_old = km == 1;
    refresh = km == 2;
    n0 = km == 0;
    n1 = km == 1;
    n2 = km == 2;
  } else if (a.mode == kModeCT) {  // FL: leap, then flip (:258,278)
    take = km == 0;
    flip_new = km == 0;
    flip_old = km == 1;
    refresh = km == 2;
    n0 = km == 0;
    n1 = km == 1;
    n2 = km == 2;
  } else {
    const bool accept = km & 1, flip = km & 2, gate = km & 4;
    take = accept;
    flip_new = accept != flip;   // accepted L F, then possibly F again
    flip_old = !accept && flip;
    refresh = gate;
    k = km & 3;
    n0 = k == 3;
    n1 = k == 2;
    n2 = gate;
    n3 = k == 1;
  }
  double* tx = a.TX + p * a.pitch;
  double* tv = a.TV + p * a.pitch;
  double* tg = a.TG + p * a.pitch;
  double ev = 0.0;
  for (int d = lane; d < a.D; d += 64) {
    const double x0 = x[d], v0 = v[d], g0 = g[d];
    double xv = x0, vv = v0;
    if (take) {
      xv = tx[d];
      vv = tv[d];
      g[d] = tg[d];
      x[d] = xv;
      if (flip_new) vv = -vv;
    } else if (flip_old) {
      vv = -vv;
    }
    if (refresh) {
      double z;
      if constexpr (REPLAY) {
        z = a.noise[p * a.pitch + d];
      } else {
        double z0, z1;
        normal_pair(a.key, pid, (uint32_t)(d >> 1), z0, z1);
        z = (d & 1) ? z1 : z0;
      }
      vv = vv * a.r_keep + z * a.r_mix;
      if (a.round32) vv = (double)(float)vv;
      ev += vv * vv;
    }
    if (a.round32) {
      xv = (double)(float)xv;
      vv = (double)(float)vv;
      if (take) x[d] = xv;
    }
    v[d] = vv;
    if (a.ring_slot) a.ring_slot[p * a.pitch + d] = xv;
    // the proposal rows are spent: they now keep the pre-move state, so that a committed single iteration can be undone
    // without a copy having been taken (mjhmc_rollback; sharded runs whose failure happened on another rank)
    tx[d] = x0;
    tv[d] = v0;
    tg[d] = g0;
  }
  if (refresh) {
    for (int o = 32; o > 0; o >>= 1) ev += __shfl_xor(ev, o);
  }
  if (lane == 0) {
    const double ex_old = a.EXs[p], ev_old = a.EVs[p], hf_old = a.Hflf[p];
    a.EXs[p] = a.hnew[p];
    a.EVs[p] = refresh ? ev / 2.0 : a.hnew[a.Npad + p];
    a.Hflf[p] = a.hnew[2 * a.Npad + p];
    a.hnew[p] = ex_old;
    a.hnew[a.Npad + p] = ev_old;
    a.hnew[2 * a.Npad + p] = hf_old;
    a.dwell[p] = a.dtmp[p];
    if (a.dwell_ring) a.dwell_ring[p] = a.dtmp[p];
    a.trans[p] = (uint8_t)k;
    if (n0) atomicAdd(&a.stats[0], 1ull);
    if (n1) atomicAdd(&a.stats[1], 1ull);
    if (n2) atomicAdd(&a.stats[2], 1ull);
    if (n3) atomicAdd(&a.stats[3], 1ull);
  }
}

// mjhmc_rollback of a multi-pass sampler: the pre-move rows and scalars hk_commit left in the proposal workspace go back
__global__ void hk_undo(double* __restrict__ X, double* __restrict__ V, double* __restrict__ G, double* __restrict__ EX,
                        double* __restrict__ EV, double* __restrict__ Hflf, const double* __restrict__ TX,
                        const double* __restrict__ TV, const double* __restrict__ TG, const double* __restrict__ hold,
                        int64_t N, int64_t Npad, int D, int pitch) {
  const int64_t p = blockIdx.x;
  if (p >= N) return;
  for (int d = threadIdx.x; d < D; d += 64) {
    X[p * pitch + d] = TX[p * pitch + d];
    V[p * pitch + d] = TV[p * pitch + d];
    G[p * pitch + d] = TG[p * pitch + d];
  }
  if (threadIdx.x == 0) {
    EX[p] = hold[p];
    EV[p] = hold[Npad + p];
    Hflf[p] = hold[2 * Npad + p];
  }
}

// ---- the workspace's device buffers: ONE table, which allocation and release both walk -------------------------------
struct RowsBuf { void** slot; size_t bytes; bool zeroed; };   // zeroed when allocated: the proposal columns' padding is read
constexpr int kRowsBufs = 11;   // the last one, the replay normals, is allocated by the first replayed attempt

std::array<RowsBuf, kRowsBufs> rows_bufs(ProposalRows* t, const mjhmc_sampler* s) {
  const size_t Np = (size_t)s->Npad, rows = 2 * Np, mb = rows * s->sh.pitch * sizeof(double);
  return {{{(void**)&t->X, mb, true},
           {(void**)&t->V, mb, true},
           {(void**)&t->G, mb, true},
           {(void**)&t->E, rows * sizeof(double), false},
           {(void**)&t->EVw, rows * sizeof(double), false},
           {(void**)&t->cold, Np * sizeof(int), false},
           {(void**)&t->coldpos, Np * sizeof(int), false},
           {(void**)&t->kmove, Np * sizeof(int), false},
           {(void**)&t->dtmp, Np * sizeof(double), false},
           {(void**)&t->hnew, 3 * Np * sizeof(double), false},
           {(void**)&t->noise, Np * s->sh.pitch * sizeof(double), false}}};
}

int rows_buf_ensure(const RowsBuf& b, hipStream_t st) {
  if (*b.slot) return 0;
  HIPCHK(hipMalloc(b.slot, b.bytes));
  if (b.zeroed) HIPCHK(hipMemsetAsync(*b.slot, 0, b.bytes, st));
  return 0;
}

int need_rows(mjhmc_sampler* s) {
  if (s->prop) return 0;
  s->prop = new ProposalRows();
  const auto bufs = rows_bufs(s->prop, s);
  for (int i = 0; i + 1 < kRowsBufs; ++i) TRY(rows_buf_ensure(bufs[i], s->stream));
  return 0;
}

}  // namespace

void proposal_rows_free(mjhmc_sampler* s) {
  if (!s->prop) return;
  for (const RowsBuf& b : rows_bufs(s->prop, s))
    if (*b.slot) (void)hipFree(*b.slot);
  delete s->prop;   // (its float32 row set releases itself)
  s->prop = nullptr;
}

void rows_axpy(hipStream_t st, double* y, const double* x, double a, int64_t n) {
  hipLaunchKernelGGL(hk_axpy, grid1(n), dim3(256), 0, st, y, x, a, n);
}
void rows_kinetic(hipStream_t st, const double* V, double* out, int64_t nrows, int D, int pitch) {
  hipLaunchKernelGGL(hk_kinetic, dim3((unsigned)nrows), dim3(64), 0, st, V, out, nrows, D, pitch);
}
void rows_gen_v(hipStream_t st, double* V, RngKey key, int64_t first_pid, int64_t N, int D, int pitch) {
  hipLaunchKernelGGL(hk_gen_v, grid1(N * ((D + 1) / 2)), dim3(256), 0, st, V, key, first_pid, N, D, pitch);
}

int upload_rows(mjhmc_sampler* s, const double* host, int64_t n, double* dst) {
  TRY(ensure_stage(s, (size_t)s->D * n));
  HIPCHK(hipMemcpyAsync(s->stage, host, (size_t)s->D * n * sizeof(double), hipMemcpyHostToDevice, s->stream));
  hipLaunchKernelGGL(hk_to_rows, grid1((int64_t)s->D * n), dim3(256), 0, s->stream, s->stage, dst, s->D, n, s->sh.pitch);
  HIPCHK(hipGetLastError());
  return 0;
}

int traj_begin_impl(mjhmc_sampler* s, int64_t* n_cols) {
  TRY(need_rows(s));
  s->undo_valid = false;   // the workspace is about to be overwritten
  ProposalRows* t = s->prop;
  const int pitch = s->sh.pitch;
  t->n_cold = 0;
  if (s->mode == MJHMC_MODE_MJHMC) {  // the cold list on the host, ascending (the order of NumPy's boolean mask)
    std::vector<double> h((size_t)s->N);
    HIPCHK(hipMemcpyAsync(h.data(), s->Hflf[s->scur], (size_t)s->N * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    std::vector<int> cold, pos((size_t)s->N, -1);
    for (int64_t p = 0; p < s->N; ++p)
      if (!(h[(size_t)p] == h[(size_t)p])) {
        pos[(size_t)p] = (int)cold.size();
        cold.push_back((int)p);
      }
    t->n_cold = (int)cold.size();
    if (t->n_cold) HIPCHK(hipMemcpyAsync(t->cold, cold.data(), cold.size() * sizeof(int), hipMemcpyHostToDevice, s->stream));
    HIPCHK(hipMemcpyAsync(t->coldpos, pos.data(), pos.size() * sizeof(int), hipMemcpyHostToDevice, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));  // the vectors go out of scope
  }
  const double* X = (const double*)s->Xcur;
  const double* V = (const double*)s->Vbuf[s->vcur];
  const double* G = (const double*)s->Gbuf[s->vcur];
  const int64_t n1 = s->N * pitch;
  hipLaunchKernelGGL(hk_copy_rows, grid1(n1), dim3(256), 0, s->stream, t->X, X, (const int*)nullptr, s->N, pitch, 1.0);
  hipLaunchKernelGGL(hk_copy_rows, grid1(n1), dim3(256), 0, s->stream, t->V, V, (const int*)nullptr, s->N, pitch, 1.0);
  hipLaunchKernelGGL(hk_copy_rows, grid1(n1), dim3(256), 0, s->stream, t->G, G, (const int*)nullptr, s->N, pitch, 1.0);
  if (t->n_cold) {
    const int64_t n2 = (int64_t)t->n_cold * pitch;
    const size_t off = (size_t)s->N * pitch;
    hipLaunchKernelGGL(hk_copy_rows, grid1(n2), dim3(256), 0, s->stream, t->X + off, X, (const int*)t->cold, (int64_t)t->n_cold, pitch, 1.0);
    hipLaunchKernelGGL(hk_copy_rows, grid1(n2), dim3(256), 0, s->stream, t->V + off, V, (const int*)t->cold, (int64_t)t->n_cold, pitch, -1.0);
    hipLaunchKernelGGL(hk_copy_rows, grid1(n2), dim3(256), 0, s->stream, t->G + off, G, (const int*)t->cold, (int64_t)t->n_cold, pitch, 1.0);
  }
  HIPCHK(hipGetLastError());
  t->n_cols = s->N + t->n_cold;
  t->phase = 1;
  t->steps = 0;
  if (n_cols) *n_cols = t->n_cols;
  return 0;
}

int traj_advance(mjhmc_sampler* s, bool closing_kick, bool last) {
  ProposalRows* t = s->prop;
  const int64_t ne = t->n_cols * s->sh.pitch;
  const double c = -s->eps / 2.;  // hmc_state.py:88
  if (closing_kick) rows_axpy(s->stream, t->V, t->G, c, ne);   // closes the step the gradient was evaluated for
  if (!last) {
    rows_axpy(s->stream, t->V, t->G, c, ne);
    rows_axpy(s->stream, t->X, t->V, s->eps, ne);
  }
  HIPCHK(hipGetLastError());
  if (!last) t->steps += 1;
  return 0;
}

// the recorded draws of a replayed attempt: normals as rows of the workspace, exponentials / uniforms as they are
static int upload_replay(mjhmc_sampler* s, const double* normal, const double* rexp, const double* runif) {
  TRY(rows_buf_ensure(rows_bufs(s->prop, s).back(), s->stream));
  TRY(upload_rows(s, normal, s->N, s->prop->noise));
  if (rexp) {
    if (!s->rexp) HIPCHK(hipMalloc((void**)&s->rexp, 3 * s->N * sizeof(double)));
    HIPCHK(hipMemcpyAsync(s->rexp, rexp, 3 * s->N * sizeof(double), hipMemcpyHostToDevice, s->stream));
  }
  if (runif) {
    if (!s->runif) HIPCHK(hipMalloc((void**)&s->runif, (2 * s->N + 1) * sizeof(double)));
    HIPCHK(hipMemcpyAsync(s->runif, runif, (2 * s->N + 1) * sizeof(double), hipMemcpyHostToDevice, s->stream));
  }
  return 0;
}

static DecideArgs decide_args(const mjhmc_sampler* s, bool replay, const RngKey& key) {
  const ProposalRows* t = s->prop;
  DecideArgs d;
  d.EX = (const double*)s->EX[s->scur];
  d.EV = (const double*)s->EV[s->scur];
  d.Hflf = (const double*)s->Hflf[s->scur];
  d.E = t->E;
  d.EVw = t->EVw;
  d.coldpos = t->coldpos;
  d.kmove = t->kmove;
  d.dtmp = t->dtmp;
  d.hnew = t->hnew;
  d.rexp = replay ? s->rexp : nullptr;
  d.runif = replay ? s->runif : nullptr;
  d.ctl = s->ctl;
  d.N = s->N; d.Npad = s->Npad; d.first_pid = s->first_pid;
  d.p_r = s->p_r; d.p_flip = s->p_flip;
  d.mode = s->mode;
  d.key = key;
  return d;
}

static CommitArgs commit_args(const mjhmc_sampler* s, bool replay, const RngKey& key, int ring_slot) {
  const ProposalRows* t = s->prop;
  CommitArgs c;
  c.X = (double*)s->Xcur;
  c.V = (double*)s->Vbuf[s->vcur];
  c.G = (double*)s->Gbuf[s->vcur];
  c.EXs = (double*)s->EX[s->scur];
  c.EVs = (double*)s->EV[s->scur];
  c.Hflf = (double*)s->Hflf[s->scur];
  c.TX = t->X;
  c.TV = t->V;
  c.TG = t->G;
  c.kmove = t->kmove;
  c.dtmp = t->dtmp;
  c.hnew = t->hnew;
  c.noise = replay ? t->noise : nullptr;
  c.dwell = s->dwell;
  c.dwell_ring = ring_slot >= 0 ? s->dwell_ring + (size_t)ring_slot * s->Npad : nullptr;
  c.trans = s->trans;
  c.ring_slot = ring_slot >= 0 ? (double*)((char*)s->ring + (size_t)ring_slot * mat_bytes(s)) : nullptr;
  c.stats = (unsigned long long*)s->stats;
  c.N = s->N; c.Npad = s->Npad; c.first_pid = s->first_pid;
  c.D = s->D; c.pitch = s->sh.pitch; c.mode = s->mode;
  c.round32 = s->sh.round32 ? 1 : 0;
  c.r_keep = std::sqrt(1.0 - s->beta);  // hmc_state.py:125-126
  c.r_mix = std::sqrt(s->beta);
  c.key = key;
  return c;
}

// float32-valued state: E, dE/dX and the kinetic energy are those of what is stored (as the float32 register kernels
// report them); one more evaluation per iteration on this fallback path, not a counted one
static int reevaluate_rounded_state(mjhmc_sampler* s) {
  TRY(wide_eval_rows(s, (const double*)s->Xcur, (double*)s->Gbuf[s->vcur], (double*)s->EX[s->scur], s->N));
  rows_kinetic(s->stream, (const double*)s->Vbuf[s->vcur], (double*)s->EV[s->scur], s->N, s->D, s->sh.pitch);
  HIPCHK(hipGetLastError());
  return 0;
}

static void attempt_stats(const mjhmc_sampler* s, const long long hs[4], bool failed, mjhmc_iter_stats* st) {
  const ProposalRows* t = s->prop;
  std::memset(st, 0, sizeof(*st));
  clocks_to_stats(s->mode, hs, st);
  if (s->mode == MJHMC_MODE_MJHMC) st->n_cold = t->n_cold;
  st->E_evals = t->n_cols;
  st->dEdX_evals = (int64_t)t->steps * t->n_cols;
  st->nonfinite = failed ? 1 : 0;
  st->L_used = t->steps;
  st->eps_used = s->eps;
  st->n_flf_run = st->n_cold;
}

int traj_finish_impl(mjhmc_sampler* s, const double* replay_normal, const double* replay_exp, const double* replay_unif,
                     int ring_slot, mjhmc_iter_stats* st) {
  ProposalRows* t = s->prop;
  const bool replay = s->mode == MJHMC_MODE_CONTROL ? (replay_unif != nullptr) : (replay_exp != nullptr);
  if (replay && !replay_normal) return mjhmc_fail(MJHMC_ERR_INVALID, "replay needs the normals as well");
  rows_kinetic(s->stream, t->V, t->EVw, t->n_cols, s->D, s->sh.pitch);
  if (replay) TRY(upload_replay(s, replay_normal, replay_exp, replay_unif));
  HIPCHK(hipMemsetAsync(s->ctl, 0, sizeof(Control), s->stream));
  HIPCHK(hipMemsetAsync(s->stats, 0, 4 * sizeof(long long), s->stream));
  const RngKey key = rng_key(s, s->tick);
  const DecideArgs d = decide_args(s, replay, key);
  if (replay) hipLaunchKernelGGL(hk_decide<true>, grid1(s->N), dim3(256), 0, s->stream, d);
  else hipLaunchKernelGGL(hk_decide<false>, grid1(s->N), dim3(256), 0, s->stream, d);
  HIPCHK(hipGetLastError());
  Control hc;
  HIPCHK(hipMemcpyAsync(&hc, s->ctl, sizeof(Control), hipMemcpyDeviceToHost, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  s->tick += 1;  // one tick per attempt, committed or not (a retry redraws)
  t->phase = 0;
  long long hs[4] = {0, 0, 0, 0};
  if (!hc.failed) {
    const CommitArgs c = commit_args(s, replay, key, ring_slot);
    if (replay) hipLaunchKernelGGL(hk_commit<true>, dim3((unsigned)s->N), dim3(64), 0, s->stream, c);
    else hipLaunchKernelGGL(hk_commit<false>, dim3((unsigned)s->N), dim3(64), 0, s->stream, c);
    HIPCHK(hipGetLastError());
    if (s->sh.round32 && !s->en->is_host()) TRY(reevaluate_rounded_state(s));
    HIPCHK(hipMemcpyAsync(hs, s->stats, sizeof(hs), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
  }
  // a committed attempt can be undone until the next one begins: hk_commit left the pre-move state in the workspace
  s->undo_valid = !hc.failed;
  s->undo_multipass = true;
  if (st) attempt_stats(s, hs, hc.failed != 0, st);
  return 0;
}

int multipass_rollback(mjhmc_sampler* s) {
  ProposalRows* t = s->prop;
  if (!t) return mjhmc_fail(MJHMC_ERR_INVALID, "nothing to roll back");
  HIPCHK(hipSetDevice(s->ctx->device));   // (a process may hold contexts on several devices)
  hipLaunchKernelGGL(hk_undo, dim3((unsigned)s->N), dim3(64), 0, s->stream, (double*)s->Xcur, (double*)s->Vbuf[s->vcur],
                     (double*)s->Gbuf[s->vcur], (double*)s->EX[s->scur], (double*)s->EV[s->scur], (double*)s->Hflf[s->scur],
                     (const double*)t->X, (const double*)t->V, (const double*)t->G, (const double*)t->hnew, s->N, s->Npad, s->D,
                     s->sh.pitch);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(s->stream));
  return 0;
}

// mjhmc_iterate for a wide sampler: n_iter sampling iterations, each L x (kick, drift, device gradient) over the proposal
// columns in HBM, then decide + commit -- the contract of the schedules of iterate.hip (stops at the first attempt with a non-finite rate)
int multipass_iterate(mjhmc_sampler* s, int n_iter, const double* replay_normal, const double* replay_exp,
                      const double* replay_unif, int ring_slot0, mjhmc_iter_stats* per_iter, int* n_done) {
  const size_t DN = (size_t)s->D * s->N;
  int done = 0;
  if (s->timing_on) HIPCHK(hipEventRecord(s->ev_total[0], s->stream));
  for (int i = 0; i < n_iter; ++i) {
    TRY(traj_begin_impl(s, nullptr));
    ProposalRows* t = s->prop;
    if (s->en->is_pot() && s->L > 0) {
      TRY(pot_trajectory_f64(s));   // fused kick / drift / downcast passes around the float32 force kernel
    } else {
      for (int l = 0; l < s->L; ++l) {
        TRY(traj_advance(s, l > 0, false));
        TRY(wide_eval_rows(s, t->X, t->G, l == s->L - 1 ? t->E : nullptr, t->n_cols));
      }
      TRY(traj_advance(s, s->L > 0, true));
      if (s->L == 0) TRY(wide_eval_rows(s, t->X, nullptr, t->E, t->n_cols));
    }
    t->phase = 2;
    mjhmc_iter_stats st;
    TRY(traj_finish_impl(s, replay_normal ? replay_normal + (size_t)i * DN : nullptr,
                         replay_exp ? replay_exp + (size_t)i * 3 * s->N : nullptr,
                         replay_unif ? replay_unif + (size_t)i * (2 * s->N + 1) : nullptr,
                         ring_slot0 >= 0 ? ring_slot0 + i : -1, &st));
    if (per_iter) per_iter[i] = st;
    if (st.nonfinite) break;
    done += 1;
  }
  if (s->timing_on) HIPCHK(hipEventRecord(s->ev_total[1], s->stream));
  s->undo_valid = (n_iter == 1 && done == 1);   // mjhmc_rollback's contract: the last call was ONE committed iteration
  s->last_jump_launches = std::min(done + 1, n_iter);
  s->timing_pending = s->timing_on;
  if (n_done) *n_done = done;
  return 0;
}
