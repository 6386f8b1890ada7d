// The multi-pass path: what its units share.  multipass.hip is the engine (workspace, kick / drift pass, decide, commit,
// rollback, multipass_iterate); host_energy.hip drives it step by step for opaque callables (mjhmc_traj_*);
// wide_energy.hip holds the built-in elementwise energies on rows of any length; pot_rows64.hip the float64-state rows
// around ProductOfT's float32 force.  What units outside this group call is declared in handles.hpp.
#pragma once
#include "handles.hpp"

// ProductOfT with float64 state: the float32 rows of one force evaluation -- [0] X, [1] dE/dX, [2] E, and [3] the
// u / phi(u) rows of the blocked evaluation (ndims > 512: pot_big()).  pot_rows64.hip
struct PotRows32 {
  float* buf[4] = {nullptr, nullptr, nullptr, nullptr};
  PotRows32() = default;
  PotRows32(const PotRows32&) = delete;
  PotRows32& operator=(const PotRows32&) = delete;
  ~PotRows32() { release(); }
  int ensure(size_t cap_rows, int pitch, bool big);   // allocates once, for cap_rows rows ([3] only when big)
  void release();
};

// proposal workspace of a multi-pass sampler: host energies (mjhmc_traj_*), wide rows, float64 ProductOfT
struct ProposalRows {
  double* X = nullptr;  // [2 Npad][pitch] proposal columns
  double* V = nullptr;
  double* G = nullptr;
  double* E = nullptr;   // [2 Npad] energies at the end points (a host energy: the caller's)
  double* EVw = nullptr; // [2 Npad] kinetic energies of the end points
  int* cold = nullptr;      // [Npad] cold particles, ascending
  int* coldpos = nullptr;   // [Npad] position in `cold`, -1 when the cache is hot
  int* kmove = nullptr;     // [Npad] decision of the attempt
  double* dtmp = nullptr;   // [Npad] dwelling time of the attempt
  double* hnew = nullptr;   // [3 Npad] EX, EV, H_flf of the successor
  double* noise = nullptr;  // [Npad][pitch] replay normals (allocated by the first replayed attempt)
  PotRows32 pot32;          // capacity 2 Npad rows (allocated by the first float32 force evaluation)
  int n_cold = 0;
  int64_t n_cols = 0;
  int phase = 0;  // 0 idle, 1 begun (stepping), 2 last kick done
  int steps = 0;
};

inline dim3 grid1(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }

// what follows is called by the units of this group alone: it stays out of the library's dynamic symbol table
#pragma GCC visibility push(hidden)

// ---- multipass.hip ---------------------------------------------------------------------------------------------------
int traj_begin_impl(mjhmc_sampler* s, int64_t* n_cols);
// one kick / drift pass of the proposal columns: [V += c g_new]; unless last: V += c g; X += eps V; steps += 1
int traj_advance(mjhmc_sampler* s, bool closing_kick, bool last);
// the workspace's E holds the energies of the end points (device): decide + commit
int traj_finish_impl(mjhmc_sampler* s, const double* replay_normal, const double* replay_exp, const double* replay_unif,
                     int ring_slot, mjhmc_iter_stats* st);
// host (D, n) float64 -> n device rows at dst (stream ordered, through s->stage)
int upload_rows(mjhmc_sampler* s, const double* host, int64_t n, double* dst);
// launches of the small row kernels (the caller checks hipGetLastError)
void rows_axpy(hipStream_t st, double* y, const double* x, double a, int64_t n);   // y += a * x
void rows_kinetic(hipStream_t st, const double* V, double* out, int64_t nrows, int D, int pitch);   // out[r] = |V[r]|^2 / 2
void rows_gen_v(hipStream_t st, double* V, RngKey key, int64_t first_pid, int64_t N, int D, int pitch);   // the normals of `key`

// ---- host_energy.hip -------------------------------------------------------------------------------------------------
int host_run_eval(mjhmc_sampler* s, const void* V, void* Vgen, void* EVout);

// ---- wide_energy.hip -------------------------------------------------------------------------------------------------
// E (nrows) and dE/dX (rows) of rows X on the device; either output may be NULL
int wide_eval_rows(mjhmc_sampler* s, const double* X, double* G, double* E, int64_t nrows);

// ---- pot_rows64.hip --------------------------------------------------------------------------------------------------
int pot_eval_rows_f64(mjhmc_sampler* s, const double* X, double* G, double* E, int64_t nrows);
int pot_trajectory_f64(mjhmc_sampler* s);   // the L leapfrog steps of a begun trajectory, and E of its end points

#pragma GCC visibility pop
