// LambdaDistribution(energy_func, energy_grad_func, init) with OPAQUE Python callables (README.md:27-36,
// mjhmc/misc/distributions.py:198-251): energies the engine has no device form of -- neither a built-in functor nor
// C expressions -- for example a dense quadratic form.  A Python callable cannot run in a kernel, so for these energies
// E and dE/dX are evaluated by the CALLER, once per leapfrog step, and everything else stays on the device: the particle
// state (X, V, dE/dX, EX, EV, the inverse-L cache), the leapfrog arithmetic in the reference's literal operation order
// (hmc_state.py:86-100), the jump decision (rates, waiting times, first minimum: the same device functions the
// elementwise kernels call), the successor selection, momentum refresh, counters, dwelling times and the sample ring.
//
// Protocol of one sampling iteration (include/mjhmc_hip.h: mjhmc_traj_*):
//   traj_begin   proposal columns [0, N): (X, V, dE/dX) of every particle -- the L proposal; MJHMC: columns [N, N + n_cold):
//                (X, -V, dE/dX) of the particles whose inverse-L cache is cold, in ascending particle order -- F L F is
//                read only through H() (markov_jump_hmc.py:360,367)
//   traj_step    [V += (-eps/2) g(caller's gradient at the X handed out last)]; unless last: V += (-eps/2) g; X += eps V; X -> caller
//   traj_finish  caller's E at the end points -> H of the proposals -> decide -> commit (or, on a non-finite rate,
//                nothing: the attempt is not committed, markov_jump_hmc.py:376-389)
// It is slow by construction (a host round trip per leapfrog step).  The passes themselves are the multi-pass engine's
// (multipass.hip); this unit is the caller-driven protocol around them.
#include <hip/hip_runtime.h>

#include "multipass.hpp"
#include "sampler_internal.hpp"

static int check_host(mjhmc_sampler* s) {
  if (!s) return mjhmc_fail(MJHMC_ERR_INVALID, "sampler is NULL");
  if (!s->en->is_host()) return mjhmc_fail(MJHMC_ERR_INVALID, "the sampler's energy is not MJHMC_E_HOST");
  return 0;
}

// run_eval of state_io.hip for a host energy: the kinetic energy of V (or the tick-0 momentum) is device work, E and dE/dX
// are the caller's (mjhmc_host_set_energy)
int host_run_eval(mjhmc_sampler* s, const void* V, void* Vgen, void* EVout) {
  if (Vgen) {
    rows_gen_v(s->stream, (double*)Vgen, rng_key(s, 0), s->first_pid, s->N, s->D, s->sh.pitch);
    HIPCHK(hipGetLastError());
    V = Vgen;
  }
  if (V && EVout) {
    rows_kinetic(s->stream, (const double*)V, (double*)EVout, s->N, s->D, s->sh.pitch);
    HIPCHK(hipGetLastError());
  }
  return 0;
}

extern "C" {

int mjhmc_host_set_energy(mjhmc_sampler* s, const double* E, const double* dEdX) {
  TRY(check_host(s));
  if (!E || !dEdX) return mjhmc_fail(MJHMC_ERR_INVALID, "NULL argument");
  HIPCHK(hipSetDevice(s->ctx->device));
  HIPCHK(hipMemcpyAsync(s->EX[s->scur], E, (size_t)s->N * sizeof(double), hipMemcpyHostToDevice, s->stream));
  TRY(upload_rows(s, dEdX, s->N, (double*)s->Gbuf[s->vcur]));
  HIPCHK(hipStreamSynchronize(s->stream));
  s->host_energy_set = true;
  return 0;
}

int mjhmc_traj_begin(mjhmc_sampler* s, int64_t* n_cols) {
  TRY(check_host(s));
  if (!n_cols) return mjhmc_fail(MJHMC_ERR_INVALID, "n_cols is NULL");
  if (!s->host_energy_set)
    return mjhmc_fail(MJHMC_ERR_INVALID, "E and dE/dX of the current state are unknown: call mjhmc_host_set_energy first");
  HIPCHK(hipSetDevice(s->ctx->device));
  return traj_begin_impl(s, n_cols);
}

int mjhmc_traj_step(mjhmc_sampler* s, const double* grad, int last, double* X_out) {
  TRY(check_host(s));
  ProposalRows* t = s->prop;
  if (!t || t->phase != 1) return mjhmc_fail(MJHMC_ERR_INVALID, "no trajectory in progress (mjhmc_traj_begin)");
  if (!last && !X_out) return mjhmc_fail(MJHMC_ERR_INVALID, "X_out is NULL");
  if (t->steps > 0 && !grad) return mjhmc_fail(MJHMC_ERR_INVALID, "the gradient at the positions handed out last is missing");
  HIPCHK(hipSetDevice(s->ctx->device));
  const int64_t n = t->n_cols;
  if (grad) {  // closes the step the caller evaluated the gradient for
    if (t->steps == 0) return mjhmc_fail(MJHMC_ERR_INVALID, "the first step uses the stored dE/dX: pass NULL");
    TRY(upload_rows(s, grad, n, t->G));
  }
  TRY(traj_advance(s, grad != nullptr, last != 0));
  if (last) {
    t->phase = 2;
    return 0;
  }
  TRY(ensure_stage(s, (size_t)s->D * n));
  return download_cols(s, t->X, nullptr, n, X_out, (size_t)s->D * n, n, 1, 0, true);
}

int mjhmc_traj_finish(mjhmc_sampler* s, const double* E, const double* replay_normal, const double* replay_exp,
                      const double* replay_unif, int ring_slot, mjhmc_iter_stats* st) {
  TRY(check_host(s));
  ProposalRows* t = s->prop;
  if (!t || t->phase != 2) return mjhmc_fail(MJHMC_ERR_INVALID, "the trajectory is not complete (mjhmc_traj_step with last != 0)");
  if (!E) return mjhmc_fail(MJHMC_ERR_INVALID, "E is NULL");
  if (ring_slot >= s->ring_slots) return mjhmc_fail(MJHMC_ERR_INVALID, "ring slot out of range");
  HIPCHK(hipSetDevice(s->ctx->device));
  HIPCHK(hipMemcpyAsync(t->E, E, (size_t)t->n_cols * sizeof(double), hipMemcpyHostToDevice, s->stream));
  return traj_finish_impl(s, replay_normal, replay_exp, replay_unif, ring_slot, st);
}

}  // extern "C"
