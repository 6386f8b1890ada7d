// What the host fills in and the kernels read: the sampler modes, the control block and every kernel argument block of the
// elementwise energies and of the dense tile kernels.  Plain structs: host code and hipRTC can both take this header.
#pragma once
#include <stdint.h>

#include "philox.hpp"  // RngKey

namespace mjhmc {

constexpr int kModeMJHMC = 0;    // MarkovJumpHMC.sampling_iteration      (markov_jump_hmc.py:355-415)
constexpr int kModeControl = 1;  // HMCBase / HMC / ControlHMC            (markov_jump_hmc.py:116-148)
constexpr int kModeCT = 2;       // ContinuousTimeHMC.sampling_iteration  (markov_jump_hmc.py:251-290)

struct Control {
  int failed;       // some attempt hit a non-finite rate
  int failed_iter;  // index (within the current mjhmc_iterate call) of that attempt
  int inv_iter;     // fused launches: 0x7fffffff - (first failed attempt), combined with atomicMax (0 = none)
};

// most sampling iterations one fused launch runs per particle (per-iteration tallies live in LDS)
constexpr int kMaxFuse = 64;

// launch_jump_t's A/B flags (JumpArgs::ab): take the generic instance instead of a specialised lane mapping
constexpr int kAbNoBlockDecide = 1, kAbNoWpp = 2, kAbNoQuad = 4, kAbNoRows = 8, kAbNoRelay = 16, kAbForceRelay = 32;

// fused MarkovJumpHMC launches of the energies with a row form run a lane per particle for rows held by 2 or 4 lanes elsewhere
inline bool fused_rows_shape(int mode, int logG, int ab) {
  return mode == kModeMJHMC && (logG == 1 || logG == 2) && !(ab & kAbNoRows);
}

template <typename T>
struct JumpArgs {
  const T* X_in;
  const T* V_in;
  T* X_out;
  T* V_out;
  const T* EX_in;
  const T* EV_in;
  T* EX_out;
  T* EV_out;
  const T* Hflf_in;   // H() of the cached inverse-L state; NaN = cache cold
  T* Hflf_out;
  double* dwell;        // [N]
  double* dwell_ring;   // [Npad] ring slot, or a scratch vector when nothing is recorded
  uint8_t* trans;       // [N]
  const T* noise;       // replay normals, particle-major [N][pitch], or nullptr
  const double* rexp;   // replay unit exponentials [3][N], or nullptr
  const double* runif;  // replay uniforms of the discrete-time samplers [2N+1] (accept, flip, R gate)
  Control* ctl;
  unsigned long long* stats;  // [4]: #L, #F, #R, #cold of this attempt
  int64_t N;
  int64_t Npad;              // rows allocated: N rounded up to a multiple of 64
  int64_t first_pid;
  int D, pitch, CH, logG;
  int L;
  int iter;             // index of this attempt inside the current mjhmc_iterate call
  // FUSED kernels: n_fuse consecutive sampling iterations per particle in one launch, the state staying in
  // registers / LDS between them (iteration it uses RNG tick key.tick + it and stats[4 * it ...]).
  // xiter != nullptr: X after iteration it is also recorded at xiter + it * xiter_stride (ring slots) and
  // its dwelling times at dwell_ring + it * Npad; X_out is then not written (the last slot is the live state).
  int defer_r;          // != 0: R-movers keep their old momentum here (always 0 since round 5: their refresh is the jump-process kernel's)
  int n_fuse;
  int ab;               // host-side launch A/B flags (kAb*): always 0 in the shipped library, set by the test build's switches
  T* xiter;
  size_t xiter_stride;  // elements of T between consecutive ring slots
  int mode;             // kModeMJHMC / kModeControl / kModeCT
  T eps, chalf;         // epsilon and -epsilon/2 (hmc_state.py:88-91)
  T r_keep, r_mix;      // sqrt(1-beta), sqrt(beta) of HMCState.R (hmc_state.py:125-126)
  double p_r, p_flip;
  RngKey key;
};

template <typename T>
struct EvalArgs {
  const T* X;     // [n][pitch]
  T* G;           // [n][pitch] or nullptr
  T* E;           // [n] or nullptr
  T* EV;          // [n] or nullptr (kinetic energy of V when V != nullptr)
  const T* V;     // optional
  T* V_out;       // when non-null: V is GENERATED (tick-0 normals) and written here
  int64_t N;
  int64_t first_pid;
  int D, pitch, CH, logG;
  RngKey key;
};

// stand-alone leapfrog operator (see mjhmc_leap_kernel)
template <typename T>
struct LeapArgs {
  const T* X;      // [n][pitch]
  const T* V;
  T* X_out;        // [n][pitch]
  T* V_out;
  T* G;            // dE/dX at the end point, or nullptr
  T* EX;           // [n] or nullptr
  T* EV;
  int64_t N;
  int D, pitch, CH, logG;
  int L;
  T eps, chalf;
};

// Round 5: a MarkovJumpHMC iteration of a big batch with several particles per wavefront as TWO launches --
// mjhmc_traj_kernel integrates (the L proposal of every particle, and beside it the inverse-L proposal of the listed
// cold-cache particles), mjhmc_decide_kernel runs the jump process (see there).
template <typename T>
struct TrajArgs {
  const T* X_in;      // [Npad][pitch] pre-move state
  const T* V_in;
  T* X_out;           // the end point of L, written for every particle as if the move were taken
  T* V_out;
  T* EX_out;          // [Npad] its energies
  T* EV_out;
  T* Hwork;           // [Npad] H() of the inverse-L proposal F L F, written for the listed particles only
  const int* list;    // the particles with a cold cache
  const int* count;   // how many -- or NULL: n_listed then (a list carried over from the previous call, its length known to the host)
  const Control* ctl;
  int64_t N;
  int D, pitch, CH, logG;
  int L;
  int n_listed;
  int inv_blocks;     // leading workgroups of the grid that walk the list (the rest: one forward slot each)
  int rows;           // energies with a row form: a lane per particle (mjhmc_traj_rows_kernel); 0 = the group form (A/B)
  T eps, chalf;
};

template <typename T>
struct JumpDecideArgs {
  const T* X_in;      // pre-move state: what an F / R mover keeps
  const T* V_in;
  T* X_out;           // in: the L proposal; out: the successor
  T* V_out;
  const T* EX_in;
  const T* EV_in;
  T* EX_out;          // in: energies of the L proposal
  T* EV_out;
  const T* Hflf_in;   // H() of the cached inverse-L state, NaN = cold: then Hwork has it
  const T* Hwork;
  T* Hflf_out;
  double* dwell;
  double* dwell_ring;
  uint8_t* trans;
  int* next_list;     // the next iteration's cold caches: this iteration's F- and R-movers
  int* next_count;
  Control* ctl;
  unsigned long long* stats;   // [4]: #L, #F, #R (the cold tally is the list's length)
  int64_t N;
  int64_t first_pid;
  int D, pitch, CH, logG;
  int iter;
  T r_keep, r_mix;
  double p_r;
  RngKey key;
};

// The argument blocks of the dense tile kernels: ProductOfT (POT; dense_pot.hip, float32 rows; dense_pot64.hip, the
// reference's float64 rows around the float32 force) and SparseImageCode (dense_sic.hip, bfloat16 or float32 rows).  S: the
// type of the stored state rows (and of `noise`, G_in / G_out); H: the per-particle scalars and the step parameters.
// A field a family does not have (G_in / G_out and D: ProductOfT only) is a NoField that
// takes no room, so that every family's block keeps its own layout (the kernels' scalar loads and registers follow it).
struct NoField {};
template <bool HAS, typename F>
struct FieldIfT {
  using type = F;
};
template <typename F>
struct FieldIfT<false, F> {
  using type = NoField;
};
template <bool HAS, typename F>
using FieldIf = typename FieldIfT<HAS, F>::type;

template <typename S, typename H, bool POT>
struct DenseJumpArgs {
  static constexpr bool kPot = POT;
  const S* X_in;
  const S* V_in;
  [[no_unique_address]] FieldIf<POT, const S*> G_in;  // dE/dX at X_in (HMCState.dEdX, hmc_state.py:36-39); float64 rows: float32 values widened (:52-53)
  S* X_out;
  S* V_out;
  [[no_unique_address]] FieldIf<POT, S*> G_out;
  const H* EX_in;
  const H* EV_in;
  const H* Hflf_in;
  H* Hwork;            // [Npad] H of the inverse-L proposal, where this iteration integrates it (the listed particles)
  int* cold_list;      // [Npad] compacted indices of the particles whose inverse-L proposal must be integrated
  int* cold_count;
  int* next_list;      // the NEXT iteration's list and counter, filled by this iteration's jump and fix kernels
  int* next_count;
  int* zero_count;     // the counter of the list two iterations back (consumed): cleared by the jump kernel for its next use
  int rescan;          // host side: build this iteration's list by a scan even if it is not the call's first (test build, MJHMC_NO_FSPEC)
  const H* Hspec_in;   // H of the L proposal of a particle that then moved by F, NaN otherwise (see dense_pot.hip: F-movers)
  H* Hspec_out;
  H* EX_out;
  H* EV_out;
  H* Hflf_out;
  double* dwell;
  double* dwell_ring;
  uint8_t* trans;
  const S* noise;      // replay normals [N][pitch] or nullptr
  const double* rexp;  // replay unit exponentials [3][N] or nullptr
  const double* runif; // replay uniforms of the discrete-time samplers [2N+1] (accept, flip, R gate) or nullptr
  Control* ctl;
  unsigned long long* stats;
  int64_t N, Npad, ntiles, first_pid;
  [[no_unique_address]] FieldIf<POT, int> D;
  int L, iter;         // L >= 1
  int mode;            // kModeMJHMC / kModeControl / kModeCT
  H eps, chalf, r_keep, r_mix;
  double p_r, p_flip;
  RngKey key;
};

// stand-alone leapfrog operator on caller-supplied states (HMCState.leapfrog / L, hmc_state.py:86-100)
template <typename S, bool POT>
struct DenseLeapArgs {
  const S* X;
  const S* V;
  S* X_out;
  S* V_out;
  float* G;        // float32 dE/dX at the end point, or nullptr (SparseImageCode: [n][P * 1024])
  float* EX;       // [n] or nullptr
  float* EV;
  int64_t N, ntiles;
  [[no_unique_address]] FieldIf<POT, int> D;
  int L;
  float eps, chalf;
};

template <typename S, bool POT>
struct DenseEvalArgs {
  const S* X;
  float* G;        // float32 dE/dX or nullptr (SparseImageCode: [Npad][1024])
  float* E;
  float* EV;
  const S* V;
  S* V_gen;
  int64_t N, ntiles, first_pid;
  [[no_unique_address]] FieldIf<POT, int> D;
  RngKey key;
};

struct LaunchShape {
  int E;      // elements per lane (template arg)
  int logG;
  int pitch;
  int CH;
};

// host-visible parameter block; each energy TU turns it into its functor
constexpr int kParamPad = 4096;  // device parameter vectors are zero padded to this many elements

struct EnergyParams {
  int kind;
  int ndims;
  double p[8];           // scalar params
  const void* dev_f64;   // device arrays (already in the state dtype), zero padded to pitch
  const void* dev_f32;
};

}  // namespace mjhmc
