// Which launch schedule an mjhmc_iterate call takes (iterate.hip runs them).  A pure decision on plain numbers: nothing of
// HIP here, so that tests/schedule_table.cpp compiles it with the host compiler alone (tests/test_schedule_cpu.py).
// How many parts a schedule splits a batch into is NOT decided here: that depends on the device's CU count and stays
// with the schedules that split (iterate_fused_t, iterate_dense_parts).
#pragma once
#include <cstdint>

namespace mjhmc {

enum class Schedule {
  Multipass,    // multipass.hip: state in HBM between the substeps (wide rows; float64 ProductOfT at L = 0)
  Fused,        // iterate_fused_t: launches of up to kMaxFuse iterations of the elementwise energies
  DenseParts,   // iterate_dense_parts: the tile kernels of ProductOfT / SparseImageCode, as free-running parts where that pays
  Compact,      // iterate_compact_t: trajectory launch + jump-process launch, the cold list carried from call to call
  Plain         // iterate_plain_t: one jump launch per iteration (also the replay streams and the user-expression energies)
};

enum class EnergyFamily {
  Dense,      // ProductOfT, the linear models, SparseImageCode: tile kernels
  User,       // user-expression energies (hipRTC-built kernels)
  Gaussian,   // ISO_GAUSS, DIAG_GAUSS
  Rows,       // an elementwise energy whose fused launches run in row form: fused_rows() of iterate.hip says so
  Other       // the remaining elementwise energies and shapes
};

// batches of the non-Gaussian elementwise energies below this many particles run fused (measured on the funnel with a group
// of lanes per particle, tools/sweep_shard_c4.py `fused_groups` / `groups`: at 125 000 particles 0.047 ms per iteration fused,
// 0.051 as trajectory + jump-process launches; at 250 000 0.094 against 0.082).  The funnels themselves no longer come here:
// their float64 rows of 9 ... 32 dims fuse in row form at every size (fused_rows).
constexpr int64_t kFuseBelow = 160000;

struct ScheduleInputs {
  EnergyFamily family = EnergyFamily::Other;
  bool wide = false;         // Shape::wide: rows only the multi-pass path holds -- or float64 ProductOfT
  bool pot64_tile = false;   // float64 ProductOfT within the tile kernels' sizes (not pot_big, not a tall linear model, not round32)
  int64_t N = 0;
  int D = 0, logG = 0;
  bool mjhmc_mode = false;   // MJHMC_MODE_MJHMC (the compacted passes are MarkovJumpHMC's)
  int L = 0, n_iter = 1;
  bool replay = false;       // any replay stream present
  // the test build's switches (always false / unset in the shipped library)
  bool no_fuse = false;           // MJHMC_NO_FUSE
  bool no_compact = false;        // MJHMC_NO_COMPACT
  bool fuse_below_set = false;    // MJHMC_FUSE_BELOW given: its value replaces kFuseBelow and the row form no longer counts
  int64_t fuse_below = kFuseBelow;
  bool pot64_multipass = false;   // MJHMC_POT64_MULTIPASS
};

inline Schedule select_schedule(const ScheduleInputs& in) {
  // ProductOfT with float64 state: the tile kernel with the state streamed through its epilogue (dense_pot64.hip); its
  // multi-pass form (the same arithmetic, bit for bit) serves L = 0 and, in the test build, the A/B switch
  const bool pot64_fused = in.wide && in.pot64_tile && in.L >= 1 && !in.pot64_multipass;
  if (in.wide && !pot64_fused) return Schedule::Multipass;

  const bool dense = in.family == EnergyFamily::Dense, user = in.family == EnergyFamily::User;
  // Fused launches: always for the Gaussian forces (one iteration is HBM-bound), for the other elementwise energies
  // while the batch is small (launch-/latency-bound) -- big batches of those take the compacted passes below instead.
  // (the funnels in row form -- a lane per particle, mjhmc_fused_rows_kernel -- are bound by the vector pipe at any batch size)
  const bool rows = in.family == EnergyFamily::Rows && !in.fuse_below_set;
  const bool fusable = !dense && !user && (in.family == EnergyFamily::Gaussian || rows || in.N < in.fuse_below || in.D <= 4);
  // (Measured in round 6 and dropped: a call of ONE iteration through the fused row kernel too -- the state read and written
  // once with the jump process inside the launch, no second launch, no list scan: 0.346 ms per call against the 0.270 of
  // trajectory launch + jump-process launch at C4's size, equal at N/8.  One wave per SIMD overlaps nothing of a tile's
  // loads and stores with its compute, and a one-iteration launch is nothing but tiles' first and last iterations.)
  if (in.n_iter >= 2 && fusable && !in.replay && !in.no_fuse) return Schedule::Fused;
  if (dense) return Schedule::DenseParts;
  // Several particles per wave and a big batch: the inverse-L trajectory of the cold-cache particles runs in the list's
  // own workgroups of mjhmc_traj_kernel instead of in every wave of the jump kernel that holds a cold particle.
  // (reached from kFuseBelow particles up, or MJHMC_NO_FUSE)
  if (in.mjhmc_mode && !user && !in.replay && in.logG < 6 && in.N >= 16384 && !in.no_compact) return Schedule::Compact;
  return Schedule::Plain;
}

}  // namespace mjhmc
