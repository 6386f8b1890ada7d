// ProductOfT in the REFERENCE'S arithmetic on the matrix cores: float64 HMCState arrays (hmc_state.py:29-38) integrated
// around a float32 force (distributions.py:398-415: float32 shared variables, allow_input_downcast=True).
//
//   V += (-eps/2) * dEdX ;  X += eps * V ;  dEdX = float64( force32( float32(X) ) ) ;  V += (-eps/2) * dEdX     (hmc_state.py:86-91)
//
// The tile kernel of dense_pot.hip keeps X, V as float32 accumulator tiles in registers.  Here they are float64 tiles in
// registers for the whole trajectory (2 x 128 registers at NB = 4; the GEMMs run with half-chunk A-row sets there to make
// the room: dense_pot_tile.hpp, gemm_dim_half).  After the second GEMM of a gradient the wave walks its accumulator (dE/dX,
// float32) in four chunks of 16 elements per lane: V += c g (twice between two drifts: the closing half kick of a step
// and the opening one of the next are two roundings, as in the reference), X += eps V in float64, and float32(X) goes
// straight into the LDS B-fragment image the first GEMM of the next gradient reads.  dE/dX stays float32 (the reference's
// force output, widened exactly where the reference assigns it into its float64 dEdX array, hmc_state.py:52-53).
//
// The particle rows are read at the start of a trajectory and written at its end only, staged through the idle B-operand
// images in LDS so that those accesses are coalesced (staged_start, staged_end_*); a leapfrog step touches no state in
// memory.  A particle that takes the L move is finished when the trajectory is; one that does not gets its pre-move rows
// copied over at the end.
//
// Same operations in the same order as the multi-pass path this replaces on the sampling path (pot_rows64.hip:
// hk_pot_kick_drift / pot_eval_kernel) and the same GEMM code: results are bit-identical to it
// (tests/test_gpu_dense_parity.py::test_pot64_fused_equals_multipass).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "dense_pot.hpp"
#include "dense_pot64_kernels.hpp"
#include "dense_pot_tile.hpp"

namespace mjhmc {

// ---------------------------------------------------------------------------------------------------
// The inverse-L proposal: which particles integrate it (not the F-movers), its tiles as items of the jump launch, the
// pending particles and the fix kernel -- dense_pot.hip has the story; this is the float64-state twin.
// ---------------------------------------------------------------------------------------------------
__global__ void pot64_cold_list_kernel(const double* __restrict__ Hflf_in, const double* __restrict__ Hspec_in, int64_t N,
                                       int* __restrict__ list, int* __restrict__ count, const Control* ctl) {
  if (ctl->failed) return;
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const double hc = p < N ? Hflf_in[p] : 0.0, hs = p < N ? Hspec_in[p] : 0.0;
  append_cold(list, count, (p < N) && !(hc == hc) && !(hs == hs), p);
}

// ---------------------------------------------------------------------------------------------------
// the jump kernel (dense_pot64_jump.inc): one sampling_iteration attempt for a tile of 32 particles
// (MODE as in pot_jump_kernel), with ProductOfT's experts
// ---------------------------------------------------------------------------------------------------
template <int NB, bool REPLAY, int MODE>
__global__ __launch_bounds__(256, 1) void pot64_jump_kernel(const Pot64JumpArgs a, const PotModel mdl) {
  const PotExperts xp;
#include "dense_pot64_jump.inc"
}

// MarkovJumpHMC's jump process for every particle (markov_jump_hmc.py:366-415), once both trajectories of the iteration
// are done -- the L proposal in the output rows with its energies in EX_out / EV_out, H of the inverse-L proposal cached
// (H_flf), handed on by the F move of the iteration before (Hspec) or integrated by this iteration's launch (Hwork):
// rates, clocks, first minimum, counters, the next iteration's list, and where the move is not L the pre-move position
// and dE/dX put back and the momentum flipped / redrawn (pot_decide_kernel's twin).
template <int NB, bool REPLAY>
__global__ __launch_bounds__(256) void pot64_decide_kernel(const Pot64JumpArgs a) {
  __shared__ Finish64Shared<NB> sh;
  if (a.ctl->failed) return;
  const int w = threadIdx.x >> 6, c = threadIdx.x & 31, h = (threadIdx.x & 63) >> 5;
  unsigned n0 = 0, n1 = 0, n2 = 0, n3 = 0;
  bool any_bad = false;
  for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int64_t p = tile * kP + c;
    const bool alive = p < a.N;
    if (w == 0 && h == 0) {
      const int64_t pp = alive ? p : 0;
      const uint32_t pid = (uint32_t)(a.first_pid + pp);
      const double EX0 = a.EX_in[p], EV0 = a.EV_in[p];
      const double H0 = EX0 + EV0;
      const double HL = a.EX_out[p] + a.EV_out[p];
      double Hflf = a.Hflf_in[p];
      const bool cold = !(Hflf == Hflf);
      if (cold) {
        Hflf = a.Hspec_in[p];                      // the L proposal of the iteration in which the particle flipped ...
        if (!(Hflf == Hflf)) Hflf = a.Hwork[p];    // ... or integrated by an inverse-L item of this iteration's launch
      }
      double best = 0.0;
      bool bad = false, gate = false;
      const int k = pot64_decide<REPLAY, kModeMJHMC>(a, H0, HL, Hflf, pp, pid, best, bad, gate);
      sh.s.move[c] = alive ? k : 0;
      any_bad |= bad && alive;
      // every move but L clears the cache; of those only the R-movers need their inverse-L proposal integrated
      append_cold(a.next_list, a.next_count, alive && k == 2, p);
      a.dwell[p] = best;
      a.dwell_ring[p] = best;
      a.trans[p] = (uint8_t)k;
      if (alive) {
        n0 += (k == 0);
        n1 += (k == 1);
        n2 += (k == 2);
        n3 += cold;   // the reference integrates F L F for every one of these
      }
      if (k != 0) {
        a.EX_out[p] = EX0;
        a.EV_out[p] = EV0;   // (an R-mover's: filled in by pot64_finish)
      }
      a.Hflf_out[p] = k == 0 ? H0 : __builtin_nan("");
      a.Hspec_out[p] = k == 1 ? HL : __builtin_nan("");
    }
    __syncthreads();
    if (__syncthreads_or(sh.s.move[c] != 0)) {   // (a tile of L-movers is finished already)
      const size_t roff = (size_t)p * (128 * NB) + 32 * NB * w + 4 * NB * h;
      VTile<NB> v;   // (unused: FIX)
      Tile<NB> g;
      pot64_finish<NB, REPLAY, kModeMJHMC, true>(a, sh, p, alive, roff, w, c, h, v, g);
      __syncthreads();
    }
  }
  if (any_bad) {
    a.ctl->failed = 1;
    a.ctl->failed_iter = a.iter;
  }
  __shared__ unsigned tally[4];
  if (threadIdx.x < 4) tally[threadIdx.x] = 0;
  __syncthreads();
  if (n0) atomicAdd(&tally[0], n0);
  if (n1) atomicAdd(&tally[1], n1);
  if (n2) atomicAdd(&tally[2], n2);
  if (n3) atomicAdd(&tally[3], n3);
  __syncthreads();
  if (threadIdx.x < 4 && tally[threadIdx.x]) atomicAdd(&a.stats[threadIdx.x], (unsigned long long)tally[threadIdx.x]);
}

static int resident_cus64() {
  int dev = 0, cus = 0;
  (void)hipGetDevice(&dev);
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  return std::max(1, cus);
}

template <int NB, int MODE>
static void launch64_mode(const Pot64JumpArgs& a, const PotModel& mdl, unsigned grid, hipStream_t st, const PotGenerated* gen) {
  const bool replay = MODE == kModeControl ? (a.runif && a.noise) : (a.rexp && a.noise);
  if (gen) pot_launch_generated(gen->jump64[MODE][replay ? 1 : 0], grid, st, a, mdl, gen->lin);
  else if (replay) hipLaunchKernelGGL((pot64_jump_kernel<NB, true, MODE>), dim3(grid), dim3(256), 0, st, a, mdl);
  else hipLaunchKernelGGL((pot64_jump_kernel<NB, false, MODE>), dim3(grid), dim3(256), 0, st, a, mdl);
}

template <int NB>
static void launch64_nb(const Pot64JumpArgs& a, const PotModel& mdl, hipStream_t st, const PotGenerated* gen) {
  const int cus = resident_cus64();
  if (a.mode == kModeMJHMC) {  // only MJHMC has the inverse-L proposal and its cache
    if (a.iter == 0 || a.rescan) {  // first iteration of a call: the three counters cleared (they are adjacent), the list from a scan
      (void)hipMemsetAsync(std::min(a.cold_count, std::min(a.next_count, a.zero_count)), 0, 3 * sizeof(int), st);
      hipLaunchKernelGGL(pot64_cold_list_kernel, dim3((unsigned)((a.N + 255) / 256)), dim3(256), 0, st, a.Hflf_in, a.Hspec_in,
                         a.N, a.cold_list, a.cold_count, (const Control*)a.ctl);
    }
    // forward tiles + at most as many inverse-L tiles (workgroups without an item leave at once)
    const unsigned grid = (unsigned)std::min<int64_t>(2 * a.ntiles, cus);
    launch64_mode<NB, kModeMJHMC>(a, mdl, grid, st, gen);
    const unsigned fgrid = (unsigned)std::min<int64_t>(a.ntiles, 4 * cus);
    if (a.rexp && a.noise) hipLaunchKernelGGL((pot64_decide_kernel<NB, true>), dim3(fgrid), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((pot64_decide_kernel<NB, false>), dim3(fgrid), dim3(256), 0, st, a);
  } else {
    const unsigned grid = (unsigned)std::min<int64_t>(a.ntiles, cus);
    if (a.mode == kModeCT) launch64_mode<NB, kModeCT>(a, mdl, grid, st, gen);
    else launch64_mode<NB, kModeControl>(a, mdl, grid, st, gen);
  }
}

void pot64_launch_jump(const Pot64JumpArgs& a, const PotModel& mdl, hipStream_t st, const PotGenerated* gen) {
  if (mdl.dim == 128) launch64_nb<1>(a, mdl, st, gen);
  else if (mdl.dim == 256) launch64_nb<2>(a, mdl, st, gen);
  else launch64_nb<4>(a, mdl, st, gen);
}

#ifdef POT_STAMPS
}  // namespace mjhmc
extern "C" int mjhmc_pot64_stamps(unsigned long long* out) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(mjhmc::g_pot_stamp), sizeof(mjhmc::g_pot_stamp));
}
extern "C" int mjhmc_pot64_item_stamps(unsigned long long* out) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(mjhmc::g_pot_istamp), sizeof(mjhmc::g_pot_istamp));
}
namespace mjhmc {
#endif

}  // namespace mjhmc
