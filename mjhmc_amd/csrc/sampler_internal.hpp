// What the translation units of the sampler share: api.hip (handles, hyper-parameters, checkpoints), iterate.hip (the
// launch schedules of mjhmc_iterate, the streamed download), state_io.hip (re-tiling, host copies, evaluation, read /
// write, the one-off operators) and ring.hip (the sample ring's readers).
#pragma once
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>

#include "handles.hpp"
#include "ring_source.hpp"

static inline int fail(int code, const std::string& msg) { return mjhmc_fail(code, msg); }
const std::string& last_error_text();   // api.hip: the calling thread's message (what a worker thread hands to its caller)

// The A/B switches of the measurement tools and of the launch-strategy tests (MJHMC_NO_FUSE, MJHMC_NO_COMPACT,
// MJHMC_NO_SPLIT, MJHMC_SPLIT_PARTS, MJHMC_NO_FSPEC, MJHMC_NO_ROWS, MJHMC_NO_LIST_CARRY, MJHMC_FUSE_BELOW, MJHMC_NO_BLOCK_DECIDE, MJHMC_NO_WPP, MJHMC_NO_QUAD, MJHMC_CHUNKS_PER_LANE,
// MJHMC_SIC_COPIES) and the failure-placing hook MJHMC_DEBUG_POISON exist only in libmjhmc_hip_test.so (built with
// -DMJHMC_TEST_HOOKS, `make test_hooks`).  The shipped library consults no environment variable on the sampling path:
// the only ones it reads at all name libraries to dlopen (MJHMC_RCCL_LIB; hipRTC / hipFFT by their sonames).
// (internal linkage: a unit built without the define must never lend its empty form to one built with it -- every unit
// that calls this is in the Makefile's HOOKS_SRCS, tests/test_hooks_wiring_cpu.py)
#ifdef MJHMC_TEST_HOOKS
static inline const char* test_env(const char* name) { return std::getenv(name); }
#else
static inline const char* test_env(const char*) { return nullptr; }
#endif

// ---------------------------------------------------------------------------------------------
// dispatch over the elementwise energies
// ---------------------------------------------------------------------------------------------
// the launchers of one elementwise energy (launchers.hpp: MJHMC_DEFINE_ENERGY_LAUNCHERS), overloaded on the argument block
#define MJHMC_ENERGY_LAUNCHERS(NAME)                                               \
  struct NAME##_launchers {                                                        \
    template <class... A> static void jump(const A&... a) { NAME##_jump(a...); }  \
    template <class... A> static void leap(const A&... a) { NAME##_leap(a...); }  \
    template <class... A> static void step(const A&... a) { NAME##_step(a...); }  \
    template <class... A> static void eval(const A&... a) { NAME##_eval(a...); }  \
  };
MJHMC_ENERGY_LAUNCHERS(iso)
MJHMC_ENERGY_LAUNCHERS(diag)
MJHMC_ENERGY_LAUNCHERS(rough)
MJHMC_ENERGY_LAUNCHERS(mm)
MJHMC_ENERGY_LAUNCHERS(funnel_neal)
MJHMC_ENERGY_LAUNCHERS(funnel_ref)
#undef MJHMC_ENERGY_LAUNCHERS

// launch(en) with the launchers of energy `kind`, e.g. with_elementwise_energy(kind, [&](auto en) { en.jump(a, ep, E, st); })
template <class F>
static int with_elementwise_energy(int kind, F&& launch) {
  switch (kind) {
    case MJHMC_E_ISO_GAUSS: launch(iso_launchers{}); return 0;
    case MJHMC_E_DIAG_GAUSS: launch(diag_launchers{}); return 0;
    case MJHMC_E_ROUGH_WELL: launch(rough_launchers{}); return 0;
    case MJHMC_E_MM_GAUSS: launch(mm_launchers{}); return 0;
    case MJHMC_E_FUNNEL_NEAL: launch(funnel_neal_launchers{}); return 0;
    case MJHMC_E_FUNNEL_REF: launch(funnel_ref_launchers{}); return 0;
    default: return fail(MJHMC_ERR_UNSUPPORTED, "energy kind has no elementwise kernels");
  }
}

// the Philox key of RNG tick `tick` (tick 0: the initial momenta of an evaluation)
static inline RngKey rng_key(const mjhmc_sampler* s, uint64_t tick) {
  return RngKey{(uint32_t)(s->seed & 0xFFFFFFFFu), (uint32_t)(s->seed >> 32), (uint32_t)(tick & 0xFFFFFFFFu),
                (uint32_t)(tick >> 32)};
}

// the clocks of one attempt from its four device tallies: L, F, R of MarkovJumpHMC; FL, F, R of ContinuousTimeHMC
// (markov_jump_hmc.py:288-290); L, F, R, FL of the discrete-time samplers (markov_jump_hmc.py:138-148).  What MarkovJumpHMC
// keeps in the fourth tally is its caller's (iterate.hip: fill_iter_stats)
static inline void clocks_to_stats(int mode, const long long hs[4], mjhmc_iter_stats* st) {
  (mode == MJHMC_MODE_CTHMC ? st->fl : st->l) = hs[0];
  st->f = hs[1];
  st->r = hs[2];
  if (mode != MJHMC_MODE_MJHMC && mode != MJHMC_MODE_CTHMC) st->fl = hs[3];
}

// ---------------------------------------------------------------------------------------------
// api.hip
// ---------------------------------------------------------------------------------------------
// the dtype a caller asks for against the energy: what mjhmc_sampler_create, mjhmc_eval and mjhmc_leapfrog refuse alike
int check_state_dtype(const mjhmc_energy* e, int dtype);
// row layout and path of a sampler (or of a one-off evaluation) of energy e with state dtype `dtype`.  On return *dtype is
// the dtype the state is STORED in (float64 where float32 was asked for rows only the multi-pass path handles: sh->round32)
int shape_for(const mjhmc_energy* e, int* dtype, Shape* sh);
// An F-mover's H(L proposal) stands in for the H of its inverse-L proposal in the next iteration (dense_pot.hip).  That
// holds for the state and the trajectory it was computed with: anything that changes either -- the step size or count,
// a state or cache write from the host, reset_flf_cache, a restore -- drops it (all NaN: every cold particle integrates).
int drop_spec(mjhmc_sampler* s);
// The "live state" of a sampler: X, V, EX, EV, H_flf, dwell and -- with_dEdX -- dE/dX of the current parities, with
// their sizes in bytes; returns how many entries (6 or 7).  Whether dE/dX belongs to it is the caller's rule and the
// rules differ: a checkpoint keeps it for every sampler that stores it (ProductOfT, host energies, wide rows), the split
// schedule's own copy for ProductOfT alone (the only such sampler it runs).
int live_state(const mjhmc_sampler* s, bool with_dEdX, void* ptrs[7], size_t sizes[7]);

// ---------------------------------------------------------------------------------------------
// iterate.hip
// ---------------------------------------------------------------------------------------------
int ensure_call_block(mjhmc_sampler* s, int rows);

// ---------------------------------------------------------------------------------------------
// state_io.hip
// ---------------------------------------------------------------------------------------------
// host (D, N) float64 -> device particle-major matrix `dst` (stream ordered)
int upload_matrix(mjhmc_sampler* s, const double* host, void* dst);
// dst[d*rs + k*cs + off] = row(k)[d] of `ncols` particle-major rows of element type `elem` (an MJHMC_F64 / _F32 / _BF16
// code: the state's, or MJHMC_F32 for the float32 dE/dX of SparseImageCode), row(k) = idx ? idx[k] : k
int launch_to_dim_major(hipStream_t st, int elem, const void* src, const int64_t* idx, double* dst, int D, int64_t ncols,
                        int pitch, int64_t rs, int64_t cs, int64_t off);
// N per-particle scalars of the state's type -> N float64 on the host (synchronises)
int read_vec(mjhmc_sampler* s, const void* dev, void* host, size_t nbytes);
int run_eval(mjhmc_sampler* s, const void* X, void* Gout, void* Eout, const void* V, void* Vgen, void* EVout);
// tiles of a dense launch over particles [0, N) of rows [0, Npad): 32 rows a tile (ProductOfT), whole particles of P
// rows each (SparseImageCode)
static inline int64_t dense_ntiles(const mjhmc_sampler* s, int64_t N, int64_t Npad) {
  if (!s->en->is_sic()) return Npad / 32;
  const int ppt = sic_particles_per_tile(s->en->sic_P);
  return (N + ppt - 1) / ppt;
}

// Device -> pageable host memory, large blocks (the sample ring, a state matrix).  A plain hipMemcpy to pageable memory
// stages through the runtime's own small pinned buffer on one thread (measured 16-25 GB/s of PCIe Gen5's ~55, less on a
// freshly allocated destination whose pages are still to be faulted in).  Here: two pinned buffers of kPipeChunk bytes; the
// DMA of chunk k + 1 runs while kCopyThreads host threads empty chunk k out of its pinned buffer (they also fault the
// destination pages in, in parallel).  sink(chunk_offset, pinned, lo, hi) takes bytes [lo, hi) of the chunk that starts at
// byte chunk_offset of the source; it is called from several threads at once, on disjoint ranges.
constexpr size_t kPipeChunk = (size_t)32 << 20;
constexpr int kCopyThreads = 8;
int ensure_pipe_pair(void* pin[2], hipEvent_t ev[2]);

template <class Sink>
static int pipe_chunks(hipStream_t st, void* const pin[2], const hipEvent_t ev[2], const void* dev_src, size_t bytes,
                       const Sink& sink) {
  const size_t nchunk = (bytes + kPipeChunk - 1) / kPipeChunk;
  auto issue = [&](size_t k) -> int {
    const size_t off = k * kPipeChunk, len = std::min(kPipeChunk, bytes - off);
    HIPCHK(hipMemcpyAsync(pin[k & 1], (const char*)dev_src + off, len, hipMemcpyDeviceToHost, st));
    HIPCHK(hipEventRecord(ev[k & 1], st));
    return 0;
  };
  TRY(issue(0));
  for (size_t k = 0; k < nchunk; ++k) {
    if (k + 1 < nchunk) TRY(issue(k + 1));  // its buffer was emptied by the host copy of chunk k - 1 (joined below)
    HIPCHK(hipEventSynchronize(ev[k & 1]));
    const size_t off = k * kPipeChunk, len = std::min(kPipeChunk, bytes - off);
    const char* src = (const char*)pin[k & 1];
    const size_t slice = (len / kCopyThreads + 4095) / 4096 * 4096;
    std::thread th[kCopyThreads];
    int nth = 0;
    for (size_t o = slice; o < len; o += slice) th[nth++] = std::thread([=, &sink] { sink(off, src, o, std::min(o + slice, len)); });
    sink(off, src, (size_t)0, std::min(slice, len));
    for (int t = 0; t < nth; ++t) th[t].join();
  }
  return 0;
}
