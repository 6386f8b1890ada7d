/*
 * mjhmc_hip.h -- C ABI of libmjhmc_hip.so, the MI355X (gfx950) engine for the particle-parallel
 * Markov-Jump-HMC hot path of rueberger/MJHMC.
 *
 * The reference has no FFI: its hot path is NumPy called from Python classes.  Each entry point
 * below replaces the reference interface cited next to it (paths relative to the reference
 * root); a reference maintainer binds them with ctypes.
 *
 * Conventions
 *   - C linkage, plain pointers and sizes.  Return 0 on success, a negative mjhmc_status
 *     otherwise; the message is available from mjhmc_last_error().  Nothing throws across the ABI.
 *   - Every pointer argument is caller-owned HOST memory, valid for the duration of the call.
 *     Matrices are C-ordered (ndims, nparticles) float64 exactly like the reference's arrays
 *     (mjhmc/samplers/markov_jump_hmc.py:29); the engine re-tiles them on the device.
 *   - Device memory is owned by the handles.  One HIP stream per sampler.  A handle is not
 *     thread-safe; distinct handles are independent.  No process-global mutable state except
 *     the last-error string of failed *_create calls (thread-local).
 */
#ifndef MJHMC_HIP_H
#define MJHMC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MJHMC_ABI_VERSION 2

typedef struct mjhmc_ctx mjhmc_ctx;         /* one per process x device                          */
typedef struct mjhmc_energy mjhmc_energy;   /* an energy model, parameters resident in HBM       */
typedef struct mjhmc_sampler mjhmc_sampler; /* particle state (HMCState) + jump-process machinery */
typedef struct mjhmc_comm mjhmc_comm;       /* this rank's end of an RCCL communicator (one process per GPU)     */

typedef enum {
  MJHMC_OK = 0,
  MJHMC_ERR_INVALID = -1,      /* bad argument                                                   */
  MJHMC_ERR_HIP = -2,          /* a HIP runtime call failed                                      */
  MJHMC_ERR_UNSUPPORTED = -3,  /* a dtype that names no arithmetic of the energy (bf16 outside   */
                               /* SPARSE_CODE), a SPARSE_CODE dictionary shape the reference     */
                               /* rejects too; every ndims of the other energies runs            */
  MJHMC_ERR_NO_DEVICE = -4,
  MJHMC_ERR_NONFINITE = -5,    /* informational: see mjhmc_iterate                               */
  MJHMC_ERR_COMM = -6          /* librccl could not be loaded, or an RCCL call failed            */
} mjhmc_status;

/* Energy models.  params are float64; layout per kind:
 *   ISO_GAUSS   {sigma}                         TestGaussian  mjhmc/misc/distributions.py:348-362, README.md:18-24
 *   DIAG_GAUSS  {j_0..j_{D-1}} diagonal of J    Gaussian      mjhmc/misc/distributions.py:256-273
 *   ROUGH_WELL  {scale1, scale2}                RoughWell     mjhmc/misc/distributions.py:283-304
 *   MM_GAUSS    {separation}                    MultimodalGaussian mjhmc/misc/distributions.py:314-335
 *   FUNNEL_NEAL {scale}                         Funnel as documented, mjhmc/misc/tf_distributions.py:142-147
 *   FUNNEL_REF  {scale}                         Funnel as coded,      mjhmc/misc/tf_distributions.py:157-165
 *   PRODUCT_OF_T {nbasis, W[D*nbasis] row-major (D,nbasis), nu[nbasis], b[nbasis]}
 *                                               ProductOfT    mjhmc/misc/distributions.py:373-433
 *                                               (nbasis == ndims, any size: the tile kernels up to 512, 512 x 512
 *                                               blocks on the multi-pass path beyond; dtype F64 = the reference's
 *                                               arithmetic, float64 state around the float32 force; F32 = float32 state)
 *   SPARSE_CODE {n_patches, img, n_coeffs, lambda, cauchy, B[img*n_coeffs], Y[n_patches*img]}
 *                                               SparseImageCode mjhmc/misc/tf_distributions.py:204-272
 *                                               (img = 256; n_coeffs = 1024 or 512, :219; 1 <= n_patches <= 32)
 */
typedef enum {
  MJHMC_E_ISO_GAUSS = 0,
  MJHMC_E_DIAG_GAUSS = 1,
  MJHMC_E_ROUGH_WELL = 2,
  MJHMC_E_MM_GAUSS = 3,
  MJHMC_E_FUNNEL_NEAL = 4,
  MJHMC_E_FUNNEL_REF = 5,
  MJHMC_E_PRODUCT_OF_T = 6,
  MJHMC_E_SPARSE_CODE = 7,
  MJHMC_E_USER_EXPR = 8,     /* created by mjhmc_energy_create_expr only */
  MJHMC_E_HOST = 9,          /* no parameters: E and dE/dX are evaluated by the CALLER (opaque Python callables of
                                LambdaDistribution, README.md:27-36); samplers of it are driven by mjhmc_traj_* below */
  MJHMC_E_LINEAR_EXPR = 10   /* created by mjhmc_energy_create_linear only */
} mjhmc_energy_kind;

/* arithmetic type of state and force.  BF16: bfloat16 state in HBM and as MFMA operands, float32
 * accumulation and integrator registers (SPARSE_CODE only). */
typedef enum { MJHMC_F64 = 0, MJHMC_F32 = 1, MJHMC_BF16 = 2 } mjhmc_dtype;

/* Sampler families (mjhmc/samplers/markov_jump_hmc.py). */
typedef enum {
  MJHMC_MODE_MJHMC = 0,   /* MarkovJumpHMC.sampling_iteration      :355-415 */
  MJHMC_MODE_CONTROL = 1, /* HMCBase / HMC / ControlHMC            :116-148 */
  MJHMC_MODE_CTHMC = 2    /* ContinuousTimeHMC.sampling_iteration  :251-290 */
} mjhmc_mode;

/* State fields (mjhmc/samplers/hmc_state.py:13-44) readable / writable through mjhmc_read/write.
 * Matrix fields are (ndims, nparticles) float64 C-order on the host side. */
typedef enum {
  MJHMC_F_X = 0,      /* HMCState.X                                  float64 (D,N)  rw */
  MJHMC_F_V = 1,      /* HMCState.V                                  float64 (D,N)  rw */
  MJHMC_F_EX = 2,     /* HMCState.EX                                 float64 (N)    r  */
  MJHMC_F_EV = 3,     /* HMCState.EV                                 float64 (N)    r  */
  MJHMC_F_DEDX = 4,   /* HMCState.dEdX (recomputed from X on demand) float64 (D,N)  r  */
  MJHMC_F_HFLF = 5,   /* H() of HMCState.cached_flf_state, NaN where the cache is cold  float64 (N) rw */
  MJHMC_F_CACHE = 6,  /* HMCState.cache_active (== H_flf is not NaN)  uint8   (N)    r  */
  MJHMC_F_DWELL = 7,  /* ContinuousTimeHMC.dwelling_times            float64 (N)    r  */
  MJHMC_F_TRANS = 8   /* argmin row of min_idx (0=L,1=F,2=R; CONTROL: bit0=FL accepted, bit1=flipped) uint8 (N) r */
} mjhmc_field;

/* Integer bookkeeping of one sampling_iteration attempt (bit-exact with the reference):
 * l/f/r/fl follow the sampler's l_count/f_count/r_count/fl_count increments
 * (markov_jump_hmc.py:143-148,288-290,413-415); E_evals/dEdX_evals are the increments of
 * Distribution.E_count / dEdX_count (mjhmc/misc/distributions.py:62-75). */
typedef struct {
  int64_t l, f, r, fl;
  int64_t n_cold;      /* particles with a cold FLF cache: the reference integrates F L F for each of them
                          (hmc_state.py:109-119) and counts the evaluations below                      */
  int64_t E_evals;
  int64_t dEdX_evals;
  int32_t nonfinite;   /* 1: some particle produced a non-finite rate (utils.py:41-48); the attempt
                          was NOT committed, state is as before the attempt                        */
  int32_t L_used;
  double eps_used;
  int64_t n_flf_run;   /* inverse-L trajectories the device actually integrated (<= n_cold): a particle that has
                          just moved by F has F L F (X, -V) = F L (X, V), the L proposal of the iteration in which
                          it flipped -- the same operations on the same numbers (the reference's authors left the
                          shortcut commented out, markov_jump_hmc.py:401); the dense kernels hand its H() on instead
                          of integrating it again.  Results and the reference's counters are unaffected           */
} mjhmc_iter_stats;

const char* mjhmc_last_error(void);
int mjhmc_abi_version(void);

int mjhmc_ctx_create(int device, mjhmc_ctx** out);
int mjhmc_ctx_destroy(mjhmc_ctx* ctx);
/* name ("<marketing name> (<gcn arch>) [<pci domain:bus:device.0>]"), CU count, HBM bytes of the bound device */
int mjhmc_ctx_info(mjhmc_ctx* ctx, char* name, size_t name_cap, int* n_cu, uint64_t* hbm_bytes);

/* Replaces constructing a Distribution subclass (mjhmc/misc/distributions.py:20-59). */
int mjhmc_energy_create(mjhmc_ctx* ctx, int kind, int ndims, const double* params, size_t nparams,
                        mjhmc_energy** out);
/* LambdaDistribution(energy_func, energy_grad_func, ...) with arbitrary callables (README.md:27-36,
 * mjhmc/misc/distributions.py:198-251).  A Python callable cannot run on the device; the caller states the same two
 * functions as C expressions of ONE coordinate for a separable energy
 *     E(x) = sum_d energy_expr(x_d)      dE/dx_d = grad_expr(x_d)
 * with `x` the coordinate (double), `d` its index (int) and `p[k]` the float64 parameters, e.g.
 * ("0.5*x*x/(p[0]*p[0])", "x/(p[0]*p[0])") or ("log(1.0 + x*x/p[d])", "2.0*x/(p[d] + x*x)").  The engine's kernel
 * templates are compiled around them with hipRTC for gfx950 (include_dir: the directory holding jump_kernel.hpp and
 * philox.hpp, mjhmc_amd/csrc of this package); float64 state; every sampler family and the replay mode work as for the
 * built-in elementwise energies.  A compile error in the expressions is returned as MJHMC_ERR_INVALID with the
 * compiler's log in mjhmc_last_error(). */
int mjhmc_energy_create_expr(mjhmc_ctx* ctx, int ndims, const char* energy_expr, const char* grad_expr,
                             const double* params, size_t nparams, const char* include_dir, mjhmc_energy** out);
/* compile-only check of a pair of expressions (needs no device): 0, or MJHMC_ERR_INVALID with the compiler's log */
int mjhmc_expr_check(int ndims, const char* energy_expr, const char* grad_expr, const char* include_dir);
/* The same for energies that are separable GIVEN a few per-particle statistics (coupled coordinates):
 *     S[k] = sum_d stat_k(x_d, d; p)                 stat_exprs: the stat_k separated by ';' (NULL / "": none)
 *     E(x) = energy0_expr(S; p) + sum_d energy_expr(x_d, d, S; p)          (energy0_expr may be NULL: 0)
 *     dE/dx_d = grad_expr(x_d, d, S; p)              with the chain-rule terms through S written out by the caller
 * e.g. Neal's funnel (mjhmc/misc/tf_distributions.py:143-147), scale p[0], D = ndims:
 *     stats  "d == 0 ? x : 0.0; d == 0 ? 0.0 : x*x"
 *     energy "0.0"      energy0 "S[0]*S[0]/(2*p[0]*p[0]) + 0.5*exp(-S[0])*S[1] + 0.5*(p[1]-1)*S[0]"      (p[1] = D)
 *     grad   "d == 0 ? x/(p[0]*p[0]) - 0.5*exp(-x)*S[1] + 0.5*(p[1]-1) : x*exp(-S[0])"
 * The statistics are recomputed at every force evaluation (one group reduction each). */
int mjhmc_energy_create_expr_coupled(mjhmc_ctx* ctx, int ndims, const char* stat_exprs, const char* energy_expr,
                                     const char* energy0_expr, const char* grad_expr, const double* params, size_t nparams,
                                     const char* include_dir, mjhmc_energy** out);
int mjhmc_expr_check_coupled(int ndims, const char* stat_exprs, const char* energy_expr, const char* energy0_expr,
                             const char* grad_expr, const char* include_dir);
/* Linear-model energies on the ProductOfT matrix-core tile kernels (MJHMC_E_LINEAR_EXPR):
 *     E(x) = sum_{j<K} f(u_j, j),   u = W x + b,   dE/dx = W^T f'(u)
 * W: nexperts x ndims row-major, b: nexperts (float64 on input, stored float32 as PRODUCT_OF_T stores its parameters);
 * energy_expr = f and grad_expr = f', C expressions evaluated in float32 of
 *     u (float, the expert's input), j (int, the expert), p[k] (the nparams shared parameters, as float),
 *     q[m] (per-expert parameter row m < n_expert_rows <= 4 at expert j; expert_params: n_expert_rows x nexperts row-major).
 * Write float literals and functions (0.5f, logf) to stay in float32.  1 <= ndims, nexperts <= 512 (both padded to 128,
 * 256 or 512); wider models return MJHMC_ERR_UNSUPPORTED.  Padded experts contribute nothing (their f and f' are masked).
 * Examples: correlated Gaussian  f "0.5f*u*u", f' "u" with W the transposed Cholesky factor of the precision;
 * softplus  "u > 20.f ? u : log1pf(expf(u))", "1.f/(1.f + expf(-u))"; ProductOfT  "q[0]*logf(1.f + u*u)",
 * "2.f*q[0]*u/(1.f + u*u)" with W / nu, b / nu and q[0] = (nu + 1) / 2.
 * dtype F64 = float64 state around the float32 force (the reference's ProductOfT arithmetic), F32 = float32 state: every
 * path of PRODUCT_OF_T.  The kernels (14 for the model's padded size) are compiled with hipRTC at creation (include_dir as
 * for mjhmc_energy_create_expr) and cached per process by their source.  Compile errors: MJHMC_ERR_INVALID with the log. */
int mjhmc_energy_create_linear(mjhmc_ctx* ctx, int ndims, int nexperts, const double* W, const double* b,
                               const char* energy_expr, const char* grad_expr, const double* params, size_t nparams,
                               const double* expert_params, int n_expert_rows, const char* include_dir, mjhmc_energy** out);
/* compile-only check of a linear-model energy's expressions (needs no device): 0, MJHMC_ERR_INVALID with the compiler's
 * log, MJHMC_ERR_UNSUPPORTED beyond 512 */
int mjhmc_linear_check(int ndims, int nexperts, const char* energy_expr, const char* grad_expr, const char* include_dir);
/* Tall linear-model energies: the same form and the same expressions with MORE experts than dims -- 1 <= ndims <= 512,
 * 1 <= nexperts <= 2^20 (a GLM posterior: one expert per data row plus ndims prior experts).  The experts are stored in
 * ceil(nexperts / P) blocks of P = ndims padded to 128, 256 or 512, and one fused matrix-core kernel (compiled with hipRTC
 * at creation, cached per process) walks the blocks per tile of 32 particles: u = W x + b never reaches memory.  j is the
 * GLOBAL expert index; q[m] reads row m at it.  The kind is MJHMC_E_LINEAR_EXPR; samplers of such an energy run the
 * engine's multi-pass path with either state dtype (as PRODUCT_OF_T beyond 512 dims), so everything built on the ring works.
 * nexperts <= 512 is legal (one or a few blocks).  ndims > 512 or nexperts > 2^20: MJHMC_ERR_UNSUPPORTED; sizes < 1, NULLs,
 * more than 4 expert rows, non-finite W / b, compile errors (with the log): MJHMC_ERR_INVALID.  Device memory of the
 * matrices: 2 * ceil(nexperts / P) * P * P * 4 bytes (reported when the allocation fails). */
int mjhmc_energy_create_linear_tall(mjhmc_ctx* ctx, int ndims, int64_t nexperts, const double* W, const double* b,
                                    const char* energy_expr, const char* grad_expr, const double* params, size_t nparams,
                                    const double* expert_params, int n_expert_rows, const char* include_dir, mjhmc_energy** out);
/* compile-only check of a tall linear-model energy (needs no device): 0, MJHMC_ERR_INVALID, MJHMC_ERR_UNSUPPORTED as above */
int mjhmc_linear_tall_check(int ndims, int64_t nexperts, const char* energy_expr, const char* grad_expr, const char* include_dir);
/* Wide linear-model energies: the same form and the same expressions with MORE dims than 512 -- 1 <= ndims <= 4096,
 * 1 <= nexperts <= 2^20 (a regression with a thousand coefficients).  Always blocks of 512: the experts in
 * nblk = ceil(nexperts / 512) blocks, the dims in ND = ceil(ndims / 512) chunks, every (block, chunk) a zero-padded
 * 512 x 512 matrix, and one fused matrix-core kernel (compiled with hipRTC at creation, cached per process) walks them per
 * tile of 32 particles: per block u = b + sum over the chunks, ascending, of W x; then dE/dx chunk by chunk, kept in the
 * caller's dE/dX rows between blocks.  u = W x + b and f'(u) never reach memory; one launch per evaluation; the result
 * depends on the model and the row alone, bit for bit.  j is the GLOBAL expert index.  The kind is MJHMC_E_LINEAR_EXPR;
 * samplers run the engine's multi-pass path with either state dtype on rows of pitch 512 ND, so everything built on the ring
 * works, except the passes that take at most 512 dims: mjhmc_pointwise_create and mjhmc_influence_create refuse a wide
 * energy (MJHMC_ERR_UNSUPPORTED).  ndims <= 512 is legal: one chunk, the operations of the tall form at P = 512 in the same
 * order.  ndims > 4096 or nexperts > 2^20: MJHMC_ERR_UNSUPPORTED, naming the limit; sizes < 1, NULLs, more than 4 expert rows,
 * non-finite W / b, compile errors (with the log): MJHMC_ERR_INVALID, sizes before the context is looked at.  Device memory of
 * the matrices: 2 * nblk * ND * 512 * 512 * 4 bytes (reported when the allocation fails). */
int mjhmc_energy_create_linear_wide(mjhmc_ctx* ctx, int ndims, int64_t nexperts, const double* W, const double* b,
                                    const char* energy_expr, const char* grad_expr, const double* params, size_t nparams,
                                    const double* expert_params, int n_expert_rows, const char* include_dir, mjhmc_energy** out);
/* compile-only check of a wide linear-model energy (needs no device): 0, MJHMC_ERR_INVALID, MJHMC_ERR_UNSUPPORTED as above */
int mjhmc_linear_wide_check(int ndims, int64_t nexperts, const char* energy_expr, const char* grad_expr, const char* include_dir);
/* Grouped linear-model energies: the tall form with a log-sum-exp over groups of experts,
 *     E(x) = sum_{j<K} f(u_j, j) + sum_{g<G} LSE_{c<C} u_{gC+c},   dE/dx = W^T phi,   phi_j = f'(u_j, j) + [j < G C] softmax_g(u)_c
 * -- multinomial logistic (softmax) regression: G = n_groups data rows of C = group_size classes as the FIRST G C experts
 * (group g is the experts g C .. g C + C - 1), then plain experts (a prior) exactly as in a tall model.  2 <= C <= 16,
 * G >= 1, G C <= nexperts <= 2^20, 1 <= ndims <= 512; nexperts <= 512 is legal.  f, f', p[k], q[m] and j (the caller's
 * expert index) are as for the tall entry point.  The group term is float32 in one stated order: m = fmaxf over c
 * ascending, t_c = expf(u_c - m), s = t_0 + ... + t_{C-1}, the term m + logf(s), the softmax t_c / s (IEEE division): no
 * overflow for any finite u.  The experts are stored so that a group lies in the registers of one lane of the matrix-core
 * tile (mjhmc_linear_grouped_layout); one fused kernel, compiled with hipRTC at creation for this C, walks the grouped
 * blocks and then the plain ones.  The kind is MJHMC_E_LINEAR_EXPR and the sampler runs the multi-pass path with either state
 * dtype, as for a tall model of any nexperts.  The per-expert passes (mjhmc_pointwise_create, mjhmc_influence_create) refuse
 * a grouped energy: MJHMC_ERR_UNSUPPORTED; its per-row pass is mjhmc_pointwise_create_grouped.  group_size < 2, n_groups < 1, G C > nexperts, NULLs, more than 4 expert rows,
 * non-finite W / b, compile errors (with the log): MJHMC_ERR_INVALID.  group_size > 16, ndims > 512, more than 2^20 slots:
 * MJHMC_ERR_UNSUPPORTED, naming the limit. */
int mjhmc_energy_create_linear_grouped(mjhmc_ctx* ctx, int ndims, int64_t nexperts, const double* W, const double* b,
                                       int group_size, int64_t n_groups, const char* energy_expr, const char* grad_expr,
                                       const double* params, size_t nparams, const double* expert_params, int n_expert_rows,
                                       const char* include_dir, mjhmc_energy** out);
/* compile-only check of a grouped linear-model energy (needs no device): 0, MJHMC_ERR_INVALID, MJHMC_ERR_UNSUPPORTED as above */
int mjhmc_linear_grouped_check(int ndims, int64_t nexperts, int group_size, int64_t n_groups, const char* energy_expr,
                               const char* grad_expr, const char* include_dir);
/* The storage order of a grouped model (needs no device): *n_slots = the slots, (grouped blocks + plain blocks) * P with
 * P = ndims padded to 128, 256 or 512, and, when slot_to_expert is not NULL (room for *n_slots entries; call once with
 * NULL for the size), the caller's expert of every slot, -1 for padding.  Slot blk P + 32 NB w + NB r32 + r (NB = P / 128,
 * w < 4 the wave, r32 = (q & 3) + 8 (q >> 2) + 4 h the accumulator row of register q < 16 in lane half h, r < NB) is slot
 * s = NB q + r of lane type (w, h); a lane type of a grouped block holds Gl = floor(16 NB / C) groups, group
 * (8 blk + 2 w + h) Gl + gl in its slots C gl .. C gl + C - 1.  The arguments are checked as by mjhmc_linear_grouped_check. */
int mjhmc_linear_grouped_layout(int ndims, int64_t nexperts, int group_size, int64_t n_groups, int64_t* slot_to_expert,
                                int64_t* n_slots);
int mjhmc_energy_destroy(mjhmc_energy* e);

/* One evaluation of E_val / dEdX_val (mjhmc/misc/distributions.py:66-81) on n columns.
 * E_out (n) and dEdX_out (D,n) may each be NULL. */
int mjhmc_eval(mjhmc_energy* e, int dtype, const double* X, int64_t n, double* E_out, double* dEdX_out);

/* Replaces HMCState.__init__ (mjhmc/samplers/hmc_state.py:13-44) as called from
 * ContinuousTimeHMC.__init__ / HMCBase.__init__ (markov_jump_hmc.py:46-65,225-234).
 *   Xinit (D,N) float64.  Vinit (D,N) float64 or NULL -> standard normals from the counter RNG
 *   (tick 0).  first_particle_id: global id of column 0 (shard offset); the RNG is keyed by
 *   global id so results do not depend on how columns are sharded over GPUs. */
int mjhmc_sampler_create(mjhmc_ctx* ctx, mjhmc_energy* e, int64_t nparticles, int64_t first_particle_id,
                         int dtype, const double* Xinit, const double* Vinit, uint64_t seed, int mode,
                         mjhmc_sampler** out);
int mjhmc_sampler_destroy(mjhmc_sampler* s);

/* epsilon, num_leapfrog_steps, p_r, beta as used by HMCState.R, p_flip
 * (markov_jump_hmc.py:67-80,189,197-200,221-223). */
int mjhmc_set_hparams(mjhmc_sampler* s, double epsilon, int num_leapfrog_steps, double p_r, double beta,
                      double p_flip);

/* Runs up to n_iter sampling_iteration()s back to back on the sampler's stream with no host
 * round trip in between.  Stops early when an attempt hits a non-finite rate: that attempt is
 * rolled back (nothing committed), *n_done is the number of committed iterations, and the
 * caller performs the reference's halve-epsilon / double-L / reset_flf_cache / retry / restore
 * sequence (markov_jump_hmc.py:376-389) through mjhmc_set_hparams + mjhmc_reset_flf_cache +
 * mjhmc_iterate(1).  Return value stays 0 in that case.
 *
 * Replay inputs (all nullable; NULL -> counter RNG):
 *   replay_normal (n_iter, D, N) the randn blocks of HMCState.R (hmc_state.py:125)
 *   replay_exp    (n_iter, 3, N) unit exponentials behind draw_from (utils.py:42), rows L,F,R
 *                 (MJHMC) or FL,F,R (CTHMC)
 *   replay_unif   (n_iter, 2N+1) CONTROL mode: rand(N) accept, rand(N) flip, random() R gate
 * per_iter: n_iter entries (nullable); entry i describes attempt i (valid for i <= *n_done).
 * ring_slot0 >= 0: iteration i additionally records its post-jump X in ring slot ring_slot0+i
 * and its dwelling times in dwell slot ring_slot0+i (see mjhmc_ring_alloc). */
int mjhmc_iterate(mjhmc_sampler* s, int n_iter, const double* replay_normal, const double* replay_exp,
                  const double* replay_unif, int ring_slot0, mjhmc_iter_stats* per_iter, int* n_done);

/* The sample loop of HMCBase.sample / ContinuousTimeHMC.sample (markov_jump_hmc.py:150-173, 293-338: an iteration, then
 * samples.append(state.copy().X)) with the copies crossing PCIe WHILE the following iterations run: mjhmc_iterate(n_iter,
 * counter RNG, ring_slot0) plus, for every iteration i as soon as its kernels are done, ring slot ring_slot0 + i re-tiled
 * and brought to host_out[:, (k0 + i) * N : (k0 + i + 1) * N] of a C-order float64 array (ndims, n_total * N) -- the layout
 * of np.concatenate(samples, axis=1) -- by a second stream and a worker thread of the call.  Returns when the slots of the
 * committed iterations are in host memory.  A ring smaller than the run (n_slots < n_total: n_total states exceed the
 * device) is walked in several calls with growing k0.  per_iter / n_done / non-finite rates: as mjhmc_iterate. */
int mjhmc_iterate_download(mjhmc_sampler* s, int n_iter, int ring_slot0, double* host_out, int64_t n_total, int64_t k0,
                           mjhmc_iter_stats* per_iter, int* n_done);

/* ---- energies only the caller can evaluate (MJHMC_E_HOST) ----------------------------------------------------------
 * LambdaDistribution(energy_func, energy_grad_func, init) takes two arbitrary Python callables (README.md:27-36,
 * mjhmc/misc/distributions.py:198-251).  When they match no built-in functor and are not stated as C expressions,
 * the sampler keeps everything on the device EXCEPT the two evaluations: the particle state (X, V, dE/dX, EX, EV, the
 * inverse-L cache), the leapfrog updates in the reference's literal order (hmc_state.py:86-100), the jump decision,
 * successor selection, momentum refresh, counters, dwelling times and the sample ring.  One sampling_iteration
 * (markov_jump_hmc.py:355-415; :116-148 and :251-290 for the other sampler families) is
 *     mjhmc_traj_begin(s, &n)                  n = N proposal columns (the L proposal of every particle) + n_cold columns
 *                                              (the inverse-L proposal F L F of the cold-cache particles, MJHMC only)
 *     X = mjhmc_traj_step(s, NULL, 0, X)       first step: uses the stored dE/dX
 *     for every further leapfrog step:  g = energy_grad_func(X);  mjhmc_traj_step(s, g, 0, X)
 *     g = energy_grad_func(X);                 mjhmc_traj_step(s, g, 1, NULL)       closing half kick
 *     mjhmc_traj_finish(s, energy_func(X), ..., &stats)      decide + commit; stats->nonfinite as mjhmc_iterate reports it
 * All matrices are (ndims, n) float64 C order, columns in the order above.  mjhmc_iterate refuses such samplers.
 * mjhmc_host_set_energy: E (N) and dE/dX (D,N) of the CURRENT state -- after mjhmc_sampler_create and after every
 * mjhmc_write of X (HMCState.__init__ evaluates both, hmc_state.py:30-38). */
int mjhmc_host_set_energy(mjhmc_sampler* s, const double* E, const double* dEdX);
int mjhmc_traj_begin(mjhmc_sampler* s, int64_t* n_cols);
int mjhmc_traj_step(mjhmc_sampler* s, const double* grad, int last, double* X_out);
/* replay_* as mjhmc_iterate's, for ONE iteration; ring_slot >= 0 records X and the dwelling times there */
int mjhmc_traj_finish(mjhmc_sampler* s, const double* E, const double* replay_normal, const double* replay_exp,
                      const double* replay_unif, int ring_slot, mjhmc_iter_stats* stats);

/* Transaction support for multi-GPU runs: the reference aborts and retries the WHOLE batch when any
 * particle hits a non-finite rate (markov_jump_hmc.py:376-389).  With columns sharded over ranks a
 * rank may have run past the iteration that failed elsewhere; it restores the checkpoint taken at the
 * start of the batch and replays (the counter RNG makes the replay bit-identical).
 * checkpoint: device copy of X, V, EX, EV, H_flf, dwell + the RNG tick.  restore: put it back. */
int mjhmc_checkpoint(mjhmc_sampler* s);
int mjhmc_restore(mjhmc_sampler* s);
/* Undo the last call when it was mjhmc_iterate(1) (or one mjhmc_traj_finish) and committed: the iteration's inputs are
 * the untouched other halves of the ping-pong buffers -- or, for the samplers that commit in place (rows wider than the
 * register kernels, host-evaluated energies), the pre-move state the commit left in its workspace -- so no copy is taken
 * beforehand (the RNG tick stays consumed). */
int mjhmc_rollback(mjhmc_sampler* s);
/* The position of the counter RNG (one tick per sampling_iteration attempt): together with X, V and H_flf
 * (mjhmc_read / mjhmc_write) it is the whole resumable state of a sampler -- mjhmc_amd's save_state / load_state write it
 * to an .npz file, and a restored sampler continues bit for bit. */
int mjhmc_get_tick(mjhmc_sampler* s, uint64_t* tick);
int mjhmc_set_tick(mjhmc_sampler* s, uint64_t tick);
/* skip n RNG ticks (a rank that did not execute a failed attempt must still consume its tick) */
int mjhmc_advance_tick(mjhmc_sampler* s, int64_t n);

/* HMCState.reset_flf_cache (hmc_state.py:145-148). */
int mjhmc_reset_flf_cache(mjhmc_sampler* s);

/* Field access for sampler.state.X / .V / .EX / ... and HMCState assignment (figures/poe_fig.py:59).
 * Writing X or V re-derives EX/EV on the device and clears the FLF cache. */
int mjhmc_read(mjhmc_sampler* s, int field, void* host_dst, size_t nbytes);
int mjhmc_write(mjhmc_sampler* s, int field, const void* host_src, size_t nbytes);

/* Sample ring for ContinuousTimeHMC.sample / HMCBase.sample (markov_jump_hmc.py:150-173,293-338):
 * n_slots snapshots of X (device resident) and of dwelling_times. */
int mjhmc_ring_alloc(mjhmc_sampler* s, int n_slots);   /* (never shrinks; a request the device cannot hold fails with the
                                                           sizes in mjhmc_last_error() and keeps the ring there was) */
/* device bytes of one ring slot (a padded state matrix + its dwelling times); free / total device memory in bytes:
 * what a caller sizes a sample ring by */
int mjhmc_ring_slot_bytes(mjhmc_sampler* s, uint64_t* bytes);
int mjhmc_mem_info(mjhmc_ctx* ctx, uint64_t* free_bytes, uint64_t* total_bytes);
/* dwell of slots [slot0, slot0+n) -> (n, N) float64 */
int mjhmc_ring_read_dwell(mjhmc_sampler* s, int slot0, int n, double* host_dst);
/* out[:, k] = X_slot[idx[k] / N][:, idx[k] % N] for k < n, i.e. the column gather of
 * `samples[:, sample_idx]` (markov_jump_hmc.py:322-328) with idx into the time-major pool.
 * out is (D, n) float64. */
int mjhmc_ring_gather(mjhmc_sampler* s, const int64_t* idx, int64_t n, double* host_out);
/* whole slots [slot0, slot0+n): (D, n*N) time-major if stacked==0 (np.concatenate(axis=1)),
 * (D, N, n) if stacked==1 (np.stack(axis=-1)). */
int mjhmc_ring_read(mjhmc_sampler* s, int slot0, int n, int stacked, double* host_out);

/* sum_k (x_k - shift) and sum_k (x_k - shift)^2 over every state element (d < ndims, particle < N) of ring
 * slots [slot0, slot0 + n): the device half of the reference's online variance estimate
 * (mjhmc/misc/gen_mj_init.py:76-98), which walks sampler.sample(1).ravel() value by value. */
int mjhmc_ring_moments(mjhmc_sampler* s, int slot0, int n, double shift, double* sum, double* sumsq);

/* Weighted sufficient statistics of ring blocks, kept on the device (csrc/estimators.hip): what a caller of
 * sampler.sample() computes next in the reference -- online_variance (mjhmc/misc/gen_mj_init.py:76-98), posterior
 * means and variances -- without the (ndims, n_samples * nbatch) download.  For states x[k][p][:] (ring slot
 * x_slot0 + k, particle p < N), weights w[k][p] and a shift vector c of ndims doubles:
 *   W = sum w,  S1_d = sum w (x_d - c_d),  S2_d = sum w (x_d - c_d)^2,  C_de = sum w (x_d - c_d)(x_e - c_e),
 * all in float64, every state dtype widened exactly; the order of addition is fixed, so the result is bit-identical
 * from run to run on one device.
 * An estimator belongs to the sampler it was created on: mjhmc_sampler_destroy frees every estimator still alive on
 * it, and the handle is INVALID from then on -- mjhmc_estimator_destroy (or any other call) on it after the sampler is
 * gone is a use after free.  Destroy estimators first, or not at all.
 * The sampler must have its ring (mjhmc_ring_alloc); want_cov != 0 also keeps the ndims x ndims matrix C and needs
 * ndims <= 512 (MJHMC_ERR_INVALID beyond: first and second moments work for every ndims). */
typedef struct mjhmc_estimator mjhmc_estimator;
int mjhmc_estimator_create(mjhmc_sampler* s, int want_cov, mjhmc_estimator** out);
int mjhmc_estimator_destroy(mjhmc_estimator* est);
/* c: ndims finite doubles, NULL = zero (the state at create).  Only while the estimator is empty: sums about
 * different shifts do not add (MJHMC_ERR_INVALID after an accumulate; mjhmc_estimator_reset first). */
int mjhmc_estimator_set_shift(mjhmc_estimator* est, const double* c);
/* Adds the n states of ring slots [x_slot0, x_slot0 + n) with the weights of dwell-ring slots [w_slot0, w_slot0 + n),
 * or unit weights for w_slot0 == -1 (the discrete-time samplers).  The iteration that fills ring slot s writes the
 * holding time of the state it LEFT (slot s - 1) to dwell slot s (mjhmc/samplers/markov_jump_hmc.py:262-277,
 * 366-395: the rates are those of self.state before the update), so the holding time of the state in slot s is in
 * dwell slot s + 1: a jump sampler's time average takes w_slot0 = x_slot0 + 1.
 * MJHMC_ERR_INVALID: slots outside the ring, n < 1, or a ring re-allocated since mjhmc_estimator_create.
 * MJHMC_ERR_NONFINITE: one of the weights is not finite (a zero total rate gives an infinite dwell); nothing of the
 * block has been added. */
int mjhmc_estimator_accumulate(mjhmc_estimator* est, int x_slot0, int w_slot0, int n);
/* The only download: W, S1[ndims], S2[ndims], C[ndims * ndims] (row-major, symmetric bit for bit; NULL to skip, must
 * be NULL for an estimator without covariance) and the number of (slot, particle) states added so far. */
int mjhmc_estimator_read(mjhmc_estimator* est, double* W, double* S1, double* S2, double* C, int64_t* n_states);
/* zero sums and count; the shift stays */
int mjhmc_estimator_reset(mjhmc_estimator* est);
/* Ring slot src_slot (state and dwelling times) copied to dst_slot on the device, on the sampler's stream: carries the
 * last state of one block to the front of the next.  MJHMC_ERR_INVALID if dst_slot holds the live state. */
int mjhmc_ring_copy(mjhmc_sampler* s, int src_slot, int dst_slot);

/* Per-chain weighted sums of ring blocks, kept on the device (csrc/chainstats.hip): what R-hat (plain and split) and
 * the multi-chain effective sample size are made of.  The reference reaches them only through
 * sample(preserve_order=True) (mjhmc/samplers/markov_jump_hmc.py:150-173, 293-338): the (ndims, nbatch, n) array on the
 * host, reduced there.  For states x[k][p][:] (ring slot x_slot0 + k, chain = particle p < N), weights w[k][p] and a
 * shift vector c of ndims doubles, per part h < n_parts (part = which half of the run, so that split R-hat sees the two
 * halves of a chain as two chains) and per chain:
 *   a0_p = sum_k w,  a1_pd = sum_k w (x_d - c_d),  a2_pd = sum_k w (x_d - c_d)^2
 * in float64 (every state dtype widened exactly), in the fixed order
 *   t = x - c;  u = w * t;  a1 = a1 + u;  a2 = a2 + u * t;  a0 = a0 + w          k ascending, from the stored sums,
 * every product rounded before its sum: the sums are bit-identical to that sequence of IEEE float64 operations and do
 * not depend on how a run is cut into accumulate calls.
 * Ownership as for mjhmc_estimator: a chainstats belongs to the sampler it was created on, mjhmc_sampler_destroy frees
 * it, and the handle is invalid from then on.  Device memory: n_parts * (2 * row pitch + 1) * Npad doubles.
 * Replaces sample(preserve_order=True) + a host reduction (markov_jump_hmc.py:150-173, 293-338); n_parts is 1 or 2 and
 * the sampler must have its ring. */
typedef struct mjhmc_chainstats mjhmc_chainstats;
int mjhmc_chainstats_create(mjhmc_sampler* s, int n_parts, mjhmc_chainstats** out);
int mjhmc_chainstats_destroy(mjhmc_chainstats* cs);
/* c: ndims finite doubles, NULL = zero (the state at create).  Only while every part is empty (MJHMC_ERR_INVALID after
 * an accumulate; mjhmc_chainstats_reset first).  The reference has no counterpart: its host reduction of
 * sample(preserve_order=True) (markov_jump_hmc.py:150-173, 293-338) is free to centre as it likes. */
int mjhmc_chainstats_set_shift(mjhmc_chainstats* cs, const double* c);
/* Adds the n states of ring slots [x_slot0, x_slot0 + n) to the chains' sums of `part`, with the weights of dwell-ring
 * slots [w_slot0, w_slot0 + n) or unit weights for w_slot0 == -1: the pairing of mjhmc_estimator_accumulate (a jump
 * sampler takes w_slot0 = x_slot0 + 1).  What appending the block to the array of sample(preserve_order=True)
 * (markov_jump_hmc.py:150-173, 293-338) is on the host.
 * MJHMC_ERR_INVALID: slots outside the ring, n < 1, part outside [0, n_parts), or a ring re-allocated since create.
 * MJHMC_ERR_NONFINITE: a weight of a chain p < N is not finite; the sums are as before the call. */
int mjhmc_chainstats_accumulate(mjhmc_chainstats* cs, int part, int x_slot0, int w_slot0, int n);
/* The fold of one part, in a fixed order (bit-identical from run to run on one device), O(ndims) download.  With
 * m_pd = a1_pd / a0_p and v_pd = a2_pd / a0_p - m_pd * m_pd over the chains p < N:
 *   *n_chains = N, *n_states_per_chain = slots accumulated, *Sw = sum_p a0_p,
 *   Sm[d] = sum_p m_pd, Sq[d] = sum_p m_pd^2, Sv[d] = sum_p v_pd          (ndims doubles each).
 * All of them add over parts and over ranks.  MJHMC_ERR_INVALID for a part nothing was added to.  The host reduction
 * of sample(preserve_order=True) (markov_jump_hmc.py:150-173, 293-338) over its last axis, then over chains. */
int mjhmc_chainstats_read(mjhmc_chainstats* cs, int part, int64_t* n_chains, int64_t* n_states_per_chain, double* Sw,
                          double* Sm, double* Sq, double* Sv);
/* The per-chain sums themselves, O(N * ndims): a0 (N), a1 and a2 (ndims, N) float64 C order, the layout of every host
 * array of the reference (a slice of sample(preserve_order=True), markov_jump_hmc.py:150-173, 293-338, reduced over
 * its last axis).  Any of the three may be NULL. */
int mjhmc_chainstats_read_chains(mjhmc_chainstats* cs, int part, double* a0, double* a1, double* a2);
/* zero sums and counts of every part; the shift stays (a fresh sample(preserve_order=True),
 * markov_jump_hmc.py:150-173, 293-338) */
int mjhmc_chainstats_reset(mjhmc_chainstats* cs);

/* Weighted marginal histograms of ring blocks, kept on the device (csrc/histograms.hip): medians, quantiles, credible
 * intervals and a CDF of every dimension without downloading the states -- what np.histogram of the rows of
 * sample(preserve_order=True) (markov_jump_hmc.py:150-173, 293-338), weighted by the holding times for the jump
 * samplers, is on the host.  n_bins bins (1 .. 1024) between lo[d] and hi[d] (ndims finite doubles each, lo < hi) plus an
 * underflow and an overflow bin per dimension; `quantum` q is a positive power of two.  With inv_d = n_bins / (hi_d -
 * lo_d) in float64, for every state element x (widened exactly to float64) and its weight w:
 *     t = (x - lo_d) * inv_d                      two rounded float64 operations, not fused
 *     bin = 0 when !(t >= 0) (NaN lands here);  n_bins + 1 when t >= n_bins;  1 + (int)t otherwise
 *     u = rint(w / q)                             nearest-even; the division is exact
 *     count[d][bin] += 1;  mass[d][bin] += u      uint64 tables [ndims][n_bins + 2]
 * and W_units += u once per state (the row sum of every mass[d]).  Every sum is an integer: the tables are bit-identical
 * from run to run, do not depend on how a run is cut into blocks, and add exactly over ranks.
 * |q * mass[d][b] - (sum of the w of bin b)| <= 0.5 * q * count[d][b].
 * Ownership as for mjhmc_estimator: a histogram belongs to the sampler it was created on (and to its ring: a
 * re-allocated ring invalidates it), mjhmc_sampler_destroy frees every one still alive and the handle is INVALID from
 * then on. */
typedef struct mjhmc_histogram mjhmc_histogram;
int mjhmc_histogram_create(mjhmc_sampler* s, int n_bins, const double* lo, const double* hi, double quantum,
                           mjhmc_histogram** out);
int mjhmc_histogram_destroy(mjhmc_histogram* h);
/* Adds the n states of ring slots [x_slot0, x_slot0 + n) with the weights of dwell-ring slots [w_slot0, w_slot0 + n),
 * or unit weights for w_slot0 == -1: the pairing of mjhmc_estimator_accumulate (a jump sampler takes w_slot0 =
 * x_slot0 + 1).  The weights are checked on the device ahead of the pass; a refused block adds nothing.
 * MJHMC_ERR_INVALID: slots outside the ring, n < 1, a ring re-allocated since create, a weight with w / q >= 2^53, or a
 * block that would take W_units to 2^63 or beyond.  MJHMC_ERR_NONFINITE: a weight that is not finite, or negative. */
int mjhmc_histogram_accumulate(mjhmc_histogram* h, int x_slot0, int w_slot0, int n);
/* count, mass: ndims * (n_bins + 2) values each, row d = [underflow, bin 0 .. n_bins - 1, overflow]; the total of the
 * units and the number of (slot, particle) states added so far. */
int mjhmc_histogram_read(mjhmc_histogram* h, uint64_t* count, uint64_t* mass, uint64_t* W_units, int64_t* n_states);
/* zero tables and totals; range, bins and quantum stay */
int mjhmc_histogram_reset(mjhmc_histogram* h);

/* Weighted JOINT histograms of pairs of state dimensions over ring blocks, kept on the device (csrc/pairhist.hip): the
 * picture the reference draws with hist_2d / gauss_2d / jump_plot (mjhmc/misc/plotting.py) -- what np.histogram2d of two
 * rows of sample(preserve_order=True) (markov_jump_hmc.py:150-173, 293-338), weighted by the holding times for the jump
 * samplers, is on the host.  The contract is that of mjhmc_histogram_accumulate, taken per axis.
 * n_pairs = P pairs (i_p, j_p) of state dimensions (pairs: int32 [P][2]; 0 <= i, j < ndims; i == j, repeated pairs and
 * both orders of a pair are legal), n_bins = B bins per axis, per pair and axis a range lo[p][a] < hi[p][a] (lo, hi:
 * double [P][2], finite; a = 0 the i axis, a = 1 the j axis), one `quantum` q, a positive power of two.  With
 * inv[p][a] = B / (hi[p][a] - lo[p][a]) in float64, for every state (its elements widened exactly to float64) of weight w:
 *     t_a = (x_a - lo[p][a]) * inv[p][a]          two rounded float64 operations, not fused
 *     b_a = 0 when !(t_a >= 0) (NaN lands here);  B + 1 when t_a >= B;  1 + (int)t_a otherwise
 *     u   = rint(w / q)                           nearest-even; the division is exact
 *     count[p][b_1][b_0] += 1;  mass[p][b_1][b_0] += u       uint64 tables [P][B + 2][B + 2], the i axis fastest
 * and W_units += u once per state.  Every sum is an integer: the tables are bit-identical from run to run, do not depend
 * on how a run is cut into blocks, and add exactly over ranks; there is no floating-point atomic in the pass.  With equal
 * range, B and q, summing pair p's tables over the j axis (all B + 2 entries, outer bins included) gives exactly dimension
 * i_p's row of mjhmc_histogram's tables of the same block.
 * Limits, each refused with MJHMC_ERR_INVALID and a message that names it: 1 <= P <= 64, 1 <= B <= 128; a sampler of 2^32
 * particles or more is refused with MJHMC_ERR_UNSUPPORTED (N < 2^32).
 * Ownership as for mjhmc_histogram: a pair histogram belongs to the sampler it was created on (and to its ring: a
 * re-allocated ring invalidates it), mjhmc_sampler_destroy frees every one still alive and the handle is INVALID from
 * then on. */
typedef struct mjhmc_pairhist mjhmc_pairhist;
int mjhmc_pairhist_create(mjhmc_sampler* s, int n_pairs, const int32_t* pairs, int n_bins, const double* lo, const double* hi,
                          double quantum, mjhmc_pairhist** out);
int mjhmc_pairhist_destroy(mjhmc_pairhist* h);
/* Adds the n states of ring slots [x_slot0, x_slot0 + n) with the weights of dwell-ring slots [w_slot0, w_slot0 + n),
 * or unit weights for w_slot0 == -1: the pairing of mjhmc_histogram_accumulate (a jump sampler takes w_slot0 =
 * x_slot0 + 1).  Rows p >= N and the dwell ring's padding are never read.  The weights are checked on the device ahead
 * of the pass by the 1-D pass's own check; a refused block adds nothing, with that pass's codes and messages:
 * MJHMC_ERR_NONFINITE: a weight that is not finite, or negative.  MJHMC_ERR_INVALID: a weight with w / q >= 2^53, a block
 * that would take W_units to 2^63 or beyond, slots outside the ring, n < 1, or a ring re-allocated since create. */
int mjhmc_pairhist_accumulate(mjhmc_pairhist* h, int x_slot0, int w_slot0, int n);
/* count, mass: n_pairs * (n_bins + 2) * (n_bins + 2) values each, table p row b_1 = [underflow of i, i bins 0 .. n_bins - 1,
 * overflow of i]; the total of the units and the number of (slot, particle) states added so far. */
int mjhmc_pairhist_read(mjhmc_pairhist* h, uint64_t* count, uint64_t* mass, uint64_t* W_units, int64_t* n_states);
/* zero tables and totals; pairs, ranges, bins and quantum stay */
int mjhmc_pairhist_reset(mjhmc_pairhist* h);

/* Device functionals: statistics of caller expressions g(x) of the recorded states (csrc/functionals.hip), for which
 * the reference has only sample(preserve_order=True) (markov_jump_hmc.py:150-173, 293-338) and NumPy on the host.  The
 * coupled-energy convention of mjhmc_energy_create_expr_coupled, as an observable:
 *     S[j] = sum_{d < ndims} stat_j(x_d, d; p)     j < J, 0 <= J <= 8
 *     g[k] = value_k(S; p)                         k < K, 1 <= K <= 16
 * `stats` and `values` hold C expressions separated by ';' (stats may be NULL or empty): a stat is an expression of `x`
 * (the coordinate, widened exactly to float64 from a float64, float32 or bfloat16 ring), `d` (its index, int) and `p[m]`
 * (the nparams float64 parameters); a value is an expression of `S[j]` and `p[m]`.  `d == 3 ? x : 0.0` picks a coordinate.
 * Everything is float64 and compiled without contraction: an expression of + - * /, comparisons and ?: rounds operation
 * by operation.  One kernel (csrc/functionals.hpp) evaluates a block of sample-ring slots into a DERIVED ring of float64
 * rows [Npad][pitchK] -- the row layout of every sample ring, K "dimensions" -- and the accumulators created ON the
 * functionals (mjhmc_estimator_create_on, ...) read that ring: their accumulate / set_shift / read / read_chains / reset
 * / destroy entry points work unchanged, with x_slot0 a slot of the DERIVED ring, w_slot0 a slot of the SAMPLER's dwell
 * ring, and K for ndims.
 * The summation order of a stat is a function of the ring's row shape alone: values are bit-identical from run to run
 * and do not depend on how a run is cut into blocks.  Rows p >= N are neither read nor written.
 * Ownership: a functionals belongs to the sampler (mjhmc_sampler_destroy frees every one still alive) and to the sample
 * ring it was created on (a re-allocated sample ring invalidates it); mjhmc_functionals_destroy frees the handles created
 * on it, which are INVALID from then on.
 * MJHMC_ERR_INVALID with a message: more than 8 stats, K outside [1, 16], NULL arguments, no sample ring yet, and
 * expressions that do not compile (the hipRTC log is the message). */
typedef struct mjhmc_functionals mjhmc_functionals;
/* compiles the expressions for float64 rows of ndims and keeps nothing: needs no device */
int mjhmc_functionals_check(int ndims, const char* stats, const char* values, const char* include_dir);
int mjhmc_functionals_create(mjhmc_sampler* s, const char* stats, const char* values, const double* params, size_t nparams,
                             const char* include_dir, mjhmc_functionals** out);
/* Energy observables: a functionals whose K = 3 values of every recorded state are
 *     g[0] = E            the potential energy exactly as the sampler's own evaluation kernel returns it for the stored row
 *                         (float32 for float32 / bfloat16 state, widened exactly)
 *     g[1] = grad_sq      sum_{d < ndims} G_d * G_d, G = dE/dX of the same evaluation, each element widened exactly
 *     g[2] = virial       sum_{d < ndims} x_d * G_d, x the stored state widened exactly
 * -- what no sum of per-coordinate expressions gives for a coupled energy.  Integration by parts gives E[x . dE/dX] =
 * ndims for every target with p(x) x -> 0 at infinity, so mean(virial) / ndims is a thermometer of the chain: 1 when it
 * keeps exp(-E).  No expressions and no hipRTC: per slot mjhmc_functionals_evaluate runs the evaluation kernels of the
 * sampler's energy on the ring slot (a ring slot has the layout of a state matrix) into scratch of the handle -- one
 * gradient matrix and one energy vector, freed with the handle and by mjhmc_sampler_destroy -- and then one kernel
 * (csrc/energy_observables.hpp) that forms the derived row [E, grad_sq, virial, 0.0]: products and sums in float64
 * without contraction, in an order that is a function of (ndims, state type, row pitch) alone, so values are bit-identical
 * from run to run and independent of the blocks.  A value that is not finite is reported as by any functionals, the
 * message naming it (E, grad_sq, virial).  These evaluations are not part of the chain: no sampler state, counter or
 * random stream is touched.  _info, _ring_alloc, _evaluate, _read, _destroy and every _create_on work as on any
 * functionals.  MJHMC_ERR_INVALID: NULL arguments, no sample ring yet; MJHMC_ERR_UNSUPPORTED: a host-evaluated energy
 * (MJHMC_E_HOST: the caller's callables are its only evaluation). */
int mjhmc_functionals_create_energy(mjhmc_sampler* s, mjhmc_functionals** out);
/* Linear projections: a functionals whose K values of every recorded state are
 *     u[k] = b[k] + sum_{d < ndims} A[k][d] * x[d]        g[k] = link(u[k], k; p)        1 <= K <= 512
 * -- R-hat and ESS along principal axes, the read-outs of a linear model, sliced marginals: directions that are not
 * coordinate axes, up to 512 of them at once, which the J <= 8 lane sums of mjhmc_functionals_create cannot state.  A is
 * (K, ndims) float64 in C order, b has K entries or is NULL (zeros).  link_expr is NULL (the identity: the kernel is in the
 * library and hipRTC is not touched) or ONE C expression of `u` (float64), `k` (the value's index, int) and `p[m]` (the
 * nparams float64 parameters), e.g. "1.0 / (1.0 + exp(-u))"; it is compiled with hipRTC around csrc/projections.hpp with
 * the library's own flags.  The handle keeps device copies of A, b and p, freed with it and by mjhmc_sampler_destroy.
 * Arithmetic (csrc/projections.hpp): an accumulator starts at b[k] and adds the products in ascending d, each product
 * rounded before its sum (no contraction), no value split over lanes and no float atomics -- a value is a function of
 * (A, b, x) alone, bit-identical for every block, state type (rows are widened exactly) and tile, and equal to the NumPy
 * loop `u = b.copy(); for d: u = u + A[:, d, None] * X[d]` bit for bit.  _info, _ring_alloc, _evaluate, _read, _destroy
 * and every _create_on work as on any functionals; a value that is not finite is reported by _evaluate, the message naming
 * the lowest such value index.  Only the ring is read: host-evaluated energies are accepted.
 * MJHMC_ERR_INVALID with a message: K outside [1, 512], NULL s, A or out, an entry of A, b or p that is not finite (the
 * first is named), no sample ring yet, a link that does not compile (the hipRTC log is the message). */
int mjhmc_functionals_create_linear(mjhmc_sampler* s, int n_values, const double* A, const double* b, const char* link_expr,
                                    const double* params, size_t nparams, const char* include_dir, mjhmc_functionals** out);
/* the checks of mjhmc_functionals_create_linear that need no device: the range of K, and the compile of link_expr (NULL:
 * nothing to compile) for float64 rows; keeps nothing */
int mjhmc_projections_check(int n_values, const char* link_expr, const char* include_dir);
int mjhmc_functionals_destroy(mjhmc_functionals* f);
/* K, and the bytes of one slot of the derived ring (Npad * pitchK * 8) */
int mjhmc_functionals_info(mjhmc_functionals* f, int* n_values, uint64_t* slot_bytes);
/* at least n_slots slots of derived ring, zeroed.  Never shrinks; a growth is a NEW ring (its contents are gone and the
 * handles created on the old one refuse to accumulate) */
int mjhmc_functionals_ring_alloc(mjhmc_functionals* f, int n_slots);
/* Derived slots [out_slot0, out_slot0 + n) from the sampler's ring slots [x_slot0, x_slot0 + n), on the sampler's
 * stream; reads a flag back (one synchronisation).  MJHMC_ERR_NONFINITE: a value of a particle p < N is not finite -- the
 * message names the lowest such value index; the slots hold what was computed and should not be accumulated.
 * MJHMC_ERR_INVALID: slots outside either ring, n < 1, no derived ring, a sample ring re-allocated since create. */
int mjhmc_functionals_evaluate(mjhmc_functionals* f, int x_slot0, int n, int out_slot0);
/* host_out: (K, n, N) float64 C order, the values of derived slots [slot0, slot0 + n) (tests and inspection) */
int mjhmc_functionals_read(mjhmc_functionals* f, int slot0, int n, double* host_out);
/* mjhmc_estimator_create / mjhmc_chainstats_create / mjhmc_histogram_create on the derived ring (which must exist):
 * K dimensions (lo, hi: K doubles each), the sampler's particles, stream and dwell ring */
int mjhmc_estimator_create_on(mjhmc_functionals* f, int want_cov, mjhmc_estimator** out);
int mjhmc_chainstats_create_on(mjhmc_functionals* f, int n_parts, mjhmc_chainstats** out);
int mjhmc_histogram_create_on(mjhmc_functionals* f, int n_bins, const double* lo, const double* hi, double quantum,
                              mjhmc_histogram** out);
/* mjhmc_pairhist_create on the derived ring: pairs of the K functional values */
int mjhmc_pairhist_create_on(mjhmc_functionals* f, int n_pairs, const int32_t* pairs, int n_bins, const double* lo,
                             const double* hi, double quantum, mjhmc_pairhist** out);

/* Cell occupancy and transition counts of the recorded chains, kept on the device (csrc/occupancy.hip, csrc/occupancy.hpp):
 * how much time the ensemble spends in each region of the state space and how often a chain moves from one region to
 * another -- the empirical transition matrices the reference builds for its toy ladders only (mjhmc/misc/mixing.py,
 * mjhmc/experiments/spectral.py), for the continuous samplers.  The accumulators above say where the ensemble is; this
 * one keeps a per-chain memory from one recorded state to the next.
 * n_centres = M centres (1 .. 64) of n_dims = K coordinates each (centres: double [M][K], finite; K must be the ring's
 * ndims), r2: M squared radii (>= 0, +inf for none) or NULL for none, `quantum` q a positive power of two.  The cells are the
 * Voronoi cells of the centres -- with radii, cut to the balls -- and one more, index M, "outside".  For a state row x (its
 * elements widened exactly to float64), m ascending:
 *     d2_m = 0.0;  for d ascending below K:  t = x_d - c[m][d];  d2_m = d2_m + t * t     every operation rounded, not fused
 *     best = +inf, label = M;  m replaces the label only when d2_m < best (strictly: the lowest index wins ties; a NaN or
 *     infinite distance is never chosen, so a state that is not finite lands outside)
 *     with r2: label = M unless best <= r2[label]
 * Tables, uint64, indexed by cell in [0, M], with u = rint(w / q) (nearest-even; the division is exact):
 *     count[a], mass[a]             states in cell a and their units
 *     trans[a][b]                   pairs (state s, state s + 1) of one chain with labels a, b
 *     from_count[a], from_mass[a]   count / mass of the states that have a successor; from_count[a] = sum_b trans[a][b]
 *     W_units                       the sum of units
 * and per chain p switches[p] (transitions with a != b; the outside cell is a cell) and visited[p] (bit m: cell m < M was
 * seen).  Every sum is an integer: the tables are bit-identical from run to run and do not depend on how a run is cut into
 * linked blocks; there is no floating-point atomic in the pass.
 * Ownership as for mjhmc_histogram: the handle belongs to the sampler it was created on (and to its ring: a re-allocated
 * ring invalidates it), mjhmc_sampler_destroy frees every one still alive and the handle is INVALID from then on.
 * MJHMC_ERR_INVALID, before anything is allocated: M outside [1, 64], a centre that is not finite, an r2 that is negative
 * or NaN, K that is not the ring's ndims, a quantum that is no power of two, no ring. */
typedef struct mjhmc_occupancy mjhmc_occupancy;
int mjhmc_occupancy_create(mjhmc_sampler* s, int n_centres, int n_dims, const double* centres, const double* r2, double quantum,
                           mjhmc_occupancy** out);
/* on the derived ring (which must exist): the cells live in the space of the K functional values */
int mjhmc_occupancy_create_on(mjhmc_functionals* f, int n_centres, int n_dims, const double* centres, const double* r2,
                              double quantum, mjhmc_occupancy** out);
int mjhmc_occupancy_destroy(mjhmc_occupancy* h);
/* Adds the n states of ring slots [x_slot0, x_slot0 + n) of every chain, in slot order, with the weights of dwell-ring
 * slots [w_slot0, w_slot0 + n) or unit weights for w_slot0 == -1: the pairing of mjhmc_histogram_accumulate.  linked = 0
 * starts new chains at x_slot0 (no transition into its state is counted; switches and visited go on); linked = 1 says
 * that slot x_slot0 follows the last state of the previous block, whose label and units every chain carries, and counts
 * that pair too.  The weights are checked on the device ahead of the pass by mjhmc_histogram_accumulate's own check; a
 * refused block adds nothing and leaves the carry as it was, with that pass's codes and messages: MJHMC_ERR_NONFINITE: a
 * weight that is not finite, or negative.  MJHMC_ERR_INVALID: a weight with w / q >= 2^53, a block that would take
 * W_units to 2^63 or beyond, slots outside the ring, n < 1, linked = 1 on a handle that holds no block, or a ring
 * re-allocated since create. */
int mjhmc_occupancy_accumulate(mjhmc_occupancy* h, int x_slot0, int w_slot0, int n, int linked);
/* count, mass, from_count, from_mass: M + 1 values each; trans: (M + 1) * (M + 1), row a = the departures from cell a;
 * chains_by_switches: 17 values, the chains with 0 .. 15 and with 16 or more switches; chains_by_cells: M + 1 values, the
 * chains that saw exactly c distinct cells < M (both tallied on the device with integer atomics); switches (uint32 [N])
 * and visited (uint64 [N]): the per-chain values themselves, either may be NULL; the number of (slot, particle) states
 * added so far. */
int mjhmc_occupancy_read(mjhmc_occupancy* h, uint64_t* count, uint64_t* mass, uint64_t* from_count, uint64_t* from_mass,
                         uint64_t* trans, uint64_t* W_units, uint64_t* chains_by_switches, uint64_t* chains_by_cells,
                         uint32_t* switches, uint64_t* visited, int64_t* n_states);
/* labels: uint8 [n][N], the labels of the first n slots of the last block given to mjhmc_occupancy_accumulate (refused or
 * not), as the pass computed them (tests and inspection) */
int mjhmc_occupancy_read_labels(mjhmc_occupancy* h, int n, uint8_t* labels);
/* zero tables, totals, switches, visited and the carry; centres, radii and quantum stay */
int mjhmc_occupancy_reset(mjhmc_occupancy* h);
/* M, K and the slots the label scratch holds (the ring's at create: n of an accumulate call is at most this) */
int mjhmc_occupancy_info(mjhmc_occupancy* h, int* n_centres, int* n_dims, int* label_slots);

/* Kernel Stein discrepancy of one recorded ensemble against exp(-E), on the device (csrc/stein.hip, csrc/stein.hpp):
 * the one question the accumulators above leave open -- is the ensemble a sample of the target? -- answered from the
 * states and dE/dX at the states alone, with no normaliser and no reference sample (Gorham & Mackey 2017).  The base
 * kernel is the inverse multiquadric with exponent -1/2, k(x,y) = (c^2 + |x-y|^2)^(-1/2); the score is -G, G = dE/dX.
 * With r2 = sum_d (x_d-y_d)^2, dd = sum_d (Gx_d-Gy_d)(x_d-y_d), gg = sum_d Gx_d*Gy_d, q = c^2 + r2, t = 1/sqrt(q):
 *     k_p(x,y) = gg*t - t^3*dd + ndims*t^3 - 3*t^5*r2
 * every sum over d < ndims taken in ascending d from the differences themselves, in float64 (every state and gradient
 * type widened exactly), every product rounded before its sum; only + - * / sqrt, so the result is IEEE-rounded
 * throughout.  The exponent is fixed.
 * A handle belongs to the sampler it was created on (mjhmc_sampler_destroy frees every one still alive, and the handle
 * is INVALID from then on) and to the sample ring of that moment (a re-allocated ring invalidates it).  It owns one
 * dE/dX matrix and one E vector in the layout the energy family writes, and one (S, Sd) partial per 64 x 64 tile of
 * pairs, sized for N at create.
 * MJHMC_ERR_INVALID: NULL arguments, c not finite or <= 0 (both before the sampler is touched), no sample ring yet;
 * MJHMC_ERR_UNSUPPORTED: a host-evaluated energy (MJHMC_E_HOST has no device evaluation of dE/dX). */
typedef struct mjhmc_stein mjhmc_stein;
int mjhmc_stein_create(mjhmc_sampler* s, double c, mjhmc_stein** out);
/* The pass on ring slot x_slot, particles p < n_use, weights w_p of dwell-ring slot w_slot (w_slot == -1: unit weights;
 * the pairing of mjhmc_estimator_accumulate, so a jump sampler takes w_slot = x_slot + 1):
 *     out[0] = W  = sum_p w_p                        out[2] = S  = sum_{i,j} w_i w_j k_p(x_i, x_j)
 *     out[1] = W2 = sum_p w_p^2                      out[3] = Sd = sum_i w_i^2 k_p(x_i, x_i)
 * V = S / W^2 is the V-statistic (>= 0 up to rounding), U = (S - Sd) / (W^2 - W2) the unbiased one (mean zero under the
 * target).  On the sampler's stream: the sampler's own evaluation kernels on the slot (as the energy observables; not
 * counted, no sampler state, counter or random stream touched), the pair kernel, the finish kernel, ONE read-back.
 * Rows p >= n_use are selected out, never multiplied by zero: they may hold anything.  No floating-point atomic; the
 * order of every addition is a function of (ndims, n_use, state type, pitch) alone, so out[] is bit-identical from run
 * to run and does not depend on how the run was cut into blocks.
 * MJHMC_ERR_INVALID: NULL arguments, slots outside the ring, n_use outside [1, N], a ring re-allocated since create.
 * MJHMC_ERR_NONFINITE: a weight, a state or a gradient of a row p < n_use is not finite (or, all of them finite, a sum
 * overflows); the message says which, and out[] is left as it was. */
int mjhmc_stein_evaluate(mjhmc_stein* k, int x_slot, int w_slot, int64_t n_use, double out[4]);
/* frees the handle's device memory (NULL: nothing) */
int mjhmc_stein_destroy(mjhmc_stein* k);

/* Device control variates: the sums from which variance-reduced expectations are formed (csrc/crossmoments.hip).  With
 * g = dE/dX, integration by parts gives E_p[g] = 0 for every target p = exp(-E) / Z that vanishes at infinity, so g is a
 * vector of ndims control variates of known mean zero (the first-order zero-variance control variates of Mira, Solgi and
 * Imparato 2013): f - beta^T g with beta = Cov(g,g)^-1 Cov(g,f) has the expectation of f and the variance of the residual
 * of a linear regression of f on g.  For states x[k][p][:] (sample-ring slot x_slot0 + k, particle p < N), their gradients
 * g[k][p][:] (ndims values each, from the sampler's own evaluation kernels), the values b[k][p][:] of the same slot and
 * particle in the handle's ring (K values each: the sample ring itself, K = ndims, or the derived ring of a functionals),
 * weights w[k][p] and a shift vector cb of K doubles, the handle keeps on the device
 *   W = sum w,   Sg_d = sum w g_d,   S2g_d = sum w g_d^2,   Cgg_de = sum w g_d g_e        (the gradient about 0, its known mean)
 *   Sb_k = sum w (b_k - cb_k),   S2b_k = sum w (b_k - cb_k)^2,   Cgb_dk = sum w g_d (b_k - cb_k)
 * all in float64, every state, gradient and ring element widened exactly, no floating-point atomic; every slot is added to
 * the running totals separately and in a fixed order, so the sums are bit-identical from run to run on one device and do
 * not depend on how a run is cut into calls.  W, Sg, S2g, Cgg and Sb, S2b are the sums of mjhmc_estimator_accumulate on the
 * gradient matrix and on the ring; Cgb is a matrix-core pass of its own (64 x 64 blocks over the ndims x K rectangle).
 * The handle owns one dE/dX matrix and one E vector in the layout the energy family writes (as mjhmc_stein) and the
 * partials of the passes.  Ownership as for mjhmc_estimator: it belongs to the sampler (and to the functionals) it was
 * created on, mjhmc_sampler_destroy frees every one still alive and the handle is INVALID from then on; a re-allocated
 * sample ring or derived ring invalidates it.  The gradient evaluations are measurement, not sampling: no sampler state,
 * counter or random stream is touched.
 * MJHMC_ERR_INVALID: NULL arguments (before the sampler is touched), no sample ring yet, ndims > 512.
 * MJHMC_ERR_UNSUPPORTED: a host-evaluated energy (MJHMC_E_HOST has no device evaluation of dE/dX), a wide (multi-pass)
 * energy. */
typedef struct mjhmc_crossmoments mjhmc_crossmoments;
int mjhmc_crossmoments_create(mjhmc_sampler* s, mjhmc_crossmoments** out);
/* mjhmc_crossmoments_create with b the K values of the functionals' derived ring (which must exist): the sums W, Sg, S2g,
 * Cgg of the sampler's gradients, Sb, S2b of the K values and Cgb (ndims x K) between them; x_slot0 then counts slots of
 * BOTH rings (derived slot j holds the values of sample-ring slot j).  MJHMC_ERR_INVALID also for K > 512 and for a
 * functionals without a derived ring. */
int mjhmc_crossmoments_create_on(mjhmc_functionals* f, mjhmc_crossmoments** out);
/* cb: K finite doubles, NULL = zero (the state at create); the shift of the sums Sb, S2b and Cgb (the gradient sums Sg,
 * S2g, Cgg are about 0 always).  Only while the handle is empty (MJHMC_ERR_INVALID after an accumulate; reset first). */
int mjhmc_crossmoments_set_shift(mjhmc_crossmoments* h, const double* cb);
/* Adds the n states of slots [x_slot0, x_slot0 + n) to the sums W, Sg, S2g, Sb, S2b, Cgg, Cgb with the weights of dwell-ring
 * slots [w_slot0, w_slot0 + n), or unit weights for w_slot0 == -1: the pairing of mjhmc_estimator_accumulate (a jump
 * sampler takes w_slot0 = x_slot0 + 1).  The call's n * N weights are checked first; then, slot by slot, the evaluation of
 * dE/dX, the moment and covariance passes on it, the moment pass on the ring slot and the cross pass.  One read-back (one
 * synchronisation) per call.  Rows p >= N are never read.
 * MJHMC_ERR_INVALID: slots outside either ring, n < 1, a ring re-allocated since create.
 * MJHMC_ERR_NONFINITE: a weight that is not finite -- nothing of the call has been added; or a state, a gradient or an
 * energy of a row p < N that is not finite -- the message names the slot, the sums may hold the value, and the handle
 * refuses every further accumulate (MJHMC_ERR_INVALID) until mjhmc_crossmoments_reset. */
int mjhmc_crossmoments_accumulate(mjhmc_crossmoments* h, int x_slot0, int w_slot0, int n);
/* The only download, none of the pointers NULL: the sums W, Sg[ndims], S2g[ndims], Sb[K], S2b[K], Cgg[ndims * ndims]
 * (row-major, symmetric bit for bit), Cgb[ndims * K] (row-major, row d = gradient component d) and the number of
 * (slot, particle) states added so far. */
int mjhmc_crossmoments_read(mjhmc_crossmoments* h, double* W, double* Sg, double* S2g, double* Sb, double* S2b, double* Cgg,
                            double* Cgb, int64_t* n_states);
/* zero the sums W, Sg, S2g, Sb, S2b, Cgg, Cgb and the count, and lift the refusal a non-finite value left; the shift stays */
int mjhmc_crossmoments_reset(mjhmc_crossmoments* h);
/* ndims (the length of Sg; Cgg is ndims x ndims) and K (the length of Sb; the sums Cgb are ndims x K) */
int mjhmc_crossmoments_info(mjhmc_crossmoments* h, int* ndims, int* n_values);
/* frees the handle's device memory and its sums (NULL: nothing) */
int mjhmc_crossmoments_destroy(mjhmc_crossmoments* h);

/* Per-expert statistics of a linear-model energy over the recorded ensemble, on the device (csrc/pointwise.hip,
 * csrc/dense_lin_pointwise.hpp): what the accumulators above do not report on -- the DATA ROWS of a regression, not its
 * coefficients.  For an energy E(x) = sum_{j<K} f(u_j, j), u = W x + b (MJHMC_E_LINEAR_EXPR, square or tall), M <= 4 value
 * expressions h_m(u, j; p, q) -- float32 C expressions of exactly the variables the energy expression sees, j the global
 * expert index -- states x[k][p][:] (sample-ring slot x_slot0 + k, particle p < N) and weights w[k][p], the handle keeps
 * per value m and expert j, with t = (double)h_m(u_j(x[k][p]), j) widened exactly,
 *   W = sum w,   S1[m][j] = sum w t,   S2[m][j] = sum (w t) t,
 * and, for the values whose bit of lme_mask is set, the pair (mx, se)[m][j]: mx = max t over the states with w > 0,
 * se = sum w exp(t - mx), kept online (a new maximum rescales se by exp(mx_old - mx_new); two pairs merge as mx = max,
 * se = se1 exp(mx1 - mx) + se2 exp(mx2 - mx); an expert that has seen no weight reads (-inf, 0)): log(se / W) + mx is the
 * log of the weighted mean of exp(t), finite where a plain mean of exp underflows.  u is formed on the matrix cores by the
 * first GEMM of the force, block of experts by block of experts, and never leaves the chip: the N x K matrix of values is
 * not stored, the result is O(M K) numbers however long the run.  Sums in float64, every product rounded before its sum;
 * a state of weight 0 is selected out, never multiplied.  No floating-point atomic: particles are cut into strips of a
 * fixed number of tiles of 32 (mjhmc_pointwise_info), a strip's tiles are taken in ascending order, a slot's strips are
 * added in ascending order, slots are added to the totals in slot order -- bit-identical from run to run, for every grid,
 * and for every cut of a run into calls.
 * Ownership as for mjhmc_estimator: the handle belongs to the sampler it was created on, mjhmc_sampler_destroy frees every
 * one still alive and the handle is INVALID from then on; a re-allocated sample ring invalidates it.  The kernel is
 * compiled with hipRTC around the values when the handle is created (code objects are cached per process by source);
 * creating an energy compiles nothing of it.  No sampler state, counter or random stream is touched.
 * mjhmc_pointwise_check: the compile alone, for a model of ndims x nexperts, with no device.
 * MJHMC_ERR_INVALID: NULL arguments, no sample ring yet, no value or more than 4 (';'-separated), an empty value, mask
 * bits beyond the M values, an expression that does not compile (the message is the compiler's log);
 * MJHMC_ERR_UNSUPPORTED: an energy that is not MJHMC_E_LINEAR_EXPR (the message names its kind). */
typedef struct mjhmc_pointwise mjhmc_pointwise;
int mjhmc_pointwise_check(int ndims, int64_t nexperts, const char* values, const char* include_dir);
int mjhmc_pointwise_create(mjhmc_sampler* s, const char* values, unsigned lme_mask, const char* include_dir,
                           mjhmc_pointwise** out);
/* the number of values M, the number of experts K and the tiles of 32 particles in a strip (a constant of the library) */
int mjhmc_pointwise_info(mjhmc_pointwise* h, int* n_values, int64_t* nexperts, int* strip_tiles);
/* Adds the n states of slots [x_slot0, x_slot0 + n) to the sums with the weights of dwell-ring slots
 * [w_slot0, w_slot0 + n), or unit weights for w_slot0 == -1: the pairing of mjhmc_estimator_accumulate (a jump sampler
 * takes w_slot0 = x_slot0 + 1).  A float64 slot is narrowed to float32 rows first (what its force is given); a float32
 * slot is read in place.  One read-back (one synchronisation) per call.  Rows p >= N are never counted.
 * MJHMC_ERR_INVALID: slots outside the ring, n < 1, a ring re-allocated since create.
 * MJHMC_ERR_NONFINITE: a weight that is negative or not finite, or a value that is not finite at a state of positive
 * weight -- the message names the lowest such value index and, for it, the lowest expert.  A refused call has added
 * nothing: it worked on a copy of the sums. */
int mjhmc_pointwise_accumulate(mjhmc_pointwise* h, int x_slot0, int w_slot0, int n);
/* The only download, none of the pointers NULL: W, S1[M * K], S2[M * K], lme_max[M * K], lme_sum[M * K] (row m = value m;
 * (-inf, 0) where the mask did not ask) and the number of (slot, particle) states added so far. */
int mjhmc_pointwise_read(mjhmc_pointwise* h, double* W, double* S1, double* S2, double* lme_max, double* lme_sum,
                         int64_t* n_states);
/* the sums back to (0, 0, 0, (-inf, 0)) and the count to 0 */
int mjhmc_pointwise_reset(mjhmc_pointwise* h);
/* frees the handle's device memory and its sums (NULL: nothing) */
int mjhmc_pointwise_destroy(mjhmc_pointwise* h);

/* Per-group ("per data row") statistics of a GROUPED linear-model energy (mjhmc_energy_create_linear_grouped), on the
 * device (csrc/dense_lin_group_pointwise.hpp): what mjhmc_pointwise_create does for the experts of a square or tall model,
 * for the G groups of C members of a grouped one -- the rows of a softmax regression.  A value is a float32 C expression
 * evaluated at a grouped expert j = g C + c (the caller's index): it sees what a mjhmc_pointwise value sees (u, j, p[k],
 * q[m]) and three names more,
 *   lse  the group's log-sum-exp, formed exactly as the energy forms it (float32, contraction off: m = fmaxf over c
 *        ascending, t_c = expf(u_c - m), s = t_0 + ... + t_{C-1} ascending, lse = m + logf(s)),
 *   sm   the member's softmax t_c / s,
 *   c    the member index 0 .. C - 1 (int).
 * Bit m of member_mask gives the kind of value m.  Clear -- PER GROUP: the value of group g is the float32 sum of the
 * expression over the group's members in ascending c (s = c ? s + t : t), one number per data row; q[0]*(u - lse) with a
 * one-hot q[0] is the row's log-likelihood, q[0]*sm the probability of its observed class.  Set -- PER MEMBER: one number
 * per grouped expert, column g C + c; sm alone is the fitted class probabilities.  The handle's column count
 * (mjhmc_pointwise_info: nexperts) is G C when a value is per member and G otherwise; a per-group value fills the first G
 * columns of its row and the columns behind them read as empty: S1 = S2 = 0, (mx, se) = (-inf, 0).  The sums, the
 * log-mean-exp pairs asked for by lme_mask, their order, the selection of weight-0 states and the refusals of
 * mjhmc_pointwise_accumulate ("expert" in its message: the column) are those of the per-expert pass; mjhmc_pointwise_accumulate,
 * _reset, _read, _info and _destroy serve the handle unchanged.  The plain experts behind the groups (the prior) are not
 * reported on.  The kernel is compiled with hipRTC for the model's C and the values' kinds when the handle is created.
 * mjhmc_pointwise_grouped_check: the compile alone, for a model of ndims x nexperts with n_groups groups of group_size,
 * with no device; the model's arguments are checked as by mjhmc_linear_grouped_check.
 * MJHMC_ERR_INVALID: NULL arguments, no sample ring yet, no value or more than 4, an empty value, lme_mask or member_mask
 * bits beyond the M values, an expression that does not compile (the message is the compiler's log), group_size < 2,
 * n_groups < 1, G C > nexperts; MJHMC_ERR_UNSUPPORTED: an energy that is not a grouped linear model (the message names
 * mjhmc_pointwise_create, the pass of the other linear models), a state that is not float32 / float64, group_size > 16,
 * ndims > 512, more than 2^20 slots. */
int mjhmc_pointwise_grouped_check(int ndims, int64_t nexperts, int group_size, int64_t n_groups, const char* values,
                                  unsigned member_mask, const char* include_dir);
int mjhmc_pointwise_create_grouped(mjhmc_sampler* s, const char* values, unsigned lme_mask, unsigned member_mask,
                                   const char* include_dir, mjhmc_pointwise** out);

/* Data-row influence of a linear-model energy, on the device (csrc/influence.hip, csrc/dense_lin_values.hpp): what ties a
 * data row to a coefficient.  For an energy E(x) = sum_{j<K} f(u_j, j), u = W x + b (MJHMC_E_LINEAR_EXPR, square or tall),
 * ONE value expression h(u, j; p, q) -- a float32 C expression of the variables a mjhmc_pointwise value sees -- the experts
 * j0 <= j < j1, states x[k][p][:] (sample-ring slot x_slot0 + k, particle p < N), weights w[k][p] and two shifts cx (ndims
 * doubles) and ct (j1 - j0 doubles), the handle keeps on the device, with t_j = (double)h(u_j(x[k][p]), j) widened exactly,
 *   W = sum w,   Sx_d = sum w (x_d - cx_d),   S2x_d = sum w (x_d - cx_d)^2,
 *   St_j = sum w (t_j - ct_j),   S2t_j = sum w (t_j - ct_j)^2,   Cxt_dj = sum w x_d (t_j - ct_j)
 * all in float64: Cov(x_d, t_j) = Cxt_dj / W - (cx_d + Sx_d / W) (St_j / W).  x enters the cross sum about 0 and only t is
 * shifted: with ct near the mean of t the sum has nothing large to cancel whatever the offset of x.  With t the pointwise
 * log-likelihood of data row j, -Cov(x, t_j) is the first-order change of the posterior mean when row j is deleted.
 * The experts are walked in panels of one block of the model's P = 128, 256 or 512 experts (mjhmc_influence_info): per
 * slot and panel the first GEMM of the force forms u on the matrix cores, the values go to a float32 panel matrix
 * [particles][P] (0 where w == 0, selected, never multiplied), and the moment pass of mjhmc_estimator and the cross pass
 * of mjhmc_crossmoments run on it (a float64 state pairs with the panel widened exactly to float64).  The N x K matrix
 * of values is never stored; scratch is a function of (N, ndims, P), not of K.  No floating-point atomic, one fixed order
 * of sums; every slot is added to the totals separately and in slot order: bit-identical from run to run and for every cut
 * of a run into calls.  Cxt exists once, ndims x (j1 - j0) doubles: a model of 2^20 experts is taken in ranges.
 * Ownership as for mjhmc_estimator: the handle belongs to the sampler it was created on, mjhmc_sampler_destroy frees every
 * one still alive and the handle is INVALID from then on; a re-allocated sample ring invalidates it.  The kernel is
 * compiled with hipRTC around the value when the handle is created.  No gradient is evaluated; no sampler state, counter
 * or random stream is touched.
 * mjhmc_influence_check: the compile alone, for a model of ndims x nexperts, with no device.
 * MJHMC_ERR_INVALID: NULL arguments, no sample ring yet, an empty value, more than one value (a ';'), an expression that
 * does not compile (the message is the compiler's log), j0 < 0, j1 > K, j0 >= j1;
 * MJHMC_ERR_UNSUPPORTED: an energy that is not MJHMC_E_LINEAR_EXPR (the message names its kind);
 * MJHMC_ERR_HIP: the totals do not fit (the message gives their size in bytes). */
typedef struct mjhmc_influence mjhmc_influence;
int mjhmc_influence_check(int ndims, int64_t nexperts, const char* value, const char* include_dir);
int mjhmc_influence_create(mjhmc_sampler* s, const char* value, int64_t j0, int64_t j1, const char* include_dir,
                           mjhmc_influence** out);
/* cx: ndims finite doubles, ct: j1 - j0 finite doubles, NULL = zero for either (the state at create).  Only while the
 * handle is empty (MJHMC_ERR_INVALID after an accumulate; reset first). */
int mjhmc_influence_set_shift(mjhmc_influence* h, const double* cx, const double* ct);
/* ndims, the experts [j0, j1), the experts of a panel P and the bytes of scratch (the panel, the float32 rows and the
 * widened panel of a float64 state, the partials of the passes): the same for every K at equal particles, ndims and P */
int mjhmc_influence_info(mjhmc_influence* h, int* ndims, int64_t* j0, int64_t* j1, int* panel_experts, int64_t* scratch_bytes);
/* Adds the n states of slots [x_slot0, x_slot0 + n) to the sums with the weights of dwell-ring slots
 * [w_slot0, w_slot0 + n), or unit weights for w_slot0 == -1: the pairing of mjhmc_pointwise_accumulate (a jump sampler
 * takes w_slot0 = x_slot0 + 1).  The call's n * N weights are checked first; then, slot by slot, the moments of the state
 * and, panel by panel, the values, their moments and the cross pass.  One read-back (one synchronisation) per call.
 * MJHMC_ERR_INVALID: slots outside the ring, n < 1, a ring re-allocated since create.
 * MJHMC_ERR_NONFINITE: a weight that is negative or not finite -- nothing of the call has been added; or a value that is
 * not finite at a state of positive weight -- the message names the lowest such expert, the sums may hold the value, and
 * the handle refuses every further accumulate (MJHMC_ERR_INVALID) until mjhmc_influence_reset. */
int mjhmc_influence_accumulate(mjhmc_influence* h, int x_slot0, int w_slot0, int n);
/* None of the pointers NULL: W, Sx[ndims], S2x[ndims], St[j1 - j0], S2t[j1 - j0] and the number of (slot, particle)
 * states added so far. */
int mjhmc_influence_read(mjhmc_influence* h, double* W, double* Sx, double* S2x, double* St, double* S2t, int64_t* n_states);
/* The columns j0 <= ja < jb <= j1 of Cxt into Cxt_out[ndims * (jb - ja)] (row-major, row d = state dimension d): a caller
 * pages a wide range through a buffer of its own size.  MJHMC_ERR_INVALID for a range outside [j0, j1). */
int mjhmc_influence_read_cross(mjhmc_influence* h, int64_t ja, int64_t jb, double* Cxt_out);
/* zero the sums and the count, and lift the refusal a value that is not finite left; the shifts stay */
int mjhmc_influence_reset(mjhmc_influence* h);
/* frees the handle's device memory and its sums (NULL: nothing) */
int mjhmc_influence_destroy(mjhmc_influence* h);

/* Fair sample paths on a uniform time grid, kept on the device (csrc/timegrid.hip): the one result the weighted
 * accumulators above cannot give -- a fair sample with its time order kept.  The reference's sample(resample=True)
 * (markov_jump_hmc.py:293-338) pools particles and steps into one weighted draw ("preserve_order has no effect if
 * resample is enabled"), and its figures take the autocorrelation of sample(resample=False), the embedded chain, whose
 * samples its own docstring calls biased.  The unbiased object is the jump process x_p(t): chain p sits in state k for
 * its holding time.  A time grid samples it at t_j = j * dt, j < n_grid, into a GRID RING of n_grid slots in the sample
 * ring's own slot layout and dtype (stored elements copied verbatim), zeroed at create.  Per chain p < N it keeps a
 * clock T[p] (float64, 0 at create) and a cursor j[p] (int32, 0 at create).
 * Ownership as for mjhmc_estimator: a time grid belongs to the sampler it was created on, mjhmc_sampler_destroy frees
 * every one still alive and the handle is INVALID from then on.  It has its own storage: a re-allocated sample ring does
 * not invalidate it.
 * MJHMC_ERR_INVALID: n_grid < 1, dt not finite or <= 0, no sample ring yet.  A grid the device cannot hold fails as
 * mjhmc_ring_alloc does (the sizes in mjhmc_last_error()) and leaves nothing behind. */
typedef struct mjhmc_timegrid mjhmc_timegrid;
int mjhmc_timegrid_create(mjhmc_sampler* s, int n_grid, double dt, mjhmc_timegrid** out);
int mjhmc_timegrid_destroy(mjhmc_timegrid* tg);
/* The n states of ring slots [x_slot0, x_slot0 + n) with the holding times of dwell-ring slots [w_slot0, w_slot0 + n),
 * or unit holding times for w_slot0 == -1: the pairing of mjhmc_estimator_accumulate (a jump sampler takes w_slot0 =
 * x_slot0 + 1).  For every chain p < N, k = 0 .. n - 1 ascending:
 *     w  = dwell[w_slot0 + k][p]                          (w_slot0 == -1: w = 1.0)
 *     Tn = T[p] + w                                       one rounded float64 addition
 *     while j[p] < n_grid and (double)j[p] * dt < Tn:     one rounded multiplication
 *         grid[j[p]][p][:] = x[x_slot0 + k][p][:];  j[p] += 1
 *     T[p] = Tn
 * Grid point t_j takes the state with T_k <= t_j < T_{k+1}; a state of zero holding time is never emitted, one that
 * spans several grid points is emitted for each.  The clock is a sequential sum from the stored value: grid, T and j do
 * not depend on how a run is cut into blocks and are bit-identical from run to run.  Rows p >= N of the sample ring, the
 * dwell ring and the grid are neither read nor written.
 * MJHMC_ERR_INVALID: slots outside either ring, n < 1.  MJHMC_ERR_NONFINITE: a holding time that is not finite or is
 * negative (checked on the device ahead of the pass); grid, clocks and cursors are as before the call.  Reading that
 * flag back is the call's only synchronisation, and unit holding times need none. */
int mjhmc_timegrid_accumulate(mjhmc_timegrid* tg, int x_slot0, int n, int w_slot0);
/* *covered = min_p j[p], the grid slots complete for every chain; *max_filled = max_p j[p] (integer reductions) */
int mjhmc_timegrid_progress(mjhmc_timegrid* tg, int* covered, int* max_filled);
/* T (N doubles) and j (N int32) of the chains; either pointer may be NULL */
int mjhmc_timegrid_read_clocks(mjhmc_timegrid* tg, double* T_host, int32_t* j_host);
/* grid slots [slot0, slot0 + n) in float64, the layouts of mjhmc_ring_read: (D, n*N) time-major if stacked==0,
 * (D, N, n) if stacked==1.  Slots a chain has not reached hold zeros for it. */
int mjhmc_timegrid_read(mjhmc_timegrid* tg, int slot0, int n, int stacked, double* host_out);
/* mjhmc_ring_autocor along the time axis of grid slots [slot0, slot0 + n): the unnormalised lag sums (n float64).
 * MJHMC_ERR_INVALID when slot0 + n > covered: a slot some chain has not reached is no sample. */
int mjhmc_timegrid_autocor(mjhmc_timegrid* tg, int slot0, int n, int linear, double* host_out);
/* clocks and cursors to zero and the grid zeroed; n_grid and dt stay */
int mjhmc_timegrid_reset(mjhmc_timegrid* tg);

/* The leapfrog operator on caller-supplied states: HMCState.leapfrog (n_steps = 1) and HMCState.L
 * (n_steps = num_leapfrog_steps) of mjhmc/samplers/hmc_state.py:86-100, in the reference's literal operation order
 * (half kicks not merged, every product rounded before its sum).  X, V and the outputs are (ndims, n) float64 C order
 * (EX_out / EV_out: n values); EX_out, EV_out, dEdX_out may be NULL.  X_out / V_out may alias X / V.
 * PRODUCT_OF_T / SPARSE_CODE run their tile kernels' integrator (float32 / bfloat16 state, half kicks between drifts
 * merged; figures/poe_fig.py:58-76 integrates snapshots of a ProductOfT sampler this way). */
int mjhmc_leapfrog(mjhmc_energy* e, int dtype, const double* X, const double* V, int64_t n, double eps, int n_steps,
                   double* X_out, double* V_out, double* EX_out, double* EV_out, double* dEdX_out);

/* The two helpers of the jump process as operators on caller arrays (mjhmc/misc/utils.py; the samplers' kernels use
 * the same device functions, `wait_time` and `first_min3` of csrc/jump_math.hpp):
 *   draw_from (utils.py:31-50): waiting times of exponential clocks.  out[i] = inf where rates[i] == 0, otherwise
 *     (1 / rates[i]) * unit_exp[i] -- numpy's exponential(scale = 1/rate) is scale * standard_exponential(), so with the
 *     standard exponentials the caller drew the result is bit-identical.  A non-finite rate is the reference's
 *     ValueError: out[i] = NaN there, *first_bad = the lowest such index, return MJHMC_ERR_NONFINITE (no bad rate:
 *     *first_bad = -1, return 0).
 *   min_idx (utils.py:15-28): which[j] = argmin over the k rows of draws[k][n] (row-major) in column j, the FIRST
 *     minimum on ties and a NaN counting as the minimum, as np.argmin does; the caller lists the columns per row. */
int mjhmc_draw_from(mjhmc_ctx* ctx, const double* rates, const double* unit_exp, int64_t n, double* out,
                    int64_t* first_bad);
int mjhmc_min_idx(mjhmc_ctx* ctx, const double* draws, int k, int64_t n, int32_t* which);

/* Autocorrelation along the time axis of ring slots [slot0, slot0 + n):
 *   out[k] = sum_{d < ndims, particle < N} sum_t x_t * x_{t+k},   k = 0 .. n-1   (n float64 to the host)
 * linear == 0: t + k wraps modulo n.  out / out[0] is fft_autocor(samples) of mjhmc/misc/autocor.py:37-49
 *              (fftn along time, |.|^2, ifftn, mean over dims and particles, normalise by lag 0).
 * linear != 0: the sum stops at t + k < n.  out[k] / (ndims * N * (n - k)) is the lag product mean
 *              np.mean(samples[:, :, :-k] * samples[:, :, k:]) of slow_autocorrelation (:177-211) and of the
 *              brute-force branch of autocorrelation (:52-117).
 * The sums are returned unnormalised so that ranks holding column shards can add theirs before dividing. */
int mjhmc_ring_autocor(mjhmc_sampler* s, int slot0, int n, int linear, double* host_out);
/* The same for a host array laid out like the reference's samples, [n_dims, n_batch, n_samples] C order,
 * i.e. n_series = n_dims * n_batch contiguous series of n_samples float64 (no sampler needed). */
int mjhmc_autocor(mjhmc_ctx* ctx, const double* samples, int64_t n_series, int n_samples, int linear,
                  double* host_out);

/* Centred linear lag sums PER DIMENSION along the time axis of n consecutive slots (csrc/lagcov.hip): what the integrated
 * autocorrelation time and the effective sample size of every coordinate are made of.  They replace the host computation
 * of mjhmc/misc/autocor.py:177-211 (slow_autocorrelation: the lag-product means of the downloaded [n_dims, n_batch,
 * n_samples] array, pooled over dimensions and taken about zero) by one streaming pass per band of 32 lags:
 *     u[t][p][d] = (double)x[t][p][d] - shift[d]                                 one rounded float64 subtraction
 *     A_out[k][d] = sum_{p < N} sum_{t = 0}^{n - 1 - k} u[t][p][d] * u[t + k][p][d]    k = 0 .. max_lag, (max_lag + 1, ndims) C order
 *     S_out[d]    = sum_{p < N} sum_{t < n} u[t][p][d]                                 ndims float64; S_out may be NULL
 * shift: ndims float64 on the host, NULL for zeros (the two give the same bits).  The sums are linear in time, not
 * circular, and unnormalised, so that ranks holding column shards add theirs; A_out[k][d] / (N * (n - k)) is the lag-k
 * product mean of dimension d.  Rows p >= N and columns d >= ndims are not read.  There is no floating-point atomic: the
 * order of addition depends on (N, ndims, n, max_lag) alone and the result is bit-identical from run to run.
 * MJHMC_ERR_INVALID (with a message): slots outside the ring or grid, n < 1, max_lag outside [0, min(n - 1, 256)], a shift
 * entry that is not finite.
 * mjhmc_grid_lagcov: grid slots [slot0, slot0 + n) of a time grid; refuses slot0 + n > covered as mjhmc_timegrid_autocor.
 * mjhmc_ring_lagcov: ring slots [slot0, slot0 + n) of a sampler (the embedded chain; a discrete-time sampler's fair path).
 * mjhmc_lagcov:      a host array laid out as for mjhmc_autocor, [n_dims, n_batch, n_samples] C order, re-tiled on the
 *                    device into a temporary time-major view that the same kernels read (no sampler needed). */
int mjhmc_grid_lagcov(mjhmc_timegrid* tg, int slot0, int n, int max_lag, const double* shift, double* A_out, double* S_out);
int mjhmc_ring_lagcov(mjhmc_sampler* s, int slot0, int n, int max_lag, const double* shift, double* A_out, double* S_out);
int mjhmc_lagcov(mjhmc_ctx* ctx, const double* samples, int n_dims, int64_t n_batch, int n_samples, int max_lag,
                 const double* shift, double* A_out, double* S_out);

/* ---- several GPUs: one process per GPU, particle COLUMNS sharded over the ranks ------------------
 * The reference is single-process; its particles are independent chains (mjhmc/samplers/hmc_state.py works column-wise
 * everywhere), so nothing is exchanged on the data path until sample() returns (markov_jump_hmc.py:150-173,293-338).
 * The communicator is RCCL (xGMI between the GPUs of a node), loaded with dlopen on first use.  Every rank calls every
 * collective in the same order.  Pointers are host memory unless stated. */
#define MJHMC_COMM_ID_BYTES 128
typedef enum { MJHMC_OP_SUM = 0, MJHMC_OP_MIN = 1, MJHMC_OP_MAX = 2 } mjhmc_reduce_op;
/* rank 0 draws the id (ncclGetUniqueId) and hands the 128 bytes to the other ranks by any host channel (file, socket) */
int mjhmc_comm_unique_id(void* id);
int mjhmc_comm_create(mjhmc_ctx* ctx, int rank, int world, const void* id, mjhmc_comm** out);
int mjhmc_comm_destroy(mjhmc_comm* c);
/* 0 when librccl can be loaded and has every entry point the communicator uses, MJHMC_ERR_COMM otherwise (needs no
 * device and enters no collective: the ranks of a job can agree on a fallback BEFORE any of them calls mjhmc_comm_create) */
int mjhmc_comm_available(void);
/* the number of ranks of the communicator as RCCL reports it (ncclCommCount) */
int mjhmc_comm_count(mjhmc_comm* c, int* count);
/* host values, in place: integer bookkeeping (l/f/r counts, E_count / dEdX_count increments: sums), the number of
 * iterations every rank committed before a non-finite rate (min: the reference retries the WHOLE batch,
 * markov_jump_hmc.py:376-389), lag sums of the autocorrelation, elapsed times (max) */
int mjhmc_comm_allreduce_i64(mjhmc_comm* c, int64_t* inout, int64_t n, int op);
int mjhmc_comm_allreduce_f64(mjhmc_comm* c, double* inout, int64_t n, int op);
/* e.g. the np.random.random draws of the resampling step (markov_jump_hmc.py:325), drawn on rank 0 */
int mjhmc_comm_bcast(mjhmc_comm* c, void* inout, size_t nbytes, int root);
/* recv = rank 0's block, rank 1's block, ... (nbytes_per_rank[r] bytes each; send: this rank's block) */
int mjhmc_comm_allgatherv(mjhmc_comm* c, const void* send, const int64_t* nbytes_per_rank, void* recv);
/* THE data-path collective, device to device: ring slots [slot0, slot0 + n) of every rank's sampler are all-gathered
 * and re-tiled on the receiving GPU; host_out is the sample block of the UNSHARDED run, columns in global particle
 * order: (D, n * N_total) time-major if stacked == 0 (np.concatenate(axis=1), markov_jump_hmc.py:170-173,336-338),
 * (D, N_total, n) if stacked != 0 (np.stack(axis=-1)).  particles_per_rank[world]: the column shard sizes.
 * host_out == NULL: this rank takes part in the collective and keeps nothing -- no re-tile, no download (a caller that
 * wants the block on ONE rank passes NULL on the others: at C4 / n = 10 every rank's copy is 2.56 GB over its PCIe link);
 * the same holds for mjhmc_comm_allgather_columns. */
int mjhmc_comm_allgather_ring(mjhmc_comm* c, mjhmc_sampler* s, int slot0, int n, int stacked,
                              const int64_t* particles_per_rank, double* host_out);
/* resampled columns (markov_jump_hmc.py:322-328): every rank gathers the n_local ring columns IT owns (local pool indices
 * slot * N_local + column, as mjhmc_ring_gather takes them) on the device, the blocks are all-gathered, host_out is
 * (D, sum columns_per_rank) with rank 0's columns first; the caller puts them in sample order. */
int mjhmc_comm_allgather_columns(mjhmc_comm* c, mjhmc_sampler* s, const int64_t* local_idx, int64_t n_local,
                                 const int64_t* columns_per_rank, double* host_out);

/* Device time of the last mjhmc_iterate call in milliseconds: ONE HIP-event pair on the sampler's stream
 * brackets its whole launch sequence (first to last jump kernel); jump_kernel_ms == total_ms and
 * n_jump_launches is the number of sampling_iteration attempts it covers. */
int mjhmc_last_timing(mjhmc_sampler* s, double* total_ms, double* jump_kernel_ms, int* n_jump_launches);

/* The event pair is two marker packets on the stream (~8 us of a call: 3 % of a one-iteration call at C4's size).
 * on = 0: calls record nothing and mjhmc_last_timing keeps reporting the last recorded call; on by default.  (The
 * reference has no counterpart: its callers time `sampling_iteration()` with the wall clock; the drop-in classes of
 * mjhmc_amd.samplers switch it off.) */
int mjhmc_set_timing(mjhmc_sampler* s, int on);

/* Stream synchronisation (bench harness). */
int mjhmc_sync(mjhmc_sampler* s);

#ifdef __cplusplus
}
#endif
#endif /* MJHMC_HIP_H */
