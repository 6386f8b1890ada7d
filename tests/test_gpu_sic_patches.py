"""GPU: the bf16 matrix-core SparseImageCode kernels (csrc/dense_sic.hip: sic_eval_kernel, sic_jump_kernel with its
inverse-L items, sic_fix_kernel, sic_leap_kernel) against the NumPy oracle on the same Philox streams at the patch counts
where the cut of a 32-column tile changes.  n_patches = P decides the kernel's whole column bookkeeping: ppt = 32 // P
particles share a tile, cpt = ppt * P columns work, the idle columns are clamped onto column cpt - 1, group_total adds
colsum[g0 .. g0 + P) per particle, and the patches come from the LDS copy up to kYLds = 4 of them and from global memory
beyond.  The other oracle tests of these kernels run P = 1 nearly everywhere and P = 2, 3, 9 in a few places at
epsilon = 2^-4; 1 and 9 are repeated here as the anchor to them.  The machinery is theirs: sic_problem, to_bf16,
check_iteration / check_control_iteration / resync of tests/helpers.py, the oracle's mixed-precision restatement
(operand_rounding = to_bf16, state_rounding of the state type) resynchronised to the device state after every compared
iteration.

What a patch count reaches (tests.helpers.sic_tile_layout restates the cut; tests/test_sic_patches_cpu.py pins it):

  P    ppt  working / idle  patches from  N    the edge
  1    32   32 / 0          LDS           70   anchor to the existing tests (the benchmark's)
  2    16   32 / 0          LDS           33   smallest group sum
  3    10   30 / 2          LDS           10   first idle columns
  4     8   32 / 0          LDS           17   last LDS-staged count (P <= kYLds)
  5     6   30 / 2          global        13   first global-memory count
  8     4   32 / 0          global         9   exact fill
  9     3   27 / 5          global         7   anchor (the reference's default)
  10    3   30 / 2          global         7   same ppt as 9, other cut
  11    2   22 / 10         global         5   many idle columns with two particles
  16    2   32 / 0          global         5   last count with two particles per tile
  17    1   17 / 15         global         5   first with one; idle columns clamp onto column 16
  31    1   31 / 1          global         4   one idle column
  32    1   32 / 0          global         4   the particle is the tile

N is 2 ppt + 1 (three tiles, the last ragged and holding one particle) at P = 2, 4, 5, 8, 10, 11, 16; 70 at P = 1 (three
tiles, six particles in the last, as the ProductOfT width module); where 2 ppt + 1 would leave too few particles for the
near-tie cap to mean anything, 10 at P = 3 (one full tile), 7 at P = 9, 5 at P = 17 and 4 at P = 31, 32 (at ppt = 1 every
tile holds exactly one particle: those batches are listed as exact fills, EXACT_FILL); also N = 1 and N = 2 ppt at
P = 4, 5, 17, 32 (single evaluations) and at P = 5, 17 (MarkovJumpHMC).  P N <= 140 columns keeps the oracle side of a
case at a few seconds.

Cases.  The model of the existing tests: sic_problem(0) (1024 atoms, NB = 4 accumulator blocks) or sic_problem(3, 512
atoms, NB = 2), X0 = a0 + 0.2 randn rounded to the state type, lambda = 0.01.
  single evaluation   every P, both priors, both dictionaries, both state types, at the table's N and at N = 1 (N = 2 ppt
                      too at P = 4, 5, 17, 32), at values the state type holds: E and dE/dX against the restatement
                      (2e-5 / 2e-4; dE/dX after the provable bf16 flips of the residual, below) and the autograd graph
                      (4e-3 / 2e-2), the energy-only call, the tick-0 momentum of all P n_coeffs dims against the oracle's
                      normals (bf16 state 3e-2; float32 state the box_muller_f32 gate of DESIGN section 6,
                      2^-20 max(r, 1), against the Box-Muller transform of the float32-rounded uniforms that
                      normal_pair_f32 hands it), EV against the stored momentum (1e-5)
  MarkovJumpHMC       every P at L = 6, bf16 state, 1024 atoms, beta = 0.2, 4 iterations; 512 atoms at P = 1, 4, 5, 16, 17,
                      32; float32 state at P = 1, 4, 5, 17, 32; the Laplace prior at P = 1, 5; L = 1 and 2 (sic_trajectory
                      merges the half kicks: at L = 1 the first and the closing scale are one pass) at P = 1, 5, 17 with
                      both dictionaries; N = 1 (24 iterations) and N = 2 ppt at P = 5, 17; after the compared iterations of
                      P = 5, 17, 32 a sample(3) whose ring slots are P n_coeffs wide
  ControlHMC          P = 5, 17, 32 in bf16 and P = 5 in float32 (the batch-wide refresh draws normals per (pid, patch)),
                      seed CONTROL_SEED: the first from 47 up whose refresh gate opens within the first two iterations
  ContinuousTimeHMC   P = 5, in the shape of tests/test_gpu_dense_parity.py::test_pot_continuous_time_sampler_vs_oracle
  replay mode         P = 5, 17: MarkovJumpHMC and ControlHMC with recorded normals of P 1024 rows
  HMCState.L()        on a snapshot at P = 5, 17, 32 and with 512 atoms at P = 5: sic_leap_kernel and the dE/dX it hands out
(The part split at one particle per tile is the 'sic_p17' case of
tests/test_gpu_dense_parity.py::test_split_launches_equal_single_launches.)

Sharper than check_iteration alone.  Its bars are relative to max |H|, and |H| is dominated by the kinetic energy (about
n_coeffs / 2 per patch): at P = 32 max |H| is about 16 000 against EX of 10^2 .. 10^3, so a potential energy with one
patch column missing from group_total would pass e_rtol = 5e-4.  After every compared iteration, for ALL particles (not
only the agreeing ones), the device's stored EX is therefore compared with the restatement evaluated at the device's own
stored X (2e-5 of the largest, the single-evaluation bar) and EV with half the sum of the stored V squared (1e-5): no
bf16 flip noise, relative to the quantity itself (`check_stored_energies`).

The gradient's one discontinuity.  The scaled residual R / P enters the second product rounded to bf16, and R is a
float32 sum of 1024 (512) products: of the 256 P N residual elements of an evaluation a few lie so close to the midpoint
of two bf16 values that float32 accumulation in another order rounds to the other one.  The gradient of that
(particle, patch) then moves by one bf16 ulp of that element times a dictionary row -- up to 5.2e-4 of the largest
gradient element at the shapes here, a step and not an error of the kernel; the float32-accumulating restatement shows
the same against the float64 one (2.3e-4 at P = 2, N = 33, 512 atoms: the reference alone misses the 2e-4 bar there).
`explain_residual_flips` moves the reference by exactly those steps and no others: only elements whose exact R / P lies
within 4 x the float32 spread of the residual (float32- against float64-accumulating restatement, no device output) of
a rounding boundary, only to the neighbour across it, whole steps chosen by a least-squares fit of the difference in
the candidates' dictionary rows.  The 2e-4 bar then holds with three decades to spare (3.3e-7 at most), which is also
what shows that nothing but such flips was in the difference.

Step sizes, fixed with the oracle alone (`choose_eps`): a power of two (the restatement rests on "rounding the scaled
residual equals scaling the rounded residual"), the smallest of {2^-5, 2^-4, 2^-3, 2^-2} at which the ORACLE's own run
over the compared iterations stays finite, makes at least two each of L, F and R, and makes an R before the last
iteration (so that an inverse-L item and the fix kernel run).  ControlHMC: accepted, rejected, refreshed;
ContinuousTimeHMC: FL, F, R.  TABLE lists, per case, epsilon, the oracle's tallies (l, f, r, fl) and the float32 spread;
tests/test_sic_patches_cpu.py recomputes all of it without a GPU and shows on the reference alone that the float32- and
the float64-accumulating restatements decide differently on at most tie_ceiling(N) particles of any compared iteration.

Tolerances.  The existing bars -- delta_rel = e_rtol = 5e-4, x_tol = 1 / 128; single evaluations 2e-5 / 2e-4 -- wherever
they hold.  A case's allowance is max(bar, 4 x its spread), the spread being the largest difference, in
check_iteration's measures, between the oracle's proposals with accumulate_dtype = float64 and float32 from the states
of the oracle's own run (`spread_of_state`; no device output involved).  x_tol is never widened: with bf16 state the
x measure is quantised -- two end points that differ before rounding by far less than an ulp are stored equal or one bf16
ulp apart, and one ulp is at most 2^-7 = 1 / 128 of the value -- so the bar already is "one flip", and 4 x a flip would
allow four.  WIDER holds the cases whose allowance exceeds a bar.

Every case prints the layout it reached (ppt, idle columns, patch source, NB, state type), epsilon, the oracle's
tallies, its spread and its allowance; single evaluations print their two errors.  The device's tallies are asserted
equal to the table's whenever no near tie occurred -- between device and compared oracle, and between the compared
oracle (which restarts every iteration from the device's state: a bf16 ulp here and there off the oracle's own) and the
oracle's own run, which the test makes alongside (`OwnRun`).

Measured on an MI355X.  Spreads: delta_rel and e_rtol 9.8e-10 .. 5.6e-5 (4 x: 2.2e-4, below the bars: WIDER is empty),
x 0 .. 3.7e-3 (bf16 ulps).  Single evaluations: E within 2.2e-7, dE/dX within 3.3e-7 after 0 .. 6 flips per evaluation
(312 in 189 evaluations; before them up to 5.2e-4, beyond 2e-4 in 18).  Stored EX against the stored X within 2.5e-7 and
EV within 2.6e-7 in every compared iteration of every case; the leap kernel's dE/dX within 2.5e-7.  No near tie between
device and compared oracle in any case; the compared oracle leaves the path of the own run in two (ControlHMC P = 5
float32 state: one accept decision; MarkovJumpHMC P = 5, N = 1: the near tie tests/test_sic_patches_cpu.py finds in its
inputs), every other case makes the moves of the table.

Sensitivity.  With `j < P` replaced by `j < (P < 9 ? P : 9)` in group_total (csrc/dense_sic.hip: a particle's energies
lose the patch columns from the tenth on; no memory access changes) the 38 SparseImageCode tests of
tests/test_gpu_parity.py and tests/test_gpu_dense_parity.py all pass, and all 47 cases of this module at P >= 10 fail
(single evaluations, MarkovJumpHMC at every L, N, dictionary and state type, ControlHMC, replay mode, the leap operator)
with the 'sic_p17' split case, while its 60 cases at P <= 9 pass."""
import functools

import numpy as np
import pytest

from oracle import mjhmc_oracle as orc
from tests.helpers import (check_control_iteration, check_iteration, resync, sic_problem, sic_tile_layout, sic_tiles,
                           to_bf16)
from tests.test_gpu_pot_widths import LIVE_DH, MARGIN, _decision, _other_decision, _proposals

gpu = pytest.mark.gpu
np.seterr(all='ignore')

LMBDA = 0.01
SEEDS = {'mj': 51, 'control': 47, 'ct': 43}        # of the device and of the oracle; 'control': CONTROL_SEED
CONTROL_SEED = 47       # the first seed from 47 up whose batch-wide refresh gate opens within the first two iterations
BETAS = {'mj': 0.2, 'control': 0.6, 'ct': 0.3}      # the existing SparseImageCode tests' / the ProductOfT continuous-time test's
CLASSES = {'mj': 'MarkovJumpHMC', 'control': 'ControlHMC', 'ct': 'ContinuousTimeHMC'}
EPS_GRID = (2.0 ** -5, 2.0 ** -4, 2.0 ** -3, 2.0 ** -2)
MIN_MOVES = 2           # of each of L, F and R in the oracle's own run
N_ITER = 4
BARS = (5e-4, 1.0 / 128, 5e-4)                      # (delta_rel, x_tol, e_rtol)
EVAL_BARS = (2e-5, 2e-4)

PATCHES = (1, 2, 3, 4, 5, 8, 9, 10, 11, 16, 17, 31, 32)
N_OF = {1: 70, 2: 33, 3: 10, 4: 17, 5: 13, 8: 9, 9: 7, 10: 7, 11: 5, 16: 5, 17: 5, 31: 4, 32: 4}
ATOMS_512 = (1, 4, 5, 16, 17, 32)
FLOAT32 = (1, 4, 5, 17, 32)
LAPLACE = (1, 5)
SHORT = (1, 5, 17)                                  # L = 1 and 2, both dictionaries
SMALL_BATCH = (5, 17)                               # N = 1 and N = 2 ppt (MarkovJumpHMC)
EVAL_SMALL = (4, 5, 17, 32)                         # N = 2 ppt (single evaluations; N = 1 at every P)
FUSED = (5, 17, 32)                                 # sample(3) after the compared iterations
CONTROL = ((5, 'bfloat16'), (17, 'bfloat16'), (32, 'bfloat16'), (5, 'float32'))
REPLAY = (5, 17)
LEAP = ((5, 1024), (17, 1024), (32, 1024), (5, 512))
STATES = ('bfloat16', 'float32')


def to_f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


ROUNDING = {'bfloat16': to_bf16, 'float32': to_f32}


def ppt_of(P):
    return sic_tile_layout(P)[0]


# batches whose last tile is full (every other (P, N) of the module has a ragged last tile): N = 2 ppt, ten particles at
# P = 3 (one tile), and every batch at one particle per tile
EXACT_FILL = ({(P, 2 * ppt_of(P)) for P in EVAL_SMALL} | {(3, 10)} | {(P, N_OF[P]) for P in (17, 31, 32)} |
              {(P, 1) for P in (17, 31, 32)})


def case(kind, P, N=None, L=6, nc=1024, state='bfloat16', cauchy=True):
    return (kind, P, N_OF[P] if N is None else N, L, nc, state, cauchy)


MJ_CASES = ([case('mj', P) for P in PATCHES] + [case('mj', P, nc=512) for P in ATOMS_512] +
            [case('mj', P, state='float32') for P in FLOAT32] + [case('mj', P, cauchy=False) for P in LAPLACE] +
            [case('mj', P, L=L, nc=nc) for P in SHORT for nc in (1024, 512) for L in (1, 2)] +
            [case('mj', P, N=N) for P in SMALL_BATCH for N in (1, 2 * ppt_of(P))])
CONTROL_CASES = [case('control', P, state=st) for P, st in CONTROL]
CT_CASE = case('ct', 5)


def n_iterations(key):
    """compared iterations: 4; 24 with one particle (so that every kind of move can occur at all); 5 for ContinuousTimeHMC
    (the ProductOfT test's)"""
    if key[0] == 'ct':
        return 5
    return 24 if key[2] == 1 else N_ITER


# (kind, P, N, L, n_coeffs, state type, Cauchy prior): (epsilon, the oracle's own (l, f, r, fl) over the compared iterations,
# the float32 spread of (delta_rel, x_tol, e_rtol))
TABLE = {
    ('mj', 1, 70, 6, 1024, 'bfloat16', True): (2.0 ** -5, (244, 12, 24, 0), (3.1e-05, 0.002, 3.1e-05)),
    ('mj', 2, 33, 6, 1024, 'bfloat16', True): (2.0 ** -5, (114, 6, 12, 0), (1.2e-05, 0.0018, 1.2e-05)),
    ('mj', 3, 10, 6, 1024, 'bfloat16', True): (2.0 ** -4, (32, 3, 5, 0), (1.3e-05, 0.0019, 1.3e-05)),
    ('mj', 4, 17, 6, 1024, 'bfloat16', True): (2.0 ** -4, (56, 3, 9, 0), (3.5e-06, 0.0018, 3.5e-06)),
    ('mj', 5, 13, 6, 1024, 'bfloat16', True): (2.0 ** -4, (44, 3, 5, 0), (8.8e-06, 0.0019, 8.8e-06)),
    ('mj', 8, 9, 6, 1024, 'bfloat16', True): (2.0 ** -4, (29, 2, 5, 0), (2.3e-06, 0.0019, 2.4e-06)),
    ('mj', 9, 7, 6, 1024, 'bfloat16', True): (2.0 ** -4, (24, 2, 2, 0), (3.2e-06, 0.002, 3.2e-06)),
    ('mj', 10, 7, 6, 1024, 'bfloat16', True): (2.0 ** -3, (17, 6, 5, 0), (6.1e-06, 0.0036, 6.2e-06)),
    ('mj', 11, 5, 6, 1024, 'bfloat16', True): (2.0 ** -4, (14, 2, 4, 0), (6.7e-07, 0.00082, 5.8e-07)),
    ('mj', 16, 5, 6, 1024, 'bfloat16', True): (2.0 ** -5, (14, 2, 4, 0), (4.4e-07, 0.00079, 4.4e-07)),
    ('mj', 17, 5, 6, 1024, 'bfloat16', True): (2.0 ** -5, (13, 2, 5, 0), (9.3e-08, 0.00039, 9.3e-08)),
    ('mj', 31, 4, 6, 1024, 'bfloat16', True): (2.0 ** -5, (6, 3, 7, 0), (1.4e-09, 4.9e-05, 1.1e-09)),
    ('mj', 32, 4, 6, 1024, 'bfloat16', True): (2.0 ** -5, (6, 3, 7, 0), (1.5e-07, 0.00084, 1.5e-07)),
    ('mj', 1, 70, 6, 512, 'bfloat16', True): (2.0 ** -5, (250, 5, 25, 0), (4.5e-05, 0.0018, 4.7e-05)),
    ('mj', 4, 17, 6, 512, 'bfloat16', True): (2.0 ** -4, (59, 2, 7, 0), (7.4e-06, 0.0027, 8.7e-06)),
    ('mj', 5, 13, 6, 512, 'bfloat16', True): (2.0 ** -5, (44, 2, 6, 0), (2.1e-06, 0.0009, 2e-06)),
    ('mj', 16, 5, 6, 512, 'bfloat16', True): (2.0 ** -3, (14, 2, 4, 0), (8.4e-07, 0.00093, 8.2e-07)),
    ('mj', 17, 5, 6, 512, 'bfloat16', True): (2.0 ** -2, (10, 5, 5, 0), (6e-06, 0.002, 6.1e-06)),
    ('mj', 32, 4, 6, 512, 'bfloat16', True): (2.0 ** -5, (7, 3, 6, 0), (1.4e-09, 1.5e-06, 1.1e-09)),
    ('mj', 1, 70, 6, 1024, 'float32', True): (2.0 ** -5, (249, 7, 24, 0), (5e-06, 2.6e-05, 5e-06)),
    ('mj', 4, 17, 6, 1024, 'float32', True): (2.0 ** -4, (58, 2, 8, 0), (1.5e-06, 1.8e-05, 1.6e-06)),
    ('mj', 5, 13, 6, 1024, 'float32', True): (2.0 ** -3, (38, 6, 8, 0), (1.5e-06, 7.2e-05, 1.3e-06)),
    ('mj', 17, 5, 6, 1024, 'float32', True): (2.0 ** -3, (12, 3, 5, 0), (7.8e-08, 8.4e-06, 1.1e-07)),
    ('mj', 32, 4, 6, 1024, 'float32', True): (2.0 ** -3, (10, 2, 4, 0), (2.3e-08, 4.6e-06, 2.1e-08)),
    ('mj', 1, 70, 6, 1024, 'bfloat16', False): (2.0 ** -5, (246, 10, 24, 0), (3.5e-05, 0.0019, 3.1e-05)),
    ('mj', 5, 13, 6, 1024, 'bfloat16', False): (2.0 ** -4, (43, 4, 5, 0), (3.4e-06, 0.002, 3.3e-06)),
    ('mj', 1, 70, 1, 1024, 'bfloat16', True): (2.0 ** -5, (249, 6, 25, 0), (5.6e-06, 0.0009, 5.6e-06)),
    ('mj', 1, 70, 2, 1024, 'bfloat16', True): (2.0 ** -5, (249, 6, 25, 0), (5.6e-05, 0.0037, 5.6e-05)),
    ('mj', 1, 70, 1, 512, 'bfloat16', True): (2.0 ** -5, (248, 5, 27, 0), (4.6e-05, 0.0018, 4.6e-05)),
    ('mj', 1, 70, 2, 512, 'bfloat16', True): (2.0 ** -5, (250, 5, 25, 0), (3.2e-05, 0.0018, 3.2e-05)),
    ('mj', 5, 13, 1, 1024, 'bfloat16', True): (2.0 ** -5, (39, 7, 6, 0), (2.1e-08, 0.00011, 2.2e-08)),
    ('mj', 5, 13, 2, 1024, 'bfloat16', True): (2.0 ** -5, (44, 2, 6, 0), (8e-08, 0.00022, 8.2e-08)),
    ('mj', 5, 13, 1, 512, 'bfloat16', True): (2.0 ** -5, (38, 8, 6, 0), (4.6e-09, 2.2e-07, 3e-09)),
    ('mj', 5, 13, 2, 512, 'bfloat16', True): (2.0 ** -5, (44, 3, 5, 0), (3.9e-08, 0.00011, 4.3e-08)),
    ('mj', 17, 5, 1, 1024, 'bfloat16', True): (2.0 ** -5, (10, 5, 5, 0), (3.4e-07, 0.00078, 3.3e-07)),
    ('mj', 17, 5, 2, 1024, 'bfloat16', True): (2.0 ** -5, (10, 5, 5, 0), (1.4e-09, 1.5e-06, 1.1e-09)),
    ('mj', 17, 5, 1, 512, 'bfloat16', True): (2.0 ** -5, (11, 4, 5, 0), (1.1e-09, 0.0, 7.7e-10)),
    ('mj', 17, 5, 2, 512, 'bfloat16', True): (2.0 ** -5, (10, 5, 5, 0), (9.8e-10, 0.00012, 8.4e-10)),
    ('mj', 5, 1, 6, 1024, 'bfloat16', True): (2.0 ** -3, (18, 3, 3, 0), (1.1e-05, 0.0022, 1.1e-05)),
    ('mj', 5, 12, 6, 1024, 'bfloat16', True): (2.0 ** -4, (39, 4, 5, 0), (3.1e-06, 0.0019, 3.1e-06)),
    ('mj', 17, 1, 6, 1024, 'bfloat16', True): (2.0 ** -5, (19, 2, 3, 0), (3.5e-07, 0.001, 3.4e-07)),
    ('mj', 17, 2, 6, 1024, 'bfloat16', True): (2.0 ** -3, (3, 2, 3, 0), (8.4e-07, 0.00098, 8.4e-07)),
    ('control', 5, 13, 6, 1024, 'bfloat16', True): (2.0 ** -5, (49, 3, 26, 0), (1.6e-06, 0.00088, 1.6e-06)),
    ('control', 17, 5, 6, 1024, 'bfloat16', True): (2.0 ** -5, (15, 5, 10, 0), (3.9e-07, 0.00085, 3.9e-07)),
    ('control', 32, 4, 6, 1024, 'bfloat16', True): (2.0 ** -4, (14, 2, 8, 0), (2e-07, 0.0017, 2e-07)),
    ('control', 5, 13, 6, 1024, 'float32', True): (2.0 ** -4, (44, 8, 26, 0), (3.1e-07, 2.5e-05, 2.9e-07)),
    ('ct', 5, 13, 6, 1024, 'bfloat16', True): (2.0 ** -3, (0, 40, 2, 23), (1.6e-05, 0.0034, 1.5e-05)),
}
# the cases whose allowance is wider than a bar: ((delta_rel, x_tol, e_rtol) allowed, the spread it comes from)
WIDER = {
}

EPS = {k: v[0] for k, v in TABLE.items()}
TALLIES = {k: v[1] for k, v in TABLE.items()}
SPREAD = {k: v[2] for k, v in TABLE.items()}


# ---------------------------------------------------------------------------------------------
# the model, the references and the device samplers
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _problem(P, nc):
    B, imgs, a0 = sic_problem(0 if nc == 1024 else 3, n_patches=P, n_coeffs=nc)
    return B, imgs, a0


def _x0(P, N, nc, state):
    a0 = _problem(P, nc)[2]
    return ROUNDING[state](a0[:, None] + 0.2 * np.random.RandomState(100 * P + N).randn(P * nc, N))


@functools.lru_cache(maxsize=None)
def _energy(P, nc, cauchy, acc=np.float64):
    B, imgs, _ = _problem(P, nc)
    return orc.SparseImageCode(B, imgs[:, :P].T, lmbda=LMBDA, cauchy=cauchy, operand_rounding=to_bf16, accumulate_dtype=acc)


def _reference(key, eps):
    kind, P, N, L, nc, state, cauchy = key
    kw = dict(epsilon=eps, beta=BETAS[kind], num_leapfrog_steps=L, rng=orc.PhiloxRNG(SEEDS[kind], np.arange(N)),
              state_rounding=ROUNDING[state])
    if kind != 'control':
        kw['resample'] = False
    o = getattr(orc, CLASSES[kind])(_energy(P, nc, cauchy), _x0(P, N, nc, state), **kw)
    o.state.V[:] = ROUNDING[state](o.state.V)       # what the state holds of the tick-0 normals
    o.state.refresh_EV()
    return o


def _distribution(P, N, nc, state, cauchy, X0):
    from mjhmc_amd.misc.distributions import SparseImageCode
    B, imgs, _ = _problem(P, nc)
    return SparseImageCode(n_patches=P, n_batches=N, cauchy=cauchy, n_basis=nc, basis=B, imgs=imgs, init=X0, state_dtype=state)


def _device(key, eps, **extra):
    from mjhmc_amd.samplers import markov_jump_hmc as M
    kind, P, N, L, nc, state, cauchy = key
    d = _distribution(P, N, nc, state, cauchy, _x0(P, N, nc, state))
    kw = dict(resample=False) if kind != 'control' else {}
    kw.update(extra)
    return getattr(M, CLASSES[kind])(distribution=d, epsilon=eps, beta=BETAS[kind], num_leapfrog_steps=L,
                                     seed=SEEDS[kind], **kw)


def _layout(P, N, nc, state):
    ppt, cpt, idle, lds = sic_tile_layout(P)
    tiles, last = sic_tiles(P, N)
    return ('P=%d ppt=%d %d working / %d idle columns, patches from %s, NB=%d, %s state, N=%d: %d tiles, %d in the last'
            % (P, ppt, cpt, idle, 'LDS' if lds else 'global memory', nc // 256, state, N, tiles, last))


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


# ---------------------------------------------------------------------------------------------
# measured on the oracle alone (tests/test_sic_patches_cpu.py runs these without a GPU)
# ---------------------------------------------------------------------------------------------
def spread_of_state(o, key):
    """The float32 spread of the oracle's current state: the largest differences between its proposals (L z and L F z)
    with the float32- and with the float64-accumulating restatement, in check_iteration's measures -- of the energy
    differences H0 - H(proposal) and of EX and EV over max(1, max |H0|), of X and V over max(1, max |X|) and
    max(1, max |V|) -- over the proposals that can be taken at all (|H0 - H| <= LIVE_DH)."""
    _, P, N, L, nc, state, cauchy = key
    H64, p64 = _proposals(o, _energy(P, nc, cauchy, np.float64))
    H32, p32 = _proposals(o, _energy(P, nc, cauchy, np.float32))
    scale = max(1.0, float(np.abs(H64).max()))
    d_delta = d_x = d_e = 0.0
    for (dh64, X64, V64, EX64, EV64), (dh32, X32, V32, EX32, EV32) in zip(p64, p32):
        live = np.isfinite(dh32) & (np.abs(dh64) <= LIVE_DH)
        if not live.any():
            continue
        d_delta = max(d_delta, float(np.abs(dh32 - dh64)[live].max()) / scale)
        d_x = max(d_x, float(np.abs(X32 - X64)[:, live].max()) / max(1.0, float(np.abs(X64[:, live]).max())),
                  float(np.abs(V32 - V64)[:, live].max()) / max(1.0, float(np.abs(V64[:, live]).max())))
        d_e = max(d_e, float(np.abs(EX32 - EX64)[live].max()) / scale, float(np.abs(EV32 - EV64)[live].max()) / scale)
    return np.array([d_delta, d_x, d_e])


@functools.lru_cache(maxsize=None)
def oracle_run(key, eps, spread=True):
    """The oracle's own run of a case from its initial state (the device sampler's seed), no device involved: the tallies
    (l, f, r, fl) over the compared iterations, whether everything stayed finite, whether an R was made before the last
    iteration and, with `spread`, per iteration the number of particles on which the float32 and the float64
    accumulation decide differently and the float32 spread (the largest over the iterations)."""
    kind, P, N, L, nc, state, cauchy = key
    n_iter = n_iterations(key)
    o = _reference(key, eps)
    e32, e64 = _energy(P, nc, cauchy, np.float32), _energy(P, nc, cauchy, np.float64)
    sp, ties, finite, early_r = np.zeros(3), [], True, False
    for t in range(n_iter):
        if spread:
            sp = np.maximum(sp, spread_of_state(o, key))
            if kind == 'mj':
                exps = np.asarray(o.rng.stream.unit_exponentials(o.rng.tick), dtype=np.float64)
                ties.append(int(np.sum(_decision(o, e32, exps) != _decision(o, e64, exps))))
            else:
                ties.append(int(np.sum(_other_decision(o, e32, CLASSES[kind]) != _other_decision(o, e64, CLASSES[kind]))))
        o.sampling_iteration()
        finite = finite and bool(np.isfinite(o.state.X).all() and np.isfinite(o.state.V).all() and
                                 np.isfinite(o.state.H()).all())
        if t == n_iter - 2:
            early_r = o.r_count > 0
    return dict(counts=(o.l_count, o.f_count, o.r_count, o.fl_count), finite=finite, early_r=early_r or n_iter == 1,
                ties=ties, spread=sp, n_iter=n_iter)


def rule_ok(run):
    """the step-size rule: finite, at least MIN_MOVES each of L (ControlHMC: accepted, ContinuousTimeHMC: FL), F and R, and an
    R before the last iteration"""
    l, f, r, fl = run['counts']
    return run['finite'] and min(l + fl, f, r) >= MIN_MOVES and run['early_r']


def choose_eps(key):
    """the smallest step size of EPS_GRID at which the oracle's own run meets the rule, and that run"""
    for eps in EPS_GRID:
        run = oracle_run(key, eps, False)
        if rule_ok(run):
            return eps, run
    raise AssertionError(('no step size of the grid meets the rule', key))


def allowance(spread):
    """max(the existing bar, MARGIN x the float32 spread) for delta_rel and e_rtol; x_tol stays the bar (one bf16 ulp: the
    module docstring)"""
    return (max(BARS[0], MARGIN * float(spread[0])), BARS[1], max(BARS[2], MARGIN * float(spread[2])))


def tolerances(key):
    tol = WIDER[key][0] if key in WIDER else BARS
    return dict(zip(('delta_rel', 'x_tol', 'e_rtol'), tol))


def _describe(key):
    kind, P, N, L, nc, state, cauchy = key
    return ('%s %s L=%d eps=2^%d %s; oracle tallies l / f / r / fl = %s; float32 spread %s, allowed %s'
            % (CLASSES[kind], _layout(P, N, nc, state), L, int(np.log2(EPS[key])), 'Cauchy' if cauchy else 'Laplace',
               ' / '.join('%d' % c for c in TALLIES[key]), ' '.join('%.2g' % v for v in SPREAD[key]),
               ' '.join('%.2g' % v for v in tolerances(key).values())))


def _tallies(o):
    return (o.l_count, o.f_count, o.r_count, o.fl_count)


class OwnRun(object):
    """The oracle's own run of the case (never resynced: the run TABLE records) next to the compared one.  The compared
    oracle restarts every iteration from the DEVICE's state, which is the own run's only within the allowance (a bf16 ulp
    here and there), so a decision can fall the other way without device and compared oracle ever disagreeing.
    `on_path`: the two oracles have made the same moves so far -- only then are the device's tallies the table's."""

    def __init__(self, key, eps):
        self.o, self.on_path = _reference(key, eps), True

    def step(self, compared):
        self.o.sampling_iteration()
        self.on_path = self.on_path and _tallies(self.o) == _tallies(compared)


def check_stored_energies(s, en, tag):
    """The device's stored EX against the restatement at the device's own stored X, and EV against the stored V, for all
    particles: relative to the quantity itself, no bf16 flip noise.  Returns the two errors."""
    X, V = s.state.X, s.state.V
    eEX = rel(s.state.EX[0], en.E_val(X)[0])
    eEV = rel(s.state.EV[0], 0.5 * np.sum(V * V, axis=0))
    assert eEX < EVAL_BARS[0] and eEV < 1e-5, (tag, 'stored EX / EV against the stored state', eEX, eEV)
    return eEX, eEV


# ---------------------------------------------------------------------------------------------
# the gradient's one discontinuity: the scaled residual R / P enters the second product rounded to bf16
# ---------------------------------------------------------------------------------------------
FLIP_MARGIN = 4.0       # x the float32 spread of the residual: how close to a rounding boundary an element must lie


def bf16_neighbour(r, up):
    """the next bf16 values above (where `up`) or below the bf16 values r (r != 0; integer steps of the bit pattern cross
    binades)"""
    r = np.asarray(r, dtype=np.float32)
    u = (r.view(np.uint32) >> np.uint32(16)).astype(np.int64)
    u = np.where((r > 0) == up, u + 1, u - 1)
    return (u.astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)


def explain_residual_flips(G, en, en32, Xs):
    """The restatement's dE/dX at Xs, moved by the bf16 flips of the scaled residual that the device can PROVABLY have taken.
    The residual R = B a - y is a sum of 1024 (512) products; R / P is rounded to bf16 before the second product.  Where
    the exact R / P lies within FLIP_MARGIN x the float32 spread of the residual (the largest |R32 - R64| / P between the
    float32- and the float64-accumulating restatement: the reference alone) of the midpoint of two bf16 values, float32
    accumulation in another order may round to the other one, and the gradient of that (particle, patch) moves by exactly
    (neighbour - rounded) x the dictionary row: a step, not an error of 2e-4.  Only such elements may be flipped, only to
    that neighbour, whole: per (particle, patch) the difference to the device's `G` is fitted by the candidates' dictionary
    rows, and a step is taken where the fit is nearer to it than to zero.  Returns (the reference, flips taken,
    candidates)."""
    P, C = en.Y.shape[0], en.B.shape[1]
    R, _ = en._resid(Xs)
    Rs = R / P                                                   # (P, img, n), exact
    window = FLIP_MARGIN * float(np.abs(en32._resid32(Xs).astype(np.float64) - R).max()) / P
    r0 = to_bf16(Rs)
    ref = en.dEdX_val(Xs).reshape(P, C, -1).copy()
    Gd = np.asarray(G, dtype=np.float64).reshape(P, C, -1)
    nb = bf16_neighbour(r0, Rs > r0)
    at_boundary = (r0 != 0) & (np.abs(Rs - 0.5 * (r0 + nb)) <= window)
    taken, candidates = 0, int(at_boundary.sum())
    for p, n in sorted(set(zip(*np.nonzero(at_boundary.any(axis=1))))):
        rows = np.nonzero(at_boundary[p, :, n])[0]
        steps = nb[p, rows, n] - r0[p, rows, n]
        # the device's column minus the reference's, in terms of the candidates' dictionary rows; a step is taken whole or not
        fit = np.linalg.lstsq(en.B[rows, :].T, Gd[p, :, n] - ref[p, :, n], rcond=None)[0]
        take = np.abs(fit - steps) < np.abs(fit)
        ref[p, :, n] += (steps * take).dot(en.B[rows, :])
        taken += int(take.sum())
    return ref.reshape(np.shape(G)), taken, candidates


def normals_of_float32_uniforms(seed, D, N):
    """The tick-0 normals as normal_pair_f32 (csrc/dense_pot.hpp) forms them, in float64: the Box-Muller transform of the two
    u53() uniforms of pair j ROUNDED TO float32 (dims 2j, 2j + 1), and the radius r of every dim's pair -- the inputs of
    box_muller_f32, whose gate is 2^-20 max(r, 1)"""
    from oracle.philox import PhiloxStream, philox4x32_10, u53
    st = PhiloxStream(seed, np.arange(N))
    npairs = (D + 1) // 2
    slots = np.arange(npairs, dtype=np.uint64)[:, None]
    w0, w1, w2, w3 = philox4x32_10(st.pid[None, :], 0, 0, slots, st.k0, st.k1)
    u1, u2 = to_f32(u53(w0, w1)), to_f32(u53(w2, w3))
    r = np.sqrt(-2.0 * np.log(u1))
    Z = np.empty((2 * npairs, N))
    Z[0::2], Z[1::2] = r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)
    return Z[:D], np.repeat(r, 2, axis=0)[:D]


# ---------------------------------------------------------------------------------------------
# single evaluations: sic_eval_kernel
# ---------------------------------------------------------------------------------------------
def eval_batches(P):
    return (N_OF[P], 1) + ((2 * ppt_of(P),) if P in EVAL_SMALL else ())


@gpu
@pytest.mark.parametrize('state', STATES)
@pytest.mark.parametrize('nc', [1024, 512])
@pytest.mark.parametrize('P', PATCHES)
def test_single_evaluation(P, nc, state):
    """d.E / d.dEdX against the restatement at the bars of tests/test_gpu_dense_parity.py (2e-5 of the largest energy, 2e-4
    of the largest gradient element) and against the reference's forward graph under autograd (4e-3 / 2e-2), both priors;
    the tick-0 momentum of a sampler against the oracle's normals in all P n_coeffs dims and EV against the stored
    momentum."""
    from oracle import autograd_energies as ag
    from mjhmc_amd.samplers.markov_jump_hmc import MarkovJumpHMC
    B, imgs, a0 = _problem(P, nc)
    D = P * nc
    for N in eval_batches(P):
        # values the state type holds: what the device stores is then the input itself (a float64 value rounded to bf16 in one
        # step and through float32 can differ by an ulp)
        X = Xs = ROUNDING[state](a0[:, None] + 0.3 * np.random.RandomState(8 + N).randn(D, N))
        for cauchy in (True, False):
            d = _distribution(P, N, nc, state, cauchy, X)
            en = _energy(P, nc, cauchy)
            E, G = d.E(X), d.dEdX(X)
            assert E.shape == (1, N) and G.shape == (D, N)
            ref, flips, candidates = explain_residual_flips(G, en, _energy(P, nc, cauchy, np.float32), Xs)
            eE, eG, eG_raw = rel(E[0], en.E_val(Xs)[0]), rel(G, ref), rel(G, en.dEdX_val(Xs))
            print('eval %s %s: E %.3g dEdX %.3g (%.3g before %d bf16 flips of the residual, %d of %d elements at a rounding boundary)'
                  % (_layout(P, N, nc, state), 'Cauchy' if cauchy else 'Laplace', eE, eG, eG_raw, flips, candidates, 256 * P * N))
            assert eE < EVAL_BARS[0] and eG < EVAL_BARS[1], (P, N, nc, state, cauchy, eE, eG, eG_raw, flips, candidates)
            Ea, ga = ag.sparse_image_code_per_column(B, imgs[:, :P].T, LMBDA, cauchy, X)
            assert rel(E[0], Ea) < 4e-3 and rel(G, ga) < 2e-2, (P, N, nc, state, cauchy, rel(E[0], Ea), rel(G, ga))
            assert np.array_equal(d.E(X), E), 'the energy-only call'
            assert (d.E_count, d.dEdX_count) == (2 * N, N)
        s = MarkovJumpHMC(distribution=d, epsilon=2.0 ** -4, beta=0.2, num_leapfrog_steps=6, seed=SEEDS['mj'], resample=False)
        Z = orc.PhiloxRNG(SEEDS['mj'], np.arange(N)).initial_normals(D, N)
        V = s.state.V
        assert V.shape == (D, N)
        if state == 'bfloat16':
            assert np.abs(V - Z).max() < 3e-2, (P, N, nc, 'tick-0 momentum', np.abs(V - Z).max())
        else:       # normal_pair_f32 rounds the two uniforms to float32 first; box_muller_f32's gate is about what follows
            Zf, r = normals_of_float32_uniforms(SEEDS['mj'], D, N)
            assert (np.abs(V - Zf) <= 2.0 ** -20 * np.maximum(r, 1.0)).all(), (P, N, nc, 'tick-0 momentum', np.abs(V - Zf).max())
            assert np.abs(V - Z).max() < 3e-2
        eEV = rel(s.state.EV[0], 0.5 * np.sum(V * V, axis=0))
        assert eEV < 1e-5, (P, N, nc, state, 'EV of the stored momentum', eEV)
        assert rel(s.state.EX[0], en.E_val(s.state.X)[0]) < EVAL_BARS[0]


# ---------------------------------------------------------------------------------------------
# MarkovJumpHMC
# ---------------------------------------------------------------------------------------------
def _ids(cases):
    return ['P%d-N%d-L%d-%d-%s-%s' % (k[1], k[2], k[3], k[4], k[5], 'cauchy' if k[6] else 'laplace') for k in cases]


@gpu
@pytest.mark.parametrize('key', MJ_CASES, ids=_ids(MJ_CASES))
def test_iterations_match_oracle(key):
    """sampling_iteration() through check_iteration with a resync after every iteration: transitions equal or provable near
    ties, X, V, EX, EV, the cache flags and the dwelling times within the case's allowance; after every iteration the
    stored EX and EV of all particles against the stored state (check_stored_energies); l + f + r, and the table's
    tallies while no near tie has occurred."""
    kind, P, N, L, nc, state, cauchy = key
    eps, n_iter, tol = EPS[key], n_iterations(key), tolerances(key)
    tag0 = _describe(key)
    print(tag0)
    s, o, own = _device(key, eps), _reference(key, eps), OwnRun(key, eps)
    en = o.energy
    if state == 'bfloat16':
        assert np.array_equal(s.state.X, o.state.X) and np.abs(s.state.V - o.state.V).max() < 3e-2, (tag0, 'tick 0')
    else:
        assert np.array_equal(s.state.X, o.state.X) and np.allclose(s.state.V, o.state.V, rtol=0, atol=2.0 ** -17), (tag0, 'tick 0')
    worst = np.maximum(np.zeros(2), check_stored_energies(s, en, tag0 + ', tick 0'))
    resync(s, o)
    ties = 0
    for t in range(n_iter):
        ties += check_iteration(s, o, tag='%s, iteration %d' % (tag0, t), **tol)
        own.step(o)
        assert s.l_count + s.f_count + s.r_count == (t + 1) * N, (tag0, t, 'l + f + r')
        worst = np.maximum(worst, check_stored_energies(s, en, '%s, iteration %d' % (tag0, t)))
        resync(s, o)
    assert _tallies(own.o) == TALLIES[key], (tag0, 'the table no longer holds the tallies of the oracle run')
    if ties == 0:
        assert (s.l_count, s.f_count, s.r_count) == (o.l_count, o.f_count, o.r_count), (tag0, 'tallies')
        if own.on_path:
            assert (s.l_count, s.f_count, s.r_count, 0) == TALLIES[key], (tag0, 'the device run does not make the moves of the table')
    print('%s: %d near ties in %d transitions, %s the path of the own run; device L / F / R = %d / %d / %d; stored EX %.3g EV %.3g'
          % (tag0, ties, n_iter * N, 'on' if own.on_path else 'OFF', s.l_count, s.f_count, s.r_count, worst[0], worst[1]))
    X = s.state.X
    assert np.array_equal(X, ROUNDING[state](X)) and (np.abs(X - to_bf16(X)).max() == 0) == (state == 'bfloat16'), (tag0, 'the state type')
    if P in FUSED and key == case('mj', P):
        out = s.sample(3)                           # ring slots of P * n_coeffs-wide rows
        assert out.shape == (P * nc, 3 * N) and np.isfinite(out).all() and np.array_equal(out[:, -N:], s.state.X), (tag0, 'sample(3)')
        check_stored_energies(s, en, tag0 + ', after sample(3)')


# ---------------------------------------------------------------------------------------------
# the other sampler families
# ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('key', CONTROL_CASES, ids=_ids(CONTROL_CASES))
def test_control_hmc_matches_oracle(key):
    """ControlHMC (Metropolis accept, flip, the batch-wide momentum refresh with normals per (pid, patch)) through
    check_control_iteration."""
    kind, P, N, L, nc, state, cauchy = key
    eps, tol = EPS[key], tolerances(key)
    tag0 = _describe(key)
    print(tag0)
    s, o, own = _device(key, eps), _reference(key, eps), OwnRun(key, eps)
    assert (s.beta, s.p_r, s.p_flip) == (o.beta, o.p_r, o.p_flip)
    en = o.energy
    resync(s, o)
    ties = 0
    for t in range(N_ITER):
        ties += check_control_iteration(s, o, tag='%s, iteration %d' % (tag0, t), **tol)
        own.step(o)
        if ties == 0:
            assert (s.l_count, s.f_count, s.r_count, s.fl_count) == (o.l_count, o.f_count, o.r_count, o.fl_count), (tag0, t)
        assert s.l_count + s.f_count == (t + 1) * N and s.fl_count == 0, (tag0, t, 'every particle flips: l (accepted) + f (rejected)')
        check_stored_energies(s, en, '%s, iteration %d' % (tag0, t))
        resync(s, o)
    assert ties <= 1, (tag0, 'near ties', ties)
    assert _tallies(own.o) == TALLIES[key], (tag0, 'the table no longer holds the tallies of the oracle run')
    if ties == 0 and own.on_path:
        assert (s.l_count, s.f_count, s.r_count, s.fl_count) == TALLIES[key], (tag0, 'the device run does not make the moves of the table')
    print('%s: %d near ties, %s the path of the own run; l / f / r / fl = %d / %d / %d / %d'
          % (tag0, ties, 'on' if own.on_path else 'OFF', s.l_count, s.f_count, s.r_count, s.fl_count))
    assert s.r_count > 0, (tag0, 'no momentum refresh in the compared iterations')


@gpu
def test_continuous_time_hmc_matches_oracle():
    """ContinuousTimeHMC at P = 5, in the form of tests/test_gpu_dense_parity.py::test_pot_continuous_time_sampler_vs_oracle."""
    key = CT_CASE
    kind, P, N, L, nc, state, cauchy = key
    eps, tol = EPS[key], tolerances(key)
    print(_describe(key))
    s, o, own = _device(key, eps), _reference(key, eps), OwnRun(key, eps)
    resync(s, o)
    for t in range(n_iterations(key)):
        s.sampling_iteration()
        o.sampling_iteration()
        own.step(o)
        # the F clock has rate 1 and R rate p_r: only the FL clock sees energies (the CPU module: no near tie in the inputs)
        assert (s.fl_count, s.f_count, s.r_count) == (o.fl_count, o.f_count, o.r_count), t
        assert s.fl_count + s.f_count + s.r_count == (t + 1) * N
        assert np.abs(s.state.X - o.state.X).max() <= tol['x_tol'] * max(1.0, np.abs(o.state.X).max())
        assert np.abs(s.state.V - o.state.V).max() <= tol['x_tol'] * max(1.0, np.abs(o.state.V).max())
        assert np.allclose(s.dwelling_times, o.dwelling_times, rtol=max(1e-3, 4 * tol['delta_rel'] * float(np.abs(o.state.H()).max())))
        check_stored_energies(s, o.energy, 'continuous time, iteration %d' % t)
        resync(s, o)
    assert _tallies(own.o) == TALLIES[key], 'the table no longer holds the tallies of the oracle run'
    print('continuous time: %s the path of the own run; l / f / r / fl = %d / %d / %d / %d'
          % ('on' if own.on_path else 'OFF', s.l_count, s.f_count, s.r_count, s.fl_count))
    if own.on_path:
        assert (s.l_count, s.f_count, s.r_count, s.fl_count) == TALLIES[key], ('the device run does not make the moves of the table',
                                                                              (s.l_count, s.f_count, s.r_count, s.fl_count))


# ---------------------------------------------------------------------------------------------
# replay mode: every draw is the caller's; the noise rows are laid out N * P rows deep
# ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('cls_name', ['MarkovJumpHMC', 'ControlHMC'])
@pytest.mark.parametrize('P', REPLAY)
def test_replay_mode(P, cls_name):
    """As tests/test_gpu_dense_parity.py::test_dense_kernels_in_replay_mode with recorded normals of P * 1024 rows, at the step
    size and the allowance of the counter-RNG case of the same P."""
    from mjhmc_amd.samplers import markov_jump_hmc as M
    base = case('mj', P)
    _, _, N, _, nc, state, cauchy = base
    eps, tol, D, T = EPS[base], tolerances(base), P * nc, 4
    rs = np.random.RandomState(123 + P)
    X0 = _x0(P, N, nc, state)
    d, en = _distribution(P, N, nc, state, cauchy, X0), _energy(P, nc, cauchy)
    kw = dict(epsilon=eps, beta=0.3, num_leapfrog_steps=5)
    V0 = to_bf16(rs.randn(D, N))
    normals = [to_bf16(rs.randn(D, N)) for _ in range(T)]          # (what the device stores of them)
    tag0 = 'replay %s %s eps=2^%d' % (cls_name, _layout(P, N, nc, state), int(np.log2(eps)))
    print(tag0)
    if cls_name == 'ControlHMC':
        u_acc, u_flip = [rs.rand(N) for _ in range(T)], [rs.rand(N) for _ in range(T)]
        u_r = [0.9, 0.1, 0.8, 0.05]                                # recorded gate uniforms: p_r = 0.178 opens the second and the last
        s = M.ControlHMC(distribution=d, Vinit=V0, seed=1, **kw)
        fired = [u < s.p_r for u in u_r]
        assert fired == [False, True, False, True]
        o = orc.ControlHMC(en, X0, V0=V0, rng=orc.ReplayRNG(normals=[normals[t] for t in range(T) if fired[t]],
                                                            uniforms=[v for t in range(T) for v in (u_acc[t], u_flip[t], u_r[t])]),
                           state_rounding=to_bf16, **kw)
        resync(s, o)
        for t in range(T):
            s.sampling_iteration(replay=[(normals[t] if fired[t] else np.zeros((D, N)), np.concatenate([u_acc[t], u_flip[t], [u_r[t]]]))])
            o.sampling_iteration()
            tr = s._dev.read(8)
            acc_o, flip_o = np.isin(np.arange(N), o.last_fl_idx), np.isin(np.arange(N), o.last_flip_idx)
            assert np.array_equal(((tr >> 1) & 1).astype(bool), flip_o), t
            same = (tr & 1).astype(bool) == acc_o
            assert (~same).sum() <= 1, t                          # (an accept decision within the kernel's energy error of a tie)
            xs = max(1.0, float(np.abs(o.state.X).max()))
            assert np.abs(s.state.X[:, same] - o.state.X[:, same]).max() <= tol['x_tol'] * xs, t
            assert np.abs(s.state.V[:, same] - o.state.V[:, same]).max() <= tol['x_tol'] * max(1.0, float(np.abs(o.state.V).max())), t
            check_stored_energies(s, en, '%s, iteration %d' % (tag0, t))
            resync(s, o)
        assert s.r_count > 0
        return
    exps = [rs.standard_exponential((3, N)) for _ in range(T)]
    s = M.MarkovJumpHMC(distribution=d, Vinit=V0, seed=1, resample=False, **kw)
    o = orc.MarkovJumpHMC(en, X0, V0=V0, resample=False, rng=orc.ReplayRNG(normals=normals, exps=exps), state_rounding=to_bf16, **kw)
    resync(s, o)
    ties = 0
    for t in range(T):
        # check_iteration drives both sides itself: hand the recorded numbers to the device through a one-shot patch
        step = s.sampling_iteration
        s.sampling_iteration = lambda step=step, t=t: step(replay=[(normals[min(o.rng.n_normals_used, T - 1)], exps[t])])
        try:
            ties += check_iteration(s, o, tag='%s, iteration %d' % (tag0, t), **tol)
        finally:
            del s.sampling_iteration
        check_stored_energies(s, en, '%s, iteration %d' % (tag0, t))
        resync(s, o)
    assert ties <= 1
    assert s.l_count + s.f_count + s.r_count == T * N and s.r_count > 0, (tag0, 'no R move: the recorded normals were never read')


# ---------------------------------------------------------------------------------------------
# HMCState.L() on a snapshot: sic_leap_kernel and the dE/dX it hands out
# ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('P,nc', LEAP)
def test_leapfrog_operator(P, nc):
    """As tests/test_gpu_dense_parity.py::test_sic_leapfrog_operator (X, V within 1 / 128 of the maximum, EX, EV within 5e-4 of
    max |H|), and the dE/dX of the end point against the restatement at the stored end point (2e-4)."""
    key = case('mj', P, nc=nc)
    _, _, N, L, _, state, cauchy = key
    eps = EPS[key]
    s = _device(key, eps)
    en = _energy(P, nc, cauchy)
    o = orc.MarkovJumpHMC(en, _x0(P, N, nc, state), epsilon=eps, beta=BETAS['mj'], num_leapfrog_steps=L, V0=s.state.V,
                          resample=False, rng=orc.ReplayRNG(), state_rounding=to_bf16)
    Z = s.state.copy().L()
    Zo = o.state.clone().L()
    assert np.abs(Z.X - Zo.X).max() <= np.abs(Zo.X).max() / 128 and np.abs(Z.V - Zo.V).max() <= np.abs(Zo.V).max() / 128
    scale = float(np.abs(Zo.H()).max())
    assert np.abs(Z.EX - Zo.EX).max() <= 5e-4 * scale and np.abs(Z.EV - Zo.EV).max() <= 5e-4 * scale
    ref, flips, candidates = explain_residual_flips(Z.dEdX, en, _energy(P, nc, cauchy, np.float32), Z.X)
    eG = rel(Z.dEdX, ref)
    print('leap: %d bf16 flips of the residual taken of %d elements at a rounding boundary; dEdX before them %.3g'
          % (flips, candidates, rel(Z.dEdX, en.dEdX_val(Z.X))))
    eEX, eEV = rel(Z.EX[0], en.E_val(Z.X)[0]), rel(Z.EV[0], 0.5 * np.sum(Z.V * Z.V, axis=0))
    print('leap %s eps=2^%d: dEdX %.3g, EX %.3g and EV %.3g of the stored end point' % (_layout(P, N, nc, state), int(np.log2(eps)), eG, eEX, eEV))
    assert eG < EVAL_BARS[1] and eEX < EVAL_BARS[0] and eEV < 1e-5, (P, nc, eG, eEX, eEV)
