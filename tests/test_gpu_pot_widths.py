"""GPU: the matrix-core ProductOfT tile kernels (pot_eval_kernel, pot_jump_kernel, pot_flf_kernel, pot_leap_kernel with
float32 state; pot64_jump_kernel, pot64_flf_kernel with float64 state) against the NumPy oracle on the same Philox
streams at the widths where their padding and the NB = 1 shortcut change: the edges of a group of eight k-rows, of a
published 32-row block and of the padded sizes 128 / 256 / 512 (NB = 1 / 2 / 4 accumulator blocks per wave).  The other
oracle tests of these kernels run ndims = 36, 200, 300 and 512 at epsilon = 0.1 and L = 5 or 6; 36 and 512 are repeated
here as the anchor to them.  The machinery is theirs: check_iteration / check_control_iteration / resync of
tests/helpers.py, the oracle resynchronised to the device state after every compared iteration.

What a width reaches (tests.helpers.pot_padded_dim restates the padded size; tests/test_pot_widths_cpu.py pins it):

  D      NB  padded rows  k-row groups kept (NB = 1)   the edge
  1      1   127           1 of 16                     one row: the whole product is one k-row
  2      1   126           1 of 16                     one Box-Muller pair
  7, 8   1   121, 120      1 of 16                     below / at the end of the first group of eight
  9      1   119           2 of 16                     row 8 alone in the second group
  33     1   95            5 of 16                     row 32 alone in the second published block
  36     1   92            5 of 16                     (the anchor to the existing tests)
  65     1   63            9 of 16                     row 64 alone in the third published block
  127    1   1             16 of 16                    odd, one padded row
  128    1   0             16 of 16                    fills NB = 1 exactly
  129    2   127           all                         the step into NB = 2
  255    2   1             all                         odd, one padded row
  256    2   0             all                         fills NB = 2 exactly
  257    4   255           all                         the step into NB = 4
  511    4   1             all                         odd, one padded row
  512    4   0             all                         fills NB = 4 exactly (the anchor; the benchmark's width)

Cases.  The model of the existing tests: W = ref_init_weights(D, D)[0] + I, bias 0.1 randn(D), beta = 0.3.
  single evaluation   every width, N = 70 (a ragged third tile of kP = 32 particles); N = 1 and N = 33 (a second tile holding
                      one particle) at D = 9, 129, 257; both state types
  MarkovJumpHMC       every width at L = 5, N = 70; L = 1 and 2 (pot_trajectory merges half kicks: L = 1 takes the closing
                      half kick at once) at D = 9, 33, 128, 129, 257, 511; N = 1 and 33 at D = 9, 129, 257; float32 state
                      (pot_*: the float64 oracle with the end points stored in float32) and float64 state (pot64_*: the
                      oracle's float32 force on float64 state, tick-0 momenta equal to 1e-13); 4 iterations with a resync
                      after each -- 12 at D = 1 and 2, where F moves are rare at every step size (until the oracle's run
                      holds at least 6), and 24 with one particle (so that every kind of move occurs)
  a fused call        sample(3, preserve_order=True) after the compared iterations at D = 33, 129, 511 (N = 70, L = 5)
  ControlHMC          D = 9, 33, 129, 257, 511, N = 70, L = 5, both state types: the batch-wide momentum refresh at odd
                      widths (column_normals masks 2 pair + 1 < D, pot_normals d + r < D; a normal in a padded row shows
                      in EV alone, which sums all 128 NB rows)
  ContinuousTimeHMC   D = 33, N = 60, L = 5, float32 state

Step sizes, fixed with the oracle alone (`choose_eps`): the smallest epsilon of {0.1, 0.3, 0.6, 1.0, 1.6, 2.5} at which
each of L, F and R is at least 2 % of the particle-iterations of the ORACLE's own run over the iterations the case
compares and nothing is non-finite.  At epsilon = 0.1 a narrow model makes no F move at all (the inverse-L items would
never run), and with L = 1 hardly any at every width.  TABLE below the imports lists, for every case, epsilon, the
oracle's tallies and shares, and the float32 spread; tests/test_pot_widths_cpu.py recomputes all of it without a GPU,
and shows on the reference alone that the float32 and the float64 force choose different transitions on at most
tie_ceiling(N) particles of any compared iteration (measured: none), so the inputs keep check_iteration inside its cap.

Tolerances.  The existing bars -- float32 state delta_rel = x_tol = e_rtol = 2e-5; float64 state delta_rel = e_rtol = 4e-6,
x_tol = 1e-6; single evaluations 4e-6 (energy) and 2e-5 (gradient) -- wherever they hold.  They were set at
epsilon = 0.1; a case's allowance is max(bar, 4 x its float32 spread), the spread being the largest difference, in
check_iteration's measures, between the oracle's proposals with force_dtype = float32 and with force_dtype = float64
from the states of the oracle's own run (`spread32_of_state`; no device output involved; 4 x: the room
tests/test_gpu_groups_oracle.py gives the same float32 products added in another order).  The spreads met: delta_rel
5.9e-8 .. 9.2e-7, x_tol 4e-8 .. 4.8e-7, e_rtol 4.6e-8 .. 6.3e-7 (TABLE, OTHER).  Five float64-state cases exceed a
bar, x_tol alone, by at most 1.7 x (WIDER).

One departure from that rule: the fused call.  It makes three iterations without a resync, so the rounding of the force
grows along it, and the one-iteration spread does not describe it.  Its spread is measured the same way on the oracle
alone, along the path the particles take: the oracle with the float32 and with the float64 force makes the three
iterations from the state its own compared iterations end in, and the last states are compared on the particles whose
transitions all agree (`fused_path_spread`, FUSED_PATH_SPREAD).  The call's (x_tol, e_rtol) is max(the case's allowance,
4 x that).  It is wider than the case's in ONE case (FUSED_WIDER): float64 state, D = 33, epsilon = 0.6, x_tol 5.2e-6
instead of 1.04e-6 -- the oracle's two forces are 1.3e-6 apart there, beyond the one-iteration bar of 1e-6 before any
device is involved, and the device ends 1.2e-6 from the oracle (V).  By the one-iteration rule alone that case would
fail at 1.2e-6 against 1.04e-6; the other five fused calls keep their case's allowance.

Every case prints the instance it reached (NB, state type), its step size, the oracle's tallies and shares, its spread
and its allowance; single evaluations print their two errors.  The device's tallies are asserted equal to the table's
whenever no near tie occurred.  Measured on an MI355X: the device makes the table's moves in every case (ControlHMC and
ContinuousTimeHMC included), no near tie in any of them; single evaluations within 7.7e-7 (energy) and 6.0e-7 (gradient); the fused calls
leave no particle off the oracle's path and end within 1.2e-6 (V at D = 33, float64 state) and 4.1e-7 (EX at D = 511).

Sensitivity.  With `< kdim` replaced by `< kdim - 1` in gemm_any<1, ...> (csrc/dense_pot_tile.hpp: the group of eight
k-rows whose first row is the model's last is dropped) the 56 ProductOfT tests of tests/test_gpu_parity.py and
tests/test_gpu_dense_parity.py (36, 200, 300, 512 dims) all pass, and all 37 cases of this module at 1, 9, 33 and 65 dims
fail (single evaluations, MarkovJumpHMC at every L and N, ControlHMC, ContinuousTimeHMC)."""
import functools

import numpy as np
import pytest

from oracle import mjhmc_oracle as orc
from tests.helpers import (_argmin_lfr, check_control_iteration, check_iteration, pot_padded_dim, ref_init_weights, resync,
                           tie_ceiling)

gpu = pytest.mark.gpu
np.seterr(all='ignore')

BETA = 0.3
SEED = 17
CONTROL_SEED = 20       # the first seed from 17 up whose batch-wide refresh gate opens within the first two iterations
CT_SEED = 43            # tests/test_gpu_dense_parity.py::test_pot_continuous_time_sampler_vs_oracle's
SEEDS = {'MarkovJumpHMC': SEED, 'ControlHMC': CONTROL_SEED, 'ContinuousTimeHMC': CT_SEED}   # of the device and of the oracle
EPS_GRID = (0.1, 0.3, 0.6, 1.0, 1.6, 2.5)
MIN_SHARE = 0.02        # of the particle-iterations, each of L, F and R in the oracle's own run
MIN_F_NARROW = 6        # ndims <= 2: F moves in the oracle's own run instead (F is rare there at every step size)
MARGIN = 4.0            # tests/test_gpu_groups_oracle.py's room for the same float32 products added in another order
LIVE_DH = 40.0          # a proposal beyond it is never taken (rate below exp(-20) of the others): not part of the spread
N_ITER = 4
N_FUSED = 3

WIDTHS = (1, 2, 7, 8, 9, 33, 36, 65, 127, 128, 129, 255, 256, 257, 511, 512)
SHORT = (9, 33, 128, 129, 257, 511)          # L = 1 and 2
SMALL_BATCH = (9, 129, 257)                  # N = 1 and 33
CONTROL = (9, 33, 129, 257, 511)
FUSED = (33, 129, 511)
STATES = ('float32', 'float64')
# (D, N, L) of the MarkovJumpHMC cases, each in both state types
MJ_CASES = ([(D, 70, 5) for D in WIDTHS] + [(D, 70, L) for D in SHORT for L in (1, 2)] +
            [(D, N, 5) for D in SMALL_BATCH for N in (1, 33)])
# the existing bars: (delta_rel, x_tol, e_rtol)
BARS = {'float32': (2e-5, 2e-5, 2e-5), 'float64': (4e-6, 1e-6, 4e-6)}


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def n_iterations(D, N):
    """compared iterations of a MarkovJumpHMC case: 4; more where 4 hold too few particle-iterations for the shares to mean
    anything -- ndims <= 2 (F is rare at every step size: until the oracle's run holds MIN_F_NARROW of them) and one
    particle (24 particle-iterations, so that each kind of move can occur at all)"""
    if N == 1:
        return 24
    return {1: 12, 2: 12}.get(D, N_ITER)


# The MarkovJumpHMC cases, each run with float32 and with float64 state (both references make the same moves at every one):
#   (D, N, L): (epsilon, the oracle's own (l, f, r) over the compared iterations, the float32 spread (of delta_rel, x_tol,
#   e_rtol) with float32 state, with float64 state)
# and what the case reaches: NB, the padded rows, the groups of eight k-rows the NB = 1 shortcut keeps, the compared
# iterations, the shares of L / F / R in per cent.
TABLE = {
    (1, 70, 5): (1.6, (698, 18, 124), (3.1e-07, 4.8e-07, 2.6e-07), (1.5e-07, 4.2e-07, 2.1e-07)),    # 1  127   1/16  12  83.1 /  2.1 / 14.8
    (2, 70, 5): (1.0, (701, 14, 125), (1.5e-07, 1.3e-07, 1.6e-07), (1.6e-07, 1.3e-07, 1.2e-07)),    # 1  126   1/16  12  83.5 /  1.7 / 14.9
    (7, 70, 5): (1.0, (227, 8, 45), (1.3e-07, 1.6e-07, 9.7e-08), (9.8e-08, 1.2e-07, 8.1e-08)),      # 1  121   1/16   4  81.1 /  2.9 / 16.1
    (8, 70, 5): (1.0, (226, 6, 48), (1.3e-07, 1.4e-07, 1.1e-07), (1.2e-07, 1.6e-07, 1.2e-07)),      # 1  120   1/16   4  80.7 /  2.1 / 17.1
    (9, 70, 5): (1.0, (224, 8, 48), (1.4e-07, 1.7e-07, 8.8e-08), (1.3e-07, 2.1e-07, 1e-07)),        # 1  119   2/16   4  80.0 /  2.9 / 17.1
    (33, 70, 5): (0.6, (208, 23, 49), (2.2e-07, 2e-07, 1.4e-07), (2e-07, 2.6e-07, 1.6e-07)),        # 1   95   5/16   4  74.3 /  8.2 / 17.5
    (36, 70, 5): (0.3, (225, 10, 45), (2e-07, 2.3e-07, 1.4e-07), (1.8e-07, 1.9e-07, 1.5e-07)),      # 1   92   5/16   4  80.4 /  3.6 / 16.1
    (65, 70, 5): (0.3, (219, 17, 44), (2.3e-07, 2.4e-07, 1.7e-07), (2.3e-07, 2.2e-07, 1.5e-07)),    # 1   63   9/16   4  78.2 /  6.1 / 15.7
    (127, 70, 5): (0.1, (228, 10, 42), (3.6e-07, 1e-07, 3e-07), (3.8e-07, 7.4e-08, 2.9e-07)),       # 1    1  16/16   4  81.4 /  3.6 / 15.0
    (128, 70, 5): (0.1, (229, 9, 42), (3.4e-07, 1.1e-07, 2.7e-07), (3.1e-07, 5.7e-08, 2.7e-07)),    # 1    0  16/16   4  81.8 /  3.2 / 15.0
    (129, 70, 5): (0.1, (231, 7, 42), (3.1e-07, 1.1e-07, 2.3e-07), (3e-07, 5.3e-08, 2.1e-07)),      # 2  127  all     4  82.5 /  2.5 / 15.0
    (255, 70, 5): (0.1, (219, 21, 40), (5.9e-07, 9.9e-08, 4.3e-07), (6e-07, 9.6e-08, 4.5e-07)),     # 2    1  all     4  78.2 /  7.5 / 14.3
    (256, 70, 5): (0.1, (219, 26, 35), (5.4e-07, 8.9e-08, 4.6e-07), (6.1e-07, 9.5e-08, 5.2e-07)),   # 2    0  all     4  78.2 /  9.3 / 12.5
    (257, 70, 5): (0.1, (217, 23, 40), (5.8e-07, 8.9e-08, 4.2e-07), (5.6e-07, 8.2e-08, 4.5e-07)),   # 4  255  all     4  77.5 /  8.2 / 14.3
    (511, 70, 5): (0.1, (194, 47, 39), (9.2e-07, 9.8e-08, 6.3e-07), (8.8e-07, 9.4e-08, 6.3e-07)),   # 4    1  all     4  69.3 / 16.8 / 13.9
    (512, 70, 5): (0.1, (195, 47, 38), (8.3e-07, 8.8e-08, 6e-07), (7.4e-07, 8.9e-08, 6.3e-07)),     # 4    0  all     4  69.6 / 16.8 / 13.6
    (9, 70, 1): (1.0, (226, 9, 45), (1.1e-07, 9.3e-08, 8.5e-08), (9.2e-08, 4e-08, 8e-08)),          # 1  119   2/16   4  80.7 /  3.2 / 16.1
    (9, 70, 2): (1.6, (212, 21, 47), (1.2e-07, 1.8e-07, 9.9e-08), (1.2e-07, 1.2e-07, 1.1e-07)),     # 1  119   2/16   4  75.7 /  7.5 / 16.8
    (33, 70, 1): (0.6, (216, 25, 39), (1.3e-07, 8.1e-08, 1.1e-07), (1.6e-07, 4.7e-08, 1.5e-07)),    # 1   95   5/16   4  77.1 /  8.9 / 13.9
    (33, 70, 2): (0.3, (227, 8, 45), (1.2e-07, 7.3e-08, 1.1e-07), (1.3e-07, 5.1e-08, 9.6e-08)),     # 1   95   5/16   4  81.1 /  2.9 / 16.1
    (128, 70, 1): (0.3, (217, 24, 39), (3.7e-07, 1.1e-07, 2.7e-07), (3.8e-07, 5.9e-08, 2.7e-07)),   # 1    0  16/16   4  77.5 /  8.6 / 13.9
    (128, 70, 2): (0.3, (194, 51, 35), (3.8e-07, 1.1e-07, 2.7e-07), (3.7e-07, 1e-07, 2.7e-07)),     # 1    0  16/16   4  69.3 / 18.2 / 12.5
    (129, 70, 1): (0.3, (213, 32, 35), (3.2e-07, 1.1e-07, 2.3e-07), (3.3e-07, 5.1e-08, 1.9e-07)),   # 2  127  all     4  76.1 / 11.4 / 12.5
    (129, 70, 2): (0.3, (186, 47, 47), (3.1e-07, 1.2e-07, 2.6e-07), (2.7e-07, 7.9e-08, 2.6e-07)),   # 2  127  all     4  66.4 / 16.8 / 16.8
    (257, 70, 1): (0.3, (184, 49, 47), (5.7e-07, 1e-07, 5e-07), (5.7e-07, 6.9e-08, 4.9e-07)),       # 4  255  all     4  65.7 / 17.5 / 16.8
    (257, 70, 2): (0.3, (154, 42, 84), (5.4e-07, 1.2e-07, 4.9e-07), (5.3e-07, 9.6e-08, 4.9e-07)),   # 4  255  all     4  55.0 / 15.0 / 30.0
    (511, 70, 1): (0.3, (162, 59, 59), (8.3e-07, 1.1e-07, 6e-07), (7.9e-07, 1.2e-07, 6e-07)),       # 4    1  all     4  57.9 / 21.1 / 21.1
    (511, 70, 2): (0.1, (228, 16, 36), (9.1e-07, 1.7e-07, 6e-07), (9.1e-07, 1.4e-07, 6e-07)),       # 4    1  all     4  81.4 /  5.7 / 12.9
    (9, 1, 5): (1.0, (20, 1, 3), (1.6e-07, 2.3e-07, 1.3e-07), (9.7e-08, 2.6e-07, 7.8e-08)),         # 1  119   2/16  24  83.3 /  4.2 / 12.5
    (9, 33, 5): (1.0, (103, 4, 25), (1.2e-07, 2e-07, 1.2e-07), (1.4e-07, 2e-07, 1.1e-07)),          # 1  119   2/16   4  78.0 /  3.0 / 18.9
    (129, 1, 5): (0.1, (20, 1, 3), (7.6e-08, 1.1e-07, 4.6e-08), (8.7e-08, 7.5e-08, 6.5e-08)),       # 2  127  all    24  83.3 /  4.2 / 12.5
    (129, 33, 5): (0.1, (102, 4, 26), (3e-07, 1.1e-07, 2.5e-07), (3.3e-07, 4.6e-08, 2.3e-07)),      # 2  127  all     4  77.3 /  3.0 / 19.7
    (257, 1, 5): (0.1, (19, 2, 3), (9.4e-08, 1.1e-07, 7.1e-08), (5.9e-08, 1e-07, 4.9e-08)),         # 4  255  all    24  79.2 /  8.3 / 12.5
    (257, 33, 5): (0.1, (97, 12, 23), (5.1e-07, 9.9e-08, 4.5e-07), (5e-07, 5.8e-08, 4.5e-07)),      # 4  255  all     4  73.5 /  9.1 / 17.4
}
# ControlHMC (N = 70, L = 5, 4 iterations, seed CONTROL_SEED) and ContinuousTimeHMC (N = 60, L = 5, 5 iterations, seed CT_SEED)
# at the step size of the MarkovJumpHMC case (D, 70, 5): the oracle's own (l, f, r, fl) and the float32 spread.  ControlHMC
# flips every particle, so l counts the accepted and f the rejected proposals; r = 70: one batch-wide refresh.
OTHER = {
    ('control', 'float32', 9): ((248, 32, 70, 0), (2e-07, 2.2e-07, 1.6e-07)),
    ('control', 'float32', 33): ((214, 66, 70, 0), (1.8e-07, 2.7e-07, 1.4e-07)),
    ('control', 'float32', 129): ((274, 6, 70, 0), (3.1e-07, 1.1e-07, 2e-07)),
    ('control', 'float32', 257): ((230, 50, 70, 0), (5.4e-07, 1.2e-07, 4.1e-07)),
    ('control', 'float32', 511): ((176, 104, 70, 0), (8e-07, 1.3e-07, 6.2e-07)),
    ('control', 'float64', 9): ((248, 32, 70, 0), (1.4e-07, 2.8e-07, 1.5e-07)),
    ('control', 'float64', 33): ((214, 66, 70, 0), (1.9e-07, 3.2e-07, 1.3e-07)),
    ('control', 'float64', 129): ((274, 6, 70, 0), (2.5e-07, 6.3e-08, 1.8e-07)),
    ('control', 'float64', 257): ((230, 50, 70, 0), (5.3e-07, 7.4e-08, 4.1e-07)),
    ('control', 'float64', 511): ((176, 104, 70, 0), (8e-07, 1.1e-07, 5.9e-07)),
    ('ct', 'float32', 33): ((0, 154, 19, 127), (2.1e-07, 2.5e-07, 1.5e-07)),
}
# The fused call of N_FUSED iterations makes them without a resync, so the rounding of the force grows along it.  Its float32
# spread (x_tol, e_rtol) is measured as the single iterations' is, on the oracle alone: the float32 and the float64 force
# make the N_FUSED iterations from the state the oracle's own compared iterations end in, and the last states are compared on
# the particles whose transitions all agree (`fused_path_spread`; all 70 in every case).
FUSED_PATH_SPREAD = {
    ('float32', 33, 70, 5): (8.3e-07, 2.5e-07),
    ('float32', 129, 70, 5): (1.2e-07, 1.9e-07),
    ('float32', 511, 70, 5): (2.8e-07, 5.1e-07),
    ('float64', 33, 70, 5): (1.3e-06, 1.5e-07),
    ('float64', 129, 70, 5): (7.1e-08, 1.7e-07),
    ('float64', 511, 70, 5): (2.1e-07, 5e-07),
}
# A DEPARTURE from the one-iteration rule, for the fused call alone: its (x_tol, e_rtol) is max(the case's allowance, MARGIN x
# the fused path spread).  One case is wider than its single iterations: at D = 33, epsilon = 0.6, float64 state, the two
# forces of the ORACLE are 1.3e-6 apart after three iterations, beyond the one-iteration x_tol (1e-6; 1.04e-6 in WIDER) before
# any device is involved; the device ends 1.2e-6 from the oracle there (V).  ((x_tol, e_rtol) allowed, the spread):
FUSED_WIDER = {
    ('float64', 33, 70, 5): ((5.2e-06, 4e-06), (1.3e-06, 1.5e-07)),
}
# The cases whose allowance is wider than the existing bar, ((delta_rel, x_tol, e_rtol) allowed, the spread it comes from):
# max(bar, MARGIN x spread) per measure.  Only x_tol of the float64 state (bar 1e-6) is ever exceeded, at the large step
# sizes of the narrow widths; every float32-state case and every other measure keeps its bar.
WIDER = {
    ('float64', 1, 70, 5): ((4e-06, 1.68e-06, 4e-06), (1.5e-07, 4.2e-07, 2.1e-07)),
    ('float64', 33, 70, 5): ((4e-06, 1.04e-06, 4e-06), (2e-07, 2.6e-07, 1.6e-07)),
    ('float64', 9, 1, 5): ((4e-06, 1.04e-06, 4e-06), (9.7e-08, 2.6e-07, 7.8e-08)),
    ('control', 'float64', 9): ((4e-06, 1.12e-06, 4e-06), (1.4e-07, 2.8e-07, 1.5e-07)),
    ('control', 'float64', 33): ((4e-06, 1.28e-06, 4e-06), (1.9e-07, 3.2e-07, 1.3e-07)),
}

EPS, SHARES, SPREAD = {}, {}, {}
for _case, (_eps, _counts, _sp32, _sp64) in TABLE.items():
    for _state, _sp in zip(STATES, (_sp32, _sp64)):
        EPS[(_state,) + _case], SHARES[(_state,) + _case], SPREAD[(_state,) + _case] = _eps, _counts, _sp
for _key, (_counts, _sp) in OTHER.items():
    EPS[_key], SHARES[_key], SPREAD[_key] = TABLE[(_key[2], 70, 5)][0], _counts, _sp


# ---------------------------------------------------------------------------------------------
# the model, the two references and the device samplers
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model(D):
    W, lognu = ref_init_weights(D, D)
    return W + np.eye(D), lognu, 0.1 * np.random.RandomState(1).randn(D)


def _x0(D, N):
    return np.random.RandomState(1000 * D + N).randn(D, N)


def _energy(D, force):
    W, lognu, b = _model(D)
    return orc.ProductOfT(W, lognu=lognu, b=b, force_dtype=force)


def _reference(state, D, N, L, eps, cls_name='MarkovJumpHMC'):
    """The oracle a case is compared with.  float32 state: the float64 force, the end points of every move stored in
    float32 (tests/test_gpu_dense_parity.py::test_pot_iterations_from_the_reference_states); float64 state: the reference's
    own arithmetic, the float32 force on float64 state and no rounding
    (::test_pot_with_the_references_arithmetic_float64_state_float32_force)."""
    X0 = _x0(D, N)
    kw = dict(epsilon=eps, beta=BETA, num_leapfrog_steps=L, rng=orc.PhiloxRNG(SEEDS[cls_name], np.arange(N)))
    if cls_name in ('MarkovJumpHMC', 'ContinuousTimeHMC'):
        kw['resample'] = False
    if state == 'float32':
        o = getattr(orc, cls_name)(_energy(D, np.float64), f32(X0), state_rounding=f32, **kw)
        o.state.V[:] = f32(o.state.V)           # what a float32 state holds of the tick-0 normals
        o.state.refresh_EV()
    else:
        o = getattr(orc, cls_name)(_energy(D, np.float32), X0, **kw)
    return o


def _device(state, D, N, L, eps, cls_name='MarkovJumpHMC'):
    from mjhmc_amd.samplers import markov_jump_hmc as M
    from mjhmc_amd.misc.distributions import ProductOfT
    W, lognu, b = _model(D)
    X0 = _x0(D, N)

    class Fixed(ProductOfT):
        def init_X(self):
            self.Xinit = X0

    class Recording(getattr(M, cls_name)):
        def _commit(self, st):
            self.trace.append((st.l, st.f, st.r))
            super(Recording, self)._commit(st)

    d = Fixed(ndims=D, nbasis=D, nbatch=N, lognu=lognu, W=W, b=b, state_dtype=state)
    kw = dict(resample=False) if cls_name in ('MarkovJumpHMC', 'ContinuousTimeHMC') else {}
    s = Recording(distribution=d, epsilon=eps, beta=BETA, num_leapfrog_steps=L, seed=SEEDS[cls_name], **kw)
    s.trace = []
    return s


def _instance(state, D):
    DIM, NB = pot_padded_dim(D)
    kept = '%d of 16 k-row groups' % (-(-D // 8)) if NB == 1 else 'all k-rows'
    return '%s NB=%d (%d padded rows, %s)' % ('pot' if state == 'float32' else 'pot64', NB, DIM - D, kept)


# ---------------------------------------------------------------------------------------------
# measured on the oracle alone (tests/test_pot_widths_cpu.py runs these without a GPU)
# ---------------------------------------------------------------------------------------------
class _other_force(object):
    """the oracle `o` with `en` as its energy for a while; both energies' evaluation counters are put back"""

    def __init__(self, o, en):
        self.o, self.en = o, en

    def __enter__(self):
        self.keep = self.o.energy
        self.counts = [(e, e.E_count, e.dEdX_count) for e in (self.keep, self.en)]
        self.o.energy = self.en

    def __exit__(self, *exc):
        self.o.energy = self.keep
        for e, a, b in self.counts:
            e.E_count, e.dEdX_count = a, b


def _proposals(o, en, n_leap=1):
    """From the oracle's current X and V with the force `en`: H0 and, for the forward and the momentum-reversed start, the
    state after `n_leap` L operators (H0 - H, X, V, EX, EV)"""
    with _other_force(o, en):
        Z0 = o.state.clone()
        Z0.refresh_EX()
        Z0.refresh_grad()
        H0 = Z0.H()[0].copy()
        out = []
        for sign in (1, -1):
            Z = Z0.clone()
            if sign < 0:
                Z.F()
            for _ in range(n_leap):
                Z.L()
            out.append((H0 - Z.H()[0], Z.X, Z.V, Z.EX[0], Z.EV[0]))
    return H0, out


def spread32_of_state(o, D, n_leap=1):
    """The float32 spread of the oracle's current state: the largest differences between its proposals (L z and L F z)
    with force_dtype = float32 and with force_dtype = float64, in check_iteration's measures -- of the energy differences
    H0 - H(proposal) and of EX and EV over max(1, max |H0|), of X and V over max(1, max |X|) and max(1, max |V|) -- over the
    proposals that can be taken at all (|H0 - H| <= LIVE_DH).  `n_leap`: after that many L operators in a row (a fused
    call of as many iterations that takes L every time: the longest a particle runs without a resync)."""
    H64, p64 = _proposals(o, _energy(D, np.float64), n_leap)
    H32, p32 = _proposals(o, _energy(D, np.float32), n_leap)
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


def _decision(o, en, exps):
    """the transitions the oracle's rule takes from its current state with the force `en` (cached inverse-L energies kept)"""
    with _other_force(o, en):
        Z0 = o.state.clone()
        Z0.refresh_EX()
        Z0.refresh_grad()
        H0 = Z0.H()[0].copy()
        HL = Z0.clone().L().H()[0]
        Hflf = Z0.clone().FLF().H()[0]
    return _argmin_lfr(H0 - HL, H0 - Hflf, o.p_r, exps)


def _other_decision(o, en, cls_name):
    """the same for the other families, whose only energy-dependent decision is about the FL proposal: ControlHMC's accept
    (u < exp(H0 - H(L z))), ContinuousTimeHMC's first clock of F (rate 1), FL (rate exp((H0 - H) / 2)) and R (rate p_r)"""
    _, ((dh, _, _, _, _), _) = _proposals(o, en)
    if cls_name == 'ControlHMC':
        return np.asarray(o.rng.stream.accept_uniforms(o.rng.tick), dtype=np.float64) < np.exp(np.minimum(dh, 0.0))
    exps = np.asarray(o.rng.stream.unit_exponentials(o.rng.tick), dtype=np.float64)
    return np.argmin(np.stack([exps[1], exps[0] / np.exp(dh) ** .5, exps[2] / o.p_r]), axis=0)


def _twin(o, en):
    """a second MarkovJumpHMC oracle with the force `en` at o's state, cached inverse-L proposals and tick"""
    t = orc.MarkovJumpHMC(en, o.state.X.copy(), resample=False, epsilon=o.epsilon, beta=BETA,
                          num_leapfrog_steps=o.num_leapfrog_steps, rng=orc.PhiloxRNG(SEED, np.arange(o.nbatch)),
                          state_rounding=o.state_rounding)
    assert t.p_r == o.p_r
    t.rng.tick = o.rng.tick
    t.state.V[:] = o.state.V
    t.state.refresh_EV()
    t.state.shadow = o.state.shadow.clone(True)
    t.state.shadow.owner = t
    t.state.shadow_ok = o.state.shadow_ok.copy()
    return t


def fused_path_spread(o, D):
    """The float32 spread of a fused call of N_FUSED iterations from the oracle's current state: two oracles, one with
    force_dtype = float32 and one with float64, make the N_FUSED iterations without a resync; on the particles whose
    transitions all agree, the differences of the last state in check_iteration's measures (x_tol, e_rtol) -- what the
    float32 rounding of the force grows to along the path the particles actually take.  Returns them and the number of
    particles compared."""
    t32, t64 = _twin(o, _energy(D, np.float32)), _twin(o, _energy(D, np.float64))
    same, scale = np.ones(o.nbatch, dtype=bool), 1.0
    for _ in range(N_FUSED):
        scale = max(scale, float(np.abs(t64.state.H()).max()))
        t32.sampling_iteration()
        t64.sampling_iteration()
        same &= t32.last_transition == t64.last_transition
    a, b = t32.state, t64.state
    d_x = max(float(np.abs(a.X - b.X)[:, same].max()) / max(1.0, float(np.abs(b.X).max())),
              float(np.abs(a.V - b.V)[:, same].max()) / max(1.0, float(np.abs(b.V).max())))
    d_e = max(float(np.abs(a.EX - b.EX)[0, same].max()), float(np.abs(a.EV - b.EV)[0, same].max())) / scale
    return np.array([d_x, d_e]), int(same.sum())


@functools.lru_cache(maxsize=None)
def oracle_run(state, D, N, L, eps, cls_name='MarkovJumpHMC', n_iter=None, fused=False):
    """The oracle's own run of a case from its initial state (seed SEEDS[cls_name], the device sampler's), no device
    involved: the tallies (l, f, r) and fl over the compared iterations, whether everything stayed finite, per iteration
    the number of particles on which the float32 and the float64 force decide differently, the float32 spread (the
    largest over the iterations) and, with `fused`, the spread of a fused call (`fused_path_spread`) from the state the
    compared iterations end in."""
    n_iter = n_iterations(D, N) if n_iter is None else n_iter
    mj = cls_name == 'MarkovJumpHMC'
    o = _reference(state, D, N, L, eps, cls_name)
    e32, e64 = _energy(D, np.float32), _energy(D, np.float64)
    spread, ties, finite = np.zeros(3), [], True
    for _ in range(n_iter):
        spread = np.maximum(spread, spread32_of_state(o, D))
        if mj:
            exps = np.asarray(o.rng.stream.unit_exponentials(o.rng.tick), dtype=np.float64)
            ties.append(int(np.sum(_decision(o, e32, exps) != _decision(o, e64, exps))))
        else:
            ties.append(int(np.sum(_other_decision(o, e32, cls_name) != _other_decision(o, e64, cls_name))))
        o.sampling_iteration()
        finite = finite and bool(np.isfinite(o.state.X).all() and np.isfinite(o.state.V).all() and
                                 np.isfinite(o.state.H()).all())
    out = dict(counts=(o.l_count, o.f_count, o.r_count), finite=finite, ties=ties, spread=spread, n_iter=n_iter,
               fl=o.fl_count, refreshed=o.r_count > 0)
    if fused:
        out['fused_spread'], out['fused_compared'] = fused_path_spread(o, D)
    return out


def shares_ok(D, N, counts, n_iter):
    """the step-size rule: each of L, F and R at least MIN_SHARE of the particle-iterations (ndims <= 2: at least
    MIN_F_NARROW F moves and the rule for L and R)"""
    l, f, r = counts
    need = MIN_SHARE * N * n_iter
    assert l + f + r == N * n_iter
    if D <= 2:
        return l >= need and r >= need and f >= MIN_F_NARROW
    return min(l, f, r) >= need


def choose_eps(state, D, N, L):
    """the smallest step size of EPS_GRID at which the oracle's own run meets the rule, and that run"""
    for eps in EPS_GRID:
        run = oracle_run(state, D, N, L, eps)
        if run['finite'] and shares_ok(D, N, run['counts'], run['n_iter']):
            return eps, run
    raise AssertionError(('no step size of the grid meets the rule', state, D, N, L))


def allowance(state, spread):
    """max(the existing bar, MARGIN x the float32 spread), per measure"""
    return tuple(max(bar, MARGIN * float(sp)) for bar, sp in zip(BARS[state], spread))


def fused_tolerances(key, state):
    """(x_tol, e_rtol) of the fused call: the case's own unless FUSED_WIDER names it"""
    tol = tolerances(key, state)
    return FUSED_WIDER[key][0] if key in FUSED_WIDER else (tol['x_tol'], tol['e_rtol'])


def tolerances(key, state):
    tol = WIDER[key][0] if key in WIDER else BARS[state]
    return dict(zip(('delta_rel', 'x_tol', 'e_rtol'), tol))


def _describe(state, D, N, L, key):
    """the case, the instance it reaches, the oracle's own tallies (MarkovJumpHMC: l / f / r, the shares of the table; the
    others: l / f / r / fl), its float32 spread and its allowance"""
    total = N * (5 if key[0] == 'ct' else n_iterations(D, N))
    return ('%s D=%d N=%d L=%d eps=%g %s; oracle tallies %s of %d (%s %%); float32 spread %s, allowed %s'
            % (key[0] if key[0] in ('control', 'ct') else 'mjhmc', D, N, L, EPS[key], _instance(state, D),
               ' / '.join('%d' % c for c in SHARES[key]), total, ' / '.join('%.1f' % (100.0 * c / total) for c in SHARES[key]),
               ' '.join('%.2g' % v for v in SPREAD[key]), ' '.join('%.2g' % v for v in tolerances(key, state).values())))


# ---------------------------------------------------------------------------------------------
# single evaluations: pot_eval_kernel, both state types
# ---------------------------------------------------------------------------------------------
EVAL = [(D, 70) for D in WIDTHS] + [(D, N) for D in SMALL_BATCH for N in (1, 33)]


@gpu
@pytest.mark.parametrize('state', STATES)
@pytest.mark.parametrize('D,N', EVAL)
def test_single_evaluation(D, N, state):
    """d.E / d.dEdX against the oracle's float32 force at the bars of tests/test_gpu_dense_parity.py (4e-6 of the largest
    energy, 2e-5 of the largest gradient element): the host-side padding and pre-scaling (w1, w2t, cb, al), the bias, the
    kept k-row groups, a ragged tile."""
    from mjhmc_amd.misc.distributions import ProductOfT
    W, lognu, b = _model(D)
    X = 1.5 * _x0(D, N)
    d = ProductOfT(ndims=D, nbasis=D, nbatch=N, lognu=lognu, W=W, b=b, state_dtype=state)
    en = _energy(D, np.float32)
    E, G = d.E(X), d.dEdX(X)
    assert E.shape == (1, N) and G.shape == (D, N)
    eE, eG = rel(E[0], en.E_val(X)[0]), rel(G, en.dEdX_val(X))
    print('eval D=%d N=%d %s: E %.3g dEdX %.3g' % (D, N, _instance(state, D), eE, eG))
    assert eE < 4e-6 and eG < 2e-5, (D, N, state, eE, eG)
    assert (d.E_count, d.dEdX_count) == (N, N)


# ---------------------------------------------------------------------------------------------
# MarkovJumpHMC
# ---------------------------------------------------------------------------------------------
def _fused_call(s, o, state, D, N, key, tag0):
    """sample(N_FUSED, preserve_order=True) from the resynced state against N_FUSED oracle iterations.  A particle's
    transitions all agree when every recorded X and dwelling time of the call is the oracle's (another transition leaves
    another position, or the same position after another clock: differences of order one, looked for at 1e-3) and its last
    transition is; on those the last state is held to check_iteration's measures at the allowance of the call
    (`fused_tolerances`: the case's own, but for FUSED_WIDER).  The others are near ties of one of the iterations: at most
    tie_ceiling(N) of them, and the tallies are the oracle's when there is none."""
    tol = fused_tolerances(key, state)
    t0 = len(s.trace)
    out = s.sample(N_FUSED, preserve_order=True)
    assert out.shape == (D, N, N_FUSED) and np.isfinite(out).all()
    dwell = s._dev.ring_read_dwell(0, N_FUSED)
    same = np.ones(N, dtype=bool)
    tallies, scale = [], 1.0
    for t in range(N_FUSED):
        before = (o.l_count, o.f_count, o.r_count)
        scale = max(scale, float(np.abs(o.state.H()).max()))
        o.sampling_iteration()
        tallies.append((o.l_count - before[0], o.f_count - before[1], o.r_count - before[2]))
        xs = max(1.0, float(np.abs(o.state.X).max()))
        same &= np.abs(out[:, :, t] - o.state.X).max(axis=0) <= 1e-3 * xs
        same &= np.isclose(dwell[t], o.dwelling_times, rtol=1e-2, atol=0)
    same &= s._dev.read(8) == o.last_transition
    assert all(sum(tr) == N for tr in s.trace[t0:]) and len(s.trace) == t0 + N_FUSED, (tag0, 'l + f + r', s.trace[t0:])
    assert int((~same).sum()) <= tie_ceiling(N), (tag0, 'fused call: particles off the oracle path', int((~same).sum()))
    if same.all():
        assert s.trace[t0:] == tallies, (tag0, 'fused call: tallies', s.trace[t0:], 'oracle', tallies)
    st, os_ = s.state, o.state
    eX = float(np.abs(st.X[:, same] - os_.X[:, same]).max()) / max(1.0, float(np.abs(os_.X).max()))
    eV = float(np.abs(st.V[:, same] - os_.V[:, same]).max()) / max(1.0, float(np.abs(os_.V).max()))
    eEX = float(np.abs(st.EX[0, same] - os_.EX[0, same]).max()) / scale
    eEV = float(np.abs(st.EV[0, same] - os_.EV[0, same]).max()) / scale
    print('%s: fused call of %d, %d particles off the oracle path, X %.3g V %.3g EX %.3g EV %.3g, allowed %s'
          % (tag0, N_FUSED, int((~same).sum()), eX, eV, eEX, eEV, tol))
    assert np.array_equal(out[:, :, -1], st.X), (tag0, 'fused call: the last recorded sample is the live state')
    assert max(eX, eV) <= tol[0] and max(eEX, eEV) <= tol[1], (tag0, 'fused call', eX, eV, eEX, eEV, 'allowed', tol)
    assert np.array_equal(st.cache_active[same], os_.shadow_ok[same]), (tag0, 'fused call: cache flags')


@gpu
@pytest.mark.parametrize('state', STATES)
@pytest.mark.parametrize('D,N,L', MJ_CASES)
def test_iterations_match_oracle(D, N, L, state):
    """sampling_iteration() through check_iteration with a resync after every iteration: transitions equal or provable near
    ties, X, V, EX, EV, the cache flags and the dwelling times within the case's allowance; l + f + r and, while no near tie
    has occurred, the evaluation counters are the oracle's.  D in FUSED (N = 70, L = 5): a fused call of three follows."""
    key = (state, D, N, L)
    eps, n_iter, tol = EPS[key], n_iterations(D, N), tolerances(key, state)
    tag0 = _describe(state, D, N, L, key)
    print(tag0)
    s = _device(state, D, N, L, eps)
    o = _reference(state, D, N, L, eps)
    d, en = s.distribution, o.energy
    if state == 'float64':
        assert np.allclose(s.state.V, o.state.V, rtol=0, atol=1e-13), (tag0, 'tick-0 momenta')
    else:
        assert np.array_equal(s.state.X, o.state.X) and np.allclose(s.state.V, o.state.V, rtol=0, atol=1e-6), (tag0, 'tick 0')
    resync(s, o)
    ties = 0
    for t in range(n_iter):
        before = (d.E_count, d.dEdX_count, en.E_count, en.dEdX_count)
        ties += check_iteration(s, o, tag='%s, iteration %d' % (tag0, t), **tol)
        assert s.l_count + s.f_count + s.r_count == (t + 1) * N, (tag0, t, 'l + f + r')
        if ties == 0:
            assert (d.E_count - before[0], d.dEdX_count - before[1]) == (en.E_count - before[2], en.dEdX_count - before[3]), \
                (tag0, t, 'evaluation counters')
        resync(s, o)
    if ties == 0:
        assert (s.l_count, s.f_count, s.r_count) == (o.l_count, o.f_count, o.r_count), (tag0, 'tallies')
        assert (s.l_count, s.f_count, s.r_count) == SHARES[key], (tag0, 'the device run does not make the moves of the table')
    assert min(s.l_count, s.f_count, s.r_count) >= 1, (tag0, 'a kind of move the step size was chosen for never occurred')
    print('%s: %d near ties in %d transitions; device L / F / R = %d / %d / %d' % (tag0, ties, n_iter * N, s.l_count, s.f_count, s.r_count))
    X = s.state.X
    assert (np.abs(X - f32(X)).max() == 0) == (state == 'float32'), (tag0, 'the state type')
    if D in FUSED and (N, L) == (70, 5):
        _fused_call(s, o, state, D, N, key, tag0)
        assert s.l_count + s.f_count + s.r_count == (n_iter + N_FUSED) * N, (tag0, 'l + f + r after the fused call')


# ---------------------------------------------------------------------------------------------
# the other sampler families
# ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('state', STATES)
@pytest.mark.parametrize('D', CONTROL)
def test_control_hmc_matches_oracle(D, state):
    """ControlHMC (Metropolis accept, flip, the batch-wide momentum refresh: the odd widths' padded rows must stay out of
    EV) through check_control_iteration, N = 70, L = 5, the step size of the MarkovJumpHMC case."""
    N, L = 70, 5
    key = ('control', state, D)
    eps, tol = EPS[key], tolerances(key, state)
    tag0 = _describe(state, D, N, L, key)
    print(tag0)
    s = _device(state, D, N, L, eps, 'ControlHMC')
    o = _reference(state, D, N, L, eps, 'ControlHMC')
    assert (s.beta, s.p_r, s.p_flip) == (o.beta, o.p_r, o.p_flip)
    d, en = s.distribution, o.energy
    resync(s, o)
    ties = 0
    for t in range(N_ITER):
        before = (d.E_count, d.dEdX_count, en.E_count, en.dEdX_count)
        ties += check_control_iteration(s, o, tag='%s, iteration %d' % (tag0, t), **tol)
        if ties == 0:
            assert (s.l_count, s.f_count, s.r_count, s.fl_count) == (o.l_count, o.f_count, o.r_count, o.fl_count), (tag0, t)
        assert (d.E_count - before[0], d.dEdX_count - before[1]) == (en.E_count - before[2], en.dEdX_count - before[3]) == (N, L * N)
        assert s.l_count + s.f_count == (t + 1) * N and s.fl_count == 0, (tag0, t, 'every particle flips: l (accepted) + f (rejected)')
        resync(s, o)
    assert ties <= 1, (tag0, 'near ties', ties)
    if ties == 0:
        assert (s.l_count, s.f_count, s.r_count, s.fl_count) == SHARES[key], (tag0, 'the device run does not make the moves of the table')
    print('%s: %d near ties; l / f / r / fl = %d / %d / %d / %d' % (tag0, ties, s.l_count, s.f_count, s.r_count, s.fl_count))
    assert s.r_count > 0, (tag0, 'no momentum refresh in the compared iterations')
    assert 0 < o.l_count + o.fl_count < N_ITER * N, (tag0, 'a trivial case: accepted moves', o.l_count + o.fl_count)


@gpu
def test_continuous_time_hmc_matches_oracle():
    """ContinuousTimeHMC at 33 dims, float32 state, in the form of
    tests/test_gpu_dense_parity.py::test_pot_continuous_time_sampler_vs_oracle."""
    state, D, N, L = 'float32', 33, 60, 5
    key = ('ct', state, D)
    eps, tol = EPS[key], tolerances(key, state)
    print(_describe(state, D, N, L, key))
    s = _device(state, D, N, L, eps, 'ContinuousTimeHMC')
    o = _reference(state, D, N, L, eps, 'ContinuousTimeHMC')
    resync(s, o)
    for t in range(5):
        s.sampling_iteration()
        o.sampling_iteration()
        # the F clock has rate 1 and R rate p_r: only the FL clock sees energies; with 60 particles a near tie is not expected
        assert (s.fl_count, s.f_count, s.r_count) == (o.fl_count, o.f_count, o.r_count), t
        assert s.fl_count + s.f_count + s.r_count == (t + 1) * N
        assert np.abs(s.state.X - o.state.X).max() <= tol['x_tol'] * max(1.0, np.abs(o.state.X).max())
        assert np.allclose(s.dwelling_times, o.dwelling_times, rtol=1e-3)
        resync(s, o)
    assert min(o.fl_count, o.f_count, o.r_count) > 0
    assert (s.l_count, s.f_count, s.r_count, s.fl_count) == SHARES[key], ('the device run does not make the moves of the table',
                                                                         (s.l_count, s.f_count, s.r_count, s.fl_count))
