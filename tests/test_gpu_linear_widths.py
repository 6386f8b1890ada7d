"""GPU: the linear-model tile kernels -- the 14 kernels hipRTC compiles around a caller's f / f' for the one NB the model
needs (lin_jump_kernel<NB, REPLAY, MODE> and lin64_jump_kernel<NB, REPLAY, MODE>, three modes, with and without replay;
lin_eval_kernel<NB>; lin_leap_kernel<NB>) -- against the NumPy oracle on the same Philox streams at every padded size, with
masked experts (K < P), padded state rows (D < P) and odd D.  The counterpart of tests/test_gpu_pot_widths.py, whose
machinery this module imports; the other oracle tests of these kernels (tests/test_gpu_linear.py) reach NB = 1 and one
NB = 4 case with K = D = P, float64 state, L = 6.  Since the built-in ProductOfT left it (kTail in pot64_trajectory and in
pot_gradient_published), the `else` branch of pot64_trajectory at NB = 4 -- momentum parked in sh.park, the full
kick_drift_pass<NB, 2> -- and gemm_dim_half's half-chunk AReg<4, 8> sets are run by lin64_jump_kernel<4, ...> alone.

The model, one expression pair throughout (one compile per NB and process): f = q[0] softplus(u), f' = q[0] / (1 + exp(-u)),
W = randn(K, D) / sqrt(D), b = 0.1 randn(K), q = 0.5 + rand(1, K) from RandomState(7 D + K), float32 values; X0 from
RandomState(1000 D + N); beta = 0.3; seeds 17 / CONTROL_SEED / CT_SEED.  The references are
tests/test_gpu_linear.py::restated's extended by q[0]: the float32 NumPy force on float64 state, and the same force with the
end points stored in float32 (state_rounding) for float32 state.

  D, K      NB  masked experts  padded rows   the edge
  100, 9    1   119             28            K << D; PotModel::ndims = max(D, K) keeps 13 of 16 k-row groups
  200, 130  2   126             56            K < D
  129, 256  2   0               127           K fills P, D one over 128, odd
  40, 257   4   255             472           NB set by K alone
  300, 200  4   312             212           K below the NB = 2 size while P = 512
  512, 400  4   112             0             full D: the benchmark's width on the branch named above
  511, 512  4   0               1             odd D (the last Box-Muller pair of a refresh is cut by d + r < D), every expert live

Cases (both state types unless noted; N = 70: three tiles of 32 particles, the third ragged).
  single evaluation   every shape at N = 70; N = 1 and 33 at the three NB = 4 shapes with K < P; rel(E) < 8e-6, rel(G) < 3.2e-5
  MarkovJumpHMC       every shape at L = 5, N = 70; L = 1 and 2 and N = 33 at (200, 130) and (512, 400); 4 iterations through
                      check_iteration with a resync after each; counters and tallies equal to the oracle's and the table's
                      whenever no near tie occurred
  a call of several   at (200, 130) and (512, 400): sample(3, preserve_order=True) against three sampling_iteration calls on
                      a twin sampler, bit for bit (X per iteration, V, EX, the counters)
  ControlHMC          (200, 130), (40, 257), (512, 400), (511, 512) through check_control_iteration
  ContinuousTimeHMC   (200, 130), (512, 400): MODE = CT, 5 iterations
  replay              (512, 400): REPLAY = true, MarkovJumpHMC in both state types (check_iteration) and ControlHMC in float64,
                      recorded normals, exponentials and uniforms to both sides
  lin_leap_kernel     DeviceEnergy.leapfrog(dtype='float32'), n = 1 and 3, at (200, 130) and (512, 400): 2e-5, dE/dX 5e-5
  the multi-pass twin lin64_jump_kernel against the test build's MJHMC_POT64_MULTIPASS=1 form of the same arithmetic
                      (lin_eval_kernel plus row passes: whole-chunk gemm_dim, nothing parked, no register-resident position)
                      at (200, 130), (300, 200), (512, 400), (511, 512) x nine (N, L, mode) cases in which every pair of values
                      occurs, eps = 0.1, p_r = 0.4, 1 + 3 iterations: X, V, dE/dX, E(X), the transitions and the counters bit
                      for bit, EV and HFLF at 1e-12, DWELL at 1e-7 (tests/test_gpu_pot64_tail_blocks.py::_compare).  Each
                      case twice: with the softplus pair, and with f = |u|, f' = u / |u|, whose padded experts give 0/0 unless
                      masked -- there every field must also be finite.  The two forms were bit-equal in all 72 cases.

Step sizes, fixed with the oracle alone (`choose_eps`, the rule of tests/test_gpu_pot_widths.py): the smallest epsilon of
{0.1, 0.3, 0.6, 1.0, 1.6, 2.5} at which each of L, F and R is at least 2 % of the particle-iterations of the ORACLE's own run
and nothing is non-finite.  TABLE and OTHER below the imports list, for every case, epsilon, the oracle's tallies and the
float32 spread; tests/test_linear_widths_cpu.py recomputes all of it without a GPU and shows that the float32 and the float64
force decide differently on at most tie_ceiling(N) particles of any compared iteration (measured: none).

Tolerances: per case and measure max(the existing bar, 4 x the float32 spread) -- the bars float32 state
delta_rel = x_tol = e_rtol = 2e-5, float64 state delta_rel = e_rtol = 4e-6, x_tol = 1e-6; the spread the largest difference,
in check_iteration's measures, between the oracle's proposals with the float32 and with the float64 NumPy force from the
states of the oracle's own run (`spread32_of_state`; no device output involved).  Spreads met: delta_rel 2.4e-8 .. 9.3e-8,
x_tol 5.6e-8 .. 3.6e-7, e_rtol 2.2e-8 .. 6.9e-8.  Four float64-state cases exceed a bar, x_tol alone, by at most 1.44 x (WIDER).

Every case prints the instance it reached (kernel family, NB, masked experts, padded rows), its step size, the oracle's tallies,
its spread and its allowance; the bit-for-bit cases print their tag.  Measured on an MI355X (2026-10-21, the kernels of
commit 9e459d3): the device makes the table's moves in all 41 sampler cases, no near tie in any of them; single evaluations
within 2.2e-7 (energy, (300, 200)) and 9.9e-7 (gradient, (511, 512)); over the MarkovJumpHMC cases X and V within 4.1e-7
(float32 state) and 3.3e-7 (float64 state), both at (40, 257), EX and EV within 1.6e-7; the leapfrog operator within 1.9e-7
(dE/dX 7.8e-7); the 72 twin cases and the four calls of several iterations equal bit for bit.

Sensitivity, measured on the MI355X with one line of a header changed at a time (the linear models' kernels are compiled from
the headers when the model is created; the built-in kernels were not rebuilt).  tests/test_gpu_linear.py has 44 tests, this
module 143.
  1. `j < lin.K ? g : 0.f` replaced by `g` in LinearExperts::phi (dense_pot_kernels.hpp): of tests/test_gpu_linear.py,
     test_padding_is_exact fails (both shapes: its L1 model) and the other 42 pass; here the 27 L1 cases of the multi-pass
     twin at (200, 130), (300, 200) and (512, 400) fail (not finite) and everything else passes -- (511, 512) has no padded
     expert, and a padded expert of the scaled softplus has q = 0 in the uploaded rows and a zero matrix row: 0 with or
     without the select.
  2. `cbase_of(c1)` replaced by `cbase_of(chunk)` in gemm_dim_half's second half_mfma_ld (dense_pot_tile.hpp): of
     tests/test_gpu_linear.py only the two 512 x 512 cases fail; here 67 fail -- all 54 twin cases at the three NB = 4 shapes,
     the 7 MarkovJumpHMC cases with float64 state at NB = 4, ControlHMC in float64 at (40, 257), (512, 400), (511, 512),
     ContinuousTimeHMC in float64 at (512, 400), both float64 replay cases.
  3. two[0] and two[1] exchanged where the `else` branch of pot64_trajectory reads the parked momentum back
     (dense_pot64_kernels.hpp): of tests/test_gpu_linear.py only the two 512 x 512 cases fail; here 65 fail -- the same as
     under 2 but for (40, 257), whose parked rows are padding (zero momentum either way).
  4. kick_drift_pass<NB, 2> replaced by <NB, 1> in that branch: the line serves every NB of a linear model (only the
     parking around it is NB = 4's), so of tests/test_gpu_linear.py 13 fail -- every float64-state comparison of iterations with
     the oracle or of a fused call with single iterations, the 36 x 36 and the 24-dim ones included -- and here 67 fail: the 48 twin cases with L = 2 and 5 at all four shapes, the 11
     float64 MarkovJumpHMC cases with L > 1, all float64 ControlHMC, ContinuousTimeHMC and replay cases.  L = 1 has no
     middle step and passes."""
import functools

import numpy as np
import pytest

from oracle import mjhmc_oracle as orc
from tests.helpers import (assert_multipass_pair_equal, check_control_iteration, check_iteration, hooks_context,
                           iterate_multipass_pair, pot_padded_dim, resync)
from tests.test_gpu_pot_widths import (BARS, BETA, EPS_GRID, LIVE_DH, N_ITER, SEEDS, STATES, _decision,
                                       _other_decision, _proposals, f32, rel, shares_ok)

gpu = pytest.mark.gpu
np.seterr(all='ignore')

ENERGY = 'q[0]*(u > 20.f ? u : log1pf(expf(u)))'
GRAD = 'q[0]/(1.f + expf(-u))'
L1 = ('fabsf(u)', 'u/fabsf(u)')           # f'(0) = 0/0: an unmasked padded expert poisons every dE/dX
EVAL_BARS = (8e-6, 3.2e-5)                # tests/test_gpu_linear.py::test_single_evaluation's: energy, gradient
LEAP_BARS = (2e-5, 5e-5)                  # tests/test_gpu_linear.py::test_state_operations': X, V, EX, EV; dE/dX
N_CT = 5                                  # compared iterations of a ContinuousTimeHMC case
N_REPLAY = 4                              # of a replay case
N_FUSED = 3

SHAPES = ((100, 9), (200, 130), (129, 256), (40, 257), (300, 200), (512, 400), (511, 512))
TWO = ((200, 130), (512, 400))            # L = 1 and 2, N = 33, the call of several iterations, ContinuousTimeHMC, the leapfrog
CONTROL = ((200, 130), (40, 257), (512, 400), (511, 512))
REPLAY = (512, 400)
SMALL_BATCH = ((40, 257), (300, 200), (512, 400))       # NB = 4 with K < P: single evaluations at N = 1 and 33
TWINS = ((200, 130), (300, 200), (512, 400), (511, 512))
# (D, K, N, L) of the MarkovJumpHMC cases, each in both state types
MJ_CASES = ([(D, K, 70, 5) for D, K in SHAPES] + [(D, K, 70, L) for D, K in TWO[::-1] for L in (1, 2)] +
            [(D, K, 33, 5) for D, K in TWO[::-1]])

# The MarkovJumpHMC cases, each run with float32 and with float64 state (both references make the same moves at every one):
#   (D, K, N, L): (epsilon, the oracle's own (l, f, r) over the 4 compared iterations, the float32 spread (of delta_rel,
#   x_tol, e_rtol) with float32 state, with float64 state)
# and what the case reaches: NB, the masked experts, the padded state rows, the shares of L / F / R in per cent.
TABLE = {
    (100, 9, 70, 5): (1.6, (228, 7, 45), (4.9e-08, 6.8e-08, 2.5e-08), (2.4e-08, 5.6e-08, 2.2e-08)),           # 1  119   28  81.4 /  2.5 / 16.1
    (200, 130, 70, 5): (0.6, (226, 11, 43), (6.2e-08, 1.9e-07, 3.7e-08), (6e-08, 2e-07, 4.6e-08)),            # 2  126   56  80.7 /  3.9 / 15.4
    (129, 256, 70, 5): (0.3, (228, 7, 45), (7e-08, 2.6e-07, 5.8e-08), (6.7e-08, 2.2e-07, 3.9e-08)),           # 2    0  127  81.4 /  2.5 / 16.1
    (40, 257, 70, 5): (0.3, (227, 10, 43), (5e-08, 3.3e-07, 3.7e-08), (4.4e-08, 2.9e-07, 2.9e-08)),           # 4  255  472  81.1 /  3.6 / 15.4
    (300, 200, 70, 5): (0.6, (224, 10, 46), (8e-08, 2.3e-07, 4.5e-08), (6.2e-08, 2.3e-07, 4.2e-08)),          # 4  312  212  80.0 /  3.6 / 16.4
    (512, 400, 70, 5): (0.3, (227, 9, 44), (5.2e-08, 2.5e-07, 3.8e-08), (4.5e-08, 2.6e-07, 4.2e-08)),         # 4  112    0  81.1 /  3.2 / 15.7
    (511, 512, 70, 5): (0.3, (226, 11, 43), (8.6e-08, 1.7e-07, 4.6e-08), (8.5e-08, 1.5e-07, 5.2e-08)),        # 4    0    1  80.7 /  3.9 / 15.4
    (512, 400, 70, 1): (0.6, (228, 11, 41), (3.9e-08, 1.9e-07, 2.6e-08), (3.6e-08, 1.7e-07, 2.4e-08)),        # 4  112    0  81.4 /  3.9 / 14.6
    (512, 400, 70, 2): (0.6, (213, 27, 40), (4.6e-08, 3.2e-07, 2.8e-08), (4e-08, 2.9e-07, 3.5e-08)),          # 4  112    0  76.1 /  9.6 / 14.3
    (200, 130, 70, 1): (0.6, (227, 7, 46), (5.8e-08, 1.1e-07, 4.3e-08), (5e-08, 9e-08, 3.8e-08)),             # 2  126   56  81.1 /  2.5 / 16.4
    (200, 130, 70, 2): (1.0, (207, 25, 48), (7.6e-08, 1.9e-07, 4.6e-08), (7.8e-08, 2e-07, 4.8e-08)),          # 2  126   56  73.9 /  8.9 / 17.1
    (512, 400, 33, 5): (0.3, (102, 5, 25), (4.7e-08, 2.4e-07, 4.2e-08), (3.9e-08, 2.1e-07, 2.7e-08)),         # 4  112    0  77.3 /  3.8 / 18.9
    (200, 130, 33, 5): (0.6, (98, 9, 25), (6.2e-08, 1.5e-07, 3.9e-08), (6.3e-08, 1.6e-07, 4e-08)),            # 2  126   56  74.2 /  6.8 / 18.9
}
# ControlHMC (N = 70, L = 5, 4 iterations, seed CONTROL_SEED), ContinuousTimeHMC (N = 70, L = 5, 5 iterations, seed CT_SEED) and
# the replay cases (N = 70, L = 5, 4 iterations on recorded numbers: MarkovJumpHMC 'replay', ControlHMC 'replay-control') at the
# step size of the MarkovJumpHMC case (D, K, 70, 5): the oracle's own (l, f, r, fl) -- 'replay': (l, f, r) -- and the float32
# spread.  ControlHMC flips every particle, so l counts the accepted and f the rejected proposals; r = 70: one batch-wide refresh.
OTHER = {
    ('control', 'float32', 200, 130): ((256, 24, 70, 0), (9.3e-08, 2.1e-07, 6.2e-08)),
    ('control', 'float32', 40, 257): ((259, 21, 70, 0), (4.3e-08, 3.4e-07, 3.8e-08)),
    ('control', 'float32', 512, 400): ((261, 19, 70, 0), (7e-08, 2.4e-07, 4.9e-08)),
    ('control', 'float32', 511, 512): ((269, 11, 70, 0), (5.3e-08, 2.2e-07, 3.9e-08)),
    ('control', 'float64', 200, 130): ((256, 24, 70, 0), (8.8e-08, 1.9e-07, 6.9e-08)),
    ('control', 'float64', 40, 257): ((259, 21, 70, 0), (4.5e-08, 3.6e-07, 4e-08)),
    ('control', 'float64', 512, 400): ((261, 19, 70, 0), (6.6e-08, 2.5e-07, 4.5e-08)),
    ('control', 'float64', 511, 512): ((269, 11, 70, 0), (4.9e-08, 1.7e-07, 4e-08)),
    ('ct', 'float32', 200, 130): ((0, 166, 21, 163), (5e-08, 1.8e-07, 4.1e-08)),
    ('ct', 'float32', 512, 400): ((0, 166, 21, 163), (4.7e-08, 2.2e-07, 2.8e-08)),
    ('ct', 'float64', 200, 130): ((0, 166, 21, 163), (4.6e-08, 1.9e-07, 3.6e-08)),
    ('ct', 'float64', 512, 400): ((0, 166, 21, 163), (5.7e-08, 2.1e-07, 3e-08)),
    ('replay', 'float32', 512, 400): ((240, 4, 36), (3.7e-08, 2.1e-07, 3.8e-08)),
    ('replay', 'float64', 512, 400): ((240, 4, 36), (3.8e-08, 2.1e-07, 2.8e-08)),
    ('replay-control', 'float64', 512, 400): ((273, 7, 70, 0), (6.1e-08, 2.1e-07, 3.7e-08)),
}
# The cases whose allowance is wider than the existing bar, ((delta_rel, x_tol, e_rtol) allowed, the spread it comes from):
# max(bar, MARGIN x spread) per measure.  Only x_tol of the float64 state (bar 1e-6) is ever exceeded, by at most 1.44 x;
# every float32-state case and every other measure keeps its bar.
WIDER = {
    ('float64', 40, 257, 70, 5): ((4e-06, 1.16e-06, 4e-06), (4.4e-08, 2.9e-07, 2.9e-08)),
    ('float64', 512, 400, 70, 5): ((4e-06, 1.04e-06, 4e-06), (4.5e-08, 2.6e-07, 4.2e-08)),
    ('float64', 512, 400, 70, 2): ((4e-06, 1.16e-06, 4e-06), (4e-08, 2.9e-07, 3.5e-08)),
    ('control', 'float64', 40, 257): ((4e-06, 1.44e-06, 4e-06), (4.5e-08, 3.6e-07, 4e-08)),
}

EPS, SHARES, SPREAD = {}, {}, {}
for _case, (_eps, _counts, _sp32, _sp64) in TABLE.items():
    for _state, _sp in zip(STATES, (_sp32, _sp64)):
        EPS[(_state,) + _case], SHARES[(_state,) + _case], SPREAD[(_state,) + _case] = _eps, _counts, _sp
for _key, (_counts, _sp) in OTHER.items():
    EPS[_key], SHARES[_key], SPREAD[_key] = TABLE[(_key[2], _key[3], 70, 5)][0], _counts, _sp


# ---------------------------------------------------------------------------------------------
# the model, the references and the device samplers
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model(D, K):
    """W (K, D), b (K,), q (1, K): float32 values in float64 arrays"""
    rs = np.random.RandomState(7 * D + K)
    W = rs.randn(K, D) / np.sqrt(D)
    b = 0.1 * rs.randn(K)
    q = 0.5 + rs.rand(1, K)
    return f32(W), f32(b), f32(q)


def _x0(D, N):
    return np.random.RandomState(1000 * D + N).randn(D, N)


def padded(D, K):
    """(P, NB) of a model: both D and K are padded to P = 128 NB"""
    return pot_padded_dim(max(D, K))


Q_MIN = 0.5         # q = 0.5 + rand: the smallest q an expert can carry


def restated(W, b, q, dtype=np.float32, wrong_q=False, padded_experts=0):
    """tests/test_gpu_linear.py::restated's force, extended by q[0]: E (1, n) and dE/dX (D, n) of the scaled softplus in
    `dtype` arithmetic, float64 out.  Two wrong kernels the evaluation bar must tell from the right one (the energy alone;
    tests/test_linear_widths_cpu.py): `padded_experts` adds that many experts at u = 0 carrying the smallest q a live
    expert can (Q_MIN log 2 each); `wrong_q` reads expert j's q at its index within its wave's 32 NB experts instead of
    the global j."""
    t = np.dtype(dtype).type
    Wt, bt, qt = W.astype(dtype), b.astype(dtype), q[0].astype(dtype)
    K, D = Wt.shape
    if wrong_q:
        qt = qt[np.arange(K) % (32 * padded(D, K)[1])]

    def u_of(X):
        return Wt.dot(X.astype(dtype)) + bt[:, None]

    def sp(u):
        return np.where(u > 20, u, np.log1p(np.exp(np.minimum(u, t(20)))))

    def E(X):
        e = (qt[:, None] * sp(u_of(X))).astype(np.float64).sum(axis=0)
        if padded_experts:
            e = e + padded_experts * Q_MIN * float(np.log(2.0))
        return e.reshape((1, -1))

    def dEdX(X):
        return Wt.T.dot((qt[:, None] / (t(1) + np.exp(-u_of(X)))).astype(dtype)).astype(np.float64)
    return E, dEdX


def _energy(D, K, force):
    return orc.LambdaEnergy(*restated(*_model(D, K), dtype=force))


def _rounding(state):
    return dict(state_rounding=f32) if state == 'float32' else {}


def _reference(state, D, K, N, L, eps, cls_name='MarkovJumpHMC'):
    """The oracle a case is compared with: the float32 NumPy force on float64 state, and for float32 state the same force
    with the end points of every move stored in float32 (tests/test_gpu_linear.py)."""
    X0 = _x0(D, N)
    kw = dict(epsilon=eps, beta=BETA, num_leapfrog_steps=L, rng=orc.PhiloxRNG(SEEDS[cls_name], np.arange(N)))
    if cls_name in ('MarkovJumpHMC', 'ContinuousTimeHMC'):
        kw['resample'] = False
    o = getattr(orc, cls_name)(_energy(D, K, np.float32), f32(X0) if state == 'float32' else X0, **dict(kw, **_rounding(state)))
    if state == 'float32':
        o.state.V[:] = f32(o.state.V)           # what a float32 state holds of the tick-0 normals
        o.state.refresh_EV()
    return o


def _dist(D, K, X0, state, exprs=(ENERGY, GRAD)):
    from mjhmc_amd.misc.distributions import LambdaDistribution
    W, b, q = _model(D, K)
    return LambdaDistribution(init=X0, device_linear=dict(W=W, b=b, energy=exprs[0], grad=exprs[1], expert_params=q),
                              state_dtype=state)


def _device(state, D, K, N, L, eps, cls_name='MarkovJumpHMC', **kw):
    from mjhmc_amd.samplers import markov_jump_hmc as M
    if cls_name in ('MarkovJumpHMC', 'ContinuousTimeHMC'):
        kw['resample'] = False
    kw.setdefault('seed', SEEDS[cls_name])
    return getattr(M, cls_name)(distribution=_dist(D, K, _x0(D, N), state), epsilon=eps, beta=BETA, num_leapfrog_steps=L, **kw)


def _instance(state, D, K, family=None):
    P, NB = padded(D, K)
    return '%s NB=%d (%d masked experts, %d padded rows)' % (family or ('lin' if state == 'float32' else 'lin64'), NB, P - K, P - D)


# ---------------------------------------------------------------------------------------------
# measured on the oracle alone (tests/test_linear_widths_cpu.py runs these without a GPU)
# ---------------------------------------------------------------------------------------------
def spread32_of_state(o, D, K, n_leap=1):
    """tests/test_gpu_pot_widths.py::spread32_of_state for the linear model: the largest differences between the oracle's
    proposals (L z and L F z) from its current state with the float32 and with the float64 NumPy force, in
    check_iteration's measures (delta_rel, x_tol, e_rtol), over the proposals that can be taken at all."""
    H64, p64 = _proposals(o, _energy(D, K, np.float64), n_leap)
    H32, p32 = _proposals(o, _energy(D, K, np.float32), n_leap)
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


def replay_numbers(D, N):
    """the recorded numbers of a replay case, as tests/test_gpu_dense_parity.py::test_dense_kernels_in_replay_mode draws
    them: X0, V0, per iteration the normals, the unit exponentials and ControlHMC's uniforms (accept, flip, refresh)"""
    rs = np.random.RandomState(123)
    X0, V0 = rs.randn(D, N), rs.randn(D, N)
    normals = [rs.randn(D, N) for _ in range(N_REPLAY)]
    unif = [(rs.rand(N), rs.rand(N), rs.rand()) for _ in range(N_REPLAY)]
    exps = [rs.standard_exponential((3, N)) for _ in range(N_REPLAY)]
    return X0, V0, normals, unif, exps


def _replay_reference(state, D, K, N, L, eps, cls_name):
    """the oracle of a replay case on orc.ReplayRNG, and what it was given: (o, X0, V0, normals, unif, exps, fired)"""
    X0, V0, normals, unif, exps = replay_numbers(D, N)
    if state == 'float32':
        X0, V0, normals = f32(X0), f32(V0), [f32(z) for z in normals]
    kw = dict(epsilon=eps, beta=BETA, num_leapfrog_steps=L, V0=V0, **_rounding(state))
    en = _energy(D, K, np.float32)
    if cls_name == 'ControlHMC':
        p_r = orc.ControlHMC(en, X0[:, :1], rng=orc.ReplayRNG(normals=[V0[:, :1]]), epsilon=eps, beta=BETA, num_leapfrog_steps=L).p_r
        fired = [u[2] < p_r for u in unif]
        rng = orc.ReplayRNG(normals=[normals[t] for t in range(N_REPLAY) if fired[t]], uniforms=[v for u in unif for v in u])
        o = orc.ControlHMC(en, X0, rng=rng, **kw)
    else:
        fired = None
        o = orc.MarkovJumpHMC(en, X0, resample=False, rng=orc.ReplayRNG(normals=normals, exps=exps), **kw)
    return o, X0, V0, normals, unif, exps, fired


@functools.lru_cache(maxsize=None)
def oracle_run(state, D, K, N, L, eps, cls_name='MarkovJumpHMC', n_iter=N_ITER, replay=False):
    """tests/test_gpu_pot_widths.py::oracle_run for the linear model: the oracle's own run of a case from its initial state
    (the device sampler's seed; `replay`: the recorded numbers), no device involved -- the tallies (l, f, r) and fl over
    the compared iterations, whether everything stayed finite, per iteration the number of particles on which the float32
    and the float64 force decide differently, and the float32 spread (the largest over the iterations)."""
    if replay:
        o = _replay_reference(state, D, K, N, L, eps, cls_name)[0]
        exps_all, unif_all = replay_numbers(D, N)[4], replay_numbers(D, N)[3]
    else:
        o = _reference(state, D, K, N, L, eps, cls_name)
    e32, e64 = _energy(D, K, np.float32), _energy(D, K, np.float64)
    spread, ties, finite = np.zeros(3), [], True
    for t in range(n_iter):
        spread = np.maximum(spread, spread32_of_state(o, D, K))
        if cls_name == 'MarkovJumpHMC':
            exps = exps_all[t] if replay else np.asarray(o.rng.stream.unit_exponentials(o.rng.tick), dtype=np.float64)
            ties.append(int(np.sum(_decision(o, e32, exps) != _decision(o, e64, exps))))
        elif replay:        # ControlHMC on recorded uniforms: the accept
            acc = [unif_all[t][0] < np.exp(np.minimum(_proposals(o, en)[1][0][0], 0.0)) for en in (e32, e64)]
            ties.append(int(np.sum(acc[0] != acc[1])))
        else:
            ties.append(int(np.sum(_other_decision(o, e32, cls_name) != _other_decision(o, e64, cls_name))))
        o.sampling_iteration()
        finite = finite and bool(np.isfinite(o.state.X).all() and np.isfinite(o.state.V).all() and
                                 np.isfinite(o.state.H()).all())
    return dict(counts=(o.l_count, o.f_count, o.r_count), finite=finite, ties=ties, spread=spread, n_iter=n_iter,
                fl=o.fl_count, refreshed=o.r_count > 0)


def choose_eps(state, D, K, N, L):
    """the smallest step size of EPS_GRID at which the oracle's own run meets the rule (shares_ok), and that run"""
    for eps in EPS_GRID:
        run = oracle_run(state, D, K, N, L, eps)
        if run['finite'] and shares_ok(D, N, run['counts'], run['n_iter']):
            return eps, run
    raise AssertionError(('no step size of the grid meets the rule', state, D, K, N, L))


def state_of(key):
    return key[1] if isinstance(key[0], str) and key[0] not in STATES else key[0]


def tolerances(key):
    tol = WIDER[key][0] if key in WIDER else BARS[state_of(key)]
    return dict(zip(('delta_rel', 'x_tol', 'e_rtol'), tol))


def _describe(key, D, K, N, L, n_iter=N_ITER):
    """the case, the instance it reaches, the oracle's own tallies, its float32 spread and its allowance"""
    state, total = state_of(key), N * n_iter
    return ('%s D=%d K=%d N=%d L=%d eps=%g %s; oracle tallies %s of %d (%s %%); float32 spread %s, allowed %s'
            % (key[0] if key[0] not in STATES else 'mjhmc', D, K, N, L, EPS[key], _instance(state, D, K),
               ' / '.join('%d' % c for c in SHARES[key]), total, ' / '.join('%.1f' % (100.0 * c / total) for c in SHARES[key]),
               ' '.join('%.2g' % v for v in SPREAD[key]), ' '.join('%.2g' % v for v in tolerances(key).values())))


# ---------------------------------------------------------------------------------------------
# single evaluations: lin_eval_kernel, both state types
# ---------------------------------------------------------------------------------------------
EVAL = [(D, K, 70) for D, K in SHAPES] + [(D, K, N) for D, K in SMALL_BATCH for N in (1, 33)]


@gpu
@pytest.mark.parametrize('state', STATES)
@pytest.mark.parametrize('D,K,N', EVAL)
def test_single_evaluation(D, K, N, state):
    """d.E / d.dEdX against the float32 NumPy force at the bars of tests/test_gpu_linear.py: the mask j < K of the energy and
    of phi, q's stride, the padded state rows, a ragged tile.  (tests/test_linear_widths_cpu.py: a padded expert counted or q
    read at another stride moves E by more than 10 bars.)"""
    X = _x0(D, N)
    d = _dist(D, K, X, state)
    Er, Gr = restated(*_model(D, K))
    E, G = d.E(X), d.dEdX(X)
    assert E.shape == (1, N) and G.shape == (D, N)
    eE, eG = rel(E, Er(X)), rel(G, Gr(X))
    print('eval D=%d K=%d N=%d %s state, %s: E %.3g dEdX %.3g' % (D, K, N, state, _instance(state, D, K, 'lin_eval'), eE, eG))
    assert eE < EVAL_BARS[0] and eG < EVAL_BARS[1], (D, K, N, state, eE, eG)
    assert (d.E_count, d.dEdX_count) == (N, N)


# ---------------------------------------------------------------------------------------------
# MarkovJumpHMC
# ---------------------------------------------------------------------------------------------
def _call_of_several(state, D, K, N, L, eps, tag0):
    """sample(N_FUSED, preserve_order=True) on one sampler against N_FUSED sampling_iteration calls on its twin, from the
    initial state: bit for bit (tests/test_gpu_linear.py::test_fused_call_equals_single_iterations_and_replay)"""
    a, c = _device(state, D, K, N, L, eps), _device(state, D, K, N, L, eps)
    out = a.sample(N_FUSED, preserve_order=True)
    assert out.shape == (D, N, N_FUSED) and np.isfinite(out).all()
    for t in range(N_FUSED):
        c.sampling_iteration()
        assert np.array_equal(c.state.X, out[:, :, t]), (tag0, 'a call of several iterations: X', t)
    for f in ('X', 'V', 'EX'):
        assert np.array_equal(getattr(a.state, f), getattr(c.state, f)), (tag0, 'a call of several iterations', f)
    assert (a.l_count, a.f_count, a.r_count) == (c.l_count, c.f_count, c.r_count), (tag0, 'a call of several iterations: tallies')
    assert a.l_count + a.f_count + a.r_count == N_FUSED * N
    d, e = a.distribution, c.distribution
    assert (d.E_count, d.dEdX_count) == (e.E_count, e.dEdX_count), (tag0, 'a call of several iterations: evaluation counters')


def _errors(s, o, scale):
    """what check_iteration has just held to (x_tol, e_rtol), as figures: the largest error of X and V and of EX and EV, in
    its measures, on the particles whose transition is the oracle's"""
    same = s._dev.read(8) == o.last_transition
    st, os_ = s.state, o.state
    eX = float(np.abs(st.X[:, same] - os_.X[:, same]).max()) / max(1.0, float(np.abs(os_.X).max()))
    eV = float(np.abs(st.V[:, same] - os_.V[:, same]).max()) / max(1.0, float(np.abs(os_.V).max()))
    eE = max(float(np.abs(st.EX[0, same] - os_.EX[0, same]).max()), float(np.abs(st.EV[0, same] - os_.EV[0, same]).max())) / scale
    return np.array([max(eX, eV), eE])


@gpu
@pytest.mark.parametrize('state', STATES)
@pytest.mark.parametrize('D,K,N,L', MJ_CASES)
def test_iterations_match_oracle(D, K, N, L, state):
    """sampling_iteration() through check_iteration with a resync after every iteration: transitions equal or provable near
    ties, X, V, EX, EV, the cache flags and the dwelling times within the case's allowance; l + f + r and, while no near tie
    has occurred, the evaluation counters and the tallies are the oracle's and the table's.  (D, K) in TWO at N = 70, L = 5:
    a call of three iterations against three single ones follows, bit for bit."""
    key = (state, D, K, N, L)
    eps, tol = EPS[key], tolerances(key)
    tag0 = _describe(key, D, K, N, L)
    print(tag0)
    s = _device(state, D, K, N, L, eps)
    o = _reference(state, D, K, N, L, eps)
    d, en = s.distribution, o.energy
    if state == 'float64':
        assert np.allclose(s.state.V, o.state.V, rtol=0, atol=1e-13), (tag0, 'tick-0 momenta')
    else:
        assert np.array_equal(s.state.X, o.state.X) and np.allclose(s.state.V, o.state.V, rtol=0, atol=1e-6), (tag0, 'tick 0')
    resync(s, o)
    ties, worst = 0, np.zeros(2)
    for t in range(N_ITER):
        before = (d.E_count, d.dEdX_count, en.E_count, en.dEdX_count)
        scale = max(1.0, float(np.abs(o.state.H()).max()))
        ties += check_iteration(s, o, tag='%s, iteration %d' % (tag0, t), **tol)
        worst = np.maximum(worst, _errors(s, o, scale))
        assert s.l_count + s.f_count + s.r_count == (t + 1) * N, (tag0, t, 'l + f + r')
        if ties == 0:
            assert (d.E_count - before[0], d.dEdX_count - before[1]) == (en.E_count - before[2], en.dEdX_count - before[3]), \
                (tag0, t, 'evaluation counters')
        resync(s, o)
    if ties == 0:
        assert (s.l_count, s.f_count, s.r_count) == (o.l_count, o.f_count, o.r_count), (tag0, 'tallies')
        assert (s.l_count, s.f_count, s.r_count) == SHARES[key], (tag0, 'the device run does not make the moves of the table')
    assert min(s.l_count, s.f_count, s.r_count) >= 1, (tag0, 'a kind of move the step size was chosen for never occurred')
    print('%s: %d near ties in %d transitions; device L / F / R = %d / %d / %d; largest error on the agreeing particles: X, V %.3g EX, EV %.3g'
          % (tag0, ties, N_ITER * N, s.l_count, s.f_count, s.r_count, worst[0], worst[1]))
    X = s.state.X
    assert (np.abs(X - f32(X)).max() == 0) == (state == 'float32'), (tag0, 'the state type')
    if (D, K) in TWO and (N, L) == (70, 5):
        _call_of_several(state, D, K, N, L, eps, tag0)


# ---------------------------------------------------------------------------------------------
# the other sampler families
# ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('state', STATES)
@pytest.mark.parametrize('D,K', CONTROL)
def test_control_hmc_matches_oracle(D, K, state):
    """ControlHMC (Metropolis accept, flip, the batch-wide momentum refresh, whose last Box-Muller pair an odd D cuts and
    whose normals must stay out of the padded rows) through check_control_iteration, N = 70, L = 5, the step size of the
    MarkovJumpHMC case."""
    N, L = 70, 5
    key = ('control', state, D, K)
    eps, tol = EPS[key], tolerances(key)
    tag0 = _describe(key, D, K, N, L)
    print(tag0)
    s = _device(state, D, K, N, L, eps, 'ControlHMC')
    o = _reference(state, D, K, N, L, eps, 'ControlHMC')
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
@pytest.mark.parametrize('state', STATES)
@pytest.mark.parametrize('D,K', TWO)
def test_continuous_time_hmc_matches_oracle(D, K, state):
    """ContinuousTimeHMC (MODE = CT), N = 70, L = 5, in the form of
    tests/test_gpu_pot_widths.py::test_continuous_time_hmc_matches_oracle."""
    N, L = 70, 5
    key = ('ct', state, D, K)
    eps, tol = EPS[key], tolerances(key)
    print(_describe(key, D, K, N, L, N_CT))
    s = _device(state, D, K, N, L, eps, 'ContinuousTimeHMC')
    o = _reference(state, D, K, N, L, eps, 'ContinuousTimeHMC')
    resync(s, o)
    for t in range(N_CT):
        s.sampling_iteration()
        o.sampling_iteration()
        # the F clock has rate 1 and R rate p_r: only the FL clock sees energies; with 70 particles a near tie is not expected
        assert (s.fl_count, s.f_count, s.r_count) == (o.fl_count, o.f_count, o.r_count), t
        assert s.fl_count + s.f_count + s.r_count == (t + 1) * N
        assert np.abs(s.state.X - o.state.X).max() <= tol['x_tol'] * max(1.0, np.abs(o.state.X).max())
        assert np.allclose(s.dwelling_times, o.dwelling_times, rtol=1e-3)
        resync(s, o)
    assert min(o.fl_count, o.f_count, o.r_count) > 0
    assert (s.l_count, s.f_count, s.r_count, s.fl_count) == SHARES[key], ('the device run does not make the moves of the table',
                                                                         (s.l_count, s.f_count, s.r_count, s.fl_count))


# ---------------------------------------------------------------------------------------------
# REPLAY = true: every draw is the caller's
# ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('state,cls_name', [('float32', 'MarkovJumpHMC'), ('float64', 'MarkovJumpHMC'), ('float64', 'ControlHMC')])
def test_replay_mode_matches_oracle(state, cls_name):
    """The REPLAY instances at (512, 400): recorded normals, exponentials and uniforms go to both sides exactly as in
    tests/test_gpu_dense_parity.py::test_dense_kernels_in_replay_mode; MarkovJumpHMC's transitions through check_iteration."""
    (D, K), N, L = REPLAY, 70, 5
    mj = cls_name == 'MarkovJumpHMC'
    key = ('replay' if mj else 'replay-control', state, D, K)
    eps, tol = EPS[key], tolerances(key)
    tag0 = _describe(key, D, K, N, L, N_REPLAY)
    print(tag0)
    o, X0, V0, normals, unif, exps, fired = _replay_reference(state, D, K, N, L, eps, cls_name)
    from mjhmc_amd.samplers import markov_jump_hmc as M
    kw = dict(resample=False) if mj else {}
    s = getattr(M, cls_name)(distribution=_dist(D, K, X0, state), Vinit=V0, seed=1, epsilon=eps, beta=BETA, num_leapfrog_steps=L, **kw)
    resync(s, o)
    ties = 0
    for t in range(N_REPLAY):
        if mj:
            # check_iteration drives both sides itself: hand the recorded numbers to the device through a one-shot patch
            step = s.sampling_iteration
            s.sampling_iteration = lambda step=step, t=t: step(replay=[(normals[min(o.rng.n_normals_used, N_REPLAY - 1)], exps[t])])
            try:
                ties += check_iteration(s, o, tag='%s, iteration %d' % (tag0, t), **tol)
            finally:
                del s.sampling_iteration
        else:
            s.sampling_iteration(replay=[(normals[t] if fired[t] else np.zeros((D, N)), np.concatenate([unif[t][0], unif[t][1], [unif[t][2]]]))])
            o.sampling_iteration()
            tr = s._dev.read(8)
            acc_o, flip_o = np.isin(np.arange(N), o.last_fl_idx), np.isin(np.arange(N), o.last_flip_idx)
            assert np.array_equal(((tr >> 1) & 1).astype(bool), flip_o), (tag0, t, 'flips')
            same = (tr & 1).astype(bool) == acc_o
            ties += int((~same).sum())
            assert np.abs(s.state.X[:, same] - o.state.X[:, same]).max() <= tol['x_tol'] * max(1.0, float(np.abs(o.state.X).max())), (tag0, t, 'X')
            assert np.abs(s.state.V[:, same] - o.state.V[:, same]).max() <= tol['x_tol'] * max(1.0, float(np.abs(o.state.V).max())), (tag0, t, 'V')
        resync(s, o)
    assert ties <= 1, (tag0, 'near ties', ties)
    got = (s.l_count, s.f_count, s.r_count) + (() if mj else (s.fl_count,))
    if ties == 0:
        assert got == SHARES[key], (tag0, 'the device run does not make the moves of the table', got)
    if not mj:
        assert sum(fired) > 0 and s.r_count > 0, (tag0, 'no momentum refresh in the compared iterations')
    print('%s: %d near ties; device tallies %s' % (tag0, ties, got))


# ---------------------------------------------------------------------------------------------
# lin_leap_kernel
# ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('D,K', TWO)
def test_leapfrog_operator(D, K, n):
    """DeviceEnergy.leapfrog(..., dtype='float32') against the oracle state's L operator on the float32 force with float32
    rounding, at the bars of tests/test_gpu_linear.py::test_state_operations."""
    N = 70
    eps = EPS[('float32', D, K, N, 5)]
    X, V = f32(1.3 * _x0(D, N)), f32(np.random.RandomState(8).randn(D, N))
    o = orc.MarkovJumpHMC(_energy(D, K, np.float32), X, V0=V, epsilon=eps, beta=BETA, num_leapfrog_steps=n, resample=False,
                          rng=orc.ReplayRNG(), state_rounding=f32)
    Zo = o.state.clone().L()
    Xd, Vd, EXd, EVd, Gd = _dist(D, K, X, 'float32').bind().leapfrog(X, V, eps, n, dtype='float32')
    err = [rel(Xd, Zo.X), rel(Vd, Zo.V), rel(EXd, Zo.EX[0]), rel(EVd, Zo.EV[0]), rel(Gd, Zo.dEdX)]
    print('leapfrog D=%d K=%d n=%d eps=%g %s: X %.3g V %.3g EX %.3g EV %.3g dEdX %.3g'
          % ((D, K, n, eps, _instance('float32', D, K, 'lin_leap')) + tuple(err)))
    assert max(err[:4]) < LEAP_BARS[0] and err[4] < LEAP_BARS[1], (D, K, n, err)
    assert np.abs(Xd - X).max() > 0.1 * eps


# ---------------------------------------------------------------------------------------------
# the float64 kernel against its multi-pass twin, bit for bit
# ---------------------------------------------------------------------------------------------
_FIELDS = ('X', 'V', 'DEDX', 'EX', 'EV', 'HFLF', 'DWELL', 'TRANS')
# tests/test_gpu_pot64_tail_blocks.py::_CASES: every pair of (L, mode), (N, L) and (N, mode) occurs
_TWIN_CASES = [(33, 1, 'MJHMC'), (32, 1, 'CTHMC'), (33, 1, 'CONTROL'),
               (32, 2, 'MJHMC'), (33, 2, 'CTHMC'), (32, 2, 'CONTROL'),
               (33, 5, 'MJHMC'), (32, 5, 'CTHMC'), (33, 5, 'CONTROL')]


def _pair(D, K, N, mode, exprs, seed=11):
    """the product library's sampler (lin64_jump_kernel) and the test build's, which MJHMC_POT64_MULTIPASS=1 sends through
    lin_eval_kernel and row passes; tests/test_gpu_pot64_tail_blocks.py::_pair from DeviceEnergy.from_linear"""
    from mjhmc_amd import engine, _lib
    W, b, q = _model(D, K)
    ens = [engine.DeviceEnergy.from_linear(c, W, b, exprs[0], exprs[1], expert_params=q) for c in (engine.context(0), hooks_context(0))]
    return [engine.DeviceSampler(en, _x0(D, N), seed=seed, dtype='float64', mode=getattr(_lib, 'MODE_' + mode)) for en in ens]


def _compare(pair, tag, finite, mode):
    from mjhmc_amd import _lib
    assert_multipass_pair_equal(pair, tag, fields=_FIELDS)
    for f in _FIELDS if finite else ():
        fa, fb = pair[0].read(getattr(_lib, 'F_' + f)), pair[1].read(getattr(_lib, 'F_' + f))
        if f in ('X', 'V', 'DEDX', 'EX', 'EV'):
            assert np.isfinite(fa).all() and np.isfinite(fb).all(), (tag, f, 'not finite')
        if f == 'HFLF':       # NaN is the empty cache's mark: the cached energies must be finite
            cached = [s.read(_lib.F_CACHE).astype(bool) for s in pair]
            assert np.array_equal(cached[0], cached[1]) and np.array_equal(~np.isnan(fa), cached[0]), (tag, 'cache flags')
            assert np.isfinite(fa[cached[0]]).all(), (tag, f, 'not finite')
        if f == 'DWELL' and mode != 'CONTROL':
            assert np.isfinite(fa).all() and (fa > 0).all(), (tag, f, 'not finite')


@gpu
@pytest.mark.parametrize('pair_name', ['softplus', 'l1'])
@pytest.mark.parametrize('N,L,mode', _TWIN_CASES)
@pytest.mark.parametrize('D,K', TWINS)
def test_float64_kernel_equals_its_multipass_twin(D, K, N, L, mode, pair_name, monkeypatch):
    """1 + 3 iterations of lin64_jump_kernel and of the multi-pass form of the same arithmetic (whole-chunk gemm_dim, no
    parked momentum, no register-resident position), eps = 0.1 and p_r = 0.4 so that R-movers list inverse-L items.  With
    the L1 pair every padded expert's f'(0) is 0/0: every field must be finite in both forms."""
    exprs = (ENERGY, GRAD) if pair_name == 'softplus' else L1
    print('twin D=%d K=%d N=%d L=%d %s %s %s' % (D, K, N, L, mode, pair_name, _instance('float64', D, K)))
    pair = _pair(D, K, N, mode, exprs)
    hparams = (0.1, L, 0.4, 0.3) if mode == 'CONTROL' else (0.1, L, 0.4, 1.0)
    stats = [[], []]
    for n_it in (1, 3):
        a, b = iterate_multipass_pair(pair, n_it, hparams, monkeypatch)
        stats[0] += a
        stats[1] += b
        _compare(pair, (D, K, N, L, mode, pair_name, n_it), pair_name == 'l1', mode)
    assert [t[:7] for t in stats[0]] == [t[:7] for t in stats[1]]
    if mode == 'MJHMC':
        n_flf_run = [t[7] for t in stats[0]]
        assert sum(n_flf_run) > 0, n_flf_run                      # inverse-L items were integrated
    for s in pair:
        s.close()
