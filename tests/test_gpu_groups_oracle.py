"""GPU: the group form of the energies that couple coordinates across the lanes of a group (FunnelNealF, FunnelRefF,
MMGaussF, the hipRTC coupled expressions S[k]; RoughWellF for the lane mapping and the padding masks) against the NumPy
oracle on the same Philox streams, at every group width from 8 to 64 lanes and every elements-per-lane form -- the widths
tests/test_gpu_rows_oracle.py (9 <= ndims <= 33) leaves out.  The machinery is that module's: `sample(n,
preserve_order=True)` or n `sampling_iteration()` calls on the product's classes, the oracle stepped alongside, the
tallies, transitions and cache flags exact, X, V, EX, EV, cached H_flf and the dwelling times within tolerance, the
oracle resynchronised to the device state between calls.

Shapes (tests.helpers.group_shape restates pick_shape; tests/test_group_shapes_cpu.py pins the table without a GPU).
`full`: the row's 16-byte chunks fill the group (launch_jump_t's condition for the FULLROW instances).  255 and 1023 are
full in that sense -- their one padding ELEMENT sits in the last chunk -- so they reach the same instances as 256 and
1024 and depend on the dim_of masks alone; 253 and 1021 are the odd ragged widths.

  float64   D      E   G  full  fused MarkovJumpHMC call            sampling_iteration()
            34     8   8  no    generic predicated (WPP 0)          generic predicated
            64     8   8  yes   generic FULLROW (WPP 0)             generic FULLROW
            100    8  16  no    generic predicated                  generic predicated
            128    8  16  yes   generic FULLROW                     generic FULLROW
            253    8  32  no    generic predicated (odd D)          --
            255    8  32  yes   block-decide WPP 6 (odd D)          --
            256    8  32  yes   block-decide WPP 6                  generic FULLROW
            300    8  64  no    generic predicated                  --
            512    8  64  yes   block-decide WPP 5                  WPP 1         (test hooks, no block decide: fused WPP 1)
            513   16  64  no    E = 16 predicated                   E = 16 predicated
            1021  16  64  no    E = 16 predicated (odd D)           --
            1023  16  64  yes   E = 16 block-decide WPP 5 (odd D)   --
            1024  16  64  yes   E = 16 block-decide WPP 5           E = 16 WPP 1
  float32   64    16   4  yes   WPP 3                               WPP 3
            100   16   8  no    generic predicated                  generic predicated
            1024  16  64  yes   block-decide WPP 5                  WPP 1
            1025  32  64  no    E = 32 predicated                   E = 32 predicated
            2048  32  64  yes   E = 32 block-decide WPP 5           E = 32 WPP 1
  ControlHMC / HMC / HMCBase / ContinuousTimeHMC always take the predicated generic instance of their mode; the coupled
  expressions always take the predicated generic single-iteration instance (a fused call is a sequence of them).

Inputs.  L = 6 leapfrog steps, beta = 0.2 (p_r = 0.112), `_initial_state` of tests/test_gpu_rows_oracle.py (the rough well:
3 N(0, 1)); 130 particles, 70 where a particle takes a whole wave (G = 64): a ragged last wave and more than one wave at
every width, and the oracle holds the whole batch.  The step sizes are chosen, with the oracle alone, so that no case
passes trivially: over the iterations a case compares, each of L, F and R moves is at least 2 % of the
particle-iterations of the ORACLE's own run and nothing becomes non-finite (EPS_C below: epsilon = c / sqrt(D)).

  oracle-only shares of L / F / R moves in per cent, 12 iterations (literal: 9) from the initial state
            neal, coupled c = 2.5   mm3 c = 6 (D <= 512), 8      rough c = 4        literal c = 0.06
  D = 34    48.2 / 22.8 / 29.0      58.9 / 32.7 /  8.4           73.1 / 17.5 / 9.4  83.5 /  7.5 /  9.0
      100   60.3 / 22.3 / 17.4      67.4 / 21.6 / 11.0           83.4 /  8.7 / 7.9  82.8 /  8.3 /  8.9
      256   68.5 / 17.1 / 14.4      87.5 /  3.5 /  9.0           83.0 /  8.7 / 8.3  81.5 /  9.9 /  8.6
      512   71.5 / 16.3 / 12.1      78.9 / 11.2 /  9.9           80.2 /  8.0 / 11.8 78.9 / 10.6 / 10.5
      1023  75.4 / 13.1 / 11.5      76.4 / 12.6 / 11.0           78.9 / 11.8 / 9.3  76.3 / 12.4 / 11.3
  (every case's own shares: the table below the imports.)

Tolerances.  float64: `close` / RTOL = 1e-10 of tests/test_gpu_parity.py, except where WIDER below names a case: there
the allowance is 4 x the largest relative difference between the oracle's run of that case and the same run from inputs
moved by one ulp (measured on the CPU with the oracle alone, never against device output).  float32 state: delta_rel,
x_tol and e_rtol are 4 x the spread between a float32 NumPy restatement of the energy (`_restated32`: the oracle's
operations on float32 arrays, the leapfrog steps included) and the float64 oracle on the case's own states, measured by
`_spread32` at the start of each case (printed; the values met are listed at F32_SPREAD below).

What float32 cannot state.  The mixture as coded is -log(exp(-a) + exp(-b)), a and b the squared distances to the two
modes, and its force goes through exp(4 s x_0): in float32 the force is NaN for x_0 > 88 / 24 = 3.7 (the + mode of
separation 3 sits at 6) and the energy is +inf from a, b > 103, which a chain reaches from about 200 dimensions up (a is
ndims / 2 at stationarity; at 2048 dimensions even the float64 oracle's exp underflows).  So the float32 mixture runs at
64 and 100 dimensions, every particle started at the - mode, and has no finite reference at 1024, 1025 and 2048: the
float32 E = 16 / 32 wave-per-particle forms are covered by the funnel alone."""
import numpy as np
import pytest

from oracle import mjhmc_oracle as orc
from tests import test_gpu_rows_oracle as R
from tests.helpers import (bits_equal, check_control_iteration, check_iteration, group_shape, hooks_context, jump_instance,
                           resync)
from tests.test_gpu_parity import close, RTOL

gpu = pytest.mark.gpu
np.seterr(all='ignore')

L = 6
BETA = R.BETA
EPS_C = {'neal': 2.5, 'coupled': 2.5, 'rough': 4.0, 'literal': 0.06}
F64_DIMS = (34, 64, 100, 128, 255, 256, 300, 512, 513, 1023, 1024)
ODD_RAGGED = (253, 1021)
F32_DIMS = (64, 100, 1024, 1025, 2048)
SOME = (34, 100, 256, 512, 1023)


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _eps(name, D):
    c = (6.0 if D <= 512 else 8.0) if name == 'mm3' else EPS_C[name]
    return c / np.sqrt(D)


def _n(D, dtype='float64'):
    return 70 if group_shape(D, dtype)[1] == 6 else 130


def _n_iter(name):
    return 3 if name == 'literal' else 4


def _path(D, fused, dtype='float64', mode='mjhmc', block_decide=True, name=''):
    E, logG, full = group_shape(D, dtype)
    fr, wpp = (False, 0) if name == 'coupled' else jump_instance(E, logG, full, fused, mode, block_decide)
    return '%s E=%d G=%d %s WPP=%d' % ('fused' if fused else 'single', E, 1 << logG, 'FULLROW' if fr else 'predicated', wpp)


# Every MarkovJumpHMC float64 case: the instance it selects, the shares of L / F / R moves (per cent of the
# particle-iterations) in the ORACLE's own run over the iterations the case compares (fused: 3 calls, single: 2 rounds,
# compact: 16 400 particles, a column subset), the largest relative difference (of X, V, EX, EV and the dwelling times, the
# measure of tests/test_gpu_rows_oracle._rel_err) between that run and the same run with X and V moved by one ulp at the
# start of every call, and the allowance where 4 x that exceeds RTOL (WIDER).  The coupled expressions always run the
# predicated generic instance, one launch per iteration; they share the Neal funnel's oracle run.
#   call     energy       D  instance                     L  /  F   /  R       one ulp  allowed
#   fused    neal        34  E=8 G=8 ragged WPP=0        48.2 / 22.8 / 29.0   1.7e-10  6.8e-10
#   fused    coupled     34  E=8 G=8 ragged WPP=0        48.2 / 22.8 / 29.0   1.7e-10  6.8e-10
#   fused    neal        64  E=8 G=8 full WPP=0          54.9 / 22.2 / 22.9   4.2e-12  -
#   fused    neal       100  E=8 G=16 ragged WPP=0       60.3 / 22.3 / 17.4   1e-12    -
#   fused    coupled    100  E=8 G=16 ragged WPP=0       60.3 / 22.3 / 17.4   1e-12    -
#   fused    neal       128  E=8 G=16 full WPP=0         62.3 / 21.3 / 16.4   3.7e-13  -
#   fused    neal       255  E=8 G=32 full WPP=6         66.1 / 21.5 / 12.4   7.7e-12  -
#   fused    neal       256  E=8 G=32 full WPP=6         68.5 / 17.1 / 14.4   6.2e-13  -
#   fused    coupled    256  E=8 G=32 full WPP=0         68.5 / 17.1 / 14.4   6.2e-13  -
#   fused    neal       300  E=8 G=64 ragged WPP=0       66.4 / 20.2 / 13.3   3.2e-13  -
#   fused    neal       512  E=8 G=64 full WPP=5         71.5 / 16.3 / 12.1   5.5e-13  -
#   fused    coupled    512  E=8 G=64 full WPP=0         71.5 / 16.3 / 12.1   5.5e-13  -
#   fused    neal       513  E=16 G=64 ragged WPP=0      71.2 / 15.5 / 13.3   5e-13    -
#   fused    neal      1023  E=16 G=64 full WPP=5        75.4 / 13.1 / 11.5   1.6e-12  -
#   fused    coupled   1023  E=16 G=64 full WPP=0        75.4 / 13.1 / 11.5   1.6e-12  -
#   fused    neal      1024  E=16 G=64 full WPP=5        72.7 / 15.2 / 12.0   7.4e-10  3e-09
#   fused    neal       253  E=8 G=32 ragged WPP=0       68.3 / 20.4 / 11.2   1.2e-12  -
#   fused    neal      1021  E=16 G=64 ragged WPP=0      73.2 / 15.8 / 11.0   9.7e-13  -
#   fused    mm3         34  E=8 G=8 ragged WPP=0        58.9 / 32.7 /  8.4   4.8e-14  -
#   fused    mm3         64  E=8 G=8 full WPP=0          66.7 / 24.9 /  8.3   1e-13    -
#   fused    mm3        100  E=8 G=16 ragged WPP=0       67.4 / 21.6 / 11.0   1.4e-13  -
#   fused    mm3        128  E=8 G=16 full WPP=0         79.7 /  6.8 / 13.5   2.1e-13  -
#   fused    mm3        255  E=8 G=32 full WPP=6         87.4 /  3.4 /  9.2   1.3e-12  -
#   fused    mm3        256  E=8 G=32 full WPP=6         87.5 /  3.5 /  9.0   6.8e-13  -
#   fused    mm3        300  E=8 G=64 ragged WPP=0       83.0 /  6.2 / 10.8   1e-12    -
#   fused    mm3        512  E=8 G=64 full WPP=5         78.9 / 11.2 /  9.9   1.5e-12  -
#   fused    mm3        513  E=16 G=64 ragged WPP=0      83.1 /  6.3 / 10.6   3.9e-12  -
#   fused    mm3       1023  E=16 G=64 full WPP=5        76.4 / 12.6 / 11.0   1.4e-12  -
#   fused    mm3       1024  E=16 G=64 full WPP=5        75.2 / 14.2 / 10.6   1.5e-12  -
#   fused    mm3        253  E=8 G=32 ragged WPP=0       86.5 /  4.6 /  9.0   1.1e-12  -
#   fused    mm3       1021  E=16 G=64 ragged WPP=0      76.5 / 12.7 / 10.7   8.2e-13  -
#   fused    literal     34  E=8 G=8 ragged WPP=0        83.5 /  7.5 /  9.0   6.2e-13  -
#   fused    literal    100  E=8 G=16 ragged WPP=0       82.8 /  8.3 /  8.9   1.9e-12  -
#   fused    literal    256  E=8 G=32 full WPP=6         81.5 /  9.9 /  8.6   1.8e-12  -
#   fused    literal    512  E=8 G=64 full WPP=5         78.9 / 10.6 / 10.5   1e-12    -
#   fused    literal   1023  E=16 G=64 full WPP=5        76.3 / 12.4 / 11.3   2.5e-12  -
#   fused    rough       34  E=8 G=8 ragged WPP=0        73.1 / 17.5 /  9.4   7.6e-09  3e-08
#   fused    rough      100  E=8 G=16 ragged WPP=0       83.4 /  8.7 /  7.9   7.3e-11  2.9e-10
#   fused    rough      256  E=8 G=32 full WPP=6         83.0 /  8.7 /  8.3   1.6e-11  -
#   fused    rough      512  E=8 G=64 full WPP=5         80.2 /  8.0 / 11.8   6.3e-12  -
#   fused    rough     1023  E=16 G=64 full WPP=5        78.9 / 11.8 /  9.3   1.9e-12  -
#   single   neal        64  E=8 G=8 full WPP=0          53.9 / 21.9 / 24.1   1.9e-12  -
#   single   neal       128  E=8 G=16 full WPP=0         61.8 / 20.5 / 17.7   3.1e-13  -
#   single   neal       256  E=8 G=32 full WPP=0         68.6 / 16.9 / 14.5   6e-13    -
#   single   neal       512  E=8 G=64 full WPP=1         72.5 / 15.4 / 12.1   5.5e-13  -
#   single   coupled    100  E=8 G=16 ragged WPP=0       59.5 / 21.8 / 18.7   1e-12    -
#   single   coupled    512  E=8 G=64 full WPP=0         72.5 / 15.4 / 12.1   5.5e-13  -
#   single   neal       513  E=16 G=64 ragged WPP=0      71.8 / 14.6 / 13.6   5e-13    -
#   single   neal      1024  E=16 G=64 full WPP=1        74.3 / 14.1 / 11.6   7.4e-10  3e-09
#   single   mm3         64  E=8 G=8 full WPP=0          67.4 / 24.4 /  8.2   1e-13    -
#   single   mm3        128  E=8 G=16 full WPP=0         79.8 /  6.8 / 13.4   1.1e-13  -
#   single   mm3        256  E=8 G=32 full WPP=0         88.6 /  2.6 /  8.8   6.5e-13  -
#   single   mm3        512  E=8 G=64 full WPP=1         79.8 / 10.2 / 10.0   1.5e-12  -
#   single   mm3        513  E=16 G=64 ragged WPP=0      85.0 /  5.4 /  9.6   1.1e-12  -
#   single   mm3       1024  E=16 G=64 full WPP=1        74.8 / 14.5 / 10.7   1.5e-12  -
#   single   literal    100  E=8 G=16 ragged WPP=0       85.4 /  5.9 /  8.7   1.9e-12  -
#   single   literal    512  E=8 G=64 full WPP=1         81.0 / 10.0 /  9.0   1e-12    -
#   single   rough      100  E=8 G=16 ragged WPP=0       85.3 /  7.0 /  7.7   6.5e-11  2.6e-10
#   single   rough      512  E=8 G=64 full WPP=1         80.2 /  8.0 / 11.8   6.3e-12  -
#   compact  neal        64  two launches, E=8 G=8       55.2 / 22.7 / 22.1   1.3e-12  -
#   compact  mm3        100  two launches, E=8 G=16      62.9 / 23.2 / 13.8   3.8e-13  -
#   long     neal       256  E=8 G=32 full WPP=6         68.4 / 18.7 / 12.8   8.1e-10  3.2e-09
#   long     mm3        512  E=8 G=64 full WPP=5         77.9 / 12.8 /  9.3   5.9e-12  -
# the ControlHMC / HMC / HMCBase / ContinuousTimeHMC cases (neal and mm3 at 100 and 1024, 8 iterations): one ulp moves the
# oracle's run by at most 2.3e-12, so RTOL holds; 23 .. 72 % of their proposals are accepted.
WIDER = {('neal', 34, True): (6.8e-10, 1.7e-10), ('coupled', 34, True): (6.8e-10, 1.7e-10),
         ('neal', 1024, True): (3.0e-9, 7.4e-10), ('neal', 1024, False): (3.0e-9, 7.4e-10),
         ('rough', 34, True): (3.0e-8, 7.6e-9), ('rough', 100, True): (2.9e-10, 7.3e-11),
         ('rough', 100, False): (2.6e-10, 6.5e-11), ('neal', 256, 'long'): (3.2e-9, 8.1e-10)}


def _rtol(name, D, fused):
    return WIDER.get((name, D, fused), (RTOL, None))[0]


# ---------------------------------------------------------------------------------------------
# MarkovJumpHMC, float64
# ---------------------------------------------------------------------------------------------
FUSED = ([(name, D) for name in ('neal', 'mm3') for D in F64_DIMS + ODD_RAGGED] +
         [(name, D) for name in ('literal', 'rough', 'coupled') for D in SOME])
SINGLE = ([(name, D) for name in ('neal', 'mm3') for D in (64, 128, 256, 512, 513, 1024)] +
          [(name, D) for name in ('literal', 'rough', 'coupled') for D in (100, 512)])


@gpu
@pytest.mark.parametrize('name,D', FUSED)
def test_fused_calls_match_oracle(name, D):
    """sample(n, preserve_order=True), n = 4 (the literal funnel: 3), three calls in a row with a resync between them."""
    worst = R._run_and_compare(name, D, L, _n(D), _n_iter(name), calls=3, fused=True, rtol=_rtol(name, D, True),
                               eps=_eps(name, D), path=_path(D, True, name=name))
    print('%s D=%d %s: largest relative differences %s' % (name, D, _path(D, True, name=name), worst))


@gpu
@pytest.mark.parametrize('name,D', SINGLE)
def test_single_iterations_match_oracle(name, D):
    """sampling_iteration() x 4, two rounds with a resync between them: FULLROW WPP = 0 / 1, the predicated forms."""
    worst = R._run_and_compare(name, D, L, _n(D), _n_iter(name), calls=2, fused=False, rtol=_rtol(name, D, False),
                               eps=_eps(name, D), path=_path(D, False, name=name))
    print('%s D=%d %s: largest relative differences %s' % (name, D, _path(D, False, name=name), worst))


LONG = [('neal', 256), ('mm3', 512)]


@gpu
@pytest.mark.parametrize('name,D', LONG)
def test_fused_call_across_the_launch_boundary(name, D):
    """One fused call of 66 iterations, the oracle stepped alongside without a resync: the block-decide kernels (WPP = 6 at
    256, WPP = 5 at 512) draw a slot's waiting-time clocks up front, per launch of at most 64 iterations."""
    rtol = WIDER.get((name, D, 'long'), (RTOL, None))[0]
    worst = R._run_and_compare(name, D, L, _n(D), 66, calls=1, fused=True, rtol=rtol, eps=_eps(name, D),
                               path=_path(D, True) + ', 66 iterations')
    print('%s D=%d, 66 iterations: largest relative differences %s' % (name, D, worst))


@gpu
@pytest.mark.parametrize('name', ['neal', 'mm3'])
def test_fused_wave_per_particle_without_block_decide(name, monkeypatch):
    """The fused WPP = 1 instance (full 64-lane rows, the clocks drawn per iteration) exists behind MJHMC_NO_BLOCK_DECIDE
    of the test-hooks library only."""
    hooks_context(0)
    monkeypatch.setenv('MJHMC_NO_BLOCK_DECIDE', '1')
    R._run_and_compare(name, 512, L, 70, 4, calls=3, fused=True, rtol=_rtol(name, 512, True), eps=_eps(name, 512),
                       path=_path(512, True, block_decide=False) + ' (test hooks)', hooks=True)


@gpu
@pytest.mark.parametrize('name,D', [('neal', 64), ('mm3', 100)])
def test_compacted_two_launch_path(name, D):
    """16 400 particles: a single iteration is the trajectory launch + the jump-process launch (mjhmc_step_kernel), the
    cold list carried from call to call; the oracle holds a column subset, the tallies obey the whole-batch identities."""
    R._run_and_compare(name, D, L, 16400, 4, calls=2, fused=False, rtol=_rtol(name, D, False), eps=_eps(name, D))


# ---------------------------------------------------------------------------------------------
# the other sampler families, float64: always the predicated generic instance of their mode
# ---------------------------------------------------------------------------------------------
def _family_counts(o):
    return dict(l=o.l_count, f=o.f_count, r=o.r_count, fl=o.fl_count)


@gpu
@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'single'])
@pytest.mark.parametrize('D', [100, 1024])
@pytest.mark.parametrize('name', ['neal', 'mm3'])
@pytest.mark.parametrize('cls_name', ['ControlHMC', 'HMC', 'HMCBase', 'ContinuousTimeHMC'])
def test_other_sampler_families(cls_name, name, D, fused):
    """kModeControl / kModeCT on the coupled energies at 16 and 64 lanes (E = 8 ragged, E = 16 full).  Single iterations of
    the discrete-time samplers go through check_control_iteration with no energy allowance: every accept and flip decision
    is the oracle's; fused calls compare every iteration's state and l / f / r / fl tallies, which leaves no room for
    another decision either."""
    N, n, eps = _n(D), 4, _eps(name, D)
    X0 = R._initial_state(name, D, N)
    s = R._sampler(name, D, N, eps, L, BETA, X0, cls_name=cls_name)
    o = R._oracle(name, D, X0, eps, L, BETA, None, cls_name=cls_name)
    assert (s.beta, s.p_r, s.p_flip) == (o.beta, o.p_r, o.p_flip)
    assert close(s.state.V, o.state.V), 'tick-0 momenta'
    jump = cls_name == 'ContinuousTimeHMC'
    tag0 = '%s %s D=%d N=%d %s' % (cls_name, name, D, N, _path(D, fused, mode='ct' if jump else 'control'))
    cmp = R._Compare(RTOL)
    en = o.energy
    for call in range(2):
        if fused:
            out = s.sample(n, preserve_order=True)
            assert out.shape == (D, N, n)
            dwell = s._dev.ring_read_dwell(0, n) if jump else None
            trace = s.trace[-n:]
            evals = []
            for t in range(n):
                tag = '%s, call %d iteration %d' % (tag0, call, t)
                before, e0 = _family_counts(o), (en.E_count, en.dEdX_count)
                o.sampling_iteration()
                want = {k: v - before[k] for k, v in _family_counts(o).items()}
                evals.append((en.E_count - e0[0], en.dEdX_count - e0[1]))
                got = {k: trace[t][k] for k in want}
                assert got == want, (tag, 'tallies', got, 'oracle', want)
                cmp('X', out[:, :, t], o.state.X, tag)
                if jump:
                    cmp('dwelling times', dwell[t], o.dwelling_times, tag)
            assert np.array_equal(s.eval_trace(n), np.array(evals)), (tag0, 'eval_trace')
        else:
            for t in range(n):
                tag = '%s, call %d iteration %d' % (tag0, call, t)
                if jump:
                    s.sampling_iteration()
                    o.sampling_iteration()
                    cmp('dwelling times', s.dwelling_times, o.dwelling_times, tag)
                else:
                    check_control_iteration(s, o, delta_rel=0.0, x_tol=RTOL, e_rtol=RTOL, tag=tag, max_ties=0)
                cmp('X', s.state.X, o.state.X, tag)
        tag = '%s, after call %d' % (tag0, call)
        assert _family_counts(s) == _family_counts(o), (tag, 'counters', _family_counts(s), _family_counts(o))
        assert (s.distribution.E_count, s.distribution.dEdX_count) == (en.E_count, en.dEdX_count), (tag, 'evaluations')
        st = s.state
        cmp('X', st.X, o.state.X, tag)
        cmp('V', st.V, o.state.V, tag)
        cmp('EX', st.EX[0], o.state.EX[0], tag)
        cmp('EV', st.EV[0], o.state.EV[0], tag)
    accepted = o.fl_count + o.l_count if not jump else o.fl_count
    assert 0 < accepted < 2 * n * N, (tag0, 'a trivial case: accepted moves', accepted)


# ---------------------------------------------------------------------------------------------
# float32 state
# ---------------------------------------------------------------------------------------------
def _restated32(name, D):
    """(E, dEdX) of `name` as the oracle computes them, on float32 arrays (Python scalars do not promote them)"""
    if name == 'neal':
        s = 3.0

        def E(X):
            ex = np.exp(-X[0, :])
            return X[0, :] ** 2 / (2. * s ** 2) + 0.5 * ex * np.sum(X[1:, :] ** 2, axis=0) + 0.5 * (D - 1) * X[0, :]

        def G(X):
            ex = np.exp(-X[0, :])
            g = np.empty_like(X)
            g[0, :] = X[0, :] / s ** 2 - 0.5 * ex * np.sum(X[1:, :] ** 2, axis=0) + 0.5 * (D - 1)
            g[1:, :] = X[1:, :] * ex
            return g
    elif name == 'literal':
        s = 1.0

        def E(X):
            return np.sum(-((X[0, :] ** 2) / (s ** 2)) + -((X[1:, :] ** 2) / np.exp(X[0, :])), axis=0)

        def G(X):
            ex = np.exp(-X[0, :])
            g = np.empty_like(X)
            g[0, :] = -2. * (D - 1) * X[0, :] / s ** 2 + ex * np.sum(X[1:, :] ** 2, axis=0)
            g[1:, :] = -2. * X[1:, :] * ex
            return g
    elif name == 'rough':
        s1, s2 = 100, 4

        def E(X):
            return np.sum((X ** 2) / (2 * s1 ** 2) + np.cos(X * 2 * np.pi / s2), axis=0)

        def G(X):
            return X / s1 ** 2 + -np.sin(X * 2 * np.pi / s2) * 2 * np.pi / s2
    else:
        S = np.zeros((D, 1), dtype=np.float32)
        S[0, 0] = 6

        def E(X):
            return -np.log(np.exp(-np.sum((X + S) ** 2, axis=0)) + np.exp(-np.sum((X - S) ** 2, axis=0)))

        def G(X):
            common = np.exp(np.sum(4 * S * X, axis=0))
            return (2 * ((X - S) * common + S + X)) / (common + 1)
    return E, G


def _leap32(G, X, V, eps, n):
    X, V = X.copy(), V.copy()
    for _ in range(n):
        V += -eps / 2. * G(X)
        X += eps * V
        V += -eps / 2. * G(X)
    return X, V


def _spread32_of_state(name, D, o, eps, n_leap, live=None):
    """float32 restatement against the float64 oracle, from the oracle's current (float32-valued) state: the largest
    differences of the energy differences H0 - H(proposal), of the proposal's X and V and of its energies, forward and
    with the momentum reversed, relative as check_iteration takes them.  Over the proposals that can be taken at all:
    |H0 - H(proposal)| <= LIVE_DH (beyond it the rate is below exp(-20) of the others, or the trajectory has blown up and
    its energy, hundreds of times max|H0|, says nothing about a rounding level).  `live`: a list that receives the two
    masks of those proposals (forward, reversed)"""
    E32, G32 = _restated32(name, D)
    en = o.energy
    counts = (en.E_count, en.dEdX_count)
    X, V = o.state.X.astype(np.float32), o.state.V.astype(np.float32)
    H0_32 = (E32(X) + np.sum(V ** 2, axis=0) / 2.).astype(np.float64)
    H0 = o.state.H()[0]
    scale = max(1.0, float(np.abs(H0).max()))
    d_delta = d_x = d_e = 0.0
    for sign in (1, -1):
        Z = o.state.clone()
        if sign < 0:
            Z.F()
        Z.L()
        Xl, Vl = _leap32(G32, X, sign * V, eps, n_leap)
        EX32, EV32 = E32(Xl).astype(np.float64), (np.sum(Vl ** 2, axis=0) / 2.).astype(np.float64)
        fin = np.isfinite(EX32 + EV32) & (np.abs(H0 - Z.H()[0]) <= LIVE_DH)
        if live is not None:
            live.append(fin)
        d_delta = max(d_delta, float(np.abs((H0_32 - EX32 - EV32) - (H0 - Z.H()[0]))[fin].max()) / scale)
        d_x = max(d_x, float(np.abs(Xl - Z.X)[:, fin].max()) / max(1.0, float(np.abs(Z.X[:, fin]).max())),
                  float(np.abs(Vl - Z.V)[:, fin].max()) / max(1.0, float(np.abs(Z.V[:, fin]).max())))
        d_e = max(d_e, float(np.abs(EX32 - Z.EX[0])[fin].max()) / scale, float(np.abs(EV32 - Z.EV[0])[fin].max()) / scale)
    en.E_count, en.dEdX_count = counts
    return d_delta, d_x, d_e


def _spread32(name, D, X0, eps, cls_name, n):
    """the spread over the n iterations of the case, on the oracle's own run: (delta_rel, x_tol, e_rtol) before the margin"""
    o = R._oracle(name, D, X0, eps, L, BETA, None, cls_name=cls_name, state_rounding=f32)
    o.state.V[:] = f32(o.state.V)
    o.state.refresh_EV()
    worst = np.zeros(3)
    for _ in range(n):
        worst = np.maximum(worst, _spread32_of_state(name, D, o, eps, L))
        o.sampling_iteration()
    return worst


MARGIN = 4.0
LIVE_DH = 40.0
# the spreads `_spread32` measured (delta_rel, x_tol, e_rtol before the margin), MarkovJumpHMC: the record of the bars met
F32_SPREAD = {('neal', 64): (3.0e-6, 2.2e-5, 2.2e-6), ('neal', 100): (5.3e-6, 2.8e-5, 4.2e-6),
              ('neal', 1024): (5.2e-7, 2.5e-5, 4.4e-7), ('neal', 1025): (7.1e-7, 3.8e-5, 5.9e-7),
              ('neal', 2048): (6.9e-7, 4.6e-5, 3.6e-7), ('mm3', 64): (3.2e-7, 3.1e-7, 2.1e-7),
              ('mm3', 100): (4.0e-7, 3.3e-7, 1.8e-7)}


def _initial_state32(name, D, N):
    X0 = R._initial_state(name, D, N)
    if name == 'mm3':               # the float32 force is NaN at the + mode (exp(24 x_0) overflows): every particle at the - mode
        X0[0] = -np.abs(X0[0])
    return f32(X0)


F32 = [('neal', D) for D in F32_DIMS] + [('mm3', D) for D in (64, 100)]


@gpu
@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'single'])
@pytest.mark.parametrize('cls_name', ['MarkovJumpHMC', 'ControlHMC'])
@pytest.mark.parametrize('name,D', F32)
def test_float32_state_matches_oracle(name, D, cls_name, fused):
    """float32 state against the oracle with state_rounding = float32 through check_iteration / check_control_iteration:
    transitions equal or provable near ties at the restatement's energy spread, at most tie_ceiling(N) of them, the oracle
    resynchronised after every iteration.  `fused`: a second sampler from the same inputs makes the same iterations in one
    fused call, and every iteration's ring slot and the final state are the checked sampler's, bit for bit -- so the fused
    kernel (WPP = 3 / 5, the predicated forms) stands against the oracle through the single-iteration one."""
    from mjhmc_amd import _lib
    N, n, eps = _n(D, 'float32'), 4, _eps(name, D)
    X0 = _initial_state32(name, D, N)
    spread = _spread32(name, D, X0, eps, cls_name, n)
    tol = dict(zip(('delta_rel', 'x_tol', 'e_rtol'), MARGIN * spread))
    tag0 = '%s %s D=%d N=%d float32 %s' % (cls_name, name, D, N, _path(D, fused, 'float32', 'mjhmc' if cls_name == 'MarkovJumpHMC' else 'control'))
    print('%s: spread %s, allowed %s' % (tag0, spread, tol))
    assert np.all(spread > 0) and np.all(spread < 1e-4), (tag0, 'the float32 restatement is not at float32 rounding level', spread)
    s = R._sampler(name, D, N, eps, L, BETA, X0, cls_name=cls_name, dtype='float32')
    o = R._oracle(name, D, X0, eps, L, BETA, None, cls_name=cls_name, state_rounding=f32)
    assert np.array_equal(s.state.X, X0)
    if fused:
        twin = R._sampler(name, D, N, eps, L, BETA, X0, cls_name=cls_name, dtype='float32')
        out = twin.sample(n, preserve_order=True)
        assert len(twin.trace) == n
    resync(s, o)
    ties = 0
    for t in range(n):
        tag = '%s, iteration %d' % (tag0, t)
        if cls_name == 'MarkovJumpHMC':
            ties += check_iteration(s, o, tag=tag, **tol)
        else:
            ties += check_control_iteration(s, o, tag=tag, **tol)
        if fused:
            assert bits_equal(out[:, :, t], s.state.X), (tag, 'the fused call and the single iterations differ')
            assert twin.trace[t] == s.trace[t], (tag, 'tallies of the fused call', twin.trace[t], s.trace[t])
        resync(s, o)
    if fused:
        for f in ('X', 'V', 'EX', 'EV', 'HFLF', 'DWELL', 'TRANS'):
            assert bits_equal(twin._dev.read(getattr(_lib, 'F_' + f)), s._dev.read(getattr(_lib, 'F_' + f))), (tag0, 'fused / single', f)
    print('%s: %d near ties in %d transitions' % (tag0, ties, n * N))


# ---------------------------------------------------------------------------------------------
# single evaluations and state operators at the same widths (mjhmc_eval_kernel, the leap kernels)
# ---------------------------------------------------------------------------------------------
EVAL = ([(name, D, 'float64') for name in ('neal', 'literal', 'mm3', 'rough') for D in (100, 512, 1023)] +
        [(name, D, 'float32') for name in ('neal', 'literal', 'rough') for D in (100, 2048)] + [('mm3', 100, 'float32')])


def _scaled_err(a, b, scale=None):
    """max |a - b| over max(1, max |b|) (or `scale`), where b is finite"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    fin = np.isfinite(b)
    sc = max(1.0, float(np.abs(b[fin]).max())) if scale is None else scale
    return float(np.abs(a - b)[fin].max()) / sc


@gpu
@pytest.mark.parametrize('name,D,dtype', EVAL)
def test_evaluations_and_state_operators(name, D, dtype):
    """d.E / d.dEdX (mjhmc_eval_kernel) and state.copy().L() / .FLF() / one .leapfrog() (the leap kernels) against the
    oracle's E_val / dEdX_val and clone().L() / .FLF() / .leap(): float64 within RTOL; float32 within 4 x the spread of the
    float32 restatement on this state (`_spread32_of_state`, on the proposals it is measured on: a trajectory that blows
    up amplifies rounding without bound), the evaluations within 4 x its own difference to the oracle
    (differences over the largest magnitude of the compared array, `_scaled_err`)."""
    N, eps = _n(D, dtype), _eps(name, D)
    single = dtype == 'float32'
    X0 = _initial_state32(name, D, N) if single else R._initial_state(name, D, N)
    s = R._sampler(name, D, N, eps, L, BETA, X0, dtype=dtype)
    o = R._oracle(name, D, X0, eps, L, BETA, None, state_rounding=f32 if single else None)
    resync(s, o)
    d, en = s.distribution, o.energy
    tag0 = '%s D=%d %s E=%d G=%d' % ((name, D, dtype) + (group_shape(D, dtype)[0], 1 << group_shape(D, dtype)[1]))
    Eo, Go = en.E_val(X0).reshape(-1), en.dEdX_val(X0)
    if single:
        E32, G32 = _restated32(name, D)
        e_tol = MARGIN * _scaled_err(E32(X0.astype(np.float32)), Eo)
        g_tol = MARGIN * _scaled_err(G32(X0.astype(np.float32)), Go)
        live = []
        sp = _spread32_of_state(name, D, o, eps, L, live)
        assert min(m.sum() for m in live) > N // 2, (tag0, 'most proposals blow up', [int(m.sum()) for m in live])
        x_tol, h_tol = MARGIN * sp[1], MARGIN * sp[2]
        print('%s: allowed E %.3g dEdX %.3g X, V %.3g EX, EV %.3g' % (tag0, e_tol, g_tol, x_tol, h_tol))
        assert 0 < max(e_tol, g_tol, x_tol, h_tol) < 1e-3, (tag0, 'not at float32 rounding level')
    else:
        e_tol = g_tol = x_tol = h_tol = None
        live = [np.ones(N, dtype=bool)] * 2

    def near(what, a, b, tol, scale=None):
        if tol is None:
            assert close(a, b), (tag0, what, 'largest relative difference %.3g' % R._rel_err(a, b))
        else:
            err = _scaled_err(a, b, scale)
            assert np.shape(a) == np.shape(b) and err <= tol, (tag0, what, err, 'allowed', tol)

    near('E', d.E(X0).reshape(-1), Eo, e_tol)
    near('dEdX', d.dEdX(X0), Go, g_tol)
    hs = max(1.0, float(np.abs(o.state.H()).max()))
    for op, m in zip(('L', 'FLF'), live):       # (float32: the proposals the spread was measured on, `_spread32_of_state`)
        Z = getattr(s.state.copy(), op)()
        Zo = getattr(o.state.clone(), op)()
        near(op + ' X', Z.X[:, m], Zo.X[:, m], x_tol)
        near(op + ' V', Z.V[:, m], Zo.V[:, m], x_tol)
        near(op + ' EX', Z.EX[0][m], Zo.EX[0][m], h_tol, None if h_tol is None else hs)
        near(op + ' EV', Z.EV[0][m], Zo.EV[0][m], h_tol, None if h_tol is None else hs)
    Z1, o1 = s.state.copy(), o.state.clone()
    Z1.leapfrog()
    o1.leap()
    near('leapfrog X', Z1.X, o1.X if not single else f32(o1.X), x_tol)
    near('leapfrog V', Z1.V, o1.V if not single else f32(o1.V), x_tol)
