"""CPU: what the ProductOfT width cases (tests/test_gpu_pot_widths.py) rest on, recomputed with the oracle alone.
tests.helpers.pot_padded_dim restates the padded size of the tile kernels (MJHMC_E_PRODUCT_OF_T in csrc/api.hip); if a
threshold moves there, the restatement is updated with it, this table fails, and the widths must be chosen again so that
every edge is still reached.  For every case of the GPU module: the oracle's own run at the chosen step size makes the
tallies of its table -- each of L, F and R at least 2 % of the particle-iterations (ndims <= 2: at least 6 F moves),
everything finite, and no smaller step size of the grid does; the float32 and the float64 force decide differently
(MarkovJumpHMC: the transition; ControlHMC: the accept; ContinuousTimeHMC: the first clock) on at most tie_ceiling(N)
particles of any compared iteration; the float32 spread is the recorded one, and every allowance in WIDER is
max(bar, 4 x spread).  The ControlHMC and ContinuousTimeHMC runs use the seeds of the GPU cases (P.SEEDS).  The fused
call's own allowance (FUSED_WIDER) is max(the case's, 4 x the recorded spread along the oracle's three-iteration path)."""
import numpy as np
import pytest

from tests import test_gpu_pot_widths as P
from tests.helpers import pot_padded_dim, tie_ceiling

# ndims: (DIM, NB, the groups of eight k-rows that hold a row below ndims)
PADDED = {1: (128, 1, 1), 2: (128, 1, 1), 7: (128, 1, 1), 8: (128, 1, 1), 9: (128, 1, 2), 32: (128, 1, 4), 33: (128, 1, 5),
          36: (128, 1, 5), 64: (128, 1, 8), 65: (128, 1, 9), 120: (128, 1, 15), 121: (128, 1, 16), 127: (128, 1, 16),
          128: (128, 1, 16), 129: (256, 2, 17), 255: (256, 2, 32), 256: (256, 2, 32), 257: (512, 4, 33), 511: (512, 4, 64),
          512: (512, 4, 64)}


@pytest.mark.parametrize('D', sorted(PADDED))
def test_padded_dim_table(D):
    DIM, NB, groups = PADDED[D]
    assert pot_padded_dim(D) == (DIM, NB) and DIM == 128 * NB and D <= DIM
    assert -(-D // 8) == groups and 8 * (groups - 1) < D <= 8 * groups


def test_padded_dim_thresholds_and_the_cases_widths():
    assert [pot_padded_dim(D)[1] for D in range(1, 513)] == [1] * 128 + [2] * 128 + [4] * 256
    for D in (0, 513):
        with pytest.raises(ValueError):
            pot_padded_dim(D)
    assert set(P.WIDTHS) <= set(PADDED)
    assert set(P.WIDTHS) == {1, 2, 7, 8, 9, 33, 65, 127, 128, 129, 255, 256, 257, 511} | {36, 512}
    assert {pot_padded_dim(D)[1] for D in P.CONTROL} == {pot_padded_dim(D)[1] for D in P.FUSED} == {1, 2, 4}
    cases = {(D, N, L) for D, N, L in P.MJ_CASES}
    assert cases == set(P.TABLE) and len(P.MJ_CASES) == len(cases)
    assert all((D, 70, 5) in cases for D in P.WIDTHS)
    assert all((D, 70, L) in cases for D in (9, 33, 128, 129, 257, 511) for L in (1, 2))
    assert all((D, N, 5) in cases for D in (9, 129, 257) for N in (1, 33))
    assert set(P.OTHER) == {('control', s, D) for s in P.STATES for D in P.CONTROL} | {('ct', 'float32', 33)}
    assert set(P.FUSED_PATH_SPREAD) == {(s, D, 70, 5) for s in P.STATES for D in P.FUSED}
    assert all(eps in P.EPS_GRID for eps in P.EPS.values())


def _same_spread(got, recorded):
    """the recorded figure is the measured one to its two digits"""
    return np.allclose(got, recorded, rtol=0.05, atol=0)


@pytest.mark.parametrize('state', P.STATES)
@pytest.mark.parametrize('D,N,L', P.MJ_CASES)
def test_markov_jump_case_on_the_oracle_alone(D, N, L, state):
    key = (state, D, N, L)
    eps = P.EPS[key]
    run = P.oracle_run(state, D, N, L, eps, fused=key in P.FUSED_PATH_SPREAD)
    assert run['finite'], key
    assert run['counts'] == P.SHARES[key], (key, 'the table no longer holds the shares of the oracle run', run['counts'])
    assert P.shares_ok(D, N, run['counts'], run['n_iter']), (key, run['counts'])
    if D <= 2:
        assert run['counts'][1] >= P.MIN_F_NARROW
    else:
        assert min(run['counts']) >= 0.02 * N * run['n_iter']
    assert len(run['ties']) == run['n_iter'] and max(run['ties']) <= tie_ceiling(N), (key, 'near ties of the inputs', run['ties'])
    assert _same_spread(run['spread'], P.SPREAD[key]), (key, 'spread', run['spread'], P.SPREAD[key])
    if key in P.FUSED_PATH_SPREAD:      # the fused call's spread is measured on (nearly) the whole batch
        assert run['fused_compared'] >= N - tie_ceiling(N), (key, 'particles the fused path spread compares', run['fused_compared'])
        assert _same_spread(run['fused_spread'], P.FUSED_PATH_SPREAD[key]), (key, 'fused path spread', run['fused_spread'])


@pytest.mark.parametrize('key', sorted(P.OTHER))
def test_other_sampler_case_on_the_oracle_alone(key):
    kind, state, D = key
    cls_name, N, n = ('ControlHMC', 70, P.N_ITER) if kind == 'control' else ('ContinuousTimeHMC', 60, 5)
    run = P.oracle_run(state, D, N, 5, P.EPS[key], cls_name, n)      # seed P.SEEDS[cls_name]: the GPU case's
    assert run['finite'] and P.EPS[key] == P.EPS[(state, D, 70, 5)]
    assert len(run['ties']) == n and max(run['ties']) <= tie_ceiling(N), (key, 'near ties of the inputs', run['ties'])
    assert run['counts'] + (run['fl'],) == P.SHARES[key], (key, run['counts'], run['fl'])
    if kind == 'control':         # a refresh, and neither every proposal accepted nor none
        assert run['refreshed'] and 0 < run['counts'][0] + run['fl'] < n * N
    else:
        assert min(run['fl'], run['counts'][1], run['counts'][2]) > 0
    assert _same_spread(run['spread'], P.SPREAD[key]), (key, 'spread', run['spread'], P.SPREAD[key])


@pytest.mark.parametrize('state', P.STATES)
@pytest.mark.parametrize('D,N,L', P.MJ_CASES)
def test_step_size_is_the_smallest_of_the_grid(D, N, L, state):
    """`choose_eps` again: no smaller step size of the grid meets the rule"""
    eps, run = P.choose_eps(state, D, N, L)
    assert eps == P.EPS[(state, D, N, L)] and run['counts'] == P.SHARES[(state, D, N, L)], (state, D, N, L, eps)


def test_wider_follows_the_rule():
    """WIDER holds exactly the cases where MARGIN x the recorded spread exceeds a bar, at max(bar, MARGIN x spread)"""
    want = {}
    for key, spread in P.SPREAD.items():
        state = key[1] if key[0] in ('control', 'ct') else key[0]
        allowed = P.allowance(state, spread)
        if allowed != P.BARS[state]:
            want[key] = allowed
    assert set(P.WIDER) == set(want)
    for key, (allowed, spread) in P.WIDER.items():
        assert spread == P.SPREAD[key] and np.allclose(allowed, want[key], rtol=1e-12, atol=0), (key, allowed, want[key])
        state = key[1] if key[0] == 'control' else key[0]
        assert all(a >= b for a, b in zip(allowed, P.BARS[state]))
    assert all(k[0] == 'float64' or k[1] == 'float64' for k in P.WIDER)       # float32 state: the bars hold everywhere


def test_fused_wider_follows_its_rule():
    """the fused call's allowance: max(the case's, MARGIN x the recorded fused path spread); FUSED_WIDER holds exactly the
    cases where that exceeds the case's own"""
    want = {}
    for key, spread in P.FUSED_PATH_SPREAD.items():
        tol = P.tolerances(key, key[0])
        own = (tol['x_tol'], tol['e_rtol'])
        allowed = tuple(max(a, P.MARGIN * sp) for a, sp in zip(own, spread))
        if allowed != own:
            want[key] = allowed
        else:
            assert P.fused_tolerances(key, key[0]) == own
    assert set(P.FUSED_WIDER) == set(want)
    for key, (allowed, spread) in P.FUSED_WIDER.items():
        assert spread == P.FUSED_PATH_SPREAD[key] and np.allclose(allowed, want[key], rtol=1e-12, atol=0), (key, allowed, want[key])
        assert P.fused_tolerances(key, key[0]) == allowed
