"""CPU: what the linear-model width cases (tests/test_gpu_linear_widths.py) rest on, recomputed with the oracle alone -- the
counterpart of tests/test_pot_widths_cpu.py.  For every case of the GPU module: the instance its table names (P, NB, the
masked experts, the padded rows) is what tests.helpers.pot_padded_dim gives for max(D, K); the oracle's own run at the
chosen step size makes the tallies of the table -- each of L, F and R at least 2 % of the particle-iterations, everything
finite -- and no smaller step size of the grid does; the float32 and the float64 NumPy force decide differently
(MarkovJumpHMC: the transition; ControlHMC: the accept; ContinuousTimeHMC: the first clock) on at most tie_ceiling(N)
particles of any compared iteration (measured: none); the float32 spread is the recorded one, and WIDER holds exactly the
allowances max(bar, 4 x spread) that exceed a bar.  The replay cases run on the recorded numbers the GPU case hands to both
sides.  Last, the evaluation bar tells two wrong kernels from the right one on the restated energy."""
import numpy as np
import pytest

from tests import test_gpu_linear_widths as Q
from tests.helpers import tie_ceiling
from tests.test_gpu_pot_widths import BARS, CONTROL_SEED, CT_SEED, EPS_GRID, MIN_SHARE, SEED, SEEDS, allowance, rel, shares_ok

# (D, K): (P, NB, masked experts, padded state rows)
INSTANCE = {(100, 9): (128, 1, 119, 28), (200, 130): (256, 2, 126, 56), (129, 256): (256, 2, 0, 127), (40, 257): (512, 4, 255, 472),
            (300, 200): (512, 4, 312, 212), (512, 400): (512, 4, 112, 0), (511, 512): (512, 4, 0, 1)}


def test_the_shapes_reach_the_instances_of_the_table():
    assert set(Q.SHAPES) == set(INSTANCE)
    for (D, K), (P, NB, masked, rows) in INSTANCE.items():
        assert Q.padded(D, K) == (P, NB) and (P - K, P - D) == (masked, rows) and P == 128 * NB
    assert (100 + 7) // 8 == 13                           # PotModel::ndims = max(D, K) keeps 13 of 16 k-row groups at (100, 9)
    assert sorted({Q.padded(D, K)[1] for D, K in Q.SHAPES}) == [1, 2, 4]
    assert all(K < Q.padded(D, K)[0] and Q.padded(D, K)[1] == 4 for D, K in Q.SMALL_BATCH)
    for sub in (Q.TWO, Q.CONTROL, Q.TWINS, (Q.REPLAY,)):
        assert set(sub) <= set(Q.SHAPES)
    assert (SEEDS['MarkovJumpHMC'], SEEDS['ControlHMC'], SEEDS['ContinuousTimeHMC']) == (SEED, CONTROL_SEED, CT_SEED) == (17, 20, 43)
    cases = set(Q.MJ_CASES)
    assert cases == set(Q.TABLE) and len(Q.MJ_CASES) == len(cases)
    assert all((D, K, 70, 5) in cases for D, K in Q.SHAPES)
    assert all((D, K, 70, L) in cases and (D, K, 33, 5) in cases for D, K in ((200, 130), (512, 400)) for L in (1, 2))
    assert set(Q.OTHER) == ({('control', s, D, K) for s in Q.STATES for D, K in ((200, 130), (40, 257), (512, 400), (511, 512))} |
                            {('ct', s, D, K) for s in Q.STATES for D, K in ((200, 130), (512, 400))} |
                            {('replay', s, 512, 400) for s in Q.STATES} | {('replay-control', 'float64', 512, 400)})
    assert all(eps in EPS_GRID for eps in Q.EPS.values())
    # the bit-for-bit cases: every pair of (L, mode), (N, L) and (N, mode) occurs
    for i, j in ((0, 1), (0, 2), (1, 2)):
        pairs = {(c[i], c[j]) for c in Q._TWIN_CASES}
        assert pairs == {(a, b) for a in {c[i] for c in Q._TWIN_CASES} for b in {c[j] for c in Q._TWIN_CASES}}
    assert {c[0] for c in Q._TWIN_CASES} == {32, 33} and {c[1] for c in Q._TWIN_CASES} == {1, 2, 5}


def test_the_model_is_the_stated_one():
    D, K = 200, 130
    rs = np.random.RandomState(7 * D + K)
    W, b, q = rs.randn(K, D) / np.sqrt(D), 0.1 * rs.randn(K), 0.5 + rs.rand(1, K)
    Wm, bm, qm = Q._model(D, K)
    for got, want in ((Wm, W), (bm, b), (qm, q)):
        assert got.dtype == np.float64 and np.array_equal(got, want.astype(np.float32).astype(np.float64))
    assert qm.min() >= Q.Q_MIN and np.array_equal(Q._x0(D, 70), np.random.RandomState(1000 * D + 70).randn(D, 70))
    # the restated force: the gradient of the restated energy (float64 arithmetic, central differences)
    E, G = Q.restated(Wm, bm, qm, dtype=np.float64)
    X = Q._x0(D, 3)
    h, d = 1e-6, np.random.RandomState(0).randn(D, 3)
    assert np.allclose((E(X + h * d) - E(X - h * d))[0] / (2 * h), (G(X) * d).sum(axis=0), rtol=1e-7)
    E32, G32 = Q.restated(Wm, bm, qm)
    assert rel(E32(X), E(X)) < 1e-6 and rel(G32(X), G(X)) < 1e-5


def _same_spread(got, recorded):
    """the recorded figure is the measured one to its two digits"""
    return np.allclose(got, recorded, rtol=0.05, atol=0)


@pytest.mark.parametrize('state', Q.STATES)
@pytest.mark.parametrize('D,K,N,L', Q.MJ_CASES)
def test_markov_jump_case_on_the_oracle_alone(D, K, N, L, state):
    """`choose_eps` again: the table's step size is the smallest of the grid that meets the rule, and its run is the table's"""
    key = (state, D, K, N, L)
    eps, run = Q.choose_eps(state, D, K, N, L)
    assert eps == Q.EPS[key], (key, 'the step size of the rule', eps)
    assert run['finite'] and run['n_iter'] == Q.N_ITER, key
    assert run['counts'] == Q.SHARES[key], (key, 'the table no longer holds the shares of the oracle run', run['counts'])
    assert shares_ok(D, N, run['counts'], run['n_iter']) and min(run['counts']) >= MIN_SHARE * N * run['n_iter'], (key, run['counts'])
    assert len(run['ties']) == run['n_iter'] and max(run['ties']) <= tie_ceiling(N), (key, 'near ties of the inputs', run['ties'])
    assert _same_spread(run['spread'], Q.SPREAD[key]), (key, 'spread', run['spread'], Q.SPREAD[key])


@pytest.mark.parametrize('key', sorted(Q.OTHER))
def test_other_sampler_case_on_the_oracle_alone(key):
    kind, state, D, K = key
    cls_name, n, replay = {'control': ('ControlHMC', Q.N_ITER, False), 'ct': ('ContinuousTimeHMC', Q.N_CT, False),
                           'replay': ('MarkovJumpHMC', Q.N_REPLAY, True), 'replay-control': ('ControlHMC', Q.N_REPLAY, True)}[kind]
    N = 70
    assert Q.EPS[key] == Q.EPS[(state, D, K, 70, 5)]
    run = Q.oracle_run(state, D, K, N, 5, Q.EPS[key], cls_name, n, replay)
    assert run['finite']
    assert len(run['ties']) == n and max(run['ties']) <= tie_ceiling(N), (key, 'near ties of the inputs', run['ties'])
    counts = run['counts'] if kind == 'replay' else run['counts'] + (run['fl'],)
    assert counts == Q.SHARES[key], (key, counts)
    if kind in ('control', 'replay-control'):         # a refresh, and neither every proposal accepted nor none
        assert run['refreshed'] and 0 < run['counts'][0] + run['fl'] < n * N
    elif kind == 'ct':
        assert min(run['fl'], run['counts'][1], run['counts'][2]) > 0
    else:
        assert min(run['counts']) > 0
    assert _same_spread(run['spread'], Q.SPREAD[key]), (key, 'spread', run['spread'], Q.SPREAD[key])


def test_wider_follows_the_rule():
    """WIDER holds exactly the cases where MARGIN x the recorded spread exceeds a bar, at max(bar, MARGIN x spread)"""
    want = {}
    for key, spread in Q.SPREAD.items():
        allowed = allowance(Q.state_of(key), spread)
        if allowed != BARS[Q.state_of(key)]:
            want[key] = allowed
    assert set(Q.WIDER) == set(want)
    for key, (allowed, spread) in Q.WIDER.items():
        assert spread == Q.SPREAD[key] and np.allclose(allowed, want[key], rtol=1e-12, atol=0), (key, allowed, want[key])
        assert all(a >= b for a, b in zip(allowed, BARS[Q.state_of(key)]))
        assert tuple(Q.tolerances(key).values()) == allowed
    assert all(Q.state_of(k) == 'float64' for k in Q.WIDER)       # float32 state: the bars hold everywhere
    assert all(tuple(Q.tolerances(k).values()) == BARS[Q.state_of(k)] for k in Q.SPREAD if k not in Q.WIDER)


@pytest.mark.parametrize('D,K', [s for s in Q.SHAPES if s[1] < Q.padded(*s)[0]])
def test_the_evaluation_bar_discriminates(D, K):
    """tests/test_gpu_linear_grouped.py::assert_the_bars_discriminate's pattern, for every shape with K < P: ONE padded
    expert counted with the smallest q a live expert carries (Q_MIN log 2), and q read at the expert's index within its
    wave's 32 NB experts instead of the global j, each move the restated energy by at least 10 evaluation bars.  (As the
    model is stored -- csrc/linear_energy.hip: rows of P floats, zero beyond K -- an expression of q[0] alone never meets the
    row stride, and a padded expert's q is 0, so that the scaled softplus of a padded expert is exactly 0 in E and in phi
    with or without the mask: the mask itself is what the L1 pair of the bit-for-bit cases holds, through 0/0.)"""
    W, b, q = Q._model(D, K)
    X = Q._x0(D, 70)
    E = Q.restated(W, b, q)[0](X)
    moved = rel(Q.restated(W, b, q, padded_experts=1)[0](X), E)
    assert moved >= 10 * Q.EVAL_BARS[0], (D, K, 'one padded expert', moved)
    if K > 32 * Q.padded(D, K)[1]:                  # (100, 9): every expert lies in the first wave's rows
        moved = rel(Q.restated(W, b, q, wrong_q=True)[0](X), E)
        assert moved >= 10 * Q.EVAL_BARS[0], (D, K, 'q at the local index', moved)
    else:
        assert np.array_equal(Q.restated(W, b, q, wrong_q=True)[0](X), E)
