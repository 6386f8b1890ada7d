"""GPU: device functionals (csrc/functionals.hip, DeviceFunctionals, ``of=`` of expectations / diagnostics / marginals).

Two arithmetic models, both stated where they are used:
  * a stat whose sum does not depend on the order of its terms (a picked coordinate, a count, two terms) and every value
    are fixed sequences of IEEE float64 operations -- ``host_values`` restates them in NumPy (whose elementwise float64
    operations round once each and never fuse) and the comparison is ``==``;
  * an order-dependent sum (``x * x``) is compared with numpy.longdouble within the summation bound derived in the test."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from tests.test_gpu_chainstats import record, _iso, _pot32, _sic_bf16, _same
from tests.test_gpu_estimators import host_sums, assert_within_bound
from tests.test_gpu_marginals import _ring

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
LD = np.longdouble
P0 = 0.375


# ---------------------------------------------------------------------------------------------------------------------
# the NumPy restatement
# ---------------------------------------------------------------------------------------------------------------------
def order_free_set(D):
    """(stats, values) of section 1 for rows of D coordinates"""
    stats = ['d == %d ? x : 0.0' % (D - 1), 'x > 0.25 ? 1.0 : 0.0'] + (['d < 2 ? 4.0 * x : 0.0'] if D >= 2 else [])
    values = ['S[0]', 'S[1]', 'S[0] * S[1] - p[0]', 'S[0] / (S[1] + 1.0)', 'S[1] > 2.0 ? 1.0 : 0.0'] + (['S[2]'] if D >= 2 else [])
    return stats, values


def host_values(X):
    """X (D, n, N) float64 states as the ring holds them -> (K, n, N), one IEEE float64 operation per NumPy operation.
    S0: one non-zero term; S1: a count (integers, exact); S2: two non-zero terms (one rounded addition, commutative)."""
    D = X.shape[0]
    S0 = X[D - 1]
    S1 = (X > 0.25).sum(axis=0).astype(np.float64)
    out = [S0, S1, S0 * S1 - P0, S0 / (S1 + 1.0), np.where(S1 > 2.0, 1.0, 0.0)]
    if D >= 2:
        out.append(4.0 * X[0] + 4.0 * X[1])
    return np.stack(out)


def pick_set(picks):
    return ['d == %d ? x : 0.0' % d for d in picks], ['S[%d]' % k for k in range(len(picks))]


def evaluated(dev, stats, values, n, params=()):
    fn = dev.functionals(values, stats, params)
    fn.ring_alloc(n)
    fn.evaluate(0, n, 0)
    return fn


# ---------------------------------------------------------------------------------------------------------------------
# 1.  values, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', [1, 2, 3, 33, 130])
@pytest.mark.parametrize('N', [1, 65, 200])
def test_values_bit_for_bit_float64(D, N):
    """one 16-byte chunk per row (D = 1, 2), a padded row (3, 33: pitch 4, 34), more chunks than a wave has lanes (130: the
    wave-per-row path); N = 1, one past a wave of rows, several workgroups"""
    n = 3
    X = np.random.RandomState(100 * D + N).randn(D, n, N) * 1.5
    ctx, dev, stored = _ring(X)
    stats, values = order_free_set(D)
    fn = evaluated(dev, stats, values, n, [P0])
    assert fn.n_values == len(values) and fn.slot_bytes == (N + 63) // 64 * 64 * 6 * 8
    got, want = fn.read(0, n), host_values(stored)
    assert got.shape == want.shape == (len(values), n, N) and np.all(np.isfinite(got))
    bad = int(np.sum(got != want))
    assert bad == 0, 'D=%d N=%d: %d of %d values differ' % (D, N, bad, want.size)


@pytest.mark.parametrize('case', ['pot36_f32', 'sic512_bf16'])
def test_values_bit_for_bit_narrow_states(case):
    """float32 rows of a ProductOfT sampler (36 of a 128-element pitch) and bfloat16 rows of a SparseImageCode sampler (512
    elements, 8 per lane), as their samplers record them"""
    s = {'pot36_f32': _pot32, 'sic512_bf16': _sic_bf16}[case]()
    n = 4
    X, w, w_slot0 = record(s, n)
    D = s._dev.ndims
    stats, values = order_free_set(D)
    fn = evaluated(s._dev, stats, values, n, [P0])
    got, want = fn.read(0, n), host_values(X[:, :n, :])
    assert np.all(np.isfinite(got))
    bad = int(np.sum(got != want))
    assert bad == 0, '%s: %d of %d values differ' % (case, bad, want.size)
    assert np.any(want[1] > 2.0) and np.any(want[0] != 0)


def test_without_stats_a_value_is_a_constant():
    ctx, dev, stored = _ring(np.random.RandomState(0).randn(5, 2, 70))
    fn = evaluated(dev, [], ['1.5', 'p[1] * 2.0 + p[0]', '3.0 > 2.0 ? -1.0 : 1.0'], 2, [0.25, 8.0])
    got = fn.read(0, 2)
    assert got.shape == (3, 2, 70)
    assert np.all(got[0] == 1.5) and np.all(got[1] == 16.25) and np.all(got[2] == -1.0)


# ---------------------------------------------------------------------------------------------------------------------
# 2.  order-dependent sums within their bound
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['f64_33', 'f64_130', 'f64_2', 'pot36_f32', 'sic512_bf16'])
def test_sum_of_squares_within_the_summation_bound(case):
    """stat x * x, value S[0]: one rounding per product (relative 2^-53 of the product) and at most D - 1 additions on the
    way to the sum, whatever their order (each relative 2^-53 of a partial sum <= the whole sum of non-negative terms):
    |device - exact| <= (D + 2) 2^-53 sum x^2, first order plus slack for the second.  Derived, not tuned.  Two
    evaluations of the same slots are equal bit for bit."""
    n = 3
    if case.startswith('f64'):
        D = int(case.split('_')[1])
        ctx, dev, X = _ring(np.random.RandomState(D).randn(D, n, 65) * 2.0 + 0.3)
    else:
        s = {'pot36_f32': _pot32, 'sic512_bf16': _sic_bf16}[case]()
        X = record(s, n)[0][:, :n, :]
        dev, D = s._dev, s._dev.ndims
    fn = dev.functionals(['S[0]'], ['x * x'])
    fn.ring_alloc(2 * n)
    fn.evaluate(0, n, 0)
    fn.evaluate(0, n, n)
    got, again = fn.read(0, n)[0], fn.read(n, n)[0]
    assert np.array_equal(got, again)
    exact = (X.astype(LD) ** 2).sum(axis=0)
    err = np.abs(got.astype(LD) - exact)
    bound = (D + 2) * LD(U) * exact
    print('%s: D = %d, max |device - longdouble| / bound = %.3g' % (case, D, float(np.max(err / bound))))
    assert np.all(np.isfinite(got)) and np.all(err <= bound)


# ---------------------------------------------------------------------------------------------------------------------
# 3.  downstream equals upstream
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D,picks', [(33, [32, 0, 7, 16, 3]), (6, [5, 0, 3, 1, 4, 2])])
def test_accumulators_on_the_derived_ring_equal_those_on_the_sample_ring(D, picks):
    """functionals that pick coordinates: the derived ring holds those coordinates, so per-chain sums and histogram tables
    on it equal the picked rows of the sample ring's bit for bit (same operations per element, integer tables), for unit
    and for dwell weights; moment and covariance sums (K = D at D = 6) meet the bound of tests/test_gpu_estimators.py."""
    n, N = 6, 301
    s = _iso(D, N, 3)
    X, w, w_slot0 = record(s, n)
    dev, K = s._dev, len(picks)
    fn = evaluated(dev, *pick_set(picks), n=n)
    assert np.array_equal(fn.read(0, n), X[picks][:, :n, :])
    shift = np.linspace(-0.4, 0.6, D)
    lo, hi, q = np.full(D, -4.0) - 0.01 * np.arange(D), np.full(D, 4.5) + 0.02 * np.arange(D), 2.0 ** -22
    up_cs, dn_cs = dev.chain_stats(1), fn.chain_stats(1)
    up_h, dn_h = dev.histogram(64, lo, hi, q), fn.histogram(64, lo[picks], hi[picks], q)
    assert dn_cs.ndims == K and dn_h.ndims == K
    up_cs.set_shift(shift)
    dn_cs.set_shift(shift[picks])
    for slot0 in (-1, w_slot0):
        for h in (up_cs, dn_cs, up_h, dn_h):
            h.reset()
            h.accumulate(0, n, w_slot0=slot0)
        a0u, a1u, a2u = up_cs.read_chains()
        a0d, a1d, a2d = dn_cs.read_chains()
        assert np.array_equal(a0u, a0d) and np.array_equal(a1u[picks], a1d) and np.array_equal(a2u[picks], a2d), slot0
        cu, mu, Wu, nu = up_h.read()
        cd, md, Wd, nd = dn_h.read()
        assert np.array_equal(cu[picks], cd) and np.array_equal(mu[picks], md) and (Wu, nu) == (Wd, nd), slot0
        assert cd.sum() == K * n * N
    if K == D:
        est = fn.estimator(True)
        est.set_shift(shift[picks])
        est.accumulate(0, n, w_slot0=w_slot0)
        W, S1, S2, C, n_states = est.read()
        host, absum = host_sums(X[picks][:, :n, :], w, shift[picks], True)
        assert n_states == n * N
        assert_within_bound((W, S1, S2, C), host, absum, n_states, 'derived ring D=K=%d' % D)


# ---------------------------------------------------------------------------------------------------------------------
# 4.  block independence and padding
# ---------------------------------------------------------------------------------------------------------------------
def test_block_independence_and_padding_rows():
    """a run of 12 slots evaluated as one block or as 5 + 5 + 2 (each block into derived slots 0 .., as the driver does):
    the same values, per-chain sums and histogram tables, bit for bit -- and again with every padding row of the sample
    ring (and of the dwell ring) filled with NaN bytes"""
    from mjhmc_amd import engine
    D, n, N = 33, 12, 65
    rs = np.random.RandomState(9)
    w = rs.standard_exponential((n, N)) + 0.01
    ctx, dev, X = _ring(rs.randn(D, n, N) * 1.2, 'float64', w)
    stats, values = ['x * x', 'd == 4 ? x : 0.0', 'x > 0.0 ? 1.0 : 0.0'], ['S[0]', 'S[1] * S[2]', 'S[0] / (S[2] + 1.0)']
    fn = dev.functionals(values, stats)
    fn.ring_alloc(n)
    lo, hi = np.array([0.0, -30.0, 0.0]), np.array([120.0, 30.0, 40.0])
    cs, hist = fn.chain_stats(1), fn.histogram(32, lo, hi, 2.0 ** -20)
    cs.set_shift(np.array([40.0, 0.5, 2.0]))

    def walk(cuts):
        cs.reset()
        hist.reset()
        vals, at = [], 0
        for k in cuts:
            fn.evaluate(at, k, 0)
            vals.append(fn.read(0, k))
            cs.accumulate(0, k, w_slot0=at)
            hist.accumulate(0, k, w_slot0=at)
            at += k
        return np.concatenate(vals, axis=1), cs.read_chains(), hist.read()

    one = walk([n])
    cut = walk([5, 5, 2])
    assert np.all(np.isfinite(one[0])) and one[0].shape == (3, n, N)
    assert np.array_equal(one[0], cut[0]) and _same(one[1], cut[1]) and _same(one[2][:2], cut[2][:2]) and one[2][2:] == cut[2][2:]
    for k in range(n):
        engine.check(ctx.lib.mjhmc_test_ring_fill_padding(dev.handle, k, 0xFF), ctx.lib)
    nan = walk([5, 5, 2])
    assert np.array_equal(one[0], nan[0]) and _same(one[1], nan[1]) and _same(one[2][:2], nan[2][:2]) and one[2][2:] == nan[2][2:]
    assert np.array_equal(dev.ring_read(0, n).reshape(D, n, N), X)


# ---------------------------------------------------------------------------------------------------------------------
# 5.  refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from mjhmc_amd import _lib
    from mjhmc_amd._lib import EngineError
    s = _iso(33, 100, 1)
    dev = s._dev
    with pytest.raises(EngineError, match='no sample ring'):
        dev.functionals(['S[0]'], ['x'])
    dev.ring_alloc(4)
    s._run(4, ring_slot0=0)
    with pytest.raises(EngineError, match="undeclared identifier 'y'"):
        dev.functionals(['S[0]'], ['x * y'])
    with pytest.raises(EngineError, match='at most 8 stats'):
        dev.functionals(['S[0]'], ['x'] * 9)
    with pytest.raises(EngineError, match=r'K must be in \[1, 16\]'):
        dev.functionals(['1.0'] * 17)
    # a value that is not finite: the flag names it, and does not stick
    bad = dev.functionals(['S[0]', '1.0 / (S[0] - S[0])'], ['x'])
    with pytest.raises(EngineError, match='no derived ring'):
        bad.evaluate(0, 1, 0)
    with pytest.raises(EngineError, match='no derived ring'):
        bad.estimator()
    bad.ring_alloc(4)
    with pytest.raises(EngineError, match='value 1 of the functionals is not finite'):
        bad.evaluate(0, 2, 0)
    assert dev.lib.mjhmc_functionals_evaluate(bad.handle, 0, 2, 0) == _lib.ERR_NONFINITE
    first = dev.functionals(['1.0 / (S[0] - S[0])'], ['x'])
    first.ring_alloc(1)
    with pytest.raises(EngineError, match='value 0 of the functionals is not finite'):
        first.evaluate(0, 1, 0)
    first.close()
    fn = dev.functionals(['S[0]'], ['x'])
    fn.ring_alloc(3)
    fn.evaluate(1, 3, 0)
    for args, msg in (((0, 5, 0), 'outside the ring of 4'), ((2, 3, 0), 'outside the ring of 4'), ((-1, 1, 0), 'outside the ring'),
                      ((0, 4, 0), 'outside the derived ring of 3'), ((0, 2, 2), 'outside the derived ring of 3'),
                      ((0, 1, -1), 'outside the derived ring'), ((0, 0, 0), 'n must be >= 1')):
        with pytest.raises(EngineError, match=msg):
            fn.evaluate(*args)
    with pytest.raises(EngineError, match='slots out of range'):
        fn.read(2, 2)
    # handles on the derived ring: its slots bound x_slot0, the sampler's dwell ring bounds w_slot0
    est, cs, hist = fn.estimator(True), fn.chain_stats(2), fn.histogram(8, -5.0, 5.0, 2.0 ** -20)
    with pytest.raises(EngineError, match='outside the ring of 3'):
        est.accumulate(0, 4)
    with pytest.raises(EngineError, match='dwell slots'):
        cs.accumulate(0, 3, w_slot0=2)
    est.accumulate(0, 3, w_slot0=1)
    cs.accumulate(0, 3, w_slot0=1, part=1)
    hist.accumulate(0, 3, w_slot0=1)
    assert est.read()[4] == 300 and cs.read(1)[:2] == (100, 3) and hist.read()[3] == 300
    with pytest.raises(ValueError):
        est.set_shift(np.zeros(33))                                  # K = 1 entries, not ndims
    fn.ring_alloc(3)                                                  # no growth: the same ring
    est.accumulate(0, 1, w_slot0=-1)
    fn.ring_alloc(6)                                                  # a new derived ring: the handles were created on the old one
    for call in (lambda: est.accumulate(0, 1), lambda: cs.accumulate(0, 1), lambda: hist.accumulate(0, 1)):
        with pytest.raises(EngineError, match='derived ring was re-allocated'):
            call()
    fresh = fn.estimator()
    fn.evaluate(0, 4, 0)
    fresh.accumulate(0, 4, w_slot0=-1)
    dev.ring_alloc(9)                                                 # a new sample ring: the functionals were created on the old one
    with pytest.raises(EngineError, match='sample ring was re-allocated after mjhmc_functionals_create'):
        fn.evaluate(0, 1, 0)
    alive = fn.chain_stats(1)
    fn.close()                                                        # frees the handles created on it ...
    for h in (est, cs, hist, fresh, alive):
        h.close()                                                     # ... whose wrappers then have nothing left to free
    bad.estimator()
    dev.close()                                                       # the sampler frees what is still alive on it
    bad.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6.  the driver
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cls', ['MarkovJumpHMC', 'ControlHMC', 'HMC'])
def test_driver_runs_the_same_run_and_reports_the_picked_coordinates(cls):
    """expectations / diagnostics / marginals with ``of=F`` against a twin sampler (same seed) without: the same
    iterations, counters, dwelling times, final state and tick.  F picks 5 of 7 coordinates: K and D share the fold tree of
    the chain statistics (its width is the next power of two of the dimension count: 8 for both), so Sm, Sq and Sv are equal
    bit for bit under the same shift and block; the histogram tables are integers and equal under the same range."""
    D, N, n_iter, picks = 7, 301, 20, [6, 0, 3, 5, 2]
    s, t = _iso(D, N, 5, cls), _iso(D, N, 5, cls)
    F = s.functionals(*reversed(pick_set(picks)), names=['x%d' % d for d in picks])
    assert F.n_values == 5 and F.names[0] == 'x6'
    lead = 1 if s._dwell_weighted else 0

    def same_run():
        assert (s.l_count, s.f_count, s.r_count, s.fl_count) == (t.l_count, t.f_count, t.r_count, t.fl_count)
        assert (s.distribution.E_count, s.distribution.dEdX_count) == (t.distribution.E_count, t.distribution.dEdX_count)
        assert np.array_equal(s.state.X, t.state.X) and np.array_equal(s.state.V, t.state.V)
        assert s._dev.get_tick() == t._dev.get_tick()
        if lead:
            assert np.array_equal(s.dwelling_times, t.dwelling_times)

    tick0 = s._dev.get_tick()
    with pytest.raises(ValueError):
        s.expectations(n_iter, of=F, shift=np.zeros(D))
    assert (s._dev.get_tick(), s._dev.ring_slots) == (tick0, 0)
    shift = np.linspace(-0.3, 0.4, D)
    ef = s.expectations(n_iter, cov=True, block=7, shift=shift[picks], of=F)
    et = t.expectations(n_iter, cov=True, block=7, shift=shift)
    same_run()
    assert s._dev.get_tick() - tick0 == n_iter + lead
    assert ef.n_states == et.n_states == n_iter * N and ef.mean.shape == (5,) and ef.cov.shape == (5, 5)
    # both are sums of the same n_states terms in different orders: twice the bound of the definition test, with the
    # |terms| bounded from the moments themselves (sum |w (x - c)| <= sqrt(W S2) by Cauchy-Schwarz)
    tol = 2 * (ef.n_states + 4) * U * np.sqrt(et.W * et.S2[picks])
    assert np.all(np.abs(ef.S1 - et.S1[picks]) <= tol) and np.all(np.abs(ef.S2 - et.S2[picks]) <= 2 * (ef.n_states + 4) * U * et.S2[picks])
    auto = s.expectations(n_iter, block=8, of=F)                         # the first block's own mean as the shift
    t.expectations(n_iter, block=8)
    same_run()
    assert auto.shift.shape == (5,) and np.any(auto.shift != 0)

    df = s.diagnostics(n_iter, split=True, block=4, shift=shift[picks], of=F)
    dt = t.diagnostics(n_iter, split=True, block=4, shift=shift)
    same_run()
    assert (df.n_chains, df.n_states) == (dt.n_chains, dt.n_states) == (2 * N, n_iter // 2) and df.grad_evals == dt.grad_evals
    assert df.Sw == dt.Sw
    for name in ('Sm', 'Sq', 'Sv'):
        assert np.array_equal(getattr(df, name), getattr(dt, name)[picks]), name
    assert np.array_equal(df.rhat, dt.rhat[picks]) and np.array_equal(df.ess, dt.ess[picks])
    s.diagnostics(n_iter, split=False, of=F)                             # default block, pooled shift of the first block
    t.diagnostics(n_iter, split=False)
    same_run()

    lo, hi = np.full(D, -5.0) - 0.1 * np.arange(D), np.full(D, 5.5)
    mf = s.marginals(n_iter, bins=48, range=(lo[picks], hi[picks]), block=6, of=F)
    mt = t.marginals(n_iter, bins=48, range=(lo, hi), block=6)
    same_run()
    assert mf.ndims == 5 and mf.quantum == mt.quantum and (mf.W_units, mf.n_states) == (mt.W_units, mt.n_states)
    assert np.array_equal(mf.counts, mt.counts[picks]) and np.array_equal(mf.units, mt.units[picks])
    auto = s.marginals(n_iter, bins=32, of=F)                            # range and quantum from the first block's moments
    t.marginals(n_iter, bins=32)
    same_run()
    # (mean -/+ 8 standard deviations of the first block; Chebyshev would allow that block itself 1 / 64 outside)
    assert auto.lo.shape == (5,) and np.all(auto.lo < auto.hi) and np.all(auto.out_of_range <= 1.0 / 64)


# ---------------------------------------------------------------------------------------------------------------------
# 7.  a known answer
# ---------------------------------------------------------------------------------------------------------------------
def test_known_answer_radius_of_a_gaussian():
    """x ~ N(0, sigma^2 I_2): r2 = |x|^2 / sigma^2 is chi-square with 2 degrees of freedom, E[r2] = 2 and
    P(r2 > t) = exp(-t / 2), so P(r2 > 2 ln 2) = 1 / 2 exactly and 2 ln 2 is the median.  8192 chains, 200 states after
    burn-in; the pooled means lie within 6 standard errors se = sqrt(var / ess), ess from diagnostics(of=F) on the
    continuing run; the histogram median within one bin width plus 6 se(P) / density of 2 ln 2 (the error of the CDF at
    the median, carried to x by the slope of the CDF there)."""
    from mjhmc_amd.misc.distributions import TestGaussian
    from mjhmc_amd.samplers.markov_jump_hmc import MarkovJumpHMC
    np.random.seed(12)
    s = MarkovJumpHMC(distribution=TestGaussian(ndims=2, nbatch=8192, sigma=1.3), epsilon=0.3, beta=0.3, num_leapfrog_steps=5,
                      seed=2024, resample=False)
    s.burn_in()
    med = 1.3862943611198906
    F = s.functionals(['S[0] / (p[0] * p[0])', 'S[0] / (p[0] * p[0]) > 1.3862943611198906 ? 1.0 : 0.0'], stats=['x * x'],
                      params=[1.3], names=['r2', 'r2 > 2 ln 2'])
    ex = s.expectations(200, of=F)
    dg = s.diagnostics(200, of=F)
    truth = np.array([2.0, 0.5])
    se = np.sqrt(ex.var / dg.ess)
    z = (ex.mean - truth) / se
    print('known answer: mean %s, se %s, ess %s, rhat %s, z-scores %s' % (ex.mean, se, dg.ess, dg.rhat, z))
    assert np.all(np.isfinite(z)) and np.all(np.abs(z) <= 6.0), z
    assert np.all(dg.ess > 0) and np.all(np.isfinite(dg.rhat))
    m = s.marginals(200, of=F)
    got = m.median[0]
    j = int(np.clip((got - m.lo[0]) // m.width[0], 0, m.bins - 1))
    tol = m.width[0] + 6.0 * se[1] / m.density[0, j]
    print('known answer: median of r2 %.5f (2 ln 2 = %.5f), bin width %.4f, density %.4f, tolerance %.4f'
          % (got, med, m.width[0], m.density[0, j], tol))
    assert abs(got - med) <= tol
    assert abs(m.density[0, j] - 0.25) < 0.05                            # the chi-square density at its median is 1 / 4


# ---------------------------------------------------------------------------------------------------------------------
# 8.  column shards on one GPU (the way tests/test_gpu_marginals.py runs them)
# ---------------------------------------------------------------------------------------------------------------------
WORKER = r'''
import sys
import numpy as np
sys.path.insert(0, %(root)r)
import torch.distributed as dist
from mjhmc_amd.parallel import Comm
from mjhmc_amd.samplers.markov_jump_hmc import MarkovJumpHMC
from mjhmc_amd.misc.distributions import TestGaussian

dist.init_process_group('gloo', init_method='tcp://127.0.0.1:%(port)d', rank=int(sys.argv[1]), world_size=2)
comm = Comm()
D, N, n_iter, B, picks = 7, 301, 20, 64, [6, 0, 3, 5, 2]
K = len(picks)
X0 = np.random.RandomState(5).randn(D, N) + 0.4


def dist_of():
    class Fixed(TestGaussian):
        def init_X(self):
            self.Xinit = X0
    return Fixed(ndims=D, nbatch=N, sigma=1.3)


def make(comm):
    return MarkovJumpHMC(distribution=dist_of(), epsilon=0.3, beta=0.3, num_leapfrog_steps=5, seed=4242, comm=comm,
                         resample=False)


def functionals(s):
    return s.functionals(['S[%%d]' %% k for k in range(K)], stats=['d == %%d ? x : 0.0' %% d for d in picks])


# rank-dependent arguments: rank 0's range and shift must win, and the ranks must agree on the smallest block
for rng, block, agreed in ((None, 4 + 3 * comm.rank, 4), ((-5.0 - comm.rank, 6.0 + comm.rank), 9 - 4 * comm.rank, 5)):
    s = make(comm)
    t0 = s._dev.get_tick()
    m = s.marginals(n_iter, bins=B, range=rng, block=block, of=functionals(s))
    assert s._dev.get_tick() - t0 == n_iter + 1, 'a rank ran more than the 21 iterations (a replayed or retried block)'
    packed = np.concatenate([m.lo, m.hi, [m.quantum]])
    assert packed.size == 2 * K + 1
    both = comm.allreduce_f64(np.concatenate([packed, -packed]), 'max')
    assert np.array_equal(both[:packed.size], -both[packed.size:]), 'the shards used different ranges or quanta'
    assert m.n_states == n_iter * N and m.counts.shape == (K, B + 2)
    shift = None if rng is None else np.full(K, 0.1) * (comm.rank + 1)
    s2 = make(comm)
    ex = s2.expectations(n_iter, cov=True, block=block, shift=shift, of=functionals(s2))
    both = comm.allreduce_f64(np.concatenate([ex.shift, -ex.shift]), 'max')
    assert ex.shift.shape == (K,) and np.array_equal(both[:K], -both[K:]), 'the shards used different shifts'
    if comm.rank == 0:
        s1 = make(None)
        m1 = s1.marginals(n_iter, bins=B, range=(m.lo, m.hi), block=agreed, of=functionals(s1))
        assert m1.quantum == m.quantum
        assert np.array_equal(m.counts, m1.counts) and np.array_equal(m.units, m1.units), 'sharded tables differ from the unsharded ones'
        assert (m.W_units, m.n_states) == (m1.W_units, m1.n_states)
        assert (s.l_count, s.f_count, s.r_count) == (s1.l_count, s1.f_count, s1.r_count)
        assert np.array_equal(s.dwelling_times, s1.dwelling_times)
        # the unsharded run recorded in one ring, its sums on the host: the reduced sums meet the definition test's bound
        from tests.test_gpu_estimators import host_sums, assert_within_bound, recorded_block
        X, dwell = recorded_block(make(None), n_iter)
        host, absum = host_sums(X[picks][:, :n_iter, :], dwell[1:n_iter + 1], ex.shift, True)
        assert ex.n_states == n_iter * N
        assert_within_bound((ex.W, ex.S1, ex.S2, ex.C), host, absum, ex.n_states, 'sharded of=F')
    comm.barrier()
print('rank %%d ok' %% comm.rank)
'''


def test_sharded_functionals_equal_unsharded(tmp_path):
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    script = tmp_path / 'worker.py'
    script.write_text(WORKER % dict(root=ROOT, port=port))
    procs = [subprocess.Popen([sys.executable, str(script), str(r)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(2)]
    outs = []
    for p in procs:
        try:
            out, _ = p.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(out.decode())
    for r, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and 'rank %d ok' % r in out, out[-3000:]
