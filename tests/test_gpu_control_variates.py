"""GPU: the device control variates (csrc/crossmoments.hip, HMCBase.cv_expectations).

The arithmetic model of every comparison with the definition is that of tests/test_gpu_estimators.py: a device sum is a
float64 sum of M = n * N terms, each term carrying at most four roundings, so per entry
    |device - host| <= (M + 4) * 2^-53 * sum |term|
with the host side computed in numpy.longdouble from the downloaded ring (ring_read / ring_read_dwell), the gradient of
every downloaded slot from DeviceEnergy.eval in the state's own type (mjhmc_eval runs the evaluation the handle runs: the
same values bit for bit, or the bound could not hold -- an element of a float32 gradient that differed in its last bit
would miss it by nine orders of magnitude)."""
import numpy as np
import pytest

from tests.test_gpu_estimators import _iso, _pot32, _sic_bf16, recorded_block

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
LD = np.longdouble
NAMES = ('W', 'Sg', 'S2g', 'Sb', 'S2b', 'Cgg', 'Cgb')


# ---------------------------------------------------------------------------------------------------------------------
# host side of the definition
# ---------------------------------------------------------------------------------------------------------------------
def host_sums(G, B, w, cb):
    """G (D, n, N) gradients, B (K, n, N) values, w (n, N) weights, cb (K,) shift -> (the seven sums, the |.| sums of the
    same terms), in numpy.longdouble"""
    D, K = G.shape[0], B.shape[0]
    g = G.astype(LD).reshape(D, -1)
    b = (B.astype(LD) - cb.astype(LD)[:, None, None]).reshape(K, -1)
    wl = w.astype(LD).reshape(-1)
    wg, wb = g * wl, b * wl
    sums = (wl.sum(), wg.sum(axis=1), (wg * g).sum(axis=1), wb.sum(axis=1), (wb * b).sum(axis=1), wg @ g.T, wg @ b.T)
    absum = (np.abs(wl).sum(), np.abs(wg).sum(axis=1), np.abs(wg * g).sum(axis=1), np.abs(wb).sum(axis=1),
             np.abs(wb * b).sum(axis=1), np.abs(wg) @ np.abs(g).T, np.abs(wg) @ np.abs(b).T)
    return sums, absum


def assert_within_bound(dev, host, absum, M, tag):
    for name, d, h, a in zip(NAMES, dev, host, absum):
        err = np.abs(np.asarray(d).astype(LD) - h)
        bound = (M + 4) * LD(U) * a
        worst = float(np.max(err / np.where(bound > 0, bound, 1)))
        print('%s %s: max |device - host| / bound = %.3g' % (tag, name, worst))
        assert np.all(err <= bound), (tag, name, worst)


def gradients(s, X, dtype):
    """dE/dX of the downloaded slots X (D, n, N) through the energy's own evaluation, in the state's type"""
    return np.stack([s._dev.energy.eval(np.ascontiguousarray(X[:, j, :]), want_E=False, dtype=dtype)[1]
                     for j in range(X.shape[1])], axis=1)


def _projections(D):
    from mjhmc_amd.samplers.markov_jump_hmc import Projections
    rs = np.random.RandomState(12)
    return Projections(rs.randn(5, D), b=rs.randn(5))


def _energy_observables(D):
    from mjhmc_amd.samplers.markov_jump_hmc import EnergyObservables
    return EnergyObservables()


# case -> (sampler, n, state type, of)
CASES = {
    'iso33x100': (lambda: _iso(33, 100, 1), 6, 'float64', None),      # pitch 34, Npad > N; third tile partial, fourth absent
    'iso130x70': (lambda: _iso(130, 70, 2), 3, 'float64', None),      # 3 x 3 blocks, the last of two columns; 17 groups + 2 lanes
    'iso5x3': (lambda: _iso(5, 3, 3), 4, 'float64', None),            # less than one group of four particles
    'pot36_f32': (_pot32, 5, 'float32', None),                        # float32 state and float32 gradient
    'sic512_bf16': (_sic_bf16, 4, 'bfloat16', None),                  # bfloat16 state, float32 gradient, 8 x 8 blocks, N = 40
    'iso33x100_projections': (lambda: _iso(33, 100, 1), 6, 'float64', _projections),   # 33 x 5: float64 derived ring, pitch 6
    'pot36_f32_energy_observables': (_pot32, 5, 'float32', _energy_observables),       # K = 3, pitch 4
}


@pytest.mark.parametrize('case', sorted(CASES))
def test_definition(case):
    """all seven sums against the definition in extended precision: unit and dwell weights, zero and non-zero shift"""
    make, n, dtype, make_of = CASES[case]
    s = make()
    X, dwell = recorded_block(s, n)
    D, N = s._dev.ndims, s._dev.nparticles
    assert np.all(np.isfinite(dwell)) and np.all(dwell[1:] > 0)
    M = n * N
    G = gradients(s, X[:, :n, :], dtype)
    assert G.shape == (D, n, N) and np.all(np.isfinite(G))
    fn = None
    if make_of is None:
        cm, B = s._dev.cross_moments(), X[:, :n, :]
    else:
        fn = s._open_functionals(make_of(D), n)
        fn.evaluate(0, n, 0)
        cm, B = fn.cross_moments(), fn.read(0, n)
    K = B.shape[0]
    assert (cm.ndims, cm.n_values) == (D, K)
    shifts = (np.zeros(K), B[:, 0, :].mean(axis=1) + 0.37 * np.cos(np.arange(K)))
    for wname, w_slot0, w in (('unit', -1, np.ones((n, N))), ('dwell', 1, dwell[1:n + 1])):
        for ci, cb in enumerate(shifts):
            cm.reset()
            cm.set_shift(cb)
            cm.accumulate(0, n, w_slot0=w_slot0)
            dev = cm.read()
            assert dev[7] == M
            host, absum = host_sums(G, B, w, cb)
            assert_within_bound(dev[:7], host, absum, M, '%s %s shift%d' % (case, wname, ci))
            assert np.array_equal(dev[5], dev[5].T), 'Cgg is not symmetric bit for bit'
    cm.close()
    if fn is not None:
        fn.close()


def _sums_equal(a, b):
    return all(np.array_equal(np.asarray(getattr(a, k)), np.asarray(getattr(b, k))) for k in NAMES) and a.n_states == b.n_states


def test_block_independence():
    """every slot is added to the running totals separately: the sums do not depend on the blocks, bit for bit"""
    c = np.linspace(-0.5, 1.0, 33)
    res = [_iso(33, 100, 1).cv_expectations(7, block=b, shift=c) for b in (1, 3, 7)]
    assert res[0].n_states == 7 * 100
    assert _sums_equal(res[0], res[1]) and _sums_equal(res[0], res[2])
    assert np.array_equal(res[0].mean, res[2].mean) and np.array_equal(res[0].coef, res[1].coef)


def test_determinism():
    """two fresh samplers, same seed, same calls: bit-identical sums"""
    a, b = (_iso(130, 70, 2).cv_expectations(5, block=2) for _ in range(2))
    assert _sums_equal(a, b) and np.array_equal(a.shift, b.shift) and np.array_equal(a.mean, b.mean)


def test_the_run_is_that_of_expectations():
    """cv_expectations(n) leaves the sampler as expectations(n) does, and its plain moments are expectations()'s own.  The
    moment pass adds a call's sum to its running totals, so the comparison of the moments takes expectations(block=1),
    which accumulates slot by slot as the control variates do; the run itself does not depend on the blocks."""
    n, c = 9, np.full(24, 0.25)
    a, b = _iso(24, 301, 5), _iso(24, 301, 5)
    tick0 = a._dev.get_tick()
    cv = a.cv_expectations(n, block=4, shift=c)
    ex = b.expectations(n, block=1, shift=c)
    assert a._dev.get_tick() - tick0 == n + 1 and a._dev.get_tick() == b._dev.get_tick()
    assert np.array_equal(a.state.X, b.state.X) and np.array_equal(a.state.V, b.state.V)
    assert (a.l_count, a.f_count, a.r_count, a.fl_count) == (b.l_count, b.f_count, b.r_count, b.fl_count)
    assert (a.distribution.E_count, a.distribution.dEdX_count) == (b.distribution.E_count, b.distribution.dEdX_count)
    assert np.array_equal(a.dwelling_times, b.dwelling_times)
    assert cv.n_states == ex.n_states == n * 301 and cv.W == ex.W
    assert np.array_equal(cv.plain.mean, ex.mean) and np.array_equal(cv.plain.var, ex.var)
    # the default block walks the same run
    d = _iso(24, 301, 5)
    d.expectations(n, shift=c)
    assert np.array_equal(a.state.X, d.state.X) and np.array_equal(a.dwelling_times, d.dwelling_times)


# ---------------------------------------------------------------------------------------------------------------------
# exactness on Gaussians: x = mu + Sigma g at every state, equilibrated or not
# ---------------------------------------------------------------------------------------------------------------------
def numpy_restatement(G, B, w):
    """the control-variate means of B (K, n, N) with G (D, n, N), weights w (n, N), in NumPy float64: (mean, variance ratio)"""
    D, K = G.shape[0], B.shape[0]
    g, b = G.reshape(D, -1), B.reshape(K, -1)
    p = w.reshape(-1) / w.sum()
    gbar, bbar = g.dot(p), b.dot(p)
    gc, bc = g - gbar[:, None], b - bbar[:, None]
    cov_gg, cov_gb = (gc * p).dot(gc.T), (gc * p).dot(bc.T)
    coef = np.linalg.solve(cov_gg, cov_gb)
    var = (bc * bc).dot(p)
    return bbar - coef.T.dot(gbar), 1.0 - np.sum(cov_gb * coef, axis=0) / var


def _aniso(seed=6):
    from mjhmc_amd.misc.distributions import Gaussian
    from mjhmc_amd.samplers.markov_jump_hmc import MarkovJumpHMC
    np.random.seed(seed)
    return MarkovJumpHMC(distribution=Gaussian(ndims=16, nbatch=128, log_conditioning=3), epsilon=0.05, beta=0.3,
                         num_leapfrog_steps=5, seed=17, resample=False)


@pytest.mark.parametrize('case', ['iso33x100', 'aniso16x128'])
def test_exact_on_gaussians(case):
    """The bound 1e-9 is measured against the NumPy float64 restatement, which gives 2e-15 to 2e-14 at condition numbers up
    to 1e3 on inputs of this kind: five orders of magnitude over the reference and seven under the plain error."""
    make, n = ((lambda: _iso(33, 100, 1)), 6) if case == 'iso33x100' else (_aniso, 6)
    cv = make().cv_expectations(n)
    s = make()
    X, dwell = recorded_block(s, n)
    ref_mean, ref_ratio = numpy_restatement(gradients(s, X[:, :n, :], 'float64'), X[:, :n, :], dwell[1:n + 1])
    plain, got, ratio = np.max(np.abs(cv.plain.mean)), np.max(np.abs(cv.mean)), np.max(np.abs(cv.variance_ratio))
    print('%s: max |plain.mean| %.3g, max |mean| %.3g (NumPy restatement %.3g), max |variance_ratio| %.3g (NumPy %.3g), '
          'max |grad_mean| %.3g' % (case, plain, got, np.max(np.abs(ref_mean)), ratio, np.max(np.abs(ref_ratio)),
                                    np.max(np.abs(cv.grad_mean))))
    assert cv.rank == s.ndims and cv.n_states == n * s.nbatch
    assert plain >= 1e-2
    assert got <= 1e-9
    assert ratio <= 1e-9


def _correlated(seed=7):
    from mjhmc_amd.misc.distributions import CorrelatedGaussian
    from mjhmc_amd.samplers.markov_jump_hmc import MarkovJumpHMC
    D, N = 36, 120
    mu = 1.0 + 0.5 * np.sin(np.arange(D))
    np.random.seed(seed)
    d = CorrelatedGaussian(ndims=D, log_conditioning=2, nbatch=N, mean=mu, state_dtype='float32')
    return MarkovJumpHMC(distribution=d, epsilon=0.1, beta=0.3, num_leapfrog_steps=6, seed=23, resample=False), mu


def test_exact_through_a_float32_force():
    """CorrelatedGaussian, non-zero mean, the force of the matrix-core tile kernels in float32 (float32 state: the
    float64-state sampler of this energy runs the multi-pass path, which the handle refuses).  x = mu + Sigma g holds up to
    the rounding of g, so the yardstick is the NumPy float64 restatement on the downloaded states and gradients; 100 x
    covers solving through a different route on sums that differ only by rounding."""
    n = 6
    s, mu = _correlated()
    cv = s.cv_expectations(n)
    r, _ = _correlated()
    X, dwell = recorded_block(r, n)
    ref_mean, _ = numpy_restatement(gradients(r, X[:, :n, :], 'float32'), X[:, :n, :], dwell[1:n + 1])
    ref_err, err, plain_err = np.max(np.abs(ref_mean - mu)), np.max(np.abs(cv.mean - mu)), np.max(np.abs(cv.plain.mean - mu))
    print('float32 force: max |mean - mu| %.3g, NumPy restatement %.3g, plain %.3g, max |variance_ratio| %.3g'
          % (err, ref_err, plain_err, np.max(np.abs(cv.variance_ratio))))
    assert err <= 100 * ref_err
    assert err <= plain_err / 1000


def test_regression_invariants_on_a_non_gaussian_target():
    cv = _pot32().cv_expectations(5)
    print('pot36_f32: variance_ratio in [%.4g, %.4g], max |grad_mean| %.3g'
          % (cv.variance_ratio.min(), cv.variance_ratio.max(), np.max(np.abs(cv.grad_mean))))
    assert cv.rank == 36 and cv.coef.shape == (36, 36) and cv.n_states == 5 * 120
    assert np.all(cv.variance_ratio >= -1e-12) and np.all(cv.variance_ratio <= 1 + 1e-12)
    # the mean, recomputed from the read sums
    gbar, m = cv.Sg / cv.W, cv.Sb / cv.W
    assert np.array_equal(gbar, cv.grad_mean)
    coef = np.linalg.solve(cv.Cgg / cv.W - np.outer(gbar, gbar), cv.Cgb / cv.W - np.outer(gbar, m))
    assert np.allclose(cv.coef, coef, rtol=0, atol=1e-9 * np.max(np.abs(coef)))
    want = cv.plain.mean - cv.coef.T.dot(gbar)
    assert np.allclose(cv.mean, want, rtol=0, atol=8 * U * np.max(np.abs(cv.plain.mean)))


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def _hooks_sampler(D=12, N=70, slots=5):
    from mjhmc_amd import engine, _lib
    from tests.helpers import hooks_context
    ctx = hooks_context(0)
    en = engine.DeviceEnergy(ctx, _lib.E_ISO_GAUSS, D, [1.0])
    dev = engine.DeviceSampler(en, np.random.RandomState(0).randn(D, N), seed=5, mode=_lib.MODE_MJHMC)
    dev.set_hparams(0.2, 5, 0.18, 1.0, 0.5)
    dev.ring_alloc(slots)
    dev.iterate(slots, ring_slot0=0)
    return ctx, dev


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_a_non_finite_dwell_adds_nothing():
    from mjhmc_amd import engine, _lib
    ctx, dev = _hooks_sampler()
    cm = dev.cross_moments()
    cm.accumulate(0, 2, w_slot0=1)
    before = cm.read()
    engine.check(ctx.lib.mjhmc_test_ring_write_dwell(dev.handle, 4, 17, float('inf')), ctx.lib)   # the LAST slot of the call
    with pytest.raises(_lib.EngineError, match='is not finite .*nothing of this block was added'):
        cm.accumulate(2, 2, w_slot0=3)
    assert _same(before, cm.read())
    cm.accumulate(2, 2, w_slot0=-1)                                  # the flag does not stick: unit weights still work
    assert cm.read()[7] == 4 * 70


def test_a_non_finite_state_names_the_slot_and_the_handle_refuses_until_reset():
    from mjhmc_amd import engine, _lib
    ctx, dev = _hooks_sampler()
    X = dev.ring_read(2, 1).reshape(12, 70).copy()
    X[7, 33] = np.nan
    engine.check(ctx.lib.mjhmc_test_ring_write(dev.handle, 2, X.ctypes.data), ctx.lib)
    cm = dev.cross_moments()
    cm.accumulate(0, 2)
    with pytest.raises(_lib.EngineError, match='a state of slot 2 is not finite') as e:
        cm.accumulate(1, 3)
    assert '(status -5)' in str(e.value)
    with pytest.raises(_lib.EngineError, match='mjhmc_crossmoments_reset first'):
        cm.accumulate(0, 1)
    with pytest.raises(_lib.EngineError, match='mjhmc_crossmoments_reset first'):
        cm.set_shift(np.zeros(12))
    cm.reset()
    cm.accumulate(0, 2)
    sums = cm.read()
    assert sums[7] == 2 * 70 and all(np.all(np.isfinite(v)) for v in sums[:7])


def test_refused_arguments():
    from mjhmc_amd import _lib
    from mjhmc_amd.misc.distributions import LambdaDistribution
    from mjhmc_amd.samplers.markov_jump_hmc import MarkovJumpHMC
    s = _iso(33, 100, 1)
    dev = s._dev
    with pytest.raises(_lib.EngineError, match='no sample ring'):
        dev.cross_moments()
    dev.ring_alloc(4)
    s._run(4, ring_slot0=0)
    cm = dev.cross_moments()
    for args, msg in (((0, 5, -1), 'outside the ring'), ((3, 2, -1), 'outside the ring'), ((-1, 1, -1), 'outside the ring'),
                      ((0, 4, 1), 'dwell slots'), ((0, 1, -2), 'dwell slots'), ((0, 0, -1), 'n must be >= 1')):
        with pytest.raises(_lib.EngineError, match=msg):
            cm.accumulate(args[0], args[1], w_slot0=args[2])
    assert cm.read()[7] == 0
    cm.accumulate(0, 3, w_slot0=1)
    with pytest.raises(_lib.EngineError, match='reset first'):
        cm.set_shift(np.ones(33))
    with pytest.raises(ValueError):
        cm.set_shift(np.ones(5))
    dev.ring_alloc(9)                                               # a new ring: the handle was sized for the old one
    with pytest.raises(_lib.EngineError, match='re-allocated'):
        cm.accumulate(0, 1)
    # a float64-state linear model runs the multi-pass path; opaque callables have no device evaluation at all
    from mjhmc_amd.misc.distributions import CorrelatedGaussian
    np.random.seed(1)
    wide = MarkovJumpHMC(distribution=CorrelatedGaussian(ndims=6, nbatch=64), epsilon=0.2, beta=0.3, num_leapfrog_steps=4,
                         seed=8, resample=False)
    wide._dev.ring_alloc(2)
    with pytest.raises(_lib.EngineError, match=r'multi-pass.*\(status -3\)'):
        wide._dev.cross_moments()
    A = np.array([[2.0, 0.5], [0.5, 1.0]])
    host = MarkovJumpHMC(distribution=LambdaDistribution(energy_func=lambda X: 0.5 * np.sum(X * (A @ X), axis=0),
                                                         energy_grad_func=lambda X: A @ X, init=np.ones((2, 64))),
                         epsilon=0.2, beta=0.3, num_leapfrog_steps=4, seed=8, resample=False)
    host._dev.ring_alloc(2)
    with pytest.raises(_lib.EngineError, match=r'host-evaluated energy.*\(status -3\)'):
        host._dev.cross_moments()
