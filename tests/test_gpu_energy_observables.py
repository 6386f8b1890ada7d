"""GPU: the energy observables [E, grad_sq, virial] of recorded states (csrc/energy_observables.hpp,
mjhmc_functionals_create_energy, ``of=sampler.energy_observables()``, ``temperature()``).

The reference is ``distribution.E_val`` / ``dEdX_val`` (mjhmc_eval, checked against the oracle elsewhere) on the states
``ring_read`` returns, one call per slot so that every row sits where it sat in the ring slot:
  * E is the same kernel on the same rows: ``==``;
  * grad_sq and virial are order-dependent sums of D rounded products: compared with numpy.longdouble sums of the reference
    gradient within the summation bound derived in ``assert_sums_within_bound``."""
import numpy as np
import pytest

from tests.test_gpu_chainstats import record, _iso, _pot32, _sic_bf16, _same, host_chain_sums, assert_fold_within_bound
from tests.test_gpu_lagcov import _funnel
from tests.test_gpu_marginals import _ring, host_hist
from tests.test_gpu_joint_marginals import host_pairhist

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
LD = np.longdouble


# ---------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------
def host_values(dist, X):
    """X (D, n, N) float64 states as the ring holds them -> E (n, N) float64 as mjhmc_eval returns it, the longdouble sums
    grad_sq, virial (n, N) of the reference gradient and the sums of |terms| their bounds are made of"""
    D, n, N = X.shape
    E = np.empty((n, N))
    gs, vr, gs_abs, vr_abs = [np.empty((n, N), dtype=LD) for _ in range(4)]
    for k in range(n):
        Xk = np.ascontiguousarray(X[:, k, :])
        E[k] = np.asarray(dist.E_val(Xk)).reshape(-1)
        G = np.asarray(dist.dEdX_val(Xk), dtype=np.float64).astype(LD)
        xl = Xk.astype(LD)
        gs[k], vr[k] = (G * G).sum(axis=0), (xl * G).sum(axis=0)
        gs_abs[k], vr_abs[k] = (G * G).sum(axis=0), np.abs(xl * G).sum(axis=0)
    return E, gs, vr, gs_abs, vr_abs


def assert_sums_within_bound(got, want, D, tag):
    """got (3, n, N) from the device, want = host_values(...).  E: ``==``.  The two sums: every product x_d * G_d (G_d * G_d)
    of exactly widened operands is rounded once, a relative 2^-53 of the term; the D terms then pass through at most
    D - 1 float64 additions on the way to the sum, whatever their order (lane partials in ascending d, then the butterfly),
    each a relative 2^-53 of a partial sum whose magnitude is at most sum_d |term_d|.  To first order
        |device - exact| <= (1 + (D - 1)) 2^-53 sum_d |term_d| = ndims 2^-53 sum_d |term_d|.
    Derived, not tuned."""
    E, gs, vr, gs_abs, vr_abs = want
    assert got.shape == (3,) + E.shape and np.all(np.isfinite(got)), tag
    bad = int(np.sum(got[0] != E))
    assert bad == 0, '%s: E differs from the evaluation kernel on %d of %d states' % (tag, bad, E.size)
    for name, g, exact, absum in (('grad_sq', got[1], gs, gs_abs), ('virial', got[2], vr, vr_abs)):
        err = np.abs(g.astype(LD) - exact)
        bound = D * LD(U) * absum
        worst = float(np.max(err / np.where(bound > 0, bound, 1)))
        print('%s %s: D = %d, max |device - longdouble| / bound = %.3g' % (tag, name, D, worst))
        assert np.all(err <= bound), (tag, name, worst)
    assert np.all(got[1] >= 0) and np.any(got[1] > 0) and np.any(got[2] != 0), tag


def evaluated(dev, n):
    fn = dev.energy_observables()
    fn.ring_alloc(n)
    fn.evaluate(0, n, 0)
    return fn


def raw_slot(ctx, fn, slot, N):
    """a derived slot as it lies on the device, (Npad, 4) float64 (the test build's mjhmc_test_functionals_read_raw)"""
    from mjhmc_amd import engine
    Npad = (N + 63) // 64 * 64
    buf = np.full((Npad, 4), np.nan)
    engine.check(ctx.lib.mjhmc_test_functionals_read_raw(fn.handle, slot, buf.ctypes.data, buf.nbytes), ctx.lib)
    return buf


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
def _gauss(D, N):
    from mjhmc_amd.misc.distributions import TestGaussian
    from mjhmc_amd.samplers.markov_jump_hmc import MarkovJumpHMC
    X0 = np.random.RandomState(100 * D + N).randn(D, N) * 1.3 + 0.5

    class Fixed(TestGaussian):
        def gen_init_X(self):
            self.Xinit = X0
    return MarkovJumpHMC(distribution=Fixed(ndims=D, nbatch=N, sigma=1.3), epsilon=0.3, beta=0.3, num_leapfrog_steps=5,
                         seed=11, resample=False)


def _pot64():
    """the ProductOfT of _pot32 with the default float64 state: the multi-pass path (wide_run_eval)"""
    from mjhmc_amd.misc.distributions import ProductOfT
    from mjhmc_amd.samplers.markov_jump_hmc import MarkovJumpHMC
    rs = np.random.RandomState(8)
    D, N = 36, 120
    sp = rs.rand(D, D)
    W = rs.randn(D, D)
    W[sp > 0.05] = 0
    W += np.eye(D)
    lognu = np.log(rs.rand(D) * 2 + 2.1)
    X0 = rs.randn(D, N)

    class FixedT(ProductOfT):
        def gen_init_X(self):
            self.Xinit = X0
    d = FixedT(ndims=D, nbasis=D, nbatch=N, lognu=lognu, W=W)
    assert d.state_dtype == 'float64'
    return MarkovJumpHMC(distribution=d, epsilon=0.1, beta=0.3, num_leapfrog_steps=6, seed=99, resample=False)


def _sic_f32():
    from mjhmc_amd.misc.distributions import SparseImageCode
    from mjhmc_amd.samplers.markov_jump_hmc import MarkovJumpHMC
    from tests.helpers import sic_problem
    B, imgs, a0 = sic_problem(3, n_patches=1, n_coeffs=512)
    N = 40
    X0 = a0[:, None] + 0.3 * np.random.RandomState(8).randn(512, N)
    d = SparseImageCode(n_patches=1, n_batches=N, cauchy=True, n_basis=512, basis=B, imgs=imgs, init=X0, state_dtype='float32')
    return MarkovJumpHMC(distribution=d, epsilon=0.0625, beta=0.3, num_leapfrog_steps=6, seed=3, resample=False)


def _coupled_expr():
    """a coupled user-expression energy (hipRTC): E = S / 2 + p0 S^2 / 4 with S = |x|^2, dE/dx_d = x_d (1 + p0 S)"""
    from mjhmc_amd.misc.distributions import LambdaDistribution
    from mjhmc_amd.samplers.markov_jump_hmc import MarkovJumpHMC
    D, N = 7, 70
    X0 = np.random.RandomState(21).randn(D, N) * 0.8
    d = LambdaDistribution(init=X0, name='quartic shell',
                           device_expr=dict(stats=['x*x'], energy='0.0', energy0='0.5*S[0] + 0.25*p[0]*S[0]*S[0]',
                                            grad='x*(1.0 + p[0]*S[0])'), device_params=[0.05])
    return MarkovJumpHMC(distribution=d, epsilon=0.15, beta=0.3, num_leapfrog_steps=5, seed=17, resample=False)


def _corr_gauss():
    """a linear-model energy on the matrix-core tile kernels: 36 dims x 120 chains, float64 state around the float32 force"""
    from mjhmc_amd.misc.distributions import CorrelatedGaussian
    from mjhmc_amd.samplers.markov_jump_hmc import MarkovJumpHMC
    np.random.seed(5)
    d = CorrelatedGaussian(ndims=36, nbatch=120, log_conditioning=1, seed=2)
    return MarkovJumpHMC(distribution=d, epsilon=0.1, beta=0.3, num_leapfrog_steps=5, seed=23, resample=False)


FAMILIES = {
    'pot36_f32': _pot32,             # float32 rows, 36 of a 128-element pitch; float32 dE/dX and E
    'pot36_f64': _pot64,             # the same energy, float64 state: narrow / force / widen passes
    'sic512_bf16': _sic_bf16,        # bfloat16 rows of 512 (8 elements a lane), float32 dE/dX: two 16-byte loads a chunk
    'sic512_f32': _sic_f32,
    'funnel32x130': _funnel,
    'coupled_expr7x70': _coupled_expr,
    'corr_gauss36x120': _corr_gauss,
}


# ---------------------------------------------------------------------------------------------------------------------
# 1.  values
# ---------------------------------------------------------------------------------------------------------------------
def _check_values(s, n, tag):
    X, w, w_slot0 = record(s, n)
    dev = s._dev
    D, N = dev.ndims, dev.nparticles
    fn = evaluated(dev, n)
    assert fn.n_values == 3 and fn.slot_bytes == (N + 63) // 64 * 64 * 4 * 8
    got = fn.read(0, n)
    assert_sums_within_bound(got, host_values(s.distribution, X[:, :n, :]), D, tag)
    again = dev.energy_observables()
    again.ring_alloc(n + 1)
    again.evaluate(0, n, 1)
    assert np.array_equal(again.read(1, n), got), 'a second handle, another derived slot: the same bits'
    assert np.all(again.read(0, 1) == 0.0)
    return fn, got, X, w, w_slot0


@pytest.mark.parametrize('D', [1, 2, 3, 33, 130])
@pytest.mark.parametrize('N', [1, 65, 200])
def test_values_gaussian_float64(D, N):
    """one 16-byte chunk per row (D = 1, 2), a padded row (3, 33: pitch 4, 34; 17 chunks), more chunks than a wave has lanes
    (130: the wave-per-row path); N = 1, one past a wave of rows (Npad > N), several workgroups"""
    s = _gauss(D, N)
    fn, got, X, w, w_slot0 = _check_values(s, 3, 'gauss D=%d N=%d' % (D, N))
    # a closed form on top: E = |x|^2 / (2 sigma^2), G = x / sigma^2, so virial = 2 E and grad_sq = 2 E / sigma^2 up to rounding
    assert np.allclose(got[2], 2 * got[0], rtol=1e-12, atol=0) and np.allclose(got[1] * 1.3 ** 2, 2 * got[0], rtol=1e-12, atol=0)


@pytest.mark.parametrize('case', sorted(FAMILIES))
def test_values_every_energy_family(case):
    s = FAMILIES[case]()
    _check_values(s, 3, case)


@pytest.mark.parametrize('D,N', [(2, 1), (33, 65), (130, 200)])
def test_row_padding_and_element_three(D, N):
    """the derived slot as the device holds it: elements 0 .. 2 of the rows p < N are the values, element 3 is 0.0, rows
    p >= N are 0.0 -- and NaN bytes in the padding rows of the SAMPLE ring change nothing, because rows p >= N are not read"""
    from mjhmc_amd import engine
    n = 3
    rs = np.random.RandomState(3)
    ctx, dev, X = _ring(rs.randn(D, n, N) * 1.1)
    fn = evaluated(dev, n)
    before = fn.read(0, n)
    for k in range(n):
        engine.check(ctx.lib.mjhmc_test_ring_fill_padding(dev.handle, k, 0xFF), ctx.lib)
    fn.evaluate(0, n, 0)
    assert np.array_equal(fn.read(0, n), before) and np.all(np.isfinite(before))
    for k in range(n):
        rows = raw_slot(ctx, fn, k, N)
        assert np.array_equal(rows[:N, :3].T, before[:, k, :])
        assert np.all(rows[:N, 3] == 0.0) and not np.any(np.signbit(rows[:N, 3]))
        assert not rows[N:].view(np.uint64).any(), 'slot %d: a padding row was written' % k
    # E_ISO_GAUSS with sigma = 1: G = x, so grad_sq == virial bit for bit, and both are sum x^2 within the bound
    assert np.array_equal(before[1], before[2])
    exact = (X.astype(LD) ** 2).sum(axis=0)
    assert np.all(np.abs(before[1].astype(LD) - exact) <= D * LD(U) * exact)


# ---------------------------------------------------------------------------------------------------------------------
# 2.  blocks and the run
# ---------------------------------------------------------------------------------------------------------------------
def _same_run(s, t):
    assert (s.l_count, s.f_count, s.r_count, s.fl_count) == (t.l_count, t.f_count, t.r_count, t.fl_count)
    assert (s.distribution.E_count, s.distribution.dEdX_count) == (t.distribution.E_count, t.distribution.dEdX_count)
    assert np.array_equal(s.state.X, t.state.X) and np.array_equal(s.state.V, t.state.V)
    assert s._dev.get_tick() == t._dev.get_tick()
    if s._dwell_weighted:
        assert np.array_equal(s.dwelling_times, t.dwelling_times)


EO_SHIFT = np.array([20.0, 25.0, 30.0])


@pytest.mark.parametrize('cls', ['MarkovJumpHMC', 'ControlHMC'])
def test_the_run_is_that_of_of_none_and_repeats_bit_for_bit(cls):
    """expectations(n, of=EO, block=b), b in {1, 3, None}, against a same-seed sampler run with of=None: final X and V,
    counters, dwelling times, tick, E_count and dEdX_count are equal (the observable's evaluations are not counted); two
    runs with the same blocks are bit-identical"""
    D, N, n_iter = 33, 100, 7
    for b in (1, 3, None):
        s, t, again = _iso(D, N, 5, cls), _iso(D, N, 5, cls), _iso(D, N, 5, cls)
        e = s.expectations(n_iter, block=b, shift=EO_SHIFT, of=s.energy_observables())
        t.expectations(n_iter, block=b)
        _same_run(s, t)
        assert e.n_states == n_iter * N and e.mean.shape == (3,) and np.all(np.isfinite(e.mean)) and np.all(e.var > 0)
        e2 = again.expectations(n_iter, block=b, shift=EO_SHIFT, of=again.energy_observables())
        _same_run(again, t)
        assert e.W == e2.W and np.array_equal(e.S1, e2.S1) and np.array_equal(e.S2, e2.S2), b


@pytest.mark.parametrize('cls', ['MarkovJumpHMC', 'ControlHMC'])
def test_expectations_are_identical_across_blocks(cls):
    """expectations(n, of=EO, block=b) for b in {1, 3, None}: identical W, S1, S2 under the same shift.  The pooled moment
    pass adds a call's sum to its running totals, so a block accumulated in one call gives sums that depend on the cut in
    their last bits (tests/test_gpu_estimators.py::test_stitching_and_bookkeeping compares "up to the order of addition");
    with of=EO the driver accumulates slot by slot, as the block was evaluated, and the sums are the same bits."""
    D, N, n_iter = 33, 100, 7
    runs = []
    for b in (1, 3, None):
        s = _iso(D, N, 5, cls)
        e = s.expectations(n_iter, block=b, shift=EO_SHIFT, of=s.energy_observables())
        runs.append((e.W, e.S1, e.S2))
        print('%s block=%s: W = %r, S1 = %r, S2 = %r' % (cls, b, e.W, e.S1.tolist(), e.S2.tolist()))
    for other in runs[1:]:
        assert runs[0][0] == other[0] and np.array_equal(runs[0][1], other[1]) and np.array_equal(runs[0][2], other[2])


@pytest.mark.parametrize('cls', ['MarkovJumpHMC', 'ControlHMC'])
def test_values_and_chain_sums_do_not_depend_on_the_blocks(cls):
    """what of the block independence is the feature's own: the derived values of a run recorded in one ring evaluated as
    one block or as 3 + 3 + 1 are the same bits, and diagnostics(of=EO) -- whose per-chain sums run over a chain's states
    in order whatever the blocks -- gives identical Sw, Sm, Sq, Sv for blocks of 1, 3 and the default"""
    D, N, n_iter = 33, 100, 7
    m = _iso(D, N, 5, cls)
    X, w, w_slot0 = record(m, n_iter)
    fn = evaluated(m._dev, n_iter)
    whole, at, cut = fn.read(0, n_iter), 0, []
    for k in (3, 3, 1):
        fn.evaluate(at, k, 0)
        cut.append(fn.read(0, k))
        at += k
    assert np.array_equal(whole, np.concatenate(cut, axis=1))
    runs = []
    for b in (1, 3, None):
        s = _iso(D, N, 5, cls)
        d = s.diagnostics(n_iter - 1, split=False, block=b, shift=EO_SHIFT, of=s.energy_observables())
        runs.append((np.float64(d.Sw), d.Sm, d.Sq, d.Sv))
    assert _same(runs[0], runs[1]) and _same(runs[0], runs[2])


# ---------------------------------------------------------------------------------------------------------------------
# 3.  each driver once
# ---------------------------------------------------------------------------------------------------------------------
def test_each_driver_equals_its_accumulator_by_hand():
    """_iso(33, 100): the twin m records the same run in one ring; its values V are E from the host evaluation and grad_sq,
    virial as the device pass gives them, after those were held against the host sums (section 1's bound).  On V the NumPy
    restatements of the passes: chain sums + fold bound (tests/test_gpu_chainstats.py), integer histogram tables
    (tests/test_gpu_marginals.py), pair tables (tests/test_gpu_joint_marginals.py)."""
    D, N, n = 33, 100, 12
    m = _iso(D, N, 7)
    X, w, w_slot0 = record(m, n)
    fn = evaluated(m._dev, n)
    V = fn.read(0, n)
    want = host_values(m.distribution, X[:, :n, :])
    assert_sums_within_bound(V, want, D, 'driver twin')
    V[0] = want[0]
    shift = np.array([18.0, 22.0, 36.0])

    s = _iso(D, N, 7)
    EO = s.energy_observables()
    d = s.diagnostics(n, split=False, block=5, shift=shift, of=EO)
    assert (d.n_chains, d.n_states) == (N, n) and d.mean.shape == (3,)
    assert_fold_within_bound((d.Sw, d.Sm, d.Sq, d.Sv), *host_chain_sums(V, w, shift), tag='diagnostics(of=EO)')
    cs = fn.chain_stats(1)
    cs.set_shift(shift)
    cs.accumulate(0, n, w_slot0=w_slot0)
    by_hand = cs.read(0)
    assert d.parts[0][:3] == by_hand[:3] and _same(d.parts[0][3:], by_hand[3:])
    assert _same(cs.read_chains(), host_chain_sums(V, w, shift))

    B = 32
    lo, hi = np.array([0.0, 0.0, 0.0]), np.array([60.0, 80.0, 100.0])
    s = _iso(D, N, 7)
    mg = s.marginals(n, bins=B, range=(lo, hi), block=5, of=s.energy_observables())
    got = (mg.counts, mg.units, mg.W_units)
    ref = host_hist(V, w, lo, hi, B, mg.quantum)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and got[2] == ref[2]
    assert mg.n_states == n * N and mg.counts[:, 1:-1].sum() > 0.9 * 3 * n * N

    s = _iso(D, N, 7)
    pairs = np.array([(0, 2)])
    jm = s.joint_marginals(n, pairs=[(0, 2)], bins=16, range=(lo, hi), block=5, of=s.energy_observables())
    ref = host_pairhist(V, w, pairs, jm.lo, jm.hi, 16, jm.quantum)
    assert np.array_equal(jm.counts, ref[0]) and np.array_equal(jm.units, ref[1]) and jm.W_units == ref[2]
    assert jm.n_states == n * N
    # TestGaussian: virial = 2 E, so the joint of (E, virial) lives on one line of cells
    assert np.count_nonzero(jm.counts[0]) <= 2 * 18


# ---------------------------------------------------------------------------------------------------------------------
# 4.  refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from mjhmc_amd import _lib
    from mjhmc_amd._lib import EngineError
    from mjhmc_amd.misc.distributions import LambdaDistribution
    from mjhmc_amd.samplers.markov_jump_hmc import MarkovJumpHMC
    # an opaque pair of callables: refused at energy_observables(), the sampler untouched
    A = np.array([[2.0, 0.5], [0.5, 1.0]])
    d = LambdaDistribution(energy_func=lambda X: 0.5 * np.sum(X * A.dot(X), axis=0).reshape(1, -1),
                           energy_grad_func=lambda X: A.dot(X), init=np.random.RandomState(1).randn(2, 70), name='dense quadratic')
    h = MarkovJumpHMC(distribution=d, epsilon=0.2, beta=0.3, num_leapfrog_steps=3, seed=5, resample=False)
    tick0, X0, V0 = h._dev.get_tick(), h.state.X.copy(), h.state.V.copy()
    counts0 = (h.distribution.E_count, h.distribution.dEdX_count)
    with pytest.raises(ValueError, match='opaque Python callables'):
        h.energy_observables()
    with pytest.raises(ValueError, match='opaque Python callables'):
        h.temperature(8)
    h._dev.ring_alloc(2)
    with pytest.raises(EngineError, match='callables are the only evaluation'):
        h._dev.energy_observables()
    assert h._dev.get_tick() == tick0 and np.array_equal(h.state.X, X0) and np.array_equal(h.state.V, V0)
    assert (h.distribution.E_count, h.distribution.dEdX_count) == counts0
    # no sample ring yet; a re-allocated one
    s = _iso(33, 100, 1)
    with pytest.raises(EngineError, match='no sample ring'):
        s._dev.energy_observables()
    s._dev.ring_alloc(3)
    s._run(3, ring_slot0=0)
    fn = s._dev.energy_observables()
    with pytest.raises(EngineError, match='no derived ring'):
        fn.evaluate(0, 1, 0)
    fn.ring_alloc(2)
    fn.evaluate(1, 2, 0)
    with pytest.raises(EngineError, match='outside the ring of 3'):
        fn.evaluate(2, 2, 0)
    with pytest.raises(EngineError, match='outside the derived ring of 2'):
        fn.evaluate(0, 3, 0)
    s._dev.ring_alloc(5)
    with pytest.raises(EngineError, match='sample ring was re-allocated'):
        fn.evaluate(0, 1, 0)
    fn.close()
    # a state whose energy overflows: the flag names E, and does not stick
    X = np.random.RandomState(2).randn(4, 2, 70)
    X[1, 1, 33] = 1e200
    ctx, dev, stored = _ring(X)
    bad = dev.energy_observables()
    bad.ring_alloc(2)
    bad.evaluate(0, 1, 0)
    with pytest.raises(EngineError, match=r'value 0 \(E\) of the energy observables is not finite'):
        bad.evaluate(0, 2, 0)
    assert dev.lib.mjhmc_functionals_evaluate(bad.handle, 1, 1, 0) == _lib.ERR_NONFINITE
    bad.evaluate(0, 1, 1)
    est = bad.estimator()
    dev.close()                                                       # the sampler frees the handle, its scratch and what was created on it
    est.close()
    bad.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5.  the thermometer
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cls', ['MarkovJumpHMC', 'ControlHMC'])
def test_thermometer_reads_one_on_a_chain_that_keeps_the_law(cls):
    """_iso(17, 1000) after burn_in(), temperature(64): |T - 1| <= 5 stderr, and 5 stderr <= 0.05 -- the second condition
    is what gives the first its power against a chain 5 % off."""
    s = _iso(17, 1000, 31, cls)
    s.burn_in()
    t = s.temperature(64)
    print('%s: T = %.6f, stderr = %.6f, z = %.3f, ESS(virial) = %.1f of %d states, rhat(E) = %.5f, <E> = %.4f'
          % (cls, t.T, t.stderr, t.z, t.diagnostics.ess[2], 64 * 1000, t.rhat_energy, t.mean_energy))
    assert t.ndims == 17 and t.diagnostics.n_chains == 2000 and t.diagnostics.n_states == 32
    assert np.isfinite(t.T) and np.isfinite(t.stderr) and t.stderr > 0
    assert 5 * t.stderr <= 0.05, (t.T, t.stderr)
    assert abs(t.T - 1) <= 5 * t.stderr, (t.T, t.stderr, t.z)
    assert abs(t.mean_energy - 17 / 2.0) <= 0.05 * 17 / 2.0             # <E> = ndims / 2 for a Gaussian (equipartition)
