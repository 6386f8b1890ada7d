"""GPU: per-expert statistics of linear models on the device (csrc/dense_lin_pointwise.hpp, csrc/pointwise.hip,
mjhmc_pointwise_*, HMCBase.pointwise / waic) against float64 NumPy restatements on the float32-rounded
model and states.  Shapes are the smallest at which each failure can occur: block boundaries of the experts, a partial last
block, a partial second tile, three strips with the last partial."""
import numpy as np
import pytest

from tests.helpers import hooks_context
from tests.test_gpu_linear import EXPRS, f32, model, rel, restated            # noqa: F401  (the linear tests' own models)

pytestmark = pytest.mark.gpu
np.seterr(all='ignore')

SOFTPLUS = EXPRS['softplus'][0]
SHAPES = [(10, 513), (129, 640), (300, 1100), (36, 36)]      # the last: mjhmc_energy_create_linear, the tile path's one block
U24 = 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------------------
# the NumPy restatement
# ---------------------------------------------------------------------------------------------------------------------
def host_u(W, b, X):
    """u (K, n) in float64 from the float32-rounded W, b, X, and the bound of its float32 evaluation in ANY order of sums:
    |du| <= gamma_D (sum_d |W||x| + |b|), gamma_D = D 2^-24 / (1 - D 2^-24)"""
    W32, b32, X32 = f32(W), f32(b), f32(X)
    D = W.shape[1]
    gamma = D * U24 / (1 - D * U24)
    return W32.dot(X32) + b32[:, None], gamma * (np.abs(W32).dot(np.abs(X32)) + np.abs(b32)[:, None])


def host_softplus(u):
    return np.where(u > 20, u, np.log1p(np.exp(np.minimum(u, 20))))


def host_stats(t, w):
    """weighted mean, sqrt(population variance) and log-mean-exp per expert of t (K, n) with weights w (n,)"""
    on = w > 0
    t, w = t[:, on], w[on]
    W = w.sum()
    mean = (t * w).sum(axis=1) / W
    sd = np.sqrt(np.maximum((w * (t - mean[:, None]) ** 2).sum(axis=1) / W, 0))
    mx = t.max(axis=1)
    return mean, sd, np.log((w * np.exp(t - mx[:, None])).sum(axis=1) / W) + mx


def host_bar(du, t, w, lipschitz=1.0):
    """the bar of a statistic of value t: per (expert, particle) lipschitz * |du| + 4 float32 ulps of |t| (expf / log1pf),
    averaged over the particles as the statistic averages"""
    on = w > 0
    e = lipschitz * du[:, on] + 4 * 2.0 ** -23 * np.abs(t[:, on])
    return (e * w[on]).sum(axis=1) / w[on].sum()


# ---------------------------------------------------------------------------------------------------------------------
# engine-level fixtures: a sampler of the test build whose ring slots hold given states and weights
# ---------------------------------------------------------------------------------------------------------------------
def ring_sampler(W, b, X, dtype='float64', q=None, w=None, energy='softplus'):
    """X (D, n, N) float32-valued states -> a DeviceSampler whose ring slots 0 .. n - 1 hold them (mjhmc_test_ring_write)
    and whose dwell slots hold w (n, N) (mjhmc_test_ring_write_dwell)"""
    from mjhmc_amd import engine, _lib
    ctx = hooks_context(0)
    K, D = W.shape
    e, g = EXPRS[energy][:2]
    make = engine.DeviceEnergy.from_linear_tall if K > 512 else engine.DeviceEnergy.from_linear
    en = make(ctx, W, b, e, g, expert_params=q)
    n, N = X.shape[1], X.shape[2]
    dev = engine.DeviceSampler(en, np.zeros((D, N)), seed=5, dtype=dtype, mode=_lib.MODE_MJHMC)
    dev.ring_alloc(n)
    for k in range(n):
        block = np.ascontiguousarray(X[:, k, :], dtype=np.float64)
        engine.check(ctx.lib.mjhmc_test_ring_write(dev.handle, k, block.ctypes.data), ctx.lib)
        if w is not None:
            for p in range(N):
                engine.check(ctx.lib.mjhmc_test_ring_write_dwell(dev.handle, k, p, float(w[k, p])), ctx.lib)
    assert np.array_equal(dev.ring_read(0, n).reshape(D, n, N), X)
    return ctx, dev


def stats_of(dev, values, flags, n, w_slot0=-1):
    from mjhmc_amd.samplers.markov_jump_hmc import PointwiseStatistics
    pw = dev.pointwise(values, flags)
    pw.accumulate(0, n, w_slot0=w_slot0)
    out = PointwiseStatistics(*(pw.read() + (flags,)))
    pw.close()
    return out


def raw(p):
    return (p.W, p.S1, p.S2, p.lme_max, p.lme_sum, p.n_states)


def same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(raw(a), raw(b)))


# ---------------------------------------------------------------------------------------------------------------------
# 1. exact structure
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('D,K', SHAPES)
def test_exact_structure(D, K, dtype):
    """values (float)j and q[0] = 1 + j / K over 45 particles of unit weight: S1 = 45 j, S2 = 45 j^2 and the mean of q[0]
    exactly, for every expert -- the global expert index across block boundaries, the mask of the last block, the rows
    beyond the batch (the second tile is partial)"""
    W, b, _ = model(D, K, 'softplus')
    q0 = 1.0 + np.arange(K) / K
    X = f32(np.random.RandomState(D).randn(D, 1, 45))
    _, dev = ring_sampler(W, b, X, dtype=dtype, q=q0[None, :])
    p = stats_of(dev, ['(float)j', 'q[0]'], [False, False], 1)
    j = np.arange(K, dtype=np.float64)
    assert p.W == 45.0 and p.n_states == 45
    assert p.S1.shape == (2, K)
    assert np.array_equal(p.S1[0], 45 * j) and np.array_equal(p.S2[0], 45 * j * j)
    assert np.array_equal(p.mean[1], f32(q0))
    assert np.all(np.isneginf(p.lme_max)) and np.all(p.lme_sum == 0.0)         # (-inf, 0) where not requested
    dev.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. values of u
# ---------------------------------------------------------------------------------------------------------------------
def u_case(D, K):
    W, b, _ = model(D, K, 'softplus')
    X = f32(np.random.RandomState(D).randn(D, 1, 45))
    return W, b, X


def u_reference(W, b, X):
    """per value ('u', softplus): (mean, sd, lme) and their bars, unit weights"""
    u, du = host_u(W, b, X[:, 0, :])
    w = np.ones(u.shape[1])
    out = []
    for t in (u, host_softplus(u)):
        out.append((host_stats(t, w), host_bar(du, t, w)))
    return u, du, out


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('D,K', SHAPES)
def test_values_of_u(D, K, dtype):
    """u and softplus(u), log-mean-exp on both, within 2x the bar computed here from the model: gamma_D (sum |W||x| + |b|)
    times the value's Lipschitz constant (1 for both) + 4 float32 ulps of |h|, averaged over the particles.  The bar
    discriminates: one dropped particle, or the expert index off by one, moves some expert's mean by more than 10 bars."""
    W, b, X = u_case(D, K)
    u, du, ref = u_reference(W, b, X)
    # the controls, on NumPy alone
    w = np.ones(45)
    for m, t in enumerate((u, host_softplus(u))):
        (mean, _, _), bar = ref[m]
        dropped = host_stats(t[:, :44], w[:44])[0]
        shifted = np.roll(mean, 1)
        assert (np.abs(dropped - mean) / bar).max() > 10 and (np.abs(shifted - mean) / bar).max() > 10, m
    _, dev = ring_sampler(W, b, X, dtype=dtype)
    p = stats_of(dev, ['u', SOFTPLUS], [True, True], 1)
    worst = 0.0
    for m in range(2):
        (mean, sd, lme), bar = ref[m]
        for name, got, want in (('mean', p.mean[m], mean), ('sd', np.sqrt(p.var[m]), sd), ('lme', p.log_mean_exp[m], lme)):
            ratio = float((np.abs(got - want) / bar).max())
            worst = max(worst, ratio)
            print('%dx%d %s value %d %s: worst error / bar = %.3f' % (D, K, dtype, m, name, ratio))
            assert ratio <= 2.0, (m, name, ratio)
    print('%dx%d %s: worst ratio %.3f' % (D, K, dtype, worst))
    dev.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. weights: the jump sampler's holding times
# ---------------------------------------------------------------------------------------------------------------------
FAMILY = (24, 700)      # test_gpu_linear_tall.py's softplus family: 6 blocks of 128, the last with 60 experts


def family_sampler(seed=23, N=96):
    from mjhmc_amd.misc.distributions import LambdaDistribution
    from mjhmc_amd.samplers.markov_jump_hmc import MarkovJumpHMC
    W, b, _ = model(FAMILY[0], FAMILY[1], 'softplus', seed=9)
    X0 = np.random.RandomState(11).randn(FAMILY[0], N)
    e, g = EXPRS['softplus'][:2]
    d = LambdaDistribution(init=X0, device_linear_tall=dict(W=W, b=b, energy=e, grad=g))
    return MarkovJumpHMC(distribution=d, seed=seed, epsilon=0.2, beta=0.3, num_leapfrog_steps=5, resample=False), W, b


def test_weights_are_the_holding_times():
    s, W, b = family_sampler()
    p = s.pointwise(6, values=['u', SOFTPLUS], log_mean_exp=[True, True])
    # the same run again: 7 iterations, the first 6 states weighted by the holding times the NEXT iteration drew
    r, _, _ = family_sampler()
    r._dev.ring_alloc(7)
    r._run(7, ring_slot0=0)
    r._publish()
    r._read_dwell()
    X = r._dev.ring_read(0, 7).reshape(FAMILY[0], 7, 96)
    dwell = r._dev.ring_read_dwell(0, 7)
    assert np.array_equal(dwell[6], r.dwelling_times)
    w = dwell[1:7].reshape(-1)
    assert np.all(w > 0) and np.all(np.isfinite(w))
    assert abs(p.W - w.sum()) <= 1e-12 * w.sum() and p.n_states == 6 * 96
    u, du = host_u(W, b, X[:, :6, :].reshape(FAMILY[0], -1))
    for m, t in enumerate((u, host_softplus(u))):
        mean, sd, lme = host_stats(t, w)
        bar = host_bar(du, t, w)
        for name, got, want in (('mean', p.mean[m], mean), ('sd', np.sqrt(p.var[m]), sd), ('lme', p.log_mean_exp[m], lme)):
            ratio = float((np.abs(got - want) / bar).max())
            print('weights value %d %s: worst error / bar = %.3f' % (m, name, ratio))
            assert ratio <= 2.0, (m, name, ratio)
    # the run is that of expectations(6), bit for bit
    t, _, _ = family_sampler()
    t.expectations(6)
    for a in (s, r):
        assert (a.l_count, a.f_count, a.r_count, a.fl_count) == (t.l_count, t.f_count, t.r_count, t.fl_count)
        assert (a.distribution.E_count, a.distribution.dEdX_count) == (t.distribution.E_count, t.distribution.dEdX_count)
        assert np.array_equal(a.state.X, t.state.X) and np.array_equal(a.state.V, t.state.V)
        assert np.array_equal(a.dwelling_times, t.dwelling_times)


# ---------------------------------------------------------------------------------------------------------------------
# 4. determinism
# ---------------------------------------------------------------------------------------------------------------------
def test_bit_identical_across_runs_and_blocks():
    from mjhmc_amd.misc.distributions import LambdaDistribution
    from mjhmc_amd.samplers.markov_jump_hmc import MarkovJumpHMC
    D, K = 512, 1537
    W, b, _ = model(D, K, 'softplus')
    e, g = EXPRS['softplus'][:2]
    # strip_tiles from the library: three strips, the last partial
    _, probe = ring_sampler(W, b, f32(np.zeros((D, 1, 8))))
    h = probe.pointwise(['u'])
    strip_tiles = h.strip_tiles
    assert h.n_values == 1 and h.nexperts == K and strip_tiles >= 1
    probe.close()
    N = strip_tiles * 32 * 2 + 13
    X0 = np.random.RandomState(2).randn(D, N)

    def run(block, n=N):
        d = LambdaDistribution(init=X0[:, :n], device_linear_tall=dict(W=W, b=b, energy=e, grad=g))
        s = MarkovJumpHMC(distribution=d, seed=31, epsilon=0.05, beta=0.3, num_leapfrog_steps=3, resample=False)
        return s.pointwise(6, values=['u', SOFTPLUS], log_mean_exp=[True, True], block=block)
    a, a2, b1, b3 = run(None), run(None), run(1), run(3)
    assert np.isfinite(a.mean).all() and np.isfinite(a.log_mean_exp).all() and a.n_states == 6 * N
    assert same_bits(a, a2)
    assert same_bits(a, b1) and same_bits(a, b3)
    small = run(None, 45)                            # the control: the first 45 particles alone give other sums
    assert not np.array_equal(small.S1, a.S1) and small.n_states == 6 * 45


# ---------------------------------------------------------------------------------------------------------------------
# 5. log-mean-exp under shifts; a particle of weight 0
# ---------------------------------------------------------------------------------------------------------------------
def dyadic_case(N=70, n=2):
    """W, b, X on small dyadic grids: u = W x + b is exact in float32 (a multiple of 2^-5, |u| < 16), and so is u - 900"""
    rs = np.random.RandomState(8)
    D, K = 10, 513
    W = rs.randint(-2, 3, size=(K, D)) / 4.0
    b = rs.randint(-4, 5, size=K) / 8.0
    X = rs.randint(-8, 9, size=(D, n, N)) / 8.0
    return W, b, X


def test_log_mean_exp_under_a_shift_of_900():
    W, b, X = dyadic_case()
    _, dev = ring_sampler(W, b, X)
    p = stats_of(dev, ['u', 'u - 900.f'], [True, True], 2)
    u = W.dot(X.reshape(10, -1)) + b[:, None]
    assert np.abs(u).max() < 16 and np.exp(u.min() - 900.0) == 0.0           # a plain mean of exp would be 0
    assert np.isfinite(p.log_mean_exp).all()
    assert np.abs(p.log_mean_exp[1] - (p.log_mean_exp[0] - 900.0)).max() <= 1e-6
    assert np.abs(p.log_mean_exp[0] - host_stats(u, np.ones(u.shape[1]))[2]).max() <= 1e-6
    assert np.array_equal(p.lme_max[1], p.lme_max[0] - 900.0) and np.array_equal(p.lme_sum[1], p.lme_sum[0])
    dev.close()


def test_a_particle_of_weight_zero_changes_nothing():
    """a hand-written dwell slot (the test build's ring hooks): particle 13 of slot 0 has weight 0 and a state of 2^60 -- a
    huge u, a huge value; the sums are those of the same ring with an ordinary state there, bit for bit"""
    W, b, X = dyadic_case()
    w = np.random.RandomState(3).randint(1, 9, size=(2, 70)) / 4.0
    w[0, 13] = 0.0
    Xh = X.copy()
    Xh[:, 0, 13] = 2.0 ** 60
    _, d1 = ring_sampler(W, b, X, w=w)
    _, d2 = ring_sampler(W, b, Xh, w=w)
    vals, flags = ['u', 'u - 900.f', 'u*u'], [True, True, False]
    p1, p2 = stats_of(d1, vals, flags, 2, w_slot0=0), stats_of(d2, vals, flags, 2, w_slot0=0)
    assert same_bits(p1, p2)
    assert p1.W == w.sum() and np.isfinite(p2.S2).all()
    u = W.dot(X.reshape(10, -1)) + b[:, None]
    assert np.array_equal(p1.S1[0], (u * w.reshape(-1)).sum(axis=1))          # dyadic: the weighted sums are exact
    d1.close()
    d2.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_a_value_that_is_not_finite_refuses_the_block():
    from mjhmc_amd import _lib
    W, b, X = dyadic_case()
    w = np.ones((2, 70))
    ctx, dev = ring_sampler(W, b, X, w=w)
    pw = dev.pointwise(['j == 7 ? logf(-1.f) : u', 'j == 3 || j == 600 ? logf(-1.f) : u'], [True, False])
    before = pw.read()
    with pytest.raises(_lib.EngineError) as err:
        pw.accumulate(0, 2)
    assert 'value 0' in str(err.value) and 'expert 7 ' in str(err.value) and 'status -5' in str(err.value)
    after = pw.read()
    assert all(np.array_equal(x, y) for x, y in zip(before, after)) and after[0] == 0.0 and after[5] == 0
    pw.close()
    # a refused weight leaves the sums of the blocks before it as they were
    from mjhmc_amd import engine
    ok = dev.pointwise(['u'], [True])
    ok.accumulate(0, 1, w_slot0=0)
    kept = ok.read()
    engine.check(ctx.lib.mjhmc_test_ring_write_dwell(dev.handle, 1, 5, -1.0), ctx.lib)
    with pytest.raises(_lib.EngineError, match='negative or not finite'):
        ok.accumulate(0, 2, w_slot0=0)
    assert all(np.array_equal(x, y) for x, y in zip(kept, ok.read()))
    ok.accumulate(0, 1, w_slot0=0)                     # and the handle goes on
    assert ok.read()[0] == 2 * kept[0]
    dev.close()                                        # a closed sampler has freed the handles
    ok.close()


def test_other_energies_are_refused_by_name():
    from mjhmc_amd import engine, _lib
    from mjhmc_amd.misc.distributions import ProductOfT
    from mjhmc_amd.samplers.markov_jump_hmc import HMC
    s = HMC(distribution=ProductOfT(ndims=36, nbasis=36, nbatch=40), epsilon=0.1, beta=0.3, num_leapfrog_steps=3, seed=1)
    before = (s.distribution.E_count, s.distribution.dEdX_count)
    with pytest.raises(ValueError, match='PRODUCT_OF_T'):
        s.pointwise(3, values=['u'])
    with pytest.raises(ValueError, match='pointwise_values'):
        s.waic(3)
    assert (s.distribution.E_count, s.distribution.dEdX_count) == before
    s._dev.ring_alloc(2)
    with pytest.raises(_lib.EngineError, match='MJHMC_E_PRODUCT_OF_T'):
        s._dev.pointwise(['u'])
    W, b, X = dyadic_case()
    _, dev = ring_sampler(W, b, X)
    import ctypes
    h = ctypes.c_void_p()
    with pytest.raises(ValueError, match='mask'):
        engine.check_args(dev.lib.mjhmc_pointwise_create(dev.handle, b'u', 2, _lib.KERNEL_HEADERS.encode(), ctypes.byref(h)), dev.lib)
    dev.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. WAIC against the closed form
# ---------------------------------------------------------------------------------------------------------------------
GLM_N = 4096


def gauss_glm():
    """test_gpu_linear_tall.py's construction: n = 1500 rows, D = 6, started from exact posterior draws"""
    from mjhmc_amd.misc.distributions import GeneralizedLinearModel
    rs = np.random.RandomState(2028)
    A = rs.randn(1500, 6)
    y = A.dot(rs.randn(6)) + rs.randn(1500)

    class FromThePosterior(GeneralizedLinearModel):
        def gen_init_X(self):
            m, c = self.posterior()
            self.Xinit = m[:, None] + np.linalg.cholesky(c).dot(np.random.RandomState(self.seed).randn(self.ndims, self.nbatch))

    d = FromThePosterior(A, y, 'gaussian', nbatch=GLM_N, seed=5)
    mean, cov = d.posterior()
    eps = 0.5 / np.sqrt(np.linalg.eigvalsh(np.linalg.inv(cov)).max())
    return d, mean, cov, eps


def waic_closed_form(d, mean, cov, widen=1.0):
    """per data row, u_i ~ N(mu_i, s_i^2) under x ~ N(mean, widen^2 cov): the exact means and standard errors over GLM_N
    independent draws of l_i = -u_i^2 / 2 and of u_i, lppd_i - const_i and Var[l_i]; and elpd_waic with the delta-method
    standard error of the SUM -- the rows share the draws, so it is the standard deviation over x of the influence function
        g(x) = sum_i [exp(l_i(x)) / E exp(l_i) - 1] - [(l_i(x) - E l_i)^2 - Var l_i]
    divided by sqrt(GLM_N), every expectation inside in closed form and the deviation over the 6-dimensional Gaussian from a
    fixed NumPy sample of 8192 draws (1 % accurate)"""
    A, y = d.features / d.noise_scale, d.targets / d.noise_scale
    n = A.shape[0]
    C = widen * widen * cov
    mu, s2 = A.dot(mean) - y, np.einsum('ij,jk,ik->i', A, C, A)
    El, Vl = -0.5 * (mu * mu + s2), 0.5 * s2 * s2 + mu * mu * s2
    lppd0 = -0.5 * np.log1p(s2) - mu * mu / (2 * (1 + s2))
    x = mean[:, None] + np.linalg.cholesky(C).dot(np.random.RandomState(77).randn(len(mean), 8192))
    l = -0.5 * (A.dot(x) - y[:, None]) ** 2
    g = (np.exp(l - lppd0[:, None]) - 1.0).sum(axis=0) - ((l - El[:, None]) ** 2 - Vl[:, None]).sum(axis=0)
    elpd = float((lppd0 + d.log_lik_constants() - Vl).sum())
    return dict(mu=mu, s=np.sqrt(s2), El=El, se_l=np.sqrt(Vl / GLM_N), se_u=np.sqrt(s2 / GLM_N), elpd=elpd,
                se_elpd=float(g.std() / np.sqrt(GLM_N)), p_waic=float(Vl.sum()), n=n)


def waic_z(wa, cf):
    """(z of every row's mean of l, z of every row's fitted u, z of elpd_waic) of a Waic against a closed form"""
    p = wa.pointwise
    n = cf['n']
    return (p.mean[0, :n] - cf['El']) / cf['se_l'], (p.mean[1, :n] - cf['mu']) / cf['se_u'], (wa.elpd_waic - cf['elpd']) / cf['se_elpd']


def test_waic_against_the_closed_form():
    from mjhmc_amd.samplers.markov_jump_hmc import HMC
    d, mean, cov, eps = gauss_glm()
    s = HMC(distribution=d, epsilon=eps, beta=0.3, num_leapfrog_steps=8, seed=13)
    wa = s.waic(1)                      # one recorded state of unit weight: 4096 posterior draws after a law-preserving step
    n = d.features.shape[0]
    assert wa.n_data == n and wa.pointwise.W == GLM_N and wa.pointwise.mean.shape == (2, n + 6)
    cf = waic_closed_form(d, mean, cov)
    zl, zu, ze = waic_z(wa, cf)
    print('waic: max |z| of mean l %.2f, of fitted %.2f; elpd_waic %.3f against %.3f +- %.3f (z %.2f); p_waic %.3f against %.3f'
          % (np.abs(zl).max(), np.abs(zu).max(), wa.elpd_waic, cf['elpd'], cf['se_elpd'], ze, wa.p_waic, cf['p_waic']))
    assert np.all(np.abs(zl) <= 6) and np.all(np.abs(zu) <= 6)
    assert abs(ze) <= 6
    assert np.allclose(wa.fitted, wa.pointwise.mean[1, :n] * d.noise_scale + d.targets)
    assert np.isclose(wa.waic, -2 * wa.elpd_waic) and wa.n_warn == 0 and wa.se > 0
    # negative control: against a posterior 1.3 x too wide the same bounds fail
    wide = waic_closed_form(d, mean, cov, widen=1.3)
    zl, zu, ze = waic_z(wa, wide)
    assert np.abs(zl).max() > 6 and abs(ze) > 6


def test_waic_of_the_logistic_regression():
    from mjhmc_amd.misc.distributions import GeneralizedLinearModel
    from mjhmc_amd.samplers.markov_jump_hmc import MarkovJumpHMC
    rs = np.random.RandomState(7)
    A = rs.randn(2000, 8)
    y = (rs.rand(2000) < 1 / (1 + np.exp(-A.dot(rs.randn(8))))).astype(float)
    d = GeneralizedLinearModel(A, y, 'logistic', nbatch=256, seed=3)
    s = MarkovJumpHMC(distribution=d, epsilon=0.01, beta=0.3, num_leapfrog_steps=8, seed=4, resample=False)
    # WAIC is a statement about posterior draws, and this sampler starts at N(0, 0.1^2), about 1 away from a posterior of
    # width 0.05: the chain is burnt in first.  Measured without: waic(40) from the start gives p_waic 276.4 and n_warn 129
    # (the NumPy oracle on the same streams: 285.5 and 129), after the smoke test's own 20 iterations 60.5 and 41 -- Var[l_i]
    # over the states is that of the approach, not of the posterior.  After 100 iterations the oracle gives 7.8 and 0.
    for _ in range(100):
        s.sampling_iteration()
    wa = s.waic(40)
    for a in (wa.lppd_i, wa.p_waic_i, wa.elpd_i, wa.fitted, wa.pointwise.mean, wa.pointwise.var):
        assert np.isfinite(a).all()
    assert np.isfinite([wa.elpd_waic, wa.p_waic, wa.lppd, wa.se, wa.waic]).all()
    print('logistic waic: elpd %.2f, p_waic %.3f, se %.2f, n_warn %d' % (wa.elpd_waic, wa.p_waic, wa.se, wa.n_warn))
    assert 0 < wa.p_waic < 2 * 8 and wa.n_warn == 0
    assert np.all((wa.fitted > 0) & (wa.fitted < 1)) and np.all(wa.pointwise.mean[1, 2000:] == 0.0)
