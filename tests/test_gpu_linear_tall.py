"""GPU: tall linear-model energies -- E(x) = sum_{j<K} f(u_j, j), u = W x + b with more than 512 experts, D <= 512 -- on
the fused block kernel (csrc/dense_lin_tall.hpp, mjhmc_energy_create_linear_tall), against NumPy
restatements of the same float32 force, and GeneralizedLinearModel on top of it.

The patterns and the bars are tests/test_gpu_linear.py's: single evaluations rel(E) < 8e-6, rel(G) < 3.2e-5 against the
float32 restatement (which stands at <= 2e-6 / 1.8e-6 from float64 on these models, while one dropped expert moves E by
>= 5e-4); sampling iterations as in its test_sampler_families_against_the_oracle."""
import numpy as np
import pytest
from scipy import stats

from oracle import mjhmc_oracle as orc
from tests.helpers import resync, check_iteration, check_control_iteration
from tests.test_gpu_linear import EXPRS, rel, restated, model, f32

pytestmark = pytest.mark.gpu
np.seterr(all='ignore')

E_BAR, G_BAR = 8e-6, 3.2e-5


def tall(X0, W, b, name, q=None, state='float64'):
    from mjhmc_amd.misc.distributions import LambdaDistribution
    e, g = EXPRS[name][:2]
    return LambdaDistribution(init=X0, device_linear_tall=dict(W=W, b=b, energy=e, grad=g, expert_params=q), state_dtype=state)


def pad_of(D):
    return 128 if D <= 128 else (256 if D <= 256 else 512)


@pytest.mark.parametrize('D,K', [(10, 513), (129, 640), (36, 1025), (512, 1537), (300, 2049)])
@pytest.mark.parametrize('name', ['quadratic', 'softplus', 'product_of_t'])
def test_single_evaluation(name, D, K):
    W, b, q = model(D, K, name)
    X = np.random.RandomState(D).randn(D, 45)
    Er, Gr = restated(W, b, name, q)
    for state in ('float64', 'float32'):
        d = tall(X, W, b, name, q, state=state)
        E, G = d.E(X), d.dEdX(X)
        assert E.shape == (1, 45) and G.shape == (D, 45)
        print('%s %dx%d %s: rel E %.3g, rel G %.3g' % (name, D, K, state, rel(E, Er(X)), rel(G, Gr(X))))
        assert rel(E, Er(X)) < E_BAR, (state, rel(E, Er(X)))
        assert rel(G, Gr(X)) < G_BAR, (state, rel(G, Gr(X)))


@pytest.mark.parametrize('D,K', [(36, 600), (200, 1000)])
def test_padding_is_exact(D, K):
    """The experts beyond K in the last block contribute nothing: softplus has f(0) = log 2, the L1 expert's f'(0) is NaN."""
    X = np.random.RandomState(3).randn(D, 40)
    for name in ('softplus', 'l1'):
        W, b, _ = model(D, K, name, seed=5)
        d = tall(X, W, b, name)
        E, G = d.E(X), d.dEdX(X)
        Er, Gr = restated(W, b, name)
        assert np.isfinite(E).all() and np.isfinite(G).all(), name
        assert rel(E, Er(X)) < E_BAR and rel(G, Gr(X)) < G_BAR, (name, rel(E, Er(X)), rel(G, Gr(X)))


@pytest.mark.parametrize('D', [10, 300])
def test_block_boundaries_and_the_global_expert_index(D):
    """f = q[0] u^2 with q[0][j] = 1 + j / K and a W whose only non-zero row is j0: E = q[0][j0] (w.x)^2 and
    dE/dx = 2 q[0][j0] (w.x) w -- the expert's own q entry (the global index, across block boundaries) or nothing fits.
    The row touches the even coordinates only: dE/dX is exactly 0 in the odd ones."""
    from mjhmc_amd.misc.distributions import LambdaDistribution
    K, P = 1100, pad_of(D)
    X = np.random.RandomState(D).randn(D, 45)
    q0 = 1.0 + np.arange(K) / K
    w = np.random.RandomState(1).randn(D)
    w[1::2] = 0.0
    w32, q32, X32 = f32(w), f32(q0), f32(X)
    for j0 in (0, P - 1, P, 2 * P - 1, 2 * P, K - 1):
        W = np.zeros((K, D))
        W[j0] = w
        for state in ('float64', 'float32'):
            d = LambdaDistribution(init=X, device_linear_tall=dict(W=W, b=None, energy='q[0]*u*u', grad='2.f*q[0]*u',
                                                                   expert_params=q0[None, :]), state_dtype=state)
            E, G = d.E(X), d.dEdX(X)
            u = w32.dot(X32)
            assert rel(E[0], q32[j0] * u * u) < E_BAR, (j0, state, rel(E[0], q32[j0] * u * u))
            assert rel(G, 2 * q32[j0] * w32[:, None] * u[None, :]) < G_BAR, (j0, state)
            assert np.all(G[1::2] == 0.0), (j0, state)


@pytest.mark.parametrize('D,K', [(36, 36), (129, 200)])
def test_consistency_with_the_tile_path(D, K):
    """K <= 512 is legal on the tall entry point and is one block there: the pad of D equals the pad of max(D, K) for these
    models, so the block is the tile path's model -- the same two GEMMs on the same operands, the same masked terms, the
    same order of sums (0 + the block's lane sum, the lane halves, the four waves), with contraction off in both compiles.
    Bit-identical by construction; asserted."""
    from tests.test_gpu_linear import dist
    W, b, q = model(D, K, 'softplus')
    X = np.random.RandomState(D).randn(D, 45)
    a, t = dist(X, W, b, 'softplus', q), tall(X, W, b, 'softplus', q)
    Ea, Ga, Et, Gt = a.E(X), a.dEdX(X), t.E(X), t.dEdX(X)
    assert rel(Et, Ea) < E_BAR and rel(Gt, Ga) < G_BAR
    assert np.array_equal(Et, Ea) and np.array_equal(Gt, Ga)


def test_determinism_and_independence_of_the_grid():
    D, K = 512, 1537
    W, b, _ = model(D, K, 'softplus')
    X = np.random.RandomState(2).randn(D, 4000)
    d = tall(X[:, :45], W, b, 'softplus')
    E1, G1 = d.E(X[:, :45]), d.dEdX(X[:, :45])
    E2, G2 = d.E(X[:, :45]), d.dEdX(X[:, :45])
    assert np.array_equal(E1, E2) and np.array_equal(G1, G2)
    Eb1, Gb1 = d.E(X), d.dEdX(X)                # 125 tiles: another grid
    Eb2, Gb2 = d.E(X), d.dEdX(X)
    assert np.array_equal(Eb1, Eb2) and np.array_equal(Gb1, Gb2)
    assert np.array_equal(Eb1[:, :45], E1) and np.array_equal(Gb1[:, :45], G1)


FAMILY = (24, 700)      # a softplus model, K != a multiple of the block (128): 6 blocks, the last with 60 experts


def _family():
    W, b, _ = model(FAMILY[0], FAMILY[1], 'softplus', seed=9)
    return W, b, 'softplus'


@pytest.mark.parametrize('state', ['float64', 'float32'])
@pytest.mark.parametrize('cls_name', ['MarkovJumpHMC', 'ControlHMC', 'HMC', 'HMCBase'])
def test_sampler_families_against_the_oracle(cls_name, state):
    from mjhmc_amd.samplers import markov_jump_hmc as M
    W, b, name = _family()
    D, N = W.shape[1], 96
    X0 = np.random.RandomState(11).randn(D, N)
    if state == 'float32':
        X0 = f32(X0)
    d = tall(X0, W, b, name, state=state)
    en = orc.LambdaEnergy(*restated(W, b, name))
    kw = dict(epsilon=0.2, beta=0.3, num_leapfrog_steps=5)
    okw = dict(state_rounding=f32) if state == 'float32' else {}
    tol = dict(delta_rel=4e-6, x_tol=1e-6, e_rtol=4e-6) if state == 'float64' else dict(delta_rel=2e-5, x_tol=2e-5, e_rtol=2e-5)
    extra = dict(resample=False) if cls_name == 'MarkovJumpHMC' else {}
    s = getattr(M, cls_name)(distribution=d, seed=23, **kw, **extra)
    o = getattr(orc, cls_name)(en, X0, rng=orc.PhiloxRNG(23, np.arange(N)), **kw, **dict(extra, **okw))
    resync(s, o)
    for t in range(5):
        if cls_name == 'MarkovJumpHMC':
            check_iteration(s, o, tag='tall %s %s it %d' % (cls_name, state, t), **tol)
        else:
            check_control_iteration(s, o, tag='tall %s %s it %d' % (cls_name, state, t), **tol)
        assert (s.l_count, s.f_count, s.r_count) == (o.l_count, o.f_count, o.r_count), t
        resync(s, o)
    out = s.sample(4, preserve_order=True)
    assert out.shape == (D, N, 4) and np.isfinite(out).all()
    assert np.array_equal(out[:, :, -1], s.state.X)


@pytest.mark.parametrize('state', ['float64', 'float32'])
def test_continuous_time_sampler_runs_on_the_tall_model(state):
    from mjhmc_amd.samplers import markov_jump_hmc as M
    W, b, name = _family()
    X0 = np.random.RandomState(2).randn(W.shape[1], 80)
    s = M.ContinuousTimeHMC(distribution=tall(X0, W, b, name, state=state), seed=5, epsilon=0.2, beta=0.3,
                            num_leapfrog_steps=5, resample=False)
    out = s.sample(6, preserve_order=True)
    assert np.isfinite(out).all() and s.fl_count + s.f_count + s.r_count > 0
    E, _ = restated(W, b, name)
    assert rel(s.state.EX, E(s.state.X)) < 2e-5


@pytest.mark.parametrize('state', ['float64', 'float32'])
def test_fused_call_equals_single_iterations(state):
    from mjhmc_amd.samplers import markov_jump_hmc as M
    W, b, name = _family()
    D, N = W.shape[1], 64
    X0 = f32(np.random.RandomState(4).randn(D, N))
    kw = dict(epsilon=0.2, beta=0.3, num_leapfrog_steps=5, seed=3, resample=False)
    a = M.MarkovJumpHMC(distribution=tall(X0, W, b, name, state=state), **kw)
    c = M.MarkovJumpHMC(distribution=tall(X0, W, b, name, state=state), **kw)
    out = a.sample(6, preserve_order=True)
    for t in range(6):
        c.sampling_iteration()
        assert np.array_equal(c.state.X, out[:, :, t]), t
    assert np.array_equal(a.state.V, c.state.V) and np.array_equal(a.state.EX, c.state.EX)
    assert (a.l_count, a.f_count, a.r_count) == (c.l_count, c.f_count, c.r_count)


@pytest.mark.parametrize('state', ['float64', 'float32'])
def test_state_operations(state):
    from mjhmc_amd.samplers import markov_jump_hmc as M
    from mjhmc_amd.samplers.hmc_state import HMCState
    W, b, name = _family()
    D, N = W.shape[1], 48
    X0 = np.random.RandomState(6).randn(D, N)
    s = M.MarkovJumpHMC(distribution=tall(X0, W, b, name, state=state), seed=1, epsilon=0.2, beta=0.3,
                        num_leapfrog_steps=5, resample=False)
    rnd = f32 if state == 'float32' else (lambda a: a)
    Xn = np.random.RandomState(7).randn(D, N) * 1.3
    Vn = np.random.RandomState(8).randn(D, N)
    s.state = HMCState(Xn, s, V=Vn)
    assert np.array_equal(s.state.X, rnd(Xn)) and np.array_equal(s.state.V, rnd(Vn))
    E, G = restated(W, b, name)
    assert rel(s.state.EX, E(rnd(Xn))) < E_BAR and rel(s.state.dEdX, G(rnd(Xn))) < G_BAR
    o = orc.MarkovJumpHMC(orc.LambdaEnergy(E, G), rnd(Xn), epsilon=0.2, beta=0.3, num_leapfrog_steps=5, V0=rnd(Vn),
                          resample=False, rng=orc.ReplayRNG())
    for op in ('L', 'FLF'):
        Z = getattr(s.state.copy(), op)()
        Zo = getattr(o.state.clone(), op)()
        assert rel(Z.X, Zo.X) < 2e-5 and rel(Z.V, Zo.V) < 2e-5, op
        assert rel(Z.EX, Zo.EX) < 2e-5 and rel(Z.EV, Zo.EV) < 2e-5 and rel(Z.dEdX, Zo.dEdX) < 5e-5, op
    Z1 = s.state.copy()
    Z1.leapfrog()
    o1 = o.state.clone()
    o1.leap()
    assert rel(Z1.X, o1.X) < 2e-5 and rel(Z1.V, o1.V) < 2e-5


@pytest.mark.parametrize('state', ['float64', 'float32'])
def test_rollback_restores_the_state(state):
    from mjhmc_amd import engine, _lib
    W, b, name = _family()
    e, g = EXPRS[name][:2]
    en = engine.DeviceEnergy.from_linear_tall(engine.context(0), W, b, e, g)
    s = engine.DeviceSampler(en, np.random.RandomState(3).randn(W.shape[1], 100), seed=5, dtype=state)
    s.set_hparams(0.2, 5, 0.3, 1.0)
    s.iterate(2)
    fields = [_lib.F_X, _lib.F_V, _lib.F_EX, _lib.F_EV, _lib.F_DEDX]
    before = [s.read(f) for f in fields]
    _, done = s.iterate(1)
    assert done == 1
    assert not np.array_equal(before[0], s.read(_lib.F_X))
    s.rollback()
    for a, f in zip(before, fields):
        assert np.array_equal(a, s.read(f), equal_nan=True), f
    s.close()


# ---------------------------------------------------------------------------------------------------------------------
# GeneralizedLinearModel
# ---------------------------------------------------------------------------------------------------------------------
GLM_N = 4096


@pytest.fixture(scope='module')
def gauss_glm():
    """n = 1500 rows, D = 6 (K = 1506, 12 blocks of 128), started from exact posterior draws; (model, mean, cov, Lc, eps)"""
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
    precision = np.linalg.inv(cov)
    eps = 0.5 / np.sqrt(np.linalg.eigvalsh(precision).max())
    return d, mean, cov, np.linalg.cholesky(precision), eps


def test_gaussian_glm_evaluates_its_own_energy(gauss_glm):
    d = gauss_glm[0]
    assert d.device_energy()[1]['tall']
    X = d.Xinit[:, :64]
    assert rel(d.E(X), d.E_host(X)) < 1e-4 and rel(d.dEdX(X), d.dEdX_host(X)) < 1e-4


def test_gaussian_glm_stationary_law(gauss_glm):
    from mjhmc_amd.samplers.markov_jump_hmc import MarkovJumpHMC
    d, mean, cov, Lc, eps = gauss_glm
    X_exact = d.Xinit.copy()

    def white(X):
        return Lc.T.dot(X - mean[:, None])

    def pvals(Z):
        return np.array([stats.kstest(Z[k], 'norm').pvalue for k in range(Z.shape[0])])
    assert pvals(white(X_exact)).min() > 1e-4
    s = MarkovJumpHMC(distribution=d, epsilon=eps, beta=0.3, num_leapfrog_steps=8, seed=13)
    for _ in range(60):
        s.sampling_iteration()
    Z = white(s.state.X)
    assert np.mean(np.abs(Z - white(X_exact)).max(axis=0) > 1e-3) > 0.9
    p = pvals(Z)
    assert p.min() > 1e-4, (p.min(), int(p.argmin()))
    assert np.median(pvals(1.3 * Z)) < 1e-6            # negative control: a wider law


def test_the_rest_of_the_stack_runs_on_the_tall_model(gauss_glm):
    from mjhmc_amd import _lib
    from mjhmc_amd.samplers.markov_jump_hmc import MarkovJumpHMC
    d, mean, cov, Lc, eps = gauss_glm
    s = MarkovJumpHMC(distribution=d, epsilon=eps, beta=0.3, num_leapfrog_steps=8, seed=17, resample=False)
    ex = s.expectations(40)
    dg = s.diagnostics(40)                       # the continuing run: its multi-chain ESS prices the pooled mean
    se = np.sqrt(ex.var / dg.ess)
    z = (ex.mean - mean) / se
    print('tall GLM: mean %s, posterior %s, se %s, z %s, rhat %s' % (ex.mean, mean, se, z, dg.rhat))
    assert np.all(np.isfinite(z)) and np.all(np.abs(z) <= 5.0), z
    t = s.temperature(40)
    print('tall GLM: T = %.6f, stderr %.6f, z = %.3f' % (t.T, t.stderr, t.z))
    assert np.isfinite(t.T) and t.stderr > 0 and abs(t.T - 1) <= 5 * t.stderr, (t.T, t.stderr)
    with pytest.raises(_lib.EngineError, match='multi-pass'):
        s.cv_expectations(4)


def test_logistic_regression_smoke():
    from mjhmc_amd.misc.distributions import GeneralizedLinearModel
    from mjhmc_amd.samplers.markov_jump_hmc import MarkovJumpHMC
    rs = np.random.RandomState(7)
    A = rs.randn(2000, 8)
    y = (rs.rand(2000) < 1 / (1 + np.exp(-A.dot(rs.randn(8))))).astype(float)
    d = GeneralizedLinearModel(A, y, 'logistic', nbatch=256, seed=3)
    s = MarkovJumpHMC(distribution=d, epsilon=0.01, beta=0.3, num_leapfrog_steps=8, seed=4, resample=False)
    for _ in range(20):
        s.sampling_iteration()
    assert np.isfinite(s.state.X).all() and np.isfinite(s.state.EX).all()
    assert rel(s.state.EX, d.E_host(s.state.X)) < 1e-4
