"""GPU: linear-model energies E(x) = sum_j f(u_j, j), u = W x + b (MJHMC_E_LINEAR_EXPR) on the ProductOfT tile kernels,
against NumPy restatements of the same float32 force (csrc/linear_energy.hip).

Bars: single evaluations at those of test_pot_single_evaluation_* (float32 kernel: a few 1e-6 relative); sampling
iterations as in test_pot_with_the_references_arithmetic_float64_state_float32_force -- transitions equal to the oracle's
except provable near ties (tests/helpers.py)."""
import numpy as np
import pytest
from scipy import stats

from oracle import mjhmc_oracle as orc
from tests.helpers import resync, check_iteration, check_control_iteration

pytestmark = pytest.mark.gpu
np.seterr(all='ignore')

f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)           # noqa: E731

# (energy, grad) as C expressions and as float32 NumPy functions of (u, q)
EXPRS = {
    'quadratic': ('0.5f*u*u', 'u', lambda u, q: np.float32(0.5) * u * u, lambda u, q: u),
    'softplus': ('u > 20.f ? u : log1pf(expf(u))', '1.f/(1.f + expf(-u))',
                 lambda u, q: np.where(u > 20, u, np.log1p(np.exp(np.minimum(u, 20)))),
                 lambda u, q: np.float32(1) / (np.float32(1) + np.exp(-u))),
    'product_of_t': ('q[0]*logf(1.f + u*u)', '2.f*q[0]*u/(1.f + u*u)',
                     lambda u, q: q[0][:, None] * np.log(np.float32(1) + u * u),
                     lambda u, q: np.float32(2) * q[0][:, None] * u / (np.float32(1) + u * u)),
    'l1': ('fabsf(u)', 'u/fabsf(u)', lambda u, q: np.abs(u), lambda u, q: np.sign(u)),     # f'(0) is NaN: padding masked
}


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def restated(W, b, name, q=None):
    """The float32 force of the model in NumPy: E (1, n) and dE/dX (D, n), float64 out (orc.LambdaEnergy callables)."""
    _, _, f, fp = EXPRS[name]
    W32, b32 = W.astype(np.float32), b.astype(np.float32)
    q32 = None if q is None else np.asarray(q, dtype=np.float32)

    def u_of(X):
        return W32.dot(X.astype(np.float32)) + b32[:, None]

    def E(X):
        return f(u_of(X), q32).astype(np.float64).sum(axis=0).reshape((1, -1))

    def dEdX(X):
        return W32.T.dot(fp(u_of(X), q32).astype(np.float32)).astype(np.float64)
    return E, dEdX


def model(D, K, name, seed=0):
    rs = np.random.RandomState(seed + 7 * D + K)
    W = rs.randn(K, D) / np.sqrt(D)
    b = 0.1 * rs.randn(K)
    q = (1.5 + rs.rand(1, K)) if name == 'product_of_t' else None
    return W, b, q


def dist(X0, W, b, name, q=None, state='float64'):
    from mjhmc_amd.misc.distributions import LambdaDistribution
    e, g = EXPRS[name][:2]
    return LambdaDistribution(init=X0, device_linear=dict(W=W, b=b, energy=e, grad=g, expert_params=q), state_dtype=state)


@pytest.mark.parametrize('D,K', [(36, 36), (10, 300), (300, 10), (129, 200), (512, 512)])
@pytest.mark.parametrize('name', ['quadratic', 'softplus', 'product_of_t'])
def test_single_evaluation(name, D, K):
    W, b, q = model(D, K, name)
    X = np.random.RandomState(D).randn(D, 45)
    d = dist(X, W, b, name, q)
    E, G = d.E(X), d.dEdX(X)
    Er, Gr = restated(W, b, name, q)
    assert E.shape == (1, 45) and G.shape == (D, 45)
    assert rel(E, Er(X)) < 8e-6, rel(E, Er(X))
    assert rel(G, Gr(X)) < 3.2e-5, rel(G, Gr(X))
    d32 = dist(X, W, b, name, q, state='float32')          # the float32-state kernels' evaluation
    assert rel(d32.E(X), Er(X)) < 8e-6 and rel(d32.dEdX(X), Gr(X)) < 3.2e-5


@pytest.mark.parametrize('D,K', [(36, 20), (200, 129)])
def test_padding_is_exact(D, K):
    """Padded experts contribute nothing: softplus has f(0) = log 2 (P - K of them would add (P - K) log 2), and the
    L1 expert's f'(0) = 0/0 is NaN (unmasked it would poison every dE/dX)."""
    X = np.random.RandomState(3).randn(D, 40)
    for name in ('softplus', 'l1'):
        W, b, _ = model(D, K, name, seed=5)
        d = dist(X, W, b, name)
        E, G = d.E(X), d.dEdX(X)
        Er, Gr = restated(W, b, name)
        assert np.isfinite(E).all() and np.isfinite(G).all(), name
        assert rel(E, Er(X)) < 8e-6 and rel(G, Gr(X)) < 3.2e-5, name


def _pot_as_linear(D, N):
    from tests.helpers import ref_init_weights
    Wp, lognu = ref_init_weights(D, D)
    Wp = (Wp + np.eye(D)).astype(np.float32).astype(np.float64)
    nu = np.exp(lognu).astype(np.float32).astype(np.float64)
    X0 = np.random.RandomState(5).randn(D, N)
    # u_j = (W^T x + b)_j / nu_j: W' = (W / nu)^T, q[0] = alpha = (nu + 1) / 2, f = alpha log(1 + u^2)
    d = dist(X0, (Wp / nu[None, :]).T, np.zeros(D), 'product_of_t', ((nu + 1) / 2)[None, :])
    return d, orc.ProductOfT(Wp, nu=nu, force_dtype=np.float32), X0


@pytest.mark.parametrize('cls_name', ['MarkovJumpHMC', 'ControlHMC'])
@pytest.mark.parametrize('D,N', [(36, 100), (512, 64)])
def test_product_of_t_as_linear_model_against_the_oracle(cls_name, D, N):
    """ProductOfT written as a linear-model energy, float64 state around the float32 force, against the oracle's
    ProductOfT(force_dtype=float32) on the same Philox streams."""
    from mjhmc_amd.samplers import markov_jump_hmc as M
    d, en, X0 = _pot_as_linear(D, N)
    assert rel(d.E(X0)[0], en.E_val(X0)[0]) < 4e-6 and rel(d.dEdX(X0), en.dEdX_val(X0)) < 2e-5
    kw = dict(epsilon=0.1, beta=0.3, num_leapfrog_steps=6)
    if cls_name == 'MarkovJumpHMC':
        s = M.MarkovJumpHMC(distribution=d, seed=17, resample=False, **kw)
        o = orc.MarkovJumpHMC(en, X0, resample=False, rng=orc.PhiloxRNG(17, np.arange(N)), **kw)
        resync(s, o)
        for t in range(5):
            check_iteration(s, o, delta_rel=4e-6, x_tol=1e-6, e_rtol=4e-6, tag='pot-as-linear it %d' % t)
            resync(s, o)
    else:
        s = M.ControlHMC(distribution=d, seed=17, **kw)
        o = orc.ControlHMC(en, X0, rng=orc.PhiloxRNG(17, np.arange(N)), **kw)
        for t in range(5):
            check_control_iteration(s, o, delta_rel=4e-6, x_tol=1e-6, e_rtol=4e-6, tag='pot-as-linear control it %d' % t)
            resync(s, o)
    out = s.sample(3, preserve_order=True)
    assert out.shape == (D, N, 3) and np.isfinite(out).all()


def _family_model(kind):
    if kind == 'gauss':          # correlated Gaussian, W = L^T of its precision
        from mjhmc_amd.misc.distributions import CorrelatedGaussian
        c = CorrelatedGaussian(ndims=24, nbatch=2, seed=3)
        return c.L.T.copy(), np.zeros(24), 'quadratic'
    W, b, _ = model(24, 40, 'softplus', seed=9)          # K != D
    return W, b, 'softplus'


@pytest.mark.parametrize('state', ['float64', 'float32'])
@pytest.mark.parametrize('cls_name', ['MarkovJumpHMC', 'ControlHMC', 'HMC', 'HMCBase'])
@pytest.mark.parametrize('kind', ['gauss', 'softplus'])
def test_sampler_families_against_the_oracle(kind, cls_name, state):
    from mjhmc_amd.samplers import markov_jump_hmc as M
    W, b, name = _family_model(kind)
    D, N = W.shape[1], 96
    X0 = np.random.RandomState(11).randn(D, N)
    if state == 'float32':
        X0 = f32(X0)
    d = dist(X0, W, b, name, state=state)
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
            check_iteration(s, o, tag='%s %s %s it %d' % (kind, cls_name, state, t), **tol)
        else:
            check_control_iteration(s, o, tag='%s %s %s it %d' % (kind, cls_name, state, t), **tol)
        assert (s.l_count, s.f_count, s.r_count) == (o.l_count, o.f_count, o.r_count), t
        resync(s, o)
    if cls_name == 'MarkovJumpHMC':
        dw = s._dev.read(7)
        assert np.isfinite(dw).all() and (dw > 0).all()
    out = s.sample(4, preserve_order=True)
    assert out.shape == (D, N, 4) and np.isfinite(out).all()
    assert np.array_equal(out[:, :, -1], s.state.X)


@pytest.mark.parametrize('state', ['float64', 'float32'])
def test_continuous_time_sampler_runs_on_the_linear_model(state):
    """ContinuousTimeHMC: the jump process of the dense kernels (kModeCT) on the linear model; every particle's stored
    energy is the float32 force's energy of its state."""
    from mjhmc_amd.samplers import markov_jump_hmc as M
    W, b, name = _family_model('softplus')
    X0 = np.random.RandomState(2).randn(W.shape[1], 80)
    d = dist(X0, W, b, name, state=state)
    s = M.ContinuousTimeHMC(distribution=d, seed=5, epsilon=0.2, beta=0.3, num_leapfrog_steps=5, resample=False)
    out = s.sample(6, preserve_order=True)
    assert np.isfinite(out).all() and s.fl_count + s.f_count + s.r_count > 0
    E, _ = restated(W, b, name)
    assert rel(s.state.EX, E(s.state.X)) < 2e-5


@pytest.mark.parametrize('state', ['float64', 'float32'])
def test_fused_call_equals_single_iterations_and_replay(state):
    """sample(n) in one fused call is bit for bit n sampling_iteration calls; replay mode (recorded normals and
    exponentials) follows the oracle."""
    from mjhmc_amd.samplers import markov_jump_hmc as M
    W, b, name = _family_model('softplus')
    D, N = W.shape[1], 64
    X0 = f32(np.random.RandomState(4).randn(D, N))
    kw = dict(epsilon=0.2, beta=0.3, num_leapfrog_steps=5, seed=3, resample=False)
    a = M.MarkovJumpHMC(distribution=dist(X0, W, b, name, state=state), **kw)
    c = M.MarkovJumpHMC(distribution=dist(X0, W, b, name, state=state), **kw)
    out = a.sample(6, preserve_order=True)
    for t in range(6):
        c.sampling_iteration()
        assert np.array_equal(c.state.X, out[:, :, t]), t
    assert np.array_equal(a.state.V, c.state.V) and np.array_equal(a.state.EX, c.state.EX)
    assert (a.l_count, a.f_count, a.r_count) == (c.l_count, c.f_count, c.r_count)
    # replay
    rng = np.random.RandomState(8)
    normals = [rng.randn(D, N) for _ in range(3)]
    exps = [rng.standard_exponential((3, N)) for _ in range(3)]
    en = orc.LambdaEnergy(*restated(W, b, name))
    s = M.MarkovJumpHMC(distribution=dist(X0, W, b, name, state=state), Vinit=X0[::-1].copy(), **kw)
    o = orc.MarkovJumpHMC(en, X0, V0=X0[::-1].copy(), rng=orc.ReplayRNG(normals=normals, exps=exps),
                          epsilon=0.2, beta=0.3, num_leapfrog_steps=5, resample=False,
                          **(dict(state_rounding=f32) if state == 'float32' else {}))
    for t in range(3):
        s.sampling_iteration(replay=[(normals[t], exps[t])])
        o.sampling_iteration()
        tr = s._dev.read(8)
        assert (tr == o.last_transition).mean() > 0.95, t
        resync(s, o)


@pytest.mark.parametrize('state', ['float64', 'float32'])
def test_state_operations(state):
    """Assigning the state (figures/poe_fig.py:59) re-evaluates E and dE/dX; state.copy().L() / .FLF() and a single
    leapfrog step follow the oracle's on the float32 force."""
    from mjhmc_amd.samplers import markov_jump_hmc as M
    from mjhmc_amd.samplers.hmc_state import HMCState
    W, b, name = _family_model('softplus')
    D, N = W.shape[1], 48
    X0 = np.random.RandomState(6).randn(D, N)
    s = M.MarkovJumpHMC(distribution=dist(X0, W, b, name, state=state), seed=1, epsilon=0.2, beta=0.3,
                        num_leapfrog_steps=5, resample=False)
    rnd = f32 if state == 'float32' else (lambda a: a)
    Xn = np.random.RandomState(7).randn(D, N) * 1.3
    Vn = np.random.RandomState(8).randn(D, N)
    s.state = HMCState(Xn, s, V=Vn)
    assert np.array_equal(s.state.X, rnd(Xn)) and np.array_equal(s.state.V, rnd(Vn))
    E, G = restated(W, b, name)
    assert rel(s.state.EX, E(rnd(Xn))) < 8e-6 and rel(s.state.dEdX, G(rnd(Xn))) < 3.2e-5
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


def test_correlated_gaussian_stationary_law():
    """CorrelatedGaussian (D = 64, conditioning 10^2) under MarkovJumpHMC from exact draws: the whitened samples
    L^T (x - mu) stay N(0, 1) per coordinate (KS p-values), and the chain moves."""
    from mjhmc_amd.misc.distributions import CorrelatedGaussian
    from mjhmc_amd.samplers.markov_jump_hmc import MarkovJumpHMC
    D, N = 64, 4096
    np.random.seed(2027)
    d = CorrelatedGaussian(ndims=D, nbatch=N, mean=np.linspace(-1, 1, D), seed=4)
    X_exact = d.Xinit.copy()

    def pvals(X):
        z = d.L.T.dot(X - d.mean[:, None])
        return np.array([stats.kstest(z[k], 'norm').pvalue for k in range(D)])
    assert pvals(X_exact).min() > 1e-4
    s = MarkovJumpHMC(distribution=d, epsilon=0.1, beta=0.3, num_leapfrog_steps=8, seed=13)
    for _ in range(60):
        s.sampling_iteration()
    X = s.state.X
    assert np.mean(np.abs(X - X_exact) > 1e-3) > 0.9
    p = pvals(X)
    assert p.min() > 1e-4, (p.min(), int(p.argmin()))
    assert np.median(pvals(1.3 * X)) < 1e-6            # negative control: a wider law
