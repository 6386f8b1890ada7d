"""GPU: grouped linear-model energies -- E(x) = sum_{j<K} f(u_j, j) + sum_{g<G} LSE_{c<C} u_{gC+c}, u = W x + b (softmax
regression) -- on the fused kernel of csrc/dense_lin_grouped.hpp (mjhmc_energy_create_linear_grouped),
against a float32 NumPy restatement, and MultinomialLogisticRegression on top of it.

The oracle is tests/test_gpu_linear.py::restated's style: W32 @ X32 + b32 in float32, the group term in float32 in the
stated order (m = max over c ascending, t_c = exp(u_c - m), s = t_0 + ... ascending, m + log(s), t_c / s), every term
widened to float64 and summed.  The bars are the project's own for this class of operations (tests/test_gpu_linear.py,
tests/test_gpu_linear_tall.py): rel(E) < 8e-6, rel(G) < 3.2e-5.  Every model also asserts on the CPU that leaving out one
group's term and exchanging one member between two neighbouring groups move the restated E or G by >= 10 x the bar."""
import numpy as np
import pytest

from oracle import mjhmc_oracle as orc
from tests.helpers import resync, check_iteration, check_control_iteration
from tests.test_gpu_linear import rel, f32

pytestmark = pytest.mark.gpu
np.seterr(all='ignore')

E_BAR, G_BAR = 8e-6, 3.2e-5
N = 45                      # two tiles of 32 particles, the second partial
one, half = np.float32(1), np.float32(0.5)

# grouped experts (q[1] = 1): f = -q[0] u; plain experts (q[1] = 0): the named f
PLAIN = {
    'quadratic': ('0.5f*u*u', 'u', lambda u: half * u * u, lambda u: u),
    'l1': ('fabsf(u)', 'u/fabsf(u)', lambda u: np.abs(u), lambda u: np.sign(u)),          # f'(0) is NaN: padding masked
}


def exprs(plain='quadratic'):
    e, g = PLAIN[plain][:2]
    return 'q[1] != 0.f ? -q[0]*u : (%s)' % e, 'q[1] != 0.f ? -q[0] : (%s)' % g


def pad_of(D):
    return 128 if D <= 128 else (256 if D <= 256 else 512)


def lane_groups(D, C):
    return 16 * (pad_of(D) // 128) // C


def model(D, C, G, plain, seed=0, onehot=True):
    """W (K, D), b (K,), q (2, K): G groups of C experts with a random one-hot q[0] (or none), then `plain` experts"""
    rs = np.random.RandomState(seed + 7 * D + 131 * C + G)
    K = G * C + plain
    W = rs.randn(K, D) / np.sqrt(D)
    b = 0.1 * rs.randn(K)
    q = np.zeros((2, K))
    if onehot:
        q[0, np.arange(G) * C + rs.randint(0, C, size=G)] = 1.0
    q[1, :G * C] = 1.0
    return W, b, q


def restated(W, b, q, C, G, plain='quadratic', skip_group=None, exchange=None):
    """The float32 force in NumPy: E (1, n) and dE/dX (D, n), float64 out.  ``skip_group``: that group's LSE term and
    softmax left out; ``exchange``: g -- the last member of group g and the first of group g + 1 trade groups."""
    f, fp = PLAIN[plain][2:]
    W32, b32, q32 = W.astype(np.float32), b.astype(np.float32), q.astype(np.float32)
    GC = G * C
    member = np.arange(GC)
    if exchange is not None:
        member[[exchange * C + C - 1, (exchange + 1) * C]] = member[[(exchange + 1) * C, exchange * C + C - 1]]
    live = np.ones(G, dtype=bool)
    if skip_group is not None:
        live[skip_group] = False

    def parts(X):
        u = W32.dot(X.astype(np.float32)) + b32[:, None]
        n = u.shape[1]
        ug = u[member].reshape(G, C, n)
        m = ug[:, 0]
        for c in range(1, C):
            m = np.maximum(m, ug[:, c])
        t = np.exp(ug - m[:, None, :])
        s = t[:, 0]
        for c in range(1, C):
            s = s + t[:, c]
        lse = m + np.log(s)
        soft = (t / s[:, None, :]) * live[:, None, None].astype(np.float32)
        own = np.where(q32[1][:, None] != 0, -q32[0][:, None] * u, f(u)).astype(np.float32)
        down = np.where(q32[1][:, None] != 0, -q32[0][:, None] * np.ones_like(u), fp(u)).astype(np.float32)
        phi = down.copy()
        phi[member] = phi[member] + soft.reshape(GC, n)
        assert lse.dtype == np.float32 and phi.dtype == np.float32 and own.dtype == np.float32
        return own, lse[live], phi

    def E(X):
        own, lse, _ = parts(X)
        return (own.astype(np.float64).sum(axis=0) + lse.astype(np.float64).sum(axis=0)).reshape((1, -1))

    def dEdX(X):
        return W32.T.dot(parts(X)[2]).astype(np.float64)
    return E, dEdX


def assert_the_bars_discriminate(W, b, q, C, G, X, plain='quadratic'):
    """CPU: one group's term left out, and one member exchanged between neighbouring groups, move the restatement by at
    least 10 x its bar"""
    Er, Gr = restated(W, b, q, C, G, plain)
    E0, G0 = Er(X), Gr(X)
    g = G // 2
    Es, Gs = restated(W, b, q, C, G, plain, skip_group=g)
    assert rel(Es(X), E0) >= 10 * E_BAR or rel(Gs(X), G0) >= 10 * G_BAR, (rel(Es(X), E0), rel(Gs(X), G0))
    Ex, Gx = restated(W, b, q, C, G, plain, exchange=min(g, G - 2))
    assert rel(Ex(X), E0) >= 10 * E_BAR or rel(Gx(X), G0) >= 10 * G_BAR, (rel(Ex(X), E0), rel(Gx(X), G0))


def dist(X0, W, b, q, C, G, plain='quadratic', state='float64'):
    from mjhmc_amd.misc.distributions import LambdaDistribution
    e, g = exprs(plain)
    return LambdaDistribution(init=X0, device_linear_grouped=dict(W=W, b=b, groups=(C, G), energy=e, grad=g, expert_params=q),
                              state_dtype=state)


def check_evaluation(W, b, q, C, G, X, plain='quadratic', tag=''):
    Er, Gr = restated(W, b, q, C, G, plain)
    E0, G0 = Er(X), Gr(X)
    for state in ('float64', 'float32'):
        d = dist(X, W, b, q, C, G, plain, state)
        E, Gd = d.E(X), d.dEdX(X)
        assert E.shape == (1, X.shape[1]) and Gd.shape == X.shape
        print('%s %s: rel E %.3g, rel G %.3g' % (tag, state, rel(E, E0), rel(Gd, G0)))
        assert np.isfinite(E).all() and np.isfinite(Gd).all(), (tag, state)
        assert rel(E, E0) < E_BAR, (tag, state, rel(E, E0))
        assert rel(Gd, G0) < G_BAR, (tag, state, rel(Gd, G0))


@pytest.mark.parametrize('D,C', [(10, 2), (10, 3), (10, 10), (10, 16), (129, 5), (129, 10), (300, 3), (300, 16)])
def test_single_evaluation(D, C):
    """G = 8 Gl + 1 (one group into the second grouped block) and 3 * 8 Gl - 2, with 0, 7 and P + 3 plain quadratic
    experts behind the groups; both state dtypes"""
    Gl, P = lane_groups(D, C), pad_of(D)
    X = np.random.RandomState(D).randn(D, N)
    for G in (8 * Gl + 1, 3 * 8 * Gl - 2):
        for plain in (0, 7, P + 3):
            W, b, q = model(D, C, G, plain)
            assert_the_bars_discriminate(W, b, q, C, G, X)
            check_evaluation(W, b, q, C, G, X, tag='%dx%d G=%d plain=%d' % (D, C, G, plain))


@pytest.mark.parametrize('D,C', [(10, 3), (300, 5)])
def test_group_boundaries(D, C):
    """f = 0 on the grouped experts, so E = sum_g LSE_g + the plain terms: t added to b of every member of group g raises
    E by t and leaves the softmax, hence dE/dX, alone -- for the first and last group of a lane type, of a block and of the
    model.  A window of C experts shifted by one is not a group: the restatement's dE/dX moves by > 10 x the bar."""
    Gl, t = lane_groups(D, C), 0.75
    G = 2 * 8 * Gl + 3
    W, b, q = model(D, C, G, 7, seed=3, onehot=False)
    X = np.random.RandomState(D + 1).randn(D, N)
    Er, Gr = restated(W, b, q, C, G)
    E0, G0 = Er(X), Gr(X)
    assert_the_bars_discriminate(W, b, q, C, G, X)
    for g in (0, Gl - 1, Gl, 8 * Gl - 1, 8 * Gl, G - 1):
        bs = b.copy()
        bs[g * C:(g + 1) * C] += t
        off = 1 if g < G - 1 else -1
        bw = b.copy()
        bw[g * C + off:(g + 1) * C + off] += t
        assert rel(restated(W, bw, q, C, G)[1](X), G0) > 10 * G_BAR, g
        for state in ('float64', 'float32'):
            d = dist(X, W, bs, q, C, G, state=state)
            E, Gd = d.E(X), d.dEdX(X)
            assert rel(E, E0 + t) < E_BAR, (g, state, rel(E, E0 + t))
            assert rel(Gd, G0) < G_BAR, (g, state, rel(Gd, G0))


def test_masking():
    """A last grouped block that is mostly empty (C = 10: one group per lane type, 8 per block; G = 9 leaves 7 of the
    second block's 8 groups and 6 of every lane's 16 slots empty): an unmasked empty group would add log C to E.  L1 plain
    experts behind the groups have f'(0) = NaN in their padding."""
    D, C, G = 36, 10, 9
    X = np.random.RandomState(3).randn(D, N)
    for plain, kind in ((0, 'quadratic'), (5, 'l1')):
        W, b, q = model(D, C, G, plain, seed=5)
        assert_the_bars_discriminate(W, b, q, C, G, X, kind)
        Er = restated(W, b, q, C, G, kind)[0]
        assert 7 * np.log(C) > 10 * E_BAR * np.abs(Er(X)).max()
        check_evaluation(W, b, q, C, G, X, kind, tag='masking plain=%d %s' % (plain, kind))


def test_range():
    """b puts members of some groups at +-200: expf(u) alone would overflow (expf(89) = inf), the shifted form does not"""
    D, C, G = 129, 5, 8 * lane_groups(129, 5) + 3
    W, b, q = model(D, C, G, 7, seed=2)
    rs = np.random.RandomState(8)
    far = rs.choice(G * C, size=40, replace=False)
    b[far] += np.where(rs.rand(40) < 0.5, 200.0, -200.0)
    X = np.random.RandomState(4).randn(D, N)
    u = W.dot(X) + b[:, None]
    assert u.max() > 190 and u.min() < -190 and not np.isfinite(np.exp(u.astype(np.float32))).all()
    assert_the_bars_discriminate(W, b, q, C, G, X)
    check_evaluation(W, b, q, C, G, X, tag='range')


def test_determinism_and_independence_of_the_grid():
    D, C = 300, 5
    G = 3 * 8 * lane_groups(D, C) - 2
    W, b, q = model(D, C, G, 515)
    X = np.random.RandomState(2).randn(D, 4000)
    d = dist(X[:, :N], W, b, q, C, G)
    E1, G1 = d.E(X[:, :N]), d.dEdX(X[:, :N])
    E2, G2 = d.E(X[:, :N]), d.dEdX(X[:, :N])
    assert np.array_equal(E1, E2) and np.array_equal(G1, G2)
    Eb1, Gb1 = d.E(X), d.dEdX(X)                # 125 tiles: another grid
    Eb2, Gb2 = d.E(X), d.dEdX(X)
    assert np.array_equal(Eb1, Eb2) and np.array_equal(Gb1, Gb2)
    assert np.array_equal(Eb1[:, :N], E1) and np.array_equal(Gb1[:, :N], G1)


FAMILY = (24, 5, 130, 24)      # D, C, G, plain: Gl = 3, 24 groups per block: 6 grouped blocks (the last with 10 groups) + 1 plain


@pytest.fixture(scope='module')
def family():
    D, C, G, plain = FAMILY
    W, b, q = model(D, C, G, plain, seed=9)
    assert_the_bars_discriminate(W, b, q, C, G, np.random.RandomState(1).randn(D, N))
    return W, b, q, C, G


@pytest.mark.parametrize('state', ['float64', 'float32'])
@pytest.mark.parametrize('cls_name', ['MarkovJumpHMC', 'ControlHMC', 'HMC', 'HMCBase'])
def test_sampler_families_against_the_oracle(family, cls_name, state):
    from mjhmc_amd.samplers import markov_jump_hmc as M
    W, b, q, C, G = family
    D, n = W.shape[1], 96
    X0 = np.random.RandomState(11).randn(D, n)
    if state == 'float32':
        X0 = f32(X0)
    d = dist(X0, W, b, q, C, G, state=state)
    en = orc.LambdaEnergy(*restated(W, b, q, C, G))
    kw = dict(epsilon=0.2, beta=0.3, num_leapfrog_steps=5)
    okw = dict(state_rounding=f32) if state == 'float32' else {}
    tol = dict(delta_rel=4e-6, x_tol=1e-6, e_rtol=4e-6) if state == 'float64' else dict(delta_rel=2e-5, x_tol=2e-5, e_rtol=2e-5)
    extra = dict(resample=False) if cls_name == 'MarkovJumpHMC' else {}
    s = getattr(M, cls_name)(distribution=d, seed=23, **kw, **extra)
    o = getattr(orc, cls_name)(en, X0, rng=orc.PhiloxRNG(23, np.arange(n)), **kw, **dict(extra, **okw))
    resync(s, o)
    for t in range(5):
        if cls_name == 'MarkovJumpHMC':
            check_iteration(s, o, tag='grouped %s %s it %d' % (cls_name, state, t), **tol)
        else:
            check_control_iteration(s, o, tag='grouped %s %s it %d' % (cls_name, state, t), **tol)
        assert (s.l_count, s.f_count, s.r_count) == (o.l_count, o.f_count, o.r_count), t
        resync(s, o)


@pytest.mark.parametrize('state', ['float64', 'float32'])
def test_fused_call_equals_single_iterations(family, state):
    from mjhmc_amd.samplers import markov_jump_hmc as M
    W, b, q, C, G = family
    D, n = W.shape[1], 64
    X0 = f32(np.random.RandomState(4).randn(D, n))
    kw = dict(epsilon=0.2, beta=0.3, num_leapfrog_steps=5, seed=3, resample=False)
    a = M.MarkovJumpHMC(distribution=dist(X0, W, b, q, C, G, state=state), **kw)
    c = M.MarkovJumpHMC(distribution=dist(X0, W, b, q, C, G, state=state), **kw)
    out = a.sample(6, preserve_order=True)
    for t in range(6):
        c.sampling_iteration()
        assert np.array_equal(c.state.X, out[:, :, t]), t
    assert np.array_equal(a.state.V, c.state.V) and np.array_equal(a.state.EX, c.state.EX)
    assert (a.l_count, a.f_count, a.r_count) == (c.l_count, c.f_count, c.r_count)


@pytest.mark.parametrize('state', ['float64', 'float32'])
def test_rollback_restores_the_state(family, state):
    from mjhmc_amd import engine, _lib
    W, b, q, C, G = family
    e, g = exprs()
    en = engine.DeviceEnergy.from_linear_grouped(engine.context(0), W, b, (C, G), e, g, expert_params=q)
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
# MultinomialLogisticRegression
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def mlr():
    """n = 300 rows, F = 4, C = 3 (K = 912: 8 grouped blocks of 40 groups, one plain block), 512 chains; (model, eps)"""
    from mjhmc_amd.misc.distributions import MultinomialLogisticRegression
    rs = np.random.RandomState(2031)
    A = rs.randn(300, 4)
    logits = A.dot(rs.randn(4, 3))
    y = np.array([rs.choice(3, p=np.exp(l - l.max()) / np.exp(l - l.max()).sum()) for l in logits])
    d = MultinomialLogisticRegression(A, y, 3, nbatch=512, seed=5)
    # the Hessian of the data term is at most (1/2) A^T A per class block (softmax covariance <= 1/2), plus the prior's 1
    eps = 0.5 / np.sqrt(0.5 * np.linalg.eigvalsh(A.T.dot(A)).max() + 1.0)
    return d, eps


def test_mlr_evaluates_its_own_energy(mlr):
    d = mlr[0]
    assert d.device_energy()[1]['groups'] == (3, 300)
    X = d.Xinit[:, :64]
    assert rel(d.E(X), d.E_host(X)) < 1e-4 and rel(d.dEdX(X), d.dEdX_host(X)) < 1e-4


def test_mlr_sampler_keeps_the_law_and_the_stack_runs(mlr):
    """After burn-in the virial thermometer reads |T - 1| < 6 stderr: T = E[x . dE/dX] / ndims is 1 for the law exp(-E) of
    the energy whose gradient the sampler integrates -- a gradient that is not grad E, or another law, fails it.  6: the
    project's bar for statistics with exact standard errors (tests/test_gpu_marginals.py, test_gpu_pointwise.py), a
    two-sided normal tail of 2e-9."""
    from mjhmc_amd.samplers.markov_jump_hmc import MarkovJumpHMC
    d, eps = mlr
    D = d.ndims
    s = MarkovJumpHMC(distribution=d, epsilon=eps, beta=0.3, num_leapfrog_steps=10, seed=13, resample=False)
    for _ in range(150):
        s.sampling_iteration()
    assert np.isfinite(s.state.X).all() and rel(s.state.EX, d.E_host(s.state.X)) < 1e-4
    t = s.temperature(40)
    print('MLR: T = %.6f, stderr %.6f, z = %.3f, rhat(E) %.4f' % (t.T, t.stderr, t.z, t.rhat_energy))
    assert np.isfinite(t.T) and t.stderr > 0 and abs(t.T - 1) < 6 * t.stderr, (t.T, t.stderr)
    # the power of the statement: Var(x . dE/dX) = 2 ndims for a Gaussian-like posterior, so 512 independent chains alone
    # give 6 stderr <= 6 sqrt(2 / (12 * 512)) = 0.108; a chain 15 % off is seen
    assert 6 * t.stderr < 0.15
    ex = s.expectations(20)
    assert ex.mean.shape == (D,) and np.isfinite(ex.mean).all() and np.isfinite(ex.var).all()
    dg = s.diagnostics(20)
    assert dg.rhat.shape == (D,) and np.isfinite(dg.rhat).all() and np.isfinite(dg.ess).all()
    mg = s.marginals(20, bins=64)
    med = np.asarray(mg.median).reshape(-1)
    assert med.shape == (D,) and np.isfinite(med).all()
    A_new = np.random.RandomState(6).randn(5, 4)
    P = s.projections(np.kron(np.eye(3), A_new), link=None)      # the 3 x 5 logits of five new rows
    px = s.expectations(20, of=P)
    assert px.mean.shape == (15,) and np.isfinite(px.mean).all()
    proba = d.predict_proba(s.state.X, A_new)
    assert proba.shape == (5, 3, 512) and np.allclose(proba.sum(axis=1), 1.0)


def test_refusals(mlr):
    from mjhmc_amd.samplers.markov_jump_hmc import MarkovJumpHMC
    from mjhmc_amd import _lib
    d, eps = mlr
    s = MarkovJumpHMC(distribution=d, epsilon=eps, beta=0.3, num_leapfrog_steps=5, seed=2, resample=False)
    for call in (lambda: s.pointwise(4, values=['u']), lambda: s.waic(4), lambda: s.influence(4, value='u'),
                 lambda: s.cv_expectations(60)):
        with pytest.raises(ValueError, match='grouped linear model'):
            call()
    s._dev.ring_alloc(4)
    for make in (lambda: s._dev.pointwise(['u'], [False]), lambda: s._dev.influence('u', (0, 4))):
        with pytest.raises(_lib.EngineError, match='grouped linear model'):
            make()
