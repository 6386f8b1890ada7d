"""GPU: wide linear-model energies -- E(x) = sum_{j<K} f(u_j, j), u = W x + b with more than 512 dims, D <= 4096 -- on
the fused kernel over blocks of 512 experts x chunks of 512 dims (csrc/dense_lin_wide.hpp,
mjhmc_energy_create_linear_wide), against NumPy restatements of the same float32 force, and
GeneralizedLinearModel beyond 512 features on top of it.

Bars.  tests/test_gpu_linear_tall.py's E_BAR = 8e-6 and G_BAR = 3.2e-5 against the float32 NumPy restatement are four times
the 2e-6 / 1.8e-6 that restatement itself stands from float64 on the tall file's models.  The sums are up to three times as
long here, so per shape the bar is max(the tall bar, 4 x the distance between the float32 restatement and float64 NumPy on
that shape) -- both are references, computed on the CPU, neither is the code under test (reference()).  The control at the end
of the file shows what such a bar still sees: one dropped expert or one zeroed dim chunk moves E by more than 10 bars."""
import numpy as np
import pytest

from oracle import mjhmc_oracle as orc
from tests.helpers import resync, check_iteration, check_control_iteration
from tests.test_gpu_linear import EXPRS, rel, restated, model, f32

np.seterr(all='ignore')
gpu = pytest.mark.gpu

E_BAR, G_BAR = 8e-6, 3.2e-5      # tests/test_gpu_linear_tall.py


def restated64(W, b, name, q=None):
    """The same force in float64 NumPy: the second reference the bars are taken from"""
    _, _, f, fp = EXPRS[name]
    q64 = None if q is None else np.asarray(q, dtype=np.float64)

    def E(X):
        return np.asarray(f(W.dot(X) + b[:, None], q64), dtype=np.float64).sum(axis=0).reshape((1, -1))

    def dEdX(X):
        return W.T.dot(np.asarray(fp(W.dot(X) + b[:, None], q64), dtype=np.float64))
    return E, dEdX


_REF = {}


def reference(D, K, name, n=45, seed=0):
    """(W, b, q, X, Er(X), Gr(X), e_bar, g_bar) of model(D, K, name): computed once per process, handed out read-only"""
    key = (D, K, name, n, seed)
    if key not in _REF:
        W, b, q = model(D, K, name, seed=seed)
        X = np.random.RandomState(D).randn(D, n)
        Er, Gr = restated(W, b, name, q)
        E64, G64 = restated64(W, b, name, q)
        E32, G32 = Er(X), Gr(X)
        e_bar, g_bar = max(E_BAR, 4 * rel(E32, E64(X))), max(G_BAR, 4 * rel(G32, G64(X)))
        for a in (W, b, X, E32, G32) + (() if q is None else (q,)):
            a.setflags(write=False)
        _REF[key] = (W, b, q, X, E32, G32, e_bar, g_bar)
    return _REF[key]


def wide(X0, W, b, name, q=None, state='float64'):
    from mjhmc_amd.misc.distributions import LambdaDistribution
    e, g = EXPRS[name][:2]
    return LambdaDistribution(init=X0, device_linear_wide=dict(W=W, b=b, energy=e, grad=g, expert_params=q), state_dtype=state)


@gpu
@pytest.mark.parametrize('D,K', [(513, 40), (1000, 513), (1025, 1100), (1536, 700)])
@pytest.mark.parametrize('name', ['quadratic', 'softplus', 'product_of_t'])
def test_single_evaluation(name, D, K):
    W, b, q, X, Er, Gr, e_bar, g_bar = reference(D, K, name)
    for state in ('float64', 'float32'):
        d = wide(X, W, b, name, q, state=state)
        E, G = d.E(X), d.dEdX(X)                                    # an energy-only call and a dE/dX-only call
        assert E.shape == (1, 45) and G.shape == (D, 45)
        print('%s %dx%d %s: rel E %.3g (bar %.3g), rel G %.3g (bar %.3g)' % (name, D, K, state, rel(E, Er), e_bar, rel(G, Gr), g_bar))
        assert rel(E, Er) < e_bar, (state, rel(E, Er), e_bar)
        assert rel(G, Gr) < g_bar, (state, rel(G, Gr), g_bar)
        Ej, Gj = d.bind().eval(X, want_E=True, want_grad=True, dtype=state)     # the joint call: the same two halves
        assert np.array_equal(Ej.reshape(1, -1), E) and np.array_equal(Gj, G), state


BOUNDARY = (1300, 1100)      # 3 chunks of dims (the last of 276), 3 blocks of experts (the last of 76)


@gpu
@pytest.mark.parametrize('j0,d0', [(0, 0), (511, 511), (512, 512), (1023, 1023), (1024, 1024), (1099, 1299), (1099, 0), (0, 1299)])
def test_chunk_and_block_boundaries(j0, d0):
    """f = q[0] u^2 with q[0][j] = 1 + j / K and a W whose only non-zero entry is (j0, d0): E = q[0][j0] (w x_d0)^2 and
    dE/dx_d0 = 2 q[0][j0] w^2 x_d0 -- the expert's own q entry (the global index, across block boundaries) and the dim's
    own chunk, or nothing fits.  Every other row of dE/dX is exactly 0."""
    from mjhmc_amd.misc.distributions import LambdaDistribution
    D, K = BOUNDARY
    X = np.random.RandomState(D).randn(D, 45)
    q0 = 1.0 + np.arange(K) / K
    w = 0.7371
    W = np.zeros((K, D))
    W[j0, d0] = w
    w32, q32, x32 = np.float32(w), np.float32(q0[j0]), X[d0].astype(np.float32)
    u32 = w32 * x32
    E32, G32 = (q32 * u32 * u32).astype(np.float64), (np.float32(2) * q32 * u32 * w32).astype(np.float64)
    u64 = w * X[d0]
    e_bar, g_bar = max(E_BAR, 4 * rel(E32, q0[j0] * u64 * u64)), max(G_BAR, 4 * rel(G32, 2 * q0[j0] * u64 * w))
    others = np.arange(D) != d0
    for state in ('float64', 'float32'):
        d = LambdaDistribution(init=X, device_linear_wide=dict(W=W, b=None, energy='q[0]*u*u', grad='2.f*q[0]*u',
                                                               expert_params=q0[None, :]), state_dtype=state)
        E, G = d.E(X), d.dEdX(X)
        print('(%d, %d) %s: rel E %.3g, rel G %.3g' % (j0, d0, state, rel(E[0], E32), rel(G[d0], G32)))
        assert rel(E[0], E32) < e_bar, (state, rel(E[0], E32), e_bar)
        assert rel(G[d0], G32) < g_bar, (state, rel(G[d0], G32), g_bar)
        assert np.all(G[others] == 0.0), state


@gpu
def test_zero_extension():
    """600 more columns of zeros in W (700 -> 1300 dims: one more chunk) change nothing, whatever the state holds there:
    E and the first 700 rows of dE/dX bit for bit, the other rows exactly 0."""
    W, b, _, X, _, _, _, _ = reference(700, 600, 'softplus')
    Wx = np.hstack([W, np.zeros((600, 600))])
    Xx = np.vstack([X, 3.0 * np.random.RandomState(8).randn(600, 45)])
    for state in ('float64', 'float32'):
        a, c = wide(X, W, b, 'softplus', state=state), wide(Xx, Wx, b, 'softplus', state=state)
        Ea, Ga, Ec, Gc = a.E(X), a.dEdX(X), c.E(Xx), c.dEdX(Xx)
        assert np.array_equal(Ea, Ec) and np.array_equal(Ga, Gc[:700]), state
        assert np.all(Gc[700:] == 0.0), state


@gpu
def test_one_chunk_is_the_tall_kernel():
    """D <= 512 on the wide entry point is one chunk of 512: per block the tall kernel's two GEMMs at P = 512 on the same
    operands in the same order, the same masked terms, the same order of sums; dE/dX passes through float32 rows between
    the blocks, which rounds nothing.  Bit-identical by construction; asserted."""
    from mjhmc_amd.misc.distributions import LambdaDistribution
    W, b, _, X, _, _, _, _ = reference(300, 1100, 'softplus')
    e, g = EXPRS['softplus'][:2]
    for state in ('float64', 'float32'):
        t = LambdaDistribution(init=X, device_linear_tall=dict(W=W, b=b, energy=e, grad=g), state_dtype=state)
        w = wide(X, W, b, 'softplus', state=state)
        assert np.array_equal(w.E(X), t.E(X)) and np.array_equal(w.dEdX(X), t.dEdX(X)), state


@gpu
def test_padding_is_exact():
    """The experts beyond K in the last block and the dims beyond D in the last chunk contribute nothing: softplus has
    f(0) = log 2, the L1 expert's f'(0) is NaN."""
    for name in ('softplus', 'l1'):
        W, b, _, X, Er, Gr, e_bar, g_bar = reference(700, 600, name, seed=5 if name == 'l1' else 0)
        d = wide(X, W, b, name)
        E, G = d.E(X), d.dEdX(X)
        assert np.isfinite(E).all() and np.isfinite(G).all(), name
        assert rel(E, Er) < e_bar and rel(G, Gr) < g_bar, (name, rel(E, Er), rel(G, Gr))


@gpu
def test_determinism_and_independence_of_the_grid():
    D, K = 1025, 1100
    W, b, _ = model(D, K, 'softplus')
    X = np.random.RandomState(2).randn(D, 4000)
    d = wide(X[:, :45], W, b, 'softplus')
    E1, G1 = d.E(X[:, :45]), d.dEdX(X[:, :45])
    E2, G2 = d.E(X[:, :45]), d.dEdX(X[:, :45])
    assert np.array_equal(E1, E2) and np.array_equal(G1, G2)
    Eb1, Gb1 = d.E(X), d.dEdX(X)                # 125 tiles: another grid
    Eb2, Gb2 = d.E(X), d.dEdX(X)
    assert np.array_equal(Eb1, Eb2) and np.array_equal(Gb1, Gb2)
    assert np.array_equal(Eb1[:, :45], E1) and np.array_equal(Gb1[:, :45], G1)


FAMILY = (600, 700)      # a softplus model of two chunks (the second of 88 dims) and two blocks (the second of 188 experts)
TALL_TOL = {'float64': dict(delta_rel=4e-6, x_tol=1e-6, e_rtol=4e-6), 'float32': dict(delta_rel=2e-5, x_tol=2e-5, e_rtol=2e-5)}
_TOL = {}


def _family():
    W, b, _ = model(FAMILY[0], FAMILY[1], 'softplus', seed=9)
    return W, b, 'softplus'


def family_tolerances(state, X0, kw):
    """tests/test_gpu_linear_tall.py's tolerances, or 4 x what the two references differ by at these sizes where that is
    more: one MarkovJumpHMC iteration of the oracle on the float32 restatement against one of the oracle on float64 NumPy,
    from the same state with the same draws -- x_tol from max |dX|, |dV| / max(1, max |.|), e_rtol and delta_rel from
    max |dEX| / max(1, max |H0|), over the particles that took the same transition.  CPU only; computed once per state."""
    if state not in _TOL:
        W, b, name = _family()
        N = X0.shape[1]
        okw = dict(state_rounding=f32) if state == 'float32' else {}
        runs = []
        for force in (restated, restated64):
            o = orc.MarkovJumpHMC(orc.LambdaEnergy(*force(W, b, name)), X0.copy(), rng=orc.PhiloxRNG(23, np.arange(N)), resample=False,
                                  **dict(kw, **okw))
            H0 = o.state.H()[0].copy()
            o.sampling_iteration()
            runs.append((o.state.X.copy(), o.state.V.copy(), o.state.EX[0].copy(), o.last_transition.copy(), H0))
        (Xa, Va, Ea, ta, H0), (Xb, Vb, Eb, tb, _) = runs
        same = ta == tb
        dx = max(np.abs(Xa - Xb)[:, same].max() / max(1.0, np.abs(Xb).max()), np.abs(Va - Vb)[:, same].max() / max(1.0, np.abs(Vb).max()))
        de = np.abs(Ea - Eb)[same].max() / max(1.0, np.abs(H0).max())
        t = TALL_TOL[state]
        _TOL[state] = dict(delta_rel=max(t['delta_rel'], 4 * de), x_tol=max(t['x_tol'], 4 * dx), e_rtol=max(t['e_rtol'], 4 * de))
        print('wide family %s: references differ by dx %.3g, de %.3g -> %r' % (state, dx, de, _TOL[state]))
    return _TOL[state]


@gpu
@pytest.mark.parametrize('state', ['float64', 'float32'])
@pytest.mark.parametrize('cls_name', ['MarkovJumpHMC', 'ControlHMC', 'HMC', 'HMCBase'])
def test_sampler_families_against_the_oracle(cls_name, state):
    """As tests/test_gpu_linear_tall.py::test_sampler_families_against_the_oracle on a model of 600 dims x 700 experts:
    transitions and counters exact (up to provable near ties), state and energies within that test's tolerances
    (float64 state: delta_rel 4e-6, x_tol 1e-6, e_rtol 4e-6; float32 state: 2e-5 each) -- or, where the sums of 600 terms
    set the two references themselves further apart than a quarter of those, within 4 x their distance
    (family_tolerances: the oracle on the float32 restatement against the oracle on float64 NumPy, one iteration at these
    sizes; the figures are printed)."""
    from mjhmc_amd.samplers import markov_jump_hmc as M
    W, b, name = _family()
    D, N = W.shape[1], 96
    X0 = np.random.RandomState(11).randn(D, N)
    if state == 'float32':
        X0 = f32(X0)
    d = wide(X0, W, b, name, state=state)
    en = orc.LambdaEnergy(*restated(W, b, name))
    kw = dict(epsilon=0.2, beta=0.3, num_leapfrog_steps=5)
    okw = dict(state_rounding=f32) if state == 'float32' else {}
    tol = family_tolerances(state, X0, kw)
    extra = dict(resample=False) if cls_name == 'MarkovJumpHMC' else {}
    s = getattr(M, cls_name)(distribution=d, seed=23, **kw, **extra)
    o = getattr(orc, cls_name)(en, X0, rng=orc.PhiloxRNG(23, np.arange(N)), **kw, **dict(extra, **okw))
    resync(s, o)
    for t in range(5):
        if cls_name == 'MarkovJumpHMC':
            check_iteration(s, o, tag='wide %s %s it %d' % (cls_name, state, t), **tol)
        else:
            check_control_iteration(s, o, tag='wide %s %s it %d' % (cls_name, state, t), **tol)
        assert (s.l_count, s.f_count, s.r_count) == (o.l_count, o.f_count, o.r_count), t
        resync(s, o)
    out = s.sample(4, preserve_order=True)
    assert out.shape == (D, N, 4) and np.isfinite(out).all()
    assert np.array_equal(out[:, :, -1], s.state.X)


@gpu
@pytest.mark.parametrize('state', ['float64', 'float32'])
def test_fused_call_equals_single_iterations(state):
    from mjhmc_amd.samplers import markov_jump_hmc as M
    W, b, name = _family()
    D, N = W.shape[1], 64
    X0 = f32(np.random.RandomState(4).randn(D, N))
    kw = dict(epsilon=0.2, beta=0.3, num_leapfrog_steps=5, seed=3, resample=False)
    a = M.MarkovJumpHMC(distribution=wide(X0, W, b, name, state=state), **kw)
    c = M.MarkovJumpHMC(distribution=wide(X0, W, b, name, state=state), **kw)
    out = a.sample(6, preserve_order=True)
    for t in range(6):
        c.sampling_iteration()
        assert np.array_equal(c.state.X, out[:, :, t]), t
    assert np.array_equal(a.state.V, c.state.V) and np.array_equal(a.state.EX, c.state.EX)
    assert (a.l_count, a.f_count, a.r_count) == (c.l_count, c.f_count, c.r_count)


@gpu
@pytest.mark.parametrize('state', ['float64', 'float32'])
def test_state_operations(state, tmp_path):
    from mjhmc_amd.samplers import markov_jump_hmc as M
    from mjhmc_amd.samplers.hmc_state import HMCState
    W, b, name = _family()
    D, N = W.shape[1], 48
    X0 = np.random.RandomState(6).randn(D, N)
    s = M.MarkovJumpHMC(distribution=wide(X0, W, b, name, state=state), seed=1, epsilon=0.2, beta=0.3,
                        num_leapfrog_steps=5, resample=False)
    rnd = f32 if state == 'float32' else (lambda a: a)
    Xn = np.random.RandomState(7).randn(D, N) * 1.3
    Vn = np.random.RandomState(8).randn(D, N)
    s.state = HMCState(Xn, s, V=Vn)
    assert np.array_equal(s.state.X, rnd(Xn)) and np.array_equal(s.state.V, rnd(Vn))
    E, G = restated(W, b, name)
    E64, G64 = restated64(W, b, name)
    e_bar = max(E_BAR, 4 * rel(E(rnd(Xn)), E64(rnd(Xn))))
    g_bar = max(G_BAR, 4 * rel(G(rnd(Xn)), G64(rnd(Xn))))
    assert rel(s.state.EX, E(rnd(Xn))) < e_bar and rel(s.state.dEdX, G(rnd(Xn))) < g_bar
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
    # save_state / load_state: the bytes come back
    path = str(tmp_path / 'wide.npz')
    s.save_state(path)
    before = (s.state.X.copy(), s.state.V.copy(), s.state.EX.copy())
    s.sampling_iteration()
    s.load_state(path)
    assert np.array_equal(s.state.X, before[0]) and np.array_equal(s.state.V, before[1]) and np.array_equal(s.state.EX, before[2])


@gpu
@pytest.mark.parametrize('state', ['float64', 'float32'])
def test_rollback_restores_the_state(state):
    from mjhmc_amd import engine, _lib
    W, b, name = _family()
    e, g = EXPRS[name][:2]
    en = engine.DeviceEnergy.from_linear_wide(engine.context(0), W, b, e, g)
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


@gpu
def test_generalized_linear_model_beyond_512_features():
    from mjhmc_amd.misc.distributions import GeneralizedLinearModel
    from mjhmc_amd.samplers.markov_jump_hmc import MarkovJumpHMC
    rs = np.random.RandomState(2031)
    n, D = 1500, 600
    A = rs.randn(n, D) / np.sqrt(D)
    y = A.dot(rs.randn(D)) + rs.randn(n)
    d = GeneralizedLinearModel(A, y, 'gaussian', nbatch=256, seed=5, wide=True)
    assert d.device_energy()[1]['wide']
    X = d.Xinit[:, :64]
    # the bars of this shape: the float32 restatement of the model's own (W, b) against its float64 E_host / dEdX_host
    Er, Gr = restated(d.W, d.b, 'quadratic')
    e_bar, g_bar = max(E_BAR, 4 * rel(Er(X), d.E_host(X))), max(G_BAR, 4 * rel(Gr(X), d.dEdX_host(X)))
    E, G = d.E(X), d.dEdX(X)
    print('wide GLM: rel E %.3g (bar %.3g), rel G %.3g (bar %.3g)' % (rel(E, d.E_host(X)), e_bar, rel(G, d.dEdX_host(X)), g_bar))
    assert rel(E, d.E_host(X)) < e_bar and rel(G, d.dEdX_host(X)) < g_bar
    s = MarkovJumpHMC(distribution=d, epsilon=0.05, beta=0.3, num_leapfrog_steps=5, seed=17, resample=False)
    ex = s.expectations(8)
    assert ex.mean.shape == (D,) and ex.var.shape == (D,) and np.isfinite(ex.mean).all() and np.isfinite(ex.var).all()
    dg = s.diagnostics(8)
    assert dg.rhat.shape == (D,) and dg.ess.shape == (D,) and np.isfinite(dg.rhat).all() and np.isfinite(dg.ess).all()
    t = s.temperature(8)
    assert np.isfinite(t.T) and np.isfinite(t.stderr)
    for call in (lambda: s.pointwise(4), lambda: s.waic(4), lambda: s.influence(4), lambda: s.cv_expectations(4)):
        with pytest.raises(ValueError, match='512 dims'):
            call()


# ---------------------------------------------------------------------------------------------------------------------
# CPU control: what the bars still see
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D,K', [(513, 40), (1000, 513), (1025, 1100), (1536, 700)])
@pytest.mark.parametrize('name', ['quadratic', 'softplus', 'product_of_t'])
def test_control_the_bars_see_a_dropped_expert_and_a_zeroed_chunk(name, D, K):
    W, b, q, X, Er, Gr, e_bar, g_bar = reference(D, K, name)
    assert e_bar < 1e-4 and g_bar < 1e-4                       # float32 sums of <= 1536 terms: the bars stay float32 bars
    keep = np.arange(K) != K // 2
    Ed = restated(W[keep], b[keep], name, None if q is None else q[:, keep])[0](X)
    Wz = W.copy()
    Wz[:, :512] = 0.0                                          # the first chunk of dims
    Ez = restated(Wz, b, name, q)[0](X)
    print('%s %dx%d: bar %.3g; a dropped expert moves E by %.3g, a zeroed chunk by %.3g' % (name, D, K, e_bar, rel(Ed, Er), rel(Ez, Er)))
    assert rel(Ed, Er) > 10 * e_bar and rel(Ez, Er) > 10 * e_bar
