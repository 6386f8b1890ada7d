"""CPU: the host side of the data-row influence (HMCBase.influence) -- the arithmetic of Influence from
hand-made sums, the refusals of influence_request that need no device, the compile of the stored-values kernel for a
square and a tall model, the ctypes prototypes, and GeneralizedLinearModel.influence_value() against its own float64
energy."""
import numpy as np
import pytest

from mjhmc_amd import _lib, engine
from mjhmc_amd.misc.distributions import ProductOfT, TestGaussian
from mjhmc_amd.samplers import markov_jump_hmc as M
from tests.test_pointwise_cpu import c_eval, glm


@pytest.fixture(scope='module', autouse=True)
def built_library():
    import os
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()


def sums_of(x, t, w, cx, ct):
    """the device sums of states x (n, D) and values t (n, J) with weights w (n,) about (cx, ct), by the book"""
    w = np.asarray(w, dtype=np.float64)[:, None]
    return (w.sum(), (w * (x - cx)).sum(axis=0), (w * (x - cx) ** 2).sum(axis=0), (w * (t - ct)).sum(axis=0),
            (w * (t - ct) ** 2).sum(axis=0), (w * x).T.dot(t - ct))


def hand_made(j0=3, n_data=None, seed=0):
    rs = np.random.RandomState(seed)
    n, D, J = 50, 4, 7
    x = 5.0 + rs.randn(n, D) * [1.0, 2.0, 0.5, 3.0]
    t = -2.0 + x.dot(rs.randn(D, J)) + rs.randn(n, J)
    t[:, 5] = 1.25                                       # a value that does not vary: zero variance, zero covariance
    w = rs.randint(0, 5, size=n) / 2.0
    cx, ct = x[0].copy(), t[0].copy()
    W, Sx, S2x, St, S2t, Cxt = sums_of(x, t, w, cx, ct)
    inf = M.Influence(W, Sx, S2x, St, S2t, Cxt, int((w >= 0).sum()), (j0, j0 + J), cx, ct, n_data=n_data)
    return inf, x, t, w


def weighted_cov(x, t, w):
    mx, mt = np.average(x, axis=0, weights=w), np.average(t, axis=0, weights=w)
    return ((x - mx) * w[:, None]).T.dot(t - mt) / w.sum(), mx, mt


def test_influence_from_hand_made_sums():
    inf, x, t, w = hand_made()
    cov, mx, mt = weighted_cov(x, t, w)
    assert inf.W == w.sum() and inf.total_weight == inf.W and inf.n_states == 50 and inf.experts == (3, 10)
    assert np.allclose(inf.mean_x, mx, rtol=1e-13) and np.allclose(inf.mean_t, mt, rtol=1e-13)
    vx = np.average((x - mx) ** 2, axis=0, weights=w)
    vt = np.average((t - mt) ** 2, axis=0, weights=w)
    assert np.allclose(inf.var_x, vx, rtol=1e-12) and np.allclose(inf.var_t, vt, rtol=1e-11, atol=1e-13)
    assert inf.cov.shape == (4, 7) and np.allclose(inf.cov, cov, rtol=1e-10, atol=1e-12)
    assert np.array_equal(inf.loo_shift, -inf.cov)
    assert np.allclose(inf.loo_mean(4), mx - cov[:, 1], rtol=1e-10)
    with pytest.raises(ValueError, match='experts in'):
        inf.loo_mean(2)
    # corr: the plain definition where both variances are positive; exactly 0 in the zero-variance column, never NaN
    live = np.arange(7) != 5
    assert np.allclose(inf.corr[:, live], cov[:, live] / np.sqrt(np.outer(vx, vt[live])), rtol=1e-9)
    assert inf.var_t[5] == 0.0 and np.all(inf.corr[:, 5] == 0.0) and np.isfinite(inf.corr).all()
    assert np.all(np.abs(inf.corr) <= 1 + 1e-12)
    assert np.abs(inf.cov[:, 5]).max() <= 1e-12


def test_the_shift_does_not_enter_the_derived_quantities():
    inf, x, t, w = hand_made()
    W, Sx, S2x, St, S2t, Cxt = sums_of(x, t, w, 0.0 * x[0], 0.0 * t[0])
    plain = M.Influence(W, Sx, S2x, St, S2t, Cxt, 50, (3, 10), np.zeros(4), np.zeros(7))
    for a, b in ((inf.cov, plain.cov), (inf.mean_x, plain.mean_x), (inf.mean_t, plain.mean_t), (inf.var_x, plain.var_x)):
        assert np.allclose(a, b, rtol=1e-9, atol=1e-11)


def test_ij_cov_distance_and_most_influential():
    inf, x, t, w = hand_made()
    I = inf.cov
    assert np.allclose(inf.ij_cov(center=False), I.dot(I.T), rtol=1e-13)
    Ic = I - I.mean(axis=1, keepdims=True)
    assert np.allclose(inf.ij_cov(), Ic.dot(Ic.T), rtol=1e-13)
    rows = [4, 9, 3]                                     # experts by their index in the model: columns 1, 6, 0
    sub = I[:, [1, 6, 0]]
    assert np.allclose(inf.ij_cov(rows=rows, center=False), sub.dot(sub.T), rtol=1e-13)
    subc = sub - sub.mean(axis=1, keepdims=True)
    assert np.allclose(inf.ij_cov(rows=rows), subc.dot(subc.T), rtol=1e-13)
    with pytest.raises(ValueError, match='experts in'):
        inf.ij_cov(rows=[10])
    # n_data: rows=None means the data rows inside the range
    part, _, _, _ = hand_made(n_data=8)
    assert np.allclose(part.ij_cov(center=False), I[:, :5].dot(I[:, :5].T), rtol=1e-13)
    P = np.diag([1.0, 0.25, 4.0, 0.5]) + 0.1
    want = np.array([I[:, j].dot(P).dot(I[:, j]) for j in range(7)])
    assert np.allclose(inf.distance(P), want, rtol=1e-12)
    with pytest.raises(ValueError, match='precision'):
        inf.distance(np.eye(3))
    top = inf.most_influential(3, precision=P)
    assert list(top) == list(3 + np.argsort(-want, kind='stable')[:3])
    scaled = np.array([(I[:, j] ** 2 / inf.var_x).sum() for j in range(7)])
    assert list(inf.most_influential(2)) == list(3 + np.argsort(-scaled, kind='stable')[:2])
    assert 8 not in inf.most_influential(6)              # the zero-variance value is the least influential


# ---------------------------------------------------------------------------------------------------------------------
# refusals that need no device
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_without_a_device():
    from mjhmc_amd.misc.distributions import LambdaDistribution
    d = glm('logistic')
    K = d.nexperts
    with pytest.raises(ValueError, match='n_iter must be >= 1'):
        M.influence_request(d, 0)
    with pytest.raises(ValueError, match='ISO_GAUSS'):
        M.influence_request(TestGaussian(ndims=3, nbatch=4), 3, value='u')
    with pytest.raises(ValueError, match='PRODUCT_OF_T'):
        M.influence_request(ProductOfT(ndims=36, nbasis=36, nbatch=4), 3)
    W = np.random.RandomState(0).randn(7, 3)
    plain = LambdaDistribution(init=np.zeros((3, 4)), device_linear=dict(W=W, b=np.zeros(7), energy='0.5f*u*u', grad='u'))
    with pytest.raises(ValueError, match='influence_value'):
        M.influence_request(plain, 3)
    assert M.influence_request(plain, 3, value='u') == ('u', (0, 7))
    with pytest.raises(ValueError, match='one value'):
        M.influence_request(d, 3, value=['u', 'u*u'])
    with pytest.raises(ValueError):
        M.influence_request(d, 3, value='u; u*u')
    with pytest.raises(ValueError):
        M.influence_request(d, 3, value='  ')
    for bad in ((-1, 5), (0, K + 1), (5, 5), (9, 4)):
        with pytest.raises(ValueError, match='not a range'):
            M.influence_request(d, 3, experts=bad)
    with pytest.raises(ValueError, match='sharded'):
        M.influence_request(d, 3, sharded=True)
    with pytest.raises(ValueError) as err:
        M.influence_request(d, 3, value='no_such_symbol + u')
    assert 'no_such_symbol' in str(err.value) and 'does not compile' in str(err.value)     # the compiler's own text
    value, experts = M.influence_request(d, 3)                # the distribution's own value compiles
    assert value == d.influence_value() and experts == (0, K)
    assert M.influence_request(d, 3, value='u', experts=(2, K - 1)) == ('u', (2, K - 1))


def test_check_compiles_for_square_and_tall_models():
    engine.influence_check(36, 36, 'q[0]*u')                      # one square block (NB = 1)
    engine.influence_check(10, 513, '(float)(j % 7)')             # tall, NB = 1
    lib = _lib.load()
    hdr = _lib.KERNEL_HEADERS.encode()
    assert lib.mjhmc_influence_check(10, 513, b'u +', hdr) == -1
    msg = lib.mjhmc_last_error()
    assert b'does not compile' in msg and b'error' in msg
    assert lib.mjhmc_influence_check(600, 10, b'u', hdr) == -3        # MJHMC_ERR_UNSUPPORTED
    assert lib.mjhmc_influence_check(10, 10, b'u;u', hdr) == -1
    assert b'ONE value' in lib.mjhmc_last_error()
    assert lib.mjhmc_influence_check(10, 10, b' ', hdr) == -1
    assert b'empty' in lib.mjhmc_last_error()
    assert lib.mjhmc_influence_check(10, 10, None, hdr) == -1


def test_prototypes_are_bound():
    lib = _lib.load()
    for name in ('check', 'create', 'set_shift', 'info', 'accumulate', 'read', 'read_cross', 'reset', 'destroy'):
        assert 'mjhmc_influence_' + name in _lib.PROTOTYPES
        assert hasattr(lib, 'mjhmc_influence_' + name)
    assert lib.mjhmc_abi_version() == 2
    assert lib.mjhmc_influence_destroy(None) == 0
    assert lib.mjhmc_influence_accumulate(None, 0, -1, 1) == -1
    assert lib.mjhmc_influence_reset(None) == -1
    assert lib.mjhmc_influence_read_cross(None, 0, 1, None) == -1


# ---------------------------------------------------------------------------------------------------------------------
# GeneralizedLinearModel.influence_value(): l = -f(u), expert by expert
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', ['gaussian', 'logistic', 'poisson'])
def test_glm_influence_value_is_minus_f(family):
    d = glm(family, noise_scale=0.7, prior_scale=2.0) if family == 'gaussian' else glm(family, prior_scale=2.0)
    v = d.influence_value()
    assert isinstance(v, str) and v == d.pointwise_values()[0][0]
    assert d.n_data == d.features.shape[0] == d.nexperts - d.ndims
    X = 0.3 * np.random.RandomState(4).randn(d.ndims, 11)
    u, f, _ = d._terms(X)
    q = None if d.q is None else [d.q[0][:, None], d.q[1][:, None]]
    ll = c_eval(v, u, np.arange(d.nexperts)[:, None], q) * np.ones_like(u)
    assert np.allclose(ll, -f, rtol=1e-12, atol=1e-14)                       # every expert, the prior's included
    assert np.allclose(-ll.sum(axis=0), d.E_host(X)[0], rtol=1e-12)
