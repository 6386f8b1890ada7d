"""CPU: linear-model energies E(x) = sum_j f(u_j, j), u = W x + b (MJHMC_E_LINEAR_EXPR, csrc/linear_energy.hip).  The
hipRTC compile of the 14 tile kernels needs no device (mjhmc_linear_check); argument and shape checks happen before any
device call."""
import ctypes

import numpy as np
import pytest

from mjhmc_amd import _lib, engine

ERR_INVALID, ERR_UNSUPPORTED = -1, -3     # include/mjhmc_hip.h

EXPRS = {
    'quadratic': ('0.5f*u*u', 'u'),
    'softplus': ('u > 20.f ? u : log1pf(expf(u))', '1.f/(1.f + expf(-u))'),
    'product_of_t': ('q[0]*logf(1.f + u*u)', '2.f*q[0]*u/(1.f + u*u)'),
}


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


@pytest.mark.parametrize('D,K', [(36, 36), (10, 300), (300, 10), (512, 512)])
@pytest.mark.parametrize('name', sorted(EXPRS))
def test_linear_kernels_compile_without_a_device(lib, name, D, K):
    e, g = EXPRS[name]
    assert lib.mjhmc_linear_check(D, K, e.encode(), g.encode(), _lib.KERNEL_HEADERS.encode()) == 0, lib.mjhmc_last_error()


def test_compile_error_is_reported(lib):
    rc = lib.mjhmc_linear_check(36, 36, b'0.5f*u*v', b'u', _lib.KERNEL_HEADERS.encode())
    assert rc == ERR_INVALID
    assert b'undeclared' in lib.mjhmc_last_error()


@pytest.mark.parametrize('D,K,code', [(513, 10, ERR_UNSUPPORTED), (10, 513, ERR_UNSUPPORTED), (10, 0, ERR_INVALID),
                                      (0, 10, ERR_INVALID)])
def test_sizes_beyond_the_tile_kernels_are_refused(lib, D, K, code):
    assert lib.mjhmc_linear_check(D, K, b'u', b'u', _lib.KERNEL_HEADERS.encode()) == code
    if code == ERR_UNSUPPORTED:
        assert b'512' in lib.mjhmc_last_error()
    # the creation entry point refuses the same before it touches a device (no context needed to see it)
    W = np.zeros((max(K, 1), max(D, 1)))
    b = np.zeros(max(K, 1))
    h = ctypes.c_void_p()
    assert lib.mjhmc_energy_create_linear(None, D, K, _lib.ptr(W), _lib.ptr(b), b'u', b'u', None, 0, None, 0,
                                          _lib.KERNEL_HEADERS.encode(), ctypes.byref(h)) < 0


@pytest.mark.parametrize('W,b,q,what', [
    (np.zeros(5), np.zeros(5), None, 'W must be'),
    (np.zeros((3, 4)), np.zeros(4), None, 'b must have'),
    (np.zeros((3, 4)), np.zeros(3), np.zeros((2, 4)), 'expert_params'),
    (np.zeros((3, 4)), np.zeros(3), np.zeros((5, 3)), 'expert_params'),
    (np.zeros((600, 4)), np.zeros(600), None, 'at most 512'),
    (np.zeros((4, 600)), np.zeros(4), None, 'at most 512'),
])
def test_bad_shapes_raise_in_python(W, b, q, what):
    with pytest.raises(ValueError, match=what):
        engine.linear_arrays(W, b, (), q)


def test_lambda_distribution_checks_its_linear_model():
    from mjhmc_amd.misc.distributions import LambdaDistribution
    X0 = np.zeros((4, 8))
    with pytest.raises(ValueError, match='columns'):
        LambdaDistribution(init=X0, device_linear=dict(W=np.eye(5), energy='0.5f*u*u', grad='u'))
    with pytest.raises(ValueError, match='b must have'):
        LambdaDistribution(init=X0, device_linear=dict(W=np.eye(4), b=np.zeros(3), energy='0.5f*u*u', grad='u'))
    d = LambdaDistribution(init=X0, device_linear=dict(W=np.ones((7, 4)), energy='0.5f*u*u', grad='u'), state_dtype='float32')
    kind, p = d.device_energy()
    assert kind == _lib.E_LINEAR_EXPR and p['W'].shape == (7, 4) and p['b'].shape == (7,) and d.state_dtype == 'float32'


def test_correlated_gaussian_description():
    from mjhmc_amd.misc.distributions import CorrelatedGaussian
    from mjhmc_amd.misc import gen_mj_init as G
    d = CorrelatedGaussian(ndims=6, nbatch=5000, mean=np.arange(6.0))
    ev = np.linalg.eigvalsh(d.cov)
    assert np.isclose(ev.max() / ev.min(), 100.0)                     # log_conditioning = 2
    kind, p = d.device_energy()
    assert kind == _lib.E_LINEAR_EXPR
    x = np.random.RandomState(1).randn(6)
    u = p['W'] @ x + p['b']
    assert np.isclose(0.5 * u @ u, 0.5 * (x - d.mean) @ d.precision @ (x - d.mean))
    assert np.abs(d.Xinit.mean(axis=1) - d.mean).max() < 0.2                # exact draws from N(mu, cov)
    assert np.abs(np.cov(d.Xinit) - d.cov).max() < 0.1 * np.abs(d.cov).max()
    assert hash(d) == hash(CorrelatedGaussian(ndims=6, nbatch=3, mean=np.arange(6.0))) != hash(CorrelatedGaussian(ndims=6))
    assert G.stable_digest(d) == G.stable_digest(CorrelatedGaussian(ndims=6, nbatch=3, mean=np.arange(6.0)))
    with pytest.raises(ValueError):
        CorrelatedGaussian(cov=np.eye(3), precision=np.eye(3))
