"""CPU: tall linear-model energies -- more than 512 experts, D <= 512, K <= 2**20 (mjhmc_energy_create_linear_tall,
csrc/dense_lin_tall.hpp) -- and GeneralizedLinearModel.  The hipRTC compile of the one fused kernel needs no
device (mjhmc_linear_tall_check); argument and shape checks happen before any device call."""
import ctypes
import os
import re

import numpy as np
import pytest

from mjhmc_amd import _lib, engine

ERR_INVALID, ERR_UNSUPPORTED = -1, -3     # include/mjhmc_hip.h

EXPRS = {
    'quadratic': ('0.5f*u*u', 'u'),
    'softplus': ('u > 20.f ? u : log1pf(expf(u))', '1.f/(1.f + expf(-u))'),
    'product_of_t': ('q[0]*logf(1.f + u*u)', '2.f*q[0]*u/(1.f + u*u)'),
}
HDR = _lib.KERNEL_HEADERS.encode()


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


@pytest.mark.parametrize('D,K', [(10, 513), (300, 2049), (512, 65536)])
@pytest.mark.parametrize('name', sorted(EXPRS))
def test_tall_kernel_compiles_without_a_device(lib, name, D, K):
    e, g = EXPRS[name]
    assert lib.mjhmc_linear_tall_check(D, K, e.encode(), g.encode(), HDR) == 0, lib.mjhmc_last_error()


def test_compile_error_is_reported(lib):
    rc = lib.mjhmc_linear_tall_check(36, 600, b'0.5f*u*v', b'u', HDR)
    assert rc == ERR_INVALID
    assert b'undeclared' in lib.mjhmc_last_error()


@pytest.mark.parametrize('D,K,code,limit', [(513, 10, ERR_UNSUPPORTED, b'512'), (10, 2 ** 20 + 1, ERR_UNSUPPORTED, b'1048576'),
                                            (10, 0, ERR_INVALID, None), (0, 10, ERR_INVALID, None)])
def test_sizes_outside_the_limits_are_refused(lib, D, K, code, limit):
    assert lib.mjhmc_linear_tall_check(D, K, b'u', b'u', HDR) == code
    if limit:
        assert limit in lib.mjhmc_last_error()
    # the creation entry point refuses the same before it touches a device (no context needed to see it)
    W = np.zeros((max(K, 1), max(D, 1)))
    b = np.zeros(max(K, 1))
    h = ctypes.c_void_p()
    assert lib.mjhmc_energy_create_linear_tall(None, D, K, _lib.ptr(W), _lib.ptr(b), b'u', b'u', None, 0, None, 0, HDR,
                                               ctypes.byref(h)) == code
    if limit:
        assert limit in lib.mjhmc_last_error()


def test_creation_without_a_context_is_refused(lib):
    W, b, h = np.zeros((600, 10)), np.zeros(600), ctypes.c_void_p()
    assert lib.mjhmc_energy_create_linear_tall(None, 10, 600, _lib.ptr(W), _lib.ptr(b), b'u', b'u', None, 0, None, 0, HDR,
                                               ctypes.byref(h)) == ERR_INVALID
    assert not h.value


def test_old_entry_points_still_refuse_beyond_512(lib):
    assert lib.mjhmc_linear_check(10, 513, b'u', b'u', HDR) == ERR_UNSUPPORTED
    assert b'no blocked form' in lib.mjhmc_last_error()
    with pytest.raises(ValueError, match='at most 512'):
        engine.linear_arrays(np.zeros((600, 4)), np.zeros(600))


@pytest.mark.parametrize('W,b,q,what', [
    (np.zeros(5), np.zeros(5), None, 'W must be'),
    (np.zeros((700, 4)), np.zeros(4), None, 'b must have'),
    (np.zeros((700, 4)), np.zeros(700), np.zeros((2, 4)), 'expert_params'),
    (np.zeros((700, 4)), np.zeros(700), np.zeros((5, 700)), 'expert_params'),
    (np.zeros((4, 600)), np.zeros(4), None, r'2\*\*20 experts and 512 dims'),
    (np.zeros((2 ** 20 + 1, 1)), np.zeros(2 ** 20 + 1), None, r'2\*\*20 experts and 512 dims'),
])
def test_bad_shapes_raise_in_python(W, b, q, what):
    with pytest.raises(ValueError, match=what):
        engine.tall_linear_arrays(W, b, (), q)


def test_tall_arrays_take_what_the_tile_form_refuses():
    W, b, p, q = engine.tall_linear_arrays(np.ones((700, 4)), None, (1, 2), np.ones(700))
    assert W.shape == (700, 4) and b.shape == (700,) and p.tolist() == [1.0, 2.0] and q.shape == (1, 700)


def test_lambda_distribution_checks_its_tall_model():
    from mjhmc_amd.misc.distributions import LambdaDistribution
    X0 = np.zeros((4, 8))
    W = np.ones((700, 4))
    with pytest.raises(ValueError, match='columns'):
        LambdaDistribution(init=X0, device_linear_tall=dict(W=np.ones((700, 5)), energy='0.5f*u*u', grad='u'))
    with pytest.raises(ValueError, match='b must have'):
        LambdaDistribution(init=X0, device_linear_tall=dict(W=W, b=np.zeros(3), energy='0.5f*u*u', grad='u'))
    with pytest.raises(ValueError, match='expert_params'):
        LambdaDistribution(init=X0, device_linear_tall=dict(W=W, energy='0.5f*u*u', grad='u', expert_params=np.zeros((1, 4))))
    with pytest.raises(ValueError, match='at most 512'):          # the tile form keeps its limit
        LambdaDistribution(init=X0, device_linear=dict(W=W, energy='0.5f*u*u', grad='u'))
    d = LambdaDistribution(init=X0, device_linear_tall=dict(W=W, energy='0.5f*u*u', grad='u'), state_dtype='float32')
    kind, p = d.device_energy()
    assert kind == _lib.E_LINEAR_EXPR and p['tall'] and p['W'].shape == (700, 4) and p['b'].shape == (700,)
    assert d.state_dtype == 'float32'


def test_header_declares_the_entry_points_and_the_abi_version_stands(lib):
    with open(os.path.join(os.path.dirname(_lib.KERNEL_HEADERS), '..', 'include', 'mjhmc_hip.h')) as f:
        text = f.read()
    assert re.search(r'int mjhmc_energy_create_linear_tall\(mjhmc_ctx\* ctx, int ndims, int64_t nexperts,', text)
    assert re.search(r'int mjhmc_linear_tall_check\(int ndims, int64_t nexperts,', text)
    assert re.search(r'#define MJHMC_ABI_VERSION 2\b', text)
    assert hasattr(lib, 'mjhmc_energy_create_linear_tall') and hasattr(lib, 'mjhmc_linear_tall_check')


def _glm(family, n=40, D=5, nbatch=7, seed=0, **kw):
    from mjhmc_amd.misc.distributions import GeneralizedLinearModel
    rs = np.random.RandomState(seed)
    A = rs.randn(n, D)
    eta = A.dot(rs.randn(D) * 0.5)
    if family == 'gaussian':
        y = eta + 0.3 * rs.randn(n)
    elif family == 'logistic':
        y = (rs.rand(n) < 1 / (1 + np.exp(-eta))).astype(float)
    else:
        y = rs.poisson(np.exp(eta)).astype(float)
    return GeneralizedLinearModel(A, y, family, nbatch=nbatch, seed=1, **kw)


@pytest.mark.parametrize('family', ['gaussian', 'logistic', 'poisson'])
def test_glm_gradient_is_the_derivative_of_its_energy(family):
    d = _glm(family, prior_scale=2.0, noise_scale=0.7)
    X = np.random.RandomState(3).randn(d.ndims, 6) * 0.4
    G = d.dEdX_host(X)
    assert d.E_host(X).shape == (1, 6) and G.shape == X.shape
    h = 1e-6
    for k in range(d.ndims):
        dX = np.zeros_like(X)
        dX[k] = h
        num = (d.E_host(X + dX) - d.E_host(X - dX))[0] / (2 * h)
        assert np.allclose(num, G[k], rtol=1e-6, atol=1e-6), (family, k)
    # the prior's share: E at 0 has no prior term, the gradient at large x is dominated by x / prior_scale^2
    kind, p = d.device_energy()
    assert p['W'].shape == (40 + 5, 5) and np.array_equal(p['W'][40:], np.eye(5) / 2.0)
    if family != 'gaussian':
        assert np.array_equal(p['expert_params'][1], np.r_[np.ones(40), np.zeros(5)])
        assert np.array_equal(p['expert_params'][0][:40], d.targets) and 'q[1]' in p['energy'] and 'q[1]' in p['grad']


def test_glm_posterior_solves_the_normal_equations():
    d = _glm('gaussian', prior_scale=1.5, noise_scale=0.3)
    mean, cov = d.posterior()
    A, y = d.features, d.targets
    precision = A.T.dot(A) / 0.3 ** 2 + np.eye(5) / 1.5 ** 2
    assert np.allclose(precision.dot(mean), A.T.dot(y) / 0.3 ** 2, rtol=1e-10)
    assert np.allclose(cov.dot(precision), np.eye(5), atol=1e-10)
    assert np.abs(d.dEdX_host(mean[:, None])).max() < 1e-8          # the mode
    with pytest.raises(NotImplementedError):
        _glm('logistic').posterior()


def test_glm_picks_its_path_by_the_expert_count():
    small = _glm('logistic', n=100, D=5)
    kind, p = small.device_energy()
    assert kind == _lib.E_LINEAR_EXPR and not p.get('tall') and p['W'].shape == (105, 5)       # the tile kernels' path
    engine.linear_arrays(p['W'], p['b'], p['params'], p['expert_params'])
    tall = _glm('logistic', n=600, D=5)
    kind, p = tall.device_energy()
    assert kind == _lib.E_LINEAR_EXPR and p['tall'] and p['W'].shape == (605, 5)
    assert tall.Xinit.shape == (5, 7) and np.abs(tall.Xinit).max() < 1.0
    from mjhmc_amd.misc.distributions import GeneralizedLinearModel
    with pytest.raises(ValueError, match='family'):
        GeneralizedLinearModel(np.zeros((3, 2)), np.zeros(3), 'probit')
    with pytest.raises(ValueError, match='targets'):
        GeneralizedLinearModel(np.zeros((3, 2)), np.zeros(4), 'gaussian')
    with pytest.raises(ValueError, match='512 dims'):
        GeneralizedLinearModel(np.zeros((3, 600)), np.zeros(3), 'gaussian')


def test_glm_hash_and_digest_are_stable_over_nbatch():
    from mjhmc_amd.misc import gen_mj_init as G
    a, b, c = _glm('logistic', n=600, nbatch=7), _glm('logistic', n=600, nbatch=50), _glm('logistic', n=600, seed=4)
    assert hash(a) == hash(b) != hash(c)
    assert G.stable_digest(a) == G.stable_digest(b) != G.stable_digest(c)
    assert G.stable_digest(_glm('poisson', n=600)) != G.stable_digest(_glm('poisson', n=600, prior_scale=2.0))
