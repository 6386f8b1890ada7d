"""CPU: wide linear-model energies -- more than 512 dims, D <= 4096, K <= 2**20 (mjhmc_energy_create_linear_wide,
csrc/dense_lin_wide.hpp) -- and GeneralizedLinearModel beyond 512 features.  The hipRTC compile of the one
fused kernel needs no device (mjhmc_linear_wide_check); argument and shape checks happen before any device call."""
import ctypes
import os
import re

import numpy as np
import pytest

from mjhmc_amd import _lib, engine
from tests.test_linear_tall_cpu import EXPRS

ERR_INVALID, ERR_UNSUPPORTED = -1, -3     # include/mjhmc_hip.h
HDR = _lib.KERNEL_HEADERS.encode()


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


@pytest.mark.parametrize('D,K', [(513, 10), (1025, 600), (4096, 65536)])
@pytest.mark.parametrize('name', sorted(EXPRS))
def test_wide_kernel_compiles_without_a_device(lib, name, D, K):
    e, g = EXPRS[name]
    assert lib.mjhmc_linear_wide_check(D, K, e.encode(), g.encode(), HDR) == 0, lib.mjhmc_last_error()


def test_compile_error_is_reported(lib):
    rc = lib.mjhmc_linear_wide_check(600, 600, b'0.5f*u*v', b'u', HDR)
    assert rc == ERR_INVALID
    assert b'undeclared' in lib.mjhmc_last_error()


@pytest.mark.parametrize('D,K,code,limit', [(4097, 10, ERR_UNSUPPORTED, b'4096'), (600, 2 ** 20 + 1, ERR_UNSUPPORTED, b'1048576'),
                                            (0, 10, ERR_INVALID, None), (600, 0, ERR_INVALID, None)])
def test_sizes_outside_the_limits_are_refused(lib, D, K, code, limit):
    assert lib.mjhmc_linear_wide_check(D, K, b'u', b'u', HDR) == code
    if limit:
        assert limit in lib.mjhmc_last_error()
    # the creation entry point refuses the same before it touches a device (no context needed to see it)
    W = np.zeros((1, 1))
    b = np.zeros(1)
    h = ctypes.c_void_p()
    assert lib.mjhmc_energy_create_linear_wide(None, D, K, _lib.ptr(W), _lib.ptr(b), b'u', b'u', None, 0, None, 0, HDR,
                                               ctypes.byref(h)) == code
    if limit:
        assert limit in lib.mjhmc_last_error()
    assert not h.value


def test_creation_without_a_context_is_refused(lib):
    W, b, h = np.zeros((10, 600)), np.zeros(10), ctypes.c_void_p()
    assert lib.mjhmc_energy_create_linear_wide(None, 600, 10, _lib.ptr(W), _lib.ptr(b), b'u', b'u', None, 0, None, 0, HDR,
                                               ctypes.byref(h)) == ERR_INVALID
    assert not h.value


def test_the_other_entry_points_keep_their_512_dims(lib):
    assert lib.mjhmc_linear_check(513, 10, b'u', b'u', HDR) == ERR_UNSUPPORTED
    assert lib.mjhmc_linear_tall_check(513, 10, b'u', b'u', HDR) == ERR_UNSUPPORTED and b'512' in lib.mjhmc_last_error()
    assert lib.mjhmc_linear_grouped_check(513, 10, 2, 2, b'u', b'u', HDR) == ERR_UNSUPPORTED
    with pytest.raises(ValueError, match='512 dims'):
        engine.tall_linear_arrays(np.zeros((4, 600)), np.zeros(4))


@pytest.mark.parametrize('W,b,q,what', [
    (np.zeros(5), np.zeros(5), None, 'W must be'),
    (np.zeros((7, 600)), np.zeros(4), None, 'b must have'),
    (np.zeros((7, 600)), np.zeros(7), np.zeros((2, 4)), 'expert_params'),
    (np.zeros((7, 600)), np.zeros(7), np.zeros((5, 7)), 'expert_params'),
    (np.zeros((4, 4097)), np.zeros(4), None, r'2\*\*20 experts and 4096 dims'),
    (np.zeros((2 ** 20 + 1, 1)), np.zeros(2 ** 20 + 1), None, r'2\*\*20 experts and 4096 dims'),
])
def test_bad_shapes_raise_in_python(W, b, q, what):
    with pytest.raises(ValueError, match=what):
        engine.wide_linear_arrays(W, b, (), q)


def test_wide_arrays_take_what_the_other_forms_refuse():
    W, b, p, q = engine.wide_linear_arrays(np.ones((700, 4096)), None, (1, 2), np.ones(700))
    assert W.shape == (700, 4096) and b.shape == (700,) and p.tolist() == [1.0, 2.0] and q.shape == (1, 700)
    W, b, p, q = engine.wide_linear_arrays(np.ones((3, 4)), None)            # one chunk is legal
    assert W.shape == (3, 4) and q.shape == (0, 3)


def test_lambda_distribution_checks_its_wide_model():
    from mjhmc_amd.misc.distributions import LambdaDistribution
    X0 = np.zeros((600, 8))
    W = np.ones((700, 600))
    with pytest.raises(ValueError, match='columns'):
        LambdaDistribution(init=X0, device_linear_wide=dict(W=np.ones((700, 601)), energy='0.5f*u*u', grad='u'))
    with pytest.raises(ValueError, match='b must have'):
        LambdaDistribution(init=X0, device_linear_wide=dict(W=W, b=np.zeros(3), energy='0.5f*u*u', grad='u'))
    with pytest.raises(ValueError, match='expert_params'):
        LambdaDistribution(init=X0, device_linear_wide=dict(W=W, energy='0.5f*u*u', grad='u', expert_params=np.zeros((1, 4))))
    with pytest.raises(ValueError, match='512 dims'):             # the tall form keeps its limit
        LambdaDistribution(init=X0, device_linear_tall=dict(W=W, energy='0.5f*u*u', grad='u'))
    with pytest.raises(ValueError, match='one of'):
        LambdaDistribution(init=X0, device_linear_tall=dict(W=W, energy='u', grad='u'),
                           device_linear_wide=dict(W=W, energy='u', grad='u'))
    with pytest.raises(ValueError, match='state_dtype'):
        LambdaDistribution(init=X0, device_linear_wide=dict(W=W, energy='u', grad='u'), state_dtype='bfloat16')
    d = LambdaDistribution(init=X0, device_linear_wide=dict(W=W, energy='0.5f*u*u', grad='u'), state_dtype='float32')
    kind, p = d.device_energy()
    assert kind == _lib.E_LINEAR_EXPR and p['wide'] and not p.get('tall') and not p.get('groups')
    assert p['W'].shape == (700, 600) and p['b'].shape == (700,) and d.state_dtype == 'float32'


def test_header_declares_the_entry_points_and_the_abi_version_stands(lib):
    with open(os.path.join(os.path.dirname(_lib.KERNEL_HEADERS), '..', 'include', 'mjhmc_hip.h')) as f:
        text = f.read()
    assert re.search(r'int mjhmc_energy_create_linear_wide\(mjhmc_ctx\* ctx, int ndims, int64_t nexperts,', text)
    assert re.search(r'int mjhmc_linear_wide_check\(int ndims, int64_t nexperts,', text)
    assert re.search(r'#define MJHMC_ABI_VERSION 2\b', text)
    assert hasattr(lib, 'mjhmc_energy_create_linear_wide') and hasattr(lib, 'mjhmc_linear_wide_check')
    assert lib.mjhmc_abi_version() == 2


def _glm(family, n=40, D=600, nbatch=7, seed=0, wide=True, **kw):
    from mjhmc_amd.misc.distributions import GeneralizedLinearModel
    rs = np.random.RandomState(seed)
    A = rs.randn(n, D) / np.sqrt(D)
    eta = A.dot(rs.randn(D) * 0.5)
    if family == 'gaussian':
        y = eta + 0.3 * rs.randn(n)
    elif family == 'logistic':
        y = (rs.rand(n) < 1 / (1 + np.exp(-eta))).astype(float)
    else:
        y = rs.poisson(np.exp(eta)).astype(float)
    return GeneralizedLinearModel(A, y, family, nbatch=nbatch, seed=1, wide=wide, **kw)


@pytest.mark.parametrize('family', ['gaussian', 'logistic', 'poisson'])
def test_glm_beyond_512_features_constructs(family):
    """n = 40 rows, D = 600 features: K = 640 experts of 600 dims, the wide form (wide=True: without the keyword the model
    is refused as it always was, which tests/test_linear_tall_cpu.py pins)"""
    d = _glm(family, prior_scale=2.0, noise_scale=0.7)
    kind, p = d.device_energy()
    assert kind == _lib.E_LINEAR_EXPR and p['wide'] and not p.get('tall')
    assert p['W'].shape == (640, 600) and np.array_equal(p['W'][40:], np.eye(600) / 2.0)
    assert d.Xinit.shape == (600, 7)
    X = np.random.RandomState(3).randn(d.ndims, 6) * 0.4
    G = d.dEdX_host(X)
    assert d.E_host(X).shape == (1, 6) and G.shape == X.shape
    h = 1e-6
    for k in (0, 1, 299, 511, 512, 599):
        dX = np.zeros_like(X)
        dX[k] = h
        num = (d.E_host(X + dX) - d.E_host(X - dX))[0] / (2 * h)
        assert np.allclose(num, G[k], rtol=1e-6, atol=1e-6), (family, k)


def test_glm_takes_the_wide_form_when_asked():
    from mjhmc_amd.misc.distributions import GeneralizedLinearModel
    assert _glm('gaussian', n=1000, D=600).device_energy()[1].get('wide')               # wide, however many experts
    one = _glm('gaussian', n=100, D=5).device_energy()[1]
    assert one.get('wide') and not one.get('tall')                                      # one chunk is legal
    tall = _glm('gaussian', n=600, D=512, wide=False).device_energy()[1]
    assert tall.get('tall') and not tall.get('wide')                                    # not asked: the choice it had
    tile = _glm('gaussian', n=100, D=5, wide=False).device_energy()[1]
    assert not tile.get('tall') and not tile.get('wide')
    with pytest.raises(ValueError, match=r'512 dims.*wide=True'):                       # not asked: the refusal it had
        _glm('gaussian', wide=False)
    with pytest.raises(ValueError, match='4096 dims'):
        GeneralizedLinearModel(np.zeros((3, 4097)), np.zeros(3), 'gaussian', wide=True)


@pytest.mark.parametrize('family', ['gaussian', 'logistic'])
def test_the_passes_of_512_dims_refuse_a_wide_model_by_name(family):
    """pointwise / influence make their checks before anything runs (pointwise_request, influence_request); waic() calls
    refuse_wide first -- the same refusal through the sampler's methods is tests/test_gpu_linear_wide.py's"""
    from mjhmc_amd.samplers import markov_jump_hmc as M
    d = _glm(family)
    with pytest.raises(ValueError, match=r'pointwise: .*wide linear model.*512 dims'):
        M.pointwise_request(d, 4)
    with pytest.raises(ValueError, match=r'pointwise: .*512 dims'):
        M.pointwise_request(d, 4, values=['u'], compile_check=False)
    with pytest.raises(ValueError, match=r'influence: .*wide linear model.*512 dims'):
        M.influence_request(d, 4)
    with pytest.raises(ValueError, match=r'waic: .*512 dims'):
        M.refuse_wide(d, 'waic')
    small = _glm(family, D=5, wide=False)
    M.refuse_wide(small, 'waic')                               # not wide: nothing
    assert M.pointwise_request(small, 4, compile_check=False)[1] == [True, False]
