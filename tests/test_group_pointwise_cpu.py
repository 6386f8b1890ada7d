"""CPU: the host side of the per-group statistics of grouped linear models (HMCBase.group_pointwise / group_waic,
mjhmc_pointwise_grouped_check / mjhmc_pointwise_create_grouped) -- the device-free compile for every group
size that has its own layout, the refusals that need no device with the codes the header documents, the ctypes prototypes,
Waic from hand-made group sums, and MultinomialLogisticRegression's value 0 against its own float64 energy."""
import re

import numpy as np
import pytest

from mjhmc_amd import _lib, engine
from mjhmc_amd.misc.distributions import GeneralizedLinearModel, MultinomialLogisticRegression, TestGaussian
from mjhmc_amd.samplers import markov_jump_hmc as M

H = _lib.KERNEL_HEADERS.encode()
INVALID, UNSUPPORTED = -1, -3              # MJHMC_ERR_INVALID, MJHMC_ERR_UNSUPPORTED (include/mjhmc_hip.h)


@pytest.fixture(scope='module', autouse=True)
def built_library():
    import os
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()


def mlr(n=40, F=3, C=4, seed=0, **kw):
    rs = np.random.RandomState(seed)
    return MultinomialLogisticRegression(rs.randn(n, F), rs.randint(0, C, size=n), C, nbatch=6, seed=1, **kw)


@pytest.mark.parametrize('D,C', [(10, 2), (10, 3), (10, 10), (129, 5), (300, 16)])
def test_check_compiles_for_every_layout(D, C):
    """the three pads (NB = 1, 2, 4), groups that fill a lane's slots (C = 2, 16) and groups that leave padding slots
    (C = 3, 5, 10), with all-group, all-member and mixed kinds: the kinds are constants of the generated source"""
    G = 8 * (16 * (1 if D <= 128 else (2 if D <= 256 else 4)) // C) + 1
    K = G * C + 7
    values = ['q[0]*(u - lse)', 'sm', '(float)c + (float)j']
    for per in (['group'] * 3, ['member'] * 3, ['group', 'member', 'group']):
        engine.group_pointwise_check(D, K, (C, G), values, per)
    engine.group_pointwise_check(D, K, (C, G), 'lse')                     # one value, every kind 'group' by default


def test_a_bad_expression_returns_the_compilers_message():
    with pytest.raises(ValueError) as err:
        engine.group_pointwise_check(10, 87, (2, 40), ['u*v'])
    assert 'the value expressions do not compile' in str(err.value) and "'v'" in str(err.value)
    lib = _lib.load()
    assert lib.mjhmc_pointwise_grouped_check(10, 87, 2, 40, b'u*v', 0, H) == INVALID
    assert lib.mjhmc_last_error().startswith(b'the value expressions do not compile')


def test_argument_refusals_return_the_documented_codes():
    lib = _lib.load()
    chk = lib.mjhmc_pointwise_grouped_check
    assert chk(10, 87, 2, 40, None, 0, H) == INVALID and chk(10, 87, 2, 40, b'u', 0, None) == INVALID
    assert chk(10, 87, 2, 40, b'u;;u', 0, H) == INVALID and b'empty' in lib.mjhmc_last_error()
    assert chk(10, 87, 2, 40, b'u;u;u;u;u', 0, H) == INVALID and b'1 to 4' in lib.mjhmc_last_error()
    assert chk(10, 87, 2, 40, b'u;sm', 4, H) == INVALID and b'per-member mask' in lib.mjhmc_last_error()
    assert chk(10, 87, 1, 40, b'u', 0, H) == INVALID and b'group_size' in lib.mjhmc_last_error()
    assert chk(10, 87, 2, 0, b'u', 0, H) == INVALID and b'n_groups' in lib.mjhmc_last_error()
    assert chk(10, 79, 2, 40, b'u', 0, H) == INVALID                                  # G C > nexperts
    assert chk(10, 1000, 17, 40, b'u', 0, H) == UNSUPPORTED and b'at most 16' in lib.mjhmc_last_error()
    assert chk(600, 87, 2, 40, b'u', 0, H) == UNSUPPORTED and b'512 dims' in lib.mjhmc_last_error()
    assert chk(10, 87, 2, 40, b'u;sm', 2, H) == 0
    import ctypes
    h = ctypes.c_void_p()
    assert lib.mjhmc_pointwise_create_grouped(None, b'u', 0, 0, H, ctypes.byref(h)) == INVALID


def test_prototypes_and_header():
    import os
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'mjhmc_hip.h')).read()
    for name in ('mjhmc_pointwise_grouped_check', 'mjhmc_pointwise_create_grouped'):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
        assert re.search(r'^int %s\(' % name, header, flags=re.M)
    assert lib.mjhmc_abi_version() == 2


def test_request_refusals_without_a_device():
    d = mlr()
    with pytest.raises(ValueError, match='n_iter must be >= 1'):
        M.group_pointwise_request(d, 0)
    with pytest.raises(ValueError, match='1 to 4 value expressions, got 5'):
        M.group_pointwise_request(d, 3, values=['u'] * 5)
    with pytest.raises(ValueError, match='1 to 4 value expressions, got 0'):
        M.group_pointwise_request(d, 3, values=[])
    with pytest.raises(ValueError, match='one flag per value'):
        M.group_pointwise_request(d, 3, values=['u', 'sm'], log_mean_exp=[True])
    with pytest.raises(ValueError, match='one kind per value'):
        M.group_pointwise_request(d, 3, values=['u', 'sm'], per=['group'])
    with pytest.raises(ValueError, match="per 'group' or per 'member', got 'row'"):
        M.group_pointwise_request(d, 3, values=['u', 'sm'], per=['group', 'row'])
    with pytest.raises(ValueError) as err:
        M.group_pointwise_request(d, 3, values=['lse', 'no_such_symbol + sm'])
    assert 'no_such_symbol' in str(err.value) and 'do not compile' in str(err.value)
    # a tall (ungrouped) model, and an energy that is no linear model, by name
    rs = np.random.RandomState(0)
    tall = GeneralizedLinearModel(rs.randn(40, 5), (rs.rand(40) < 0.5).astype(float), 'logistic', nbatch=8, seed=1)
    with pytest.raises(ValueError, match='GeneralizedLinearModel is a linear model without groups'):
        M.group_pointwise_request(tall, 3, values=['u'])
    with pytest.raises(ValueError, match='ISO_GAUSS'):
        M.group_pointwise_request(TestGaussian(ndims=3, nbatch=4), 3, values=['u'])
    values, flags, per = M.group_pointwise_request(d, 3)               # the distribution's own values compile
    assert values == ['q[0]*(u - lse)', 'sm'] and flags == [True, False] and per == ['group', 'member']
    with pytest.raises(ValueError, match='belong to values='):
        M.group_pointwise_request(d, 3, per=['group', 'member'])
    values, flags, per = M.group_pointwise_request(d, 3, values='lse', log_mean_exp=[True])
    assert values == ['lse'] and flags == [True] and per == ['group']
    # the per-expert passes still refuse the grouped model, and now name the pass that takes it
    with pytest.raises(ValueError, match='grouped linear model.*group_pointwise'):
        M.pointwise_request(d, 3, values=['u'])


def test_args():
    assert engine.group_pointwise_args(['u', 'sm', 'lse'], [True, False, True], ['group', 'member', 'member']) == (b'u;sm;lse', 5, 6)
    assert engine.group_pointwise_args('u') == (b'u', 0, 0)
    assert engine.group_pointwise_args('u', None, 'member') == (b'u', 0, 1)


def sums_of(t, w):
    """the device sums of values t (n, ...) with weights w (n,): S1, S2 and the (max, sum) pair"""
    ww = w.reshape((-1,) + (1,) * (t.ndim - 1))
    mx = t.max(axis=0)
    return (ww * t).sum(axis=0), (ww * t * t).sum(axis=0), mx, (ww * np.exp(t - mx)).sum(axis=0)


def test_waic_from_hand_made_group_sums():
    """what group_waic() builds: value 0's (G,) statistics as the one row of a Waic, the (G, C) means as ``fitted``"""
    rs = np.random.RandomState(3)
    G, C, S = 7, 3, 200
    ll = -0.5 * rs.randn(S, G) ** 2
    ll[:, 1] *= 4.0                                                    # a row whose variance is above 0.4
    sm = rs.rand(S, G, C)
    sm /= sm.sum(axis=2, keepdims=True)
    w = rs.rand(S)
    a, b = sums_of(ll, w), sums_of(sm, w)
    p0 = M.PointwiseStatistics(w.sum(), a[0], a[1], a[2], a[3], S, [True])
    p1 = M.PointwiseStatistics(w.sum(), b[0], b[1], np.full((G, C), -np.inf), np.zeros((G, C)), S, [False])
    assert p0.mean.shape == (G,) and p0.log_mean_exp.shape == (G,) and np.isfinite(p0.log_mean_exp).all()
    assert p1.mean.shape == (G, C) and np.isnan(p1.log_mean_exp).all()
    rows = M.PointwiseStatistics(p0.W, p0.S1[None], p0.S2[None], p0.lme_max[None], p0.lme_sum[None], S, p0.flags)
    const = np.zeros(G)
    wa = M.Waic(rows, G, const, p1.mean)
    mean = (w[:, None] * ll).sum(axis=0) / w.sum()
    lppd = np.log((w[:, None] * np.exp(ll)).sum(axis=0) / w.sum())
    pw = (w[:, None] * (ll - mean) ** 2).sum(axis=0) / w.sum()
    assert np.allclose(wa.lppd_i, lppd, atol=1e-13) and np.allclose(wa.p_waic_i, pw, rtol=1e-11)
    assert np.isclose(wa.elpd_waic, (lppd - pw).sum()) and wa.waic == -2.0 * wa.elpd_waic
    assert np.isclose(wa.se, np.sqrt(G * np.var(lppd - pw))) and wa.n_data == G
    assert wa.fitted.shape == (G, C) and np.allclose(wa.fitted.sum(axis=1), 1.0)
    assert np.allclose(wa.fitted, (w[:, None, None] * sm).sum(axis=0) / w.sum())
    assert wa.n_warn == int((pw > 0.4).sum()) and wa.n_warn >= 1


def test_mlr_value_0_is_minus_the_energy_without_the_prior():
    """group_values()[0] evaluated in NumPy from _logits and summed over the rows, minus the prior's term, is -E_host"""
    d = mlr(n=57, F=4, C=5, prior_scale=1.7)
    (v0, v1), flags, per = d.group_values()
    assert (v0, v1) == ('q[0]*(u - lse)', 'sm') and flags == [True, False] and per == ['group', 'member']
    assert np.array_equal(d.log_lik_constants(), np.zeros(57))
    X = 0.4 * np.random.RandomState(4).randn(d.ndims, 11)
    u = d._logits(X)                                                   # (n, C, N)
    lse, sm = d._lse(u)
    q0 = d.q[0][:57 * 5].reshape(57, 5)[:, :, None]
    ll = eval(v0, dict(q=[q0], u=u, lse=lse[:, None, :])).sum(axis=1)   # per group: summed over the members
    prior = 0.5 * (X * X).sum(axis=0) / d.prior_scale ** 2
    got, want = ll.sum(axis=0) - prior, -d.E_host(X)[0]
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    assert np.allclose(np.exp(ll), np.take_along_axis(sm, d.targets[:, None, None], axis=1)[:, 0], rtol=1e-12)
    assert np.array_equal(eval(v1, dict(sm=sm)), d.predict_proba(X))
