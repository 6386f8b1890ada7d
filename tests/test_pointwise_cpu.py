"""CPU: the host side of the per-expert statistics (HMCBase.pointwise / waic) -- the arithmetic of
PointwiseStatistics and Waic from hand-made sums, GeneralizedLinearModel's value expressions and constants against its own
float64 energy and scipy's densities, the refusals that need no device, and the ctypes prototypes."""
import re

import numpy as np
import pytest
from scipy import stats

from mjhmc_amd import _lib, engine
from mjhmc_amd.misc.distributions import GeneralizedLinearModel, TestGaussian
from mjhmc_amd.samplers import markov_jump_hmc as M


@pytest.fixture(scope='module', autouse=True)
def built_library():
    import os
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()


def sums_of(t, w):
    """the device sums of values t (n, K) with weights w (n,): W, S1, S2 (1, K) and the (max, sum) pair, by the book"""
    w = np.asarray(w, dtype=np.float64)
    on = w > 0
    W = w.sum()
    S1, S2 = (w[:, None] * t).sum(axis=0), (w[:, None] * t * t).sum(axis=0)
    mx = t[on].max(axis=0) if on.any() else np.full(t.shape[1], -np.inf)
    se = (w[on, None] * np.exp(t[on] - mx)).sum(axis=0) if on.any() else np.zeros(t.shape[1])
    return W, S1[None], S2[None], mx[None], se[None]


def test_statistics_from_hand_made_sums():
    rs = np.random.RandomState(0)
    t = rs.randn(50, 7)
    w = rs.rand(50)
    W, S1, S2, mx, se = sums_of(t, w)
    p = M.PointwiseStatistics(W, S1, S2, mx, se, 50, [True])
    mean = (w[:, None] * t).sum(axis=0) / w.sum()
    assert np.allclose(p.mean[0], mean, rtol=1e-14)
    assert np.allclose(p.var[0], (w[:, None] * (t - mean) ** 2).sum(axis=0) / w.sum(), rtol=1e-12)
    assert np.allclose(p.log_mean_exp[0], np.log((w[:, None] * np.exp(t)).sum(axis=0) / w.sum()), rtol=0, atol=1e-13)
    assert p.total_weight == W and p.n_states == 50
    # a row that did not ask reads NaN; a variance that rounds below zero is clipped
    q = M.PointwiseStatistics(2.0, np.array([[2.0]]), np.array([[2.0 - 1e-15]]), np.array([[-np.inf]]), np.array([[0.0]]), 2, [False])
    assert np.isnan(q.log_mean_exp[0, 0]) and q.var[0, 0] == 0.0


def test_log_mean_exp_near_minus_800_and_an_expert_without_weight():
    """values near -800: exp underflows to 0 and a plain log(mean(exp)) is -inf; the pair stays finite.  An expert whose
    states all have weight 0 reads (-inf, 0): log_mean_exp = -inf, never NaN"""
    rs = np.random.RandomState(1)
    t = -800.0 + rs.randn(40, 5)
    w = np.ones(40)
    with np.errstate(divide='ignore'):
        assert np.all(np.isneginf(np.log(np.mean(np.exp(t), axis=0))))
    W, S1, S2, mx, se = sums_of(t, w)
    p = M.PointwiseStatistics(W, S1, S2, mx, se, 40, [True])
    assert np.isfinite(p.log_mean_exp).all()
    assert np.allclose(p.log_mean_exp[0], np.log(np.mean(np.exp(t + 800.0), axis=0)) - 800.0, rtol=0, atol=1e-12)
    mx[0, 2], se[0, 2] = -np.inf, 0.0
    p = M.PointwiseStatistics(W, S1, S2, mx, se, 40, [True])
    assert np.isneginf(p.log_mean_exp[0, 2]) and np.isfinite(np.delete(p.log_mean_exp[0], 2)).all()


def test_merge_of_pairs():
    rs = np.random.RandomState(2)
    t = -800.0 + 3 * rs.randn(60, 4)
    w = rs.rand(60)
    whole = sums_of(t, w)
    a, b = sums_of(t[:25], w[:25]), sums_of(t[25:], w[25:])
    mx, se = M.merge_log_sum_exp(a[3], a[4], b[3], b[4])
    assert np.array_equal(mx, whole[3]) and np.allclose(se, whole[4], rtol=1e-13)
    # an empty pair is the identity on either side, and two empty pairs stay empty: no NaN from -inf - (-inf)
    e = (np.full((1, 4), -np.inf), np.zeros((1, 4)))
    for mx2, se2 in (M.merge_log_sum_exp(a[3], a[4], *e), M.merge_log_sum_exp(e[0], e[1], a[3], a[4])):
        assert np.array_equal(mx2, a[3]) and np.array_equal(se2, a[4])
    mx0, se0 = M.merge_log_sum_exp(e[0], e[1], *e)
    assert np.all(np.isneginf(mx0)) and np.all(se0 == 0.0)
    # the online update is the merge with a one-term pair (mx = t, se = w)
    mx1, se1 = np.array([-np.inf]), np.array([0.0])
    for k in range(60):
        mx1, se1 = M.merge_log_sum_exp(mx1, se1, t[k, :1], w[k:k + 1])
    assert mx1[0] == whole[3][0, 0] and np.isclose(se1[0], whole[4][0, 0], rtol=1e-13)


def test_waic_arithmetic():
    rs = np.random.RandomState(3)
    n, K, S = 6, 9, 200                          # 6 data rows, 3 more experts (a prior's), 200 states
    ll = -0.5 * rs.randn(S, K) ** 2
    ll[:, 1] *= 4.0                              # a row the model explains badly: its variance is above 0.4
    fit = rs.randn(S, K)
    w = rs.rand(S)
    a, b = sums_of(ll, w), sums_of(fit, w)
    p = M.PointwiseStatistics(a[0], np.vstack([a[1], b[1]]), np.vstack([a[2], b[2]]), np.vstack([a[3], np.full((1, K), -np.inf)]),
                              np.vstack([a[4], np.zeros((1, K))]), S, [True, False])
    const = rs.randn(n)
    wa = M.Waic(p, n, const)
    mean = (w[:, None] * ll).sum(axis=0) / w.sum()
    lppd = np.log((w[:, None] * np.exp(ll)).sum(axis=0) / w.sum())[:n] + const
    pw = ((w[:, None] * (ll - mean) ** 2).sum(axis=0) / w.sum())[:n]            # the population variance, not S - 1
    assert np.allclose(wa.lppd_i, lppd, atol=1e-13) and np.allclose(wa.p_waic_i, pw, rtol=1e-11)
    assert np.isclose(wa.elpd_waic, (lppd - pw).sum()) and np.isclose(wa.waic, -2 * (lppd - pw).sum())
    assert np.isclose(wa.lppd, lppd.sum()) and np.isclose(wa.p_waic, pw.sum())
    assert np.isclose(wa.se, np.sqrt(n * np.var(lppd - pw)))
    assert np.allclose(wa.fitted, ((w[:, None] * fit).sum(axis=0) / w.sum())[:n])
    assert wa.n_warn == int((pw > 0.4).sum()) and wa.n_warn >= 1
    assert wa.pointwise is p and wa.n_data == n


# ---------------------------------------------------------------------------------------------------------------------
# GeneralizedLinearModel: the value expressions restated in NumPy, against E_host and scipy
# ---------------------------------------------------------------------------------------------------------------------
def glm(family, n=40, D=5, seed=0, **kw):
    rs = np.random.RandomState(seed)
    A = rs.randn(n, D)
    eta = A.dot(0.5 * rs.randn(D))
    y = {'gaussian': eta + 0.7 * rs.randn(n), 'logistic': (rs.rand(n) < 1 / (1 + np.exp(-eta))).astype(float),
         'poisson': rs.poisson(np.exp(eta)).astype(float)}[family]
    return GeneralizedLinearModel(A, y, family, nbatch=8, seed=1, **kw)


def c_eval(expr, u, j, q):
    """a float32 C expression of the GLM's vocabulary (u, q[m], ?:, expf, log1pf, float literals) evaluated in NumPy"""
    e = re.sub(r'(\d+\.\d*|\.\d+|\d+)f\b', r'\1', expr)

    def tern(s):
        depth, k = 0, 0
        while k < len(s):                              # the first ? at depth 0 and its matching :
            depth += s[k] == '('
            depth -= s[k] == ')'
            if s[k] == '?' and depth == 0:
                d2, m = 0, k + 1
                while not (s[m] == ':' and d2 == 0):
                    d2 += s[m] == '('
                    d2 -= s[m] == ')'
                    m += 1
                return 'np.where(%s, %s, %s)' % (tern(s[:k]), tern(s[k + 1:m]), tern(s[m + 1:]))
            k += 1
        out, k = '', 0
        while k < len(s):                              # parenthesised parts may hold a ternary of their own
            if s[k] == '(':
                d2, m = 1, k + 1
                while d2:
                    d2 += s[m] == '('
                    d2 -= s[m] == ')'
                    m += 1
                out += '(' + tern(s[k + 1:m - 1]) + ')'
                k = m
            else:
                out += s[k]
                k += 1
        return out
    with np.errstate(all='ignore'):
        return eval(tern(e), dict(np=np, u=u, j=j, q=q, expf=np.exp, log1pf=np.log1p, logf=np.log))


@pytest.mark.parametrize('family', ['gaussian', 'logistic', 'poisson'])
def test_glm_values_against_the_host_energy(family):
    d = glm(family, noise_scale=0.7, prior_scale=2.0) if family == 'gaussian' else glm(family, prior_scale=2.0)
    (v0, v1), flags = d.pointwise_values()
    assert flags == [True, False]
    n, K = d.features.shape[0], d.nexperts
    X = 0.3 * np.random.RandomState(4).randn(d.ndims, 11)
    u = d.W.dot(X) + d.b[:, None]
    q = None if d.q is None else [d.q[0][:, None], d.q[1][:, None]]
    j = np.arange(K)[:, None]
    ll = c_eval(v0, u, j, q) * np.ones_like(u)
    assert np.allclose(-ll.sum(axis=0), d.E_host(X)[0], rtol=1e-12)          # -sum_j l_j = E
    fit = c_eval(v1, u, j, q) * np.ones_like(u)
    eta = d.features.dot(X)
    want = {'gaussian': eta, 'logistic': 1 / (1 + np.exp(-eta)), 'poisson': np.exp(eta)}[family]
    assert np.allclose(d.fitted_from_value(fit[:n].T).T, want, rtol=1e-12)
    if family != 'gaussian':
        assert np.all(fit[n:] == 0.0)                                        # the prior's experts have no fitted value
    # l + constants is the log-density of the data rows
    y = d.targets[:, None]
    logp = {'gaussian': lambda: stats.norm.logpdf(y, loc=eta, scale=d.noise_scale),
            'logistic': lambda: stats.bernoulli.logpmf(y, 1 / (1 + np.exp(-eta))),
            'poisson': lambda: stats.poisson.logpmf(y, np.exp(eta))}[family]()
    const = d.log_lik_constants()
    assert const.shape == (n,)
    assert np.allclose(ll[:n] + const[:, None], logp, rtol=1e-11, atol=1e-11)


# ---------------------------------------------------------------------------------------------------------------------
# refusals that need no device
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_without_a_device():
    d = glm('logistic')
    with pytest.raises(ValueError, match='n_iter must be >= 1'):
        M.pointwise_request(d, 0)
    with pytest.raises(ValueError, match='1 to 4 value expressions, got 5'):
        M.pointwise_request(d, 3, values=['u'] * 5)
    with pytest.raises(ValueError, match='1 to 4 value expressions, got 0'):
        M.pointwise_request(d, 3, values=[])
    with pytest.raises(ValueError, match='one flag per value'):
        M.pointwise_request(d, 3, values=['u', 'u*u'], log_mean_exp=[True])
    with pytest.raises(ValueError) as err:
        M.pointwise_request(d, 3, values=['u', 'no_such_symbol + u'])
    assert 'no_such_symbol' in str(err.value) and 'do not compile' in str(err.value)      # the compiler's own text
    with pytest.raises(ValueError, match='ISO_GAUSS'):
        M.pointwise_request(TestGaussian(ndims=3, nbatch=4), 3, values=['u'])
    values, flags = M.pointwise_request(d, 3)                 # the distribution's own values compile
    assert len(values) == 2 and flags == [True, False]
    values, flags = M.pointwise_request(d, 3, values='u', log_mean_exp=[True])
    assert values == ['u'] and flags == [True]


def test_check_compiles_for_square_and_tall_models():
    engine.pointwise_check(36, 36, ['u', 'q[0]*u'])               # one square block (NB = 1)
    engine.pointwise_check(300, 1100, ['(float)j'])               # tall, NB = 4
    lib = _lib.load()
    assert lib.mjhmc_pointwise_check(600, 10, b'u', _lib.KERNEL_HEADERS.encode()) == -3       # MJHMC_ERR_UNSUPPORTED
    assert lib.mjhmc_pointwise_check(10, 10, b'u;;u', _lib.KERNEL_HEADERS.encode()) == -1
    assert b'empty' in lib.mjhmc_last_error()


def test_prototypes_are_bound():
    lib = _lib.load()
    for name in ('check', 'create', 'info', 'accumulate', 'read', 'reset', 'destroy'):
        assert 'mjhmc_pointwise_' + name in _lib.PROTOTYPES
        assert hasattr(lib, 'mjhmc_pointwise_' + name)
    assert lib.mjhmc_abi_version() == 2
    assert lib.mjhmc_pointwise_destroy(None) == 0
    assert lib.mjhmc_pointwise_accumulate(None, 0, -1, 1) == -1
