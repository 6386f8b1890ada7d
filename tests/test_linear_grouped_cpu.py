"""CPU: grouped linear-model energies -- E(x) = sum_j f(u_j, j) + sum_{g<G} LSE_{c<C} u_{gC+c} (softmax regression;
mjhmc_energy_create_linear_grouped, csrc/dense_lin_grouped.hpp) -- and MultinomialLogisticRegression.
The storage order (mjhmc_linear_grouped_layout) and the hipRTC compile of the fused kernel (mjhmc_linear_grouped_check)
need no device; argument and shape checks happen before any device call."""
import ctypes
import os
import re

import numpy as np
import pytest

from mjhmc_amd import _lib, engine

HDR = _lib.KERNEL_HEADERS.encode()
ERR_INVALID, ERR_UNSUPPORTED = -1, -3     # include/mjhmc_hip.h
SOFTMAX = ('-q[0]*u', '-q[0]')


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


def pad_of(D):
    return 128 if D <= 128 else (256 if D <= 256 else 512)


def acc_row(q, h):
    """dense_pot_tile.hpp:21-23, restated: the accumulator row of register q in lane half h"""
    return (q & 3) + 8 * (q >> 2) + 4 * h


def cases():
    """the (D, C, G, K) of tests/test_gpu_linear_grouped.py's single evaluations: G = 8 Gl + 1 and 3 * 8 Gl - 2, with 0, 7
    and P + 3 plain experts behind the groups"""
    out = []
    for D, C in [(10, 2), (10, 3), (10, 10), (10, 16), (129, 5), (129, 10), (300, 3), (300, 16)]:
        P = pad_of(D)
        Gl = 16 * (P // 128) // C
        for G in (8 * Gl + 1, 3 * 8 * Gl - 2):
            for plain in (0, 7, P + 3):
                out.append((D, C, G, G * C + plain))
    return out


@pytest.mark.parametrize('D,C,G,K', cases())
def test_layout(lib, D, C, G, K):
    s2e = engine.grouped_linear_layout(D, K, (C, G), lib)
    P = pad_of(D)
    NB = P // 128
    Gl = 16 * NB // C
    nbg = -(-G // (8 * Gl))
    nbp = -(-(K - G * C) // P)
    assert s2e.shape == ((nbg + nbp) * P,)
    used = s2e[s2e >= 0]
    assert np.array_equal(np.sort(used), np.arange(K))                   # every caller j < K exactly once; the rest is -1
    assert np.all(s2e[s2e < 0] == -1)
    # the lane (blk, w, h) and the lane's slot s = NB q + r of every storage slot, from acc_row restated
    where = {}
    for blk in range(nbg):
        for w in range(4):
            for h in range(2):
                for q in range(16):
                    for r in range(NB):
                        where[blk * P + 32 * NB * w + NB * acc_row(q, h) + r] = (blk, w, h, NB * q + r)
    assert sorted(where) == list(range(nbg * P))
    lane_of = {}
    for slot, (blk, w, h, s) in where.items():
        j = int(s2e[slot])
        if j < 0:
            continue
        assert j < G * C                                                 # grouped blocks hold grouped experts only
        g, c = divmod(j, C)
        assert lane_of.setdefault(g, (blk, w, h)) == (blk, w, h)         # the members of a group share (blk, w, h)
        assert s == C * (s // C) + c and s // C < Gl                     # member c in slot C gl + c of the lane
        assert g == ((8 * blk + 2 * w + h) * Gl + s // C)                # the arithmetic of the caller's j
    assert len(lane_of) == G
    # the plain experts: blocks of their own, in the caller's order
    plain = s2e[nbg * P:]
    n_plain = K - G * C
    assert np.array_equal(plain[:n_plain], np.arange(G * C, K)) and np.all(plain[n_plain:] == -1)


def test_layout_utilisation_matches_the_formula(lib):
    """8 Gl C / P of the slots of a full grouped block are used"""
    for D in (10, 129, 300):
        P = pad_of(D)
        for C in range(2, 17):
            Gl = 16 * (P // 128) // C
            s2e = engine.grouped_linear_layout(D, 8 * Gl * C, (C, 8 * Gl), lib)
            assert s2e.shape == (P,) and np.sum(s2e >= 0) == 8 * Gl * C


@pytest.mark.parametrize('D,C', [(10, 2), (10, 10), (129, 16), (300, 3)])
def test_kernel_compiles_without_a_device(lib, D, C):
    e, g = ('q[1] != 0.f ? -q[0]*u : 0.5f*u*u', 'q[1] != 0.f ? -q[0] : u')
    assert lib.mjhmc_linear_grouped_check(D, 40 * C + 7, C, 40, e.encode(), g.encode(), HDR) == 0, lib.mjhmc_last_error()


def test_compile_errors_carry_the_compilers_message(lib):
    rc = lib.mjhmc_linear_grouped_check(36, 600, 3, 100, b'0.5f*u*v', b'u', HDR)
    assert rc == ERR_INVALID
    msg = lib.mjhmc_last_error().decode()
    assert "undeclared identifier 'v'" in msg, msg


@pytest.mark.parametrize('D,K,C,G,code,words', [
    (10, 600, 17, 10, ERR_UNSUPPORTED, 'at most 16'),
    (513, 600, 3, 10, ERR_UNSUPPORTED, 'at most 512'),
    (512, 2 ** 20, 9, 2 ** 20 // 9, ERR_UNSUPPORTED, '2^20'),        # 9 of 16 slots used: more slots than 2^20
    (10, 600, 1, 10, ERR_INVALID, 'group_size >= 2'),
    (10, 600, 3, 0, ERR_INVALID, 'n_groups >= 1'),
    (10, 600, 3, 201, ERR_INVALID, 'more than the model'),
])
def test_size_limits(lib, D, K, C, G, code, words):
    assert lib.mjhmc_linear_grouped_check(D, K, C, G, b'u', b'u', HDR) == code
    assert words in lib.mjhmc_last_error().decode(), lib.mjhmc_last_error()
    n = ctypes.c_int64(0)
    assert lib.mjhmc_linear_grouped_layout(D, K, C, G, None, ctypes.byref(n)) == code


def test_creation_checks_come_before_any_device_call(lib):
    W, b = np.ones((12, 4)), np.zeros(12)
    out = ctypes.c_void_p()
    args = (b'u', b'u', None, 0, None, 0, HDR, ctypes.byref(out))
    assert lib.mjhmc_energy_create_linear_grouped(None, 4, 12, _lib.ptr(W), _lib.ptr(b), 3, 4, *args) == ERR_INVALID    # NULL ctx
    assert lib.mjhmc_energy_create_linear_grouped(None, 4, 12, _lib.ptr(W), _lib.ptr(b), 17, 4, *args) == ERR_UNSUPPORTED
    assert lib.mjhmc_energy_create_linear_grouped(None, 4, 12, _lib.ptr(W), _lib.ptr(b), 3, 5, *args) == ERR_INVALID
    assert lib.mjhmc_linear_grouped_layout(4, 12, 3, 4, None, None) == ERR_INVALID


def test_python_argument_checks():
    from mjhmc_amd.misc.distributions import LambdaDistribution
    X0 = np.zeros((4, 8))
    W = np.ones((12, 4))
    base = dict(W=W, energy=SOFTMAX[0], grad=SOFTMAX[1])
    for groups in ((1, 4), (17, 1), (3, 0), (3, 5), 3):
        with pytest.raises(ValueError, match='group'):
            LambdaDistribution(init=X0, device_linear_grouped=dict(base, groups=groups))
    with pytest.raises(ValueError, match='groups'):
        LambdaDistribution(init=X0, device_linear_grouped=base)
    with pytest.raises(ValueError, match='one of'):
        LambdaDistribution(init=X0, device_linear_grouped=dict(base, groups=(3, 4)), device_linear_tall=base)
    with pytest.raises(ValueError, match='columns'):
        LambdaDistribution(init=np.zeros((5, 8)), device_linear_grouped=dict(base, groups=(3, 4)))
    d = LambdaDistribution(init=X0, device_linear_grouped=dict(base, groups=(3, 4)), state_dtype='float32')
    kind, params = d.device_energy()
    assert kind == _lib.E_LINEAR_EXPR and params['groups'] == (3, 4) and params['tall']


def test_the_header_declares_the_entry_points(lib):
    with open(os.path.join(os.path.dirname(_lib.KERNEL_HEADERS), '..', 'include', 'mjhmc_hip.h')) as f:
        text = f.read()
    assert re.search(r'int mjhmc_energy_create_linear_grouped\(mjhmc_ctx\* ctx, int ndims, int64_t nexperts,', text)
    assert re.search(r'int mjhmc_linear_grouped_check\(int ndims, int64_t nexperts, int group_size, int64_t n_groups,', text)
    assert re.search(r'int mjhmc_linear_grouped_layout\(int ndims, int64_t nexperts, int group_size, int64_t n_groups, int64_t\* slot_to_expert,', text)
    assert re.search(r'#define MJHMC_ABI_VERSION 2\b', text)
    for name in ('mjhmc_energy_create_linear_grouped', 'mjhmc_linear_grouped_check', 'mjhmc_linear_grouped_layout'):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)


# ---------------------------------------------------------------------------------------------------------------------
# MultinomialLogisticRegression on the host
# ---------------------------------------------------------------------------------------------------------------------
def mlr(n=40, F=3, C=4, seed=0, **kw):
    from mjhmc_amd.misc.distributions import MultinomialLogisticRegression
    rs = np.random.RandomState(seed)
    A = rs.randn(n, F)
    y = rs.randint(0, C, size=n)
    return MultinomialLogisticRegression(A, y, C, nbatch=6, seed=1, **kw)


def test_mlr_is_a_grouped_linear_model():
    d = mlr()
    n, F, C = 40, 3, 4
    kind, p = d.device_energy()
    assert kind == _lib.E_LINEAR_EXPR and p['groups'] == (C, n) and d.ndims == C * F and d.Xinit.shape == (C * F, 6)
    assert p['W'].shape == (n * C + C * F, C * F)
    i, c = 7, 2
    row = np.zeros(C * F)
    row[c * F:(c + 1) * F] = d.features[i]
    assert np.array_equal(p['W'][i * C + c], row)                                  # the row a_i in block c
    assert p['expert_params'][0][i * C + c] == float(c == d.targets[i]) and p['expert_params'][1][i * C + c] == 1.0
    assert np.array_equal(p['W'][n * C:], np.eye(C * F)) and np.all(p['expert_params'][:, n * C:] == 0)
    assert hash(d) == hash(mlr()) and hash(d) != hash(mlr(seed=1))


def test_mlr_host_energy_is_the_linear_model_form():
    """E_host against the form of the issue written out on W, b, q: sum_j f(u_j, j) + sum_g LSE, in float64"""
    d = mlr(prior_scale=0.7)
    p = d.device_energy()[1]
    C, n = p['groups']
    X = np.random.RandomState(3).randn(d.ndims, 5)
    u = p['W'].dot(X) + p['b'][:, None]
    q0, q1 = p['expert_params']
    f = np.where(q1[:, None] != 0, -q0[:, None] * u, 0.5 * u * u).sum(axis=0)
    ug = u[:n * C].reshape(n, C, -1)
    lse = np.log(np.exp(ug - ug.max(axis=1, keepdims=True)).sum(axis=1)) + ug.max(axis=1)
    assert np.allclose(d.E_host(X)[0], f + lse.sum(axis=0), rtol=1e-13, atol=0)


def test_mlr_gradient_is_the_derivative_of_the_energy():
    """Central differences of E_host with step h: the truncation error is h^2 / 6 |E'''| and the rounding error
    eps |E| / h per component.  With h = 1e-5, |E| ~ 1e2 and third derivatives of order n |a|^3 ~ 1e2 that is
    ~2e-9 + ~2e-9 absolute on gradients of order 10: the bar 1e-6 relative to max |G| leaves two orders of margin and is
    five orders below a wrong sign or a missing term (order 1)."""
    d = mlr(prior_scale=0.7)
    X = np.random.RandomState(4).randn(d.ndims, 3)
    G = d.dEdX_host(X)
    h = 1e-5
    num = np.empty_like(G)
    for k in range(d.ndims):
        e = np.zeros((d.ndims, 1))
        e[k] = h
        num[k] = (d.E_host(X + e)[0] - d.E_host(X - e)[0]) / (2 * h)
    assert np.abs(num - G).max() < 1e-6 * np.abs(G).max(), np.abs(num - G).max()


def test_mlr_is_invariant_to_a_common_shift_of_the_class_rows_up_to_the_prior():
    d = mlr(prior_scale=2.0)
    C, F = d.n_classes, d.features.shape[1]
    X = np.random.RandomState(5).randn(d.ndims, 4)
    v = np.random.RandomState(6).randn(F)
    Xs = (X.reshape(C, F, -1) + v[None, :, None]).reshape(X.shape)
    prior = lambda Z: 0.5 * np.sum(Z * Z, axis=0) / d.prior_scale ** 2        # noqa: E731
    assert np.allclose(d.E_host(X)[0] - prior(X), d.E_host(Xs)[0] - prior(Xs), rtol=1e-12, atol=1e-10)
    assert np.abs(d.E_host(X)[0] - d.E_host(Xs)[0]).min() > 1e-3              # (the prior does see the shift)
    P = d.predict_proba(X)
    assert P.shape == (40, C, 4) and np.allclose(P.sum(axis=1), 1.0) and np.allclose(P, d.predict_proba(Xs))


def test_mlr_with_two_classes_is_logistic_regression():
    """C = 2: LSE(u_0, u_1) - u_y = softplus(a.(beta_1 - beta_0)) - y a.(beta_1 - beta_0): the data term of
    GeneralizedLinearModel('logistic') at beta_1 - beta_0 (the priors differ: two N(0, s^2) rows against one)."""
    from mjhmc_amd.misc.distributions import GeneralizedLinearModel
    d = mlr(C=2)
    F = d.features.shape[1]
    glm = GeneralizedLinearModel(d.features, d.targets.astype(float), 'logistic', nbatch=4, seed=1)
    X = np.random.RandomState(7).randn(2 * F, 5)
    beta = X[F:] - X[:F]
    data = lambda m, Z: m.E_host(Z)[0] - 0.5 * np.sum(Z * Z, axis=0) / m.prior_scale ** 2      # noqa: E731
    assert np.allclose(data(d, X), data(glm, beta), rtol=1e-12, atol=1e-10)
    Gd = d.dEdX_host(X) - X / d.prior_scale ** 2
    Gg = glm.dEdX_host(beta) - beta / glm.prior_scale ** 2
    assert np.allclose(Gd[F:], Gg, rtol=1e-11, atol=1e-11) and np.allclose(Gd[:F], -Gg, rtol=1e-11, atol=1e-11)


def test_mlr_argument_validation():
    from mjhmc_amd.misc.distributions import MultinomialLogisticRegression as M
    A = np.ones((5, 3))
    y = np.array([0, 1, 2, 0, 1])
    for bad in (dict(features=np.ones(5)), dict(targets=y[:4]), dict(targets=np.array([0, 1, 3, 0, 1])),
                dict(targets=np.array([0, 1, -1, 0, 1])), dict(targets=np.array([0, 1, 1.5, 0, 1])), dict(n_classes=1),
                dict(n_classes=17), dict(prior_scale=0.0), dict(state_dtype='bfloat16'),
                dict(features=np.ones((5, 200)))):                              # 3 * 200 dims > 512
        kw = dict(dict(features=A, targets=y, n_classes=3), **bad)
        with pytest.raises(ValueError):
            M(**kw)


def test_per_expert_passes_refuse_a_grouped_model_by_name():
    """the device-free halves of pointwise / influence (the sampler methods call them first)"""
    from mjhmc_amd.samplers.markov_jump_hmc import pointwise_request, influence_request
    d = mlr()
    with pytest.raises(ValueError, match='grouped linear model'):
        pointwise_request(d, 4, values=['u'])
    with pytest.raises(ValueError, match='grouped linear model'):
        influence_request(d, 4, value='u')
