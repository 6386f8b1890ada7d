"""CPU: the arithmetic of ``Diagnostics`` (R-hat, multi-chain ESS) from hand-made per-chain sums against direct NumPy, the
sharded reduction's packing, and the argument checks of ``diagnostics()`` that come before any device work."""
import numpy as np
import pytest


def chain_sums(X, w, c):
    """X (D, N, n) states, w (N, n) weights, c (D,) shift -> what DeviceChainStats.read() folds: (N, n, Sw, Sm, Sq, Sv)"""
    a0 = w.sum(axis=1)
    t = X - c[:, None, None]
    m = (w * t).sum(axis=2) / a0
    v = (w * t * t).sum(axis=2) / a0 - m * m
    return X.shape[1], X.shape[2], float(a0.sum()), m.sum(axis=1), (m * m).sum(axis=1), v.sum(axis=1)


def test_unit_weights_are_the_textbook_rhat_and_the_variance_of_the_chain_means():
    from mjhmc_amd.samplers.markov_jump_hmc import Diagnostics
    rs = np.random.RandomState(0)
    D, N, n = 3, 40, 12
    X = rs.randn(D, N, n) + np.array([0.5, -1.0, 2.0])[:, None, None] + 0.3 * rs.randn(1, N, 1)
    c = np.array([0.4, -0.9, 1.7])
    d = Diagnostics([chain_sums(X, np.ones((N, n)), c)], c, grad_evals=N * n * 5)
    means = X.mean(axis=2)                                    # (D, N)
    B_over_n = means.var(axis=1, ddof=1)
    W = X.var(axis=2, ddof=1).mean(axis=1)                    # the textbook within-chain variance
    var_plus = (n - 1.0) / n * W + B_over_n
    assert (d.n_chains, d.n_states, d.total_weight, d.grad_evals) == (N, n, N * n, N * n * 5)
    assert np.allclose(d.mean, means.mean(axis=1), rtol=1e-13, atol=0)
    assert np.allclose(d.chain_mean_avg, means.mean(axis=1) - c, rtol=1e-12, atol=0)
    assert np.allclose(d.between, B_over_n, rtol=1e-11, atol=0)
    assert np.allclose(d.within, X.var(axis=2).mean(axis=1), rtol=1e-11, atol=0)
    assert np.allclose(d.var_plus, var_plus, rtol=1e-11, atol=0)
    assert np.allclose(d.rhat, np.sqrt(var_plus / W), rtol=1e-11, atol=0)
    assert np.allclose(d.ess_per_chain, var_plus / B_over_n, rtol=1e-11, atol=0)
    assert np.allclose(d.ess, N * var_plus / B_over_n, rtol=1e-11, atol=0)
    assert np.allclose(d.ess_per_grad, d.ess / (N * n * 5), rtol=1e-15, atol=0)


def test_two_parts_are_twice_the_chains_and_weights_enter_through_the_chain_means():
    from mjhmc_amd.samplers.markov_jump_hmc import Diagnostics
    rs = np.random.RandomState(1)
    D, N, n = 2, 25, 8
    X = rs.randn(D, N, 2 * n)
    w = rs.standard_exponential((N, 2 * n)) + 0.1
    c = np.zeros(D)
    d = Diagnostics([chain_sums(X[:, :, :n], w[:, :n], c), chain_sums(X[:, :, n:], w[:, n:], c)], c, grad_evals=7)
    # the 2 N half chains as chains of their own
    Xh = np.concatenate([X[:, :, :n], X[:, :, n:]], axis=1)
    wh = np.concatenate([w[:, :n], w[:, n:]], axis=0)
    m = (wh * Xh).sum(axis=2) / wh.sum(axis=1)
    v = (wh * (Xh - m[:, :, None]) ** 2).sum(axis=2) / wh.sum(axis=1)
    assert (d.n_chains, d.n_states) == (2 * N, n)
    assert np.isclose(d.total_weight, w.sum(), rtol=1e-14)
    assert np.allclose(d.between, m.var(axis=1, ddof=1), rtol=1e-11, atol=0)
    assert np.allclose(d.within, v.mean(axis=1), rtol=1e-11, atol=0)
    assert np.allclose(d.rhat, np.sqrt((n - 1.0) / n * (v.mean(axis=1) + m.var(axis=1, ddof=1)) / v.mean(axis=1)), rtol=1e-11, atol=0)
    assert np.allclose(d.ess, 2 * N * (v.mean(axis=1) + m.var(axis=1, ddof=1)) / m.var(axis=1, ddof=1), rtol=1e-11, atol=0)
    assert np.allclose(d.mean, m.mean(axis=1), rtol=1e-12, atol=1e-15)


def test_sharded_reduction_adds_every_sum_in_one_collective():
    from mjhmc_amd.parallel import reduce_chain_sums

    class TwoEqualRanks(object):
        calls = 0

        def allreduce_f64(self, values, op='sum'):
            self.calls += 1
            assert op == 'sum'
            return 2.0 * np.asarray(values, dtype=np.float64)

    D = 3
    parts = [(5, 4, 1.5, np.arange(D) + 1.0, np.arange(D) + 2.0, np.arange(D) + 3.0),
             (5, 4, 2.5, np.arange(D) + 4.0, np.arange(D) + 5.0, np.arange(D) + 6.0)]
    comm = TwoEqualRanks()
    out = reduce_chain_sums(comm, parts)
    assert comm.calls == 1
    for (M, n, Sw, Sm, Sq, Sv), (M0, n0, Sw0, Sm0, Sq0, Sv0) in zip(out, parts):
        assert (M, n, Sw) == (2 * M0, n0, 2 * Sw0)
        assert np.array_equal(Sm, 2 * Sm0) and np.array_equal(Sq, 2 * Sq0) and np.array_equal(Sv, 2 * Sv0)


def test_diagnostics_argument_checks_come_before_any_device_work():
    """a sampler object that has no device at all: the ValueErrors must be raised before anything touches it"""
    from mjhmc_amd.samplers.markov_jump_hmc import HMCBase
    s = HMCBase.__new__(HMCBase)
    s._dev, s.ndims = None, 4
    for kwargs in (dict(n_iter=3), dict(n_iter=2), dict(n_iter=7), dict(n_iter=0), dict(n_iter=1, split=False),
                   dict(n_iter=0, split=False), dict(n_iter=8, shift=np.zeros(3))):
        with pytest.raises(ValueError):
            s.diagnostics(**kwargs)


def test_binding_declares_the_chainstats_entry_points_and_the_ring_write_hook():
    from mjhmc_amd import _lib, engine
    for name in ('create', 'destroy', 'set_shift', 'accumulate', 'read', 'read_chains', 'reset'):
        assert 'mjhmc_chainstats_' + name in _lib.PROTOTYPES
    assert 'mjhmc_test_ring_write' in _lib.TEST_HOOK_PROTOTYPES and 'mjhmc_test_ring_write' not in _lib.PROTOTYPES
    assert hasattr(engine, 'DeviceChainStats') and hasattr(engine.DeviceSampler, 'chain_stats')
