"""CPU: the integrated autocorrelation time from lag sums (misc.autocor.integrated_autocorrelation_time), the arithmetic and
the argument checks of Paths.lag_cov / iat / ess on a stub grid, the binding and the build wiring of csrc/lagcov.hip."""
import os
import re
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'mjhmc_amd', 'csrc')


def iat(*args):
    from mjhmc_amd.misc.autocor import integrated_autocorrelation_time
    return integrated_autocorrelation_time(*args)


def ar1_sums(phi, n, K, scale=1.0):
    """exact lag sums of an AR(1) series: A[k] = scale (n - k) phi^k, so that rho[k] = phi^k"""
    k = np.arange(K + 1)
    return scale * (n - k) * float(phi) ** k


def host_lag_sums(x, K, shift):
    """x (D, N, n) -> A (K + 1, D), S (D,) of u = x - shift[d]: the NumPy restatement"""
    u = x - shift[:, None, None]
    n = x.shape[2]
    return np.array([np.sum(u[:, :, :n - k] * u[:, :, k:], axis=(1, 2)) for k in range(K + 1)]), u.sum(axis=(1, 2))


# ---------------------------------------------------------------------------------------------------------------------
# 1.  integrated_autocorrelation_time
# ---------------------------------------------------------------------------------------------------------------------
def test_white_noise_has_tau_one():
    """phi = 0: rho_1 = 0, Gamma_0 = 1, Gamma_1 = 0, m* = 1, tau = 1"""
    A = np.stack([ar1_sums(0.0, 1000, 255), ar1_sums(0.0, 1000, 255, scale=7.5)], axis=1)
    rho, tau, window, converged = iat(A, 1000, 12)
    assert rho.shape == (256, 2) and np.array_equal(rho[0], [1.0, 1.0]) and not rho[1:].any()
    assert np.array_equal(tau, [1.0, 1.0]) and np.array_equal(window, [2, 2]) and converged.all()
    assert window.dtype.kind == 'i' and converged.dtype == bool


@pytest.mark.parametrize('phi', [0.5, 0.9])
def test_ar1_tau_is_the_closed_form_less_the_tail_the_window_cuts(phi):
    """rho_k = phi^k: every pair sum Gamma_m = phi^(2m) (1 + phi) is positive and decreasing, so m* = M = 128, the monotone
    step changes nothing and tau = -1 + 2 sum_{k < 256} phi^k = (1 + phi) / (1 - phi) - 2 phi^256 / (1 - phi): the closed form
    less the geometric tail beyond lag 255.  What is left is the rounding of 256 powers, divisions and additions: 256
    operations of relative error 2^-53 each on terms that sum to tau + 1."""
    n, K, chains = 100000, 255, 9
    A = np.stack([ar1_sums(phi, n, K), ar1_sums(phi, n, K, scale=0.03)], axis=1)
    rho, tau, window, converged = iat(A, n, chains)
    np.testing.assert_allclose(rho[:, 0], phi ** np.arange(K + 1), rtol=8 * 2.0 ** -53 * (K + 1), atol=0)
    want = (1 + phi) / (1 - phi) - 2 * phi ** (K + 1) / (1 - phi)
    assert np.all(np.abs(tau - want) <= 4 * (K + 1) * 2.0 ** -53 * (want + 1)), (tau, want)
    assert np.array_equal(window, [256, 256])
    assert not converged.any()                               # no Gamma_m <= 0 inside the window: the formula says so
    # the tail is what separates it from the closed form (visible for 0.9, below rounding for 0.5)
    assert want <= (1 + phi) / (1 - phi)


def test_a_window_that_is_too_short_is_not_converged():
    rho, tau, window, converged = iat(ar1_sums(0.99, 5000, 15), 5000, 4)
    assert rho.shape == (16, 1) and window[0] == 16 and not converged[0]
    assert 0 < tau[0] < (1 + 0.99) / (1 - 0.99)              # a lower bound of the true 199


def test_the_monotone_step_caps_a_bump():
    """rho by hand: Gamma = 1.5, 0.3, 0.6 (the bump), 0.1, -0.05 -> m* = 4, Gamma' = 1.5, 0.3, 0.3, 0.1, tau = -1 + 2 * 2.2"""
    n = 1000
    rho = np.array([1.0, 0.5, 0.2, 0.1, 0.4, 0.2, 0.06, 0.04, -0.02, -0.03, 0.5, 0.5])
    A = rho * (n - np.arange(rho.size)) / n * 3.0
    r, tau, window, converged = iat(A[:, None], n, 1)
    np.testing.assert_allclose(r[:, 0], rho, rtol=1e-14, atol=0)
    np.testing.assert_allclose(tau, [-1 + 2 * (1.5 + 0.3 + 0.3 + 0.1)], rtol=1e-14, atol=0)
    assert window[0] == 8 and converged[0]
    # without the bump nothing is capped
    rho2 = rho.copy()
    rho2[4:6] = [0.1, 0.05]
    _, tau2, _, _ = iat((rho2 * (n - np.arange(rho.size)) / n)[:, None], n, 1)
    np.testing.assert_allclose(tau2, [-1 + 2 * (1.5 + 0.3 + 0.15 + 0.1)], rtol=1e-14, atol=0)


def test_a_constant_dimension_gives_nan_without_warnings():
    A = np.stack([ar1_sums(0.5, 100, 31), np.zeros(32), ar1_sums(0.5, 100, 31)], axis=1)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        rho, tau, window, converged = iat(A, 100, 3)
        bad = A.copy()
        bad[3, 0] = np.inf
        rho_b, tau_b, window_b, converged_b = iat(bad, 100, 3)
    assert np.isnan(rho[:, 1]).all() and np.isnan(tau[1]) and window[1] == 0 and not converged[1]
    assert np.isfinite(rho[:, [0, 2]]).all() and tau[0] == tau[2] and np.isfinite(tau[0])
    assert np.isnan(tau_b[0]) and np.isnan(rho_b[:, 0]).all() and tau_b[2] == tau[2]


def test_anticorrelation_gives_tau_below_one():
    rho, tau, window, converged = iat(ar1_sums(-0.6, 4000, 255), 4000, 2)
    want = (1 - 0.6) / (1 + 0.6)
    assert tau[0] < 1 and abs(tau[0] - want) <= 1e-12


def test_no_pair_gives_nan():
    """K = 0 has no pair; a first pair that is not positive stops at m* = 0"""
    rho, tau, window, converged = iat(np.array([[2.0, 3.0]]), 5, 1)
    assert np.array_equal(rho, [[1.0, 1.0]]) and np.isnan(tau).all() and not window.any() and not converged.any()
    rho, tau, window, converged = iat(np.array([[2.0], [-2.5 * 4 / 5]]), 5, 1)        # rho_1 = -1.25: Gamma_0 < 0
    assert np.isnan(tau[0]) and window[0] == 0 and not converged[0]
    for bad in (lambda: iat(np.ones((4, 2)), 3, 1), lambda: iat(np.ones((4, 2)), 10, 0), lambda: iat(np.ones((2, 2, 2)), 10, 1)):
        with pytest.raises(ValueError):
            bad()


# ---------------------------------------------------------------------------------------------------------------------
# 2.  Paths on a stub grid
# ---------------------------------------------------------------------------------------------------------------------
class StubGrid(object):
    def __init__(self, x):
        self.x, self.ndims, self.calls = x, x.shape[0], []

    def lag_cov(self, slot0, n, max_lag, shift=None):
        self.calls.append((slot0, n, max_lag, None if shift is None else np.array(shift)))
        if not 0 <= max_lag <= min(n - 1, 256):
            raise ValueError('max_lag must be in [0, min(n - 1, 256)]')
        return host_lag_sums(self.x[:, :, slot0:slot0 + n], max_lag, np.zeros(self.ndims) if shift is None else shift)

    def close(self):
        pass


def _series(D=3, N=6, n=40, seed=2):
    rs = np.random.RandomState(seed)
    e = rs.randn(D, N, n)
    x = np.empty_like(e)
    x[:, :, 0] = e[:, :, 0]
    for t in range(1, n):
        x[:, :, t] = 0.6 * x[:, :, t - 1] + e[:, :, t]
    return x * np.array([1.0, 10.0, 0.1])[:D, None, None] + np.array([5.0, -2.0, 0.5])[:D, None, None]


def test_paths_lag_cov_iat_and_ess_on_a_stub():
    from mjhmc_amd.samplers.markov_jump_hmc import Paths
    x = _series()
    g = StubGrid(x)
    p = Paths(g, dt=0.25, n_grid=40, covered=36, mean_time=12.0, grad_evals_per_chain=300.0, n_chains=6)
    A0, S0, shift0 = p.lag_cov(5, center=False)
    assert len(g.calls) == 1 and g.calls[0][:3] == (0, 36, 5) and g.calls[0][3] is None and not shift0.any()
    wantA, wantS = host_lag_sums(x[:, :, :36], 5, np.zeros(3))
    assert np.array_equal(A0, wantA) and np.array_equal(S0, wantS)
    del g.calls[:]
    A, S, shift = p.lag_cov(7, n=30)
    assert [c[:3] for c in g.calls] == [(0, 30, 0), (0, 30, 7)] and g.calls[0][3] is None
    mean = host_lag_sums(x[:, :, :30], 0, np.zeros(3))[1] / (6.0 * 30)
    assert np.array_equal(shift, mean) and np.array_equal(g.calls[1][3], mean)
    wantA, wantS = host_lag_sums(x[:, :, :30], 7, mean)
    assert np.array_equal(A, wantA) and np.array_equal(S, wantS)
    assert np.all(np.abs(S) <= 1e-9 * np.abs(x[:, :, :30]).sum(axis=(1, 2)))       # centred

    t = p.iat()
    assert t.n == 36 and t.max_lag == 35 and t.rho.shape == (36, 3)
    rho, tau, window, converged = iat(p.lag_cov(35)[0], 36, 6)
    assert np.array_equal(t.rho, rho) and np.array_equal(t.tau, tau) and np.array_equal(t.window, window)
    assert np.array_equal(t.converged, converged)
    assert np.array_equal(t.tau_time, tau * 0.25) and np.array_equal(t.tau_grad_evals, tau * 0.25 * (300.0 / 12.0))
    # the scale of a dimension and its mean do not matter to rho: the three dimensions differ in both
    assert np.all(np.isfinite(t.tau)) and np.all(t.tau > 1)
    e = p.ess(11, n=30)
    t11 = p.iat(11, n=30)
    assert np.array_equal(e.ess, 6 * 30 / t11.tau) and np.array_equal(e.ess_per_grad, e.ess / (6 * 300.0))
    assert np.array_equal(e.tau, t11.tau) and np.array_equal(e.converged, t11.converged)

    class TwoEqualRanks(object):
        def allreduce_f64(self, v, op='sum'):
            return 2 * np.asarray(v)
    q = Paths(g, 0.25, 40, 36, 12.0, 300.0, 12, comm=TwoEqualRanks())            # two ranks with the same six chains
    Aq, Sq, shiftq = q.lag_cov(7, n=30)
    assert np.array_equal(shiftq, shift) and np.array_equal(Aq, 2 * A) and Aq.shape == (8, 3)
    np.testing.assert_allclose(q.iat(11, n=30).tau, t11.tau, rtol=1e-14, atol=0)


def test_paths_argument_checks_need_no_device():
    from mjhmc_amd.samplers.markov_jump_hmc import Paths
    g = StubGrid(_series())
    p = Paths(g, dt=0.25, n_grid=40, covered=36, mean_time=12.0, grad_evals_per_chain=300.0, n_chains=6)
    for call in (p.lag_cov, p.iat, p.ess):
        for bad in (37, 40, 0, -1):
            with pytest.raises(ValueError, match='covered'):
                call(3, n=bad)
    assert not g.calls                                        # refused before the grid was asked
    for bad in (36, -1, 300):                                 # the grid's own refusal comes through as ValueError
        with pytest.raises(ValueError, match='max_lag'):
            p.lag_cov(bad)
    with pytest.raises(ValueError, match='max_lag'):
        p.iat(30, n=30)
    p.close()
    for call in (lambda: p.lag_cov(3), lambda: p.iat(), lambda: p.ess(3)):
        with pytest.raises(ValueError, match='closed'):
            call()


def test_engine_wrappers_check_shapes_before_the_library():
    from mjhmc_amd import engine, _lib
    ctx = engine.Context.__new__(engine.Context)              # no device: anything that reached the library would fail
    ctx.lib, ctx.handle = None, None
    with pytest.raises(ValueError, match='n_dims, n_batch, n_samples'):
        ctx.lag_cov(np.zeros((3, 4)), 1)
    with pytest.raises(ValueError, match='expected shape'):
        ctx.lag_cov(np.zeros((3, 4, 5)), 1, shift=np.zeros(4))
    assert issubclass(_lib.EngineValueError, ValueError) and issubclass(_lib.EngineValueError, _lib.EngineError)
    for cls, name in ((engine.Context, 'lag_cov'), (engine.DeviceSampler, 'ring_lag_cov'), (engine.DeviceTimeGrid, 'lag_cov')):
        assert callable(getattr(cls, name))


# ---------------------------------------------------------------------------------------------------------------------
# 3.  binding, library, build wiring
# ---------------------------------------------------------------------------------------------------------------------
NEW = ('mjhmc_grid_lagcov', 'mjhmc_ring_lagcov', 'mjhmc_lagcov')


def test_binding_and_header_declare_the_entry_points():
    from mjhmc_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'mjhmc_hip.h')).read()
    assert 'mjhmc/misc/autocor.py:177-211' in header[header.index('csrc/lagcov.hip'):header.index('int mjhmc_grid_lagcov')]
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for name in NEW:
        assert re.search(r'\b%s\s*\(' % name, code), name
        assert name in _lib.PROTOTYPES, name
    assert len(_lib.PROTOTYPES['mjhmc_lagcov'][1]) == 9 and len(_lib.PROTOTYPES['mjhmc_ring_lagcov'][1]) == 7


def test_library_refuses_bad_arguments_without_a_device():
    """the checks that come before any device call: NULL handles and outputs (the range checks need a handle: GPU tests)"""
    import ctypes
    from mjhmc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    out = np.zeros(4)
    fake = ctypes.c_void_p(8)
    assert lib.mjhmc_abi_version() == 2                       # additive: no existing entry point changed
    for rc in (lib.mjhmc_grid_lagcov(None, 0, 2, 1, None, _lib.ptr(out), None),
               lib.mjhmc_grid_lagcov(fake, 0, 2, 1, None, None, None),
               lib.mjhmc_ring_lagcov(None, 0, 2, 1, None, _lib.ptr(out), None),
               lib.mjhmc_ring_lagcov(fake, 0, 2, 1, None, None, None),
               lib.mjhmc_lagcov(None, _lib.ptr(out), 1, 1, 2, 1, None, _lib.ptr(out), None),
               lib.mjhmc_lagcov(fake, None, 1, 1, 2, 1, None, _lib.ptr(out), None),
               lib.mjhmc_lagcov(fake, _lib.ptr(out), 1, 1, 2, 1, None, None, None)):
        assert rc == -1 and b'NULL argument' in lib.mjhmc_last_error()


def test_sources_are_wired_into_the_makefile():
    mk = open(os.path.join(CSRC, 'Makefile')).read()
    for var in ('SRCS', 'ASAN_SRCS'):
        m = re.search(r'^%s\s*=\s*(.*)$' % var, mk, flags=re.M)
        assert m and 'lagcov.hip' in m.group(1).split(), var
    assert mk.count('lagcov.hpp') == 3                        # a dependency of all three object rules
    assert os.path.exists(os.path.join(CSRC, 'lagcov.hip')) and os.path.exists(os.path.join(CSRC, 'lagcov.hpp'))


def test_lagcov_has_no_atomics():
    """bit-identical from run to run because nothing is added out of order: per-block partials and a second kernel"""
    src = open(os.path.join(CSRC, 'lagcov.hip')).read()
    code = re.sub(r'//[^\n]*', '', src)
    assert 'atomic' not in code.lower()
    assert 'lagcov_finish' in code and '__builtin_fma' in code
