"""GPU: centred linear lag sums per dimension (csrc/lagcov.hip; Context.lag_cov, DeviceSampler.ring_lag_cov,
DeviceTimeGrid.lag_cov, Paths.lag_cov / iat / ess).

The reference is NumPy float64 on the same inputs, u = x - shift[d] with the same single rounded subtraction:
    A_ref[k][d] = sum u[:, :-k] u[:, k:]      B[k][d] = sum |u[:, :-k] u[:, k:]|
and the bound is derived, not tuned: a sum of n N products added in any order, fused or not, is within
(n N + 8) 2^-53 B of the exact sum; for S it is (n N + 2) 2^-53 sum |u|."""
import numpy as np
import pytest

from tests.test_gpu_chainstats import _iso, _pot32

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -53


def host_sums(x, K, shift=None):
    """x (D, N, n) -> A (K + 1, D), B (K + 1, D), S (D,), sum |u| (D,)"""
    D, N, n = x.shape
    u = x - (np.zeros(D) if shift is None else np.asarray(shift, dtype=np.float64))[:, None, None]
    A, B = np.empty((K + 1, D)), np.empty((K + 1, D))
    for k in range(K + 1):
        prod = u[:, :, :n - k] * u[:, :, k:]
        A[k], B[k] = prod.sum(axis=(1, 2)), np.abs(prod).sum(axis=(1, 2))
    return A, B, u.sum(axis=(1, 2)), np.abs(u).sum(axis=(1, 2))


def assert_within_bound(got, x, K, shift=None, tag='', factor=1.0):
    A, S = got
    D, N, n = x.shape
    Ar, B, Sr, U = host_sums(x, K, shift)
    assert A.shape == (K + 1, D) and S.shape == (D,), tag
    assert np.isfinite(A).all() and np.isfinite(S).all(), tag + ': a value that is not finite (a padding row or column was read)'
    errA, boundA = np.abs(A - Ar), factor * (n * N + 8) * EPS * B
    errS, boundS = np.abs(S - Sr), factor * (n * N + 2) * EPS * U
    print('%s: max |A - A_ref| / bound = %.3g, max |S - S_ref| / bound = %.3g'
          % (tag, float(np.max(errA / np.maximum(boundA, 1e-300))), float(np.max(errS / np.maximum(boundS, 1e-300)))))
    assert np.all(errA <= boundA), (tag, np.argwhere(errA > boundA)[:5])
    assert np.all(errS <= boundS), (tag, np.argwhere(errS > boundS)[:5])


def synthetic(D, N, n, seed):
    """a different scale and a non-zero mean per dimension: a swapped dimension cannot pass"""
    d = np.arange(D)
    scale = 0.5 + (d % 7) + 0.01 * d
    mean = 2.0 - 0.3 * (d % 5) + 0.002 * d
    return np.random.RandomState(seed).randn(D, N, n) * scale[:, None, None] + mean[:, None, None]


def ctx():
    from mjhmc_amd import engine
    return engine.context(0)


# D: pitch > D (1, 17, 33), several particles per wave (1, 2, 4, 17, 32), one row per wave (64) and column chunks (65, 130, 512)
# N: around the padding to 64 and more than one block;  n: shorter than, equal to and across the 32-step tile
# K: 0, the band boundary from both sides (31, 32, 33), three bands (69), the last lag with one product per chain (n - 1)
CASES = [
    (1, 1, 2, 0), (1, 1, 2, 1), (1, 63, 9, 8), (1, 64, 33, 32), (1, 65, 70, 69), (1, 300, 70, 31), (1, 300, 2, 1),
    (2, 1, 9, 7), (2, 63, 2, 1), (2, 64, 70, 33), (2, 65, 33, 31), (2, 300, 9, 0), (2, 300, 70, 69), (2, 100, 33, 32),
    (17, 1, 70, 32), (17, 63, 33, 7), (17, 64, 9, 1), (17, 65, 70, 69), (17, 300, 2, 1), (17, 65, 33, 32), (17, 65, 33, 31),
    (33, 1, 33, 32), (33, 63, 70, 33), (33, 64, 2, 0), (33, 65, 9, 8), (33, 300, 70, 31), (33, 65, 70, 32), (33, 130, 33, 1),
    (512, 1, 9, 8), (512, 63, 33, 31), (512, 64, 70, 32), (512, 65, 70, 69), (512, 300, 33, 32), (512, 65, 2, 1), (512, 300, 70, 7),
    (64, 65, 33, 32), (65, 64, 33, 31), (130, 65, 9, 8), (32, 130, 70, 33), (4, 300, 33, 7),
]


@pytest.mark.parametrize('D,N,n,K', CASES)
def test_definition_on_synthetic_series(D, N, n, K):
    x = synthetic(D, N, n, 1000 * D + 10 * N + n)
    assert_within_bound(ctx().lag_cov(x, K), x, K, tag='D=%d N=%d n=%d K=%d' % (D, N, n, K))


def test_shift_and_determinism():
    D, N, n, K = 17, 65, 70, 33
    x = synthetic(D, N, n, 5)
    c = ctx()
    none = c.lag_cov(x, K)
    zero = c.lag_cov(x, K, shift=np.zeros(D))
    again = c.lag_cov(x, K)
    for a, b in ((none, zero), (none, again)):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    shift = x.mean(axis=(1, 2)) + 0.01 * np.arange(D)
    got = c.lag_cov(x, K, shift=shift)
    assert_within_bound(got, x, K, shift, tag='shifted')
    assert np.array_equal(got[0], c.lag_cov(x, K, shift=shift)[0])
    assert not np.array_equal(got[0], none[0])


# ---------------------------------------------------------------------------------------------------------------------
# rings and grids
# ---------------------------------------------------------------------------------------------------------------------
def _funnel():
    from mjhmc_amd.misc.distributions import Funnel
    from mjhmc_amd.samplers.markov_jump_hmc import MarkovJumpHMC
    np.random.seed(12)
    return MarkovJumpHMC(distribution=Funnel(ndims=32, nbatch=130), epsilon=0.1, beta=0.3, num_leapfrog_steps=5, seed=31,
                         resample=False)


SAMPLERS = {
    'control_2x100': lambda: _iso(2, 100, 3, 'ControlHMC'),
    'hmc_17x65': lambda: _iso(17, 65, 4, 'HMC'),              # N = 65: 63 padding rows in every slot
    'mjhmc_funnel_32x130': _funnel,
    'mjhmc_pot36_f32': _pot32,                                # float32 state
}


@pytest.mark.parametrize('name', sorted(SAMPLERS))
def test_paths_and_rings_against_numpy(name):
    s = SAMPLERS[name]()
    p = s.paths(40)
    n = p.covered
    assert n >= 8, n
    K = min(n - 1, 33)
    x = p.read()
    assert x.shape == (s.ndims, s.nbatch, n)
    A, S, shift = p.lag_cov(K, center=False)
    assert not shift.any()
    assert_within_bound((A, S), x, K, tag=name + ' grid, about zero')
    A, S, shift = p.lag_cov(K)
    mean = x.mean(axis=(1, 2))
    assert np.all(np.abs(shift - mean) <= 1e-12 * np.abs(x).mean(axis=(1, 2)))
    assert_within_bound((A, S), x, K, shift, tag=name + ' grid, centred')
    # the sampler's own ring: the last block of the run as recorded
    dev = s._dev
    m = dev.ring_slots
    xr = dev.ring_read(0, m, stacked=True)
    Kr = min(m - 1, 33)
    assert_within_bound(dev.ring_lag_cov(0, m, Kr), xr, Kr, tag=name + ' ring')
    c = xr.mean(axis=(1, 2))
    assert_within_bound(dev.ring_lag_cov(2, m - 3, 5, shift=c), xr[:, :, 2:m - 1], 5, c, tag=name + ' ring slots [2, m - 1)')
    p.close()


def test_sum_over_dimensions_is_the_pooled_autocorrelation():
    """shift = None: sum_d A[k][d] is mjhmc_timegrid_autocor(linear=1)[k].  n = 16 takes its direct path: both are sums of
    the same n N D products per lag, so they differ by at most the two bounds -- (n N + 8) 2^-53 B[k][d] summed over d for the
    lag sums, (n N D + 8) 2^-53 sum_d B[k][d] for the pooled one -- plus the D additions of this test's own sum over d,
    D 2^-53 sum_d |A[k][d]|.  n = 40 takes its transform path, which tests/test_gpu_autocor.py grants 1e-10 absolute on
    normalised values."""
    s = _iso(17, 65, 4, 'HMC')
    p = s.paths(40)
    assert p.covered == 40
    tg = p._grid
    D, N = 17, 65
    n = 16
    x = p.read(n)
    A, _ = tg.lag_cov(0, n, n - 1)
    pooled = tg.autocor(0, n, linear=True)
    _, B, _, _ = host_sums(x, n - 1)
    bound = (n * N + 8) * EPS * B.sum(axis=1) + (n * N * D + 8) * EPS * B.sum(axis=1) + D * EPS * np.abs(A).sum(axis=1)
    err = np.abs(A.sum(axis=1) - pooled)
    print('direct path: max err / bound = %.3g' % float(np.max(err / bound)))
    assert np.all(err <= bound)
    n = 40
    A, _ = tg.lag_cov(0, n, n - 1)
    pooled = tg.autocor(0, n, linear=True)
    mine = A.sum(axis=1)
    np.testing.assert_allclose(mine / mine[0], pooled / pooled[0], rtol=0, atol=1e-10)
    p.close()


def test_shards_add():
    """the same 130 columns as one sampler and as two of 65 with first_particle_id 0 and 65 (the counter RNG is a function
    of (seed, particle id, tick): the shards' rings are the columns of the whole ring): A1 + A2 against A within twice
    the bound"""
    from mjhmc_amd import engine, _lib
    c = ctx()
    D, N, n, K = 17, 130, 40, 33
    rs = np.random.RandomState(9)
    X0, V0 = rs.randn(D, N) * 1.3 + 0.5, rs.randn(D, N)
    en = engine.DeviceEnergy(c, _lib.E_ISO_GAUSS, D, [1.3])

    def run(cols, first):
        dev = engine.DeviceSampler(en, np.ascontiguousarray(X0[:, cols]), np.ascontiguousarray(V0[:, cols]), seed=77, first_particle_id=first, mode=_lib.MODE_MJHMC)
        dev.set_hparams(0.3, 5, 0.18, 1.0, 0.5)
        dev.ring_alloc(n)
        _, done = dev.iterate(n, ring_slot0=0)
        assert done == n
        return dev, dev.ring_read(0, n, stacked=True)

    whole, xw = run(slice(0, 130), 0)
    a, xa = run(slice(0, 65), 0)
    b, xb = run(slice(65, 130), 65)
    assert np.array_equal(xw[:, :65], xa) and np.array_equal(xw[:, 65:], xb)
    shift = xw.mean(axis=(1, 2))
    Aw, Sw = whole.ring_lag_cov(0, n, K, shift=shift)
    Aa, Sa = a.ring_lag_cov(0, n, K, shift=shift)
    Ab, Sb = b.ring_lag_cov(0, n, K, shift=shift)
    assert_within_bound((Aw, Sw), xw, K, shift, tag='unsharded')
    _, B, _, U = host_sums(xw, K, shift)
    assert np.all(np.abs(Aa + Ab - Aw) <= 2 * (n * N + 8) * EPS * B)
    assert np.all(np.abs(Sa + Sb - Sw) <= 2 * (n * N + 2) * EPS * U)
    for dev in (whole, a, b):
        dev.close()


def test_iat_and_ess_end_to_end():
    """p.iat() / p.ess() against integrated_autocorrelation_time fed with the NumPy sums of p.read().  The two can differ
    only where a Gamma_m sits within rounding of zero and flips m*: the NumPy side must show every |Gamma_m|, m <= m*,
    above 1e-6 (a condition on the input); then window and converged are equal and tau / ess agree to 1e-9 relative (the
    bound over A[0] is orders below that at these sizes)."""
    from mjhmc_amd.misc.autocor import integrated_autocorrelation_time
    s = _funnel()
    p = s.paths(40)
    n = p.covered
    assert n >= 8
    x = p.read()
    D, N = 32, 130
    K = n - 1
    mean = x.sum(axis=(1, 2)) / (float(N) * n)
    Ar, _, _, _ = host_sums(x, K, mean)
    rho, tau, window, converged = integrated_autocorrelation_time(Ar, n, N)
    M = (K + 1) // 2
    gamma = rho[0:2 * M:2] + rho[1:2 * M:2]
    for d in range(D):
        upto = min(window[d] // 2, M - 1)
        assert np.all(np.abs(gamma[:upto + 1, d]) > 1e-6), (d, gamma[:upto + 1, d])
    t = p.iat()
    assert t.max_lag == K and t.n == n
    assert np.array_equal(t.window, window) and np.array_equal(t.converged, converged)
    live = np.isfinite(tau)
    assert live.any() and np.array_equal(np.isfinite(t.tau), live)
    np.testing.assert_allclose(t.tau[live], tau[live], rtol=1e-9, atol=0)
    np.testing.assert_allclose(t.rho, rho, rtol=0, atol=1e-9)
    np.testing.assert_allclose(t.tau_time[live], tau[live] * p.dt, rtol=1e-9, atol=0)
    np.testing.assert_allclose(t.tau_grad_evals[live], tau[live] * p.dt * p.grad_evals_per_time, rtol=1e-9, atol=0)
    e = p.ess()
    np.testing.assert_allclose(e.ess[live], N * n / tau[live], rtol=1e-9, atol=0)
    np.testing.assert_allclose(e.ess_per_grad[live], N * n / tau[live] / (N * p.grad_evals_per_chain), rtol=1e-9, atol=0)
    print('funnel 32 x 130, %d grid points: tau %s, converged %d of %d' % (n, np.round(t.tau[:4], 2), int(converged.sum()), D))
    p.close()


def test_refusals_carry_the_library_message():
    from mjhmc_amd import _lib
    s = _iso(3, 65, 2)
    p = s.paths(60, n_grid=20)
    covered = p.covered
    assert 4 <= covered <= 20
    tg = p._grid
    tg.lag_cov(0, covered, covered - 1)
    if covered < 20:
        with pytest.raises(ValueError, match='covered grid'):
            tg.lag_cov(0, covered + 1, 1)
    with pytest.raises(ValueError, match='covered grid'):
        tg.lag_cov(0, 21, 1)
    with pytest.raises(ValueError, match='covered'):
        p.lag_cov(1, n=covered + 1)
    for call in (lambda: tg.lag_cov(0, covered, covered), lambda: p.lag_cov(covered), lambda: p.iat(covered),
                 lambda: tg.lag_cov(0, covered, -1), lambda: p.lag_cov(-1), lambda: s._dev.ring_lag_cov(0, 2, 2),
                 lambda: s._dev.ring_lag_cov(0, 2, -1)):
        with pytest.raises(ValueError, match=r'max_lag must be in \[0, min\(n - 1, 256\)') as ei:
            call()
        assert isinstance(ei.value, _lib.EngineError) and '(status -1)' in str(ei.value)
    long = synthetic(1, 2, 300, 1)
    ctx().lag_cov(long, 256)
    with pytest.raises(ValueError, match=r'= 256\], got 257'):
        ctx().lag_cov(long, 257)
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match=r'shift\[1\] is not finite'):
            tg.lag_cov(0, covered, 1, shift=np.array([0.0, bad, 0.0]))
        with pytest.raises(ValueError, match=r'shift\[0\] is not finite'):
            ctx().lag_cov(long, 1, shift=np.array([bad]))
    with pytest.raises(ValueError, match='outside the ring'):
        s._dev.ring_lag_cov(0, s._dev.ring_slots + 1, 1)
    with pytest.raises(ValueError, match='outside the ring'):
        s._dev.ring_lag_cov(-1, 2, 1)
    p.close()
    for call in (lambda: p.lag_cov(1), lambda: p.iat(), lambda: p.ess()):
        with pytest.raises(ValueError, match='closed'):
            call()
