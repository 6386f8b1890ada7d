"""GPU: dwell-time-weighted moments and covariance from the sample ring (csrc/estimators.hip, HMCBase.expectations).

The arithmetic model every comparison uses: a device sum is a float64 sum of M = n * N terms, each term carrying at most
four roundings (two differences, the product, the weight), so per entry
    |device - host| <= (M + 4) * 2^-53 * sum |term|
with the host side computed in numpy.longdouble from the downloaded ring (ring_read / ring_read_dwell)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
LD = np.longdouble


# ---------------------------------------------------------------------------------------------------------------------
# host side of the definition
# ---------------------------------------------------------------------------------------------------------------------
def host_sums(X, w, c, want_cov):
    """X (D, n, N) float64 states, w (n, N) weights, c (D,) shift -> ((W, S1, S2, C), (|.| sums of the same terms))"""
    D = X.shape[0]
    xc = (X.astype(LD) - c.astype(LD)[:, None, None]).reshape(D, -1)
    wl = w.astype(LD).reshape(-1)
    W = wl.sum()
    t1 = xc * wl
    S1, A1 = t1.sum(axis=1), np.abs(t1).sum(axis=1)
    t2 = t1 * xc
    S2, A2 = t2.sum(axis=1), np.abs(t2).sum(axis=1)
    C = AC = None
    if want_cov:
        C = t1 @ xc.T
        AC = np.abs(t1) @ np.abs(xc).T
    return (W, S1, S2, C), (np.abs(wl).sum(), A1, A2, AC)


def assert_within_bound(dev, host, absum, M, tag):
    names = ('W', 'S1', 'S2', 'C')
    for name, d, h, a in zip(names, dev, host, absum):
        if h is None:
            assert d is None, (tag, name)
            continue
        err = np.abs(np.asarray(d).astype(LD) - h)
        bound = (M + 4) * LD(U) * a
        worst = float(np.max(err / np.where(bound > 0, bound, 1)))
        print('%s %s: max |device - host| / bound = %.3g' % (tag, name, worst))
        assert np.all(err <= bound), (tag, name, worst)


def recorded_block(s, n):
    """n + 1 recorded iterations of a jump sampler: states (D, n + 1, N), dwelling times (n + 1, N)"""
    dev = s._dev
    dev.ring_alloc(n + 1)
    s._run(n + 1, ring_slot0=0)
    s._publish()
    X = dev.ring_read(0, n + 1).reshape(dev.ndims, n + 1, dev.nparticles)
    return X, dev.ring_read_dwell(0, n + 1)


def device_sums(est, n, w_slot0, c):
    est.reset()
    est.set_shift(c)
    est.accumulate(0, n, w_slot0=w_slot0)
    W, S1, S2, C, n_states = est.read()
    return (W, S1, S2, C), n_states


def _iso(D, N, seed):
    from mjhmc_amd.misc.distributions import TestGaussian
    from mjhmc_amd.samplers.markov_jump_hmc import MarkovJumpHMC
    X0 = np.random.RandomState(seed).randn(D, N) * 1.3 + 0.5

    class Fixed(TestGaussian):
        def gen_init_X(self):
            self.Xinit = X0
    return MarkovJumpHMC(distribution=Fixed(ndims=D, nbatch=N, sigma=1.3), epsilon=0.3, beta=0.3, num_leapfrog_steps=5,
                         seed=11, resample=False)


def _pot32():
    from mjhmc_amd.misc.distributions import ProductOfT
    from mjhmc_amd.samplers.markov_jump_hmc import MarkovJumpHMC
    rs = np.random.RandomState(8)
    D, N = 36, 120
    sp = rs.rand(D, D)
    W = rs.randn(D, D)
    W[sp > 0.05] = 0
    W += np.eye(D)
    lognu = np.log(rs.rand(D) * 2 + 2.1)
    X0 = rs.randn(D, N)

    class FixedT(ProductOfT):
        def gen_init_X(self):
            self.Xinit = X0
    d = FixedT(ndims=D, nbasis=D, nbatch=N, lognu=lognu, W=W, state_dtype='float32')
    return MarkovJumpHMC(distribution=d, epsilon=0.1, beta=0.3, num_leapfrog_steps=6, seed=99, resample=False)


def _sic_bf16():
    from mjhmc_amd.misc.distributions import SparseImageCode
    from mjhmc_amd.samplers.markov_jump_hmc import MarkovJumpHMC
    from tests.helpers import sic_problem
    B, imgs, a0 = sic_problem(3, n_patches=1, n_coeffs=512)
    N = 40
    X0 = a0[:, None] + 0.3 * np.random.RandomState(8).randn(512, N)
    d = SparseImageCode(n_patches=1, n_batches=N, cauchy=True, n_basis=512, basis=B, imgs=imgs, init=X0, state_dtype='bfloat16')
    return MarkovJumpHMC(distribution=d, epsilon=0.0625, beta=0.3, num_leapfrog_steps=6, seed=3, resample=False)


CASES = {
    'iso33x100': (lambda: _iso(33, 100, 1), 6, True),          # row padding (pitch 34) and Npad > N
    'iso512x4096': (lambda: _iso(512, 4096, 2), 2, True),
    'pot36_f32': (_pot32, 5, True),
    'sic512_bf16': (_sic_bf16, 4, True),
    'iso1030_multipass': (lambda: _iso(1030, 90, 3), 3, False),  # D > 512: moments only
}


@pytest.mark.parametrize('case', sorted(CASES))
def test_definition(case):
    """W, S1, S2, C against the definition in extended precision: unit and dwell weights, zero and non-zero shift."""
    make, n, want_cov = CASES[case]
    s = make()
    X, dwell = recorded_block(s, n)
    D, N = s._dev.ndims, s._dev.nparticles
    assert np.all(np.isfinite(dwell)) and np.all(dwell[1:] > 0)
    M = n * N
    est = s._dev.estimator(want_cov)
    shifts = (np.zeros(D), X[:, 0, :].mean(axis=1) + 0.37 * np.cos(np.arange(D)))
    results = {}
    for wname, w_slot0, w in (('unit', -1, np.ones((n, N))), ('dwell', 1, dwell[1:n + 1])):
        for ci, c in enumerate(shifts):
            dev, n_states = device_sums(est, n, w_slot0, c)
            assert n_states == M
            host, absum = host_sums(X[:, :n, :], w, c, want_cov)
            assert_within_bound(dev, host, absum, M, '%s %s shift%d' % (case, wname, ci))
            results[wname, ci] = dev
            if want_cov:
                C = dev[3]
                assert np.array_equal(C, C.T), 'C is not symmetric bit for bit'
                err = np.abs(np.diag(C).astype(LD) - dev[2].astype(LD))
                assert np.all(err <= (M + 4) * LD(U) * absum[2]), 'diag(C) and S2 disagree'
    # the pairing the reference's resampler uses (slot s with dwell s) is a different estimator
    other, _ = device_sums(est, n, 0, shifts[1])
    host0, absum0 = host_sums(X[:, :n, :], dwell[:n], shifts[1], False)
    assert_within_bound(other[:3] + (None,), host0, absum0, M, case + ' pairing s/s')
    assert not np.array_equal(other[1], results['dwell', 1][1])
    est.close()


def test_determinism():
    """two fresh samplers, same seed, same calls: bit-identical sums"""
    out = []
    for _ in range(2):
        s = _iso(70, 3000, 4)
        s._dev.ring_alloc(6)
        s._run(6, ring_slot0=0)
        est = s._dev.estimator(True)
        est.set_shift(np.linspace(-1, 1, 70))
        est.accumulate(0, 3, w_slot0=1)
        est.accumulate(2, 3, w_slot0=3)
        out.append(est.read())
    for a, b in zip(*out):
        assert np.array_equal(a, b)
    assert out[0][4] == 6 * 3000


def _ref_run(n_iter):
    s = _iso(24, 301, 5)
    s.sample(n_iter, preserve_order=False)
    return s


def test_stitching_and_bookkeeping():
    """expectations(n_iter) of a jump sampler runs n_iter + 1 iterations (the last one only supplies the last holding
    time); blocks of 7 and one block of 64 give the same sums up to the order of addition, and the sampler is left as
    sample(n_iter + 1, resample=False) leaves it."""
    n_iter = 50
    res, samplers = [], []
    for block in (7, 64):
        s = _iso(24, 301, 5)
        tick0 = s._dev.get_tick()
        res.append(s.expectations(n_iter, cov=True, block=block, shift=np.full(24, 0.25)))
        assert s._dev.get_tick() - tick0 == n_iter + 1
        samplers.append(s)
    # the same run recorded in one ring, its sums on the host: both block sizes meet the bound of the definition test
    X, dwell = recorded_block(_iso(24, 301, 5), n_iter)
    host, absum = host_sums(X[:, :n_iter, :], dwell[1:n_iter + 1], np.full(24, 0.25), True)
    for block, ex in zip((7, 64), res):
        assert ex.n_states == n_iter * 301
        assert_within_bound((ex.W, ex.S1, ex.S2, ex.C), host, absum, ex.n_states, 'stitching block=%d' % block)
    ref = _ref_run(n_iter + 1)
    for s in samplers:
        assert (s.l_count, s.f_count, s.r_count, s.fl_count) == (ref.l_count, ref.f_count, ref.r_count, ref.fl_count)
        assert (s.distribution.E_count, s.distribution.dEdX_count) == (ref.distribution.E_count, ref.distribution.dEdX_count)
        assert np.array_equal(s.state.X, ref.state.X) and np.array_equal(s.state.V, ref.state.V)
        assert np.array_equal(s.dwelling_times, ref.dwelling_times)
        assert s._dev.get_tick() == ref._dev.get_tick()


def test_auto_shift_returns_moments_about_the_true_mean():
    s1, s2 = _iso(24, 301, 5), _iso(24, 301, 5)
    a = s1.expectations(30, cov=True, block=8)                      # shift: the first block's own mean
    b = s2.expectations(30, cov=True, block=8, shift=np.zeros(24))
    assert a.n_states == b.n_states and np.any(a.shift != 0)
    assert np.allclose(a.mean, b.mean, rtol=0, atol=1e-12) and np.allclose(a.var, b.var, rtol=1e-11, atol=0)
    assert np.allclose(a.cov, b.cov, rtol=0, atol=1e-11) and np.allclose(np.diag(a.cov), a.var, rtol=1e-12, atol=0)


def test_weighted_variance_is_the_pooled_dwell_weighted_variance():
    """gen_mj_init.weighted_variance against the pooled variance of the same run recorded in one ring: every value of
    every state weighted by the state's holding time (dwell slot s + 1), about the grand weighted mean"""
    from mjhmc_amd.misc.gen_mj_init import weighted_variance, online_variance
    n = 12
    s = _iso(24, 301, 5)
    got, same = weighted_variance(s, s.distribution, n)
    assert same is s and s._dev.get_tick() == _iso(24, 301, 5)._dev.get_tick() + n + 1
    X, dwell = recorded_block(_iso(24, 301, 5), n)
    x = X[:, :n, :].astype(LD)
    w = np.broadcast_to(dwell[1:n + 1].astype(LD), x.shape)
    grand = (w * x).sum() / w.sum()
    want = (w * (x - grand) ** 2).sum() / w.sum()
    print('weighted_variance %.15g, from the ring %.15g' % (got, float(want)))
    # float64 sums of M = n * N * D terms of one sign (squares) plus a handful of operations on O(1) numbers
    assert abs(got - float(want)) <= 4 * (n * 301 * 24 + 4) * U * float(want)
    # the embedded chain's (unweighted) variance is a different number
    emb, _ = online_variance(_iso(24, 301, 5), s.distribution, n)
    assert abs(emb - got) > 1e-6 * got


# ---------------------------------------------------------------------------------------------------------------------
# the law of the estimate
# ---------------------------------------------------------------------------------------------------------------------
def _z_scores(mean_hat, cov_hat, mean, cov, N):
    lam, Uv = np.linalg.eigh(cov)
    z_mean = np.abs(Uv.T @ (mean_hat - mean)) / np.sqrt(lam / N)
    z_cov = np.abs(np.einsum('di,de,ei->i', Uv, cov_hat, Uv) / lam - 1) / np.sqrt(2.0 / N)
    return float(z_mean.max()), float(z_cov.max())


def _moments(W, S1, S2, C, c):
    m1 = S1 / W
    return c + m1, C / W - np.outer(m1, m1)


def test_law_correlated_gaussian_with_negative_controls():
    """N independent stationary chains: a time average has at most the variance of one exact draw, so along every
    eigenvector of the true covariance z_mean <= 5 and z_cov <= 5 (Gaussian law and N alone).  The same recorded run with
    unit weights (the embedded chain) and with the pairing slot s / dwell s must fall OUTSIDE that bound.
    Oracle arithmetic on the CPU (NumPy seed 3): max z_mean 0.14, max z_cov 0.38; pairing s/s 20.1; unit weights 14.6.
    Device (MI355X, float32 force, counter RNG; this test prints them): expectations() z_mean 0.27, z_cov 0.49; on the
    recorded run dwell s + 1: 0.24 / 0.62, pairing s/s: z_cov 20.6, unit weights: z_cov 14.9; ControlHMC 0.09 / 0.40."""
    from mjhmc_amd.misc.distributions import CorrelatedGaussian
    from mjhmc_amd.samplers.markov_jump_hmc import MarkovJumpHMC, ControlHMC
    N, D, n_iter = 8192, 6, 200
    mean = np.array([1.0, -2.0, 0.5, 3.0, -0.7, 0.2])
    np.random.seed(3)
    d = CorrelatedGaussian(ndims=D, log_conditioning=2, nbatch=N, mean=mean)
    s = MarkovJumpHMC(distribution=d, epsilon=0.4, num_leapfrog_steps=6, beta=0.3, seed=21, resample=False)
    ex = s.expectations(n_iter, cov=True)
    assert ex.n_states == n_iter * N
    zm, zc = _z_scores(ex.mean, ex.cov, d.mean, d.cov, N)
    print('law: dwell s+1  z_mean %.3f z_cov %.3f' % (zm, zc))
    assert zm <= 5 and zc <= 5
    # negative controls on ONE recorded run
    s = MarkovJumpHMC(distribution=CorrelatedGaussian(ndims=D, log_conditioning=2, nbatch=N, mean=mean), epsilon=0.4,
                      num_leapfrog_steps=6, beta=0.3, seed=21, resample=False)
    s._dev.ring_alloc(n_iter + 1)
    s._run(n_iter + 1, ring_slot0=0)
    s._publish()
    est = s._dev.estimator(True)
    z = {}
    for name, w_slot0 in (('dwell s+1', 1), ('dwell s', 0), ('unit', -1)):
        (W, S1, S2, C), _ = device_sums(est, n_iter, w_slot0, mean)
        z[name] = _z_scores(*_moments(W, S1, S2, C, mean), d.mean, d.cov, N)
        print('law (recorded run): %-10s z_mean %.3f z_cov %.3f' % ((name,) + z[name]))
    assert z['dwell s+1'][0] <= 5 and z['dwell s+1'][1] <= 5
    assert z['dwell s'][1] > 5 and z['unit'][1] > 5
    # a discrete-time sampler's own law needs no weighting
    np.random.seed(4)
    dc = CorrelatedGaussian(ndims=D, log_conditioning=2, nbatch=N, mean=mean)
    c = ControlHMC(distribution=dc, epsilon=0.4, num_leapfrog_steps=6, beta=0.3, seed=22)
    exc = c.expectations(n_iter, cov=True)
    assert exc.n_states == n_iter * N and exc.total_weight == n_iter * N
    zm, zc = _z_scores(exc.mean, exc.cov, dc.mean, dc.cov, N)
    print('law: ControlHMC unit weights z_mean %.3f z_cov %.3f' % (zm, zc))
    assert zm <= 5 and zc <= 5


# ---------------------------------------------------------------------------------------------------------------------
# failure paths that need a sampler
# ---------------------------------------------------------------------------------------------------------------------
def test_failure_paths():
    from mjhmc_amd._lib import EngineError
    s = _iso(33, 100, 1)
    dev = s._dev
    with pytest.raises(EngineError, match='no sample ring'):
        dev.estimator(False)
    dev.ring_alloc(4)
    s._run(4, ring_slot0=0)
    est = dev.estimator(True)
    for args, msg in (((0, 5, -1), 'outside the ring'), ((3, 2, -1), 'outside the ring'), ((-1, 1, -1), 'outside the ring'),
                      ((0, 4, 1), 'dwell slots'), ((0, 1, -2), 'dwell slots'), ((0, 0, -1), 'n must be >= 1')):
        with pytest.raises(EngineError, match=msg):
            est.accumulate(args[0], args[1], w_slot0=args[2])
    est.accumulate(0, 3, w_slot0=1)
    with pytest.raises(EngineError, match='reset first'):
        est.set_shift(np.ones(33))
    with pytest.raises(ValueError):
        est.set_shift(np.ones(5))
    nocov = dev.estimator(False)
    assert nocov.read()[3] is None
    import ctypes
    buf = np.empty(33 * 33)
    W, n = ctypes.c_double(), ctypes.c_int64()
    assert dev.lib.mjhmc_estimator_read(nocov.handle, ctypes.byref(W), buf.ctypes.data, buf.ctypes.data, buf.ctypes.data,
                                        ctypes.byref(n)) == -1
    assert b'without the covariance' in dev.lib.mjhmc_last_error()
    dev.ring_alloc(9)                                               # a new ring: the estimator was sized for the old one
    with pytest.raises(EngineError, match='re-allocated'):
        est.accumulate(0, 1)
    dev.iterate(1, ring_slot0=2)                                    # the live state now sits in slot 2
    with pytest.raises(EngineError, match='live state'):
        dev.ring_copy(5, 2)
    wide = _iso(1030, 20, 3)
    wide._dev.ring_alloc(2)
    with pytest.raises(EngineError, match='at most 512 dims'):
        wide._dev.estimator(True)
    with pytest.raises(EngineError, match='at most 512 dims'):
        wide.expectations(3, cov=True)
    with pytest.raises(ValueError):
        s.expectations(0)


def test_infinite_dwell_raises_and_adds_nothing():
    """a zero total rate leaves an infinite dwelling time in the dwell ring (written here through the test build's hook)"""
    from mjhmc_amd import engine, _lib
    from tests.helpers import hooks_context
    ctx = hooks_context(0)
    D, N = 12, 70
    en = engine.DeviceEnergy(ctx, _lib.E_ISO_GAUSS, D, [1.0])
    dev = engine.DeviceSampler(en, np.random.RandomState(0).randn(D, N), seed=5, mode=_lib.MODE_MJHMC)
    dev.set_hparams(0.2, 5, 0.18, 1.0, 0.5)
    dev.ring_alloc(5)
    dev.iterate(5, ring_slot0=0)
    est = dev.estimator(True)
    est.accumulate(0, 2, w_slot0=1)
    before = est.read()
    engine.check(ctx.lib.mjhmc_test_ring_write_dwell(dev.handle, 3, 17, float('inf')), ctx.lib)
    with pytest.raises(_lib.EngineError, match='not finite'):
        est.accumulate(2, 2, w_slot0=3)
    after = est.read()
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    est.accumulate(2, 2, w_slot0=-1)                                # the flag does not stick: unit weights still work
    assert est.read()[4] == 4 * N


def test_host_energy_sampler_records_into_the_same_ring():
    """opaque callables (MJHMC_E_HOST): the iterations record state and dwelling times into the ring like every other
    sampler, so expectations() works on them"""
    from mjhmc_amd.misc.distributions import LambdaDistribution
    from mjhmc_amd.samplers.markov_jump_hmc import MarkovJumpHMC
    from mjhmc_amd import _lib
    rs = np.random.RandomState(2)
    D, N = 5, 64
    A = rs.randn(D, D)
    A = A @ A.T / D + np.eye(D)
    d = LambdaDistribution(energy_func=lambda X: 0.5 * np.sum(X * (A @ X), axis=0), energy_grad_func=lambda X: A @ X,
                           init=rs.randn(D, N))
    s = MarkovJumpHMC(distribution=d, epsilon=0.2, beta=0.3, num_leapfrog_steps=4, seed=8, resample=False)
    assert s._dev.energy.kind == _lib.E_HOST
    ex = s.expectations(6, cov=True, block=4, shift=np.zeros(D))
    n = 6
    assert ex.n_states == n * N
    # the last block (2 states) is still in the ring: slots 0 .. 1 with dwell 1 .. 2
    X = s._dev.ring_read(0, 3).reshape(D, 3, N)
    dwell = s._dev.ring_read_dwell(0, 3)
    assert np.array_equal(X[:, 2, :], s.state.X)
    est = s._dev.estimator(True)
    dev, _ = device_sums(est, 2, 1, np.zeros(D))
    host, absum = host_sums(X[:, :2, :], dwell[1:3], np.zeros(D), True)
    assert_within_bound(dev, host, absum, 2 * N, 'host energy')


# ---------------------------------------------------------------------------------------------------------------------
# column shards on one GPU (the way test_gpu_sharded.py runs them)
# ---------------------------------------------------------------------------------------------------------------------
WORKER = r'''
import sys
import numpy as np
sys.path.insert(0, %(root)r)
import torch.distributed as dist
from mjhmc_amd.parallel import Comm
from mjhmc_amd.samplers.markov_jump_hmc import MarkovJumpHMC
from mjhmc_amd.misc.distributions import TestGaussian

dist.init_process_group('gloo', init_method='tcp://127.0.0.1:%(port)d', rank=int(sys.argv[1]), world_size=2)
comm = Comm()
D, N = 24, 301
X0 = np.random.RandomState(5).randn(D, N) + 0.4


def dist_of():
    class Fixed(TestGaussian):
        def init_X(self):
            self.Xinit = X0
    return Fixed(ndims=D, nbatch=N, sigma=1.3)


def run(comm, shift, block):
    s = MarkovJumpHMC(distribution=dist_of(), epsilon=0.3, beta=0.3, num_leapfrog_steps=5,
                      seed=4242, comm=comm, resample=False)
    t0 = s._dev.get_tick()
    ex = s.expectations(20, cov=True, block=block, shift=shift)
    return s, ex, s._dev.get_tick() - t0


# rank-dependent arguments: rank 0's shift must win, and the ranks must agree on the smallest block (_run is collective:
# ranks that walked the run in different blocks would book good iterations as failed, or hang in mismatched collectives)
for shift, block in ((None, 6 + 5 * comm.rank), (np.full(D, 0.1) * (comm.rank + 1), 9 - 4 * comm.rank), (None, None)):
    s, ex, ticks = run(comm, shift, block)
    assert ticks == 21, 'a rank ran more than the 21 iterations (a replayed or retried block)'
    assert (s.epsilon, s.num_leapfrog_steps) == (0.3, 5)
    both = comm.allreduce_f64(np.concatenate([ex.shift, -ex.shift]), 'max')
    assert np.array_equal(both[:D], -both[D:]), 'the shards used different shifts'
    if shift is not None:
        assert np.array_equal(ex.shift, np.full(D, 0.1))
    if comm.rank == 0:
        s1, ex1, _ = run(None, ex.shift, 6)
        assert ex.n_states == ex1.n_states == 20 * N
        # the unsharded run recorded in one ring, its sums on the host: the reduced sums meet the definition test's bound
        from tests.test_gpu_estimators import host_sums, assert_within_bound, recorded_block
        s2 = MarkovJumpHMC(distribution=dist_of(), epsilon=0.3, beta=0.3, num_leapfrog_steps=5, seed=4242, resample=False)
        X, dwell = recorded_block(s2, 20)
        host, absum = host_sums(X[:, :20, :], dwell[1:21], ex.shift, True)
        assert_within_bound((ex.W, ex.S1, ex.S2, ex.C), host, absum, ex.n_states, 'sharded')
        assert_within_bound((ex1.W, ex1.S1, ex1.S2, ex1.C), host, absum, ex.n_states, 'unsharded')
        assert (s.l_count, s.f_count, s.r_count) == (s1.l_count, s1.f_count, s1.r_count)
        assert np.array_equal(s.dwelling_times, s1.dwelling_times)
    comm.barrier()
print('rank %%d ok' %% comm.rank)
'''


def test_sharded_sums_equal_unsharded(tmp_path):
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    script = tmp_path / 'worker.py'
    script.write_text(WORKER % dict(root=ROOT, port=port))
    procs = [subprocess.Popen([sys.executable, str(script), str(r)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(2)]
    outs = []
    for p in procs:
        try:
            out, _ = p.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(out.decode())
    for r, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and 'rank %d ok' % r in out, out[-3000:]
