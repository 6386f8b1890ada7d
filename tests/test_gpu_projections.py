"""GPU: linear projections of the recorded states (csrc/projections.hpp, mjhmc_functionals_create_linear,
``DeviceSampler.projections``, ``of=sampler.projections(A, b)``).

The arithmetic contract makes one reference serve every shape: an accumulator starts at b[k] and adds the products
A[k][d] * x[d] in ascending d, each product rounded before its sum, nothing fused and nothing split -- ``numpy_loop``
restates it (NumPy's elementwise float64 operations round once each and never fuse) on the states ``ring_read`` returns
(narrow states come back widened exactly), and the comparison is ``np.array_equal`` on the float64 bit patterns."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from tests.test_gpu_chainstats import record, _iso, _same
from tests.test_gpu_marginals import _ring

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------------
# the NumPy restatement
# ---------------------------------------------------------------------------------------------------------------------
def numpy_loop(A, b, X):
    """A (K, D), b (K,) or None, X (D, n, N) float64 states as the ring holds them -> u (K, n, N):
    u = b; for d ascending: u = u + A[:, d] * X[d] -- one rounded product and one rounded sum per (k, d)"""
    K, D = A.shape
    u = np.zeros((K,) + X.shape[1:]) if b is None else np.broadcast_to(np.asarray(b, dtype=np.float64)[:, None, None], (K,) + X.shape[1:]).copy()
    for d in range(D):
        prod = A[:, d, None, None] * X[d][None]
        u = u + prod
    return u


def bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def evaluated(dev, A, b=None, n=1, link=None, params=()):
    fn = dev.projections(A, b, link, params)
    fn.ring_alloc(n)
    fn.evaluate(0, n, 0)
    return fn


def raw_slot(ctx, fn, slot, N):
    """a derived slot as it lies on the device, (Npad, pitchK) float64 (the test build's mjhmc_test_functionals_read_raw)"""
    from mjhmc_amd import engine
    Npad = (N + 63) // 64 * 64
    buf = np.full((Npad, (fn.n_values + 1) // 2 * 2), np.nan)
    assert buf.nbytes == fn.slot_bytes
    engine.check(ctx.lib.mjhmc_test_functionals_read_raw(fn.handle, slot, buf.ctypes.data, buf.nbytes), ctx.lib)
    return buf


def _pot36_f32(N=200):
    """ProductOfT 36 with float32 state: float32 rows, 36 of a 128-element pitch"""
    from mjhmc_amd.misc.distributions import ProductOfT
    from mjhmc_amd.samplers.markov_jump_hmc import MarkovJumpHMC
    rs = np.random.RandomState(8)
    D = 36
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


def _sic512_bf16(N=200):
    """SparseImageCode, 512 coefficients of a 128-pixel patch, bfloat16 state: rows of 512 elements, 8 per 16 bytes"""
    from mjhmc_amd.misc.distributions import SparseImageCode
    from mjhmc_amd.samplers.markov_jump_hmc import MarkovJumpHMC
    from tests.helpers import sic_problem
    B, imgs, a0 = sic_problem(3, n_patches=1, n_coeffs=512)
    X0 = a0[:, None] + 0.3 * np.random.RandomState(8).randn(512, N)
    d = SparseImageCode(n_patches=1, n_batches=N, cauchy=True, n_basis=512, basis=B, imgs=imgs, init=X0, state_dtype='bfloat16')
    return MarkovJumpHMC(distribution=d, epsilon=0.0625, beta=0.3, num_leapfrog_steps=6, seed=3, resample=False)


# ---------------------------------------------------------------------------------------------------------------------
# 1.  values, bit for bit, float64 state
# ---------------------------------------------------------------------------------------------------------------------
KS = [1, 3, 17, 64, 65]


@pytest.mark.parametrize('D', [1, 2, 3, 33, 130])
@pytest.mark.parametrize('N', [1, 65, 200])
def test_values_bit_for_bit_float64(D, N):
    """D: one 16-byte chunk per row (1, 2), a padded row (3, 33), a partial d chunk (every D here: the chunk is 16), more
    than one chunk (33, 130); N: a partial row tile (1), one tile plus one row (65), several workgroups (200); K: the
    16-value tile (1, 3), the 64-value tile partly filled (17), full (64) and one tile plus one value (65); odd K, whose
    padding element must read 0.0, is checked on the raw slot in section 3"""
    n = 3
    rs = np.random.RandomState(100 * D + N)
    ctx, dev, X = _ring(rs.randn(D, n, N) * 1.5)
    for K in KS:
        A, b = rs.randn(K, D), rs.randn(K)
        fn = evaluated(dev, A, b, n)
        assert fn.n_values == K and fn.slot_bytes == (N + 63) // 64 * 64 * ((K + 1) // 2 * 2) * 8
        got, want = fn.read(0, n), numpy_loop(A, b, X)
        assert got.shape == (K, n, N) and np.all(np.isfinite(got))
        bad = int(np.sum(got.view(np.uint64) != want.view(np.uint64)))
        assert bad == 0, 'D=%d N=%d K=%d: %d of %d values differ' % (D, N, K, bad, want.size)
        if K in (3, 65):
            zero = evaluated(dev, A, np.zeros(K), n).read(0, n)
            none = evaluated(dev, A, None, n).read(0, n)
            assert bits_equal(none, zero) and bits_equal(none, numpy_loop(A, None, X)), 'b=None is b = zeros'
        fn.close()


def test_values_bit_for_bit_512_directions():
    D, N, K, n = 130, 200, 512, 3
    rs = np.random.RandomState(7)
    ctx, dev, X = _ring(rs.randn(D, n, N) * 1.5)
    A, b = rs.randn(K, D), rs.randn(K)
    got = evaluated(dev, A, b, n).read(0, n)
    assert bits_equal(got, numpy_loop(A, b, X))


def test_values_bit_for_bit_wide_rows():
    """D = 1300: rows wider than the register kernels hold (Shape::wide, the multi-pass sampler), 82 d chunks"""
    D, N, K, n = 1300, 65, 3, 3
    s = _iso(D, N, 3)
    X = record(s, n)[0][:, :n, :]
    rs = np.random.RandomState(13)
    A, b = rs.randn(K, D), rs.randn(K)
    got = evaluated(s._dev, A, b, n).read(0, n)
    assert np.all(np.isfinite(got)) and bits_equal(got, numpy_loop(A, b, X))


# ---------------------------------------------------------------------------------------------------------------------
# 2.  narrow states
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['pot36_f32', 'sic512_bf16'])
def test_values_bit_for_bit_narrow_states(case):
    """float32 rows of a ProductOfT sampler and bfloat16 rows of a SparseImageCode sampler, as their samplers record them,
    widened exactly: the same NumPy loop on the widened values, bit for bit, in both tiles"""
    s = {'pot36_f32': _pot36_f32, 'sic512_bf16': _sic512_bf16}[case]()
    n = 3
    X = record(s, n)[0][:, :n, :]
    D, N = s._dev.ndims, s._dev.nparticles
    assert N == 200 and X.shape == (D, n, N) and np.any(X != 0)
    rs = np.random.RandomState(D)
    for K in (3, 65):
        A, b = rs.randn(K, D), rs.randn(K)
        got = evaluated(s._dev, A, b, n).read(0, n)
        assert np.all(np.isfinite(got))
        assert bits_equal(got, numpy_loop(A, b, X)), '%s K=%d' % (case, K)


# ---------------------------------------------------------------------------------------------------------------------
# 3.  padding and layout
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D,N,K', [(2, 1, 1), (33, 65, 3), (33, 65, 17), (130, 200, 65)])
def test_row_padding_and_the_padding_element(D, N, K):
    """the derived slot as the device holds it: elements 0 .. K - 1 of the rows p < N are the values, element K (odd K) is
    +0.0, rows p >= N stay zero -- and NaN bytes in the padding rows of the SAMPLE ring change nothing (rows p >= N are
    not read)"""
    from mjhmc_amd import engine
    n = 3
    rs = np.random.RandomState(3)
    ctx, dev, X = _ring(rs.randn(D, n, N) * 1.1)
    A, b = rs.randn(K, D), rs.randn(K)
    fn = evaluated(dev, A, b, n)
    before = fn.read(0, n)
    assert bits_equal(before, numpy_loop(A, b, X))
    for k in range(n):
        engine.check(ctx.lib.mjhmc_test_ring_fill_padding(dev.handle, k, 0xFF), ctx.lib)
    fn.evaluate(0, n, 0)
    assert bits_equal(fn.read(0, n), before)
    for k in range(n):
        rows = raw_slot(ctx, fn, k, N)
        assert bits_equal(np.ascontiguousarray(rows[:N, :K].T), before[:, k, :])
        assert not rows[:N, K:].view(np.uint64).any(), 'slot %d: a padding element is not +0.0' % k
        assert not rows[N:].view(np.uint64).any(), 'slot %d: a padding row was written' % k


def test_blocks_and_output_slots():
    """slots evaluated in blocks of 1, 2 and all give identical bits; evaluating into out_slot0 > 0 leaves the other derived
    slots untouched"""
    D, N, K, n = 33, 65, 17, 6
    rs = np.random.RandomState(5)
    ctx, dev, X = _ring(rs.randn(D, n, N))
    A, b = rs.randn(K, D), rs.randn(K)
    fn = dev.projections(A, b)
    fn.ring_alloc(n + 2)
    fn.evaluate(0, n, 0)
    whole = fn.read(0, n)
    assert bits_equal(whole, numpy_loop(A, b, X))
    for step in (1, 2):
        parts = []
        for at in range(0, n, step):
            fn.evaluate(at, step, 0)
            parts.append(fn.read(0, step))
        assert bits_equal(np.concatenate(parts, axis=1), whole), step
    fn.evaluate(0, n, 0)
    assert not np.any(fn.read(n, 2)), 'slots never written are zero'
    fn.evaluate(2, 2, n)                                   # states 2, 3 into derived slots n, n + 1
    assert bits_equal(fn.read(0, n), whole), 'the other slots are untouched'
    assert bits_equal(fn.read(n, 2), whole[:, 2:4, :])
    fn.evaluate(4, 1, 1)
    after = fn.read(0, n + 2)
    assert bits_equal(after[:, 1], whole[:, 4]) and bits_equal(after[:, 0], whole[:, 0]) and bits_equal(after[:, 2:n], whole[:, 2:n])


# ---------------------------------------------------------------------------------------------------------------------
# 4.  the link
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [3, 65])
def test_link(K):
    """'u' through hipRTC equals the library's identity kernel; an expression of + * > ?: equals the same NumPy expression
    (one IEEE operation each, nothing fused); k reaches the link"""
    D, N, n = 33, 65, 2
    rs = np.random.RandomState(K)
    ctx, dev, X = _ring(rs.randn(D, n, N))
    A, b = rs.randn(K, D), rs.randn(K)
    u = numpy_loop(A, b, X)
    ident = evaluated(dev, A, b, n).read(0, n)
    assert bits_equal(ident, u)
    assert bits_equal(evaluated(dev, A, b, n, link='u').read(0, n), ident), 'the hipRTC build against the hipcc build'
    p = [0.75, 0.5]
    got = evaluated(dev, A, b, n, link='p[0] * u * u + (u > p[1] ? 1.0 : 0.0)', params=p).read(0, n)
    want = p[0] * u * u + np.where(u > p[1], 1.0, 0.0)
    assert bits_equal(got, want)
    got = evaluated(dev, A, b, n, link='k == 1 ? -u : u').read(0, n)
    want = u.copy()
    want[1] = -u[1]
    assert bits_equal(got, want)


def test_a_value_that_is_not_finite_is_named():
    from mjhmc_amd import _lib
    from mjhmc_amd._lib import EngineError
    D, N, K, n = 33, 65, 5, 2
    rs = np.random.RandomState(2)
    ctx, dev, X = _ring(rs.randn(D, n, N))
    A = rs.randn(K, D)
    bad = dev.projections(A, None, '1.0 / (u - u)')
    bad.ring_alloc(n)
    with pytest.raises(EngineError, match='value 0 of the projections is not finite'):
        bad.evaluate(0, n, 0)
    assert dev.lib.mjhmc_functionals_evaluate(bad.handle, 0, 1, 0) == _lib.ERR_NONFINITE
    # a finite link, row 2 of A scaled to overflow: the message names value 2, not 0 -- and the flag does not stick
    big = A.copy()
    big[2] = 1e308 * np.where(rs.rand(D) < 0.5, -1.0, 1.0)
    for link in (None, 'u'):
        over = dev.projections(big, None, link)
        over.ring_alloc(n)
        with pytest.raises(EngineError, match='value 2 of the projections is not finite'):
            over.evaluate(0, n, 0)
        with pytest.raises(EngineError, match='value 2 of the projections is not finite'):
            over.evaluate(1, 1, 0)
    fine = evaluated(dev, A, None, n)
    assert bits_equal(fine.read(0, n), numpy_loop(A, None, X))


# ---------------------------------------------------------------------------------------------------------------------
# 5.  downstream equals upstream
# ---------------------------------------------------------------------------------------------------------------------
def test_accumulators_on_the_derived_ring_equal_those_on_the_sample_ring():
    """one-hot rows picking coordinates [32, 0, 7, 16, 3] of D = 33, b = 0: the derived values equal the picked
    coordinates as numbers (0.0 + 1.0 * x is exact; a -0.0 would become +0.0, which no accumulator can see).  The
    accumulators created on the projections are then compared with the same accumulators on sample rings:
      * the 33-dimensional ring itself, at the picked coordinates: per-chain sums, histogram tables and pair tables, whose
        operations per element do not depend on the row's width -- bit for bit;
      * a 5-dimensional sample ring that HOLDS the picked coordinates (the sample ring restricted to them: the row layout
        of the derived ring), same weights: estimator(cov=True), chain_stats, histogram and pair_histogram -- bit for bit,
        for unit and for dwell weights."""
    D, picks, n, N = 33, [32, 0, 7, 16, 3], 6, 301
    K = len(picks)
    rs = np.random.RandomState(17)
    w = rs.standard_exponential((n, N)) + 0.01
    ctx, dev, X = _ring(rs.randn(D, n, N) * 1.3 + 0.5, 'float64', w)
    ctx5, dev5, X5 = _ring(X[picks], 'float64', w)
    assert bits_equal(X5, X[picks])
    A = np.zeros((K, D))
    A[np.arange(K), picks] = 1.0
    fn = evaluated(dev, A, np.zeros(K), n)
    assert np.array_equal(fn.read(0, n), X[picks])
    shift = np.linspace(-0.4, 0.6, D)
    lo, hi, q = np.full(D, -4.0) - 0.01 * np.arange(D), np.full(D, 4.5) + 0.02 * np.arange(D), 2.0 ** -22
    pairs_dn = np.array([(0, 1), (4, 2), (3, 3)])
    pairs_up = np.asarray(picks)[pairs_dn]
    up = (dev.chain_stats(1), dev.histogram(64, lo, hi, q), dev.pair_histogram(pairs_up, 16, lo[pairs_up], hi[pairs_up], q))
    dn = (fn.chain_stats(1), fn.histogram(64, lo[picks], hi[picks], q),
          fn.pair_histogram(pairs_dn, 16, lo[pairs_up], hi[pairs_up], q), fn.estimator(True))
    r5 = (dev5.chain_stats(1), dev5.histogram(64, lo[picks], hi[picks], q),
          dev5.pair_histogram(pairs_dn, 16, lo[pairs_up], hi[pairs_up], q), dev5.estimator(True))
    assert all(h.ndims == K for h in dn)
    up[0].set_shift(shift)
    for h in (dn[0], dn[3], r5[0], r5[3]):
        h.set_shift(shift[picks])
    for slot0 in (-1, 0):
        for h in up + dn + r5:
            h.reset()
            h.accumulate(0, n, w_slot0=slot0)
        a0u, a1u, a2u = up[0].read_chains()
        a0d, a1d, a2d = dn[0].read_chains()
        assert np.array_equal(a0u, a0d) and np.array_equal(a1u[picks], a1d) and np.array_equal(a2u[picks], a2d), slot0
        cu, mu, Wu, nu = up[1].read()
        cd, md, Wd, nd = dn[1].read()
        assert np.array_equal(cu[picks], cd) and np.array_equal(mu[picks], md) and (Wu, nu) == (Wd, nd), slot0
        assert cd.sum() == K * n * N
        pu, pd = up[2].read(), dn[2].read()
        assert np.array_equal(pu[0], pd[0]) and np.array_equal(pu[1], pd[1]) and pu[2:] == pd[2:], slot0
        # the 5-dimensional sample ring: the same layout, the same bits, the pooled moments and the covariance included
        assert _same(dn[0].read_chains(), r5[0].read_chains()) and dn[0].read(0)[:3] == r5[0].read(0)[:3], slot0
        assert _same(dn[0].read(0)[3:], r5[0].read(0)[3:]), slot0
        for i in (1, 2):
            a, b5 = dn[i].read(), r5[i].read()
            assert np.array_equal(a[0], b5[0]) and np.array_equal(a[1], b5[1]) and a[2:] == b5[2:], (i, slot0)
        Wd_, S1d, S2d, Cd, nsd = dn[3].read()
        W5, S15, S25, C5, ns5 = r5[3].read()
        assert (Wd_, nsd) == (W5, ns5) and nsd == n * N
        assert bits_equal(S1d, S15) and bits_equal(S2d, S25) and bits_equal(Cd, C5), slot0


# ---------------------------------------------------------------------------------------------------------------------
# 6.  the drivers
# ---------------------------------------------------------------------------------------------------------------------
def _same_run(s, t):
    assert (s.l_count, s.f_count, s.r_count, s.fl_count) == (t.l_count, t.f_count, t.r_count, t.fl_count)
    assert (s.distribution.E_count, s.distribution.dEdX_count) == (t.distribution.E_count, t.distribution.dEdX_count)
    assert np.array_equal(s.state.X, t.state.X) and np.array_equal(s.state.V, t.state.V)
    assert s._dev.get_tick() == t._dev.get_tick()
    if s._dwell_weighted:
        assert np.array_equal(s.dwelling_times, t.dwelling_times)


@pytest.mark.parametrize('cls', ['MarkovJumpHMC', 'ControlHMC', 'HMC'])
def test_drivers(cls):
    """every driver with ``of=P`` against a same-seed twin with ``of=None`` (the same run), against a second ``of=P`` run
    (the same bits), and against its accumulator driven by hand on a twin that recorded the whole run in one ring and
    evaluated the same projections block by block as the driver does"""
    D, N, n, K = 7, 301, 20, 5
    rs = np.random.RandomState(31)
    A, b = rs.randn(K, D), rs.randn(K)
    new = lambda: _iso(D, N, 5, cls)
    m = new()
    P = m.projections(A, b, names=['a%d' % k for k in range(K)])
    assert P.n_values == K and P.names[0] == 'a0'
    lead = 1 if m._dwell_weighted else 0
    X, w, w_slot0 = record(m, n)
    fn = m._dev.projections(A, b)
    fn.ring_alloc(n)
    fn.evaluate(0, n, 0)
    V = fn.read(0, n)
    assert bits_equal(V, numpy_loop(A, b, X[:, :n, :]))
    shift = np.linspace(-0.3, 0.4, K)

    def blocks(length, block, at=0):
        while length > 0:
            k = min(block, length)
            yield at, k
            at, length = at + k, length - k

    # expectations
    s, t, again = new(), new(), new()
    tick0 = s._dev.get_tick()
    with pytest.raises(ValueError):
        s.expectations(n, of=P, shift=np.zeros(D))
    assert (s._dev.get_tick(), s._dev.ring_slots) == (tick0, 0)
    e = s.expectations(n, cov=True, block=7, shift=shift, of=P)
    t.expectations(n, cov=True, block=7)
    _same_run(s, t)
    assert s._dev.get_tick() - tick0 == n + lead
    assert e.n_states == n * N and e.mean.shape == (K,) and e.cov.shape == (K, K)
    e2 = again.expectations(n, cov=True, block=7, shift=shift, of=P)
    _same_run(again, t)
    est = fn.estimator(True)
    est.set_shift(shift)
    for at, k in blocks(n, 7):
        fn.evaluate(at, k, 0)
        est.accumulate(0, k, w_slot0=at + 1 if lead else -1)
    W, S1, S2, C, n_states = est.read()
    for other in ((e2.W, e2.S1, e2.S2, e2.C, e2.n_states), (W, S1, S2, C, n_states)):
        assert e.W == other[0] and e.n_states == other[4]
        assert bits_equal(e.S1, other[1]) and bits_equal(e.S2, other[2]) and bits_equal(e.C, other[3])
    auto = s.expectations(n, block=8, of=P)                # the first block's own mean as the shift
    t.expectations(n, block=8)
    _same_run(s, t)
    assert auto.shift.shape == (K,) and np.any(auto.shift != 0)
    fn.evaluate(0, n, 0)

    # diagnostics: per-chain sums run over a chain's states in order whatever the blocks
    s, t, again = new(), new(), new()
    d = s.diagnostics(n, split=True, block=4, shift=shift, of=P)
    dt = t.diagnostics(n, split=True, block=4)
    _same_run(s, t)
    assert (d.n_chains, d.n_states) == (2 * N, n // 2) and d.mean.shape == (K,) and d.grad_evals == dt.grad_evals
    cs = fn.chain_stats(2)
    cs.set_shift(shift)
    for part, (at, k) in enumerate(blocks(n, n // 2)):
        cs.accumulate(at, k, w_slot0=at + 1 if lead else -1, part=part)
    for part in range(2):
        by_hand = cs.read(part)
        assert d.parts[part][:3] == by_hand[:3] and _same(d.parts[part][3:], by_hand[3:]), part
    for blk in (1, None):
        o = again if blk is None else new()
        d2 = o.diagnostics(n, split=True, block=blk, shift=shift, of=P)
        _same_run(o, t)
        assert d2.Sw == d.Sw and _same((d2.Sm, d2.Sq, d2.Sv), (d.Sm, d.Sq, d.Sv)), blk
        assert bits_equal(d2.rhat, d.rhat) and bits_equal(d2.ess, d.ess)

    # marginals: integer tables
    lo, hi = np.full(K, -12.0) - 0.1 * np.arange(K), np.full(K, 12.5)
    s, t, again = new(), new(), new()
    mg = s.marginals(n, bins=48, range=(lo, hi), block=6, of=P)
    t.marginals(n, bins=48, range=(-6.0, 6.0), block=6)
    _same_run(s, t)
    assert mg.ndims == K and mg.n_states == n * N and mg.counts.shape == (K, 50)
    hist = fn.histogram(48, lo, hi, mg.quantum)
    hist.accumulate(0, n, w_slot0=w_slot0)
    c, u, Wu, ns = hist.read()
    assert np.array_equal(mg.counts, c) and np.array_equal(mg.units, u) and (mg.W_units, mg.n_states) == (Wu, ns)
    assert mg.counts[:, 1:-1].sum() > 0.9 * K * n * N
    m2 = again.marginals(n, bins=48, range=(lo, hi), block=6, of=P)
    assert m2.quantum == mg.quantum and np.array_equal(m2.counts, mg.counts) and np.array_equal(m2.units, mg.units)
    o = new()
    m3 = o.marginals(n, bins=48, range=(lo, hi), block=None, of=P)
    _same_run(o, t)
    assert np.array_equal(m3.counts, mg.counts), 'the counts do not depend on the blocks'
    if m3.quantum == mg.quantum:                           # (a jump sampler takes the quantum from its first block's weights)
        assert np.array_equal(m3.units, mg.units) and m3.W_units == mg.W_units
    else:
        assert lead
    auto = s.marginals(n, bins=32, of=P)                   # range and quantum from the first block's moments
    t.marginals(n, bins=32)
    _same_run(s, t)
    assert auto.lo.shape == (K,) and np.all(auto.lo < auto.hi) and np.all(auto.out_of_range <= 1.0 / 64)

    # joint marginals
    pairs = np.array([(0, 2), (4, 1)])
    s, t, again = new(), new(), new()
    jm = s.joint_marginals(n, pairs=pairs, bins=16, range=(lo, hi), block=6, of=P)
    t.joint_marginals(n, pairs=pairs, bins=16, range=(-6.0, 6.0), block=6)
    _same_run(s, t)
    assert jm.n_states == n * N and jm.counts.shape == (2, 18, 18)
    ph = fn.pair_histogram(pairs, 16, lo[pairs], hi[pairs], jm.quantum)
    ph.accumulate(0, n, w_slot0=w_slot0)
    c, u, Wu, ns = ph.read()
    assert np.array_equal(jm.counts, c) and np.array_equal(jm.units, u) and (jm.W_units, jm.n_states) == (Wu, ns)
    j2 = again.joint_marginals(n, pairs=pairs, bins=16, range=(lo, hi), block=6, of=P)
    assert j2.quantum == jm.quantum and np.array_equal(j2.counts, jm.counts) and np.array_equal(j2.units, jm.units)
    o = new()
    j3 = o.joint_marginals(n, pairs=pairs, bins=16, range=(lo, hi), block=None, of=P)
    _same_run(o, t)
    assert np.array_equal(j3.counts, jm.counts)


# ---------------------------------------------------------------------------------------------------------------------
# 7.  a known answer
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cls', ['MarkovJumpHMC', 'ControlHMC'])
def test_known_answer_along_a_random_direction(cls):
    """x ~ N(0, I_17), a a unit vector: a . x + 3 is N(3, 1).  1000 chains after burn_in(), 64 states: with se =
    sqrt(var_plus / ess) from diagnostics(64, of=P), |mean - 3| <= 5 se and 5 se <= 0.05 (the second condition gives the
    first its power); rhat < 1.05; and from expectations(64, of=P) on the continuing run |var - 1| <= 0.1"""
    from mjhmc_amd.misc.distributions import TestGaussian
    from mjhmc_amd.samplers import markov_jump_hmc as mj
    np.random.seed(12)
    kw = dict(resample=False) if cls == 'MarkovJumpHMC' else {}
    s = getattr(mj, cls)(distribution=TestGaussian(ndims=17, nbatch=1000, sigma=1.0), epsilon=0.4, beta=0.3,
                         num_leapfrog_steps=4, seed=2024, **kw)
    s.burn_in()
    a = np.random.RandomState(4).randn(17)
    a /= np.sqrt(a.dot(a))
    P = s.projections(a, b=3.0)
    assert P.n_values == 1
    d = s.diagnostics(64, of=P)
    se = np.sqrt(d.var_plus / d.ess)
    ex = s.expectations(64, of=P)
    print('%s: mean %r, se %r, ess %r, rhat %r, var %r' % (cls, d.mean, se, d.ess, d.rhat, ex.var))
    assert d.mean.shape == (1,) and np.all(np.isfinite(se))
    assert abs(d.mean[0] - 3.0) <= 5 * se[0] and 5 * se[0] <= 0.05
    assert d.rhat[0] < 1.05
    assert abs(ex.var[0] - 1.0) <= 0.1


# ---------------------------------------------------------------------------------------------------------------------
# 8.  principal axes
# ---------------------------------------------------------------------------------------------------------------------
def test_principal_axes_whiten_a_correlated_gaussian():
    """CorrelatedGaussian, D = 8, covariance spectrum 0.1 .. 10 (condition number 100), 1000 chains started from the law
    itself: the principal axes of a first run of 64 states, whitened, turn the covariance of a second run into the
    identity within 0.25 (max-abs) and its mean into zero within 5 / sqrt(ess) per axis, ess from diagnostics(64, of=P).
    The bounds test the wiring -- rotation, b, whitening -- not the sampler."""
    from mjhmc_amd.misc.distributions import CorrelatedGaussian
    from mjhmc_amd.samplers.markov_jump_hmc import MarkovJumpHMC, Projections
    np.random.seed(5)
    dist = CorrelatedGaussian(ndims=8, nbatch=1000, log_conditioning=2, seed=2)
    lam = np.linalg.eigvalsh(dist.cov)
    assert lam[-1] / lam[0] >= 100 * (1 - 1e-9)
    s = MarkovJumpHMC(distribution=dist, epsilon=0.15, beta=0.3, num_leapfrog_steps=5, seed=23, resample=False)
    ex = s.expectations(64, cov=True)
    P = Projections.principal(ex, whiten=True)
    assert P.n_values == 8 and np.max(np.abs(P.A @ ex.cov @ P.A.T - np.eye(8))) <= 1e-10
    ew = s.expectations(64, cov=True, of=P)
    d = s.diagnostics(64, of=P)
    dev_cov = np.max(np.abs(ew.cov - np.eye(8)))
    print('principal axes: max |cov - I| = %.4f, mean %r, 5 / sqrt(ess) %r, rhat %r' % (dev_cov, ew.mean, 5 / np.sqrt(d.ess), d.rhat))
    assert dev_cov <= 0.25
    assert np.all(np.abs(ew.mean) <= 5 / np.sqrt(d.ess))


# ---------------------------------------------------------------------------------------------------------------------
# 9.  refusals on the device
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from mjhmc_amd._lib import EngineError
    D, N = 33, 100
    s = _iso(D, N, 1)
    dev = s._dev
    rs = np.random.RandomState(0)
    A = rs.randn(4, D)
    with pytest.raises(EngineError, match='no sample ring'):
        dev.projections(A)
    dev.ring_alloc(4)
    s._run(4, ring_slot0=0)
    with pytest.raises(EngineError, match=r'K must be in \[1, 512\], got 513'):
        dev.projections(rs.randn(513, D))
    with pytest.raises(ValueError, match=r'\(K, ndims = 33\)'):
        dev.projections(rs.randn(4, D + 1))
    for what, args in ((r'A\[1\]\[2\] is not finite', (np.where(np.arange(4 * D).reshape(4, D) == D + 2, np.nan, A),)),
                       (r'b\[3\] is not finite', (A, np.array([0.0, 0.0, 0.0, np.inf]))),
                       (r'p\[1\] is not finite', (A, None, 'u + p[0]', [1.0, -np.inf]))):
        with pytest.raises(EngineError, match=what):
            dev.projections(*args)
    with pytest.raises(EngineError, match="undeclared identifier 'y'"):
        dev.projections(A, None, 'u * y')
    fn = dev.projections(A)
    with pytest.raises(EngineError, match='no derived ring'):
        fn.evaluate(0, 1, 0)
    with pytest.raises(EngineError, match='no derived ring'):
        fn.estimator()
    fn.ring_alloc(3)
    fn.evaluate(1, 3, 0)
    for args, msg in (((0, 5, 0), 'outside the ring of 4'), ((2, 3, 0), 'outside the ring of 4'), ((-1, 1, 0), 'outside the ring'),
                      ((0, 4, 0), 'outside the derived ring of 3'), ((0, 2, 2), 'outside the derived ring of 3'),
                      ((0, 1, -1), 'outside the derived ring'), ((0, 0, 0), 'n must be >= 1')):
        with pytest.raises(EngineError, match=msg):
            fn.evaluate(*args)
    est = fn.estimator(True)
    est.accumulate(0, 3, w_slot0=1)
    assert est.read()[4] == 3 * N
    dev.ring_alloc(9)                                      # a new sample ring: the projections were created on the old one
    with pytest.raises(EngineError, match='sample ring was re-allocated'):
        fn.evaluate(0, 1, 0)
    fn.close()
    est.close()
    # the sampler works afterwards
    s._run(4, ring_slot0=0)
    s._publish()
    X = dev.ring_read(0, 4).reshape(D, 4, N)
    assert bits_equal(evaluated(dev, A, None, 4).read(0, 4), numpy_loop(A, None, X))
    e = s.expectations(6, of=s.projections(A))
    assert e.mean.shape == (4,) and np.all(np.isfinite(e.mean))
    keep = dev.projections(A)
    dev.close()                                            # the sampler frees the handle and its device copies
    keep.close()


def test_a_host_evaluated_energy_is_accepted():
    """only the ring is read: an energy given as opaque Python callables has projections like any other"""
    from mjhmc_amd.misc.distributions import LambdaDistribution
    from mjhmc_amd.samplers.markov_jump_hmc import MarkovJumpHMC
    Q = np.array([[2.0, 0.5], [0.5, 1.0]])
    d = LambdaDistribution(energy_func=lambda X: 0.5 * np.sum(X * Q.dot(X), axis=0).reshape(1, -1),
                           energy_grad_func=lambda X: Q.dot(X), init=np.random.RandomState(1).randn(2, 70), name='dense quadratic')
    h = MarkovJumpHMC(distribution=d, epsilon=0.2, beta=0.3, num_leapfrog_steps=3, seed=5, resample=False)
    A, b = np.array([[1.0, -1.0], [0.5, 0.25], [0.0, 2.0]]), np.array([0.1, 0.2, 0.3])
    X = record(h, 3)[0][:, :3, :]
    assert bits_equal(evaluated(h._dev, A, b, 3).read(0, 3), numpy_loop(A, b, X))


# ---------------------------------------------------------------------------------------------------------------------
# 10.  column shards on one GPU (the harness of tests/test_gpu_functionals.py::test_sharded_functionals_equal_unsharded)
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
D, N, n_iter, K = 33, 301, 20, 5
X0 = np.random.RandomState(5).randn(D, N) + 0.4
rs = np.random.RandomState(6)
A, b = rs.randn(K, D), rs.randn(K)


def dist_of():
    class Fixed(TestGaussian):
        def init_X(self):
            self.Xinit = X0
    return Fixed(ndims=D, nbatch=N, sigma=1.3)


def make(comm):
    return MarkovJumpHMC(distribution=dist_of(), epsilon=0.3, beta=0.3, num_leapfrog_steps=5, seed=4242, comm=comm,
                         resample=False)


# rank-dependent arguments: rank 0's shift must win, and the ranks must agree on the smallest block
for shift0, block, agreed in ((None, 4 + 3 * comm.rank, 4), (np.full(K, 0.1), 9 - 4 * comm.rank, 5)):
    shift = None if shift0 is None else shift0 * (comm.rank + 1)
    s = make(comm)
    t0 = s._dev.get_tick()
    ex = s.expectations(n_iter, cov=True, block=block, shift=shift, of=s.projections(A, b))
    assert s._dev.get_tick() - t0 == n_iter + 1, 'a rank ran more than the 21 iterations (a replayed or retried block)'
    both = comm.allreduce_f64(np.concatenate([ex.shift, -ex.shift]), 'max')
    assert ex.shift.shape == (K,) and np.array_equal(both[:K], -both[K:]), 'the shards used different shifts'
    s2 = make(comm)
    dg = s2.diagnostics(n_iter, split=False, block=block, shift=shift, of=s2.projections(A, b))
    both = comm.allreduce_f64(np.concatenate([dg.shift, -dg.shift]), 'max')
    assert np.array_equal(both[:K], -both[K:]), 'the shards used different shifts'
    if comm.rank == 0:
        # the unsharded run recorded in one ring, the NumPy loop on its states, its sums on the host: the reduced sums meet
        # the bounds of the definition tests; the run itself is the unsharded one
        from tests.test_gpu_estimators import host_sums, assert_within_bound, recorded_block
        from tests.test_gpu_chainstats import host_chain_sums, assert_fold_within_bound
        from tests.test_gpu_projections import numpy_loop
        s1 = make(None)
        e1 = s1.expectations(n_iter, cov=True, block=agreed, shift=ex.shift, of=s1.projections(A, b))
        assert (s.l_count, s.f_count, s.r_count) == (s1.l_count, s1.f_count, s1.r_count)
        assert np.array_equal(s.dwelling_times, s1.dwelling_times)
        assert ex.n_states == e1.n_states == n_iter * N
        X, dwell = recorded_block(make(None), n_iter)
        V = numpy_loop(A, b, X[:, :n_iter, :])
        w = dwell[1:n_iter + 1]
        host, absum = host_sums(V, w, ex.shift, True)
        assert_within_bound((ex.W, ex.S1, ex.S2, ex.C), host, absum, ex.n_states, 'sharded of=P')
        assert_within_bound((e1.W, e1.S1, e1.S2, e1.C), host, absum, e1.n_states, 'unsharded of=P')
        assert (dg.n_chains, dg.n_states) == (N, n_iter)
        # (the two ranks' folds are added on top of each fold: one more addition on the way into the sum)
        assert_fold_within_bound((dg.Sw, dg.Sm, dg.Sq, dg.Sv), *host_chain_sums(V, w, dg.shift), tag='sharded diagnostics(of=P)',
                                 extra_depth=1)
    comm.barrier()
print('rank %%d ok' %% comm.rank)
'''


def test_sharded_projections_equal_unsharded(tmp_path):
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
