"""GPU: dwell-weighted marginal histograms on the device (csrc/histograms.hip, DeviceHistogram, HMCBase.marginals).

The definition (include/mjhmc_hip.h: mjhmc_histogram_create) is integer arithmetic behind two rounded float64 operations
per element; ``host_hist`` restates it in NumPy (whose elementwise float64 operations round once each and never fuse) and
every comparison of tables is ``==``."""
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------------
# the NumPy restatement
# ---------------------------------------------------------------------------------------------------------------------
def host_bins(X, lo, hi, B):
    """X (D, ...) float64 -> bin indices: t = (x - lo) * inv with inv = B / (hi - lo); 0 when !(t >= 0) (NaN too), B + 1
    when t >= B, 1 + (int)t otherwise"""
    shape = (-1,) + (1,) * (X.ndim - 1)
    inv = float(B) / (hi - lo)
    with np.errstate(invalid='ignore', over='ignore'):
        d = X - lo.reshape(shape)
        t = d * inv.reshape(shape)
        inside = (t >= 0) & (t < B)
        inner = 1 + np.where(inside, t, 0.0).astype(np.int64)
        return np.where(~(t >= 0), 0, np.where(t >= B, B + 1, inner))


def host_units(w, q):
    """u = rint(w / q), nearest-even, as unsigned 64-bit integers"""
    return np.rint(w / q).astype(np.uint64)


def host_hist(X, w, lo, hi, B, q):
    """X (D, n, N) float64 states as the ring holds them, w (n, N) weights -> count, mass (D, B + 2) uint64, W_units"""
    D = X.shape[0]
    bins = host_bins(X, lo, hi, B).reshape(D, -1)
    u = host_units(w, q).ravel()
    count, mass = np.zeros((D, B + 2), dtype=np.uint64), np.zeros((D, B + 2), dtype=np.uint64)
    for d in range(D):
        count[d] = np.bincount(bins[d], minlength=B + 2).astype(np.uint64)
        np.add.at(mass[d], bins[d], u)
    return count, mass, int(u.sum(dtype=np.uint64))


def _ring(X, dtype='float64', w=None, slots=None):
    """a sampler of the test build whose ring slots 0 .. n - 1 hold X (D, n, N) rounded to ``dtype`` (mjhmc_test_ring_write)
    and whose dwell slots 0 .. n - 1 hold w (n, N) (mjhmc_test_ring_write_dwell); returns it and the states as stored"""
    from mjhmc_amd import engine, _lib
    from tests.helpers import hooks_context
    ctx = hooks_context(0)
    D, n, N = X.shape
    if dtype == 'bfloat16':                                   # bfloat16 state is SparseImageCode's alone
        from mjhmc_amd.misc.distributions import SparseImageCode
        from tests.helpers import sic_problem
        assert D == 512
        Bm, imgs, a0 = sic_problem(3, n_patches=1, n_coeffs=512)
        kind, params = SparseImageCode(n_patches=1, n_batches=N, cauchy=True, n_basis=512, basis=Bm, imgs=imgs,
                                       init=np.tile(a0[:, None], (1, N)), state_dtype='bfloat16').device_energy()
        en = engine.DeviceEnergy(ctx, kind, D, params)
    else:
        en = engine.DeviceEnergy(ctx, _lib.E_ISO_GAUSS, D, [1.0])
    dev = engine.DeviceSampler(en, np.zeros((D, N)), seed=5, dtype=dtype, mode=_lib.MODE_MJHMC)
    dev.ring_alloc(slots or n)
    for k in range(n):
        block = np.ascontiguousarray(X[:, k, :])             # (kept alive across the call: the hook reads it)
        engine.check(ctx.lib.mjhmc_test_ring_write(dev.handle, k, block.ctypes.data), ctx.lib)
        if w is not None:
            for p in range(N):
                engine.check(ctx.lib.mjhmc_test_ring_write_dwell(dev.handle, k, p, float(w[k, p])), ctx.lib)
    stored = dev.ring_read(0, n).reshape(D, n, N)
    if w is not None:
        assert np.array_equal(dev.ring_read_dwell(0, n), w)
    return ctx, dev, stored


def _ranges(D, B):
    """dimension 0: a dyadic range (every edge is a float64, a bfloat16 for small B); the others irregular"""
    lo = -2.0 - 0.013 * np.arange(D)
    hi = 2.0 + 0.031 * np.arange(D)
    return lo, hi


def _states(D, n, N, B, lo, hi, seed):
    """normal draws wider than the range, with values exactly on computed edges, below lo, at lo, at hi, beyond hi, signed
    zeros, infinities and NaN planted in every dimension"""
    rs = np.random.RandomState(seed)
    X = rs.randn(D, n, N) * 1.5
    special = lambda d: np.concatenate([lo[d] + np.arange(B + 1) * ((hi[d] - lo[d]) / B),
                                        [lo[d], hi[d], np.nextafter(lo[d], -np.inf), np.nextafter(hi[d], -np.inf), lo[d] - 1.0,
                                         hi[d] + 3.0, 0.0, -0.0, np.inf, -np.inf, np.nan]])
    for d in range(D):
        sp = special(d)
        flat = X[d].reshape(-1)
        m = min(sp.size, flat.size)
        at = rs.choice(flat.size, size=m, replace=False)
        flat[at] = rs.permutation(sp)[:m]
    return X


def _same_tables(got, want, tag):
    for name, g, h in zip(('count', 'mass'), got[:2], want[:2]):
        assert g.shape == h.shape and g.dtype == np.uint64, (tag, name)
        bad = int(np.sum(g != h))
        assert bad == 0, '%s %s: %d of %d bins differ' % (tag, name, bad, h.size)
    assert got[2] == want[2], (tag, 'W_units', got[2], want[2])


# state type, ndims, N, B.  Lane widths 2 / 4 / 8 elements (float64 / float32 / bfloat16); pitches that are not the row
# length (33 -> 34, 5 -> 8); every N of {1, 63, 64, 65, 4096} and every B of {1, 7, 256, 1024} with every state type;
# strips narrower than a lane's 16 bytes (float32 and bfloat16 at B = 1024)
DEFINITION_CASES = [
    ('float64', 33, 65, 7), ('float64', 2, 4096, 256), ('float64', 33, 63, 1024), ('float64', 5, 1, 1), ('float64', 512, 64, 256),
    ('float32', 36, 65, 256), ('float32', 5, 63, 7), ('float32', 9, 4096, 1024), ('float32', 3, 1, 1), ('float32', 70, 64, 7),
    ('bfloat16', 512, 65, 256), ('bfloat16', 512, 63, 1024), ('bfloat16', 512, 64, 7), ('bfloat16', 512, 1, 1),
    ('bfloat16', 512, 4096, 256),
]


# ---------------------------------------------------------------------------------------------------------------------
# 1.  the definition, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype,D,N,B', DEFINITION_CASES)
def test_definition_bit_for_bit(dtype, D, N, B):
    """count, mass and W_units == the NumPy restatement, for the dwell pairing (weights of all magnitudes around the
    quantum, zero among them) and for unit weights (two quanta)"""
    n = 2 if N >= 4096 else 3
    lo, hi = _ranges(D, B)
    rs = np.random.RandomState(N + B)
    w = rs.standard_exponential((n, N)) * 10.0 ** rs.randint(-4, 3, size=(n, N))
    w.reshape(-1)[:: 7] = 0.0
    q = 2.0 ** -20
    ctx, dev, X = _ring(_states(D, n, N, B, lo, hi, seed=B + N), dtype, w)
    planted = n * N >= B + 12                                  # every special value of _states found a place
    if dtype != 'float64':
        assert (np.any(np.isnan(X)) or not planted) and np.array_equal(X[np.isfinite(X)], X[np.isfinite(X)].astype(np.float32))
    h = dev.histogram(B, lo, hi, q)
    h.accumulate(0, n, w_slot0=0)
    got = h.read()
    want = host_hist(X, w, lo, hi, B, q)
    _same_tables(got, want, 'dwell')
    assert got[3] == n * N and np.all(got[0].sum(axis=1) == n * N) and np.all(got[1].sum(axis=1) == got[2])
    if planted:
        assert got[0][:, 0].min() >= 3 and got[0][:, -1].min() >= 2             # NaN, -inf, lo - 1 below; +inf, hi + 3 above
    h.close()
    for qu in (1.0, 0.125):
        hu = dev.histogram(B, lo, hi, qu)
        hu.accumulate(0, n, w_slot0=-1)
        _same_tables(hu.read(), host_hist(X, np.ones((n, N)), lo, hi, B, qu), 'unit weights, q = %g' % qu)
        hu.close()
    dev.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2.  independence of the blocks, and of the run
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype,D,N,B', [('float64', 33, 333, 256), ('float32', 36, 130, 64), ('bfloat16', 512, 65, 1024)])
def test_block_independence(dtype, D, N, B):
    """one call, blocks of one slot, an uneven cut, and a second run on a fresh sampler: the same tables"""
    n = 6
    lo, hi = _ranges(D, B)
    w = np.random.RandomState(3).standard_exponential((n, N)) + 1e-3
    q = 2.0 ** -24
    results = []
    for run in range(2):
        ctx, dev, X = _ring(_states(D, n, N, B, lo, hi, seed=9), dtype, w)
        h = dev.histogram(B, lo, hi, q)
        for cuts in ([n], [1] * n, [2, 1, n - 3]) if run == 0 else ([4, 2],):
            h.reset()
            at = 0
            for k in cuts:
                h.accumulate(at, k, w_slot0=at)
                at += k
            results.append(h.read())
            assert results[-1][3] == n * N
        if run == 0:
            want = host_hist(X, w, lo, hi, B, q)
        dev.close()
    for i, r in enumerate(results):
        _same_tables(r, want, 'cut %d' % i)


# ---------------------------------------------------------------------------------------------------------------------
# 3.  the quantisation bound
# ---------------------------------------------------------------------------------------------------------------------
def test_quantisation_bound_bin_by_bin():
    """|q mass - sum w| <= 0.5 q count against float64 NumPy sums of the weights of every bin, with a quantum coarse
    enough that the rounding shows.  (The float64 sum of a bin's <= 3 000 weights of size ~1 carries an error below
    3 000 * 2^-53 * sum, five orders below the 0.5 q count it is compared with.)"""
    D, n, N, B = 6, 3, 1000, 32
    lo, hi = _ranges(D, B)
    rs = np.random.RandomState(12)
    w = rs.standard_exponential((n, N)) + 0.01
    q = 2.0 ** -6
    ctx, dev, X = _ring(rs.randn(D, n, N) * 1.2, 'float64', w)
    h = dev.histogram(B, lo, hi, q)
    h.accumulate(0, n, w_slot0=0)
    count, mass, W_units, n_states = h.read()
    bins = host_bins(X, lo, hi, B).reshape(D, -1)
    worst = 0.0
    for d in range(D):
        sums = np.bincount(bins[d], weights=w.ravel(), minlength=B + 2)
        err = np.abs(q * mass[d].astype(np.float64) - sums)
        bound = 0.5 * q * count[d].astype(np.float64)
        assert np.all(err <= bound), (d, err, bound)
        worst = max(worst, float(np.max(err / np.where(bound > 0, bound, 1.0))))
    print('quantisation: worst |q mass - sum w| / (0.5 q count) = %.3f' % worst)
    assert worst > 0.0, 'a quantum this coarse must round something'
    assert abs(q * W_units - w.sum()) <= 0.5 * q * n * N
    dev.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4.  padding rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype,D,N', [('float64', 5, 1), ('float64', 33, 65), ('float32', 6, 63), ('bfloat16', 512, 65)])
def test_padding_rows_do_not_contribute(dtype, D, N):
    """rows N <= p < Npad of every slot, and the dwell ring's padding entries, filled with 0xFF bytes (NaN as a state of
    every type and as a weight): a pass that read them would count them in the underflow bin, a check that read them would
    refuse the block"""
    from mjhmc_amd import engine
    n, B = 3, 16
    lo, hi = _ranges(D, B)
    rs = np.random.RandomState(N)
    w = rs.standard_exponential((n, N)) + 0.5
    ctx, dev, X = _ring(rs.randn(D, n, N), dtype, w)
    for k in range(n):
        engine.check(ctx.lib.mjhmc_test_ring_fill_padding(dev.handle, k, 0xFF), ctx.lib)
    assert np.array_equal(dev.ring_read(0, n).reshape(D, n, N), X)
    q = 2.0 ** -16
    h = dev.histogram(B, lo, hi, q)
    h.accumulate(0, n, w_slot0=0)
    _same_tables(h.read(), host_hist(X, w, lo, hi, B, q), 'padding, dwell')
    h.reset()
    h.accumulate(0, n, w_slot0=-1)
    got = h.read()
    _same_tables(got, host_hist(X, np.ones((n, N)), lo, hi, B, q), 'padding, unit')
    assert np.all(got[0].sum(axis=1) == n * N)
    dev.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5.  refusals add nothing
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_add_nothing():
    from mjhmc_amd import engine, _lib
    D, n, N, B = 7, 4, 70, 32
    lo, hi = _ranges(D, B)
    rs = np.random.RandomState(2)
    w = rs.standard_exponential((n, N)) + 0.1
    q = 2.0 ** -30
    ctx, dev, X = _ring(rs.randn(D, n, N), 'float64', w)
    h = dev.histogram(B, lo, hi, q)
    h.accumulate(0, 2, w_slot0=0)
    before = h.read()
    _same_tables(before, host_hist(X[:, :2], w[:2], lo, hi, B, q), 'first block')

    def poke(value):
        engine.check(ctx.lib.mjhmc_test_ring_write_dwell(dev.handle, 3, 17, float(value)), ctx.lib)

    for value, code, msg in ((float('inf'), _lib.ERR_NONFINITE, 'not finite'), (float('nan'), _lib.ERR_NONFINITE, 'not finite'),
                             (-0.25, _lib.ERR_NONFINITE, 'negative'), (q * 2.0 ** 53, -1, '2\\^53'), (1e300, -1, '2\\^53')):
        poke(value)
        with pytest.raises(_lib.EngineError, match=msg):
            h.accumulate(2, 2, w_slot0=2)
        assert ctx.lib.mjhmc_histogram_accumulate(h.handle, 2, 2, 2) == code, value
        after = h.read()
        _same_tables(after, before, 'after a refused block (%r)' % value)
        assert after[3] == before[3] == 2 * N
    poke(q * (2.0 ** 53 - 1.0))                                 # the largest weight the quantum takes
    w[3, 17] = q * (2.0 ** 53 - 1.0)
    h.accumulate(2, 2, w_slot0=2)                               # the flags do not stick
    _same_tables(h.read(), host_hist(X, w, lo, hi, B, q), 'after the refusals')
    dev.close()


def test_total_of_two_to_the_63_is_refused():
    """4096 weights of 2^52 quanta each are 2^64 quanta; 1024 of them are 2^62, which a second such block takes to 2^63"""
    from mjhmc_amd import _lib
    D, B, q = 2, 8, 2.0 ** -40
    lo, hi = _ranges(D, B)
    rs = np.random.RandomState(4)
    ctx, dev, X = _ring(rs.randn(D, 1, 4096), 'float64', np.full((1, 4096), q * 2.0 ** 52))
    h = dev.histogram(B, lo, hi, q)
    with pytest.raises(_lib.EngineError, match='2\\^63'):
        h.accumulate(0, 1, w_slot0=0)
    assert ctx.lib.mjhmc_histogram_accumulate(h.handle, 0, 0, 1) == -1
    got = h.read()
    assert not got[0].any() and not got[1].any() and got[2:] == (0, 0)
    dev.close()
    ctx, dev, X = _ring(rs.randn(D, 2, 1024), 'float64', np.full((2, 1024), q * 2.0 ** 52))
    h = dev.histogram(B, lo, hi, q)
    h.accumulate(0, 1, w_slot0=0)
    before = h.read()
    assert before[2] == 2 ** 62
    with pytest.raises(_lib.EngineError, match='2\\^63'):
        h.accumulate(1, 1, w_slot0=1)
    _same_tables(h.read(), before, 'after the refused second block')
    hu = dev.histogram(B, lo, hi, 2.0 ** -60)                  # a unit weight of 2^60 quanta
    with pytest.raises(_lib.EngineError, match='2\\^53'):
        hu.accumulate(0, 1, w_slot0=-1)
    assert not hu.read()[0].any()
    dev.close()


def test_invalid_arguments():
    from mjhmc_amd._lib import EngineError
    from tests.test_gpu_chainstats import _iso
    s = _iso(33, 100, 1)
    dev = s._dev
    with pytest.raises(EngineError, match='no sample ring'):
        dev.histogram(16, -1.0, 1.0)
    dev.ring_alloc(4)
    s._run(4, ring_slot0=0)
    for bins in (0, 1025):
        with pytest.raises(EngineError, match='n_bins must be in'):
            dev.histogram(bins, -1.0, 1.0)
    for lo, hi, msg in ((1.0, 1.0, 'lo must be below hi'), (2.0, 1.0, 'lo must be below hi'), (-np.inf, 1.0, 'not finite'),
                        (0.0, np.nan, 'not finite'), (np.zeros(33), np.r_[np.ones(32), 0.0], 'dimension 32')):
        with pytest.raises(EngineError, match=msg):
            dev.histogram(16, lo, hi)
    for q in (0.0, 3.0, -2.0, np.inf):
        with pytest.raises(EngineError, match='power of two'):
            dev.histogram(16, -1.0, 1.0, q)
    with pytest.raises(ValueError):
        dev.histogram(16, np.zeros(5), 1.0)
    h = dev.histogram(16, -4.0, 4.0, 2.0 ** -20)
    for args, msg in (((0, 5, -1), 'outside the ring'), ((3, 2, -1), 'outside the ring'), ((-1, 1, -1), 'outside the ring'),
                      ((0, 4, 1), 'dwell slots'), ((0, 1, -2), 'dwell slots'), ((0, 0, -1), 'n must be >= 1')):
        with pytest.raises(EngineError, match=msg):
            h.accumulate(args[0], args[1], w_slot0=args[2])
    assert h.read()[2:] == (0, 0)
    h.accumulate(0, 3, w_slot0=1)
    assert h.read()[3] == 300
    h.reset()
    assert h.read()[2:] == (0, 0) and not h.read()[0].any()
    dev.ring_alloc(9)                                               # a new ring: the plan was made for the old one
    with pytest.raises(EngineError, match='re-allocated'):
        h.accumulate(0, 1)
    assert dev.lib.mjhmc_histogram_accumulate(h.handle, 0, -1, 1) == -1
    h.close()
    alive = dev.histogram(16, -4.0, 4.0)
    dev.close()                                                     # the sampler frees what is still alive on it
    alive.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6.  a known answer, with a negative control
# ---------------------------------------------------------------------------------------------------------------------
def _Phi(x):
    return 0.5 * (1.0 + np.vectorize(math.erf)(np.asarray(x, dtype=np.float64) / math.sqrt(2.0)))


def test_known_answer_exponentially_tilted_normal_with_negative_control():
    """X ~ N(0, 1) i.i.d. in D = 4 dimensions, w = exp(x_0): the weighted law of dimension 0 is N(1, 1), the others stay
    N(0, 1).  At every edge t with 0.01 < F(t) < 0.99:  |cdf(t) - F(t)| <= 6 sigma,
        sigma^2 = (sum_{x <= t} u^2 (1 - F)^2 + sum_{x > t} u^2 F^2) / (sum u)^2
    the delta-method variance of the self-normalised estimate, from the same data.  (A NumPy restatement of the
    definition on the CPU reaches at most 4.8 sigma over seeds 0 .. 19.)  Negative control: the same table scored against
    Phi(t), the unweighted law, is off by more than 500 sigma in dimension 0; asserted > 50."""
    from mjhmc_amd.samplers.markov_jump_hmc import Marginals
    D, n, N, B = 4, 16, 4096, 256
    X = np.random.RandomState(0).randn(D, n, N)
    w = np.exp(X[0])
    q = 2.0 ** (math.floor(math.log2(w.mean())) - 24)
    lo, hi = np.full(D, -8.0), np.full(D, 9.0)
    ctx, dev, stored = _ring(X, 'float64', w)
    assert np.array_equal(stored, X)
    h = dev.histogram(B, lo, hi, q)
    h.accumulate(0, n, w_slot0=0)
    count, units, W_units, n_states = h.read()
    dev.close()
    _same_tables((count, units, W_units), host_hist(X, w, lo, hi, B, q), 'known answer')
    m = Marginals(lo, hi, B, q, count, units, W_units, n_states)
    assert np.all(m.out_of_range == 0.0) and n_states == n * N
    u = host_units(w, q).astype(np.float64).ravel()
    worst = np.zeros(D)
    control = 0.0
    for d in range(D):
        x = X[d].ravel()
        order = np.argsort(x)
        below = np.concatenate([[0.0], np.cumsum(u[order] ** 2)])          # sum of u^2 over the k smallest x
        for t, est in zip(m.edges[d], m.cdf(m.edges[d])[d]):
            F = float(_Phi(t - 1.0 if d == 0 else t))
            if not 0.01 < F < 0.99:
                continue
            k = np.searchsorted(x[order], t, side='right')
            sigma = math.sqrt(below[k] * (1 - F) ** 2 + (below[-1] - below[k]) * F ** 2) / u.sum()
            worst[d] = max(worst[d], abs(est - F) / sigma)
            if d == 0:
                control = max(control, abs(est - float(_Phi(t))) / sigma)
    print('known answer: worst |cdf - F| / sigma per dimension %s; dimension 0 against the unweighted law %.0f sigma'
          % (np.round(worst, 2), control))
    assert np.all(worst <= 6.0), worst
    assert control > 50.0, control
    assert np.all(np.abs(m.median - [1.0, 0.0, 0.0, 0.0]) < 0.05)
    lo95, hi95 = m.interval(0.95)
    assert np.all(np.abs(lo95 - [-0.96, -1.96, -1.96, -1.96]) < 0.1) and np.all(np.abs(hi95 - [2.96, 1.96, 1.96, 1.96]) < 0.1)


# ---------------------------------------------------------------------------------------------------------------------
# 7.  the driver
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cls', ['MarkovJumpHMC', 'ControlHMC'])
def test_driver_leaves_the_sampler_as_expectations_does(cls):
    """marginals(30, block=7): counters, dwelling times, final state and RNG tick as expectations(30) from the same seed;
    the tables equal the NumPy histogram of the same chain recorded in one ring (states of sample(preserve_order=True),
    weights of the dwell ring) at the returned range and quantum"""
    from tests.test_gpu_chainstats import _iso, record
    n_iter, D, N, B = 30, 24, 301, 64
    s = _iso(D, N, 5, cls)
    tick0 = s._dev.get_tick()
    for kwargs in (dict(n_iter=0), dict(n_iter=4, bins=2000), dict(n_iter=4, range=(1.0, 0.0)), dict(n_iter=4, range=(np.zeros(3), 1.0))):
        with pytest.raises(ValueError):
            s.marginals(**kwargs)
    assert (s._dev.get_tick(), s._dev.ring_slots) == (tick0, 0)
    m = s.marginals(n_iter, bins=B, block=7)
    lead = 1 if s._dwell_weighted else 0
    assert s._dev.get_tick() - tick0 == n_iter + lead
    ref = _iso(D, N, 5, cls)
    e = ref.expectations(n_iter, block=11, shift=np.zeros(D))
    assert (s.l_count, s.f_count, s.r_count, s.fl_count) == (ref.l_count, ref.f_count, ref.r_count, ref.fl_count)
    assert (s.distribution.E_count, s.distribution.dEdX_count) == (ref.distribution.E_count, ref.distribution.dEdX_count)
    assert np.array_equal(s.state.X, ref.state.X) and np.array_equal(s.state.V, ref.state.V)
    assert s._dev.get_tick() == ref._dev.get_tick()
    if lead:
        assert np.array_equal(s.dwelling_times, ref.dwelling_times)
    # the same run in one ring
    X, w, w_slot0 = record(_iso(D, N, 5, cls), n_iter)
    X = X[:, :n_iter, :]
    first_w, first_x = w[:7], X[:, :7, :]
    mean = (first_w[None] * first_x).sum(axis=(1, 2)) / first_w.sum()
    sd = np.sqrt((first_w[None] * first_x ** 2).sum(axis=(1, 2)) / first_w.sum() - mean ** 2)
    assert np.allclose(m.lo, mean - 8.0 * sd, rtol=0, atol=1e-9) and np.allclose(m.hi, mean + 8.0 * sd, rtol=0, atol=1e-9)
    if lead:
        assert m.quantum == 2.0 ** (math.floor(math.log2(first_w.mean())) - 24)
    else:
        assert m.quantum == 1.0
    want = host_hist(X, w, m.lo, m.hi, B, m.quantum)
    _same_tables((m.counts, m.units, m.W_units), want, 'driver ' + cls)
    assert m.n_states == n_iter * N and m.edges.shape == (D, B + 1)
    assert all(int(row.sum(dtype=np.uint64)) == m.W_units for row in m.units)          # sum(mass[d]) q / total_weight == 1
    assert m.total_weight == m.quantum * m.W_units
    assert abs(m.total_weight - e.total_weight) <= 0.5 * m.quantum * m.n_states + 1e-12 * e.total_weight
    assert np.all(m.out_of_range == 0.0)
    assert np.all(np.abs(m.median - e.mean) < 0.5 * np.sqrt(e.var))
    # a caller's range, scalars: no moment pass for the unit-weight samplers, the same quantum for the weighted ones
    t = _iso(D, N, 5, cls)
    mt = t.marginals(n_iter, bins=B, range=(-6.0, 7.0))
    assert t._dev.get_tick() == s._dev.get_tick() and mt.quantum == (host_q(w) if lead else 1.0)
    _same_tables((mt.counts, mt.units, mt.W_units), host_hist(X, w, np.full(D, -6.0), np.full(D, 7.0), B, mt.quantum),
                 'driver, given range ' + cls)


def host_q(w):
    """the driver's quantum when the whole run is its first block"""
    return 2.0 ** (math.floor(math.log2(w.mean())) - 24)


# ---------------------------------------------------------------------------------------------------------------------
# 8.  column shards on one GPU (the way test_gpu_sharded.py runs them)
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
D, N, n_iter, B = 24, 301, 20, 128
X0 = np.random.RandomState(5).randn(D, N) + 0.4


def dist_of():
    class Fixed(TestGaussian):
        def init_X(self):
            self.Xinit = X0
    return Fixed(ndims=D, nbatch=N, sigma=1.3)


def make(comm):
    return MarkovJumpHMC(distribution=dist_of(), epsilon=0.3, beta=0.3, num_leapfrog_steps=5, seed=4242, comm=comm,
                         resample=False)


# rank-dependent arguments: rank 0's range must win, and the ranks must agree on the smallest block
# (the unsharded twin walks the run in the block the ranks agree on: the quantum comes from the first block's mean weight)
for rng, block, agreed in ((None, 4 + 3 * comm.rank, 4), ((-5.0 - comm.rank, 6.0 + comm.rank), 9 - 4 * comm.rank, 5), (None, None, None)):
    s = make(comm)
    t0 = s._dev.get_tick()
    m = s.marginals(n_iter, bins=B, range=rng, block=block)
    assert s._dev.get_tick() - t0 == n_iter + 1, 'a rank ran more than the 21 iterations (a replayed or retried block)'
    packed = np.concatenate([m.lo, m.hi, [m.quantum]])
    both = comm.allreduce_f64(np.concatenate([packed, -packed]), 'max')
    assert np.array_equal(both[:packed.size], -both[packed.size:]), 'the shards used different ranges or quanta'
    if rng is not None:
        assert np.all(m.lo == -5.0) and np.all(m.hi == 6.0)
    assert m.n_states == n_iter * N
    if comm.rank == 0:
        s1 = make(None)
        m1 = s1.marginals(n_iter, bins=B, range=(m.lo, m.hi), block=agreed)
        assert m1.quantum == m.quantum
        assert np.array_equal(m.counts, m1.counts) and np.array_equal(m.units, m1.units), 'sharded tables differ from the unsharded ones'
        assert (m.W_units, m.n_states) == (m1.W_units, m1.n_states)
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
