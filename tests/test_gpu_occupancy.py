"""GPU: cell occupancy and transition counts of the recorded chains (csrc/occupancy.hip, csrc/occupancy.hpp,
DeviceOccupancy, HMCBase.occupancy).

The definition (include/mjhmc_hip.h: mjhmc_occupancy_create) is integer arithmetic behind three rounded float64 operations
per (state, centre, dimension); ``host_labels`` / ``host_tables`` of tests/test_occupancy_cpu.py restate it in NumPy and
every comparison of labels, tables and tallies is ``==``."""
import math

import numpy as np
import pytest

from tests.test_occupancy_cpu import host_labels, host_tables, host_units
from tests.test_gpu_marginals import _ring

pytestmark = pytest.mark.gpu

TABLES = ('count', 'mass', 'from_count', 'from_mass', 'trans', 'chains_by_switches', 'chains_by_cells', 'switches', 'visited')


def _same(got, want, tag):
    for name in TABLES:
        g, h = got[name], want[name]
        assert g.shape == h.shape and g.dtype == h.dtype, (tag, name, g.shape, h.shape, g.dtype, h.dtype)
        bad = int(np.sum(g != h))
        assert bad == 0, '%s %s: %d of %d entries differ' % (tag, name, bad, h.size)
    assert got['W_units'] == want['W_units'], (tag, 'W_units', got['W_units'], want['W_units'])
    assert got['n_states'] == want['n_states'], (tag, 'n_states')


def _problem(D, n, N, M, integer, radius, seed):
    """states (D, n, N) and centres (M, D): small integers (exact ties; centre M - 1 a copy of centre 0) or Gaussian draws;
    NaN, +inf and -inf planted in a few rows; a radius vector near the 0.6 quantile of the nearest distance"""
    rs = np.random.RandomState(seed)
    if integer:
        X = rs.randint(-2, 3, size=(D, n, N)).astype(np.float64)
        C = rs.randint(-2, 3, size=(M, D)).astype(np.float64)
        if M >= 2:
            C[M - 1] = C[0]
    else:
        X = rs.randn(D, n, N)
        C = rs.randn(M, D)
    flat = X.reshape(D, -1)
    for j, v in enumerate((np.nan, np.inf, -np.inf)):
        if flat.shape[1] > 2 * j + 1:
            flat[rs.randint(D), 2 * j + 1] = v
    r2 = None
    if radius:
        with np.errstate(invalid='ignore'):
            near = ((X[None] - C.reshape(M, D, 1, 1)) ** 2).sum(axis=1).min(axis=0)
        r = np.sqrt(np.nanquantile(np.where(np.isfinite(near), near, np.nan), 0.6)) * (0.97 + 0.06 * rs.rand(M))
        r2 = r * r
    return X, C, r2


def _want(X, w, C, r2, q, starts=(0,)):
    labels = host_labels(X, C, r2)
    n, N = labels.shape
    units = host_units(w, q) if w is not None else np.full((n, N), np.uint64(round(1.0 / q)), dtype=np.uint64)
    return labels, host_tables(labels, units, C.shape[0], starts)


# ---------------------------------------------------------------------------------------------------------------------
# 1.  the definition, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
# state type, ndims, N, M, integer data, radius, weighted.  D: one element (1), a row narrower than 16 bytes of float64 (3),
# a padded row and a partial d chunk (33), several chunks (512); N: a partial row tile (1, 63), more than one workgroup of
# either kernel (257, 1000); M: both tiles (<= 16: 1, 2, 7; > 16: 17, 64), a padded tile at every M but 64
DEFINITION_CASES = [
    ('float64', 1, 1, 1, True, False, False), ('float64', 3, 63, 2, True, True, True), ('float64', 33, 257, 7, False, False, True),
    ('float64', 512, 1000, 64, False, True, False), ('float64', 33, 1000, 17, True, False, True),
    ('float64', 3, 257, 64, False, False, False), ('float64', 512, 63, 7, True, True, False),
    ('float64', 1, 1000, 2, False, True, True),
    ('float32', 1, 63, 7, True, True, False), ('float32', 3, 1000, 17, False, False, True), ('float32', 33, 1, 64, True, False, True),
    ('float32', 512, 257, 2, False, True, True), ('float32', 33, 257, 1, False, True, False),
    ('bfloat16', 512, 63, 17, True, False, False), ('bfloat16', 512, 257, 64, False, True, True),
    ('bfloat16', 512, 1, 1, False, False, True), ('bfloat16', 512, 1000, 2, True, True, False),
]


@pytest.mark.parametrize('dtype,D,N,M,integer,radius,weighted', DEFINITION_CASES)
def test_definition_bit_for_bit(dtype, D, N, M, integer, radius, weighted):
    n, q = 5, 2.0 ** -20
    X, C, r2 = _problem(D, n, N, M, integer, radius, seed=D + 7 * N + 13 * M)
    rs = np.random.RandomState(N + M)
    w = rs.standard_exponential((n, N)) + 0.1 if weighted else None
    ctx, dev, stored = _ring(X, dtype, w)
    occ = dev.occupancy(C, r2, q)
    assert occ.info() == (M, D, n)
    occ.accumulate(0, n, w_slot0=0 if weighted else -1)
    labels, want = _want(stored, w, C, r2, q)
    got_labels = occ.read_labels(n)
    assert got_labels.dtype == np.uint8 and got_labels.shape == (n, N)
    assert int(np.sum(got_labels != labels)) == 0, 'labels: %d of %d differ' % (np.sum(got_labels != labels), labels.size)
    _same(occ.read(chains=True), want, 'definition')
    assert int(want['count'][M]) >= min(3, n * N // 2), 'the planted rows that are not finite must land outside'
    if integer and M >= 2:
        assert want['count'][M - 1] == 0, 'the copy of centre 0 must take nothing'
    if radius and N >= 63:
        assert want['count'][M] > 3 and want['count'][:M].sum() > 0, 'the radius must cut some states off and keep some'
    dev.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2.  the tables do not depend on the blocks
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype,D,N,M', [('float64', 3, 257, 7), ('float32', 33, 63, 17), ('bfloat16', 512, 65, 2)])
def test_block_independence(dtype, D, N, M):
    n, q = 7, 2.0 ** -18
    X, C, r2 = _problem(D, n, N, M, dtype != 'float32', True, seed=N)
    w = np.random.RandomState(3).standard_exponential((n, N)) + 0.2
    ctx, dev, stored = _ring(X, dtype, w)
    _, want = _want(stored, w, C, r2, q)
    occ = dev.occupancy(C, r2, q)
    occ.accumulate(0, n, w_slot0=0)
    _same(occ.read(chains=True), want, 'one call')
    occ.reset()
    for k in range(n):
        occ.accumulate(k, 1, w_slot0=k, linked=k > 0)
    _same(occ.read(chains=True), want, 'seven calls')
    occ.reset()
    occ.accumulate(0, 3, w_slot0=0)
    occ.accumulate(3, 4, w_slot0=3, linked=True)
    _same(occ.read(chains=True), want, '3 + 4, linked')
    assert int(want['trans'].sum()) == N * (n - 1)
    occ.reset()
    occ.accumulate(0, 3, w_slot0=0)
    occ.accumulate(3, 4, w_slot0=3, linked=False)
    cut = occ.read(chains=True)
    _same(cut, _want(stored, w, C, r2, q, starts=(0, 3))[1], '3 + 4, cut')
    assert int(cut['trans'].sum()) == N * (n - 1) - N, 'the cut must lose exactly N transitions'
    assert np.array_equal(cut['count'], want['count']) and np.array_equal(cut['mass'], want['mass'])
    dev.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3.  padding
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype,D,N,M', [('float64', 3, 63, 7), ('float64', 1, 1, 2), ('float32', 33, 65, 64), ('bfloat16', 512, 65, 17)])
def test_padding_rows_and_elements_change_nothing(dtype, D, N, M):
    """rows N <= p < Npad of every slot and the dwell ring's padding entries, and the elements ndims <= d < pitch of every
    row, filled with 0xFF bytes (NaN as a state of every type and as a weight): a label that read one would be "outside", a
    check that read one would refuse the block"""
    from mjhmc_amd import engine
    n, q = 3, 2.0 ** -16
    rs = np.random.RandomState(N)
    X, C = rs.randn(D, n, N), rs.randn(M, D)
    w = rs.standard_exponential((n, N)) + 0.5
    ctx, dev, stored = _ring(X, dtype, w)
    for k in range(n):
        engine.check(ctx.lib.mjhmc_test_ring_fill_padding(dev.handle, k, 0xFF), ctx.lib)
        engine.check(ctx.lib.mjhmc_test_ring_fill_element_padding(dev.handle, k, 0xFF), ctx.lib)
    assert np.array_equal(dev.ring_read(0, n).reshape(D, n, N), stored)
    occ = dev.occupancy(C, None, q)
    for w_slot0, wk in ((0, w), (-1, None)):
        occ.reset()
        occ.accumulate(0, n, w_slot0=w_slot0)
        labels, want = _want(stored, wk, C, None, q)
        assert np.array_equal(occ.read_labels(n), labels)
        got = occ.read(chains=True)
        _same(got, want, 'padding, w_slot0 = %d' % w_slot0)
        assert got['count'][M] == 0 and int(got['count'].sum()) == n * N
    dev.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4.  refusals add nothing
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_add_nothing_and_keep_the_carry():
    from mjhmc_amd import engine, _lib
    D, n, N, M = 7, 4, 70, 5
    rs = np.random.RandomState(2)
    X, C = rs.randn(D, n, N), rs.randn(M, D)
    w = rs.standard_exponential((n, N)) + 0.1
    q = 2.0 ** -30
    ctx, dev, stored = _ring(X, 'float64', w)
    occ = dev.occupancy(C, None, q)
    occ.accumulate(0, 2, w_slot0=0)
    before = occ.read(chains=True)
    _same(before, _want(stored[:, :2], w[:2], C, None, q)[1], 'first block')

    def poke(value):
        engine.check(ctx.lib.mjhmc_test_ring_write_dwell(dev.handle, 3, 17, float(value)), ctx.lib)

    for value, code, msg in ((-0.25, _lib.ERR_NONFINITE, 'negative'), (float('nan'), _lib.ERR_NONFINITE, 'not finite'),
                             (float('inf'), _lib.ERR_NONFINITE, 'not finite'), (q * 2.0 ** 53, -1, '2\\^53'), (1e300, -1, '2\\^53')):
        poke(value)
        with pytest.raises(_lib.EngineError, match=msg):
            occ.accumulate(2, 2, w_slot0=2, linked=True)
        assert ctx.lib.mjhmc_occupancy_accumulate(occ.handle, 2, 2, 2, 1) == code, value
        after = occ.read(chains=True)
        _same(after, before, 'after a refused block (%r)' % value)
        assert after['n_states'] == 2 * N
    poke(q * (2.0 ** 53 - 1.0))                                 # the largest weight the quantum takes
    w[3, 17] = q * (2.0 ** 53 - 1.0)
    occ.accumulate(2, 2, w_slot0=2, linked=True)                # the flags do not stick, and the carry is that of slot 1
    whole = _want(stored, w, C, None, q)[1]
    _same(occ.read(chains=True), whole, 'after the refusals')
    # what the valid call added: the tables of a fresh handle fed that call alone, plus the N pairs across the cut
    fresh = dev.occupancy(C, None, q)
    fresh.accumulate(2, 2, w_slot0=2)
    alone = fresh.read(chains=True)
    _same(alone, _want(stored[:, 2:], w[2:], C, None, q)[1], 'the valid call alone')
    added = whole['trans'] - before['trans'] - alone['trans']
    assert int(added.sum()) == N and np.array_equal(whole['count'], before['count'] + alone['count'])
    # reset: the bits of a new handle
    occ.reset()
    empty = occ.read(chains=True)
    assert all(not empty[k].any() for k in TABLES if k not in ('chains_by_switches', 'chains_by_cells'))
    assert empty['chains_by_switches'][0] == N and empty['chains_by_cells'][0] == N and empty['W_units'] == empty['n_states'] == 0
    with pytest.raises(_lib.EngineError, match='linked = 1'):
        occ.accumulate(2, 2, w_slot0=2, linked=True)
    occ.accumulate(2, 2, w_slot0=2)
    _same(occ.read(chains=True), alone, 'after reset')
    dev.close()


def test_total_of_two_to_the_63_is_refused():
    """1024 weights of 2^52 quanta each are 2^62 quanta, which a second such block takes to 2^63"""
    from mjhmc_amd import _lib
    D, M, q = 2, 3, 2.0 ** -40
    rs = np.random.RandomState(4)
    C = rs.randn(M, D)
    w = np.full((2, 1024), q * 2.0 ** 52)
    ctx, dev, stored = _ring(rs.randn(D, 2, 1024), 'float64', w)
    occ = dev.occupancy(C, None, q)
    occ.accumulate(0, 1, w_slot0=0)
    before = occ.read(chains=True)
    assert before['W_units'] == 2 ** 62
    with pytest.raises(_lib.EngineError, match='2\\^63'):
        occ.accumulate(1, 1, w_slot0=1, linked=True)
    assert ctx.lib.mjhmc_occupancy_accumulate(occ.handle, 1, 1, 1, 1) == -1
    _same(occ.read(chains=True), before, 'after the refused second block')
    assert not before['trans'].any()
    hu = dev.occupancy(C, None, 2.0 ** -60)                    # a unit weight of 2^60 quanta
    with pytest.raises(_lib.EngineError, match='2\\^53'):
        hu.accumulate(0, 1, w_slot0=-1)
    assert not hu.read()['count'].any()
    dev.close()


def test_invalid_arguments():
    from mjhmc_amd._lib import EngineError
    from tests.test_gpu_chainstats import _iso
    s = _iso(33, 100, 1)
    dev = s._dev
    C = np.zeros((3, 33))
    with pytest.raises(ValueError, match='no sample ring'):
        dev.occupancy(C)
    dev.ring_alloc(4)
    s._run(4, ring_slot0=0)
    for M in (0, 65):
        with pytest.raises(ValueError, match='M must be in'):
            dev.occupancy(np.zeros((M, 33)))
    for bad in (np.nan, np.inf):
        Cb = C.copy()
        Cb[2, 32] = bad
        with pytest.raises(ValueError, match='coordinate 32 of centre 2'):
            dev.occupancy(Cb)
    for r2 in (-1.0, np.nan, [1.0, 2.0, -0.0625]):
        with pytest.raises(ValueError, match='negative or NaN'):
            dev.occupancy(C, r2)
    with pytest.raises(ValueError, match='32 coordinates'):
        dev.occupancy(np.zeros((3, 32)))
    for q in (0.0, 3.0, -2.0, np.inf):
        with pytest.raises(ValueError, match='power of two'):
            dev.occupancy(C, None, q)
    occ = dev.occupancy(C, [np.inf, 0.0, 4.0], 2.0 ** -20)           # +inf: no radius for that centre; 0 is a radius
    for args, msg in (((0, 5, -1), 'outside the ring'), ((-1, 1, -1), 'outside the ring'), ((0, 4, 1), 'dwell slots'),
                      ((0, 0, -1), 'n must be >= 1')):
        with pytest.raises(EngineError, match=msg):
            occ.accumulate(args[0], args[1], w_slot0=args[2])
    assert occ.read()['n_states'] == 0
    occ.accumulate(0, 3, w_slot0=1)
    assert occ.read()['n_states'] == 300
    dev.ring_alloc(9)                                               # a new ring: the scratch was sized for the old one
    with pytest.raises(EngineError, match='re-allocated'):
        occ.accumulate(0, 1)
    occ.close()
    alive = dev.occupancy(C)
    dev.close()                                                     # the sampler frees what is still alive on it
    alive.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5.  cells in the space of functional values
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K,M', [(3, 5), (2, 64)])
def test_on_projections(K, M):
    D, n, N, q = 33, 4, 130, 2.0 ** -20
    rs = np.random.RandomState(K)
    w = rs.standard_exponential((n, N)) + 0.1
    ctx, dev, stored = _ring(rs.randn(D, n, N), 'float64', w)
    fn = dev.projections(rs.randn(K, D) / math.sqrt(D))
    fn.ring_alloc(n)
    fn.evaluate(0, n, 0)
    vals = fn.read(0, n)                                            # (K, n, N)
    C = rs.randn(M, K)
    r2 = np.full(M, 0.5)
    occ = fn.occupancy(C, r2, q)
    assert occ.info()[:2] == (M, K)
    occ.accumulate(0, n, w_slot0=0)
    labels, want = _want(vals, w, C, r2, q)
    assert np.array_equal(occ.read_labels(n), labels)
    _same(occ.read(chains=True), want, 'of projections')
    assert 0 < want['count'][M] < n * N
    with pytest.raises(ValueError, match='derived ring'):
        fn.occupancy(np.zeros((2, D)))
    dev.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6.  through the sampler
# ---------------------------------------------------------------------------------------------------------------------
def _centres(D):
    C = np.zeros((3, D))
    C[0, 0], C[2, 0] = -1.0, 2.0
    C[1, :2] = 0.5
    return C


@pytest.mark.parametrize('cls', ['HMC', 'ControlHMC', 'MarkovJumpHMC'])
def test_driver_leaves_the_sampler_as_expectations_does(cls):
    """occupancy(30, block=7): counters, dwelling times, final state and RNG tick as expectations(30) from the same seed;
    the tables equal the oracle on the same chain recorded in one ring"""
    from tests.test_gpu_chainstats import _iso, record
    n_iter, D, N = 30, 24, 301
    C, radius = _centres(D), np.array([6.0, 7.0, 6.5])
    s = _iso(D, N, 5, cls)
    tick0, grad0 = s._dev.get_tick(), s.distribution.dEdX_count
    for kwargs in (dict(n_iter=1), dict(centres=np.zeros((2, D + 1))), dict(centres=np.zeros((65, D))), dict(radius=-1.0)):
        args = dict(n_iter=4, centres=C)
        args.update(kwargs)
        with pytest.raises(ValueError):
            s.occupancy(**args)
    assert (s._dev.get_tick(), s._dev.ring_slots) == (tick0, 0)
    o = s.occupancy(n_iter, C, radius=radius, block=7)
    lead = 1 if s._dwell_weighted else 0
    assert s._dev.get_tick() - tick0 == n_iter + lead
    ref = _iso(D, N, 5, cls)
    ref.expectations(n_iter, block=11, shift=np.zeros(D))
    assert (s.l_count, s.f_count, s.r_count, s.fl_count) == (ref.l_count, ref.f_count, ref.r_count, ref.fl_count)
    assert (s.distribution.E_count, s.distribution.dEdX_count) == (ref.distribution.E_count, ref.distribution.dEdX_count)
    assert np.array_equal(s.state.X, ref.state.X) and np.array_equal(s.state.V, ref.state.V)
    assert s._dev.get_tick() == ref._dev.get_tick()
    if lead:
        assert np.array_equal(s.dwelling_times, ref.dwelling_times)
    X, w, _ = record(_iso(D, N, 5, cls), n_iter)
    X = X[:, :n_iter, :]
    q = 2.0 ** (math.floor(math.log2(w[:7].mean())) - 24) if lead else 1.0
    assert o.quantum == q
    _, want = _want(X, w, C, radius * radius, q)
    got = dict(o.tables, switches=want['switches'], visited=want['visited'])       # (the driver downloads no per-chain values)
    _same(got, want, 'driver ' + cls)
    assert o.n_states == n_iter * N and o.grad_evals == s.distribution.dEdX_count - grad0 > 0 and o.n_chains == N
    assert abs(o.weight.sum() - 1.0) < 1e-12 and o.crossings == int(want['switches'].sum())


@pytest.mark.parametrize('cls', ['HMC', 'MarkovJumpHMC'])
def test_result_does_not_depend_on_the_block(cls):
    from tests.test_gpu_chainstats import _iso
    n_iter, D, N = 10, 5, 130
    C = _centres(D)
    runs = [_iso(D, N, 9, cls).occupancy(n_iter, C, radius=3.0, block=b) for b in (1, 3, None)]
    for o in runs[1:]:
        # (a jump sampler takes its quantum from the first block, which differs: compare counts, and units per quantum)
        for name in ('count', 'from_count', 'trans', 'chains_by_switches', 'chains_by_cells'):
            assert np.array_equal(o.tables[name], runs[0].tables[name]), name
        if o.quantum == runs[0].quantum:
            assert np.array_equal(o.units, runs[0].units) and np.array_equal(o.from_units, runs[0].from_units)
            assert o.W_units == runs[0].W_units
    if cls == 'HMC':
        assert all(o.quantum == 1.0 for o in runs)


def _Phi(x):
    return 0.5 * (1.0 + math.erf(x / math.sqrt(2.0)))


@pytest.mark.parametrize('cls', ['HMC', 'ControlHMC', 'MarkovJumpHMC'])
def test_known_answer_with_negative_control(cls):
    """TestGaussian(ndims=2, nbatch=4096, sigma=1) started from exact draws, 8 states per chain, centres (-2, 0), (0, 0),
    (2, 0): the cell boundaries are x_0 = -/+ 1, the exact weights Phi(-1), 1 - 2 Phi(-1), Phi(-1).  The chains are
    independent and each starts in equilibrium, so the variance of a weight is at most p (1 - p) / 4096 whatever the mixing:
    |weight - p| <= 6 sqrt(p (1 - p) / 4096), that is 0.034 / 0.044 / 0.034 -- derived, not measured.  Negative control:
    sigma = 1.3 started from 1.3 randn has the exact weights 0.221 / 0.558 / 0.221, off by 0.062 / 0.124 / 0.062, and must
    miss every one of the same bounds."""
    from mjhmc_amd.misc.distributions import TestGaussian
    from mjhmc_amd.samplers import markov_jump_hmc as mj
    N, n_iter = 4096, 8
    C = np.array([[-2.0, 0.0], [0.0, 0.0], [2.0, 0.0]])
    p = np.array([_Phi(-1.0), 1.0 - 2.0 * _Phi(-1.0), _Phi(-1.0)])
    bound = 6.0 * np.sqrt(p * (1.0 - p) / N)
    assert np.allclose(bound, [0.034, 0.044, 0.034], atol=5e-4)

    def run(sigma):
        X0 = sigma * np.random.RandomState(17).randn(2, N)

        class Fixed(TestGaussian):
            def gen_init_X(self):
                self.Xinit = X0
        kw = dict(resample=False) if cls == 'MarkovJumpHMC' else {}
        s = getattr(mj, cls)(distribution=Fixed(ndims=2, nbatch=N, sigma=sigma), epsilon=0.3, beta=0.3, num_leapfrog_steps=5,
                             seed=23, **kw)
        o = s.occupancy(n_iter, C)
        assert o.n_states == n_iter * N and o.counts[3] == 0 and abs(o.weight.sum() - 1.0) < 1e-12
        return o.weight[:3]

    weight = run(1.0)
    print('%s: weights %s, exact %s, |difference| %s, bound %s' % (cls, weight, p, np.abs(weight - p), bound))
    control = run(1.3)
    print('%s: control weights %s, |difference| %s' % (cls, control, np.abs(control - p)))
    assert np.all(np.abs(weight - p) <= bound), (weight, p, bound)
    assert np.all(np.abs(control - p) > bound), (control, p, bound)


def test_bookkeeping_on_the_multimodal_gaussian():
    """integer identities only, no statistical claim"""
    from mjhmc_amd.misc.distributions import MultimodalGaussian
    from mjhmc_amd.samplers.markov_jump_hmc import MarkovJumpHMC
    N, n = 512, 12
    np.random.seed(3)
    d = MultimodalGaussian(ndims=2, nbatch=N)
    assert d.modes().tolist() == [[-6.0, 0.0], [6.0, 0.0]]
    s = MarkovJumpHMC(distribution=d, epsilon=0.3, beta=0.3, num_leapfrog_steps=5, seed=4, resample=False)
    # (the driver keeps the handle to itself: the same run through it and, for the per-chain values, by hand)
    o = s.occupancy(n, d.modes(), block=5)
    assert int(o.counts.sum()) == N * n == o.n_states
    assert int(o.trans.sum()) == N * (n - 1)
    assert np.array_equal(o.trans.sum(axis=1), o.from_counts)
    assert int(o.chains_by_cells.sum()) == N and int(o.chains_by_switches.sum()) == N
    assert int(o.units.sum()) == o.W_units and int(o.from_units.sum()) <= o.W_units
    assert o.crossings == int(o.trans.sum() - np.trace(o.trans))
    assert o.transition_matrix().shape == (3, 3) and np.allclose(o.transition_matrix().sum(axis=1), 1.0)
    assert np.allclose(o.rate_matrix().sum(axis=1), 0.0, atol=1e-9)
    # crossings = sum_p switches, on a handle whose per-chain values are read
    dev = s._dev
    occ = dev.occupancy(d.modes(), None, o.quantum)
    s._run(6, ring_slot0=0)
    occ.accumulate(0, 5, w_slot0=1)
    t = occ.read(chains=True)
    assert int(t['trans'].sum() - np.trace(t['trans'])) == int(t['switches'].sum(dtype=np.uint64))
    assert int(t['chains_by_switches'][0]) == int(np.sum(t['switches'] == 0))
    occ.close()
