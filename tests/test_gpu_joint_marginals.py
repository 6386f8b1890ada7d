"""GPU: dwell-weighted joint histograms of pairs of dimensions on the device (csrc/pairhist.hip, DevicePairHistogram,
HMCBase.joint_marginals).

The definition (include/mjhmc_hip.h: mjhmc_pairhist_create) is integer arithmetic behind two rounded float64 operations
per axis; ``host_pairhist`` restates it in NumPy (whose elementwise float64 operations round once each and never fuse) and
every comparison of tables is ``==``.  Rings are written through the test build's hooks, one dwell entry per call: n * N
stays in the low thousands."""
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LDS_BUDGET, MAX_GROUP = 65536, 8          # csrc/pairhist.hpp (tests/test_joint_marginals_cpu.py reads them from there)


def group_of(B):
    """pairs a workgroup bins at B bins per axis; 0: the global form"""
    return min(MAX_GROUP, LDS_BUDGET // ((B + 2) ** 2 * 12))


# ---------------------------------------------------------------------------------------------------------------------
# the NumPy restatement
# ---------------------------------------------------------------------------------------------------------------------
def host_axis_bins(x, lo, hi, B):
    """x float64 of any shape, scalar lo < hi -> bin indices: t = (x - lo) * inv with inv = B / (hi - lo); 0 when
    !(t >= 0) (NaN too), B + 1 when t >= B, 1 + (int)t otherwise"""
    inv = np.float64(B) / (np.float64(hi) - np.float64(lo))
    with np.errstate(invalid='ignore', over='ignore'):
        d = x - np.float64(lo)
        t = d * inv
        inside = (t >= 0) & (t < B)
        inner = 1 + np.where(inside, t, 0.0).astype(np.int64)
        return np.where(~(t >= 0), 0, np.where(t >= B, B + 1, inner))


def host_units(w, q):
    """u = rint(w / q), nearest-even, as unsigned 64-bit integers"""
    return np.rint(w / q).astype(np.uint64)


def host_pairhist(X, w, pairs, lo, hi, B, q):
    """X (D, n, N) float64 states as the ring holds them, w (n, N) weights, pairs (P, 2), lo / hi (P, 2) ->
    count, mass (P, B + 2, B + 2) uint64 indexed [pair][bin of j][bin of i], W_units"""
    P, nb = len(pairs), B + 2
    u = host_units(w, q).ravel()
    count, mass = np.zeros((P, nb * nb), dtype=np.uint64), np.zeros((P, nb * nb), dtype=np.uint64)
    for p, (i, j) in enumerate(pairs):
        b0 = host_axis_bins(X[i], lo[p, 0], hi[p, 0], B).ravel()
        b1 = host_axis_bins(X[j], lo[p, 1], hi[p, 1], B).ravel()
        cell = b1 * nb + b0
        count[p] = np.bincount(cell, minlength=nb * nb).astype(np.uint64)
        np.add.at(mass[p], cell, u)
    return count.reshape(P, nb, nb), mass.reshape(P, nb, nb), int(u.sum(dtype=np.uint64))


def _same_tables(got, want, tag):
    for name, g, h in zip(('count', 'mass'), got[:2], want[:2]):
        assert g.shape == h.shape and g.dtype == np.uint64, (tag, name, g.shape, h.shape)
        bad = int(np.sum(g != h))
        assert bad == 0, '%s %s: %d of %d cells differ' % (tag, name, bad, h.size)
    assert got[2] == want[2], (tag, 'W_units', got[2], want[2])


def _ring(*args, **kwargs):
    from tests.test_gpu_marginals import _ring as ring
    return ring(*args, **kwargs)


def _dim_ranges(D):
    """dimension 0: a dyadic range (every edge is a float64, a bfloat16 for small B); the others irregular"""
    return -2.0 - 0.013 * np.arange(D), 2.0 + 0.031 * np.arange(D)


def _pairs(D, P, seed=0):
    """both orders of a pair, a diagonal pair and a repeated pair first, then random ones (diagonals among them)"""
    a, b = 0, D - 1
    head = [(a, b), (b, a), (1 % D, 1 % D), (a, b), (D // 2, a)]
    rs = np.random.RandomState(seed)
    rest = [tuple(int(v) for v in rs.randint(0, D, size=2)) for _ in range(max(0, P - len(head)))]
    return np.array((head + rest)[:P], dtype=np.int32)


def _pair_ranges(pairs, lo_d, hi_d):
    """per pair and axis: the dimension's range, moved a little from pair to pair (pair 0 keeps it: values planted on its
    edges sit on edges)"""
    shift = 0.0071 * (np.arange(len(pairs)) % 3)
    return lo_d[pairs] - shift[:, None], hi_d[pairs] + 2.0 * shift[:, None]


def _states(D, n, N, B, lo, hi, pairs, seed):
    """normal draws wider than the range; in every dimension values exactly on computed edges, below lo, at lo, at hi,
    beyond hi, signed zeros, infinities and NaN; and whole states in each of the four corner cells of every pair (i != j)"""
    rs = np.random.RandomState(seed)
    X = rs.randn(D, n, N) * 1.5
    flat = X.reshape(D, -1)
    for d in range(D):
        sp = np.concatenate([lo[d] + np.arange(B + 1) * ((hi[d] - lo[d]) / B),
                             [lo[d], hi[d], np.nextafter(lo[d], -np.inf), np.nextafter(hi[d], -np.inf), lo[d] - 1.0, hi[d] + 3.0,
                              0.0, -0.0, np.inf, -np.inf, np.nan]])
        m = min(sp.size, flat.shape[1])
        flat[d, rs.choice(flat.shape[1], size=m, replace=False)] = rs.permutation(sp)[:m]
    # corners: whole states below / above in every dimension, and split by the dimension's rank in each pair
    at = rs.choice(flat.shape[1], size=min(flat.shape[1], 2 + 2 * len(pairs)), replace=False)
    for t, col in enumerate(at):
        if t == 0:
            flat[:, col] = lo - 1.0
        elif t == 1:
            flat[:, col] = hi + 3.0
        else:
            i, j = pairs[(t - 2) // 2]
            down, up = (i, j) if t % 2 == 0 else (j, i)
            flat[up, col] = hi[up] + 3.0
            flat[down, col] = lo[down] - 1.0               # (i == j: below)
    return X


# state type, ndims, N, B, P.  Every N of {1, 63, 65, 333}, D of {2, 5, 33} (512: bfloat16), B of {1, 7, 32, 64, 128} and
# the two B around the switch from LDS tables to the global form (71, 72); P of {1, 3, 64}, the largest group of pairs of
# a workgroup and one more (8 and 9 at B = 7, 4 and 5 at B = 32)
DEFINITION_CASES = [
    ('float64', 33, 65, 7, 8), ('float64', 33, 63, 7, 9), ('float64', 5, 333, 32, 4), ('float64', 5, 65, 32, 5),
    ('float64', 2, 333, 64, 3), ('float64', 33, 1, 1, 64), ('float64', 5, 65, 71, 3), ('float64', 5, 63, 72, 3),
    ('float64', 33, 333, 128, 1),
    ('float32', 5, 63, 7, 3), ('float32', 33, 65, 128, 3), ('float32', 2, 333, 64, 1), ('float32', 33, 1, 32, 64),
    ('float32', 5, 65, 72, 9),
    ('bfloat16', 512, 65, 32, 5), ('bfloat16', 512, 63, 72, 3), ('bfloat16', 512, 1, 1, 1), ('bfloat16', 512, 333, 7, 9),
    ('bfloat16', 512, 65, 71, 64),
]


def test_the_cases_stand_on_both_sides_of_every_switch():
    assert group_of(71) == 1 and group_of(72) == 0 and group_of(7) == 8 and group_of(32) == 4 and group_of(64) == 1
    Bs = {c[3] for c in DEFINITION_CASES}
    assert {1, 7, 32, 64, 128, 71, 72} <= Bs
    for dtype in ('float64', 'float32', 'bfloat16'):
        assert {group_of(c[3]) > 0 for c in DEFINITION_CASES if c[0] == dtype} == {True, False}, dtype
    assert {(7, 8), (7, 9), (32, 4), (32, 5)} <= {(c[3], c[4]) for c in DEFINITION_CASES}


# ---------------------------------------------------------------------------------------------------------------------
# 1.  the definition, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype,D,N,B,P', DEFINITION_CASES)
def test_definition_bit_for_bit(dtype, D, N, B, P):
    """count, mass, W_units and n_states == the NumPy restatement, for the dwell pairing (weights of all magnitudes around
    the quantum, zero among them) and for unit weights (two quanta)"""
    n = 3
    lo_d, hi_d = _dim_ranges(D)
    pairs = _pairs(D, P, seed=B + P)
    lo, hi = _pair_ranges(pairs, lo_d, hi_d)
    rs = np.random.RandomState(N + B)
    w = rs.standard_exponential((n, N)) * 10.0 ** rs.randint(-4, 3, size=(n, N))
    w.reshape(-1)[:: 7] = 0.0
    q = 2.0 ** -20
    ctx, dev, X = _ring(_states(D, n, N, B, lo_d, hi_d, pairs, seed=B + N), dtype, w)
    if dtype != 'float64':
        assert np.array_equal(X[np.isfinite(X)], X[np.isfinite(X)].astype(np.float32))
    h = dev.pair_histogram(pairs, B, lo, hi, q)
    h.accumulate(0, n, w_slot0=0)
    got = h.read()
    want = host_pairhist(X, w, pairs, lo, hi, B, q)
    _same_tables(got, want, 'dwell')
    assert got[3] == n * N
    assert np.all(got[0].reshape(P, -1).sum(axis=1) == n * N) and np.all(got[1].reshape(P, -1).sum(axis=1) == got[2])
    if n * N >= 2 + 2 * P and D > 1:
        for p, (i, j) in enumerate(pairs):                  # the planted corner states: all four corner cells are occupied
            corners = got[0][p][[0, 0, -1, -1], [0, -1, 0, -1]]
            assert np.all(corners >= 1) if i != j else (corners[0] >= 1 and corners[3] >= 1 and corners[1] == corners[2] == 0), (p, corners)
    if n * N >= B + 12:
        assert np.isnan(X).any() and np.isinf(X).any()
    h.close()
    for qu in (1.0, 0.125):
        hu = dev.pair_histogram(pairs, B, lo, hi, qu)
        hu.accumulate(0, n, w_slot0=-1)
        gu = hu.read()
        _same_tables(gu, host_pairhist(X, np.ones((n, N)), pairs, lo, hi, B, qu), 'unit weights, q = %g' % qu)
        assert gu[3] == n * N
        hu.close()
    dev.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2.  transposition, and the marginals of the 1-D pass
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype,D,N,B', [('float64', 5, 333, 32), ('float32', 33, 65, 128), ('bfloat16', 512, 63, 7), ('float64', 2, 65, 72)])
def test_transposition_and_marginal_consistency(dtype, D, N, B):
    """with one range per dimension: pair (j, i)'s tables are the transposes of pair (i, j)'s, and a pair's tables summed
    over either axis (all B + 2 entries) are the rows of the device 1-D histogram (mjhmc_histogram) of the same block,
    range, B and q -- exactly"""
    n = 3
    lo_d, hi_d = _dim_ranges(D)
    pairs = np.array([(0, D - 1), (D - 1, 0), (1, 1), (D // 2, 1), (1, D // 2), (0, D - 1)], dtype=np.int32)
    rs = np.random.RandomState(B)
    w = rs.standard_exponential((n, N)) + 1e-3
    q = 2.0 ** -22
    ctx, dev, X = _ring(_states(D, n, N, B, lo_d, hi_d, pairs, seed=N), dtype, w)
    for w_slot0 in (0, -1):
        h2 = dev.pair_histogram(pairs, B, lo_d[pairs], hi_d[pairs], q)
        h1 = dev.histogram(B, lo_d, hi_d, q)
        h2.accumulate(0, n, w_slot0=w_slot0)
        h1.accumulate(0, n, w_slot0=w_slot0)
        count, mass, W, ns = h2.read()
        c1, m1, W1, ns1 = h1.read()
        assert (W, ns) == (W1, ns1)
        for a, b in ((0, 1), (3, 4)):
            assert np.array_equal(count[a], count[b].T) and np.array_equal(mass[a], mass[b].T), (a, b)
        assert np.array_equal(count[0], count[5]) and np.array_equal(mass[0], mass[5])          # the repeated pair
        off = ~np.eye(B + 2, dtype=bool)
        assert not count[2][off].any() and not mass[2][off].any()                                # (i, i) lives on the diagonal
        for p, (i, j) in enumerate(pairs):
            for tab, one in ((count, c1), (mass, m1)):
                assert np.array_equal(tab[p].sum(axis=0, dtype=np.uint64), one[i]), (p, 'i axis')   # summed over the j axis
                assert np.array_equal(tab[p].sum(axis=1, dtype=np.uint64), one[j]), (p, 'j axis')
        h2.close()
        h1.close()
    dev.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3.  independence of the blocks
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype,D,N,B,P', [('float64', 33, 333, 32, 5), ('float32', 5, 130, 128, 3), ('bfloat16', 512, 65, 64, 2)])
def test_block_independence(dtype, D, N, B, P):
    """one call, blocks of one slot, an uneven cut, the calls in another order, and a second run on a fresh sampler: the
    same tables"""
    n = 6
    lo_d, hi_d = _dim_ranges(D)
    pairs = _pairs(D, P, seed=1)
    lo, hi = _pair_ranges(pairs, lo_d, hi_d)
    w = np.random.RandomState(3).standard_exponential((n, N)) + 1e-3
    q = 2.0 ** -24
    results = []
    for run in range(2):
        ctx, dev, X = _ring(_states(D, n, N, B, lo_d, hi_d, pairs, seed=9), dtype, w)
        h = dev.pair_histogram(pairs, B, lo, hi, q)
        cuts = ([(0, n)], [(k, 1) for k in range(n)], [(0, 2), (2, 1), (3, n - 3)], [(3, 3), (0, 3)],
                [(4, 2), (1, 3), (0, 1)]) if run == 0 else ([(0, 4), (4, 2)],)
        for calls in cuts:
            h.reset()
            for at, k in calls:
                h.accumulate(at, k, w_slot0=at)
            results.append(h.read())
            assert results[-1][3] == n * N
        if run == 0:
            want = host_pairhist(X, w, pairs, lo, hi, B, q)
        dev.close()
    for i, r in enumerate(results):
        _same_tables(r, want, 'cut %d' % i)


# ---------------------------------------------------------------------------------------------------------------------
# 4.  padding rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype,D,N,B', [('float64', 5, 1, 16), ('float64', 33, 65, 72), ('float32', 6, 63, 16), ('bfloat16', 512, 65, 16),
                                          ('float32', 2, 1, 128), ('float64', 3, 63, 7)])
def test_padding_rows_do_not_contribute(dtype, D, N, B):
    """rows N <= p < Npad of every slot, and the dwell ring's padding entries, filled with 0xFF bytes (NaN as a state of
    every type and as a weight): a pass that read them would count them in the corner cell, a check that read them would
    refuse the block"""
    from mjhmc_amd import engine
    n = 3
    lo_d, hi_d = _dim_ranges(D)
    pairs = _pairs(D, 3)
    lo, hi = _pair_ranges(pairs, lo_d, hi_d)
    rs = np.random.RandomState(N)
    w = rs.standard_exponential((n, N)) + 0.5
    ctx, dev, X = _ring(rs.randn(D, n, N), dtype, w)
    for k in range(n):
        engine.check(ctx.lib.mjhmc_test_ring_fill_padding(dev.handle, k, 0xFF), ctx.lib)
    assert np.array_equal(dev.ring_read(0, n).reshape(D, n, N), X)
    q = 2.0 ** -16
    h = dev.pair_histogram(pairs, B, lo, hi, q)
    h.accumulate(0, n, w_slot0=0)
    _same_tables(h.read(), host_pairhist(X, w, pairs, lo, hi, B, q), 'padding, dwell')
    h.reset()
    h.accumulate(0, n, w_slot0=-1)
    got = h.read()
    _same_tables(got, host_pairhist(X, np.ones((n, N)), pairs, lo, hi, B, q), 'padding, unit')
    assert np.all(got[0].reshape(3, -1).sum(axis=1) == n * N)
    dev.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5.  refusals add nothing
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', [32, 96])
def test_refusals_add_nothing(B):
    """the 1-D pass's refusals, codes and wording (tests/test_gpu_marginals.py), in both forms of the pass"""
    from mjhmc_amd import engine, _lib
    D, n, N = 7, 4, 70
    lo_d, hi_d = _dim_ranges(D)
    pairs = _pairs(D, 5)
    lo, hi = _pair_ranges(pairs, lo_d, hi_d)
    rs = np.random.RandomState(2)
    w = rs.standard_exponential((n, N)) + 0.1
    q = 2.0 ** -30
    ctx, dev, X = _ring(rs.randn(D, n, N), 'float64', w)
    h = dev.pair_histogram(pairs, B, lo, hi, q)
    h1 = dev.histogram(B, lo_d, hi_d, q)
    h.accumulate(0, 2, w_slot0=0)
    before = h.read()
    _same_tables(before, host_pairhist(X[:, :2], w[:2], pairs, lo, hi, B, q), 'first block')

    def poke(value):
        engine.check(ctx.lib.mjhmc_test_ring_write_dwell(dev.handle, 3, 17, float(value)), ctx.lib)

    for value, code, msg in ((float('inf'), _lib.ERR_NONFINITE, 'not finite'), (float('nan'), _lib.ERR_NONFINITE, 'not finite'),
                             (-0.25, _lib.ERR_NONFINITE, 'negative'), (q * 2.0 ** 53, -1, '2\\^53'), (1e300, -1, '2\\^53')):
        poke(value)
        with pytest.raises(_lib.EngineError, match=msg):
            h.accumulate(2, 2, w_slot0=2)
        assert ctx.lib.mjhmc_pairhist_accumulate(h.handle, 2, 2, 2) == code, value
        text = ctx.lib.mjhmc_last_error()
        assert ctx.lib.mjhmc_histogram_accumulate(h1.handle, 2, 2, 2) == code and ctx.lib.mjhmc_last_error() == text, value
        after = h.read()
        _same_tables(after, before, 'after a refused block (%r)' % value)
        assert after[3] == before[3] == 2 * N
    poke(q * (2.0 ** 53 - 1.0))                                 # the largest weight the quantum takes
    w[3, 17] = q * (2.0 ** 53 - 1.0)
    h.accumulate(2, 2, w_slot0=2)                               # the flags do not stick
    _same_tables(h.read(), host_pairhist(X, w, pairs, lo, hi, B, q), 'after the refusals')
    dev.close()


def test_total_of_two_to_the_63_is_refused():
    """600 weights of 2^53 - 1 quanta are about 2^62.2 quanta: one slot of them fits, two reach 2^63"""
    from mjhmc_amd import _lib
    D, B, N, q = 2, 8, 600, 2.0 ** -40
    lo_d, hi_d = _dim_ranges(D)
    pairs = _pairs(D, 2)
    big = q * (2.0 ** 53 - 1.0)
    assert 2 * N * (2 ** 53 - 1) >= 2 ** 63 > N * (2 ** 53 - 1)
    ctx, dev, X = _ring(np.random.RandomState(4).randn(D, 2, N), 'float64', np.full((2, N), big))
    h = dev.pair_histogram(pairs, B, lo_d[pairs], hi_d[pairs], q)
    with pytest.raises(_lib.EngineError, match='2\\^63'):
        h.accumulate(0, 2, w_slot0=0)
    assert ctx.lib.mjhmc_pairhist_accumulate(h.handle, 0, 0, 2) == -1
    got = h.read()
    assert not got[0].any() and not got[1].any() and got[2:] == (0, 0)
    h.accumulate(0, 1, w_slot0=0)
    before = h.read()
    assert before[2] == N * (2 ** 53 - 1) and before[3] == N
    with pytest.raises(_lib.EngineError, match='2\\^63'):
        h.accumulate(1, 1, w_slot0=1)
    _same_tables(h.read(), before, 'after the refused second block')
    hu = dev.pair_histogram(pairs, B, lo_d[pairs], hi_d[pairs], 2.0 ** -60)      # a unit weight of 2^60 quanta
    with pytest.raises(_lib.EngineError, match='2\\^53'):
        hu.accumulate(0, 1, w_slot0=-1)
    assert not hu.read()[0].any()
    dev.close()


def test_invalid_arguments():
    import ctypes
    from mjhmc_amd._lib import EngineError, ptr
    from tests.test_gpu_chainstats import _iso
    s = _iso(33, 100, 1)
    dev = s._dev
    ok = [(0, 1), (5, 32)]
    with pytest.raises(EngineError, match='no sample ring'):
        dev.pair_histogram(ok, 16, -1.0, 1.0)
    dev.ring_alloc(4)
    s._run(4, ring_slot0=0)
    for pairs in (np.zeros((0, 2), dtype=np.int32), [(0, 1)] * 65):
        with pytest.raises(EngineError, match=r'n_pairs must be in \[1, 64\]'):
            dev.pair_histogram(pairs, 16, -1.0, 1.0)
    for pairs in ([(0, 33)], [(-1, 0)], [(0, 1), (2, 3), (33, 0)]):
        with pytest.raises(EngineError, match='outside'):
            dev.pair_histogram(pairs, 16, -1.0, 1.0)
    for bins in (0, 129):
        with pytest.raises(EngineError, match=r'n_bins must be in \[1, 128\]'):
            dev.pair_histogram(ok, bins, -1.0, 1.0)
    two = np.array([[0.0, 0.0], [0.0, 1.0]])
    for lo, hi, msg in ((1.0, 1.0, 'lo must be below hi'), (2.0, 1.0, 'lo must be below hi'), (-np.inf, 1.0, 'not finite'),
                        (0.0, np.nan, 'not finite'), (two, 1.0, 'pair 1, axis 1')):
        with pytest.raises(EngineError, match=msg):
            dev.pair_histogram(ok, 16, lo, hi)
    for q in (0.0, 3.0, -2.0, np.inf):
        with pytest.raises(EngineError, match='power of two'):
            dev.pair_histogram(ok, 16, -1.0, 1.0, q)
    with pytest.raises(ValueError):
        dev.pair_histogram(ok, 16, np.zeros(5), 1.0)
    pr, lo, hi = np.array(ok, dtype=np.int32), np.full((2, 2), -1.0), np.full((2, 2), 1.0)
    out = ctypes.c_void_p()
    good = [dev.handle, 2, ptr(pr), 16, ptr(lo), ptr(hi), 0.5, ctypes.byref(out)]
    for at in (0, 2, 4, 5, 7):
        args = list(good)
        args[at] = None
        assert dev.lib.mjhmc_pairhist_create(*args) == -1 and b'NULL argument' in dev.lib.mjhmc_last_error(), at
    assert out.value is None
    h = dev.pair_histogram(ok, 16, -4.0, 4.0, 2.0 ** -20)
    for args, msg in (((0, 5, -1), 'outside the ring'), ((3, 2, -1), 'outside the ring'), ((-1, 1, -1), 'outside the ring'),
                      ((0, 4, 1), 'dwell slots'), ((0, 1, -2), 'dwell slots'), ((0, 0, -1), 'n must be >= 1')):
        with pytest.raises(EngineError, match=msg):
            h.accumulate(args[0], args[1], w_slot0=args[2])
    assert h.read()[2:] == (0, 0) and not h.read()[0].any()
    h.accumulate(0, 3, w_slot0=1)
    assert h.read()[3] == 300
    h.reset()
    assert h.read()[2:] == (0, 0) and not h.read()[0].any()
    dev.ring_alloc(9)                                               # a new ring: the handle belongs to the old one
    with pytest.raises(EngineError, match='re-allocated'):
        h.accumulate(0, 1)
    assert dev.lib.mjhmc_pairhist_accumulate(h.handle, 0, -1, 1) == -1
    assert not h.read()[0].any()
    h.close()
    alive = dev.pair_histogram(ok, 16, -4.0, 4.0)
    dev.close()                                                     # the sampler frees what is still alive on it
    alive.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6.  the driver
# ---------------------------------------------------------------------------------------------------------------------
def _same_run(s, t, lead):
    assert (s.l_count, s.f_count, s.r_count, s.fl_count) == (t.l_count, t.f_count, t.r_count, t.fl_count)
    assert (s.distribution.E_count, s.distribution.dEdX_count) == (t.distribution.E_count, t.distribution.dEdX_count)
    assert np.array_equal(s.state.X, t.state.X) and np.array_equal(s.state.V, t.state.V)
    assert s._dev.get_tick() == t._dev.get_tick()
    if lead:
        assert np.array_equal(s.dwelling_times, t.dwelling_times)


@pytest.mark.parametrize('cls', ['MarkovJumpHMC', 'ControlHMC'])
def test_driver_is_the_run_of_marginals(cls):
    """joint_marginals(30, pairs, block=7): counters, dwelling times, final state and RNG tick as marginals(30, block=7) from
    the same seed, the same range and quantum; the tables equal the NumPy definition on the same chain recorded in one
    ring; marginal(p, axis) equals marginals() of that dimension table for table"""
    from tests.test_gpu_chainstats import _iso, record
    n_iter, D, N, B = 30, 24, 301, 24
    pairs = np.array([(0, 23), (23, 0), (5, 5), (7, 2), (0, 23)])
    s, t = _iso(D, N, 5, cls), _iso(D, N, 5, cls)
    lead = 1 if s._dwell_weighted else 0
    tick0 = s._dev.get_tick()
    for kwargs in (dict(n_iter=0, pairs=pairs), dict(n_iter=4, pairs=pairs, bins=129), dict(n_iter=4, pairs=[(0, 24)]),
                   dict(n_iter=4, pairs=pairs, range=(1.0, 0.0))):
        with pytest.raises(ValueError):
            s.joint_marginals(**kwargs)
    assert (s._dev.get_tick(), s._dev.ring_slots) == (tick0, 0)
    jm = s.joint_marginals(n_iter, pairs, bins=B, block=7)
    m = t.marginals(n_iter, bins=B, block=7)
    assert s._dev.get_tick() - tick0 == n_iter + lead
    _same_run(s, t, lead)
    assert jm.quantum == m.quantum and (jm.W_units, jm.n_states) == (m.W_units, m.n_states) == (m.W_units, n_iter * N)
    assert np.array_equal(jm.lo, m.lo[pairs]) and np.array_equal(jm.hi, m.hi[pairs])
    assert jm.counts.shape == (5, B + 2, B + 2) and jm.density.shape == (5, B, B) and jm.edges_x.shape == (5, B + 1)
    X, w, w_slot0 = record(_iso(D, N, 5, cls), n_iter)
    X = X[:, :n_iter, :]
    want = host_pairhist(X, w, pairs, jm.lo, jm.hi, B, jm.quantum)
    _same_tables((jm.counts, jm.units, jm.W_units), want, 'driver ' + cls)
    for p, (i, j) in enumerate(pairs):
        for axis, d in ((0, i), (1, j)):
            one = jm.marginal(p, axis)
            assert np.array_equal(one.counts[0], m.counts[d]) and np.array_equal(one.units[0], m.units[d]), (p, axis)
            assert np.array_equal(one.edges[0], m.edges[d]) and np.array_equal(one.density[0], m.density[d])
            assert one.out_of_range[0] == m.out_of_range[d] and one.median[0] == m.median[d]
    assert np.all(jm.out_of_range <= 2.0 / 64)
    area = (jm.edges_x[:, 1] - jm.edges_x[:, 0]) * (jm.edges_y[:, 1] - jm.edges_y[:, 0])
    assert np.allclose(jm.density.sum(axis=(1, 2)) * area, 1.0 - jm.out_of_range, rtol=1e-12, atol=0)
    thr, mask = jm.hdr(0.5)
    assert mask.shape == (5, B, B) and np.all(mask.reshape(5, -1).sum(axis=1) >= 1)
    # a caller's range, scalars, whole run in one block
    s2 = _iso(D, N, 5, cls)
    j2 = s2.joint_marginals(n_iter, pairs, bins=B, range=(-6.0, 7.0))
    assert s2._dev.get_tick() == s._dev.get_tick()
    assert j2.quantum == (2.0 ** (math.floor(math.log2(w.mean())) - 24) if lead else 1.0)
    _same_tables((j2.counts, j2.units, j2.W_units),
                 host_pairhist(X, w, pairs, np.full((5, 2), -6.0), np.full((5, 2), 7.0), B, j2.quantum), 'driver, given range ' + cls)


def test_joint_of_functionals_on_the_funnel():
    """of=F with F = (x_0, sum_k x_k^2) on Neal's funnel: the joint of the derived ring equals the host definition applied
    to F's values of the same run (read back from a derived ring of a twin that recorded the run in one ring), and the run
    is that of marginals() on another twin"""
    from mjhmc_amd.misc.distributions import Funnel
    from mjhmc_amd.samplers.markov_jump_hmc import MarkovJumpHMC
    from tests.test_gpu_chainstats import record
    n_iter, B = 24, 40

    def funnel():
        np.random.seed(12)
        return MarkovJumpHMC(distribution=Funnel(ndims=8, nbatch=130), epsilon=0.1, beta=0.3, num_leapfrog_steps=5, seed=31,
                             resample=False)

    s, t, r = funnel(), funnel(), funnel()
    F = s.functionals(['S[0]', 'S[1]'], stats=['d == 0 ? x : 0.0', 'x * x'], names=['x0', 'r2'])
    pairs = [(0, 1), (1, 0), (1, 1)]
    lo, hi = np.array([-9.0, 0.0]), np.array([9.0, 200.0])
    jm = s.joint_marginals(n_iter, pairs, bins=B, range=(lo, hi), block=5, of=F)
    t.marginals(n_iter, bins=16, block=5)
    _same_run(s, t, 1)
    X, w, w_slot0 = record(r, n_iter)
    fn = r._dev.functionals(F.values, F.stats, F.params)
    fn.ring_alloc(n_iter)
    fn.evaluate(0, n_iter, 0)
    G = fn.read(0, n_iter)                                      # (2, n_iter, N)
    fn.close()
    assert np.array_equal(G[0], X[0, :n_iter]) and np.all(G[1] >= G[0] ** 2)
    assert jm.quantum == 2.0 ** (math.floor(math.log2(w[:5].mean())) - 24)
    pr = np.array(pairs)
    want = host_pairhist(G, w, pr, lo[pr], hi[pr], B, jm.quantum)
    _same_tables((jm.counts, jm.units, jm.W_units), want, 'of=F')
    assert jm.n_states == n_iter * 130 and np.array_equal(jm.counts[0], jm.counts[1].T)
    auto = s.joint_marginals(n_iter, [(0, 1)], bins=16, of=F)    # range and quantum from the first block's moments of F
    t.marginals(n_iter, bins=16)
    _same_run(s, t, 1)
    assert auto.lo.shape == (1, 2) and np.all(auto.lo < auto.hi) and auto.n_states == n_iter * 130


# ---------------------------------------------------------------------------------------------------------------------
# 7.  column shards on one GPU (the way tests/test_gpu_marginals.py runs them)
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
D, N, n_iter = 24, 301, 20
X0 = np.random.RandomState(5).randn(D, N) + 0.4
PAIRS = [(0, 23), (23, 0), (4, 4), (9, 2)]


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
for B, rng, block, agreed in ((32, None, 4 + 3 * comm.rank, 4), (96, (-5.0 - comm.rank, 6.0 + comm.rank), 9 - 4 * comm.rank, 5)):
    s = make(comm)
    t0 = s._dev.get_tick()
    m = s.joint_marginals(n_iter, PAIRS, bins=B, range=rng, block=block)
    assert s._dev.get_tick() - t0 == n_iter + 1, 'a rank ran more than the 21 iterations (a replayed or retried block)'
    packed = np.concatenate([m.lo.ravel(), m.hi.ravel(), [m.quantum]])
    both = comm.allreduce_f64(np.concatenate([packed, -packed]), 'max')
    assert np.array_equal(both[:packed.size], -both[packed.size:]), 'the shards used different ranges or quanta'
    if rng is not None:
        assert np.all(m.lo == -5.0) and np.all(m.hi == 6.0)
    assert m.n_states == n_iter * N
    if comm.rank == 0:
        s1 = make(None)
        lo_d, hi_d = np.zeros(D), np.ones(D)
        for (i, j), l, h in zip(PAIRS, m.lo, m.hi):
            lo_d[i], lo_d[j], hi_d[i], hi_d[j] = l[0], l[1], h[0], h[1]
        m1 = s1.joint_marginals(n_iter, PAIRS, bins=B, range=(lo_d, hi_d), block=agreed)
        assert m1.quantum == m.quantum and np.array_equal(m1.lo, m.lo) and np.array_equal(m1.hi, m.hi)
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
