"""CPU: the argument refusals of the mjhmc_histogram_* entry points that need no device, the arithmetic of ``Marginals`` on
a hand-made table, the sharded reduction's packing, and the wiring of csrc/histograms.hip into the build."""
import ctypes
import os
import re

import numpy as np
import pytest

from mjhmc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'mjhmc_amd', 'csrc')


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_every_entry_point_refuses_bad_arguments_with_a_message(lib):
    lo, hi = np.zeros(4), np.ones(4)
    out = ctypes.c_void_p()
    fake = ctypes.c_void_p(1)                     # never dereferenced: the checks below come before the sampler is touched
    for bins in (0, -3, 1025):
        assert lib.mjhmc_histogram_create(fake, bins, _lib.ptr(lo), _lib.ptr(hi), 1.0, ctypes.byref(out)) == -1
        assert b'n_bins must be in [1, 1024]' in lib.mjhmc_last_error()
    for q in (0.0, -1.0, 3.0, 0.3, float('inf'), float('nan'), 2.0 ** -1060, 2.0 ** 1023):
        assert lib.mjhmc_histogram_create(fake, 16, _lib.ptr(lo), _lib.ptr(hi), q, ctypes.byref(out)) == -1, q
        assert b'power of two' in lib.mjhmc_last_error(), q
    for args in ((None, 16, _lib.ptr(lo), _lib.ptr(hi), 0.5, ctypes.byref(out)), (fake, 16, None, _lib.ptr(hi), 0.5, ctypes.byref(out)),
                 (fake, 16, _lib.ptr(lo), None, 0.5, ctypes.byref(out)), (fake, 16, _lib.ptr(lo), _lib.ptr(hi), 0.5, None)):
        assert lib.mjhmc_histogram_create(*args) == -1
        assert b'NULL argument' in lib.mjhmc_last_error()
    assert out.value is None
    assert lib.mjhmc_histogram_accumulate(None, 0, -1, 1) == -1 and b'histogram is NULL' in lib.mjhmc_last_error()
    assert lib.mjhmc_histogram_reset(None) == -1 and b'histogram is NULL' in lib.mjhmc_last_error()
    W, n = ctypes.c_uint64(), ctypes.c_int64()
    assert lib.mjhmc_histogram_read(None, None, None, ctypes.byref(W), ctypes.byref(n)) == -1
    assert b'NULL argument' in lib.mjhmc_last_error()
    assert lib.mjhmc_histogram_destroy(None) == 0
    assert lib.mjhmc_abi_version() == 2


def test_binding_declares_the_histogram_entry_points():
    from mjhmc_amd import engine
    from mjhmc_amd.samplers.markov_jump_hmc import HMCBase, Marginals  # noqa: F401
    for name in ('create', 'destroy', 'accumulate', 'read', 'reset'):
        assert 'mjhmc_histogram_' + name in _lib.PROTOTYPES
    assert hasattr(engine, 'DeviceHistogram') and hasattr(engine.DeviceSampler, 'histogram') and hasattr(HMCBase, 'marginals')


def test_marginals_arithmetic_on_a_hand_made_table():
    from mjhmc_amd.samplers.markov_jump_hmc import Marginals
    # two dimensions of four bins; units chosen so that every ratio below is a dyadic fraction (exact in float64)
    units = np.array([[1, 2, 4, 1, 0, 0],           # one unit below lo, none above hi; bin 3 is empty
                      [0, 8, 8, 16, 16, 16]], dtype=np.uint64)
    counts = np.array([[1, 1, 2, 1, 0, 0], [0, 2, 2, 4, 4, 4]], dtype=np.uint64)
    # (the two rows have different totals here only to exercise each separately: one Marginals per row total)
    m0 = Marginals([0.0], [4.0], 4, 0.5, counts[:1], units[:1], 8, 5)
    m1 = Marginals([-2.0], [2.0], 4, 0.5, counts[1:], units[1:], 64, 16)
    assert m0.edges.shape == (1, 5) and np.array_equal(m0.edges[0], [0, 1, 2, 3, 4]) and np.array_equal(m1.edges[0], [-2, -1, 0, 1, 2])
    assert np.array_equal(m0.mass, 0.5 * units[:1]) and m0.total_weight == 4.0 and m0.n_states == 5 and m1.total_weight == 32.0
    assert np.array_equal(m0.counts, counts[:1])
    assert np.array_equal(m0.density[0], [0.25, 0.5, 0.125, 0.0]) and np.array_equal(m1.density[0], [0.125, 0.125, 0.25, 0.25])
    assert np.array_equal(m0.out_of_range, [0.125]) and np.array_equal(m1.out_of_range, [0.25])
    # cdf: exact at the edges (the underflow bin counts as below lo), linear inside a bin, NaN outside the range
    assert np.array_equal(m0.cdf(m0.edges[0])[0], [0.125, 0.375, 0.875, 1.0, 1.0])
    assert np.array_equal(m1.cdf(m1.edges[0])[0], [0.0, 0.125, 0.25, 0.5, 0.75])
    assert np.array_equal(m0.cdf([0.5, 1.25, 2.5])[0], [0.25, 0.5, 0.9375])
    assert np.all(np.isnan(m0.cdf([-0.001, 4.001, np.nan])))
    assert m0.cdf(1.25).shape == (1,) and m0.cdf(np.array([[1.25, 2.5]])).shape == (1, 2)
    # quantile is the inverse inside every bin that holds weight
    for m, xs in ((m0, [0.0, 0.25, 0.5, 1.0, 1.25, 1.75, 2.0, 2.5, 3.0]), (m1, [-2.0, -1.5, -0.75, 0.0, 0.125, 1.0, 1.5, 2.0])):
        assert np.array_equal(m.quantile(m.cdf(xs)), np.array([xs])), (m.quantile(m.cdf(xs)), xs)
    assert np.array_equal(m0.quantile(1.0), [3.0])              # the smallest x with cdf(x) = 1: the empty bin adds nothing
    assert np.array_equal(m0.median, [1.25]) and np.array_equal(m1.median, [1.0])
    lo50, hi50 = m0.interval(0.5)
    assert np.array_equal(lo50, [0.5]) and np.array_equal(hi50, [1.75])
    assert np.array_equal(np.concatenate(m1.interval(0.5)), [0.0, 2.0])
    # the answer lies in an outer bin: below lo for m0 (1/8 of the weight is there), above hi for m1 (1/4)
    with pytest.raises(ValueError, match='outer bin'):
        m0.quantile(0.0625)
    with pytest.raises(ValueError, match='outer bin'):
        m1.quantile(0.875)
    with pytest.raises(ValueError, match='outer bin'):
        m1.interval(0.75)
    with pytest.raises(ValueError):
        m0.quantile(1.5)
    with pytest.raises(ValueError):
        m0.interval(1.0)


def test_marginals_argument_checks_come_before_any_device_work():
    from mjhmc_amd.samplers.markov_jump_hmc import HMCBase
    s = HMCBase.__new__(HMCBase)
    s._dev, s.ndims = None, 4
    for kwargs in (dict(n_iter=0), dict(n_iter=3, bins=0), dict(n_iter=3, bins=1025), dict(n_iter=3, range=(0.0,)),
                   dict(n_iter=3, range=(np.zeros(3), 1.0)), dict(n_iter=3, range=(1.0, 1.0)), dict(n_iter=3, range=(0.0, np.inf)),
                   dict(n_iter=3, range=(np.zeros(4), np.array([1.0, 1.0, 0.0, 1.0]))), dict(n_iter=3, span=0.0)):
        with pytest.raises(ValueError):
            s.marginals(**kwargs)


def test_sharded_reduction_adds_the_integer_tables_in_one_collective():
    from mjhmc_amd.parallel import reduce_histogram

    class TwoEqualRanks(object):
        calls = 0

        def allreduce_ints(self, values, op='sum'):
            self.calls += 1
            assert op == 'sum' and np.asarray(values).dtype == np.int64
            return 2 * np.asarray(values)

    counts = np.arange(12, dtype=np.uint64).reshape(2, 6)
    units = counts * np.uint64(2 ** 40) + np.uint64(3)
    comm = TwoEqualRanks()
    c, u, W, n = reduce_histogram(comm, counts, units, 2 ** 61 + 1, 77)
    assert comm.calls == 1 and c.dtype == np.uint64 and u.dtype == np.uint64
    assert np.array_equal(c, 2 * counts) and np.array_equal(u, 2 * units) and (W, n) == (2 ** 62 + 2, 154)
    with pytest.raises(OverflowError):
        reduce_histogram(comm, counts, units, 2 ** 62, 77)


def test_sources_are_wired_into_all_three_makefile_lists():
    mk = open(os.path.join(CSRC, 'Makefile')).read()
    for var in ('SRCS', 'ASAN_SRCS', 'HOOKS_SRCS'):
        m = re.search(r'^%s\s*=\s*(.*)$' % var, mk, flags=re.M)
        assert m and 'histograms.hip' in m.group(1).split(), var
    assert mk.count('histograms.hpp') == 3              # a dependency of all three object rules
    assert os.path.exists(os.path.join(CSRC, 'histograms.hip')) and os.path.exists(os.path.join(CSRC, 'histograms.hpp'))


def test_histograms_use_integer_atomics_only():
    """the tables are exact because every sum is an integer: no atomicAdd on a float or double, no unsafe-fp-atomics"""
    src = open(os.path.join(CSRC, 'histograms.hip')).read()
    code = re.sub(r'//[^\n]*', '', src)
    adds = re.findall(r'atomicAdd\s*\(\s*&\s*(\w+)', code)
    assert adds, 'the binning is LDS / global integer atomics'
    for name in set(adds):
        decl = re.search(r'\b(u64|uint32_t|unsigned long long|unsigned int)\s*\*\s*(?:const\s+|__restrict__\s+)*%s\b' % name, code)
        assert decl, 'atomicAdd target %s is not declared as an unsigned integer pointer' % name
    for word in ('atomicAdd_f', 'unsafeAtomicAdd', 'atomic_add_f', '__hip_atomic_fetch_add', 'atomicExch', 'atomicCAS'):
        assert word not in code, word
    assert not re.search(r'atomicAdd\s*\(\s*\(?\s*(float|double)', code)
