"""CPU: the arithmetic of ``JointMarginals`` on hand-made integer tables, the host-side argument checks of
``joint_marginals`` and of the mjhmc_pairhist_* entry points that need no device, and the wiring of csrc/pairhist.hip into
the build."""
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


def _tables():
    """two pairs of three bins per axis, tables [j bin][i bin] with outer rows and columns; W_units = 64 for both.  Units
    are chosen so that every ratio below is a dyadic fraction (exact in float64)."""
    u0 = np.array([[0, 0, 0, 0, 0],
                   [0, 8, 4, 4, 0],
                   [0, 4, 16, 2, 0],
                   [0, 2, 8, 16, 0],
                   [0, 0, 0, 0, 0]], dtype=np.uint64)          # everything inside
    u1 = np.array([[1, 0, 2, 0, 1],
                   [0, 8, 8, 8, 4],
                   [2, 8, 8, 4, 0],
                   [0, 4, 4, 0, 0],
                   [1, 0, 0, 0, 1]], dtype=np.uint64)          # 12 of 64 units in outer cells; ties among the 8s and the 4s
    units = np.stack([u0, u1])
    counts = (units + np.uint64(1)) // np.uint64(2)
    assert int(u0.sum()) == 64 and int(u1.sum()) == 64
    return counts, units


def _jm():
    from mjhmc_amd.samplers.markov_jump_hmc import JointMarginals
    counts, units = _tables()
    lo = np.array([[0.0, -1.0], [-2.0, 0.0]])
    hi = np.array([[3.0, 2.0], [4.0, 1.5]])
    return JointMarginals([(0, 1), (2, 2)], lo, hi, 3, 0.5, counts, units, 64, 40), counts, units


def test_density_edges_and_out_of_range():
    m, counts, units = _jm()
    assert m.n_pairs == 2 and m.counts.shape == m.units.shape == (2, 5, 5) and m.density.shape == (2, 3, 3)
    assert np.array_equal(m.pairs, [[0, 1], [2, 2]]) and m.total_weight == 32.0 and m.n_states == 40
    assert np.array_equal(m.mass, 0.5 * units.astype(np.float64))
    assert m.edges_x.shape == m.edges_y.shape == (2, 4)
    assert np.array_equal(m.edges_x, [[0, 1, 2, 3], [-2, 0, 2, 4]]) and np.array_equal(m.edges_y, [[-1, 0, 1, 2], [0, 0.5, 1.0, 1.5]])
    assert np.array_equal(m.out_of_range, [0.0, 12.0 / 64])
    area = np.array([1.0 * 1.0, 2.0 * 0.5])
    assert np.array_equal(m.density.sum(axis=(1, 2)) * area, 1.0 - m.out_of_range)
    assert np.array_equal(m.density[0], units[0, 1:-1, 1:-1] / 64.0)
    assert m.density[1][0, 2] == 8 / 64.0 and m.density[1][2, 0] == 4 / 64.0       # [j bin][i bin]


def test_marginal_equals_a_marginals_of_the_summed_tables():
    from mjhmc_amd.samplers.markov_jump_hmc import Marginals
    m, counts, units = _jm()
    for p in range(2):
        for axis in range(2):
            got = m.marginal(p, axis)
            over = 0 if axis == 0 else 1                       # axis 0 (the i axis) is what remains after summing over j bins
            want = Marginals([m.lo[p, axis]], [m.hi[p, axis]], 3, 0.5, counts[p].sum(axis=over)[None], units[p].sum(axis=over)[None],
                             64, 40)
            for name in ('counts', 'units', 'edges', 'density', 'out_of_range', 'mass'):
                assert np.array_equal(getattr(got, name), getattr(want, name)), (p, axis, name)
            assert (got.W_units, got.n_states, got.quantum, got.bins) == (64, 40, 0.5, 3)
            assert int(got.units.sum()) == 64
    # the i axis of pair 1: columns of the table
    assert np.array_equal(m.marginal(1, 0).units[0], [4, 20, 22, 12, 6]) and np.array_equal(m.marginal(1, 1).units[0], [4, 28, 22, 8, 2])
    assert np.array_equal(m.marginal(0, 0).cdf([1.0, 2.0]), [[14 / 64.0, 42 / 64.0]])
    for bad in ((2, 0), (-1, 0), (0, 2)):
        with pytest.raises(ValueError):
            m.marginal(*bad)


def _check_hdr(m, level):
    thr, mask = m.hdr(level)
    assert mask.shape == (m.n_pairs, m.bins, m.bins) and mask.dtype == bool and thr.shape == (m.n_pairs,)
    for p in range(m.n_pairs):
        inner = m.units[p, 1:-1, 1:-1]
        held = int(inner[mask[p]].sum())
        assert held >= level * m.W_units, (p, level, held)
        lowest = int(inner[mask[p]].min())
        assert held - lowest < level * m.W_units, 'dropping the lowest-density cell must fall below the level'
        assert thr[p] == lowest / (m.W_units * m.cell_area[p])
        assert int(inner[~mask[p]].max(initial=0)) <= lowest, 'a cell left out is denser than one taken'
    return mask


def test_hdr_minimal_monotone_deterministic():
    m, counts, units = _jm()
    levels = [0.05, 0.25, 0.3, 0.5, 0.625, 0.75, 0.8125]
    masks = [_check_hdr(m, lv) for lv in levels]
    for a, b in zip(masks[:-1], masks[1:]):
        assert np.all(b[a]), 'the region of a higher level contains the region of a lower one'
    # ties: pair 1 holds five inner cells of 8 units, at flattened inner indices 0, 1, 2, 3, 4; they are taken in that order
    for n_cells, level in ((1, 0.125), (2, 0.25), (3, 0.375), (4, 0.5), (5, 0.625)):
        thr, mask = m.hdr(level)
        assert np.array_equal(np.flatnonzero(mask[1]), np.arange(n_cells)), (level, np.flatnonzero(mask[1]))
        assert thr[1] == 8 / 64.0
    thr, mask = m.hdr(0.6875)                                   # then the 4s, again by index: inner indices 5, 6, 7
    assert np.array_equal(np.flatnonzero(mask[1]), np.arange(6))
    again = m.hdr(0.6875)
    assert np.array_equal(again[1], mask) and np.array_equal(again[0], thr)
    # pair 0: 16 + 16 = 32 units = exactly one half: two cells, the first of the two 16s first
    thr, mask = m.hdr(0.25)
    assert np.array_equal(np.flatnonzero(mask[0]), [4]) and thr[0] == 16 / 64.0
    thr, mask = m.hdr(0.5)
    assert np.array_equal(np.flatnonzero(mask[0]), [4, 8])


def test_hdr_refuses_a_level_the_inner_cells_do_not_hold():
    from mjhmc_amd.samplers.markov_jump_hmc import JointMarginals
    m, counts, units = _jm()
    assert m.out_of_range[1] == 0.1875
    m.hdr(0.8125)                                              # exactly 1 - out_of_range: every inner cell that holds weight
    with pytest.raises(ValueError, match='pair 1'):
        m.hdr(0.82)
    with pytest.raises(ValueError, match='pair 1'):
        m.hdr(1.0)
    inside = JointMarginals([(0, 1)], m.lo[:1], m.hi[:1], 3, 0.5, counts[:1], units[:1], 64, 40)
    thr, mask = inside.hdr(1.0)
    assert mask.all() and thr[0] == 2 / 64.0
    for level in (0.0, -0.1, 1.5, float('nan')):
        with pytest.raises(ValueError):
            m.hdr(level)
    empty = JointMarginals([(0, 1)], m.lo[:1], m.hi[:1], 3, 0.5, 0 * counts[:1], 0 * units[:1], 0, 0)
    with pytest.raises(ValueError):
        empty.hdr(0.5)


def test_joint_marginals_argument_checks_come_before_any_device_work():
    from mjhmc_amd.samplers.markov_jump_hmc import HMCBase, Functionals
    s = HMCBase.__new__(HMCBase)
    s._dev, s.ndims = None, 4
    ok = [(0, 1)]
    for kwargs in (dict(n_iter=0, pairs=ok), dict(n_iter=3, pairs=ok, bins=0), dict(n_iter=3, pairs=ok, bins=129),
                   dict(n_iter=3, pairs=[]), dict(n_iter=3, pairs=[(0, 1)] * 65), dict(n_iter=3, pairs=[(0, 4)]),
                   dict(n_iter=3, pairs=[(-1, 0)]), dict(n_iter=3, pairs=[0, 1]), dict(n_iter=3, pairs=[(0, 1, 2)]),
                   dict(n_iter=3, pairs=[(0.5, 1.0)]), dict(n_iter=3, pairs=ok, range=(0.0,)),
                   dict(n_iter=3, pairs=ok, range=(np.zeros(3), 1.0)), dict(n_iter=3, pairs=ok, range=(1.0, 1.0)),
                   dict(n_iter=3, pairs=ok, range=(0.0, np.inf)),
                   dict(n_iter=3, pairs=ok, range=(np.zeros(4), np.array([1.0, 1.0, 0.0, 1.0]))), dict(n_iter=3, pairs=ok, span=0.0)):
        with pytest.raises(ValueError):
            s.joint_marginals(**kwargs)
    F = Functionals(['S[0]', 'S[1]'], stats=['x', 'x * x'])
    for kwargs in (dict(pairs=[(0, 2)]), dict(pairs=ok, range=(np.zeros(4), np.ones(4)))):   # K = 2 values, not ndims = 4
        with pytest.raises(ValueError):
            s.joint_marginals(3, of=F, **kwargs)


def test_every_entry_point_refuses_bad_arguments_with_a_message(lib):
    pairs = np.array([[0, 1], [1, 0]], dtype=np.int32)
    lo, hi = np.zeros((2, 2)), np.ones((2, 2))
    out = ctypes.c_void_p()
    fake = ctypes.c_void_p(1)                     # never dereferenced: the checks below come before the sampler is touched
    P = _lib.ptr
    for n_pairs in (0, -1, 65):
        assert lib.mjhmc_pairhist_create(fake, n_pairs, P(pairs), 16, P(lo), P(hi), 1.0, ctypes.byref(out)) == -1
        assert b'n_pairs must be in [1, 64]' in lib.mjhmc_last_error()
        assert lib.mjhmc_pairhist_create_on(fake, n_pairs, P(pairs), 16, P(lo), P(hi), 1.0, ctypes.byref(out)) == -1
    for bins in (0, -3, 129):
        assert lib.mjhmc_pairhist_create(fake, 2, P(pairs), bins, P(lo), P(hi), 1.0, ctypes.byref(out)) == -1
        assert b'n_bins must be in [1, 128]' in lib.mjhmc_last_error()
    for q in (0.0, -1.0, 3.0, 0.3, float('inf'), float('nan'), 2.0 ** -1060, 2.0 ** 1023):
        assert lib.mjhmc_pairhist_create(fake, 2, P(pairs), 16, P(lo), P(hi), q, ctypes.byref(out)) == -1, q
        assert b'power of two' in lib.mjhmc_last_error(), q
    good = [fake, 2, P(pairs), 16, P(lo), P(hi), 0.5, ctypes.byref(out)]
    for at in (0, 2, 4, 5, 7):
        args = list(good)
        args[at] = None
        assert lib.mjhmc_pairhist_create(*args) == -1 and b'NULL argument' in lib.mjhmc_last_error(), at
        assert lib.mjhmc_pairhist_create_on(*args) == -1 and b'NULL argument' in lib.mjhmc_last_error(), at
    assert out.value is None
    assert lib.mjhmc_pairhist_accumulate(None, 0, -1, 1) == -1 and b'pair histogram is NULL' in lib.mjhmc_last_error()
    assert lib.mjhmc_pairhist_reset(None) == -1 and b'pair histogram is NULL' in lib.mjhmc_last_error()
    W, n = ctypes.c_uint64(), ctypes.c_int64()
    assert lib.mjhmc_pairhist_read(None, None, None, ctypes.byref(W), ctypes.byref(n)) == -1
    assert b'NULL argument' in lib.mjhmc_last_error()
    assert lib.mjhmc_pairhist_destroy(None) == 0
    assert lib.mjhmc_abi_version() == 2


def test_binding_and_header_declare_the_pairhist_entry_points():
    from mjhmc_amd import engine
    from mjhmc_amd.samplers.markov_jump_hmc import HMCBase, JointMarginals  # noqa: F401
    header = open(os.path.join(ROOT, 'include', 'mjhmc_hip.h')).read()
    for name in ('create', 'create_on', 'destroy', 'accumulate', 'read', 'reset'):
        assert 'mjhmc_pairhist_' + name in _lib.PROTOTYPES
        assert re.search(r'\bint mjhmc_pairhist_%s\(' % name, header), name
    assert len(_lib.PROTOTYPES['mjhmc_pairhist_create'][1]) == len(_lib.PROTOTYPES['mjhmc_pairhist_create_on'][1]) == 8
    assert hasattr(engine, 'DevicePairHistogram') and hasattr(engine.DeviceSampler, 'pair_histogram')
    assert hasattr(engine.DeviceFunctionals, 'pair_histogram') and hasattr(HMCBase, 'joint_marginals')


def plan_constants():
    """(LDS budget in bytes, largest group of pairs) as csrc/pairhist.hpp states them"""
    hpp = open(os.path.join(CSRC, 'pairhist.hpp')).read()
    budget = int(re.search(r'kPairhistLdsBudget\s*=\s*(\d+)', hpp).group(1))
    group = int(re.search(r'kPairhistMaxGroup\s*=\s*(\d+)', hpp).group(1))
    return budget, group


def test_lds_budget_is_what_a_workgroup_gets_without_an_attribute():
    budget, group = plan_constants()
    assert budget <= 65536 and group >= 1
    per_pair = lambda B: (B + 2) ** 2 * 12                      # noqa: E731  (mass u64 + count u32 per cell)
    assert per_pair(71) <= budget < per_pair(72)                # the switch from the LDS form to the global form
    assert budget // per_pair(32) >= 2                          # several pairs per workgroup at B <= 32


def test_sources_are_wired_into_the_makefile():
    mk = open(os.path.join(CSRC, 'Makefile')).read()
    srcs = re.search(r'^SRCS\s*=\s*(.*)$', mk, flags=re.M).group(1).split()
    assert 'pairhist.hip' in srcs
    for var in ('ASAN_SRCS', 'HOOKS_SRCS'):                    # host-logic and hook lists are as they were: a regular object there
        assert 'pairhist.hip' not in re.search(r'^%s\s*=\s*(.*)$' % var, mk, flags=re.M).group(1).split(), var
    assert mk.count('pairhist.hpp') == 3                       # a dependency of all three object rules
    assert os.path.exists(os.path.join(CSRC, 'pairhist.hip')) and os.path.exists(os.path.join(CSRC, 'pairhist.hpp'))


def test_pair_histograms_use_integer_atomics_only():
    """the tables are exact because every sum is an integer: no atomicAdd on a float or double"""
    src = open(os.path.join(CSRC, 'pairhist.hip')).read()
    code = re.sub(r'//[^\n]*', '', src)
    adds = re.findall(r'atomicAdd\s*\(\s*&\s*(\w+)', code)
    assert adds, 'the binning is LDS / global integer atomics'
    for name in set(adds):
        decl = re.search(r'\b(u64|uint32_t|unsigned long long|unsigned int)\s*\*\s*(?:const\s+|__restrict__\s+)*%s\b' % name, code)
        assert decl, 'atomicAdd target %s is not declared as an unsigned integer pointer' % name
    for word in ('atomicAdd_f', 'unsafeAtomicAdd', 'atomic_add_f', '__hip_atomic_fetch_add', 'atomicExch', 'atomicCAS'):
        assert word not in code, word
    assert not re.search(r'atomicAdd\s*\(\s*\(?\s*(float|double)', code)
    assert 'pairhist_kernel' in code and not re.search(r'__global__[^;{]*\bvoid\s+(?!pairhist_)\w+\s*\(', code)
