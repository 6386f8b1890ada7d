"""CPU: the time grid's definition against its closed form, the arithmetic of Paths, the binding and the build wiring
(csrc/timegrid.hip, include/mjhmc_hip.h: mjhmc_timegrid_*, HMCBase.paths)."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'mjhmc_amd', 'csrc')


def host_grid(X, w, dt, J, T=None, j=None, G=None):
    """the definition (tests/test_gpu_timegrid.py holds the same restatement for the device comparisons)"""
    D, n, N = X.shape
    G = np.zeros((D, J, N)) if G is None else G.copy()
    T = np.zeros(N) if T is None else T.copy()
    j = np.zeros(N, dtype=np.int64) if j is None else j.copy()
    for k in range(n):
        Tn = T + w[k]
        for p in range(N):
            while j[p] < J and float(j[p]) * dt < Tn[p]:
                G[:, j[p], p] = X[:, k, p]
                j[p] += 1
        T = Tn
    return G, T, j


def test_host_grid_is_the_searchsorted_formulation_and_blocks_do_not_matter():
    """grid point t_j = j dt takes the state k with T_k <= t_j < T_{k+1}: k = searchsorted(cumsum(w), t_j, 'right').  Dyadic
    holding times put clocks exactly on grid points (and include zeros); cutting the run in two changes nothing."""
    rs = np.random.RandomState(0)
    for trial in range(200):
        D, n, N, J = 2, rs.randint(1, 9), rs.randint(1, 6), rs.randint(1, 20)
        X = rs.randn(D, n, N)
        if trial % 2:
            w, dt = rs.randint(0, 9, (n, N)) * 0.125, 0.25
        else:
            w, dt = rs.exponential(1.0, (n, N)), 0.7
        G, T, j = host_grid(X, w, dt, J)
        cum = np.cumsum(w, axis=0)
        assert np.array_equal(T, cum[-1])
        t = np.arange(J) * dt
        for p in range(N):
            k = np.searchsorted(cum[:, p], t, side='right')
            ok = k < n
            assert j[p] == ok.sum(), (trial, p)
            assert np.array_equal(G[:, :j[p], p], X[:, k[ok], p])
            assert np.all(G[:, j[p]:, p] == 0)
        c = rs.randint(0, n + 1)
        G1, T1, j1 = host_grid(X[:, :c], w[:c], dt, J)
        G2, T2, j2 = host_grid(X[:, c:], w[c:], dt, J, T1, j1, G1)
        assert np.array_equal(G2, G) and np.array_equal(T2, T) and np.array_equal(j2, j)


class StubGrid(object):
    def __init__(self, x):
        self.x, self.closed, self.calls = x, 0, []

    def read(self, slot0, n, stacked=True):
        self.calls.append(('read', slot0, n, stacked))
        return self.x[:, :, slot0:slot0 + n]

    def autocor(self, slot0, n, linear=False):
        self.calls.append(('autocor', slot0, n, linear))
        x = self.x[:, :, slot0:slot0 + n]
        if linear:
            return np.array([np.sum(x[:, :, :n - k] * x[:, :, k:]) for k in range(n)])
        return np.array([np.sum(x * np.roll(x, -k, axis=2)) for k in range(n)])

    def close(self):
        self.closed += 1


def test_paths_arithmetic_on_a_stub():
    from mjhmc_amd.samplers.markov_jump_hmc import Paths
    x = np.random.RandomState(1).randn(3, 5, 12)
    g = StubGrid(x)
    p = Paths(g, dt=0.25, n_grid=12, covered=9, mean_time=40.0, grad_evals_per_chain=130.0, n_chains=5)
    assert (p.dt, p.n_grid, p.covered, p.mean_time, p.n_chains) == (0.25, 12, 9, 40.0, 5)
    assert p.grad_evals_per_time == 130.0 / 40.0
    assert np.array_equal(p.read(), x[:, :, :9]) and np.array_equal(p.read(4), x[:, :, :4])
    for bad in (10, 12, 0, -1):
        with pytest.raises(ValueError):
            p.read(bad)
        with pytest.raises(ValueError):
            p.autocor(bad)
    assert all(c[2] <= 9 for c in g.calls)
    ac = p.autocor()
    sums = g.autocor(0, 9)
    assert ac.shape == (9,) and ac[0] == 1.0 and np.array_equal(ac, sums / sums[0])
    lin = p.autocor(6, linear=True)
    means = np.array([np.mean(x[:, :, :6 - k] * x[:, :, k:6]) for k in range(6)])
    np.testing.assert_allclose(lin, means / means[0], rtol=1e-13, atol=0)

    class TwoEqualRanks(object):
        def allreduce_f64(self, v, op='sum'):
            return 2 * np.asarray(v)
    q = Paths(g, 0.25, 12, 9, 40.0, 130.0, 10, comm=TwoEqualRanks())
    np.testing.assert_allclose(q.autocor(), ac, rtol=1e-15, atol=0)   # shards add their lag sums before the division
    p.close()
    p.close()
    assert g.closed == 1
    with pytest.raises(ValueError):
        p.read()
    assert np.isnan(Paths(None, 1.0, 1, 0, 0.0, 3.0, 1).grad_evals_per_time)


def test_paths_argument_checks_come_before_any_device_work():
    from mjhmc_amd.samplers.markov_jump_hmc import HMCBase
    s = HMCBase.__new__(HMCBase)
    s._dev, s.ndims = None, 4
    for kwargs in (dict(n_iter=0), dict(n_iter=3, n_grid=0), dict(n_iter=3, dt=0.0), dict(n_iter=3, dt=-1.0),
                   dict(n_iter=3, dt=np.inf), dict(n_iter=3, dt=np.nan)):
        with pytest.raises(ValueError):
            s.paths(**kwargs)


def test_binding_declares_every_timegrid_prototype_of_the_header():
    from mjhmc_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'mjhmc_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    declared = set(re.findall(r'\b(mjhmc_timegrid_[a-z0-9_]+)\s*\(', header))
    assert declared == {'mjhmc_timegrid_' + n for n in ('create', 'destroy', 'accumulate', 'progress', 'read_clocks', 'read',
                                                        'autocor', 'reset')}
    bound = {n for n in _lib.PROTOTYPES if n.startswith('mjhmc_timegrid_')}
    assert bound == declared, bound ^ declared
    assert 'mjhmc_test_timegrid_read_raw' in _lib.TEST_HOOK_PROTOTYPES and 'mjhmc_test_timegrid_read_raw' not in _lib.PROTOTYPES
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        for n in declared:
            assert hasattr(lib, n), n
        assert lib.mjhmc_abi_version() == 2               # additive: no existing entry point changed
        assert not hasattr(lib, 'mjhmc_test_timegrid_read_raw')   # the hook is the test build's alone


def test_sources_are_wired_into_all_three_makefile_lists():
    mk = open(os.path.join(CSRC, 'Makefile')).read()
    for var in ('SRCS', 'ASAN_SRCS', 'HOOKS_SRCS'):
        m = re.search(r'^%s\s*=\s*(.*)$' % var, mk, flags=re.M)
        assert m and 'timegrid.hip' in m.group(1).split(), var
    assert mk.count('timegrid.hpp') == 3                    # a dependency of all three object rules
    assert os.path.exists(os.path.join(CSRC, 'timegrid.hip')) and os.path.exists(os.path.join(CSRC, 'timegrid.hpp'))


def test_timegrid_has_no_floating_point_atomic():
    """grid, clocks and cursors are bit-identical from run to run because nothing is added out of order: the only atomics
    are the integer maxima of the extent kernel"""
    src = open(os.path.join(CSRC, 'timegrid.hip')).read()
    code = re.sub(r'//[^\n]*', '', src)
    for word in ('atomicAdd', 'atomicAdd_f', 'unsafeAtomicAdd', 'atomic_add_f', '__hip_atomic_fetch_add', 'atomicExch', 'atomicCAS',
                 'atomicSub', 'unsafe-fp-atomics'):
        assert word not in code, word
    targets = re.findall(r'atomic(\w+)\s*\(\s*&\s*(\w+)', code)
    assert targets and all(op == 'Max' for op, _ in targets), targets
    for _, name in set(targets):
        assert re.search(r'\bint\s*\*\s*(?:const\s+|__restrict__\s+)*%s\b' % name, code), name
    assert '__shared__ double' not in code and '__shared__ float' not in code
