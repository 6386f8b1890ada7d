"""No GPU: the NumPy restatement of the occupancy contract (csrc/occupancy.hip), the ``Occupancy`` result on hand tables, and
``HMCBase.occupancy`` against the fake device of tests/test_recorded_run_cpu.py.

``host_labels`` / ``host_tables`` are written from the contract alone -- NumPy's elementwise float64 operations round once
each and never fuse -- and tests/test_gpu_occupancy.py compares the device tables with them as integers."""
import numpy as np
import pytest

from tests import test_recorded_run_cpu as rr


# ---------------------------------------------------------------------------------------------------------------------
# the NumPy restatement
# ---------------------------------------------------------------------------------------------------------------------
def host_labels(X, centres, r2=None):
    """X (K, ...) float64 states as the ring holds them, centres (M, K), r2 (M,) or None -> labels uint8 of shape
    X.shape[1:]: d2_m = 0.0, then d2_m = d2_m + (x_d - c[m][d])^2 for d ascending; the lowest m with the strictly smallest
    finite d2 (M, "outside", when there is none); with r2, M unless best <= r2[label]"""
    centres = np.asarray(centres, dtype=np.float64)
    M, K = centres.shape
    assert X.shape[0] == K
    shape = X.shape[1:]
    d2 = np.zeros((M,) + shape)
    with np.errstate(invalid='ignore', over='ignore'):
        for d in range(K):
            t = X[d][None] - centres[:, d].reshape((M,) + (1,) * len(shape))
            d2 = d2 + t * t
        best = np.full(shape, np.inf)
        label = np.full(shape, M, dtype=np.int64)
        for m in range(M):
            win = d2[m] < best
            best = np.where(win, d2[m], best)
            label = np.where(win, m, label)
        if r2 is not None:
            r = np.append(np.asarray(r2, dtype=np.float64), np.inf)
            label = np.where((label < M) & ~(best <= r[label]), M, label)
    return label.astype(np.uint8)


def host_units(w, q):
    """u = rint(w / q), nearest-even, as unsigned 64-bit integers"""
    return np.rint(w / q).astype(np.uint64)


def host_tables(labels, units, M, starts=(0,)):
    """labels (n, N), units (n, N) uint64 in slot order; ``starts``: the slots at which new chains start (no pair into
    them).  Returns the dict of DeviceOccupancy.read(chains=True)."""
    labels = np.asarray(labels, dtype=np.int64)
    units = np.asarray(units, dtype=np.uint64)
    n, N = labels.shape
    C = M + 1
    t = dict((k, np.zeros(C, dtype=np.uint64)) for k in ('count', 'mass', 'from_count', 'from_mass', 'chains_by_cells'))
    t['trans'] = np.zeros((C, C), dtype=np.uint64)
    t['chains_by_switches'] = np.zeros(17, dtype=np.uint64)
    t['switches'] = np.zeros(N, dtype=np.uint32)
    t['visited'] = np.zeros(N, dtype=np.uint64)
    for p in range(N):
        for s in range(n):
            a = int(labels[s, p])
            t['count'][a] += np.uint64(1)
            t['mass'][a] += units[s, p]
            if a < M:
                t['visited'][p] |= np.uint64(1) << np.uint64(a)
            if s + 1 < n and (s + 1) not in starts:
                b = int(labels[s + 1, p])
                t['from_count'][a] += np.uint64(1)
                t['from_mass'][a] += units[s, p]
                t['trans'][a, b] += np.uint64(1)
                t['switches'][p] += np.uint32(a != b)
        t['chains_by_switches'][min(int(t['switches'][p]), 16)] += np.uint64(1)
        t['chains_by_cells'][bin(int(t['visited'][p])).count('1')] += np.uint64(1)
    t['W_units'] = int(units.sum(dtype=np.uint64))
    t['n_states'] = n * N
    return t


# ---------------------------------------------------------------------------------------------------------------------
# 1.  the oracle on an example small enough to verify by eye
# ---------------------------------------------------------------------------------------------------------------------
def _hand():
    """3 chains x 4 states in the plane, centres (0, 0) and (2, 0), radius 1.5 for both.
    chain 0: (0, 0) -> 0;  (1, 0): d2 = 1 to both, a tie -> 0;  (2, 0.5) -> 1;  (2, 0) -> 1
    chain 1: (NaN, 0) -> outside;  (2, 0) -> 1;  (5, 0): nearest is centre 1 at d2 = 9 > 2.25, a radius miss -> outside;  (0, 0) -> 0
    chain 2: (0, 0) four times: it never leaves"""
    chains = [[(0, 0), (1, 0), (2, 0.5), (2, 0)],
              [(np.nan, 0), (2, 0), (5, 0), (0, 0)],
              [(0, 0), (0, 0), (0, 0), (0, 0)]]
    X = np.array(chains, dtype=np.float64).transpose(2, 1, 0)         # (K, n, N)
    w = np.array([[1, 2, 1], [3, 1, 1], [1, 1, 1], [2, 4, 1]], dtype=np.float64)
    return X, w, np.array([[0.0, 0.0], [2.0, 0.0]]), np.array([2.25, 2.25])


def test_the_oracle_on_a_hand_example():
    X, w, centres, r2 = _hand()
    labels = host_labels(X, centres, r2)
    assert labels.tolist() == [[0, 2, 0], [0, 1, 0], [1, 2, 0], [1, 0, 0]]
    # without the radius the far state belongs to centre 1; the NaN row stays outside
    assert host_labels(X, centres).tolist() == [[0, 2, 0], [0, 1, 0], [1, 1, 0], [1, 0, 0]]
    t = host_tables(labels, host_units(w, 1.0), 2)
    assert t['count'].tolist() == [7, 3, 2] and t['mass'].tolist() == [12, 4, 3] and t['W_units'] == 19
    assert t['trans'].tolist() == [[4, 1, 0], [0, 1, 1], [1, 1, 0]]
    assert t['from_count'].tolist() == [5, 2, 2] and t['from_mass'].tolist() == [7, 2, 3]
    assert t['trans'].sum(axis=1).tolist() == t['from_count'].tolist()
    assert t['switches'].tolist() == [1, 3, 0] and t['visited'].tolist() == [3, 3, 1]
    assert t['chains_by_switches'].tolist() == [1, 1, 0, 1] + [0] * 13
    assert t['chains_by_cells'].tolist() == [0, 1, 2]
    # a cut before slot 2 loses exactly one pair per chain: (0 -> 1), (1 -> outside), (0 -> 0)
    c = host_tables(labels, host_units(w, 1.0), 2, starts=(0, 2))
    assert int(c['trans'].sum()) == 6 and (t['trans'] - c['trans']).tolist() == [[1, 1, 0], [0, 0, 1], [0, 0, 0]]
    assert c['count'].tolist() == t['count'].tolist() and c['switches'].tolist() == [0, 2, 0]
    # units: nearest-even in quanta
    assert host_units(np.array([0.5, 1.5, 2.5, 0.26]), 1.0).tolist() == [0, 2, 2, 0]
    assert host_units(np.array([0.5, 0.75]), 0.5).tolist() == [1, 2]


def test_ties_and_two_identical_centres():
    X = np.array([[1.0, -1.0, 0.0, 3.0]])                              # K = 1
    centres = np.array([[2.0], [0.0], [2.0], [0.0]])
    # 1: d2 = 1 to all four -> 0;  -1: centres 1 and 3 at 1 -> 1;  0 -> 1;  3 -> 0: the copies 2 and 3 never win
    assert host_labels(X, centres).tolist() == [0, 1, 1, 0]
    assert host_labels(np.array([[np.inf, -np.inf, 1e200]]), centres).tolist() == [4, 4, 4]     # inf distances: outside


# ---------------------------------------------------------------------------------------------------------------------
# 2.  Occupancy on hand tables
# ---------------------------------------------------------------------------------------------------------------------
def _tables(trans, from_mass=None, count=None, mass=None, by_switches=(0,), by_cells=None):
    trans = np.asarray(trans, dtype=np.uint64)
    C = trans.shape[0]
    from_count = trans.sum(axis=1).astype(np.uint64)
    from_mass = from_count if from_mass is None else np.asarray(from_mass, dtype=np.uint64)
    count = from_count if count is None else np.asarray(count, dtype=np.uint64)
    mass = from_mass if mass is None else np.asarray(mass, dtype=np.uint64)
    sw = np.zeros(17, dtype=np.uint64)
    sw[:len(by_switches)] = by_switches
    return dict(count=count, mass=mass, from_count=from_count, from_mass=from_mass, trans=trans, W_units=int(mass.sum()),
                chains_by_switches=sw, chains_by_cells=np.zeros(C, dtype=np.uint64) if by_cells is None else by_cells,
                n_states=int(count.sum()))


def _occupancy(tables, q=1.0, grad_evals=0):
    from mjhmc_amd.samplers.markov_jump_hmc import Occupancy
    M = tables['trans'].shape[0] - 1
    return Occupancy(tables, q, np.zeros((M, 2)), tables['n_states'], grad_evals)


def test_two_cells_discrete_time():
    a, b = 0.1, 0.2                                                  # exit probabilities of cells 0 and 1
    o = _occupancy(_tables([[900, 100], [100, 400]], by_switches=(3, 1)), grad_evals=3000)
    assert np.allclose(o.transition_matrix(), [[1 - a, a], [b, 1 - b]], rtol=1e-15, atol=0)
    assert np.allclose(o.rate_matrix(), o.transition_matrix() - np.eye(2), rtol=0, atol=1e-16)     # P - I
    assert np.allclose(o.stationary(), np.array([b, a]) / (a + b), rtol=1e-12, atol=0)
    assert abs(o.spectral_gap() - (1 - abs(1 - a - b))) < 1e-12
    assert abs(o.relaxation_time() - 1 / (a + b)) < 1e-12 / (a + b)
    assert abs(o.relaxation_grads() - (1 / (a + b)) * 3000 / 1500.0) < 1e-9
    assert np.allclose(o.weight, [1000 / 1500.0, 500 / 1500.0], rtol=1e-15)
    assert np.allclose(o.mean_residence, [1 / a, 1 / b], rtol=1e-12)
    assert o.crossings == 200 and o.crossings_per_grad == 200 / 3000.0
    assert o.never_left == 0.75 and o.n_chains == 4


def test_two_cells_process_time():
    q = 0.5                                                          # 1000 and 125 time units before 100 exits each
    o = _occupancy(_tables([[900, 100], [100, 400]], from_mass=[2000, 250]), q=q)
    ra, rb = 100 / 1000.0, 100 / 125.0
    assert np.allclose(o.rate_matrix(), [[-ra, ra], [rb, -rb]], rtol=1e-15)
    assert np.allclose(o.stationary(), np.array([rb, ra]) / (ra + rb), rtol=1e-12)
    assert abs(o.relaxation_time() - 1 / (ra + rb)) < 1e-12                     # the 2 x 2 generator's eigenvalues: 0, -(ra + rb)
    assert np.allclose(o.mean_residence, [1 / ra, 1 / rb], rtol=1e-12)
    assert abs(o.spectral_gap() - 0.3) < 1e-12                                  # (of the jump chain, whatever the holding times)
    assert np.isnan(o.relaxation_grads())                                       # no gradient count was given


def test_a_cell_never_visited_and_the_identity_row():
    # three cells, the middle one never seen; cell 2 seen once, as a chain's last state: no departure, the identity row
    t = _tables([[8, 0, 2], [0, 0, 0], [0, 0, 0]], count=[10, 0, 3], mass=[10, 0, 3])
    o = _occupancy(t)
    P = o.transition_matrix()
    assert P[1].tolist() == [0, 1, 0] and P[2].tolist() == [0, 0, 1] and np.allclose(P[0], [0.8, 0, 0.2])
    assert o.rate_matrix()[1].tolist() == [0, 0, 0] and o.rate_matrix()[2].tolist() == [0, 0, 0]
    pi = o.stationary()
    assert pi[1] == 0 and abs(pi.sum() - 1) < 1e-12 and abs(pi[2] - 1) < 1e-12   # everything ends in the cell nothing leaves
    assert o.visited.tolist() == [True, False, True]
    # on the visited cells P = [[0.8, 0.2], [0, 1]] and Q = [[-0.2, 0.2], [0, 0]]: eigenvalues 1, 0.8 and 0, -0.2
    assert abs(o.spectral_gap() - 0.2) < 1e-12 and abs(o.relaxation_time() - 5.0) < 1e-9
    assert o.mean_residence[0] == 5.0 and o.mean_residence[2] == np.inf
    one = _occupancy(_tables([[5, 0], [0, 0]]))
    assert np.isnan(one.spectral_gap()) and np.isnan(one.relaxation_time()) and one.stationary().tolist() == [1, 0]
    assert one.crossings == 0


# ---------------------------------------------------------------------------------------------------------------------
# 3.  the driver against the fake device
# ---------------------------------------------------------------------------------------------------------------------
class OccHandle(rr.Handle):
    def accumulate(self, x_slot0, n, w_slot0=-1, linked=False):
        self.world.add(self.name, 'accumulate', x_slot0, n, w_slot0, linked)
        self.world.maybe_fail()

    def read(self, chains=False):
        self.world.add(self.name, 'read')
        return _tables(np.ones((self.M + 1, self.M + 1)))


@pytest.fixture(autouse=True)
def fake_occupancy(monkeypatch):
    def occupancy(self, centres, r2=None, q=1.0):
        h = OccHandle(self.world, 'occupancy', self.K, M=len(centres))
        self.world.add(self.name, 'occupancy', centres, r2, q)
        return h
    monkeypatch.setattr(rr.Source, 'occupancy', occupancy, raising=False)


CENTRES = np.array([[0.0] * rr.D, [1.0] * rr.D])


@pytest.mark.parametrize('lead', [0, 1])
@pytest.mark.parametrize('n_iter,block', [(7, 3), (6, 3), (2, 5), (5, 1)])
def test_the_block_walk_links_every_block_but_the_first(n_iter, block, lead):
    s, world = rr.make(lead)
    o = s.occupancy(n_iter, CENTRES, block=block)
    ks = rr._blocks_of(n_iter, min(block, n_iter))
    w0 = 1 if lead else -1
    assert [e[2] for e in world.calls('accumulate') if e[0].startswith('occupancy')] == \
        [(0, k, w0, i > 0) for i, k in enumerate(ks)]
    created = world.calls('occupancy')
    assert len(created) == 1 and created[0][0] == 'dev'
    centres, r2, q = created[0][2]
    assert centres == rr._plain(CENTRES) and r2 is None
    if lead:                                               # the quantum of marginals(): the fake first block has W / n = 8 / 4
        assert q == 2.0 ** (1 - 24) and len(world.calls('estimator')) == 1
    else:
        assert q == 1.0 and not world.calls('estimator')
    assert [h.kind for h in world.handles if h.kind == 'occupancy'] == ['occupancy']
    for h in world.handles:
        assert len(world.calls('close', h.name)) == 1, h.name
    assert len(world.calls('_publish')) == 1 and len(world.calls('_read_dwell')) == lead
    assert o.n_cells == 3 and o.quantum == q


def test_the_radius_reaches_the_device_squared():
    s, world = rr.make(0)
    s.occupancy(4, CENTRES, radius=[0.5, 3.0])
    assert world.calls('occupancy')[0][2][1] == ('array', 0.25, 9.0)
    s, world = rr.make(0)
    s.occupancy(4, CENTRES, radius=2.0)
    assert world.calls('occupancy')[0][2][1] == ('array', 4.0, 4.0)


def test_of_puts_the_cells_into_the_value_space():
    s, world = rr.make(1)
    of = rr.functionals()                                  # two values
    s.occupancy(5, np.zeros((3, 2)), of=of, block=2)
    created = world.calls('occupancy')
    assert len(created) == 1 and created[0][0].startswith('functionals')
    assert len(world.calls('evaluate')) == 3
    for h in world.handles:
        assert len(world.calls('close', h.name)) == 1, h.name
    with pytest.raises(ValueError, match='n_values = 2'):
        rr.make(1)[0].occupancy(5, np.zeros((3, rr.D)), of=of)


@pytest.mark.parametrize('lead', [0, 1])
def test_a_failing_block_closes_every_handle_once(lead):
    s, world = rr.make(lead, fail=True)
    with pytest.raises(RuntimeError, match='boom'):
        s.occupancy(7, CENTRES, block=2)
    assert world.handles
    for h in world.handles:
        assert len(world.calls('close', h.name)) == 1, h.name
    assert not world.calls('_publish') and not world.calls('read', 'occupancy#%d' % (len(world.handles) - 1))


BAD = [
    (dict(n_iter=1), 'n_iter'),
    (dict(n_iter=0), 'n_iter'),
    (dict(centres=np.zeros(rr.D)), 'centres'),
    (dict(centres=np.zeros((2, rr.D + 1))), 'centres'),
    (dict(centres=np.zeros((0, rr.D))), 'centres'),
    (dict(centres=np.zeros((65, rr.D))), 'centres'),
    (dict(centres=np.full((2, rr.D), np.nan)), 'finite'),
    (dict(centres=np.full((2, rr.D), np.inf)), 'finite'),
    (dict(radius=-1.0), 'radius'),
    (dict(radius=[1.0, np.nan]), 'radius'),
    (dict(radius=[1.0, 2.0, 3.0]), 'radius'),
]


@pytest.mark.parametrize('kw,word', BAD)
def test_a_bad_argument_raises_before_the_first_device_call(kw, word):
    s, world = rr.make(1)
    args = dict(n_iter=4, centres=CENTRES)
    args.update(kw)
    with pytest.raises(ValueError, match=word):
        s.occupancy(**args)
    assert world.log == []


def test_a_sharded_sampler_is_refused_before_the_driver():
    s, world = rr.make(1, comm=True)
    with pytest.raises(ValueError, match='occupancy: a sharded sampler'):
        s.occupancy(4, CENTRES)
    assert world.log == []


def test_modes_of_the_multimodal_gaussian():
    from mjhmc_amd.misc.distributions import MultimodalGaussian
    d = MultimodalGaussian(ndims=3, nbatch=4, separation=3)
    assert d.modes().tolist() == [[-6.0, 0.0, 0.0], [6.0, 0.0, 0.0]]                 # csrc/energy_mm.hip: sep0 = 2 * separation
