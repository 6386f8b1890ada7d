"""The recorded-run driver of the nine ring statistics (HMCBase._RecordedRun) against a fake device: no GPU, no library.

A sampler made by ``HMCBase.__new__`` gets a recording stub for ``_dev`` and for ``_run`` / ``_publish`` / ``_read_dwell``;
every call lands in one log as ``(who, what, args)``.  What is pinned here is the protocol -- the block walk, the block of
a sharded sampler, who closes what when a block fails, and that a refused argument touches nothing -- not a number.
"""
import numpy as np
import pytest

METHODS = ('stein_discrepancy', 'expectations', 'cv_expectations', 'pointwise', 'influence', 'diagnostics', 'marginals',
           'joint_marginals', 'paths')
TAKES_OF = ('expectations', 'cv_expectations', 'diagnostics', 'marginals', 'joint_marginals')
SHARDED = ('expectations', 'diagnostics', 'marginals', 'joint_marginals', 'paths')
D, N, EXPERTS = 4, 6, 5                                    # ndims, particles, experts of the fake linear model


def _plain(v):
    """arguments as they compare and print: arrays as nested tuples"""
    if isinstance(v, np.ndarray):
        return ('array',) + tuple(_plain(x) for x in v.tolist())
    if isinstance(v, (list, tuple)):
        return tuple(_plain(x) for x in v)
    if isinstance(v, (np.floating, np.integer, np.bool_)):
        return v.item()
    return v


class World(object):
    """the log, the handles in the order they were created, and when to fail"""

    def __init__(self, budget=3, fail=False):
        self.log, self.handles, self.blocks, self.budget, self.fail, self.error = [], [], 0, budget, fail, None

    def add(self, who, what, *args):
        self.log.append((who, what, _plain(args)))

    def calls(self, what, who=None):
        return [e for e in self.log if e[1] == what and (who is None or e[0] == who)]

    def maybe_fail(self):
        if self.fail and self.blocks == 2:
            self.error = RuntimeError('boom in block 2')
            self.add('world', 'fail')
            raise self.error


class Source(object):
    """the factories a DeviceSampler and a DeviceFunctionals share: accumulators over K dimensions"""

    def _make(self, kind, *args, **kw):
        h = Handle(self.world, kind, kw.pop('K', self.K), **kw)
        self.world.add(self.name, kind, *args)
        return h

    def estimator(self, want_cov=False):
        return self._make('estimator', want_cov, want_cov=want_cov)

    def chain_stats(self, n_parts=1):
        return self._make('chain_stats', n_parts)

    def histogram(self, bins, lo, hi, quantum=1.0):
        return self._make('histogram', bins, lo, hi, quantum, bins=bins)

    def pair_histogram(self, pairs, bins, lo, hi, quantum=1.0):
        return self._make('pair_histogram', pairs, bins, lo, hi, quantum, bins=bins, pairs=len(pairs))

    def cross_moments(self):
        return self._make('cross_moments')


class Handle(Source):
    def __init__(self, world, kind, K, want_cov=False, bins=0, pairs=0, M=1):
        self.world, self.kind, self.K, self.want_cov, self.bins, self.pairs, self.M = world, kind, K, want_cov, bins, pairs, M
        self.name = '%s#%d' % (kind, len(world.handles))
        self.n_values, self.ring_slots = K, 0
        world.handles.append(self)

    def ring_alloc(self, n_slots):
        self.world.add(self.name, 'ring_alloc', n_slots)
        self.ring_slots = max(self.ring_slots, n_slots)

    def evaluate(self, a, b=-1, c=None):
        self.world.add(self.name, 'evaluate', a, b, c)
        if self.kind == 'stein':                           # (it has no accumulate: its evaluate is what a block can fail in)
            self.world.maybe_fail()
            return (2.0, 1.0, 0.5, 0.1)

    def accumulate(self, x_slot0, n, w_slot0=-1, part=0):
        self.world.add(self.name, 'accumulate', x_slot0, n, w_slot0, part)
        self.world.maybe_fail()

    def set_shift(self, *c):
        self.world.add(self.name, 'set_shift', *c)

    def reset(self):
        self.world.add(self.name, 'reset')

    def close(self):
        self.world.add(self.name, 'close')

    def progress(self):
        self.world.add(self.name, 'progress')
        return 3, 3

    def read_clocks(self):
        self.world.add(self.name, 'read_clocks')
        return np.ones(N), np.zeros(N, dtype=np.int32)

    def read_cross(self):
        self.world.add(self.name, 'read_cross')
        return np.zeros((D, self.K))

    def read(self, part=0):
        self.world.add(self.name, 'read', part)
        K, v = self.K, np.arange(self.K) + 1.0
        if self.kind == 'estimator':
            return 8.0, v, v * v + 8.0, (8.0 * np.eye(K) if self.want_cov else None), 4
        if self.kind == 'cross_moments':
            return 8.0, np.zeros(D), 8.0 * np.ones(D), v, v * v + 8.0, 8.0 * np.eye(D), np.zeros((D, K)), 4
        if self.kind == 'pointwise':
            t = np.ones((self.M, K))
            return 8.0, t, 2.0 * t, t, t, 4
        if self.kind == 'influence':
            return 8.0, np.ones(D), 9.0 * np.ones(D), v, v * v + 8.0, 4
        if self.kind == 'chain_stats':
            return N, 3, 8.0, N * np.ones(K), 2.0 * N * np.ones(K), N * np.ones(K)
        shape = (K, self.bins + 2) if self.kind == 'histogram' else (self.pairs, self.bins + 2, self.bins + 2)
        return np.ones(shape, dtype=np.uint64), np.ones(shape, dtype=np.uint64), 5, 4


class Dev(Source):
    name, K, ndims, nparticles = 'dev', D, D, N

    def __init__(self, world):
        self.world, self.ring_slots = world, 0

    def ring_alloc(self, n_slots):
        self.world.add('dev', 'ring_alloc', n_slots)
        self.ring_slots = max(self.ring_slots, n_slots)

    def ring_slot_bytes(self):
        self.world.add('dev', 'ring_slot_bytes')
        return 4096

    def ring_budget_slots(self, n_wanted, share=0.6, staging=True, extra_bytes=0, reserve_bytes=0):
        self.world.add('dev', 'ring_budget_slots', n_wanted, share, staging, extra_bytes, reserve_bytes)
        return min(n_wanted, self.world.budget)

    def ring_copy(self, src_slot, dst_slot):
        self.world.add('dev', 'ring_copy', src_slot, dst_slot)

    def functionals(self, values, stats=(), params=()):
        return self._make('functionals', values, stats, params, K=len(values))

    def energy_observables(self):
        return self._make('functionals', 'energy', K=3)

    def projections(self, A, b=None, link=None, params=()):
        return self._make('functionals', A, b, link, params, K=len(A))

    def time_grid(self, n_grid, dt):
        return self._make('time_grid', n_grid, dt)

    def stein(self, c):
        return self._make('stein', c)

    def pointwise(self, values, log_mean_exp=None):
        return self._make('pointwise', values, log_mean_exp, K=EXPERTS, M=len(values))

    def influence(self, value, experts=None):
        return self._make('influence', value, experts, K=experts[1] - experts[0])


class Comm(object):
    """a communicator of one rank whose 'min' never exceeds ``cap``: the other rank's block"""

    def __init__(self, world, cap=2):
        self.world, self.cap = world, cap

    def allreduce_ints(self, vals, op):
        self.world.add('comm', 'allreduce_ints', vals, op)
        return [min(int(v), self.cap) for v in vals] if op == 'min' else list(vals)

    def allreduce_f64(self, x, op='sum'):
        self.world.add('comm', 'allreduce_f64', x, op)
        return x

    def bcast(self, x, root=0):
        self.world.add('comm', 'bcast', x, root)
        return x


class LinearModel(object):
    """as much of a distribution as the nine methods ask for before they reach the device"""
    dEdX_count, n_data = 0, EXPERTS

    def device_energy(self):
        from mjhmc_amd import _lib
        return _lib.E_LINEAR_EXPR, {'W': np.zeros((EXPERTS, D))}


def make(lead, comm=False, budget=3, fail=False):
    from mjhmc_amd.samplers.markov_jump_hmc import HMCBase
    world = World(budget, fail)
    s = HMCBase.__new__(HMCBase)
    s._dev, s.ndims, s.nbatch, s.distribution = Dev(world), D, N, LinearModel()
    s._comm = Comm(world) if comm else None
    s._dwell_weighted = bool(lead)

    def _run(n_iter, ring_slot0=-1, replay=None, download=None, keep_trace=False):
        world.blocks += 1
        world.add('sampler', '_run', n_iter, ring_slot0, keep_trace)
    s._run = _run
    s._publish = lambda: world.add('sampler', '_publish')
    s._read_dwell = lambda: world.add('sampler', '_read_dwell')
    return s, world


def call(s, method, n_iter=4, **kw):
    """``method`` with the arguments it cannot do without"""
    if method == 'pointwise':
        kw.setdefault('values', ['u'])
    elif method == 'influence':
        kw.setdefault('value', 'u')
    elif method == 'joint_marginals':
        kw.setdefault('pairs', [(0, 1), (1, 0)])
    return getattr(s, method)(n_iter, **kw)


def functionals():
    from mjhmc_amd.samplers.markov_jump_hmc import Functionals
    return Functionals(['S[0]', 'S[0] * S[0]'], stats=['x'])


@pytest.fixture(autouse=True)
def no_compile_check(monkeypatch):
    """pointwise() and influence() compile their expressions before anything runs: that is the library's work"""
    from mjhmc_amd import engine
    monkeypatch.setattr(engine, 'pointwise_check', lambda *a: None)
    monkeypatch.setattr(engine, 'influence_check', lambda *a: None)


def _walk(world):
    """[(ring_copy args or None, _run args)] of every block"""
    out, copy = [], None
    for who, what, args in world.log:
        if what == 'ring_copy':
            copy = args
        elif what == '_run':
            out.append((copy, args))
            copy = None
    return out


def _blocks_of(n_iter, block):
    ks = [block] * (n_iter // block) + ([n_iter % block] if n_iter % block else [])
    return ks


# ---------------------------------------------------------------------------------------------------------------------
# 1.  the walk
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lead', [0, 1])
@pytest.mark.parametrize('n_iter,block', [(7, 3), (6, 3), (1, 5)])
@pytest.mark.parametrize('method', ['expectations', 'pointwise', 'paths'])
def test_the_walk(method, n_iter, block, lead):
    s, world = make(lead)
    call(s, method, n_iter, block=block)
    block = min(block, n_iter)
    ks = _blocks_of(n_iter, block)
    assert world.calls('ring_alloc', 'dev')[-1][2] == (block + lead,)
    assert not world.calls('ring_budget_slots')            # the caller's block needs no budget
    walk = _walk(world)
    assert len(walk) == len(ks)
    for i, (k, (copy, run)) in enumerate(zip(ks, walk)):
        if not lead:
            assert copy is None and run == (k, 0, i > 0)
        elif i == 0:
            assert copy is None and run == (k + 1, 0, False)
        else:
            assert copy == (ks[i - 1], 0) and run == (k, 1, True)
    assert [e[1] for e in world.log if e[0] == 'sampler' and e[1] != '_run'] == ['_publish'] + ['_read_dwell'] * lead
    assert world.log.index(('sampler', '_publish', ())) > max(i for i, e in enumerate(world.log) if e[1] == 'accumulate')


@pytest.mark.parametrize('lead', [0, 1])
def test_a_block_from_the_budget_is_clamped_to_the_run(lead):
    s, world = make(lead, budget=3)
    call(s, 'expectations', 7)
    assert world.calls('ring_budget_slots')[0][2] == (7 + lead, 0.6, False, 0, 0)
    assert world.calls('ring_alloc', 'dev') == [('dev', 'ring_alloc', (3,))]         # 3 slots: the lead slot is one of them
    assert [run[0] for _, run in _walk(world)] == ([3, 2, 2, 1] if lead else [3, 3, 1])
    s, world = make(lead, budget=1)                         # never less than one state per block
    call(s, 'expectations', 2)
    assert world.calls('ring_alloc', 'dev')[-1][2] == (1 + lead,)


@pytest.mark.parametrize('lead', [0, 1])
def test_split_diagnostics_never_straddle_the_half_boundary(lead):
    s, world = make(lead)
    call(s, 'diagnostics', 10, split=True, block=4)
    acc = [e[2] for e in world.log if e[0].startswith('chain_stats') and e[1] == 'accumulate']
    assert [(a[1], a[3]) for a in acc] == [(4, 0), (1, 0), (4, 1), (1, 1)]           # (k, part)
    assert [run[0] for _, run in _walk(world)] == ([5, 1, 4, 1] if lead else [4, 1, 4, 1])
    s, world = make(lead)
    call(s, 'diagnostics', 10, split=False, block=4)
    assert [e[2][1] for e in world.log if e[0].startswith('chain_stats') and e[1] == 'accumulate'] == [4, 4, 2]


@pytest.mark.parametrize('lead', [0, 1])
@pytest.mark.parametrize('method', ['diagnostics', 'paths'])
def test_two_stage_start(method, lead):
    """what exists before the budget is taken is counted by it; chain sums made on a ring that then grows are made again"""
    s, world = make(lead, budget=3)
    kw = dict(dt=0.5) if method == 'paths' else dict(of=functionals())
    call(s, method, 8, **kw)
    names = [(e[0], e[1]) for e in world.log[:world.log.index(world.calls('_run')[0])]]
    if method == 'paths':                                  # the grid has storage of its own: it stays
        assert names == [('dev', 'ring_alloc'), ('dev', 'time_grid'), ('dev', 'ring_budget_slots'), ('dev', 'ring_alloc')]
        assert world.calls('ring_budget_slots')[0][2][-1] == 0
    else:
        assert names == [('dev', 'ring_alloc'), ('dev', 'functionals'), ('functionals#0', 'ring_alloc'),
                         ('functionals#0', 'chain_stats'), ('dev', 'ring_budget_slots'), ('chain_stats#1', 'close'),
                         ('functionals#0', 'close'), ('dev', 'ring_alloc'), ('dev', 'functionals'),
                         ('functionals#2', 'ring_alloc'), ('functionals#2', 'chain_stats')]
    assert [e[2] for e in world.calls('ring_alloc', 'dev')] == [(1 + lead,), (3,)]
    if method == 'diagnostics':                            # a ring that is large enough already is left alone
        s, world = make(lead)
        call(s, method, 8, block=1)
        assert [e[2] for e in world.calls('ring_alloc', 'dev')] == [(1 + lead,)]
        assert not [e for e in world.log[:world.log.index(world.calls('_run')[0])] if e[1] == 'close']
    else:                                                  # a grid that waits for its dt is spoken for
        s, world = make(lead, budget=3)
        call(s, method, 8, dt=None)
        if lead:
            assert world.calls('ring_budget_slots')[0][2][-1] == 8 * 4096


# ---------------------------------------------------------------------------------------------------------------------
# 2.  the block of a sharded sampler
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lead', [0, 1])
@pytest.mark.parametrize('block', [None, 5, 1])
@pytest.mark.parametrize('method', SHARDED)
def test_a_sharded_sampler_walks_the_smallest_block_of_all_ranks(method, block, lead):
    s, world = make(lead, comm=True, budget=4)
    call(s, method, 6, block=block, **(dict(split=False) if method == 'diagnostics' else {}))
    own = block or 4 - lead                                # this rank's: the budget's 4 slots hold the lead slot too
    want = min(2, own)                                     # the comm stub's other rank has room for 2
    mine = [e for e in world.calls('allreduce_ints') if e[2][1] == 'min'][0]
    assert mine[2] == ((own,), 'min')                      # this rank's own block goes in, clamped to the run
    assert world.calls('ring_alloc', 'dev')[-1][2] == (want + lead,)
    ks = [run[0] for _, run in _walk(world)]
    assert ks == [k + (lead if i == 0 else 0) for i, k in enumerate(_blocks_of(6, want))]


# ---------------------------------------------------------------------------------------------------------------------
# 3.  a block that fails
# ---------------------------------------------------------------------------------------------------------------------
def _cases():
    for method in METHODS:
        for of in ((None, 'functionals') if method in TAKES_OF else (None,)):
            yield method, of


@pytest.mark.parametrize('lead', [0, 1])
@pytest.mark.parametrize('method,of', list(_cases()))
def test_a_failing_block_closes_every_handle_once_latest_first(method, of, lead):
    s, world = make(lead, fail=True)
    kw = dict(of=functionals()) if of else {}
    with pytest.raises(RuntimeError) as info:
        call(s, method, 4, block=2, **kw)
    assert info.value is world.error                        # unchanged, not wrapped
    assert world.blocks == 2 and not world.calls('_publish') and not world.calls('_read_dwell')
    closes = [e[0] for e in world.calls('close')]
    assert sorted(closes) == sorted(h.name for h in world.handles)                    # every handle, exactly once
    at = world.log.index(('world', 'fail', ()))
    before = [e[0] for e in world.log[:at] if e[1] == 'close']
    after = [e[0] for e in world.log[at:] if e[1] == 'close']
    open_at_failure = [h.name for h in world.handles if h.name not in before]
    assert after == open_at_failure[::-1]                   # latest first
    if of:
        assert after[-1].startswith('functionals')         # the of handle last: the others sit on its ring
    assert len(after) == (2 if of else 1)                   # (the first block's throw-away handles went in the first block)


@pytest.mark.parametrize('lead', [0, 1])
@pytest.mark.parametrize('method,of', list(_cases()))
def test_a_run_that_succeeds_closes_every_handle_once_but_the_grid(method, of, lead):
    s, world = make(lead)
    result = call(s, method, 4, block=2, **(dict(of=functionals()) if of else {}))
    closes = [e[0] for e in world.calls('close')]
    kept = [h.name for h in world.handles if h.kind == 'time_grid']
    assert sorted(closes + kept) == sorted(h.name for h in world.handles) and len(kept) == (method == 'paths')
    if of:
        assert closes[-1].startswith('functionals')
    if method == 'paths':                                  # the grid is the caller's: Paths.close() frees it
        result.close()
        assert [e[0] for e in world.calls('close')][-1] == kept[0]


@pytest.mark.parametrize('dt', [None, 0.5])
def test_paths_closes_its_grid_when_a_block_fails(dt):
    s, world = make(1, fail=True)
    with pytest.raises(RuntimeError):
        s.paths(4, dt=dt, block=2)
    grids = [h.name for h in world.handles if h.kind == 'time_grid']
    assert len(grids) == 1 and [e[0] for e in world.calls('close')].count(grids[0]) == 1


# ---------------------------------------------------------------------------------------------------------------------
# 4.  a refused argument touches nothing
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('method,kw', [
    ('stein_discrepancy', dict(every=0)),
    ('expectations', dict(n_iter=0)),
    ('cv_expectations', dict(shift=np.zeros(D + 1))),
    ('pointwise', dict(values=['u'] * 5)),
    ('influence', dict(experts=(3, 2))),
    ('diagnostics', dict(n_iter=5, split=True)),
    ('diagnostics', dict(shift=np.zeros(D + 1))),
    ('marginals', dict(range=(1.0, 0.0))),
    ('marginals', dict(bins=0)),
    ('joint_marginals', dict(pairs=[(0, D)])),
    ('joint_marginals', dict(range=(0.0, 1.0, 2.0))),
    ('paths', dict(dt=0.0)),
])
def test_a_refused_argument_raises_before_the_first_call(method, kw):
    s, world = make(1)
    with pytest.raises(ValueError):
        call(s, method, **dict(dict(n_iter=4), **kw))
    assert world.log == []


def test_the_four_that_refuse_a_sharded_sampler_refuse_it_before_the_driver():
    for method in ('stein_discrepancy', 'cv_expectations', 'pointwise', 'influence'):
        s, world = make(1, comm=True)
        with pytest.raises(ValueError, match='sharded'):
            call(s, method)
        assert world.log == []
