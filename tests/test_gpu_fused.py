"""GPU: fused launches (several sampling iterations per kernel launch, state kept on chip between them) are
an implementation detail: mjhmc_iterate(n) must equal n single-iteration calls bit for bit -- state, energies,
dwelling times, transitions, the per-iteration counters, the ring snapshots -- for every sampler mode and
lane mapping, across the 64-iteration launch boundary, and when an iteration in the middle of a launch meets a
non-finite rate (whole-batch abort, markov_jump_hmc.py:376-389)."""
import numpy as np
import pytest

from tests.helpers import bits_equal, hooks_context

pytestmark = pytest.mark.gpu
FIELDS = ('X', 'V', 'EX', 'EV', 'HFLF', 'DWELL', 'TRANS')


def _pair(kind, D, N, mode, seed=5, params=None, scale=1.0, dtype='float64', dtype2=None, libs='pp'):
    """two samplers from the same inputs; libs: per sampler 'p' = the product library, 'h' = the test build (the only
    one that reads the MJHMC_NO_* / MJHMC_DEBUG_POISON environment switches)"""
    from mjhmc_amd import engine, _lib
    rs = np.random.RandomState(D * 7 + N)
    X0 = rs.randn(D, N) * scale
    out = []
    for which, dt in zip(libs, (dtype, dtype2 or dtype)):
        ctx = engine.context(0) if which == 'p' else hooks_context(0)
        en = engine.DeviceEnergy(ctx, getattr(_lib, kind), D, params if params is not None else [1.0])
        out.append(engine.DeviceSampler(en, X0, seed=seed, mode=mode, dtype=dt))
    return out, _lib


def _same_state(a, b, _lib, fields=FIELDS):
    for f in fields:
        fa, fb = a.read(getattr(_lib, 'F_' + f)), b.read(getattr(_lib, 'F_' + f))
        assert bits_equal(fa, fb), f


def _stats_tuple(st):
    return (st.l, st.f, st.r, st.fl, st.n_cold, st.E_evals, st.dEdX_evals, st.nonfinite, st.L_used)


@pytest.mark.parametrize('kind,D,N,mode_name,n_iter', [
    ('E_ISO_GAUSS', 512, 130, 'MODE_MJHMC', 7),      # wave per particle
    ('E_ISO_GAUSS', 256, 131, 'MODE_MJHMC', 9),      # half a wave per particle, clocks drawn up front (WPP = 6); odd slot count
    ('E_DIAG_GAUSS', 256, 64, 'MODE_MJHMC', 66),     # the same across the 64-iteration launch boundary
    ('E_ISO_GAUSS', 64, 500, 'MODE_MJHMC', 70),      # crosses the 64-iteration launch boundary
    ('E_ISO_GAUSS', 40, 129, 'MODE_MJHMC', 5),       # ragged rows (predicated chunks)
    ('E_ISO_GAUSS', 2, 100, 'MODE_MJHMC', 9),
    ('E_DIAG_GAUSS', 32, 300, 'MODE_MJHMC', 6),
    ('E_FUNNEL_NEAL', 32, 300, 'MODE_MJHMC', 6),      # the funnels fuse in row form (a lane per particle, mjhmc_fused_rows_kernel):
    ('E_FUNNEL_NEAL', 31, 20011, 'MODE_MJHMC', 5),    #   full rows of four-lane groups, a ragged last tile (one tile per wave: the grid holds 65 536 particles)
    ('E_FUNNEL_NEAL', 31, 200003, 'MODE_MJHMC', 5),   #   the same with a persistent grid: every wave walks several tiles
    ('E_FUNNEL_NEAL', 21, 131, 'MODE_MJHMC', 70),     #   short rows; across the 64-iteration launch boundary
    ('E_FUNNEL_NEAL', 16, 700, 'MODE_MJHMC', 9),      #   two-lane groups, full rows
    ('E_FUNNEL_NEAL', 11, 65, 'MODE_MJHMC', 7),       #   two-lane groups, short rows
    ('E_ROUGH_WELL', 4, 48, 'MODE_MJHMC', 8),
    ('E_MM_GAUSS', 3, 40, 'MODE_MJHMC', 8),
    ('E_MM_GAUSS', 32, 300, 'MODE_MJHMC', 6),         # the mixture in row form too (round 6): full rows of four-lane groups,
    ('E_MM_GAUSS', 27, 20011, 'MODE_MJHMC', 5),       #   short rows, a ragged last tile (trajectory launch in row form on the single-iteration side),
    ('E_MM_GAUSS', 27, 200003, 'MODE_MJHMC', 5),      #   the same with a persistent grid walking several tiles,
    ('E_MM_GAUSS', 12, 700, 'MODE_MJHMC', 9),         #   two-lane groups
    ('E_ROUGH_WELL', 40, 200, 'MODE_CONTROL', 6),
    ('E_ISO_GAUSS', 16, 200, 'MODE_CONTROL', 12),
    ('E_ISO_GAUSS', 24, 77, 'MODE_CTHMC', 12),
])
def test_fused_equals_single_iterations(kind, D, N, mode_name, n_iter):
    params = {'E_FUNNEL_NEAL': [3.0], 'E_FUNNEL_REF': [1.0], 'E_ROUGH_WELL': [100.0, 4.0], 'E_MM_GAUSS': [3.0],
              'E_DIAG_GAUSS': list(10.0 ** np.linspace(-2, 0, D))}.get(kind, [1.3])
    from mjhmc_amd import _lib
    mode = getattr(_lib, mode_name)
    (a, b), _lib = _pair(kind, D, N, mode, params=params)
    for s in (a, b):
        s.set_hparams(0.2, 6, 0.1, 1.0, 0.5)
    a.ring_alloc(n_iter)
    b.ring_alloc(n_iter)
    stats_a, done_a = a.iterate(n_iter, ring_slot0=0)
    assert done_a == n_iter
    stats_b = []
    for i in range(n_iter):
        st, d = b.iterate(1, ring_slot0=i)
        assert d == 1
        stats_b.append(st[0])
    _same_state(a, b, _lib)
    assert [_stats_tuple(s) for s in stats_a[:n_iter]] == [_stats_tuple(s) for s in stats_b]
    assert bits_equal(a.ring_read(0, n_iter, stacked=True), b.ring_read(0, n_iter, stacked=True))
    assert bits_equal(a.ring_read_dwell(0, n_iter), b.ring_read_dwell(0, n_iter))
    # and without a ring, continuing from the live state that now sits in the last ring slot
    stats_a, done_a = a.iterate(3)
    for i in range(3):
        b.iterate(1)
    assert done_a == 3
    _same_state(a, b, _lib)


@pytest.mark.parametrize('kind,D,N', [('E_ISO_GAUSS', 512, 70), ('E_ISO_GAUSS', 24, 301),
                                      ('E_FUNNEL_NEAL', 32, 300), ('E_FUNNEL_NEAL', 14, 200)])   # the funnels: the fused row kernel
def test_fused_failure_in_the_middle_of_a_launch(kind, D, N):
    """A few columns blow up after some iterations: the fused call must stop exactly where the sequence of
    single iterations stops, with the same state, counters and RNG position."""
    from mjhmc_amd import _lib
    params = [3.0] if kind == 'E_FUNNEL_NEAL' else [1.0]
    lo = 0.02 if kind == 'E_FUNNEL_NEAL' else 0.6    # (the funnel is stiff where x0 is negative: it fails at far smaller scales)
    # Far out in the Gaussian the leapfrog energy error (~ eps^2 |x|^2 / 8) reaches several hundred, so now
    # and then exp(H0 - H1) overflows: scan the initial scale for a first failure after a few good iterations
    found = None
    s_thr = np.sqrt(709.0 / (0.011 * D))     # scale at which the MEAN energy error of the L proposal overflows exp
    for scale in np.linspace(lo, 1.0, 161) * s_thr:
        (p, _), _lib = _pair(kind, D, N, _lib.MODE_MJHMC, params=params, scale=float(scale))
        p.set_hparams(0.5, 5, 0.1, 1.0, 0.5)
        k = 0
        while k < 30:
            _, d = p.iterate(1)
            if d == 0:
                break
            k += 1
        if 1 <= k < 30:
            found = (scale, k)
            break
    if found is None:
        pytest.skip('no initial scale with a late first failure for this shape')
    scale, k = found
    eps = 0.5
    (a, b), _lib = _pair(kind, D, N, _lib.MODE_MJHMC, params=params, scale=float(scale))
    for s in (a, b):
        s.set_hparams(eps, 5, 0.1, 1.0, 0.5)
        s.ring_alloc(40)
    stats_a, done_a = a.iterate(40, ring_slot0=0)
    assert done_a == k
    stats_b = []
    for i in range(k + 1):
        st, d = b.iterate(1, ring_slot0=i)
        stats_b.append(st[0])
        assert d == (1 if i < k else 0)
    # dwelling_times / transitions are only defined once the retry has succeeded (the reference assigns them
    # after draw_from returned, markov_jump_hmc.py:392-396): compared after the retry below
    _same_state(a, b, _lib, fields=('X', 'V', 'EX', 'EV', 'HFLF'))
    assert [_stats_tuple(s) for s in stats_a[:k + 1]] == [_stats_tuple(s) for s in stats_b]
    assert stats_a[k].nonfinite == 1
    assert bits_equal(a.ring_read(0, k, stacked=True), b.ring_read(0, k, stacked=True))
    # both consumed the failed attempt's tick: the retry protocol continues identically
    for s in (a, b):
        s.set_hparams(eps * 0.5, 10, 0.1, 1.0, 0.5)
        s.reset_flf_cache()
    sa, da = a.iterate(2)
    for _ in range(2):
        sb, db = b.iterate(1)
    _same_state(a, b, _lib)


@pytest.mark.parametrize('kind,D,N', [('E_ISO_GAUSS', 512, 70), ('E_ISO_GAUSS', 48, 200), ('E_FUNNEL_NEAL', 32, 300),
                                      ('E_DIAG_GAUSS', 10, 333)])
def test_float32_state(kind, D, N):
    """float32 state (the reference's TensorFlow energies run in float32, tf_distributions.py:89): the fused and
    the single-iteration kernels agree bit for bit, and one iteration from the same float32-representable state
    follows the float64 sampler: same transitions except at near ties, state within float32 rounding."""
    from mjhmc_amd import _lib
    params = {'E_FUNNEL_NEAL': [3.0], 'E_DIAG_GAUSS': list(10.0 ** np.linspace(-2, 0, D))}.get(kind, [1.0])
    (a, b), _lib = _pair(kind, D, N, _lib.MODE_MJHMC, params=params, dtype='float32')
    for s in (a, b):
        s.set_hparams(0.1, 6, 0.1, 1.0, 0.5)
    sa, da = a.iterate(9)
    for _ in range(9):
        b.iterate(1)
    assert da == 9
    _same_state(a, b, _lib)
    # one iteration, float32 vs float64 kernels, from identical (float32-representable) X and V
    (c, d), _lib = _pair(kind, D, N, _lib.MODE_MJHMC, params=params, dtype='float32', dtype2='float64')
    X32, V32 = c.read(_lib.F_X), c.read(_lib.F_V)
    d.write(_lib.F_X, X32)
    d.write(_lib.F_V, V32)
    for s in (c, d):
        s.set_hparams(0.1, 6, 0.1, 1.0, 0.5)
        s.iterate(1)
    tc, td = c.read(_lib.F_TRANS), d.read(_lib.F_TRANS)
    same = tc == td
    assert same.mean() > 0.97, same.mean()
    Xc, Xd = c.read(_lib.F_X)[:, same], d.read(_lib.F_X)[:, same]
    scale = np.abs(Xd).max()
    assert np.abs(Xc - Xd).max() <= 2e-5 * scale
    assert np.allclose(c.read(_lib.F_EX)[same], d.read(_lib.F_EX)[same], rtol=2e-4, atol=2e-4 * scale)


@pytest.mark.parametrize('kind,D,N', [('E_FUNNEL_NEAL', 32, 20000), ('E_ISO_GAUSS', 6, 70001), ('E_ROUGH_WELL', 40, 16400),
                                      # the trajectory launch in row form (a lane per particle, mjhmc_traj_rows_kernel): full and
                                      # short rows of four-lane and two-lane groups, a last tile with padding rows
                                      ('E_FUNNEL_NEAL', 31, 20011), ('E_FUNNEL_NEAL', 21, 9000), ('E_FUNNEL_REF', 16, 40001),
                                      ('E_FUNNEL_REF', 11, 33000), ('E_FUNNEL_NEAL', 9, 16385)])
def test_compacted_inverse_pass_equals_in_kernel(kind, D, N, monkeypatch):
    """Big batches with several particles per wave run an iteration as two launches -- every trajectory (the inverse-L
    proposals of the cold caches in workgroups of their own), then the jump process with a lane per particle, whose movers
    are the next iteration's list (step_kernel.hpp: mjhmc_step_kernel); it must be invisible: state, scalars, transitions
    and the per-iteration counters (the cold tallies come from the list lengths) equal the jump kernel's, which does
    all of it per slot.  (Both samplers from the test build with fused launches switched off: below 160 000 particles
    the product would fuse the multi-iteration calls.)"""
    from mjhmc_amd import _lib
    params = {'E_FUNNEL_NEAL': [3.0], 'E_FUNNEL_REF': [3.0], 'E_ROUGH_WELL': [100.0, 4.0]}.get(kind, [1.0])
    monkeypatch.setenv('MJHMC_NO_FUSE', '1')
    (a, b), _lib = _pair(kind, D, N, _lib.MODE_MJHMC, params=params, libs='hh')
    for s in (a, b):
        s.set_hparams(0.05, 7, 0.1, 1.0, 0.5)
    stats_a, stats_b = [], []
    for it in range(4):
        monkeypatch.delenv('MJHMC_NO_COMPACT', raising=False)
        st, d = a.iterate(1) if it % 2 == 0 else a.iterate(3)
        stats_a += st
        monkeypatch.setenv('MJHMC_NO_COMPACT', '1')
        st, d = b.iterate(1) if it % 2 == 0 else b.iterate(3)
        stats_b += st
    _same_state(a, b, _lib)
    assert [_stats_tuple(s) for s in stats_a] == [_stats_tuple(s) for s in stats_b]
    assert sum(s.n_cold for s in stats_a) > 0 and stats_a[0].n_cold == N        # first iteration: every cache is cold


@pytest.mark.parametrize('kind,D,N', [('E_FUNNEL_NEAL', 32, 20000), ('E_FUNNEL_NEAL', 21, 20011), ('E_ROUGH_WELL', 40, 16400)])
def test_list_carried_between_calls_equals_a_scan_per_call(kind, D, N, monkeypatch):
    """Round 6: a call of the compacted passes that follows a committed call of the same path starts from the list the
    previous call's last jump process left (its movers ARE the cold caches) instead of scanning H_flf -- the
    sampling_iteration() callers' path, one iteration per call.  Invisible: a sampler that scans at every call
    (MJHMC_NO_LIST_CARRY) sees the same state and counters, across everything that must drop the carried list on the way
    -- calls of odd and even length (the two lists alternate), a cache write, reset_flf_cache, a rollback, a state write,
    checkpoint / restore, a fused call in between, new hyper-parameters (which keep it)."""
    from mjhmc_amd import _lib
    params = {'E_FUNNEL_NEAL': [3.0], 'E_FUNNEL_REF': [3.0], 'E_ROUGH_WELL': [100.0, 4.0]}.get(kind, [1.0])
    (a, b), _lib = _pair(kind, D, N, _lib.MODE_MJHMC, params=params, libs='hh')
    for s in (a, b):
        s.set_hparams(0.05, 7, 0.1, 1.0, 0.5)
    stats_a, stats_b = [], []

    def both(op):
        monkeypatch.setenv('MJHMC_NO_FUSE', '1')
        monkeypatch.delenv('MJHMC_NO_LIST_CARRY', raising=False)
        ra = op(a)
        monkeypatch.setenv('MJHMC_NO_LIST_CARRY', '1')
        rb = op(b)
        monkeypatch.delenv('MJHMC_NO_LIST_CARRY', raising=False)
        return ra, rb

    def run(n):
        (sa, da), (sb, db) = both(lambda s: s.iterate(n))
        assert da == db == n
        stats_a.extend(sa)
        stats_b.extend(sb)
        _same_state(a, b, _lib)

    for n in (1, 1, 1, 2, 1, 3, 1):            # odd / even call lengths: the carried list changes sides
        run(n)
    h = a.read(_lib.F_HFLF)
    h[::3] = np.nan                             # a cache write from the host: a third of the caches cold again
    both(lambda s: s.write(_lib.F_HFLF, h))
    run(1)
    assert stats_a[-1].n_cold >= (N + 2) // 3
    run(1)
    both(lambda s: s.reset_flf_cache())
    run(1)
    assert stats_a[-1].n_cold == N
    run(1)
    both(lambda s: s.rollback())                # back to the state before that iteration: ITS list, not the successor's
    run(1)
    run(2)
    both(lambda s: s.checkpoint())
    run(1)
    run(1)
    both(lambda s: s.restore())
    run(1)
    X = a.read(_lib.F_X)
    both(lambda s: s.write(_lib.F_X, X * 1.01))   # a state write clears every cache
    run(1)
    assert stats_a[-1].n_cold == N
    run(1)
    for s in (a, b):                               # new hyper-parameters leave the caches -- and the list -- as they are
        s.set_hparams(0.04, 5, 0.1, 1.0, 0.5)
    run(1)
    run(1)
    monkeypatch.delenv('MJHMC_NO_FUSE', raising=False)    # a fused call in between (the product fuses below 160 000 particles)
    (sa, da), (sb, db) = a.iterate(4), b.iterate(4)
    assert da == db == 4
    _same_state(a, b, _lib)
    run(1)
    run(1)
    assert [_stats_tuple(s) for s in stats_a] == [_stats_tuple(s) for s in stats_b]
    assert 0 < stats_a[1].n_cold < N // 2


def test_timing_switched_off_changes_nothing_but_the_markers():
    """mjhmc_set_timing(0): calls record no HIP-event pair (the drop-in classes run that way); the chain is the same, and
    mjhmc_last_timing keeps reporting the last RECORDED call instead of failing on events that were never recorded."""
    from mjhmc_amd import _lib
    (a, b), _lib = _pair('E_ISO_GAUSS', 64, 500, _lib.MODE_MJHMC)
    for s in (a, b):
        s.set_hparams(0.05, 7, 0.1, 1.0, 0.5)
    a.iterate(3)
    b.iterate(3)
    t_before = b.last_timing()
    assert t_before['n_jump_launches'] == 3 and t_before['total_ms'] > 0
    b.set_timing(False)
    for n in (1, 5, 1):
        sa, da = a.iterate(n)
        sb, db = b.iterate(n)
        assert da == db == n and [_stats_tuple(x) for x in sa] == [_stats_tuple(x) for x in sb]
    _same_state(a, b, _lib)
    assert b.last_timing()['total_ms'] == t_before['total_ms']          # nothing recorded since
    b.set_timing(True)
    b.iterate(2)
    assert b.last_timing()['total_ms'] > 0 and b.last_timing()['total_ms'] != t_before['total_ms']


def test_compacted_passes_failure_in_the_middle_of_a_batch(monkeypatch):
    """A non-finite rate in iteration i > 0 of a multi-iteration call through the compacted passes: the call stops
    there and the state is the one iteration i-1 handed on -- INCLUDING the momentum refresh of its R-movers, which
    rides in the inverse-L pass of iteration i (iterate.hip, iterate_compact_t) -- exactly as without the compacted passes.
    (Gaussian force with fusing switched off: its energy error grows as particles drift outwards, which gives late
    first failures; see test_fused_failure_in_the_middle_of_a_launch.)"""
    from mjhmc_amd import _lib
    D, N = 24, 20000
    monkeypatch.setenv('MJHMC_NO_FUSE', '1')
    s_thr = np.sqrt(709.0 / (0.011 * D))
    mid = 0
    for scale in np.linspace(0.45, 0.9, 46) * s_thr:
        (a, b), _lib = _pair('E_ISO_GAUSS', D, N, _lib.MODE_MJHMC, params=[1.0], scale=float(scale), libs='hh')
        for s in (a, b):
            s.set_hparams(0.5, 5, 0.1, 1.0, 0.5)
        monkeypatch.delenv('MJHMC_NO_COMPACT', raising=False)
        st_a, done_a = a.iterate(12)
        monkeypatch.setenv('MJHMC_NO_COMPACT', '1')
        st_b, done_b = b.iterate(12)
        monkeypatch.delenv('MJHMC_NO_COMPACT', raising=False)
        assert done_a == done_b, scale
        # dwelling times / transitions are only defined once the retry has succeeded (see the fused test above)
        _same_state(a, b, _lib, fields=('X', 'V', 'EX', 'EV', 'HFLF'))
        assert [_stats_tuple(s) for s in st_a[:done_a]] == [_stats_tuple(s) for s in st_b[:done_b]]
        if 0 < done_a < 12:
            mid += 1
            assert st_a[done_a].nonfinite == 1 and st_b[done_b].nonfinite == 1
            # the retry protocol continues identically from the rolled-back state
            for s in (a, b):
                s.set_hparams(0.25, 10, 0.1, 1.0, 0.5)
                s.reset_flf_cache()
            sa, da = a.iterate(3)
            monkeypatch.setenv('MJHMC_NO_COMPACT', '1')
            sb, db = b.iterate(3)
            monkeypatch.delenv('MJHMC_NO_COMPACT', raising=False)
            assert da == db
            _same_state(a, b, _lib, fields=('X', 'V', 'EX', 'EV', 'HFLF') if da < 3 else FIELDS)
        a.close()
        b.close()
        if mid >= 2 or done_a == 0:
            break
    if mid == 0:
        pytest.skip('no initial scale with a first failure in the middle of the batch')


@pytest.mark.parametrize('kind,D,N', [('E_ISO_GAUSS', 512, 33000), ('E_DIAG_GAUSS', 64, 263000),
                                      ('E_ISO_GAUSS', 24, 530003),      # a quad of lanes per particle
                                      ('E_ISO_GAUSS', 40, 270001)])     # ragged rows (predicated chunks)
def test_split_fused_launch_equals_single_launch(kind, D, N, monkeypatch, mode_name='MODE_MJHMC'):
    """A big fused launch runs as two halves on two streams (iterate.hip, iterate_fused_t): invisible in the results, and a
    non-finite rate in either half ends the call like an unsplit one."""
    from mjhmc_amd import _lib
    params = list(10.0 ** np.linspace(-1, 0, D)) if kind == 'E_DIAG_GAUSS' else [1.0]
    (a, b), _lib = _pair(kind, D, N, getattr(_lib, mode_name), params=params, libs='ph')
    (ha, hb), _lib = _pair(kind, D, N, getattr(_lib, mode_name), params=params, libs='hh')      # the pair that can be poisoned
    for s in (a, b, ha, hb):
        s.set_hparams(0.1, 4, 0.1, 1.0, 0.5)
    for n_it in (6, 1, 70 if D == 512 else 3):                     # 70: two fused launches, the parts meet in between
        monkeypatch.delenv('MJHMC_NO_SPLIT', raising=False)
        sa, da = a.iterate(n_it)
        monkeypatch.setenv('MJHMC_NO_SPLIT', '1')
        sb, db = b.iterate(n_it)
        monkeypatch.delenv('MJHMC_NO_SPLIT', raising=False)
        assert da == db == n_it
        assert [_stats_tuple(t) for t in sa] == [_stats_tuple(t) for t in sb]
        _same_state(a, b, _lib)
    if mode_name == 'MODE_CONTROL':
        return                                                     # the discrete-time samplers have no rates to be non-finite
    a, b = ha, hb                                                  # both from the test build: only it can place a failure
    for poison in ('0:7', '0:%d' % (N - 3)):                       # first half, second half
        monkeypatch.setenv('MJHMC_DEBUG_POISON', poison)
        sa, da = a.iterate(5)
        monkeypatch.setenv('MJHMC_NO_SPLIT', '1')
        sb, db = b.iterate(5)
        monkeypatch.delenv('MJHMC_NO_SPLIT', raising=False)
        monkeypatch.delenv('MJHMC_DEBUG_POISON', raising=False)
        assert da == db == 0 and sa[0].nonfinite == 1 and sb[0].nonfinite == 1
        _same_state(a, b, _lib, fields=('X', 'V', 'EX', 'EV', 'HFLF'))
        for s in (a, b):
            s.write(_lib.F_V, s.read(_lib.F_V))                    # heals the poisoned EV
            s.reset_flf_cache()
        sa, da = a.iterate(4)
        monkeypatch.setenv('MJHMC_NO_SPLIT', '1')
        sb, db = b.iterate(4)
        monkeypatch.delenv('MJHMC_NO_SPLIT', raising=False)
        assert da == db == 4
        _same_state(a, b, _lib)


@pytest.mark.parametrize('mode_name', ['MODE_CONTROL', 'MODE_CTHMC'])
def test_split_fused_launch_other_sampler_families(mode_name, monkeypatch):
    test_split_fused_launch_equals_single_launch('E_ISO_GAUSS', 64, 263000, monkeypatch, mode_name=mode_name)


@pytest.mark.parametrize('kind,D,N,n_iter,p_r,ring', [
    ('E_FUNNEL_NEAL', 32, 1000, 9, 0.05, False),      # four-wave workgroup tiles, the last one with three live waves and a ragged row count
    ('E_FUNNEL_NEAL', 32, 255, 6, 0.05, True),        # one workgroup tile, ragged; ring snapshots
    ('E_FUNNEL_NEAL', 32, 20011, 5, 0.05, False),     # a grid of 79 workgroup tiles (below the 256 resident: one tile each)
    ('E_FUNNEL_NEAL', 32, 200003, 5, 0.05, False),    # a persistent grid walking several workgroup tiles (above 65 536 particles)
    ('E_FUNNEL_NEAL', 32, 700, 8, 2.0, False),        # refresh rate 2: more than 32 cold caches per workgroup -- the pool overflows
    ('E_FUNNEL_NEAL', 31, 513, 7, 0.3, True),         #   every iteration, the lanes beyond it integrate in their own wave
    ('E_FUNNEL_NEAL', 21, 300, 70, 0.05, False),      # short rows; across the 64-iteration launch boundary
    ('E_FUNNEL_NEAL', 16, 1500, 9, 0.1, True),        # two-lane groups (a pooled particle on two lanes of ONE chunk column each)
    ('E_FUNNEL_NEAL', 11, 65, 7, 0.1, False),         # two-lane groups, short rows
    ('E_FUNNEL_NEAL', 32, 300, 5, 0.0, False),        # no refresh at all: the pool is empty after the first iteration
    ('E_MM_GAUSS', 32, 1000, 7, 0.1, True),           # the mixture's row form (exp(4 sep x_0) once per particle; a division per coordinate)
    ('E_MM_GAUSS', 14, 513, 6, 0.5, False),           #   two-lane groups, the pool overflowing
])
def test_relay_kernel_equals_the_one_wave_kernel(kind, D, N, n_iter, p_r, ring, monkeypatch):
    """mjhmc_fused_rows_relay_kernel (four-wave workgroups pool their cold caches, the pool's inverse-L trajectories relayed
    in four parts on two lanes per particle: the product's fused row form from kRelayMinL = 12 leapfrog steps up) against
    mjhmc_fused_rows_kernel (round 5's one-wave workgroups, every wave integrating the inverse-L proposal in all its lanes:
    the form shorter trajectories keep): state, scalars, ring and tallies bit for bit, from a chain's first iteration (every
    cache cold: the pool holds 32 of a workgroup's 256) through warm ones, over several calls.  L = 5 with both kernels
    FORCED (test build: MJHMC_FORCE_RELAY / MJHMC_NO_RELAY; parts of one or two leapfrog steps, one of them empty), then
    L = 13 with the product library's own choice -- the relay -- against the forced one-wave kernel."""
    for L, libs in ((5, 'hh'), (13, 'ph')):
        (a, b), _lib = _pair(kind, D, N, 0, params=[1.0] if kind == 'E_FUNNEL_REF' else [3.0], scale=0.7, libs=libs)
        for s in (a, b):
            s.set_hparams(0.05 if L == 5 else 0.02, L, p_r, 1.0, 0.5)
            if ring:
                s.ring_alloc(n_iter)
        for call in range(3):
            monkeypatch.delenv('MJHMC_NO_RELAY', raising=False)
            monkeypatch.setenv('MJHMC_FORCE_RELAY', '1')
            sa, da = a.iterate(n_iter, ring_slot0=0) if ring else a.iterate(n_iter)
            monkeypatch.delenv('MJHMC_FORCE_RELAY', raising=False)
            monkeypatch.setenv('MJHMC_NO_RELAY', '1')
            sb, db = b.iterate(n_iter, ring_slot0=0) if ring else b.iterate(n_iter)
            monkeypatch.delenv('MJHMC_NO_RELAY', raising=False)
            assert da == db == n_iter
            assert [_stats_tuple(t) for t in sa] == [_stats_tuple(t) for t in sb], (L, call)
            _same_state(a, b, _lib)
            if ring:
                assert bits_equal(a.ring_read(0, n_iter), b.ring_read(0, n_iter))
                assert bits_equal(a.ring_read_dwell(0, n_iter), b.ring_read_dwell(0, n_iter))
        a.close()
        b.close()
