"""GPU: fair sample paths on a uniform time grid (csrc/timegrid.hip, DeviceTimeGrid, HMCBase.paths).

The definition (include/mjhmc_hip.h: mjhmc_timegrid_accumulate) is one float64 addition and one float64 multiplication
per step and a verbatim copy of stored elements; ``host_grid`` restates it in NumPy and every comparison of grids,
clocks and cursors is ``==``."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from tests.test_gpu_chainstats import record, _iso, _pot32, _sic_bf16
from tests.test_gpu_marginals import _ring

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATOL = 1e-10                      # the project's bar for normalised autocorrelations (tests/test_gpu_autocor.py)


# ---------------------------------------------------------------------------------------------------------------------
# the NumPy restatement
# ---------------------------------------------------------------------------------------------------------------------
def host_grid(X, w, dt, J, T=None, j=None, G=None):
    """X (D, n, N) float64 states as the ring holds them, w (n, N) holding times -> grid (D, J, N), clocks T (N,), cursors
    j (N,), continuing from (T, j, G) when given.  Per chain, k ascending: Tn = T + w; while j < J and float(j) * dt < Tn:
    G[:, j] = X[:, k]; j += 1; T = Tn."""
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


def _weights(kind, n, N, seed):
    rs = np.random.RandomState(seed)
    if kind == 'dyadic':          # zeros, and sums that land exactly on grid points of dt = 0.25: pins < against <=
        return rs.randint(0, 9, (n, N)) * 0.125, 0.25
    return rs.exponential(1.0, (n, N)), 0.7


def _dev_grid(tg):
    """(grid (D, n_grid, N), T, j, (covered, max_filled)) of a DeviceTimeGrid"""
    G = tg.read(0, tg.n_grid, stacked=False).reshape(tg.ndims, tg.n_grid, tg.nparticles)
    T, j = tg.read_clocks()
    return G, T, j, tg.progress()


def _assert_same(tg, want, tag):
    G, T, j, (covered, max_filled) = _dev_grid(tg)
    Gh, Th, jh = want
    assert j.dtype == np.int32 and np.array_equal(j, jh), (tag, 'cursors')
    assert np.array_equal(T, Th), (tag, 'clocks')
    bad = int(np.sum(G != Gh))
    assert bad == 0, '%s: %d of %d grid elements differ' % (tag, bad, Gh.size)
    assert (covered, max_filled) == (int(jh.min()), int(jh.max())), (tag, covered, max_filled)


def _status(excinfo):
    return int(str(excinfo.value).rsplit('(status ', 1)[1].rstrip(')'))


# float64: every D of {1, 3, 33, 130, 512} with every N of {1, 63, 64, 65, 200} (one to 256 chunks per row, pitches that
# are not the row length, rows that straddle waves and workgroups, particle counts around the padding to 64); float32 with
# pitch 8 for 5 dimensions and 36 dimensions; bfloat16 (SparseImageCode's state) at 512
DEFINITION_CASES = [('float64', D, N) for D in (1, 3, 33, 130, 512) for N in (1, 63, 64, 65, 200)] + \
    [('float32', 5, 65), ('float32', 36, 65), ('bfloat16', 512, 64)]


# ---------------------------------------------------------------------------------------------------------------------
# 1.  the definition, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype,D,N', DEFINITION_CASES)
def test_definition_bit_for_bit(dtype, D, N):
    n = 6
    X = np.random.RandomState(D * 1000 + N).randn(D, n, N)
    for kind in ('dyadic', 'exponential'):
        w, dt = _weights(kind, n, N, D + 7 * N)
        ctx, dev, stored = _ring(X, dtype, w)
        _, _, jfull = host_grid(stored, w, dt, 10 ** 6)       # every chain's coverage
        for n_grid in sorted({max(1, int(jfull.min()) - 1), int(jfull.max()) + 3, 1}):
            tg = dev.time_grid(n_grid, dt)
            tg.accumulate(0, n, w_slot0=0)
            want = host_grid(stored, w, dt, n_grid)
            _assert_same(tg, want, '%s D=%d N=%d %s n_grid=%d' % (dtype, D, N, kind, n_grid))
            if n_grid > jfull.max():                          # unfilled slots stay zero
                G = _dev_grid(tg)[0]
                for p in range(N):
                    assert not G[:, want[2][p]:, p].any()
            tg.close()
        dev.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2.  blocks
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype,D,N', [('float64', 33, 65), ('float64', 512, 63), ('float32', 5, 65), ('bfloat16', 512, 64)])
def test_blocks_do_not_matter(dtype, D, N):
    n = 6
    X = np.random.RandomState(3).randn(D, n, N)
    for kind in ('dyadic', 'exponential'):
        w, dt = _weights(kind, n, N, 17)
        ctx, dev, stored = _ring(X, dtype, w)
        one, cut = dev.time_grid(9, dt), dev.time_grid(9, dt)
        one.accumulate(0, 6, w_slot0=0)
        for x0, k in ((0, 2), (2, 1), (3, 3)):
            cut.accumulate(x0, k, w_slot0=x0)
        want = host_grid(stored, w, dt, 9)
        _assert_same(one, want, 'one block ' + kind)
        _assert_same(cut, want, 'three blocks ' + kind)
        # reset: a fresh grid
        cut.reset()
        assert not _dev_grid(cut)[0].any() and cut.progress() == (0, 0)
        cut.accumulate(0, 6, w_slot0=0)
        _assert_same(cut, want, 'after reset ' + kind)
        # unit holding times and dt = 1: the grid is the ring
        unit = dev.time_grid(n, 1.0)
        unit.accumulate(0, 4)
        unit.accumulate(4, 2)
        G, T, j, prog = _dev_grid(unit)
        assert np.array_equal(G, stored) and np.all(T == n) and np.all(j == n) and prog == (n, n)
        dev.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3.  padding rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype,D,N', [('float64', 33, 65), ('float32', 5, 1), ('bfloat16', 512, 63)])
def test_padding_rows_are_neither_read_nor_written(dtype, D, N):
    from mjhmc_amd import engine
    n, n_grid = 6, 7
    X = np.random.RandomState(4).randn(D, n, N)
    w, dt = _weights('exponential', n, N, 5)
    ctx, dev, stored = _ring(X, dtype, w)
    for k in range(n):                                        # NaN in every state type and as a holding time
        engine.check(ctx.lib.mjhmc_test_ring_fill_padding(dev.handle, k, 0xFF), ctx.lib)
    tg = dev.time_grid(n_grid, dt)
    tg.accumulate(0, n, w_slot0=0)
    _assert_same(tg, host_grid(stored, w, dt, n_grid), 'padding ' + dtype)
    Npad = (N + 63) // 64 * 64
    raw_bytes = dev.ring_slot_bytes() - 8 * Npad
    row = raw_bytes // Npad
    buf = np.empty(raw_bytes, dtype=np.uint8)
    seen = 0
    for slot in range(n_grid):
        engine.check(ctx.lib.mjhmc_test_timegrid_read_raw(tg.handle, slot, buf.ctypes.data, buf.nbytes), ctx.lib)
        assert not buf[N * row:].any(), 'grid slot %d: a padding row was written' % slot
        seen += int(buf[:N * row].any())
    assert seen > 0
    dev.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4.  refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_as_it_was():
    from mjhmc_amd import engine, _lib
    D, n, N = 33, 6, 65
    X = np.random.RandomState(6).randn(D, n, N)
    w, dt = _weights('exponential', n, N, 8)
    ctx, dev, stored = _ring(X, 'float64', w)
    tg = dev.time_grid(8, dt)
    tg.accumulate(0, 3, w_slot0=0)
    before = host_grid(stored[:, :3], w[:3], dt, 8)
    _assert_same(tg, before, 'first block')
    for bad in (np.inf, np.nan, -0.25):
        engine.check(ctx.lib.mjhmc_test_ring_write_dwell(dev.handle, 4, 64, float(bad)), ctx.lib)
        with pytest.raises(_lib.EngineError) as ei:
            tg.accumulate(3, 3, w_slot0=3)
        assert _status(ei) == _lib.ERR_NONFINITE, str(ei.value)
        _assert_same(tg, before, 'refused block (%r)' % bad)
    engine.check(ctx.lib.mjhmc_test_ring_write_dwell(dev.handle, 4, 64, float(w[4, 64])), ctx.lib)
    tg.accumulate(3, 3, w_slot0=3)
    _assert_same(tg, host_grid(stored, w, dt, 8), 'accepted after the poke was undone')
    # MJHMC_ERR_INVALID
    for args in ((0, dt), (-3, dt), (4, 0.0), (4, -1.0), (4, np.inf), (4, np.nan)):
        with pytest.raises(_lib.EngineError) as ei:
            dev.time_grid(*args)
        assert _status(ei) == -1, (args, str(ei.value))
    for args in ((0, 0, 0), (0, 7, 0), (-1, 2, 0), (5, 2, 0), (0, 2, 5), (0, 2, -2)):
        with pytest.raises(_lib.EngineError) as ei:
            tg.accumulate(args[0], args[1], w_slot0=args[2])
        assert _status(ei) == -1, (args, str(ei.value))
    covered = tg.progress()[0]
    assert 0 < covered < 8
    tg.autocor(0, covered)
    for call in (lambda: tg.autocor(0, covered + 1), lambda: tg.autocor(1, covered), lambda: tg.autocor(0, 0),
                 lambda: tg.read(0, 9), lambda: tg.read(-1, 2), lambda: tg.read(0, 0)):
        with pytest.raises(_lib.EngineError) as ei:
            call()
        assert _status(ei) == -1, str(ei.value)
    _assert_same(tg, host_grid(stored, w, dt, 8), 'after the refused calls')
    # no sample ring yet
    en = engine.DeviceEnergy(ctx, _lib.E_ISO_GAUSS, 3, [1.0])
    bare = engine.DeviceSampler(en, np.zeros((3, 5)), seed=1)
    with pytest.raises(_lib.EngineError) as ei:
        bare.time_grid(4, 1.0)
    assert _status(ei) == -1 and 'ring' in str(ei.value)
    # the grid has its own storage: a re-allocated sample ring does not invalidate it, and the sampler frees it
    dev.ring_alloc(n + 2)
    assert not dev.ring_read(0, n).any()                      # (a new ring, zeroed)
    _assert_same(tg, host_grid(stored, w, dt, 8), 'after the ring grew')
    dev.close()
    tg.close()                                                # (a closed sampler freed it already: no second free)


# ---------------------------------------------------------------------------------------------------------------------
# 5.  autocorrelation along the grid
# ---------------------------------------------------------------------------------------------------------------------
def test_autocorrelation_along_the_grid():
    from mjhmc_amd import engine
    s = _iso(3, 65, 2)
    p = s.paths(120, n_grid=40)
    assert p.covered == 40, p.covered
    for n in (8, 40):                                         # either side of the 32-sample direct / transform switch
        x = p.read(n)
        assert x.shape == (3, 65, n)
        for linear in (False, True):
            sums = engine.context(0).autocor(x, linear=linear)
            if linear:
                sums = sums / (n - np.arange(n))
            want = sums / sums[0]
            got = p.autocor(n, linear=linear)
            print('n=%d linear=%d: max |device - host| = %.3g' % (n, linear, float(np.max(np.abs(got - want)))))
            np.testing.assert_allclose(got, want, rtol=0, atol=ATOL)
    p.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6.  the driver
# ---------------------------------------------------------------------------------------------------------------------
def _bookkeeping(s):
    st = s.state
    return dict(counts=(s.l_count, s.f_count, s.r_count, s.fl_count, s.distribution.E_count, s.distribution.dEdX_count),
                dwell=np.array(s.dwelling_times), X=st.X, V=st.V, tick=s._dev.get_tick())


def test_driver_runs_what_expectations_runs():
    n_iter = 24
    a, b = _iso(4, 200, 9), _iso(4, 200, 9)
    grad0 = a.distribution.dEdX_count                         # (the constructor's own gradient is not the run's)
    p = a.paths(n_iter)
    b.expectations(n_iter)
    ka, kb = _bookkeeping(a), _bookkeeping(b)
    assert ka['counts'] == kb['counts'] and ka['tick'] == kb['tick']
    for name in ('dwell', 'X', 'V'):
        assert np.array_equal(ka[name], kb[name]), name
    assert p.n_grid == n_iter and p.dt > 0 and 0 < p.covered <= n_iter
    # the restatement on a third twin's recorded run
    X, w, _ = record(_iso(4, 200, 9), n_iter)
    assert p.dt == w.sum() / w.size or abs(p.dt - w.mean()) <= 1e-12 * p.dt    # the first (only) block's mean holding time
    G, T, j = host_grid(X[:, :n_iter], w, p.dt, n_iter)
    assert p.covered == j.min() and p.n_chains == 200
    assert np.array_equal(p.read(), np.transpose(G[:, :p.covered], (0, 2, 1)))
    assert np.array_equal(p._grid.read_clocks()[0], T)
    assert abs(p.mean_time - T.mean()) <= 1e-12 * T.mean()
    grads = (ka['counts'][5] - grad0) / 200.0
    assert abs(p.grad_evals_per_time - grads / T.mean()) <= 1e-12 * p.grad_evals_per_time
    with pytest.raises(ValueError):
        p.read(p.covered + 1)
    # blocks
    grids = []
    for block in (5, 24):
        q = _iso(4, 200, 9).paths(n_iter, dt=p.dt, block=block)
        grids.append((q._grid.read(0, n_iter), q._grid.read_clocks(), q.covered))
        q.close()
    assert np.array_equal(grids[0][0], grids[1][0]) and grids[0][2] == grids[1][2] == p.covered
    assert np.array_equal(grids[0][1][0], grids[1][1][0]) and np.array_equal(grids[0][1][1], grids[1][1][1])
    assert np.array_equal(grids[0][0], p._grid.read(0, n_iter))
    p.close()
    # a discrete-time sampler: unit holding times, dt = 1, the grid is its own ring
    h = _iso(4, 200, 9, 'HMC').paths(n_iter)
    Xh, wh, w0 = record(_iso(4, 200, 9, 'HMC'), n_iter)
    assert w0 == -1 and h.dt == 1.0 and h.covered == n_iter and h.mean_time == n_iter
    assert np.array_equal(h.read(), np.transpose(Xh, (0, 2, 1)))
    h.close()


@pytest.mark.parametrize('make', [_pot32, _sic_bf16], ids=['pot36_f32', 'sic512_bf16'])
def test_driver_other_state_types(make):
    n_iter = 6
    p = make().paths(n_iter, block=4)
    X, w, _ = record(make(), n_iter)
    dt = p.dt
    G, T, j = host_grid(X[:, :n_iter], w, dt, n_iter)
    assert p.covered == j.min()
    assert np.array_equal(p._grid.read(0, n_iter), np.transpose(G, (0, 2, 1)))
    p.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7.  the law of the grid
# ---------------------------------------------------------------------------------------------------------------------
def _z_along_eigenvectors(x, mean, cov, N):
    """x (D, N, n): per chain y_p = the mean over the last axis of (u . (x - mean))^2 along each eigenvector u of the true
    covariance (eigenvalue lam); z = (mean_p y_p - lam) / (std_p y_p / sqrt(N))"""
    lam, U = np.linalg.eigh(cov)
    proj = np.einsum('di,dpn->ipn', U, x - mean[:, None, None])
    y = (proj * proj).mean(axis=2)
    return (y.mean(axis=1) - lam) / (y.std(axis=1, ddof=1) / np.sqrt(N))


def test_law_of_the_grid_with_the_embedded_chain_as_negative_control():
    """N independent chains started from the target: every grid point of every chain follows the target, so along each
    eigenvector of the true covariance the per-chain time average of the squared (centred) projection has mean lam, and
    the z score of its mean over N = 8192 chains is a standard normal: |z| < 5 follows from N alone.  The same statistic
    on the raw ring slots (the embedded chain, every state once) is the negative control.  (The projection is centred on
    the target's mean, which is not zero here.)
    Device (MI355X; the test prints both): max |z| 1.16 on the grid, 49.6 on the embedded chain."""
    from mjhmc_amd.misc.distributions import CorrelatedGaussian
    from mjhmc_amd.samplers.markov_jump_hmc import MarkovJumpHMC
    N, D, n_iter = 8192, 6, 200
    n_grid = n_iter // 2
    mean = np.array([1.0, -2.0, 0.5, 3.0, -0.7, 0.2])

    def make():
        np.random.seed(3)
        d = CorrelatedGaussian(ndims=D, log_conditioning=2, nbatch=N, mean=mean)
        return d, MarkovJumpHMC(distribution=d, epsilon=0.4, num_leapfrog_steps=6, beta=0.3, seed=21, resample=False)
    d, s = make()
    p = s.paths(n_iter, n_grid=n_grid)
    assert p.covered == n_grid, (p.covered, n_grid)
    x = p.read()[:, :, n_grid // 4:]
    p.close()
    z = _z_along_eigenvectors(x, d.mean, d.cov, N)
    d2, s2 = make()
    Xr, _, _ = record(s2, n_iter)
    zc = _z_along_eigenvectors(np.transpose(Xr[:, n_iter // 4:n_iter], (0, 2, 1)), d2.mean, d2.cov, N)
    print('law of the grid: max |z| %.3f; the embedded chain (every state once): max |z| %.3f'
          % (float(np.abs(z).max()), float(np.abs(zc).max())))
    assert np.abs(z).max() < 5


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
D, N, n_iter = 24, 301, 20
X0 = np.random.RandomState(5).randn(D, N) + 0.4


def dist_of():
    class Fixed(TestGaussian):
        def init_X(self):
            self.Xinit = X0
    return Fixed(ndims=D, nbatch=N, sigma=1.3)


def make(comm):
    return MarkovJumpHMC(distribution=dist_of(), epsilon=0.3, beta=0.3, num_leapfrog_steps=5, seed=4242, comm=comm,
                         resample=False)


# rank-dependent arguments: rank 0's dt must win, and the ranks must agree on the smallest block
for dt, dt_agreed, block, agreed in ((None, None, 4 + 3 * comm.rank, 4), (0.5 + comm.rank, 0.5, 9 - 4 * comm.rank, 5), (None, None, None, None)):
    s = make(comm)
    t0 = s._dev.get_tick()
    p = s.paths(n_iter, dt=dt, block=block)
    assert s._dev.get_tick() - t0 == n_iter + 1, 'a rank ran more than the 21 iterations (a replayed or retried block)'
    both = comm.allreduce_f64(np.array([p.dt, -p.dt, p.covered, -p.covered, p.mean_time, -p.mean_time]), 'max')
    assert np.array_equal(both[0::2], -both[1::2]), 'the shards disagree on dt, covered or mean_time'
    if dt_agreed is not None:
        assert p.dt == dt_agreed
    local = p._grid.read(0, n_iter)
    jl = p._grid.read_clocks()[1]
    s1 = make(None)
    p1 = s1.paths(n_iter, dt=p.dt, block=agreed)
    whole = p1._grid.read(0, n_iter)
    j1 = p1._grid.read_clocks()[1]
    c0 = int(sum(s._plan.counts[:comm.rank]))
    cols = slice(c0, c0 + local.shape[1])
    assert np.array_equal(local, whole[:, cols]), 'a shard of the grid differs from its columns of the unsharded grid'
    assert np.array_equal(jl, j1[cols])
    assert p.covered == p1.covered == int(j1.min()) and p.covered <= int(jl.min()) and p.n_chains == N
    assert abs(p.mean_time - p1.mean_time) <= 1e-12 * p1.mean_time
    assert abs(p.grad_evals_per_time - p1.grad_evals_per_time) <= 1e-12 * p1.grad_evals_per_time
    np.testing.assert_allclose(p.autocor(), p1.autocor(), rtol=0, atol=1e-10)
    assert (s.l_count, s.f_count, s.r_count) == (s1.l_count, s1.f_count, s1.r_count)
    assert np.array_equal(s.dwelling_times, s1.dwelling_times)
    p.close()
    p1.close()
    comm.barrier()
print('rank %%d ok' %% comm.rank)
'''


def test_sharded_grids_concatenate_to_the_unsharded_grid(tmp_path):
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
