"""GPU: the row form of the funnels and the mixture (a lane per particle: mjhmc_fused_rows_relay_kernel,
mjhmc_fused_rows_kernel, mjhmc_traj_rows_kernel + the jump-process launch) against the NumPy oracle on the same Philox
streams -- not only against each other (tests/test_gpu_fused.py), so that a mistake both kernels share is caught too.

Every path is selected by its real condition through the public classes: fused calls (`sample(n)`, n >= 2) run the relay
kernel from 12 leapfrog steps up for the funnels and from 4 up for the mixture, the one-wave kernel below that for the
funnels, and the fused group form for the mixture below 4; single-iteration calls (`sampling_iteration()`) run the group
form's jump kernel below 16 384 particles and the row trajectory launch + the jump-process launch from there up.  The
float64 row form covers 9 <= ndims <= 32 (two lanes per particle up to 16, four up to 32); 8 and 33 are the group form on
either side of it.

Protocol: `sample(n, preserve_order=True)` gives the state after every iteration; the oracle steps one iteration at a time
and each one is compared.  The oracle holds the whole batch up to 1000 particles -- then every iteration's l / f / r
tallies, cold-cache count and E / dE/dX evaluations equal its own -- and a fixed column subset above (the RNG is keyed by
global particle id), where the whole-batch identities of test_full_size_c4_funnel hold instead.  After every call the
transitions and cache flags are exact and X, V, EX, EV, H_flf and the dwelling times are within 1e-10 (`close`); the
oracle is then resynchronised to the device state, so that drift is bounded by one call."""
import re

import numpy as np
import pytest

from oracle import mjhmc_oracle as orc
from tests.helpers import resync
from tests.test_gpu_parity import close, RTOL

pytestmark = pytest.mark.gpu
np.seterr(all='ignore')

SEED = 0x7A11F00D
BETA = 0.2                       # p_r = -log(1 - beta) / 2 = 0.112
P_R_OVERFLOW = 2.0               # > 32 cold caches per relay workgroup of 256 particles: the pool overflows every iteration
DIMS = (8, 9, 13, 16, 17, 21, 27, 31, 32, 33)
FULL_BATCH_MAX = 1000


def _energy(name, D):
    from mjhmc_amd.misc import distributions as Dm
    if name == 'neal':
        return Dm.Funnel, dict(scale=3.0), orc.FunnelNeal(3.0)
    if name == 'literal':
        return Dm.Funnel, dict(scale=1.0, literal=True), orc.FunnelLiteral(1.0)
    if name == 'rough':
        return Dm.RoughWell, dict(), orc.RoughWell(100, 4)
    if name == 'coupled':                    # Neal's funnel as hipRTC coupled expressions S[k] (built in _sampler)
        return Dm.LambdaDistribution, dict(device_params=[3.0, float(D)]), orc.FunnelNeal(3.0)
    sep = {'mm3': 3, 'mm1': 1}[name]
    return Dm.MultimodalGaussian, dict(separation=sep), orc.MultimodalGaussian(D, sep)


def _initial_state(name, D, N):
    rs = np.random.RandomState(D * 1009 + N)
    X = rs.randn(D, N)
    if name in ('neal', 'coupled'):          # the funnel's own law, x0 ~ N(0, 1.5^2)
        X[0] *= 1.5
        X[1:] *= np.exp(X[0] / 2.)
    elif name == 'literal':                  # the literal funnel diverges: start near the origin
        X *= 0.3
    elif name == 'rough':                    # a few periods of the cosine around the origin
        X *= 3.0
    else:                                    # the mixture: half of the particles at each mode (+-2 sep on dimension 0)
        sep = {'mm3': 3, 'mm1': 1}[name]
        X *= 0.7
        X[0] += np.where(rs.rand(N) < 0.5, -2. * sep, 2. * sep)
    return X


def _eps(name, L):
    return {'neal': 0.05 if L >= 12 else 0.1, 'literal': 0.0015 if L >= 12 else 0.005, 'mm3': 0.1, 'mm1': 0.1}[name]


def _path(name, D, L, fused):
    """the launch path the engine selects (iterate.hip: fused_rows; schedule.hpp: select_schedule; launchers.hpp: launch_fused_rows)"""
    rows = 9 <= D <= 32
    mm = name.startswith('mm')
    if not fused:
        return 'single iteration (group form)'
    if not rows or (mm and L < 4):
        return 'fused group form'
    return 'relay kernel' if L >= (4 if mm else 12) else 'one-wave kernel'


def _stats(st):
    return dict(l=st.l, f=st.f, r=st.r, fl=st.fl, n_cold=st.n_cold, E=st.E_evals, dEdX=st.dEdX_evals, nonfinite=st.nonfinite,
                L=st.L_used)


def _sampler(name, D, N, eps, L, beta, X0, seed=SEED, cls_name='MarkovJumpHMC', dtype='float64', hooks=False):
    """the product's sampler `cls_name` (MarkovJumpHMC) on `name`, recording the IterStats of every attempt (`attempts`)
    and of every committed iteration (`trace`) on the way.  `dtype`: the state type; `hooks`: the energy is bound to the
    test-hooks library (tests.helpers.hooks_context), the only one that reads the MJHMC_NO_* switches"""
    from mjhmc_amd.samplers import markov_jump_hmc as M
    base, kw, en = _energy(name, D)

    class Fixed(base):
        state_dtype = dtype

        def init_X(self):
            self.Xinit = X0

        if hooks:
            def bind(self, device=0):
                from mjhmc_amd import engine
                from tests.helpers import hooks_context
                if self._dev is None:
                    kind, params = self.device_energy()
                    self._dev = engine.DeviceEnergy(hooks_context(device), kind, self.ndims, params)
                return self._dev

    class Recording(getattr(M, cls_name)):
        def _account(self, st):
            self.attempts.append(_stats(st))
            super(Recording, self)._account(st)

        def _commit(self, st):
            self.trace.append(_stats(st))
            super(Recording, self)._commit(st)

    if name == 'coupled':
        from tests.test_gpu_parity import FUNNEL_EXPR
        assert dtype == 'float64' and not hooks
        d = base(energy_func=en.E_val, energy_grad_func=en.dEdX_val, init=X0, name='funnel as expressions',
                 device_expr=FUNNEL_EXPR, **kw)
    else:
        d = Fixed(ndims=D, nbatch=N, **kw)
    extra = dict(resample=False) if cls_name in ('MarkovJumpHMC', 'ContinuousTimeHMC') else {}
    s = Recording(distribution=d, epsilon=eps, beta=beta, num_leapfrog_steps=L, seed=seed, **extra)
    s.attempts, s.trace = [], []
    return s


def _columns(N):
    """None (the whole batch) up to FULL_BATCH_MAX particles; above, 96 random columns, the first and the last one, the
    rest of the last (ragged) tile and, where there are any, columns above 131 072"""
    if N <= FULL_BATCH_MAX:
        return None
    rs = np.random.RandomState(N)
    cols = set(rs.choice(N, size=96, replace=False).tolist()) | {0, N - 1}
    cols |= set(range(N // 64 * 64, N))
    if N > 131072 + 64:
        cols |= set(rs.choice(np.arange(131073, N), size=16, replace=False).tolist())
    return np.array(sorted(cols))


def _oracle(name, D, X0, eps, L, beta, cols, cls_name='MarkovJumpHMC', state_rounding=None):
    _, _, en = _energy(name, D)
    ids = np.arange(X0.shape[1]) if cols is None else cols
    extra = dict(resample=False) if cls_name in ('MarkovJumpHMC', 'ContinuousTimeHMC') else {}
    return getattr(orc, cls_name)(en, X0[:, ids], epsilon=eps, beta=beta, num_leapfrog_steps=L,
                                  rng=orc.PhiloxRNG(SEED, ids), state_rounding=state_rounding, **extra)


def _near(a, b, rtol):
    if rtol == RTOL:
        return close(a, b)
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    fin = np.abs(b[np.isfinite(b)])
    scale = float(fin.max()) if fin.size else 1.0
    return a.shape == b.shape and np.allclose(a, b, rtol=rtol, atol=rtol * 1e-2 * max(scale, 1e-300), equal_nan=True)


def _rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    fin = np.isfinite(b)
    scale = max(1e-300, float(np.abs(b[fin]).max())) if fin.any() else 1.0
    return float(np.max(np.abs(a[fin] - b[fin]) / (np.abs(b[fin]) + 1e-2 * scale))) if fin.any() else 0.0


def _oracle_iteration(o):
    """one oracle sampling_iteration; returns what the device's IterStats of that iteration must hold"""
    en = o.energy
    before = (o.l_count, o.f_count, o.r_count, en.E_count, en.dEdX_count)
    n_cold = int(np.sum(~o.state.shadow_ok))
    o.sampling_iteration()
    return dict(l=o.l_count - before[0], f=o.f_count - before[1], r=o.r_count - before[2], n_cold=n_cold,
                E=en.E_count - before[3], dEdX=en.dEdX_count - before[4])


def _check_counts(st, want, N, L, n_cold_expected, tag):
    """one committed iteration's IterStats: equal to the oracle's (whole batch) or the whole-batch identities (subset)"""
    assert st['nonfinite'] == 0, (tag, 'non-finite rate')
    if want is not None:
        got = {k: st[k] for k in want}
        assert got == want, (tag, 'counts', got, 'oracle', want)
    else:
        assert st['l'] + st['f'] + st['r'] == N, (tag, 'l + f + r', st)
        assert st['n_cold'] == n_cold_expected, (tag, 'n_cold', st['n_cold'], 'expected', n_cold_expected)
        assert st['E'] == N + st['n_cold'] and st['dEdX'] == L * (N + st['n_cold']), (tag, 'evaluations', st)


class _Compare(object):
    """`close`-style comparisons at relative tolerance `rtol` that remember the largest relative difference met"""

    def __init__(self, rtol=RTOL):
        self.rtol, self.worst = rtol, {}

    def __call__(self, what, a, b, tag):
        err = _rel_err(a, b)
        self.worst[what] = max(self.worst.get(what, 0.0), err)
        assert _near(a, b, self.rtol), (tag, what, 'largest relative difference %.3g, allowed %.3g' % (err, self.rtol))


def _check_after_call(s, o, cols, tag, cmp):
    from mjhmc_amd import _lib
    sel = slice(None) if cols is None else cols
    st = s.state
    assert np.array_equal(s._dev.read(_lib.F_TRANS)[sel], o.last_transition), (tag, 'last transitions')
    assert np.array_equal(st.cache_active[sel], o.state.shadow_ok), (tag, 'cache flags')
    cmp('X', st.X[:, sel], o.state.X, tag)
    cmp('V', st.V[:, sel], o.state.V, tag)
    cmp('EX', st.EX[0, sel], o.state.EX[0], tag)
    cmp('EV', st.EV[0, sel], o.state.EV[0], tag)
    warm = o.state.shadow_ok
    cmp('cached H_flf', st.H_flf[0, sel][warm], o.state.shadow.H()[0][warm], tag)
    cmp('dwelling times', s.dwelling_times[sel], o.dwelling_times, tag)


def _run_and_compare(name, D, L, N, n_iter, p_r=None, calls=3, fused=True, rtol=RTOL, eps=None, path=None, hooks=False):
    """`calls` calls of n_iter iterations (fused: sample(n_iter); else n_iter sampling_iteration() calls), each iteration
    compared with the oracle; returns the largest relative difference met per compared quantity.  `eps`: the step size
    (default: _eps); `path`: the launch path for the messages (default: _path, which knows the row range only); `hooks`:
    the sampler runs on the test-hooks library"""
    eps = _eps(name, L) if eps is None else eps
    X0 = _initial_state(name, D, N)
    s = _sampler(name, D, N, eps, L, BETA, X0, hooks=hooks)
    cols = _columns(N)
    sel = slice(None) if cols is None else cols
    o = _oracle(name, D, X0, eps, L, BETA, cols)
    if p_r is not None:
        s.p_r = o.p_r = p_r
    assert close(s.state.V[:, sel], o.state.V), 'tick-0 momenta'
    explicit_path, path = path, _path(name, D, L, fused)
    if explicit_path is not None:
        path = explicit_path
    elif not fused and N >= 16384:
        path = 'single iteration (row trajectory + jump process)' if 9 <= D <= 32 else 'single iteration (compacted group form)'
    n_cold_expected = N
    cmp = _Compare(rtol)
    for call in range(calls):
        tag0 = '%s D=%d N=%d L=%d p_r=%.3g, %s, call %d' % (name, D, N, L, s.p_r, path, call)
        t0 = len(s.trace)
        if fused:
            out = s.sample(n_iter, preserve_order=True)
            assert out.shape == (D, N, n_iter)
            Xs = [out[:, sel, t] for t in range(n_iter)]
            dwell = s._dev.ring_read_dwell(0, n_iter)[:, sel]
            del out
        else:
            Xs, dwell = [], []
            for _ in range(n_iter):
                s.sampling_iteration()
                Xs.append(s.state.X[:, sel])
                dwell.append(s.dwelling_times[sel])
        trace = s.trace[t0:]
        assert len(trace) == n_iter and len(s.attempts) == len(s.trace), (tag0, 'attempts', len(trace), len(s.attempts))
        evals = []
        for t in range(n_iter):
            tag = '%s, iteration %d' % (tag0, t)
            want = _oracle_iteration(o)
            evals.append((want['E'], want['dEdX']))
            _check_counts(trace[t], want if cols is None else None, N, L, n_cold_expected, tag)
            n_cold_expected = N - trace[t]['l']
            cmp('X', Xs[t], o.state.X, tag)
            cmp('dwelling times', dwell[t], o.dwelling_times, tag)
        if fused and cols is None:
            assert np.array_equal(s.eval_trace(n_iter), np.array(evals)), (tag0, 'eval_trace')
        _check_after_call(s, o, cols, tag0, cmp)
        resync(s, o, cols)
    return cmp.worst


FUSED = ([('neal', D, L, 700, 4, None) for L in (15, 5) for D in DIMS] +
         [('literal', D, L, 700, 3, None) for L in (15, 5) for D in (9, 13, 16, 21, 31, 32)] +
         [('mm3', D, 6, 700, 4, None) for D in DIMS] +
         [('mm3', D, 3, 700, 4, None) for D in (9, 16, 21, 32)] +
         [('mm1', 13, 6, 700, 4, None), ('mm1', 27, 6, 700, 4, None)] +
         # fewer particles than a wave tile
         [('neal', 21, 15, 40, 5, None), ('neal', 13, 5, 40, 5, None), ('mm3', 16, 6, 40, 5, None)] +
         # no refresh: the relay pool is empty after the first iteration
         [('neal', 32, 15, 700, 5, 0.0), ('neal', 17, 5, 700, 5, 0.0), ('mm3', 27, 6, 700, 5, 0.0)] +
         # the pool overflowing, odd ndims: a padding coordinate must not pick up a refreshed momentum
         [('neal', 31, 15, 700, 4, P_R_OVERFLOW), ('neal', 13, 15, 700, 4, P_R_OVERFLOW),
          ('neal', 21, 5, 700, 4, P_R_OVERFLOW), ('literal', 9, 15, 700, 3, P_R_OVERFLOW),
          ('mm3', 27, 6, 700, 4, P_R_OVERFLOW), ('mm3', 9, 6, 700, 4, P_R_OVERFLOW)] +
         # persistent grids: above 65 536 particles every wave walks a second tile (one relay workgroup / four one-wave
         # blocks resident per CU on 256 CUs); a column subset with ids above 131 072 and the last, ragged tile
         [('neal', 31, 15, 200003, 3, None), ('neal', 13, 5, 200003, 3, None), ('mm3', 27, 6, 200003, 3, None)])


@pytest.mark.parametrize('name,D,L,N,n_iter,p_r', FUSED)
def test_fused_calls_match_oracle(name, D, L, N, n_iter, p_r):
    """Fused calls, three in a row on one sampler (two at 200 003 particles), the cold caches carried from call to call:
    the relay kernel (L = 15 / mixture L = 6), the one-wave kernel (funnels, L = 5) and the mixture's fused group form
    (L = 3) at every row template and both neighbours of the row range, 700 particles (11 wave tiles: a last relay
    workgroup with three live waves, a ragged last tile), fewer than a wave tile, no refresh, an overflowing pool and
    200 003 particles."""
    _run_and_compare(name, D, L, N, n_iter, p_r=p_r, calls=2 if N > FULL_BATCH_MAX else 3)


@pytest.mark.parametrize('name,D,L,n_iter,rtol', [('neal', 21, 15, 70, 3.2e-9), ('neal', 13, 5, 66, 8e-10), ('mm3', 17, 6, 68, RTOL)])
def test_long_fused_call_matches_oracle(name, D, L, n_iter, rtol):
    """One fused call across the 64-iteration launch boundary, the oracle stepped alongside without a resync: the tallies
    and transitions exact all the way, the states within `rtol`.  Over so many iterations the funnel's ulp-level
    differences grow; the largest relative differences measured on an MI355X (of X, V, EX, EV, H_flf and the dwelling
    times, every iteration) are 3.2e-10 (V) for the relay kernel at D = 21, 7.5e-11 (V) for the one-wave kernel at D = 13
    and 1.9e-12 (dwelling times) for the mixture: each funnel case is bounded at 10x its figure, the mixture at 1e-10."""
    worst = _run_and_compare(name, D, L, 300, n_iter, calls=1, rtol=rtol)
    print('%s D=%d L=%d, %d iterations: largest relative differences %s' % (name, D, L, n_iter, worst))


SINGLE = ([(name, D, 300) for name in ('neal', 'literal', 'mm3') for D in DIMS] + [('mm1', 17, 300)] +
          [('neal', D, 20011) for D in (9, 16, 21, 32, 33)] + [('literal', D, 20011) for D in (13, 31)] +
          [('mm3', D, 20011) for D in (17, 27)])


@pytest.mark.parametrize('name,D,N', SINGLE)
def test_single_iterations_match_oracle(name, D, N):
    """sampling_iteration() calls: the group form's jump kernel below 16 384 particles (a group of lanes per particle:
    group_bcast0 / dim_of), the row trajectory launch + the jump-process launch from there up, with the cold list carried
    from call to call."""
    L = {'neal': 15, 'literal': 5}.get(name, 6)
    _run_and_compare(name, D, L, N, 4, calls=2, fused=False)


@pytest.mark.parametrize('D,L,rtol', [(14, 15, 1e-8), (14, 5, RTOL), (32, 15, 2e-9), (32, 5, RTOL)])
def test_nonfinite_rate_in_the_middle_of_a_fused_row_launch(D, L, rtol, capsys):
    """The Neal funnel in row form meets a non-finite rate at iteration k of a fused call: the iterations before it are the
    fused launch's, the retried one (epsilon halved, L doubled, the caches wiped: markov_jump_hmc.py:376-389) is a single
    call in the group form, and the fused launch resumes after it.  Everything equals the oracle's loop with its own retry
    recursion: every iteration's state, tallies and evaluations, the retry depths printed, the restored hyper-parameters.
    (The initial scale is found as in test_gpu_fused.py::test_fused_failure_in_the_middle_of_a_launch.  It puts energies up
    to 1e57 in the batch, and the relay cases' iterations after the retry amplify ulp-level differences: the largest
    relative differences measured on an MI355X are 1.7e-9 (dwelling times) at D = 14, L = 15 and 1.3e-10 (X) at D = 32,
    L = 15, bounded at 1e-8 and 2e-9; the one-wave cases stay within 1e-10.)"""
    from mjhmc_amd import engine, _lib
    N, eps = 200 if D == 14 else 300, 0.5
    beta = 1. - np.exp(-0.2)                       # p_r = 0.1
    found = None
    s_thr = np.sqrt(709.0 / (0.011 * D))
    rs = np.random.RandomState(D * 7 + N)
    Z = rs.randn(D, N)
    ctx = engine.context(0)
    en = engine.DeviceEnergy(ctx, _lib.E_FUNNEL_NEAL, D, [3.0])
    for scale in np.linspace(0.02, 1.0, 161) * s_thr:
        p = engine.DeviceSampler(en, Z * scale, seed=SEED)
        p.set_hparams(eps, L, -np.log(1 - beta) * 0.5, 1.0, 0.5)
        k = 0
        while k < 9:
            _, d = p.iterate(1)
            if d == 0:
                break
            k += 1
        p.close()
        if 1 <= k < 9:
            found = (float(scale), k)
            break
    assert found is not None, 'no initial scale with a first failure after 1 .. 8 good iterations'
    scale, k = found
    X0 = Z * scale
    n_iter = k + 4
    s = _sampler('neal', D, N, eps, L, beta, X0)
    o = _oracle('neal', D, X0, eps, L, beta, None)
    tag0 = 'neal D=%d N=%d L=%d scale %.4g, %s, failure at iteration %d' % (D, N, L, scale, _path('neal', D, L, True), k)
    capsys.readouterr()
    out = s.sample(n_iter, preserve_order=True)
    printed = [float(x) for x in re.findall(r'doubling back\. Depth: ([0-9.]+)', capsys.readouterr().out)]
    dwell = s._dev.ring_read_dwell(0, n_iter)
    assert len(s.trace) == n_iter
    assert sum(a['nonfinite'] for a in s.attempts) == len(s.attempts) - n_iter >= 1, (tag0, s.attempts)
    assert s.attempts[k]['nonfinite'] == 1 and all(a['nonfinite'] == 0 for a in s.attempts[:k]), (tag0, s.attempts)
    evals = []
    cmp = _Compare(rtol)
    for t in range(n_iter):
        tag = '%s, iteration %d' % (tag0, t)
        n_retries = len(getattr(o, 'retry_depths', []))
        want = _oracle_iteration(o)
        n_retries = len(getattr(o, 'retry_depths', [])) - n_retries
        assert (n_retries > 0) == (t == k) or t > k, (tag, 'the oracle retried', n_retries)
        evals.append((want['E'], want['dEdX']))
        st = dict(s.trace[t])
        assert {k_: st[k_] for k_ in ('l', 'f', 'r')} == {k_: want[k_] for k_ in ('l', 'f', 'r')}, (tag, st, want)
        assert st['L'] == L << n_retries, (tag, 'leapfrog steps', st['L'], 'oracle retries', n_retries)
        cmp('X', out[:, :, t], o.state.X, tag)
        cmp('dwelling times', dwell[t], o.dwelling_times, tag)
    assert np.array_equal(s.eval_trace(n_iter), np.array(evals)), (tag0, 'evaluations per iteration, the retries included')
    assert printed == list(o.retry_depths), (tag0, 'retry depths', printed, o.retry_depths)
    assert (s.epsilon, s.num_leapfrog_steps) == (eps, L) == (o.epsilon, o.num_leapfrog_steps)
    _check_after_call(s, o, None, tag0, cmp)
