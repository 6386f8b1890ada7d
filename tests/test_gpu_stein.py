"""GPU: the kernel Stein discrepancy of a recorded ensemble (csrc/stein.hpp, mjhmc_stein_*, ``DeviceSampler.stein``,
``HMCBase.stein_discrepancy``).

The reference is the header's formula in numpy.longdouble on the states ``ring_read`` returns and ``dist.dEdX_val`` of them
(mjhmc_eval: the evaluation kernel the pass itself runs on the slot, checked against the oracle elsewhere), one call per
slot so that every row sits where it sat in the ring slot -- as tests/test_gpu_energy_observables.py::host_values does.
The device sums are held against it within the first-order rounding bound derived in ``reference``."""
import ctypes

import numpy as np
import pytest

from tests.test_gpu_chainstats import record, _iso, _pot32, _sic_bf16
from tests.test_gpu_energy_observables import _pot64, _same_run
from tests.test_gpu_lagcov import _funnel
from tests.test_gpu_marginals import _ring

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
LD = np.longdouble


# ---------------------------------------------------------------------------------------------------------------------
# the reference and its bound
# ---------------------------------------------------------------------------------------------------------------------
def chain_length(n_use):
    """the longest chain of float64 additions behind S (csrc/stein.hpp): 16 in the thread, 6 in the wave's butterfly, 3 over
    the four waves, then ceil(n_tiles / 256) per finishing thread, 6 and 3 again"""
    nt = (n_use + 63) // 64
    tiles = nt * (nt + 1) // 2
    return 16 + 6 + 3 + (tiles + 255) // 256 + 6 + 3


def reference(X, G, w, c):
    """X, G (D, n) float64 (the stored states and the evaluation kernel's gradient, widened), w (n,) float64, c float64 ->
    (W, W2, S, Sd) in longdouble and a first-order bound on |device - exact| for each.

    The bound, with u = 2^-53 and every operand of the device exactly one of the reference's inputs:
      r2 = sum_d dx^2, dx = fl(xi - xj):     each term carries 2 u (dx, twice) + u (the product) and passes through at most
                                             D - 1 additions of partial sums <= the sum of |terms|:   (D + 2) u r2
      dd = sum_d dg dx:                      u (dg) + u (dx) + u (product), D - 1 additions:          (D + 2) u dd_abs
      gg = sum_d gi gj:                      u (product), D - 1 additions:                             D u gg_abs
    where dd_abs, gg_abs are the sums of |terms|.  The epilogue rounds 11 times (csrc/stein.hpp):
      q = c2 + r2 [1]      relative error eq <= (D + 2) u r2 / q + u
      s = sqrt(q) [2]      eq / 2 + u
      t = 1 / s   [3]      et = eq / 2 + 2 u
      t2 = t t    [4]      2 et + u
      t3 = t2 t   [5]      e3 = 3 et + 2 u
      t5 = t3 t2  [6]      e5 = 5 et + 4 u
      A1 = gg t        [7]   |err| <= gg_abs t (D u + et + u)
      A2 = t3 dd       [8]   |err| <= dd_abs t3 ((D + 2) u + e3 + u)
      A3 = nd t3       [9]   |err| <= nd t3 (e3 + u)
      A4 = (3 t5) r2   [10, 11]  |err| <= 3 t5 r2 (e5 + u + (D + 2) u + u)
      k = ((A1 - A2) + A3) - A4   three additions [12 .. 14 counted with the sums], each <= u K_abs,
          K_abs = gg_abs t + dd_abs t3 + nd t3 + 3 t5 r2
      v = (wi wj) k    two products: 2 u wi wj K_abs
    and the reduction adds one rounding per addition on its longest chain, chain_length(n) of them, each a relative u of a
    partial sum of magnitude <= sum_ij wi wj K_abs.  W: ceil(n / 256) + 9 additions; W2 one product more.  Derived, not tuned."""
    D, n = X.shape
    x, g, wl = X.astype(LD), G.astype(LD), w.astype(LD)
    c2 = LD(np.float64(c) * np.float64(c))                       # (the device's c2 = c * c, rounded once on the host)
    dx = x[:, :, None] - x[:, None, :]
    dg = g[:, :, None] - g[:, None, :]
    r2 = (dx * dx).sum(axis=0)
    dd, dd_abs = (dg * dx).sum(axis=0), np.abs(dg * dx).sum(axis=0)
    gij = g[:, :, None] * g[:, None, :]
    gg, gg_abs = gij.sum(axis=0), np.abs(gij).sum(axis=0)
    q = c2 + r2
    t = 1 / np.sqrt(q)
    t3, t5 = t ** 3, t ** 5
    nd = LD(D)
    k = gg * t - t3 * dd + nd * t3 - 3 * t5 * r2
    u = LD(U)
    eq = (D + 2) * u * r2 / q + u
    et = eq / 2 + 2 * u
    e3, e5 = 3 * et + 2 * u, 5 * et + 4 * u
    K_abs = gg_abs * t + dd_abs * t3 + nd * t3 + 3 * t5 * r2
    dk = (gg_abs * t * (D * u + et + u) + dd_abs * t3 * ((D + 2) * u + e3 + u) + nd * t3 * (e3 + u)
          + 3 * t5 * r2 * (e5 + (D + 4) * u) + 3 * u * K_abs)
    ww = wl[:, None] * wl[None, :]
    per_pair = ww * (dk + (2 + chain_length(n)) * u * K_abs)
    S, Sd = (ww * k).sum(), (np.diag(ww) * np.diag(k)).sum()
    Lw = (n + 255) // 256 + 9
    W, W2 = wl.sum(), (wl * wl).sum()
    bounds = (Lw * u * np.abs(wl).sum(), (Lw + 1) * u * W2, per_pair.sum(), np.diag(per_pair).sum())
    return (W, W2, S, Sd), bounds


def assert_within_bound(got, want, bounds, tag):
    assert len(got) == 4 and np.all(np.isfinite(got)), (tag, got)
    worst = 0.0
    for name, g, exact, b in zip(('W', 'W2', 'S', 'Sd'), got, want, bounds):
        err = abs(LD(g) - exact)
        ratio = float(err / b) if b > 0 else (0.0 if err == 0 else np.inf)
        worst = max(worst, ratio)
        print('%s %s: device = %r, longdouble = %.20g, |err| / bound = %.3g' % (tag, name, g, float(exact), ratio))
        assert err <= b, (tag, name, g, float(exact), float(err), float(b))
    return worst


def slot_inputs(s, X, k):
    """the states of recorded slot k (D, N) as stored and the evaluation kernel's gradient of them, float64"""
    Xk = np.ascontiguousarray(X[:, k, :])
    return Xk, np.asarray(s.distribution.dEdX_val(Xk), dtype=np.float64)


CASES = {
    'control_iso2x100_f64': lambda: _iso(2, 100, 3, 'ControlHMC'),   # unit weights, a partial edge tile, one 16-byte chunk per row
    'mjhmc_iso33x130_f64': lambda: _iso(33, 130, 1),                 # dwell weights, pitch 34, 3 row tiles (2-row edge), D % 16 != 0
    'pot36_f32': _pot32,                                             # float32 state and gradient
    'pot36_f64': _pot64,                                             # the wide float64-state ProductOfT path
    'funnel32x130': _funnel,
    'sic512_bf16': _sic_bf16,                                        # bfloat16 state, float32 gradient, pitch == ndims
}


@pytest.fixture(scope='module')
def iso33():
    """the 33 x 130 ring, shared by the prefix and determinism tests: sampler, states, weights, slot inputs of slot 0"""
    s = CASES['mjhmc_iso33x130_f64']()
    X, w, w_slot0 = record(s, 2)
    Xk, G = slot_inputs(s, X, 0)
    return s, X, w, w_slot0, Xk, G


# ---------------------------------------------------------------------------------------------------------------------
# 1.  values
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', sorted(CASES))
def test_values_against_longdouble(case):
    s = CASES[case]()
    n = 2
    X, w, w_slot0 = record(s, n)
    dev = s._dev
    D, N = dev.ndims, dev.nparticles
    c = float(np.sqrt(D))
    counts0 = (s.distribution.E_count, s.distribution.dEdX_count)
    tick0 = dev.get_tick()
    st = dev.stein(c)
    got = [st.evaluate(k, w_slot0 + k if w_slot0 >= 0 else -1, N) for k in range(n)]
    assert dev.get_tick() == tick0 and (s.distribution.E_count, s.distribution.dEdX_count) == counts0
    for k in range(n):
        Xk, G = slot_inputs(s, X, k)
        assert np.all(np.isfinite(G)) and np.any(G != 0)
        want, bounds = reference(Xk, G, w[k], c)
        assert_within_bound(got[k], want, bounds, '%s slot %d (D = %d, N = %d, c = %.4g)' % (case, k, D, N, c))
        W, W2, S, Sd = got[k]
        assert Sd > 0 and S / W ** 2 > -1e-12 and W * W > W2
    if w_slot0 < 0:
        assert got[0][0] == N and got[0][1] == N
    # unit weights on a jump sampler's slot too, and the literature's c = 1
    one = dev.stein(1.0)
    Xk, G = slot_inputs(s, X, 0)
    want, bounds = reference(Xk, G, np.ones(N), 1.0)
    assert_within_bound(one.evaluate(0, -1, N), want, bounds, '%s unit weights, c = 1' % case)
    one.close()
    st.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2.  prefixes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_use', [1, 2, 64, 65, 130])
def test_n_use_prefixes(iso33, n_use):
    s, X, w, w_slot0, Xk, G = iso33
    c = float(np.sqrt(33))
    st = s._dev.stein(c)
    got = st.evaluate(0, w_slot0, n_use)
    want, bounds = reference(Xk[:, :n_use], G[:, :n_use], w[0][:n_use], c)
    assert_within_bound(got, want, bounds, 'prefix n_use = %d' % n_use)
    if n_use == 1:
        assert got[2] == got[3] and got[1] == got[0] * got[0]
    st.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3.  rows >= n_use are selected out, not multiplied by zero
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_nan_beyond_the_prefix_changes_nothing(dtype):
    D, N, n_use = 5, 130, 70
    rs = np.random.RandomState(6)
    X = rs.randn(D, 2, N)
    X[:, 1, :] = X[:, 0, :]
    X[:, 1, n_use:] = np.nan                                  # slot 1: the same prefix, NaN in every row >= n_use
    X[2, 1, n_use + 3] = np.inf
    from mjhmc_amd import engine
    w = rs.rand(2, N) + 0.5
    w[1] = w[0]
    ctx, dev, stored = _ring(X, dtype=dtype, w=w)
    for p in range(n_use, N):                                 # ... and in every weight >= n_use
        engine.check(ctx.lib.mjhmc_test_ring_write_dwell(dev.handle, 1, p, float('nan')), ctx.lib)
    st = dev.stein(1.5)
    clean, dirty = st.evaluate(0, 0, n_use), st.evaluate(1, 1, n_use)
    assert np.all(np.isfinite(dirty)) and dirty == clean, (clean, dirty)
    want, bounds = reference(stored[:, 0, :n_use], stored[:, 0, :n_use], w[0][:n_use], 1.5)   # E_ISO_GAUSS, sigma = 1: G = x
    assert_within_bound(dirty, want, bounds, 'NaN rows beyond the prefix (%s)' % dtype)
    dev.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4.  bad weights and states
# ---------------------------------------------------------------------------------------------------------------------
def test_nonfinite_weights_and_states_are_refused_with_a_message():
    from mjhmc_amd import engine, _lib
    from mjhmc_amd._lib import EngineError
    D, N = 3, 100
    rs = np.random.RandomState(7)
    X = rs.randn(D, 2, N)
    X[1, 1, 40] = np.nan                                      # slot 1: a NaN state inside the prefix
    w = rs.rand(2, N) + 0.5
    ctx, dev, stored = _ring(X, w=w)
    st = dev.stein(1.0)
    good = st.evaluate(0, 0, N)
    out = np.full(4, -7.0)
    for bad in (np.inf, np.nan):
        engine.check(ctx.lib.mjhmc_test_ring_write_dwell(dev.handle, 0, 77, float(bad)), ctx.lib)
        assert ctx.lib.mjhmc_stein_evaluate(st.handle, 0, 0, N, out.ctypes.data_as(ctypes.c_void_p)) == _lib.ERR_NONFINITE
        assert b'a weight among the first 100 particles in dwell slot 0 is not finite' in ctx.lib.mjhmc_last_error()
        assert np.all(out == -7.0)
        with pytest.raises(EngineError, match='a weight among'):
            st.evaluate(0, 0, N)
        assert st.evaluate(0, 0, 77) == st.evaluate(0, 0, 77) and np.all(np.isfinite(st.evaluate(0, 0, 77)))   # outside the prefix: fine
        assert st.evaluate(0, -1, N)[0] == N                                                     # unit weights: not read
    engine.check(ctx.lib.mjhmc_test_ring_write_dwell(dev.handle, 0, 77, float(w[0, 77])), ctx.lib)
    assert st.evaluate(0, 0, N) == good                                             # the flag does not stick
    with pytest.raises(EngineError, match='a state among the first 41 particles in slot 1 is not finite'):
        st.evaluate(1, 1, 41)
    assert np.all(np.isfinite(st.evaluate(1, 1, 40)))
    assert st.evaluate(0, 0, N) == good
    # argument refusals
    for args, msg in (((2, -1, N), 'state slot 2 is outside the ring of 2'), ((-1, -1, N), 'outside the ring'),
                      ((0, 2, N), 'dwell slot 2 is outside the ring of 2'), ((0, -2, N), 'outside the ring'),
                      ((0, -1, 0), r'n_use must be in \[1, 100\]'), ((0, -1, N + 1), r'n_use must be in \[1, 100\]')):
        with pytest.raises(ValueError, match=msg):
            st.evaluate(*args)
    dev.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5.  determinism, blocks, the run
# ---------------------------------------------------------------------------------------------------------------------
def test_two_evaluations_are_equal(iso33):
    s, X, w, w_slot0, Xk, G = iso33
    a, b = s._dev.stein(2.0), s._dev.stein(2.0)
    first = a.evaluate(0, w_slot0, 130)
    a.evaluate(1, w_slot0 + 1, 65)                            # something else in the partials and the scratch in between
    assert a.evaluate(0, w_slot0, 130) == first and b.evaluate(0, w_slot0, 130) == first
    a.close()
    b.close()


@pytest.mark.parametrize('cls', ['MarkovJumpHMC', 'ControlHMC'])
def test_driver_is_block_independent_and_the_run_is_that_of_expectations(cls):
    D, N, n_iter = 33, 100, 6
    s, s2, t = _iso(D, N, 5, cls), _iso(D, N, 5, cls), _iso(D, N, 5, cls)
    r = s.stein_discrepancy(n_iter, block=2)
    r2 = s2.stein_discrepancy(n_iter, block=6)
    t.expectations(n_iter)
    _same_run(s, t)
    _same_run(s2, t)
    assert r.iterations.tolist() == list(range(n_iter)) and r.n_particles == N and r.c == float(np.sqrt(D))
    for name in ('iterations', 'W', 'W2', 'S', 'Sd', 'v', 'u', 'ksd'):
        assert np.array_equal(getattr(r, name), getattr(r2, name)), name
    assert np.all(np.isfinite(r.u)) and np.all(r.v > 0) and np.isfinite(r.mean_u)
    if cls == 'ControlHMC':
        assert np.all(r.W == N) and np.all(r.W2 == N)
    # every second state of a prefix: the same numbers as the full curve's where they coincide only for the same prefix
    s3 = _iso(D, N, 5, cls)
    r3 = s3.stein_discrepancy(n_iter, every=2, particles=N, c=float(np.sqrt(D)), block=4)
    _same_run(s3, t)
    assert r3.iterations.tolist() == [0, 2, 4] and np.array_equal(r3.S, r.S[::2]) and np.array_equal(r3.u, r.u[::2])
    s4 = _iso(D, N, 5, cls)
    r4 = s4.stein_discrepancy(2, particles=1)
    assert np.all(np.isnan(r4.u)) and np.array_equal(r4.S, r4.Sd) and np.isnan(r4.mean_u)


# ---------------------------------------------------------------------------------------------------------------------
# 6.  separation: the feature does its job
# ---------------------------------------------------------------------------------------------------------------------
def _gauss_ring(X, sigma):
    """tests.test_gpu_marginals._ring for one slot of TestGaussian(sigma): its energy is E_ISO_GAUSS {sigma}"""
    from mjhmc_amd import engine, _lib
    from tests.helpers import hooks_context
    ctx = hooks_context(0)
    D, N = X.shape
    en = engine.DeviceEnergy(ctx, _lib.E_ISO_GAUSS, D, [sigma])
    dev = engine.DeviceSampler(en, np.zeros((D, N)), seed=5, mode=_lib.MODE_MJHMC)
    dev.ring_alloc(1)
    block = np.ascontiguousarray(X)
    engine.check(ctx.lib.mjhmc_test_ring_write(dev.handle, 0, block.ctypes.data), ctx.lib)
    assert np.array_equal(dev.ring_read(0, 1).reshape(D, N), X)
    return dev


def _u(W, W2, S, Sd):
    return float((S - Sd) / (W * W - W2))


def test_a_shifted_ensemble_is_told_from_an_exact_one():
    sigma, N = 1.3, 512
    X = sigma * np.random.RandomState(0).randn(2, N)
    host, device = [], []
    for Xr in (X, X + 0.5):
        want, bounds = reference(Xr, Xr / sigma ** 2, np.ones(N), 1.0)
        host.append(_u(*want))
        dev = _gauss_ring(Xr, sigma)
        st = dev.stein(1.0)
        got = st.evaluate(0, -1, N)
        device.append(_u(*got))
        assert abs(_u(*got) - _u(*want)) < 1e-9, (got, want)      # (the kernel's own gradient may differ from x / sigma^2 in its last bit)
        dev.close()
    print('u exact / shifted: NumPy %.6g / %.6g, device %.6g / %.6g' % (host[0], host[1], device[0], device[1]))
    assert host[1] > 10 * abs(host[0]), host                  # the input separates ...
    assert device[1] > 10 * abs(device[0]), device            # ... and so does the device


# ---------------------------------------------------------------------------------------------------------------------
# 7.  lifetime
# ---------------------------------------------------------------------------------------------------------------------
def test_the_sampler_frees_the_handle_and_a_reallocated_ring_is_refused():
    from mjhmc_amd import engine, _lib
    from mjhmc_amd._lib import EngineError
    ctx = engine.Context(0)
    D, N = 512, 4096
    gbytes = N * D * 8                                        # the handle's dE/dX matrix: 16 MiB
    free0, _ = ctx.mem_info()
    en = engine.DeviceEnergy(ctx, _lib.E_ISO_GAUSS, D, [1.0])
    dev = engine.DeviceSampler(en, np.random.RandomState(0).randn(D, N), seed=1)
    with pytest.raises(EngineError, match='no sample ring'):
        dev.stein(1.0)
    dev.ring_alloc(1)
    free_a, _ = ctx.mem_info()
    st = dev.stein(1.0)
    free_b, _ = ctx.mem_info()
    assert free_a - free_b >= gbytes, (free_a, free_b)
    assert st.evaluate(0, -1, 64)[0] == 64                    # (slot 0 holds zeros: k_p is finite there)
    dev.ring_alloc(3)
    with pytest.raises(ValueError, match='sample ring was re-allocated'):
        st.evaluate(0, -1, 64)
    again = dev.stein(1.0)
    assert again.evaluate(2, -1, 64)[0] == 64
    again.close()                                             # one handle destroyed by hand ...
    dev.close()                                               # ... the other by the sampler
    st.close()
    free_c, _ = ctx.mem_info()
    assert free_c >= free0 - gbytes // 2, 'the handle outlived its sampler: free %d before the sampler, %d after' % (free0, free_c)


def test_a_host_energy_is_refused():
    from mjhmc_amd._lib import EngineError
    from mjhmc_amd.misc.distributions import LambdaDistribution
    from mjhmc_amd.samplers.markov_jump_hmc import MarkovJumpHMC
    A = np.array([[2.0, 0.5], [0.5, 1.0]])
    d = LambdaDistribution(energy_func=lambda X: 0.5 * np.sum(X * A.dot(X), axis=0).reshape(1, -1),
                           energy_grad_func=lambda X: A.dot(X), init=np.random.RandomState(1).randn(2, 70), name='dense quadratic')
    h = MarkovJumpHMC(distribution=d, epsilon=0.2, beta=0.3, num_leapfrog_steps=3, seed=5, resample=False)
    with pytest.raises(ValueError, match='opaque Python callables'):
        h.stein_discrepancy(4)
    h._dev.ring_alloc(2)
    with pytest.raises(EngineError, match='callables are the only evaluation'):
        h._dev.stein(1.0)
