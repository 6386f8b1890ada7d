"""GPU: per-group ("per data row") statistics of grouped linear models on the device (csrc/dense_lin_group_pointwise.hpp,
mjhmc_pointwise_create_grouped, HMCBase.group_pointwise / group_waic) against float64 NumPy on the
float32-rounded model and states.  Shapes are the smallest at which each failure can occur: every pad (NB = 1, 2, 4), groups
that fill a lane's slots (C = 2, 16) and groups that leave padding slots (C = 3, 5, 10), one group into the second grouped
block and a mostly empty last block, a partial second tile, three strips with the last partial.

THE BAR of a statistic of a value t at a column (``group_bars``), in the manner of tests/test_gpu_pointwise.py::host_bar:
per (column, particle)

    e = L dU + (C + 4) 2^-23 + 2^-23 (|lse| + |t|)        [+ (C - 1) 2^-24 |lse| for the summed lse]

averaged over the particles as the statistic averages.  dU is the sup over the group's members of the bound of u = W x + b
evaluated in float32 in ANY order of sums (host_u), L the value's Lipschitz constant in that sup norm: 2 for u_y - lse
(|d u_y| + |d lse|, lse being 1-Lipschitz), 1/2 for the softmax (row c of its Jacobian sm_c (delta_ck - sm_k) has absolute sum
2 sm_c (1 - sm_c) <= 1/2), 1 for lse.  The rest are the float32 steps of the group term given u, with eta = 2^-23, a rounded
operation at eta / 2 relative and expf / logf at 2 eta:
  * m = max: exact.  d_c = u_c - m rounds at (eta / 2) |d_c|, which t_c = expf(d_c) turns into a RELATIVE (eta / 2) |d_c|;
    t_c |d_c| <= 1 / e and s >= 1 (the member with d = 0), so it reaches s at <= (eta / 2)(C - 1) / e, with expf's own 2 eta and
    the C - 1 additions' (C - 1) eta / 2:  rel(s) <= eta (0.69 (C - 1) + 2);
  * lse = m + logf(s): rel(s) is the absolute error of log s, logf adds 2 eta log C, the addition (eta / 2) |lse|:
    |d lse| <= eta (0.69 (C - 1) + 2 + 2 log C) + (eta / 2) |lse| <= (C + 4) eta + (eta / 2) |lse| for every 2 <= C <= 16
    (C = 2: 4.1 <= 6; C = 16: 17.9 <= 20);
  * q[0] (u - lse) with a one-hot q[0]: the subtraction at (eta / 2) |t|, the product with 0 or 1 and the sum of one
    non-zero term exact -- below the form above;
  * sm_c = t_c / s: sm_c (rel(t_c) + rel(s) + eta / 2) <= eta ((C + 4) sm_c + 1), below the form above as sm_c <= 1;
  * the per-group sum of lse is C |d lse| + (C - 1)(eta / 2) C |lse|; the host divides by C.
Every test asserts <= 2 bars (the headroom of the pointwise tests) and, on the CPU, that the float32 restatement of the same
arithmetic lies within 1 bar and that the mistakes the bar must see move some column by more than 10."""
import ctypes

import numpy as np
import pytest

from tests.helpers import hooks_context
from tests.test_gpu_linear import f32
from tests.test_gpu_linear_grouped import FAMILY, dist, exprs, lane_groups, mlr, model      # noqa: F401  (mlr: the fixture)
from tests.test_gpu_pointwise import host_bar, host_stats, host_u
from tests.test_gpu_pointwise import ring_sampler as tall_ring_sampler

pytestmark = pytest.mark.gpu
np.seterr(all='ignore')

ETA = 2.0 ** -23
N = 45                                        # two tiles of 32 particles, the second partial
SHAPES = [(10, 2), (10, 3), (10, 10), (129, 5), (300, 16)]
LL, SM, LSE = 'q[0]*(u - lse)', 'sm', 'lse'
# GeneralizedLinearModel's 'logistic' log-likelihood (q[0] = y, q[1] = 1 on the data rows): y u - softplus(u)
LOGISTIC_L = '-(q[1] != 0.f ? ((u > 20.f ? u : log1pf(expf(u))) - q[0]*u) : (0.5f*u*u))'
VALUES, FLAGS, PER = [LL, SM, LSE], [True, False, False], ['group', 'member', 'group']


# ---------------------------------------------------------------------------------------------------------------------
# engine-level fixtures: a sampler of the test build whose ring slots hold given states and weights
# ---------------------------------------------------------------------------------------------------------------------
def ring_sampler(W, b, q, C, G, X, dtype='float64', w=None):
    """X (D, n, N) float32-valued states -> a DeviceSampler of the grouped model whose ring slots 0 .. n - 1 hold them and
    whose dwell slots hold w (n, N)"""
    from mjhmc_amd import engine, _lib
    ctx = hooks_context(0)
    D = W.shape[1]
    e, g = exprs()
    en = engine.DeviceEnergy.from_linear_grouped(ctx, W, b, (C, G), e, g, expert_params=q)
    n, Np = X.shape[1], X.shape[2]
    dev = engine.DeviceSampler(en, np.zeros((D, Np)), seed=5, dtype=dtype, mode=_lib.MODE_MJHMC)
    dev.ring_alloc(n)
    for k in range(n):
        block = np.ascontiguousarray(X[:, k, :], dtype=np.float64)
        engine.check(ctx.lib.mjhmc_test_ring_write(dev.handle, k, block.ctypes.data), ctx.lib)
        if w is not None:
            for p in range(Np):
                engine.check(ctx.lib.mjhmc_test_ring_write_dwell(dev.handle, k, p, float(w[k, p])), ctx.lib)
    assert np.array_equal(dev.ring_read(0, n).reshape(D, n, Np), X)
    return ctx, dev


def sums_of(dev, values, flags, per, n, w_slot0=-1):
    """the raw device sums (W, S1, S2, mx, se, n_states) and the handle's column count"""
    pw = dev.group_pointwise(values, flags, per)
    pw.accumulate(0, n, w_slot0=w_slot0)
    out, cols = pw.read(), pw.nexperts
    pw.close()
    return out, cols


def stats_of(sums, m, shape, flag=True):
    from mjhmc_amd.samplers.markov_jump_hmc import PointwiseStatistics
    W, S1, S2, mx, se, n_states = sums
    k = int(np.prod(shape))
    return PointwiseStatistics(W, *([a[m, :k].reshape(shape) for a in (S1, S2, mx, se)] + [n_states, [flag]]))


def same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------------------------
# the NumPy references: float64 on the float32-rounded model, and the float32 restatement of the device's arithmetic
# ---------------------------------------------------------------------------------------------------------------------
def members(C, G, exchange=None):
    m = np.arange(G * C)
    if exchange is not None:           # the last member of group g and the first of group g + 1 trade groups
        m[[exchange * C + C - 1, (exchange + 1) * C]] = m[[(exchange + 1) * C, exchange * C + C - 1]]
    return m


def group_reference(W, b, q, C, G, X, exchange=None, skip_lse=None, rounded=True):
    """float64: (ll (G, n), sm (G, C, n), lse (G, n)) of states X (D, n), the sup bound dU (G, n) of the float32 logits.
    ``rounded=False``: the logits of W, b, X as given (float64) -- the roundings of W and of x to float32 are then two more
    of the D the any-order bound of host_u counts, gamma_{D + 2} in place of gamma_D"""
    GC, D = G * C, W.shape[1]
    if rounded:
        u, du = host_u(W[:GC], b[:GC], X)
    else:
        gamma = (D + 2) * 2.0 ** -24 / (1 - (D + 2) * 2.0 ** -24)
        u = W[:GC].dot(X) + b[:GC, None]
        du = gamma * (np.abs(W[:GC]).dot(np.abs(X)) + np.abs(b[:GC])[:, None])
    mem = members(C, G, exchange)
    ug, dU = u[mem].reshape(G, C, -1), du[mem].reshape(G, C, -1).max(axis=1)
    m = ug.max(axis=1)
    t = np.exp(ug - m[:, None])
    s = t.sum(axis=1)
    lse = m + np.log(s)
    if skip_lse is not None:
        lse[skip_lse] = 0.0
    q0 = f32(q[0, :GC])[mem].reshape(G, C)
    return (q0[:, :, None] * (ug - lse[:, None])).sum(axis=1), t / s[:, None], lse, dU


def group_restated(W, b, q, C, G, X):
    """the device's arithmetic in float32 NumPy (tests/test_gpu_linear_grouped.py::restated's group term): m = max over c
    ascending, t_c = exp(u_c - m), s ascending, lse = m + log(s), t_c / s; the per-group sums as s = c ? s + t : t.
    Returns float64 (ll, sm, the summed lse / C)."""
    GC = G * C
    u = (f32(W[:GC]).astype(np.float32).dot(f32(X).astype(np.float32)) + f32(b[:GC]).astype(np.float32)[:, None])
    ug = u.reshape(G, C, -1)
    m = ug[:, 0]
    for c in range(1, C):
        m = np.maximum(m, ug[:, c])
    t = np.exp(ug - m[:, None])
    s = t[:, 0]
    for c in range(1, C):
        s = s + t[:, c]
    lse = m + np.log(s)
    q0 = q[0, :GC].astype(np.float32).reshape(G, C)
    term = q0[:, :, None] * (ug - lse[:, None])
    ll, ls = term[:, 0], lse
    for c in range(1, C):
        ll, ls = ll + term[:, c], ls + lse
    sm = t / s[:, None]
    assert ll.dtype == np.float32 and sm.dtype == np.float32 and ls.dtype == np.float32
    return ll.astype(np.float64), sm.astype(np.float64), ls.astype(np.float64) / C


def group_bars(C, ll, sm, lse, dU, w):
    """the bars (module docstring) of the statistics of ll (G,), sm (G, C) and the summed lse / C (G,)"""
    def avg(e):
        on = w > 0
        return (e[..., on] * w[on]).sum(axis=-1) / w[on].sum()
    steps = (C + 4) * ETA
    return (avg(2.0 * dU + steps + ETA * (np.abs(lse) + np.abs(ll))),
            avg(0.5 * dU[:, None] + steps + ETA * (np.abs(lse)[:, None] + np.abs(sm))),
            avg(1.0 * dU + steps + ETA * (np.abs(lse) + np.abs(lse)) + (C - 1) * 0.5 * ETA * np.abs(lse)))


def flat_stats(t, w):
    """host_stats over the last axis of t (..., n): (mean, sd, lme), each of t's leading shape"""
    lead = t.shape[:-1]
    return tuple(a.reshape(lead) for a in host_stats(t.reshape(-1, t.shape[-1]), w))


def worst(got, want, bar):
    return float((np.abs(got - want) / bar).max())


def check_against_reference(sums, C, G, ref, w, tag, lme_only=False):
    """the device statistics of VALUES within 2 bars of the float64 reference ``ref`` = (ll, sm, lse, dU)"""
    ll, sm, lse, dU = ref
    bars = group_bars(C, ll, sm, lse, dU, w)
    for m, (t, shape, scale) in enumerate(((ll, (G,), 1.0), (sm, (G, C), 1.0), (lse, (G,), float(C)))):
        p = stats_of(sums, m, shape, FLAGS[m])
        for a in (p.mean, p.var) + ((p.log_mean_exp,) if FLAGS[m] else ()):
            assert np.isfinite(a).all(), (tag, m)
        mean, sd, lme = flat_stats(t, w)
        rows = [('lme', p.log_mean_exp, lme)] if FLAGS[m] else []
        if not lme_only:
            rows += [('mean', p.mean / scale, mean), ('sd', np.sqrt(p.var) / scale, sd)]
        for name, got, want in rows:
            ratio = worst(got, want, bars[m])
            print('%s value %d %s: worst error / bar = %.3f' % (tag, m, name, ratio))
            assert ratio <= 2.0, (tag, m, name, ratio)
    return bars


# ---------------------------------------------------------------------------------------------------------------------
# 1. exact structure
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('D,C', SHAPES)
def test_exact_structure(D, C, dtype):
    """integers below 2^24 over 45 particles of unit weight pin the slot -> column map across lane types, blocks, padding
    slots (C = 3, 10) and the mostly empty last block (G = 8 Gl + 1): per group (float)j sums to C^2 g + C (C - 1) / 2,
    q[1] to C, (float)c to C (C - 1) / 2; per member (float)j is j and a ramp in q[0] comes back as its float32 self"""
    Gl = lane_groups(D, C)
    X = f32(np.random.RandomState(D).randn(D, 1, N))
    for G in (8 * Gl + 1, 3 * 8 * Gl - 2):
        for plain in (0, 7):
            W, b, q = model(D, C, G, plain)
            GC = G * C
            q[0] = 1.0 + np.arange(GC + plain) / (GC + plain)
            _, dev = ring_sampler(W, b, q, C, G, X, dtype=dtype)
            g, j = np.arange(G, dtype=np.float64), np.arange(GC, dtype=np.float64)
            (Wt, S1, S2, mx, se, ns), cols = sums_of(dev, ['(float)j', 'q[1]', 'q[0]', '(float)j'], [False] * 4,
                                                     ['group', 'group', 'member', 'member'], 1)
            assert Wt == 45.0 and ns == 45 and cols == GC and S1.shape == (4, GC)
            jsum = C * C * g + C * (C - 1) / 2
            assert jsum.max() < 2 ** 24
            assert np.array_equal(S1[0, :G], 45 * jsum) and np.array_equal(S2[0, :G], 45 * jsum * jsum), (G, plain)
            assert np.array_equal(S1[1, :G], np.full(G, 45.0 * C)) and np.array_equal(S2[1, :G], np.full(G, 45.0 * C * C))
            assert np.array_equal(S1[2] / 45.0, f32(q[0, :GC])), (G, plain)
            assert np.array_equal(S1[3], 45 * j) and np.array_equal(S2[3], 45 * j * j), (G, plain)
            # a per-group value fills the first G columns; the rest read as empty, and nothing asked for a log-mean-exp
            assert np.all(S1[:2, G:] == 0.0) and np.all(S2[:2, G:] == 0.0)
            assert np.all(np.isneginf(mx)) and np.all(se == 0.0)
            # every value per group: the handle has G columns
            (Wt, S1, S2, mx, se, ns), cols = sums_of(dev, ['(float)c'], [True], ['group'], 1)
            assert cols == G and S1.shape == (1, G)
            assert np.array_equal(S1[0], np.full(G, 45.0 * C * (C - 1) / 2))
            assert np.array_equal(mx[0], np.full(G, C * (C - 1) / 2.0)) and np.array_equal(se[0], np.full(G, 45.0))
            dev.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. values against float64 NumPy
# ---------------------------------------------------------------------------------------------------------------------
def assert_the_bars_hold_and_discriminate(W, b, q, C, G, X, w, ref, bars):
    """CPU: the float32 restatement within 1 bar of float64; one dropped particle, the group index off by one, one member
    exchanged between neighbouring groups, and one group's lse left out (the values that see it) each move some column's
    mean by more than 10 bars"""
    ll, sm, lse, _ = ref
    for m, (t, r) in enumerate(zip((ll, sm, lse), group_restated(W, b, q, C, G, X))):
        for name, got, want in zip(('mean', 'sd', 'lme'), flat_stats(r, w), flat_stats(t, w)):
            if name != 'lme' or FLAGS[m]:
                assert worst(got, want, bars[m]) <= 1.0, ('restated', m, name, worst(got, want, bars[m]))
    g = G // 2
    ex = group_reference(W, b, q, C, G, X, exchange=min(g, G - 2))
    sk = group_reference(W, b, q, C, G, X, skip_lse=g)
    last = np.flatnonzero(w > 0)[-1]
    wd = w.copy()
    wd[last] = 0.0
    for m, t in enumerate((ll, sm, lse)):
        mean = flat_stats(t, w)[0]
        assert worst(flat_stats(t, wd)[0], mean, bars[m]) > 10, ('dropped', m)
        assert worst(np.roll(mean, 1, axis=0), mean, bars[m]) > 10, ('off by one', m)
        assert worst(flat_stats(ex[m], w)[0], mean, bars[m]) > 10, ('exchange', m)
        if m != 1:                     # (the softmax does not see lse)
            assert worst(flat_stats(sk[m], w)[0], mean, bars[m]) > 10, ('lse left out', m)


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('D,C', [(10, 3), (129, 5), (300, 16)])
def test_values_against_float64(D, C, dtype):
    """the log-likelihood q[0]*(u - lse) per group (log-mean-exp on), sm per member and lse summed per group (divided by C
    here): mean, sd and log-mean-exp within 2 bars (module docstring); the softmax means of a group sum to 1"""
    G = 8 * lane_groups(D, C) + 1
    W, b, q = model(D, C, G, 7)
    X = f32(np.random.RandomState(D).randn(D, 1, N))
    w = np.ones(N)
    ref = group_reference(W, b, q, C, G, X[:, 0, :])
    bars = group_bars(C, *ref, w)
    assert_the_bars_hold_and_discriminate(W, b, q, C, G, X[:, 0, :], w, ref, bars)
    _, dev = ring_sampler(W, b, q, C, G, X, dtype=dtype)
    sums, cols = sums_of(dev, VALUES, FLAGS, PER, 1)
    assert cols == G * C
    check_against_reference(sums, C, G, ref, w, '%dx%d %s' % (D, C, dtype))
    fitted = stats_of(sums, 1, (G, C), False).mean
    assert np.abs(fitted.sum(axis=1) - 1.0).max() <= 2 * C * ETA
    dev.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. range
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_range(dtype):
    """tests/test_gpu_linear_grouped.py::test_range's model: b puts members of some groups at +-200, where expf(u) alone
    overflows and exp(log-likelihood) underflows; every statistic is finite and the log-mean-exp of the log-likelihood
    stays within the bar"""
    D, C = 129, 5
    G = 8 * lane_groups(D, C) + 3
    W, b, q = model(D, C, G, 7, seed=2)
    rs = np.random.RandomState(8)
    far = rs.choice(G * C, size=40, replace=False)
    b[far] += np.where(rs.rand(40) < 0.5, 200.0, -200.0)
    X = f32(np.random.RandomState(4).randn(D, 1, N))
    w = np.ones(N)
    ref = group_reference(W, b, q, C, G, X[:, 0, :])
    assert ref[0].min() < -190 and np.exp(ref[0].min()) < 1e-80
    bars = group_bars(C, *ref, w)
    r = group_restated(W, b, q, C, G, X[:, 0, :])
    assert worst(flat_stats(r[0], w)[2], flat_stats(ref[0], w)[2], bars[0]) <= 1.0
    _, dev = ring_sampler(W, b, q, C, G, X, dtype=dtype)
    sums, _ = sums_of(dev, VALUES, FLAGS, PER, 1)
    for a in sums[1:3]:
        assert np.isfinite(a).all()
    assert np.isfinite(sums[3][0, :G]).all() and np.isfinite(sums[4][0, :G]).all()
    check_against_reference(sums, C, G, ref, w, 'range %s' % dtype, lme_only=True)
    dev.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. C = 2 is logistic regression
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_two_classes_are_logistic_regression(dtype):
    """rows a_i, classes {0, 1}: u_y - LSE(u_0, u_1) of the grouped model at x is y v - softplus(v), v = a_i . beta, of the
    'logistic' tall expression at beta = x[F:2F] - x[:F] -- exact for states on the 2^-8 grid of [-4, 4].  Per data row the
    mean, sd and log-mean-exp of the two passes agree within the sum of their bars."""
    F, C = 5, 2
    G = 8 * lane_groups(2 * F, C) + 1
    rs = np.random.RandomState(12)
    A = rs.randn(G, F) / np.sqrt(F)
    y = rs.randint(0, 2, size=G)
    Wg = np.zeros((G, C, C * F))
    for c in range(C):
        Wg[:, c, c * F:(c + 1) * F] = A
    Wg, bg = Wg.reshape(G * C, C * F), np.zeros(G * C)
    qg = np.vstack([(np.arange(C)[None, :] == y[:, None]).astype(float).reshape(-1), np.ones(G * C)])
    Xg = rs.randint(-1024, 1025, size=(C * F, 1, N)) / 256.0
    beta = Xg[F:] - Xg[:F]
    assert np.array_equal(f32(Xg), Xg) and np.array_equal(f32(beta), beta)
    w = np.ones(N)
    # the grouped pass
    ll, sm, lse, dU = group_reference(Wg, bg, qg, C, G, Xg[:, 0, :])
    bar_g = group_bars(C, ll, sm, lse, dU, w)[0]
    _, dev = ring_sampler(Wg, bg, qg, C, G, Xg, dtype=dtype)
    sums, cols = sums_of(dev, [LL], [True], ['group'], 1)
    assert cols == G
    pg = stats_of(sums, 0, (G,))
    dev.close()
    # the per-expert pass of the logistic tall expression on the same rows (tests/test_gpu_pointwise.py's fixtures)
    from mjhmc_amd.samplers.markov_jump_hmc import PointwiseStatistics
    qt = np.vstack([y.astype(float), np.ones(G)])
    _, tall = tall_ring_sampler(A, np.zeros(G), beta, dtype=dtype, q=qt)
    pw = tall.pointwise([LOGISTIC_L], [True])
    pw.accumulate(0, 1)
    pt = PointwiseStatistics(*(pw.read() + ([True],)))
    tall.close()
    v, dv = host_u(A, np.zeros(G), beta[:, 0, :])
    lt = y[:, None] * v - np.where(v > 20, v, np.log1p(np.exp(np.minimum(v, 20))))
    bar_t = host_bar(dv, lt, w)                                       # |dl / dv| = |y - sigmoid(v)| <= 1
    assert np.abs(lt - ll).max() <= 1e-12                             # the two float64 references are one function
    for name, got_g, got_t in (('mean', pg.mean, pt.mean[0]), ('sd', np.sqrt(pg.var), np.sqrt(pt.var[0])),
                               ('lme', pg.log_mean_exp, pt.log_mean_exp[0])):
        ratio = worst(got_g, got_t, bar_g + bar_t)
        print('C = 2 against logistic %s %s: worst difference / (sum of bars) = %.3f' % (dtype, name, ratio))
        assert ratio <= 1.0, (name, ratio)
    assert worst(np.roll(pt.mean[0], 1), pt.mean[0], bar_g + bar_t) > 10      # (another row's statistic is seen)


# ---------------------------------------------------------------------------------------------------------------------
# 5. weights, the run, determinism
# ---------------------------------------------------------------------------------------------------------------------
def family_model():
    D, C, G, plain = FAMILY
    return model(D, C, G, plain, seed=9) + (C, G)


def family_sampler(n=96, seed=23, init_seed=11):
    from mjhmc_amd.samplers.markov_jump_hmc import MarkovJumpHMC
    W, b, q, C, G = family_model()
    X0 = np.random.RandomState(init_seed).randn(FAMILY[0], n)
    return MarkovJumpHMC(distribution=dist(X0, W, b, q, C, G), seed=seed, epsilon=0.2, beta=0.3, num_leapfrog_steps=5,
                         resample=False)


def test_weights_are_the_holding_times():
    """tests/test_gpu_pointwise.py::test_weights_are_the_holding_times's method on the grouped family"""
    W, b, q, C, G = family_model()
    D = FAMILY[0]
    s = family_sampler()
    out = s.group_pointwise(6, values=VALUES, log_mean_exp=FLAGS, per=PER)
    assert [p.mean.shape for p in out] == [(G,), (G, C), (G,)]
    # the same run again: 7 iterations, the first 6 states weighted by the holding times the NEXT iteration drew
    r = family_sampler()
    r._dev.ring_alloc(7)
    r._run(7, ring_slot0=0)
    r._publish()
    r._read_dwell()
    X = r._dev.ring_read(0, 7).reshape(D, 7, 96)
    dwell = r._dev.ring_read_dwell(0, 7)
    assert np.array_equal(dwell[6], r.dwelling_times)
    w = dwell[1:7].reshape(-1)
    assert np.all(w > 0) and np.all(np.isfinite(w))
    for p in out:
        assert abs(p.W - w.sum()) <= 1e-12 * w.sum() and p.n_states == 6 * 96
    ref = group_reference(W, b, q, C, G, X[:, :6, :].reshape(D, -1))
    bars = group_bars(C, *ref, w)
    for m, (t, scale) in enumerate(zip(ref[:3], (1.0, 1.0, float(C)))):
        mean, sd, lme = flat_stats(t, w)
        rows = [('mean', out[m].mean / scale, mean), ('sd', np.sqrt(out[m].var) / scale, sd)]
        if FLAGS[m]:
            rows.append(('lme', out[m].log_mean_exp, lme))
        else:
            assert np.isnan(out[m].log_mean_exp).all()
        for name, got, want in rows:
            ratio = worst(got, want, bars[m])
            print('weights value %d %s: worst error / bar = %.3f' % (m, name, ratio))
            assert ratio <= 2.0, (m, name, ratio)
    # unit weights are seen: the bar tells the holding times from them
    assert worst(flat_stats(ref[0], np.ones_like(w))[0], flat_stats(ref[0], w)[0], bars[0]) > 10
    # the run is that of expectations(6), bit for bit: the pass itself adds nothing to the energy counters
    t = family_sampler()
    t.expectations(6)
    for a in (s, r):
        assert (a.l_count, a.f_count, a.r_count, a.fl_count) == (t.l_count, t.f_count, t.r_count, t.fl_count)
        assert (a.distribution.E_count, a.distribution.dEdX_count) == (t.distribution.E_count, t.distribution.dEdX_count)
        assert np.array_equal(a.state.X, t.state.X) and np.array_equal(a.state.V, t.state.V)
        assert np.array_equal(a.dwelling_times, t.dwelling_times)


def test_bit_identical_across_runs_and_blocks():
    W, b, q, C, G = family_model()
    _, probe = ring_sampler(W, b, q, C, G, f32(np.zeros((FAMILY[0], 1, 8))))
    h = probe.group_pointwise(['u'])
    strip_tiles = h.strip_tiles
    assert h.n_values == 1 and h.nexperts == G and strip_tiles >= 1
    probe.close()
    Np = strip_tiles * 32 * 2 + 13                      # three strips, the last partial

    X0 = np.random.RandomState(2).randn(FAMILY[0], Np)

    def run(block, n=Np):
        from mjhmc_amd.samplers.markov_jump_hmc import MarkovJumpHMC
        s = MarkovJumpHMC(distribution=dist(X0[:, :n], W, b, q, C, G), seed=31, epsilon=0.2, beta=0.3, num_leapfrog_steps=5,
                          resample=False)
        return s.group_pointwise(6, values=VALUES, log_mean_exp=[True, True, False], per=PER, block=block)

    def raw(out):
        return [a for p in out for a in (p.W, p.S1, p.S2, p.lme_max, p.lme_sum, p.n_states)]
    a, a2, b1, b3 = run(None), run(None), run(1), run(3)
    assert all(np.isfinite(p.mean).all() for p in a) and np.isfinite(a[0].log_mean_exp).all() and a[0].n_states == 6 * Np
    assert same_bits(raw(a), raw(a2))
    assert same_bits(raw(a), raw(b1)) and same_bits(raw(a), raw(b3))
    small = run(None, 45)                               # the control: the first 45 particles alone give other sums
    assert not np.array_equal(small[0].S1, a[0].S1) and not np.array_equal(small[1].S1, a[1].S1) and small[0].n_states == 6 * 45


# ---------------------------------------------------------------------------------------------------------------------
# 6. refusals; a particle of weight 0
# ---------------------------------------------------------------------------------------------------------------------
def small_case(n=2):
    D, C = 10, 3
    G = 8 * lane_groups(D, C) + 1
    W, b, q = model(D, C, G, 7, seed=4)
    X = f32(np.random.RandomState(6).randn(D, n, N))
    return W, b, q, C, G, X


def test_a_value_that_is_not_finite_refuses_the_block():
    from mjhmc_amd import _lib
    W, b, q, C, G, X = small_case()
    _, dev = ring_sampler(W, b, q, C, G, X, w=np.ones((2, N)))
    bad = 'j == 7 ? 1.f/(u - u) : u'                    # member 7 = member 1 of group 2
    pw = dev.group_pointwise(['u', bad, bad], [False, True, False], ['member', 'group', 'member'])
    before = pw.read()
    with pytest.raises(_lib.EngineError) as err:
        pw.accumulate(0, 2)
    assert 'value 1 ' in str(err.value) and 'expert 2 ' in str(err.value) and 'status -5' in str(err.value)
    after = pw.read()
    assert same_bits(before, after) and after[0] == 0.0 and after[5] == 0
    pw.close()
    pw = dev.group_pointwise([bad], [False], ['member'])
    with pytest.raises(_lib.EngineError) as err:
        pw.accumulate(0, 2)
    assert 'value 0 ' in str(err.value) and 'expert 7 ' in str(err.value)
    pw.close()
    # a refused block has added nothing and the handle goes on: slot 1 holds one state whose logits overflow the value
    Xh = X.copy()
    Xh[:, 1, 13] = 2.0 ** 60
    _, dev2 = ring_sampler(W, b, q, C, G, Xh, w=np.ones((2, N)))
    u = f32(W[:G * C]).dot(Xh[:, 1, 13])
    first = int(np.flatnonzero(u > 1e6)[0])
    ok = dev2.group_pointwise(['u > 1e6f ? 1.f/(u - u) : u'], [True], ['member'])
    ok.accumulate(0, 1, w_slot0=0)
    kept = ok.read()
    with pytest.raises(_lib.EngineError) as err:
        ok.accumulate(0, 2, w_slot0=0)
    assert 'value 0 ' in str(err.value) and ('expert %d ' % first) in str(err.value)
    assert same_bits(kept, ok.read())
    ok.accumulate(0, 1, w_slot0=0)
    assert ok.read()[0] == 2 * kept[0] and np.array_equal(ok.read()[1], 2 * kept[1])
    dev.close()
    dev2.close()
    ok.close()                                          # (a closed sampler has freed the handle)


def test_a_particle_of_weight_zero_changes_nothing():
    """particle 13 of slot 0 has weight 0 and a state of 2^60 -- huge logits, an lse and values that are not finite; the
    sums are those of the same ring with an ordinary state there, bit for bit"""
    W, b, q, C, G, X = small_case()
    w = np.random.RandomState(3).randint(1, 9, size=(2, N)) / 4.0
    w[0, 13] = 0.0
    Xh = X.copy()
    Xh[:, 0, 13] = 2.0 ** 60
    _, d1 = ring_sampler(W, b, q, C, G, X, w=w)
    _, d2 = ring_sampler(W, b, q, C, G, Xh, w=w)
    values, flags, per = VALUES + ['u*u'], FLAGS + [True], PER + ['member']
    s1, _ = sums_of(d1, values, flags, per, 2, w_slot0=0)
    s2, _ = sums_of(d2, values, flags, per, 2, w_slot0=0)
    assert same_bits(s1, s2)
    assert s1[0] == w.sum() and np.isfinite(s2[2]).all() and s1[5] == 2 * N
    d1.close()
    d2.close()


def test_other_energies_are_refused_by_name():
    from mjhmc_amd import engine, _lib
    from mjhmc_amd.misc.distributions import ProductOfT
    from mjhmc_amd.samplers.markov_jump_hmc import HMC
    s = HMC(distribution=ProductOfT(ndims=36, nbasis=36, nbatch=40), epsilon=0.1, beta=0.3, num_leapfrog_steps=3, seed=1)
    before = (s.distribution.E_count, s.distribution.dEdX_count)
    with pytest.raises(ValueError, match='PRODUCT_OF_T'):
        s.group_pointwise(3, values=['u'])
    with pytest.raises(ValueError, match='group_values'):
        s.group_waic(3)
    assert (s.distribution.E_count, s.distribution.dEdX_count) == before
    s._dev.ring_alloc(2)
    with pytest.raises(_lib.EngineError, match='MJHMC_E_PRODUCT_OF_T.*mjhmc_pointwise_create'):
        s._dev.group_pointwise(['u'])
    # a tall model: its experts are its rows, and the message names the pass that reports on them
    rs = np.random.RandomState(1)
    Wt, bt = rs.randn(513, 10) / 3.0, 0.1 * rs.randn(513)
    _, tall = tall_ring_sampler(Wt, bt, f32(rs.randn(10, 1, N)))
    with pytest.raises(_lib.EngineError, match='without groups.*mjhmc_pointwise_create'):
        tall.group_pointwise(['u'])
    tall.close()
    W, b, q, C, G, X = small_case(1)
    _, dev = ring_sampler(W, b, q, C, G, X)
    h = ctypes.c_void_p()
    H = _lib.KERNEL_HEADERS.encode()
    for lme, member in ((2, 0), (0, 2)):
        with pytest.raises(ValueError, match='mask'):
            engine.check_args(dev.lib.mjhmc_pointwise_create_grouped(dev.handle, b'u', lme, member, H, ctypes.byref(h)), dev.lib)
    dev.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. group_waic on MultinomialLogisticRegression
# ---------------------------------------------------------------------------------------------------------------------
def test_group_waic_of_the_softmax_regression(mlr):
    """tests/test_gpu_linear_grouped.py's model (300 rows, F = 4, C = 3, 512 chains) after its 150 burn-in iterations:
    lppd_i, p_waic_i and fitted against predict_proba and the log-likelihood from _logits, in float64 NumPy on the same
    run's downloaded states and holding times (one block: the ring still holds the run)"""
    from mjhmc_amd.samplers.markov_jump_hmc import MarkovJumpHMC
    d, eps = mlr
    n, C, D, n_iter = 300, 3, d.ndims, 20
    s = MarkovJumpHMC(distribution=d, epsilon=eps, beta=0.3, num_leapfrog_steps=10, seed=13, resample=False)
    for _ in range(150):
        s.sampling_iteration()
    wa = s.group_waic(n_iter, block=n_iter)
    for a in (wa.lppd_i, wa.p_waic_i, wa.elpd_i, wa.fitted, wa.pointwise.mean, wa.pointwise.var):
        assert np.isfinite(a).all()
    assert np.isfinite([wa.elpd_waic, wa.p_waic, wa.lppd, wa.se, wa.waic]).all()
    print('softmax waic: elpd %.2f, p_waic %.3f, se %.2f, n_warn %d' % (wa.elpd_waic, wa.p_waic, wa.se, wa.n_warn))
    assert wa.n_data == n and wa.lppd_i.shape == (n,) and wa.fitted.shape == (n, C)
    assert np.abs(wa.fitted.sum(axis=1) - 1.0).max() <= 6 * ETA and np.all((wa.fitted > 0) & (wa.fitted < 1))
    assert 0 < wa.p_waic < 2 * D and wa.n_warn == 0
    assert wa.waic == -2.0 * wa.elpd_waic
    # the NumPy path on the run the ring still holds: slots 0 .. n_iter, state k weighted by the dwell of slot k + 1
    X = s._dev.ring_read(0, n_iter + 1).reshape(D, n_iter + 1, 512)
    dwell = s._dev.ring_read_dwell(0, n_iter + 1)
    assert np.array_equal(dwell[n_iter], s.dwelling_times)
    w = dwell[1:].reshape(-1)
    assert abs(wa.pointwise.W - w.sum()) <= 1e-12 * w.sum()
    Xs = X[:, :n_iter, :].reshape(D, -1)
    u = d._logits(Xs)                                                  # (n, C, states)
    lse, proba = d._lse(u)
    assert np.array_equal(proba, d.predict_proba(Xs))
    ll = np.take_along_axis(u, d.targets[:, None, None], axis=1)[:, 0] - lse
    ref = group_reference(d.W, d.b, d.q, C, n, Xs, rounded=False)      # the same functions from W; and the bound dU
    assert np.abs(ref[0] - ll).max() <= 1e-10 and np.abs(ref[1] - proba).max() <= 1e-12
    bars = group_bars(C, ll, proba, lse, ref[3], w)
    mean, sd, lme = flat_stats(ll, w)
    for name, got, want, bar in (('lppd_i', wa.lppd_i, lme, bars[0]), ('sqrt p_waic_i', np.sqrt(wa.p_waic_i), sd, bars[0]),
                                 ('p_waic_i', wa.p_waic_i, sd * sd, bars[0]), ('fitted', wa.fitted, flat_stats(proba, w)[0], bars[1])):
        ratio = worst(got, want, bar)
        print('softmax waic %s: worst error / bar = %.3f' % (name, ratio))
        assert ratio <= 2.0, (name, ratio)
