"""GPU: the data-row influence of linear models on the device (csrc/dense_lin_values.hpp, csrc/influence.hip,
mjhmc_influence_*, HMCBase.influence) against float64 NumPy restatements on the float32-rounded model and
states, on test_gpu_pointwise.py's own samplers.  Shapes are the smallest at which each failure can occur: block boundaries
of the experts, a partial last block, a partial second tile, an expert range that straddles blocks."""
import numpy as np
import pytest

from tests.test_gpu_pointwise import (FAMILY, GLM_N, SHAPES, dyadic_case, f32, family_sampler, gauss_glm, host_u,  # noqa: F401
                                      model, ring_sampler, u_case)

pytestmark = pytest.mark.gpu
np.seterr(all='ignore')

EPS = 2.0 ** -53
NAMES = ('W', 'Sx', 'S2x', 'St', 'S2t', 'n_states', 'Cxt')


def sums_of(dev, value, n, experts=None, w_slot0=-1, shift=None, x_slot0=0):
    """(W, Sx, S2x, St, S2t, n_states, Cxt) of one accumulate call on a fresh handle"""
    h = dev.influence(value, experts)
    if shift is not None:
        h.set_shift(*shift)
    h.accumulate(x_slot0, n, w_slot0=w_slot0)
    out = h.read() + (h.read_cross(),)
    h.close()
    return out


def same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def host_sums(X, t, w, cx, ct):
    """the sums restated in float64: X (D, n) states, t (J, n) values, w (n,) weights; rows of weight 0 selected out"""
    on = w > 0
    X, t, w = X[:, on], t[:, on], w[on]
    dx, dt = X - cx[:, None], t - ct[:, None]
    return (w.sum(), (w * dx).sum(axis=1), (w * dx * dx).sum(axis=1), (w * dt).sum(axis=1), (w * dt * dt).sum(axis=1),
            (w * X).dot(dt.T))


def quarter_weights(seed, shape, zeros=((0, 3), (0, 40))):
    w = np.random.RandomState(seed).randint(0, 33, size=shape) / 4.0
    for z in zeros:
        w[z] = 0.0
    return w


# ---------------------------------------------------------------------------------------------------------------------
# 1. exact structure
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('D,K', SHAPES)
def test_exact_structure(D, K, dtype):
    """X multiples of 2^-4 in [-4, 4], weights multiples of 1/4 in [0, 8] (some 0), value (float)(j % 7), integer ct, cx on
    the grid of X: every product and sum is exact in float64 in any order, so every sum equals the NumPy restatement bit
    for bit -- the global expert index across blocks, the mask of the last block, the rows beyond the batch (the second
    tile is partial), the weight-0 select"""
    W, b, _ = model(D, K, 'softplus')
    rs = np.random.RandomState(D + K)
    X = rs.randint(-64, 65, size=(D, 1, 45)) / 16.0
    w = quarter_weights(D, (1, 45))
    cx = rs.randint(-16, 17, size=D) / 16.0
    ct = (np.arange(K) % 3).astype(np.float64)
    _, dev = ring_sampler(W, b, X, dtype=dtype, w=w)
    got = sums_of(dev, '(float)(j % 7)', 1, w_slot0=0, shift=(cx, ct))
    t = np.repeat((np.arange(K) % 7).astype(np.float64)[:, None], 45, axis=1)
    want = host_sums(X[:, 0, :], t, w[0], cx, ct)
    assert got[5] == 45 and got[6].shape == (D, K)
    for name, g, h in zip(('W', 'Sx', 'S2x', 'St', 'S2t', 'Cxt'), got[:5] + (got[6],), want):
        assert np.array_equal(g, h), name
    assert np.any(got[6] != 0.0)
    dev.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. value u against the float64 restatement, a bar derived operation by operation
# ---------------------------------------------------------------------------------------------------------------------
def u_bar(X, w, u, du, ct):
    """(bar of Cxt (D, K), bar of St (K,)) for value u: the float32 error of u weighted as the sum weights it,
    sum_p w |x_pd| |du_pj|, plus the float64 accumulation of n = particles terms, each product formed from two rounded
    factors: (n + 2) 2^-53 sum_p w |x_pd| |t_pj - ct_j|, |t - ct| <= |u - ct| + du"""
    n = X.shape[1]
    dev = np.abs(u - ct[:, None]) + du
    cross = (w * np.abs(X)).dot(du.T) + (n + 2) * EPS * (w * np.abs(X)).dot(dev.T)
    first = (w * du).sum(axis=1) + (n + 2) * EPS * (w * dev).sum(axis=1)
    return cross, first


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('D,K', SHAPES)
def test_value_u_against_float64(D, K, dtype):
    W, b, X = u_case(D, K)
    w = quarter_weights(K, (1, 45))
    u, du = host_u(W, b, X[:, 0, :])
    ct = np.round(u.mean(axis=1))
    cx = np.zeros(D)
    _, dev = ring_sampler(W, b, X, dtype=dtype, w=w)
    got = sums_of(dev, 'u', 1, w_slot0=0, shift=(cx, ct))
    want = host_sums(X[:, 0, :], u, w[0], cx, ct)
    cross_bar, first_bar = u_bar(X[:, 0, :], w[0], u, du, ct)
    r_cross = float((np.abs(got[6] - want[5]) / cross_bar).max())
    r_first = float((np.abs(got[3] - want[3]) / first_bar).max())
    print('%dx%d %s value u: worst error / bar: Cxt %.4f, St %.4f' % (D, K, dtype, r_cross, r_first))
    assert got[0] == want[0] and got[5] == 45
    assert r_cross <= 1.0 and r_first <= 1.0
    # negative control: the same bar fails against a model with one row perturbed
    jbad = K // 2
    Wp = W.copy()
    Wp[jbad] = Wp[jbad] * (1 + 2.0 ** -6)
    up, _ = host_u(Wp, b, X[:, 0, :])
    wrong = host_sums(X[:, 0, :], up, w[0], cx, ct)
    assert (np.abs(got[6] - wrong[5]) / cross_bar)[:, jbad].max() > 1.0
    assert np.array_equal(np.delete(wrong[5], jbad, axis=1), np.delete(want[5], jbad, axis=1))
    dev.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. expert ranges and paged reads
# ---------------------------------------------------------------------------------------------------------------------
def test_expert_range_and_paged_read():
    D, K = 129, 640                                      # blocks of 256: [0, 256), [256, 512), [512, 640)
    W, b, X = u_case(D, K)
    w = quarter_weights(1, (1, 45))
    u, _ = host_u(W, b, X[:, 0, :])
    ct = np.round(u.mean(axis=1))
    cx = np.full(D, 0.25)
    _, dev = ring_sampler(W, b, X, w=w)
    with pytest.raises(ValueError, match='not a range'):
        dev.influence('u', (100, 700))
    for bad in ((-1, 5), (7, 7), (9, 3)):
        with pytest.raises(ValueError, match='not a range'):
            dev.influence('u', bad)
    full = sums_of(dev, 'u', 1, w_slot0=0, shift=(cx, ct))
    part = sums_of(dev, 'u', 1, experts=(100, 600), w_slot0=0, shift=(cx, ct[100:600]))
    assert part[6].shape == (D, 500)
    assert same_bits(part[:3], full[:3]) and part[5] == full[5]
    assert np.array_equal(part[3], full[3][100:600]) and np.array_equal(part[4], full[4][100:600])
    assert np.array_equal(part[6], full[6][:, 100:600])
    one = sums_of(dev, 'u', 1, experts=(511, 512), w_slot0=0, shift=(cx, ct[511:512]))      # the last column of a block
    assert np.array_equal(one[6], full[6][:, 511:512]) and np.array_equal(one[3], full[3][511:512])
    h = dev.influence('u', (100, 600))
    h.set_shift(cx, ct[100:600])
    h.accumulate(0, 1, w_slot0=0)
    assert h.experts == (100, 600) and h.panel_experts == 256 and h.ndims == D
    pages = [h.read_cross(a, min(a + 97, 600)) for a in range(100, 600, 97)]
    assert np.array_equal(np.concatenate(pages, axis=1), part[6])
    with pytest.raises(ValueError, match='columns'):
        h.read_cross(99, 200)
    with pytest.raises(ValueError, match='only while|reset first'):
        h.set_shift(cx, ct[100:600])                    # a shift after the first accumulate
    h.close()
    dev.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. determinism
# ---------------------------------------------------------------------------------------------------------------------
def raw(i):
    return (i.W, i.Sx, i.S2x, i.St, i.S2t, i.n_states, i.Cxt)


def test_bit_identical_across_runs_and_blocks():
    """FAMILY = (24, 700), 96 particles, holding-time weights: two runs agree bit for bit, and under a given shift so do
    block = 1, 2 and all -- every slot goes onto the totals separately"""
    def run(block, shift):
        s, _, _ = family_sampler()
        return s.influence(6, value='u', block=block, shift=shift)
    a, a2 = run(None, None), run(None, None)
    assert a.n_states == 6 * 96 and a.cov.shape == FAMILY and np.isfinite(a.cov).all() and np.any(a.cov != 0)
    assert same_bits(raw(a), raw(a2)) and np.array_equal(a.ct, a2.ct)
    shift = (a.cx, a.ct)
    b0, b1, b2 = run(None, shift), run(1, shift), run(2, shift)
    assert same_bits(raw(a), raw(b0))                    # block = all under the first block's own means is the default run
    assert same_bits(raw(b0), raw(b1)) and same_bits(raw(b0), raw(b2))
    s, _, _ = family_sampler(N=45)                       # the control: other particles give other sums
    small = s.influence(6, value='u', shift=shift)
    assert small.n_states == 6 * 45 and not np.array_equal(small.St, a.St)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the shift; the pointwise pass and the estimator on the same states
# ---------------------------------------------------------------------------------------------------------------------
def test_shift_and_the_other_passes():
    from mjhmc_amd.samplers.markov_jump_hmc import Influence, PointwiseStatistics
    D, K = 10, 513
    W, b, X = u_case(D, K)
    x = X[:, 0, :]
    w = quarter_weights(5, (1, 45))
    u, du = host_u(W, b, x)
    n = x.shape[1]
    Wsum = w.sum()
    mean_u = (w[0] * u).sum(axis=1) / Wsum
    cx = np.zeros(D)
    cta, ctb = np.round(mean_u), np.round(mean_u) + 3.0
    _, dev = ring_sampler(W, b, X, w=w)
    infs = []
    for ct in (cta, ctb):
        got = sums_of(dev, 'u', 1, w_slot0=0, shift=(cx, ct))
        infs.append(Influence(got[0], got[1], got[2], got[3], got[4], got[6], got[5], (0, K), cx, ct))
    ia, ib = infs
    mx = np.abs(ia.mean_x)

    def cov_bar(ct):
        """cov = Cxt / W - mean_x (St / W): the float64 accumulation of the three sums Cxt, St and Sx (test 2's term for
        each, St and Sx weighted by the factor they are multiplied with) and four roundings of the final operations"""
        dev_t = np.abs(u - ct[:, None]) + du
        ax, at = (w[0] * np.abs(x)).sum(axis=1), (w[0] * dev_t).sum(axis=1)       # sum w |x|, sum w |t - ct|
        big = (w[0] * np.abs(x)).dot(dev_t.T) + np.outer(mx, at) + np.outer(ax, at) / Wsum
        return ((n + 2) * EPS * big + 4 * EPS * big) / Wsum
    ratio = float((np.abs(ia.cov - ib.cov) / (cov_bar(cta) + cov_bar(ctb))).max())
    print('shift: worst |cov_a - cov_b| / bar = %.4f' % ratio)
    assert ratio <= 1.0
    assert not np.array_equal(ia.Cxt, ib.Cxt)
    # mean and variance of t against the pointwise pass on the same states: the same float32 values, other float64 sums
    pw = dev.pointwise(['u'], [False])
    pw.accumulate(0, 1, w_slot0=0)
    p = PointwiseStatistics(*(pw.read() + ([False],)))
    pw.close()
    t_abs = np.abs(u) + du
    m1 = (w[0] * t_abs).sum(axis=1) / Wsum                # mean |t|
    m2 = (w[0] * t_abs * t_abs).sum(axis=1) / Wsum        # mean t^2
    for inf, ct in ((ia, cta), (ib, ctb)):
        d1 = (w[0] * (np.abs(u - ct[:, None]) + du)).sum(axis=1) / Wsum
        d2 = (w[0] * (np.abs(u - ct[:, None]) + du) ** 2).sum(axis=1) / Wsum
        mean_bar = (n + 2) * EPS * (m1 + d1) + 3 * EPS * (m1 + np.abs(ct))
        # var = S2 / W - m^2 on both sides: the sums' accumulation, the square of a mean with error e: 2 |m| e, three roundings
        e_pw, e_in = (n + 2) * EPS * m1, (n + 2) * EPS * d1
        var_bar = (n + 3) * EPS * (m2 + d2) + 2 * m1 * e_pw + 2 * d1 * e_in + 3 * EPS * (m2 + d2)
        r_mean = float((np.abs(inf.mean_t - p.mean[0]) / mean_bar).max())
        r_var = float((np.abs(inf.var_t - p.var[0]) / var_bar).max())
        print('shift: mean_t against pointwise %.4f of the bar, var_t %.4f' % (r_mean, r_var))
        assert r_mean <= 1.0 and r_var <= 1.0
    est = dev.estimator(False)
    est.accumulate(0, 1, w_slot0=0)
    We, S1e, S2e = est.read()[:3]
    est.close()
    assert ia.W == We == Wsum and np.array_equal(ia.Sx, S1e) and np.array_equal(ia.S2x, S2e)
    dev.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. a particle of weight zero; 7. a value that is not finite
# ---------------------------------------------------------------------------------------------------------------------
NAN_ABOVE = 'u > 1000.f ? logf(-1.f) : u'


def test_a_particle_of_weight_zero_with_a_nan_value_changes_nothing():
    W, b, X = dyadic_case()
    w = np.random.RandomState(3).randint(1, 9, size=(2, 70)) / 4.0
    w[0, 13] = 0.0
    Xh = X.copy()
    Xh[:, 0, 13] = 2.0 ** 20                              # u = 2^20 sum_d W_jd + ...: NaN values at half of the experts
    assert (W.sum(axis=1) * 2.0 ** 20 > 2000).sum() > 100
    ct = np.zeros(513)
    cx = np.full(10, 0.125)
    for dtype in ('float64', 'float32'):
        _, d1 = ring_sampler(W, b, X, dtype=dtype, w=w)
        _, d2 = ring_sampler(W, b, Xh, dtype=dtype, w=w)
        s1 = sums_of(d1, NAN_ABOVE, 2, w_slot0=0, shift=(cx, ct))
        s2 = sums_of(d2, NAN_ABOVE, 2, w_slot0=0, shift=(cx, ct))
        assert same_bits(s1, s2), dtype
        assert s1[0] == w.sum() and np.isfinite(s2[6]).all()
        u = W.dot(X.reshape(10, -1)) + b[:, None]
        want = host_sums(X.reshape(10, -1), u, w.reshape(-1), cx, ct)         # dyadic: every sum is exact
        assert np.array_equal(s1[6], want[5]) and np.array_equal(s1[3], want[3]) and np.array_equal(s1[4], want[4])
        d1.close()
        d2.close()


def test_a_value_that_is_not_finite_refuses_until_reset():
    from mjhmc_amd import _lib, engine
    W, b, X = dyadic_case()
    Xh = X.copy()
    Xh[:, 1, 13] = 2.0 ** 20                              # slot 1 holds the state whose values are NaN; slot 0 is ordinary
    w = np.ones((2, 70))
    ctx, dev = ring_sampler(W, b, Xh, w=w)
    u1 = W.dot(Xh[:, 1, 13]) + b
    lowest = int(np.argmax(u1 > 1000))
    assert u1[lowest] > 2000 and not np.any((u1[:lowest] > 900))
    shift = (np.zeros(10), np.zeros(513))
    fresh = sums_of(dev, NAN_ABOVE, 1, w_slot0=0, shift=shift)
    h = dev.influence(NAN_ABOVE)
    h.set_shift(*shift)
    with pytest.raises(_lib.EngineError) as err:
        h.accumulate(0, 2, w_slot0=0)
    assert 'expert %d ' % lowest in str(err.value) and 'status -5' in str(err.value)
    with pytest.raises(_lib.EngineError, match='reset first'):
        h.accumulate(0, 1, w_slot0=0)
    h.reset()
    h.accumulate(0, 1, w_slot0=0)
    assert same_bits(h.read() + (h.read_cross(),), fresh)
    # a refused weight adds nothing and the handle goes on
    engine.check(ctx.lib.mjhmc_test_ring_write_dwell(dev.handle, 1, 5, -1.0), ctx.lib)
    with pytest.raises(_lib.EngineError, match='negative or not finite'):
        h.accumulate(0, 2, w_slot0=0)
    assert same_bits(h.read() + (h.read_cross(),), fresh)
    h.accumulate(0, 1, w_slot0=0)
    assert h.read()[0] == 2 * fresh[0] and np.array_equal(h.read_cross(), 2 * fresh[6])
    dev.close()                                           # a closed sampler has freed the handles
    h.close()


# ---------------------------------------------------------------------------------------------------------------------
# 8. other energies; the scratch does not grow with K
# ---------------------------------------------------------------------------------------------------------------------
def test_other_energies_are_refused_by_name():
    from mjhmc_amd import _lib
    from mjhmc_amd.misc.distributions import Funnel, ProductOfT
    from mjhmc_amd.samplers.markov_jump_hmc import HMC
    for dist, name in ((ProductOfT(ndims=36, nbasis=36, nbatch=40), 'PRODUCT_OF_T'), (Funnel(nbatch=40, ndims=10), 'FUNNEL_NEAL')):
        s = HMC(distribution=dist, epsilon=0.1, beta=0.3, num_leapfrog_steps=3, seed=1)
        before = (s.distribution.E_count, s.distribution.dEdX_count)
        with pytest.raises(ValueError, match=name):
            s.influence(3, value='u')
        assert (s.distribution.E_count, s.distribution.dEdX_count) == before
        s._dev.ring_alloc(2)
        with pytest.raises(_lib.EngineError, match='MJHMC_E_' + name):
            s._dev.influence('u')


def test_scratch_does_not_depend_on_the_number_of_experts():
    info = []
    for K in (513, 1100):
        W, b, _ = model(10, K, 'softplus')
        _, dev = ring_sampler(W, b, f32(np.zeros((10, 1, 45))))
        h = dev.influence('u')
        info.append((h.panel_experts, h.scratch_bytes, h.experts))
        h.close()
        dev.close()
    assert info[0][0] == info[1][0] == 128 and info[0][1] == info[1][1] > 0
    assert info[0][2] == (0, 513) and info[1][2] == (0, 1100)


# ---------------------------------------------------------------------------------------------------------------------
# 9. sampler level
# ---------------------------------------------------------------------------------------------------------------------
def test_the_run_is_that_of_expectations():
    s, W, b = family_sampler()
    inf = s.influence(6, value='u')
    t, _, _ = family_sampler()
    t.expectations(6)
    assert (s.l_count, s.f_count, s.r_count, s.fl_count) == (t.l_count, t.f_count, t.r_count, t.fl_count)
    assert (s.distribution.E_count, s.distribution.dEdX_count) == (t.distribution.E_count, t.distribution.dEdX_count)
    assert np.array_equal(s.state.X, t.state.X) and np.array_equal(s.state.V, t.state.V)
    assert np.array_equal(s.dwelling_times, t.dwelling_times)
    # the same run again at engine level: 7 iterations, the first 6 states weighted by the holding times the NEXT one drew
    r, _, _ = family_sampler()
    r._dev.ring_alloc(7)
    r._run(7, ring_slot0=0)
    got = sums_of(r._dev, 'u', 6, w_slot0=1, shift=(inf.cx, inf.ct))
    assert same_bits(got, raw(inf))
    dwell = r._dev.ring_read_dwell(0, 7)
    assert inf.n_states == 6 * 96 and abs(inf.W - dwell[1:7].sum()) <= 1e-12 * inf.W
    assert inf.experts == (0, FAMILY[1]) and inf.n_data is None


# ---------------------------------------------------------------------------------------------------------------------
# 10. the closed form of a Gaussian regression
# ---------------------------------------------------------------------------------------------------------------------
def glm_closed_form(d, mean, cov, widen=1.0):
    """Cov(x_d, l_j) and the exact standard error of its estimate from GLM_N independent draws x ~ N(mean, widen^2 cov),
    l_j = -u_j^2 / 2, u = W x + b.  With z = x - mean, v = w_j . z ~ N(0, s^2), r = W mean + b, c = (C w_j)_d:
    l - E l = -r v - (v^2 - s^2) / 2, so Cov(z_d, l_j) = -c r (Stein's lemma) and
    Var[z_d (l_j - E l_j)] = r^2 (C_dd s^2 + 2 c^2) + (2 C_dd s^4 + 8 c^2 s^2) / 4 - (c r)^2   (Isserlis)"""
    C = widen * widen * cov
    r = d.W.dot(mean) + d.b
    c = C.dot(d.W.T)                                      # (D, K)
    s2 = np.einsum('jd,de,je->j', d.W, C, d.W)
    Cdd = np.diag(C)[:, None]
    var = r * r * (Cdd * s2 + 2 * c * c) + 0.25 * (2 * Cdd * s2 * s2 + 8 * c * c * s2) - (c * r) ** 2
    return -c * r, np.sqrt(var / GLM_N)


def test_influence_against_the_closed_form():
    from mjhmc_amd.samplers.markov_jump_hmc import HMC
    d, mean, cov, eps = gauss_glm()
    s = HMC(distribution=d, epsilon=eps, beta=0.3, num_leapfrog_steps=8, seed=13)
    inf = s.influence(1)                # one recorded state of unit weight: 4096 posterior draws after a law-preserving step
    n = d.features.shape[0]
    assert inf.W == GLM_N and inf.cov.shape == (6, n + 6) and inf.n_data == n == d.n_data
    want, se = glm_closed_form(d, mean, cov)
    z = (inf.cov - want) / se
    wide, se_wide = glm_closed_form(d, mean, cov, widen=1.3)
    zw = (inf.cov - wide) / se_wide
    print('influence: max |z| of the %d entries %.2f; against a posterior 1.3 x too wide %.2f, %d entries beyond 6'
          % (z.size, np.abs(z).max(), np.abs(zw).max(), int((np.abs(zw) > 6).sum())))
    # for information: first-order case deletion against the exact refit, and the infinitesimal jackknife against cov
    P = d.W.T.dot(d.W)
    for j in list(inf.most_influential(2, precision=P)) + [0]:
        wj = d.W[j]
        refit = np.linalg.solve(P - np.outer(wj, wj), -(d.W.T.dot(d.b) - wj * d.b[j]))
        print('influence: row %4d  exact refit shift %s\n                     loo_shift        %s'
              % (j, np.array2string(refit - mean, precision=5), np.array2string(inf.loo_shift[:, j], precision=5)))
    print('influence: diag(ij_cov) / diag(cov) = %s' % np.array2string(np.diag(inf.ij_cov()) / np.diag(cov), precision=3))
    assert np.all(np.abs(z) <= 6)
    assert np.abs(zw).max() > 6
