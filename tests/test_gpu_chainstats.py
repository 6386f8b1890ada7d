"""GPU: per-chain sums, their fold, R-hat and the multi-chain effective sample size (csrc/chainstats.hip,
DeviceChainStats, HMCBase.diagnostics).

Two arithmetic models, both stated where they are used:
  * the chain pass is a fixed sequence of IEEE float64 operations per element -- ``host_chain_sums`` below restates it
    in NumPy (whose elementwise float64 operations round once each and never fuse) and the comparison is ``==``;
  * the fold adds N terms per output in a fixed tree -- ``fold_depth`` restates its geometry, and the comparison is the
    summation bound  depth * 2^-53 * sum |terms|  against the same sums taken in numpy.longdouble."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
LD = np.longdouble


# ---------------------------------------------------------------------------------------------------------------------
# the NumPy restatement
# ---------------------------------------------------------------------------------------------------------------------
def host_chain_sums(X, w, c, start=None):
    """X (D, n, N) float64 states, w (n, N) weights, c (D,) shift, start = (a0, a1, a2) stored sums or None.  The chain
    pass's operation order, one IEEE float64 operation per line and element, k ascending:
        t = x - c;  u = w * t;  a1 = a1 + u;  a2 = a2 + u * t;  a0 = a0 + w"""
    D, n, N = X.shape
    a0, a1, a2 = (np.zeros(N), np.zeros((D, N)), np.zeros((D, N))) if start is None else [a.copy() for a in start]
    for k in range(n):
        t = X[:, k, :] - c[:, None]
        u = w[k][None, :] * t
        a1 = a1 + u
        p = u * t
        a2 = a2 + p
        a0 = a0 + w[k]
    return a0, a1, a2


def fold_depth(N, D):
    """Additions a term passes through in the fold (chainstats.hpp: ChainFoldPlan): a workgroup is cw column lanes x rw =
    256 / cw row lanes, gx workgroups share the chains.  A term is added into its row lane's running sum (that sum takes
    ceil(N / (gx rw)) terms), the rw row-lane sums of a workgroup are added in order, the finish kernel's lane adds
    ceil(gx / 16) workgroup sums and its 16 lane sums are added in order."""
    cw = 1
    while cw < min(D, 256):
        cw *= 2
    cw = min(cw, 256)
    gy = (D + cw - 1) // cw
    rw = 256 // cw
    gx = max(1, min(max(1, 1024 // gy), (N + rw * 4 - 1) // (rw * 4)))
    return (N + gx * rw - 1) // (gx * rw) + rw + (gx + 15) // 16 + 16


def host_fold(a0, a1, a2):
    """the fold's sums in numpy.longdouble from the per-chain sums, and per output the sum of |terms| its error bound is
    made of.  Terms: a0; m = a1 / a0 (one rounding on the device); m^2 (three); v = a2 / a0 - m^2, whose roundings are
    relative to the operands of the subtraction, u (|a2 / a0| + 3 m^2 + |v|) <= 4 u (|a2 / a0| + m^2): the operands, not
    the difference, are the terms of Sv's bound."""
    a0l, a1l, a2l = a0.astype(LD), a1.astype(LD), a2.astype(LD)
    m = a1l / a0l
    q = a2l / a0l
    v = q - m * m
    sums = (a0l.sum(), m.sum(axis=1), (m * m).sum(axis=1), v.sum(axis=1))
    absum = (np.abs(a0l).sum(), np.abs(m).sum(axis=1), (m * m).sum(axis=1), (np.abs(q) + m * m).sum(axis=1))
    return sums, absum


def assert_fold_within_bound(dev, a0, a1, a2, tag, extra_depth=0):
    """dev = (Sw, Sm, Sq, Sv) of the device; bound (A + 4) * 2^-53 * sum |terms| with A = fold_depth: A additions on the
    way into the sum, at most 4 roundings in the term itself (host_fold)."""
    D, N = a1.shape
    A = fold_depth(N, D) + extra_depth
    host, absum = host_fold(a0, a1, a2)
    for name, d, h, a in zip(('Sw', 'Sm', 'Sq', 'Sv'), dev, host, absum):
        err = np.abs(np.asarray(d).astype(LD) - h)
        bound = (A + 4) * LD(U) * a
        worst = float(np.max(err / np.where(bound > 0, bound, 1)))
        print('%s %s: depth %d, max |device - host| / bound = %.3g' % (tag, name, A, worst))
        assert np.all(np.isfinite(np.asarray(d))) and np.all(err <= bound), (tag, name, worst)


def record(s, n):
    """n + lead recorded iterations: states (D, n + lead, N), weights of the states 0 .. n - 1 (n, N), dwell slot of the
    first weight (-1: unit weights)"""
    dev = s._dev
    lead = 1 if s._dwell_weighted else 0
    dev.ring_alloc(n + lead)
    s._run(n + lead, ring_slot0=0)
    s._publish()
    X = dev.ring_read(0, n + lead).reshape(dev.ndims, n + lead, dev.nparticles)
    w = dev.ring_read_dwell(0, n + lead)[1:n + 1] if lead else np.ones((n, dev.nparticles))
    return X, w, (1 if lead else -1)


def _iso(D, N, seed, cls=None):
    from mjhmc_amd.misc.distributions import TestGaussian
    from mjhmc_amd.samplers import markov_jump_hmc as mj
    X0 = np.random.RandomState(seed).randn(D, N) * 1.3 + 0.5

    class Fixed(TestGaussian):
        def gen_init_X(self):
            self.Xinit = X0
    kw = dict(resample=False) if cls in (None, 'MarkovJumpHMC') else {}
    return getattr(mj, cls or 'MarkovJumpHMC')(distribution=Fixed(ndims=D, nbatch=N, sigma=1.3), epsilon=0.3, beta=0.3,
                                               num_leapfrog_steps=5, seed=11, **kw)


def _pot32():
    from mjhmc_amd.misc.distributions import ProductOfT
    from mjhmc_amd.samplers.markov_jump_hmc import MarkovJumpHMC
    rs = np.random.RandomState(8)
    D, N = 36, 120
    sp = rs.rand(D, D)
    W = rs.randn(D, D)
    W[sp > 0.05] = 0
    W += np.eye(D)
    lognu = np.log(rs.rand(D) * 2 + 2.1)
    X0 = rs.randn(D, N)

    class FixedT(ProductOfT):
        def gen_init_X(self):
            self.Xinit = X0
    d = FixedT(ndims=D, nbasis=D, nbatch=N, lognu=lognu, W=W, state_dtype='float32')
    return MarkovJumpHMC(distribution=d, epsilon=0.1, beta=0.3, num_leapfrog_steps=6, seed=99, resample=False)


def _sic_bf16():
    from mjhmc_amd.misc.distributions import SparseImageCode
    from mjhmc_amd.samplers.markov_jump_hmc import MarkovJumpHMC
    from tests.helpers import sic_problem
    B, imgs, a0 = sic_problem(3, n_patches=1, n_coeffs=512)
    N = 40
    X0 = a0[:, None] + 0.3 * np.random.RandomState(8).randn(512, N)
    d = SparseImageCode(n_patches=1, n_batches=N, cauchy=True, n_basis=512, basis=B, imgs=imgs, init=X0, state_dtype='bfloat16')
    return MarkovJumpHMC(distribution=d, epsilon=0.0625, beta=0.3, num_leapfrog_steps=6, seed=3, resample=False)


CASES = {
    'iso2x1000_f64': (lambda: _iso(2, 1000, 1), 9),             # one 16-byte chunk per row; N not a multiple of 64
    'iso33x100_f64': (lambda: _iso(33, 100, 1), 6),             # row padding (pitch 34): 17 chunks, not a power of two
    'iso512x333_f64': (lambda: _iso(512, 333, 2), 5),
    'iso33x100_control': (lambda: _iso(33, 100, 4, 'ControlHMC'), 7),   # a discrete-time sampler
    'pot36_f32': (_pot32, 5),
    'sic512_bf16': (_sic_bf16, 6),
}


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------------------------
# 1. + 2.  the definition, bit for bit, and its independence of the blocks
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', sorted(CASES))
def test_definition_bit_for_bit(case):
    """read_chains == the sequential NumPy restatement on every element: both pairings (dwell slot s + 1 where the
    sampler has dwelling times, unit weights) and a non-zero shift."""
    make, n = CASES[case]
    s = make()
    X, w, w_slot0 = record(s, n)
    D, N = s._dev.ndims, s._dev.nparticles
    assert N % 64 != 0 and np.all(np.isfinite(w)) and np.all(w > 0)
    c = X[:, 0, :].mean(axis=1) + 0.37 * np.cos(np.arange(D))
    cs = s._dev.chain_stats(1)
    pairings = [('unit', -1, np.ones((n, N)))] + ([('dwell s+1', w_slot0, w)] if w_slot0 >= 0 else [])
    for name, slot0, wt in pairings:
        for shift in (c, np.zeros(D)):
            cs.reset()
            cs.set_shift(shift)
            cs.accumulate(0, n, w_slot0=slot0)
            got = cs.read_chains()
            want = host_chain_sums(X[:, :n, :], wt, shift)
            for what, g, h in zip(('a0', 'a1', 'a2'), got, want):
                assert g.shape == h.shape
                bad = int(np.sum(g != h))
                assert bad == 0, '%s %s %s: %d of %d elements differ' % (case, name, what, bad, h.size)
    cs.close()


@pytest.mark.parametrize('case', ['iso33x100_f64', 'sic512_bf16', 'iso33x100_control'])
def test_block_independence(case):
    """one block, blocks of one slot, an uneven cut: the same per-chain sums bit for bit"""
    make, n = CASES[case]
    s = make()
    X, w, w_slot0 = record(s, n)
    cs = s._dev.chain_stats(2)
    cs.set_shift(np.linspace(-0.5, 0.5, s._dev.ndims))
    results = []
    for cuts in ([n], [1] * n, [2, 1, n - 3]):
        cs.reset()
        at = 0
        for k in cuts:
            cs.accumulate(at, k, w_slot0=(at + 1 if w_slot0 >= 0 else -1), part=1)
            at += k
        results.append(cs.read_chains(1))
        assert cs.read(1)[:2] == (s._dev.nparticles, n)
        assert not np.any(cs.read_chains(0)[0]), 'part 0 was never given anything'
    assert _same(results[0], results[1]) and _same(results[0], results[2])
    assert _same(results[0], host_chain_sums(X[:, :n, :], w, np.linspace(-0.5, 0.5, s._dev.ndims)))


# ---------------------------------------------------------------------------------------------------------------------
# 3.  the fold
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['iso2x1000_f64', 'iso33x100_f64', 'iso512x333_f64', 'pot36_f32'])
def test_fold_against_extended_precision(case):
    make, n = CASES[case]
    s = make()
    X, w, w_slot0 = record(s, n)
    cs = s._dev.chain_stats(1)
    cs.set_shift(X[:, 0, :].mean(axis=1))
    cs.accumulate(0, n, w_slot0=w_slot0)
    M, n_per, Sw, Sm, Sq, Sv = cs.read()
    assert (M, n_per) == (s._dev.nparticles, n)
    assert_fold_within_bound((Sw, Sm, Sq, Sv), *cs.read_chains(), tag=case)


def test_fold_is_bit_identical_from_run_to_run():
    out = []
    for _ in range(2):
        s = _iso(70, 3000, 4)
        s._dev.ring_alloc(7)
        s._run(7, ring_slot0=0)
        cs = s._dev.chain_stats(2)
        cs.set_shift(np.linspace(-1, 1, 70))
        cs.accumulate(0, 3, w_slot0=1, part=0)
        cs.accumulate(3, 3, w_slot0=4, part=1)
        out.append(cs.read(0)[2:] + cs.read(1)[2:])
    assert _same(out[0], out[1])


def _synthetic(X, n_parts=1, ring=None):
    """a sampler of the test build whose ring slots 0 .. n - 1 hold X (D, n, N) (mjhmc_test_ring_write)"""
    from mjhmc_amd import engine, _lib
    from tests.helpers import hooks_context
    ctx = hooks_context(0)
    D, n, N = X.shape
    en = engine.DeviceEnergy(ctx, _lib.E_ISO_GAUSS, D, [1.0])
    dev = engine.DeviceSampler(en, np.zeros((D, N)), seed=5, mode=_lib.MODE_MJHMC)
    dev.ring_alloc(ring or n)
    for k in range(n):
        block = np.ascontiguousarray(X[:, k, :])             # (kept alive across the call: the hook reads it)
        engine.check(ctx.lib.mjhmc_test_ring_write(dev.handle, k, block.ctypes.data), ctx.lib)
    assert np.array_equal(dev.ring_read(0, n).reshape(D, n, N), X)
    return ctx, dev


@pytest.mark.parametrize('N', [1, 65])
def test_padding_rows_do_not_contribute(N):
    """N = 1 and N = 65 leave 63 padding rows whose sums are zero: a fold that read them would divide by zero"""
    rs = np.random.RandomState(N)
    D, n = 5, 4
    X = rs.randn(D, n, N) + 2.0
    ctx, dev = _synthetic(X)
    cs = dev.chain_stats(1)
    cs.accumulate(0, n, w_slot0=-1)
    chains = cs.read_chains()
    assert _same(chains, host_chain_sums(X, np.ones((n, N)), np.zeros(D)))
    M, n_per, Sw, Sm, Sq, Sv = cs.read()
    assert (M, n_per, Sw) == (N, n, float(N * n))
    assert_fold_within_bound((Sw, Sm, Sq, Sv), *chains, tag='padding N=%d' % N)


# ---------------------------------------------------------------------------------------------------------------------
# 4.  a known answer
# ---------------------------------------------------------------------------------------------------------------------
def _direct_diagnostics(X, w, n_parts):
    """every field of Diagnostics straight from the data (X (D, n, N), w (n, N)), in numpy.longdouble, chains cut into
    n_parts pieces: the plain definitions, no sums about a shift"""
    D, n, N = X.shape
    h = n // n_parts
    Xc = np.concatenate([X[:, i * h:(i + 1) * h, :] for i in range(n_parts)], axis=2).astype(LD)    # (D, h, M)
    wc = np.concatenate([w[i * h:(i + 1) * h, :] for i in range(n_parts)], axis=1).astype(LD)       # (h, M)
    M = N * n_parts
    a0 = wc.sum(axis=0)
    m = (wc * Xc).sum(axis=1) / a0
    v = (wc * (Xc - m[:, None, :]) ** 2).sum(axis=1) / a0
    avg = m.mean(axis=1)
    between = ((m - avg[:, None]) ** 2).sum(axis=1) / (M - 1)
    within = v.mean(axis=1)
    var_plus = within + between
    return dict(n_chains=M, n_states=h, total_weight=a0.sum(), mean=avg, between=between, within=within, var_plus=var_plus,
                rhat=np.sqrt((h - LD(1)) / h * var_plus / within), ess_per_chain=var_plus / between,
                ess=M * var_plus / between), np.abs(m).sum(axis=1)


def _assert_fields(d, want, sum_abs_m, tag):
    """1e-12 relative on every field, except the two that are a sum of terms of both signs divided by M: the mean of the
    chain means (and ``mean`` = shift + it) can be arbitrarily small against its terms, so they get the fold's own bound
    (depth + 4) 2^-53 sum |m| / M, plus two roundings of the result -- the derived bound, larger than 1e-12 relative."""
    M, D = d.n_chains, d.mean.size
    A = fold_depth(M // len(d.parts), D) + len(d.parts)
    assert (d.n_chains, d.n_states) == (want['n_chains'], want['n_states'])
    assert abs(d.total_weight - want['total_weight']) <= 1e-12 * want['total_weight']
    for name in ('between', 'within', 'var_plus', 'rhat', 'ess_per_chain', 'ess'):
        got, w = getattr(d, name), want[name]
        rel = float(np.max(np.abs(got.astype(LD) - w) / np.abs(w)))
        print('%s %-14s max relative difference %.3g' % (tag, name, rel))
        assert rel <= 1e-12, (tag, name, rel)
    bound = (A + 4) * LD(U) * sum_abs_m / M + 2 * LD(U) * np.abs(want['mean'])      # (the division by M, the shift's addition)
    for name, got in (('mean', d.mean), ('chain_mean_avg + shift', d.chain_mean_avg + d.shift)):
        err = np.abs(got.astype(LD) - want['mean'])
        print('%s %-14s max |difference| / derived bound %.3g' % (tag, name, float(np.max(err / bound))))
        assert np.all(err <= bound), (tag, name)
    assert np.array_equal(d.ess_per_grad, d.ess / d.grad_evals)


def test_known_answer_ar1_with_negative_control():
    """AR(1) chains x_{k+1} = rho x_k + sqrt(1 - rho^2) e, stationary, unit variance: exactly
        Var(chain mean) = (1 / n) (1 + 2 sum_{k=1}^{n-1} (1 - k / n) rho^k)
    and ess_per_chain estimates 1 / Var(chain mean) with relative standard error sqrt(2 / (M - 1)): M = 16 384 chains,
    bound 5 sigma = 5.5 %.  Negative control: + 1.0 (one standard deviation) on every state of the first half of the
    chains must push R-hat above 1.1 in every dimension (NumPy over 5 seeds: 1.143 .. 1.146 plain, 1.170 .. 1.173 split,
    against 1.02 without the offset)."""
    from mjhmc_amd.samplers.markov_jump_hmc import Diagnostics
    M, n, D, rho = 16384, 64, 4, 0.6
    rs = np.random.RandomState(20260)
    X = np.empty((D, n, M))
    X[:, 0, :] = rs.randn(D, M)
    for k in range(1, n):
        X[:, k, :] = rho * X[:, k - 1, :] + np.sqrt(1 - rho * rho) * rs.randn(D, M)
    w = np.ones((n, M))

    def var_of_mean(h):
        k = np.arange(1, h)
        return (1.0 + 2.0 * np.sum((1.0 - k / float(h)) * rho ** k)) / h

    for offset in (0.0, 1.0):
        Xo = X.copy()
        Xo[:, :, :M // 2] += offset
        ctx, dev = _synthetic(Xo)
        data = dev.ring_read(0, n).reshape(D, n, M)
        for n_parts in (1, 2):
            cs = dev.chain_stats(n_parts)
            h = n // n_parts
            for part in range(n_parts):
                cs.accumulate(part * h, h, w_slot0=-1, part=part)
            d = Diagnostics([cs.read(part) for part in range(n_parts)], np.zeros(D), grad_evals=M * n)
            cs.close()
            tag = 'AR(1) offset %.0f %s' % (offset, 'split' if n_parts == 2 else 'plain')
            want, sum_abs_m = _direct_diagnostics(data, w, n_parts)
            _assert_fields(d, want, sum_abs_m, tag)
            print('%s: rhat %s, ess_per_chain %s (exact %.4f)' % (tag, d.rhat, d.ess_per_chain, 1.0 / var_of_mean(h)))
            if offset == 0.0:
                rel = np.abs(d.ess_per_chain * var_of_mean(h) - 1.0)
                assert np.all(rel <= 5.0 * np.sqrt(2.0 / (M - 1))), (tag, rel)
                assert np.all(d.rhat < 1.1)
            else:
                assert np.all(d.rhat > 1.1), (tag, d.rhat)


# ---------------------------------------------------------------------------------------------------------------------
# 5.  the driver
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cls', ['MarkovJumpHMC', 'ControlHMC'])
def test_driver_leaves_the_sampler_as_expectations_does(cls):
    """diagnostics(30, block=7): halves of 15 states in blocks of 7, 7, 1 (three per half).  Counters, dwelling times,
    final state and RNG tick as expectations(30) from the same seed; the sums of each half equal a one-block manual
    accumulation over the same run recorded in one ring, bit for bit (same chain sums, same fold)."""
    n_iter, D, N = 30, 24, 301
    s = _iso(D, N, 5, cls)
    tick0, grad0 = s._dev.get_tick(), s.distribution.dEdX_count
    for kwargs in (dict(n_iter=5), dict(n_iter=2), dict(n_iter=1, split=False), dict(n_iter=8, shift=np.zeros(D + 1))):
        with pytest.raises(ValueError):
            s.diagnostics(**kwargs)
    assert (s._dev.get_tick(), s._dev.ring_slots, s.distribution.dEdX_count) == (tick0, 0, grad0)
    shift = None if cls == 'MarkovJumpHMC' else np.full(D, 0.25)
    d = s.diagnostics(n_iter, split=True, block=7, shift=shift)
    lead = 1 if s._dwell_weighted else 0
    assert s._dev.get_tick() - tick0 == n_iter + lead
    assert d.grad_evals == s.distribution.dEdX_count - grad0 and d.grad_evals > 0
    assert (d.n_chains, d.n_states) == (2 * N, n_iter // 2)
    assert np.array_equal(d.ess_per_grad, d.ess / d.grad_evals)
    ref = _iso(D, N, 5, cls)
    ref.expectations(n_iter, block=11, shift=np.zeros(D))
    assert (s.l_count, s.f_count, s.r_count, s.fl_count) == (ref.l_count, ref.f_count, ref.r_count, ref.fl_count)
    assert (s.distribution.E_count, s.distribution.dEdX_count) == (ref.distribution.E_count, ref.distribution.dEdX_count)
    assert np.array_equal(s.state.X, ref.state.X) and np.array_equal(s.state.V, ref.state.V)
    assert s._dev.get_tick() == ref._dev.get_tick()
    if lead:
        assert np.array_equal(s.dwelling_times, ref.dwelling_times)
    # the same run in one ring
    m = _iso(D, N, 5, cls)
    X, w, w_slot0 = record(m, n_iter)
    h = n_iter // 2
    if shift is None:                                    # the pooled (weighted) mean of the first block of 7 states
        pooled = (w[:7][None] * X[:, :7, :]).sum(axis=(1, 2)) / w[:7].sum()
        assert np.allclose(d.shift, pooled, rtol=0, atol=1e-12) and np.any(d.shift != 0)
    cs = m._dev.chain_stats(2)
    cs.set_shift(d.shift)
    cs.accumulate(0, h, w_slot0=w_slot0, part=0)
    cs.accumulate(h, h, w_slot0=(h + 1 if lead else -1), part=1)
    for part in range(2):
        got, want = d.parts[part], cs.read(part)
        assert got[:3] == want[:3] and _same(got[3:], want[3:]), part
        assert _same(cs.read_chains(part), host_chain_sums(X[:, part * h:(part + 1) * h, :], w[part * h:(part + 1) * h], d.shift))
    # unsplit, whole chains, default block
    u = _iso(D, N, 5, cls)
    du = u.diagnostics(n_iter, split=False, shift=d.shift)
    assert (du.n_chains, du.n_states) == (N, n_iter) and u._dev.get_tick() == s._dev.get_tick()
    whole = host_chain_sums(X[:, :n_iter, :], w, d.shift)
    assert_fold_within_bound((du.Sw, du.Sm, du.Sq, du.Sv), *whole, tag='driver unsplit ' + cls)
    assert np.all(du.rhat > 0.9) and np.all(du.ess > 0)


# ---------------------------------------------------------------------------------------------------------------------
# 6.  failure paths
# ---------------------------------------------------------------------------------------------------------------------
def test_infinite_dwell_raises_and_adds_nothing():
    """a zero total rate leaves an infinite dwelling time in the dwell ring (written here through the test build's hook)"""
    from mjhmc_amd import engine, _lib
    from tests.helpers import hooks_context
    ctx = hooks_context(0)
    D, N = 12, 70
    en = engine.DeviceEnergy(ctx, _lib.E_ISO_GAUSS, D, [1.0])
    dev = engine.DeviceSampler(en, np.random.RandomState(0).randn(D, N), seed=5, mode=_lib.MODE_MJHMC)
    dev.set_hparams(0.2, 5, 0.18, 1.0, 0.5)
    dev.ring_alloc(5)
    dev.iterate(5, ring_slot0=0)
    X = dev.ring_read(0, 5).reshape(D, 5, N)
    dwell = dev.ring_read_dwell(0, 5)
    cs = dev.chain_stats(1)
    cs.accumulate(0, 2, w_slot0=1)
    before = cs.read_chains()
    engine.check(ctx.lib.mjhmc_test_ring_write_dwell(dev.handle, 3, 17, float('inf')), ctx.lib)
    with pytest.raises(_lib.EngineError, match='not finite'):
        cs.accumulate(2, 2, w_slot0=3)
    assert ctx.lib.mjhmc_chainstats_accumulate(cs.handle, 0, 2, 3, 2) == _lib.ERR_NONFINITE
    assert _same(before, cs.read_chains()) and cs.read()[1] == 2
    engine.check(ctx.lib.mjhmc_test_ring_write_dwell(dev.handle, 3, 17, float(dwell[3, 17])), ctx.lib)
    cs.accumulate(2, 2, w_slot0=3)                                  # the flag does not stick: the finite block adds normally
    assert _same(cs.read_chains(), host_chain_sums(X[:, :4, :], dwell[1:5], np.zeros(D))) and cs.read()[1] == 4


def test_invalid_arguments():
    from mjhmc_amd._lib import EngineError
    s = _iso(33, 100, 1)
    dev = s._dev
    with pytest.raises(EngineError, match='no sample ring'):
        dev.chain_stats(1)
    dev.ring_alloc(4)
    s._run(4, ring_slot0=0)
    for n_parts in (0, 3):
        with pytest.raises(EngineError, match='n_parts must be 1 or 2'):
            dev.chain_stats(n_parts)
    cs = dev.chain_stats(2)
    for args, msg in (((0, 5, -1, 0), 'outside the ring'), ((3, 2, -1, 0), 'outside the ring'), ((-1, 1, -1, 0), 'outside the ring'),
                      ((0, 4, 1, 0), 'dwell slots'), ((0, 1, -2, 0), 'dwell slots'), ((0, 0, -1, 0), 'n must be >= 1'),
                      ((0, 1, -1, 2), r'part 2 is outside \[0, 2\)'), ((0, 1, -1, -1), 'part -1 is outside')):
        with pytest.raises(EngineError, match=msg):
            cs.accumulate(args[0], args[1], w_slot0=args[2], part=args[3])
    with pytest.raises(EngineError, match='nothing has been added'):
        cs.read(1)
    with pytest.raises(EngineError, match='is outside'):
        cs.read_chains(2)
    assert not np.any(cs.read_chains(0)[1])
    cs.accumulate(0, 3, w_slot0=1, part=1)
    with pytest.raises(EngineError, match='reset first'):
        cs.set_shift(np.ones(33))
    with pytest.raises(ValueError):
        cs.set_shift(np.ones(5))
    cs.reset()
    cs.set_shift(np.ones(33))
    dev.ring_alloc(9)                                               # a new ring: the sums were created on the old one
    with pytest.raises(EngineError, match='re-allocated'):
        cs.accumulate(0, 1)
    assert dev.lib.mjhmc_chainstats_accumulate(cs.handle, 0, 0, -1, 1) == -1
    cs.close()
    alive = dev.chain_stats(1)
    dev.close()                                                     # the sampler frees what is still alive on it
    alive.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7.  column shards on one GPU (the way test_gpu_sharded.py runs them)
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


# rank-dependent arguments: rank 0's shift must win, and the ranks must agree on the smallest block
for shift, block in ((None, 4 + 3 * comm.rank), (np.full(D, 0.1) * (comm.rank + 1), 9 - 4 * comm.rank), (None, None)):
    s = make(comm)
    t0 = s._dev.get_tick()
    d = s.diagnostics(n_iter, split=True, block=block, shift=shift)
    assert s._dev.get_tick() - t0 == n_iter + 1, 'a rank ran more than the 21 iterations (a replayed or retried block)'
    both = comm.allreduce_f64(np.concatenate([d.shift, -d.shift]), 'max')
    assert np.array_equal(both[:D], -both[D:]), 'the shards used different shifts'
    if shift is not None:
        assert np.array_equal(d.shift, np.full(D, 0.1))
    assert d.n_chains == 2 * N and d.n_states == n_iter // 2
    assert [p[0] for p in d.parts] == [N, N]
    if comm.rank == 0:
        from tests.test_gpu_chainstats import host_chain_sums, assert_fold_within_bound, record, fold_depth
        s1 = make(None)
        d1 = s1.diagnostics(n_iter, split=True, block=6, shift=d.shift)
        assert d1.n_chains == d.n_chains
        # the unsharded run recorded in one ring: its per-chain sums are the terms of both folds.  A shard's fold is at
        # most as deep as the whole run's (fewer chains, same columns); adding the two ranks is one more addition
        X, w, w_slot0 = record(make(None), n_iter)
        h = n_iter // 2
        assert max(fold_depth(150, D), fold_depth(151, D)) <= fold_depth(N, D)
        for part in range(2):
            chains = host_chain_sums(X[:, part * h:(part + 1) * h, :], w[part * h:(part + 1) * h], d.shift)
            assert_fold_within_bound(d.parts[part][2:], *chains, tag='sharded part %%d' %% part, extra_depth=1)
            assert_fold_within_bound(d1.parts[part][2:], *chains, tag='unsharded part %%d' %% part)
        assert np.allclose(d.rhat, d1.rhat, rtol=1e-12, atol=0) and np.allclose(d.ess, d1.ess, rtol=1e-10, atol=0)
        assert (s.l_count, s.f_count, s.r_count) == (s1.l_count, s1.f_count, s1.r_count)
        assert np.array_equal(s.dwelling_times, s1.dwelling_times)
    comm.barrier()
print('rank %%d ok' %% comm.rank)
'''


def test_sharded_sums_equal_unsharded(tmp_path):
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
