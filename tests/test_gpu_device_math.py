"""The hand-written device math against long double: neg_log_unit, sincospi_unit, box_muller (csrc/philox.hpp),
box_muller_f32 (csrc/dense_pot.hpp), exp_normal / exp_any / exp_neg / exp_neg_k and jump_rate (csrc/jump_math.hpp),
called through the probe of the test build (csrc/device_math_probe.hip: the product's own inline functions, one lane per
element), and normal_pair's keying against oracle/philox.py.  References, measure and input sets: tests/device_math_ref.py
(checked against 200-bit mpmath by tests/test_device_math_cpu.py).  Every test prints its measured maximum (pytest -s).

Measured on an MI355X [gate]: neg_log_unit 0.715 ulp [2]; sincospi_unit 1.327 / 1.203 x 2^-53 [1.5], |s^2 + c^2 - 1| 1.896
x 2^-53 [4]; box_muller 2.485 x 2^-53 r [5]; box_muller_f32 1.468 x 2^-23 max(r, 1) [2^-20]; exp_normal / exp_any 0.825 ulp
[2], subnormal results 0.743 x 2^-1074 [2]; exp_neg 0.844 ulp [2]; jump_rate 0.844 ulp on (-708, 709) [2], 0.671 / 0.725 ulp
on the literal ranges with a normal exp(dH) [16] ("Device math")."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import philox as ph
from tests import device_math_ref as ref
from tests.helpers import bits_equal, hooks_context

pytestmark = pytest.mark.gpu

LD = ref.LD
U53 = 2.0 ** -53            # one ulp of [1/2, 1)
MIN_NORMAL = 2.0 ** -1022


def probe(which, a, b=None, second=False):
    from mjhmc_amd._lib import check, ptr
    ctx = hooks_context()
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = None if b is None else np.ascontiguousarray(b, dtype=np.float64)
    out0 = np.full(a.shape, np.nan)
    out1 = np.full(a.shape, np.nan) if second else None
    check(ctx.lib.mjhmc_test_device_math(ctx.handle, int(which), ptr(a), ptr(b), int(a.size), ptr(out0), ptr(out1)), ctx.lib)
    return (out0, out1) if second else out0


@functools.lru_cache(maxsize=None)
def exp_set():
    h = ref.exp_inputs()
    h.setflags(write=False)
    return h


@functools.lru_cache(maxsize=None)
def box_muller_set():
    """inputs and the long-double reference, shared by the float64 and float32 tests"""
    u1, u2 = ref.box_muller_inputs()
    return u1, u2, ref.box_muller_ref(u1, u2)


def test_neg_log_unit():
    u = ref.log_inputs()
    got = probe(0, u)
    err = ref.ulp_err(got, ref.neg_log_ref(u))
    print('neg_log_unit: max %.3f ulp over %d inputs (at u = %r)' % (err.max(), u.size, u[err.argmax()]))
    assert np.all(np.isfinite(got))
    assert np.all(got >= 0) and not np.signbit(got).any(), u[(got < 0) | np.signbit(got)][:8]
    assert got[u == 1.0].view(np.uint64)[0] == 0                                   # +0.0, bit for bit
    assert ref.ulp_err(got[u == U53], LD(53) * np.log(LD(2)))[0] <= 2
    assert err.max() <= 2, (err.max(), u[err.argmax()])


def test_sincospi_unit():
    t = ref.angle_inputs()
    s, c = probe(1, t, second=True)
    ws, wc = ref.sincospi_ref(t)
    es = (np.abs(s.astype(LD) - ws) / LD(U53)).astype(np.float64)
    ec = (np.abs(c.astype(LD) - wc) / LD(U53)).astype(np.float64)
    norm = (np.abs(s.astype(LD) ** 2 + c.astype(LD) ** 2 - 1) / LD(U53)).astype(np.float64)
    print('sincospi_unit: max |s - sin| %.3f, |c - cos| %.3f, |s^2 + c^2 - 1| %.3f (x 2^-53) over %d angles'
          % (es.max(), ec.max(), norm.max(), t.size))
    for x, vs, vc in ((0.0, 0, 1), (0.5, 1, 0), (1.0, 0, -1), (1.5, -1, 0), (2.0, 0, 1)):
        i = int(np.nonzero(t == x)[0][0])
        assert s[i] == vs and c[i] == vc, (x, s[i], c[i])
    assert es.max() <= 1.5 and ec.max() <= 1.5, (t[es.argmax()], es.max(), t[ec.argmax()], ec.max())
    assert norm.max() <= 4, (t[norm.argmax()], norm.max())


def test_box_muller():
    u1, u2, (w0, w1, r) = box_muller_set()
    z0, z1 = probe(2, u1, u2, second=True)
    assert np.all(np.isfinite(z0)) and np.all(np.isfinite(z1))
    with np.errstate(invalid='ignore', divide='ignore'):
        e0 = (np.abs(z0.astype(LD) - w0) / (LD(U53) * r)).astype(np.float64)
        e1 = (np.abs(z1.astype(LD) - w1) / (LD(U53) * r)).astype(np.float64)
    live = r > 0
    zmax = max(np.abs(z0).max(), np.abs(z1).max())
    print('box_muller: max |z - z_ref| / r_ref = %.3f, %.3f (x 2^-53) over %d pairs; max |z| = %r (sqrt(106 ln 2) = %r)'
          % (e0[live].max(), e1[live].max(), u1.size, zmax, float(np.sqrt(LD(106) * np.log(LD(2))))))
    # radius: 2 ulp of the log, halved by the square root, plus the root's rounding: <= 2 x 2^-53 relative; the
    # trigonometric factor: 1.5 x 2^-53 absolute; the product's rounding: 5 x 2^-53 r in all
    assert e0[live].max() <= 5 and e1[live].max() <= 5, (e0[live].max(), e1[live].max())
    one = u1 == 1.0
    assert one.sum() > 1000 and np.all(z0[one] == 0) and np.all(z1[one] == 0)      # a zero radius: +-0
    # |z| <= sqrt(106 ln 2), the radius of u1 = 2^-53 -- as far as float64 can say so: that number is not a float64 (the
    # correctly rounded radius is the float64 above it), so the ceiling carries the accuracy gate's 5 x 2^-53 r
    ceiling = np.sqrt(LD(106) * np.log(LD(2))) * (1 + 5 * LD(U53))
    assert np.abs(z0).astype(LD).max() <= ceiling and np.abs(z1).astype(LD).max() <= ceiling


def test_box_muller_f32():
    u1, u2, _ = box_muller_set()
    z0, z1 = probe(3, u1, u2, second=True)
    u1f, u2f = u1.astype(np.float32).astype(np.float64), u2.astype(np.float32).astype(np.float64)
    assert np.all(u1f > 0)
    w0, w1, r = ref.box_muller_ref(u1f, u2f)                                       # on the float-rounded inputs
    assert np.all(np.isfinite(z0)) and np.all(np.isfinite(z1))
    scale = np.maximum(r, LD(1))
    e0 = (np.abs(z0.astype(LD) - w0) / scale).astype(np.float64)
    e1 = (np.abs(z1.astype(LD) - w1) / scale).astype(np.float64)
    print('box_muller_f32: max |z - z_ref| / max(r_ref, 1) = %.3f, %.3f (x 2^-23) over %d pairs'
          % (e0.max() * 2.0 ** 23, e1.max() * 2.0 ** 23, u1.size))
    # logf 3 ulp, sqrtf 3 ulp, sincospif 4 ulp (the OpenCL limits of the library calls): <= 7 x 2^-23 composed, plus the
    # product's rounding -- the gate is 2^-20, loose on purpose: a wrong quadrant, pairing or a zero in the log is O(1)
    assert e0.max() <= 2.0 ** -20 and e1.max() <= 2.0 ** -20, (e0.max(), e1.max())
    assert np.all(z0.astype(np.float32) == z0) and np.all(z1.astype(np.float32) == z1)   # widened float32 values


def test_exp_chains():
    h = exp_set()
    core = h[np.isfinite(h) & (np.abs(h) <= 1100)]                                 # what exp_any hands to exp_normal
    want = ref.exp_ref(core)
    forms = [probe(w, core) for w in (4, 5, 6)]
    for name, got in zip(('exp_normal<true, false>', 'exp_normal<true, true>', 'exp_normal<false, true>'), forms):
        err = ref.ulp_err(got, want)
        w64 = ref.to_f64(want)
        nrm = np.isfinite(w64) & (w64 >= MIN_NORMAL)
        sub = w64 < MIN_NORMAL
        print('%s: max %.3f ulp (normal results), %.3f x 2^-1074 (subnormal results) over %d inputs'
              % (name, err[nrm].max(), err[sub].max(), core.size))
        assert err[nrm].max() <= 2, (name, core[nrm][err[nrm].argmax()], err[nrm].max())
        assert err[sub].max() <= 2, (name, core[sub][err[sub].argmax()], err[sub].max())
        assert np.all(got[np.isinf(w64)] == np.inf), name
    fast = np.abs(core) < 708
    assert fast.sum() > 100000
    assert bits_equal(forms[0][fast], forms[1][fast]) and bits_equal(forms[0][fast], forms[2][fast])

    # exp_any on every input, the specials included
    any_ = probe(7, h)
    want_all = ref.exp_ref(h)
    err = ref.ulp_err(any_, want_all)
    w64 = ref.to_f64(want_all)
    print('exp_any: max %.3f ulp over %d inputs (subnormal results in units of 2^-1074; 0, inf and NaN included)' % (err.max(), h.size))
    assert err.max() <= 2, (h[err.argmax()], err.max())
    assert np.all(any_[h >= 709.7828] == np.inf) and (h >= 709.7828).sum() > 500
    assert np.all(any_[h <= -746] == 0) and (h <= -746).sum() > 500
    assert np.isnan(any_[np.isnan(h)]).all() and np.isnan(h).sum() == 1
    assert any_[h == np.inf][0] == np.inf and any_[h == -np.inf][0] == 0
    with np.errstate(invalid='ignore'):
        sel = np.abs(h) < 708
    assert bits_equal(any_[sel], probe(6, h[sel]))

    # exp_neg(x) = exp(-x): both signs of every input, so that -x runs over the whole set
    x = np.concatenate([h[~np.isnan(h)], -h[~np.isnan(h)]])
    neg = probe(8, x)
    err = ref.ulp_err(neg, ref.exp_ref(-x))
    print('exp_neg: max %.3f ulp over %d inputs' % (err.max(), x.size))
    assert err.max() <= 2, (x[err.argmax()], err.max())
    fin = np.isfinite(x)
    assert bits_equal(neg[fin], probe(7, -x[fin]))                                 # the negated constant and argument are exact
    assert bits_equal(probe(9, x[fin]), neg[fin])                                  # exp_neg_k: "operation for operation"


def test_jump_rate():
    dH = exp_set()
    got = probe(10, dH)
    assert bits_equal(got, probe(11, dH))                                          # constants in scalar registers: the same bits
    nan = np.isnan(dH)
    assert np.isnan(got[nan]).all() and not np.isnan(got[~nan]).any()
    e_ld = ref.exp_ref(dH)                                                         # exp(dH) in long double ...
    with np.errstate(invalid='ignore'):
        want = np.sqrt(e_ld)                                                       # ... and exp(dH) ** .5 == exp(dH / 2)
    err = ref.ulp_err(got, want)
    fast = (dH > -708) & (dH < 709)
    print('jump_rate: max %.3f ulp on (-708, 709) over %d inputs' % (err[fast].max(), fast.sum()))
    assert err[fast].max() <= 2, (dH[fast][err[fast].argmax()], err[fast].max())
    # the literal ranges: exp(dH) ** .5 with the double exp in between
    assert np.all(got[dH >= 709.7828] == np.inf) and (dH >= 709.7828).sum() > 500
    top = (dH >= 709) & (dH <= 709.78)
    assert top.sum() > 100 and np.all(np.isfinite(got[top]))
    low = (dH > ref.LN_DBL_MIN) & (dH <= -708)                                     # exp(dH) still a normal number
    print('jump_rate: max %.3f ulp on [709, 709.78], %.3f ulp on (-708.396, -708]' % (err[top].max(), err[low].max()))
    assert err[top].max() <= 16 and err[low].max() <= 16
    gap = (dH > 709.78) & (dH < 709.7828)
    assert np.all((got[gap] == np.inf) | (err[gap] <= 16))
    # subnormal exp(dH) = k 2^-1074: the rate is the correctly rounded root of that coarse value
    band = (dH > -750) & (dH < -708.39)
    assert (band & (dH > -745.14)).sum() > 2500
    kr = e_ld[band] * LD(2.0) ** 1074
    k0 = np.floor(kr)
    ok = np.zeros(band.sum(), dtype=bool)
    for dk in (-1, 0, 1, 2):
        k = k0 + dk
        cand = np.sqrt(np.ldexp(np.maximum(k, 0).astype(np.float64), -1074))
        ok |= (np.abs(k - kr) <= 1) & (k >= 0) & (got[band] == cand)
    assert ok.all(), (dH[band][~ok][:8], got[band][~ok][:8])
    assert np.all(got[dH <= -750] == 0) and (dH <= -750).sum() > 500 and got[dH == -np.inf][0] == 0


def test_normal_pair_keying():
    from mjhmc_amd._lib import check, ptr
    ctx = hooks_context()
    seed = 0x9E3779B97F4A7C15                                                      # both words in use
    n_pairs = 5
    every = []
    for tick in (0, 1, 2 ** 32 + 5):
        for first in (0, 2 ** 31, 2 ** 32 - 64):
            out = np.full((64, n_pairs, 2), np.nan)
            check(ctx.lib.mjhmc_test_normal_pairs(ctx.handle, ctypes.c_uint64(seed), ctypes.c_uint64(tick), first, 64, n_pairs,
                                                  ptr(out)), ctx.lib)
            pid = (first + np.arange(64, dtype=np.uint64))[:, None]
            pair = np.arange(n_pairs, dtype=np.uint64)[None, :]
            w0, w1, w2, w3 = ph.philox4x32_10(pid, tick & 0xFFFFFFFF, tick >> 32, pair, seed & 0xFFFFFFFF, seed >> 32)
            u1, u2 = ph.u53(w0, w1), ph.u53(w2, w3)
            z0, z1 = probe(2, u1.ravel(), u2.ravel(), second=True)
            assert bits_equal(out[:, :, 0].ravel(), z0) and bits_equal(out[:, :, 1].ravel(), z1), (tick, first)
            every.append(out.ravel())
    every = np.concatenate(every)
    assert np.unique(every).size == every.size == 9 * 64 * n_pairs * 2             # every (tick, pid, pair) its own draw
    assert abs(every.mean()) < 0.1 and 0.9 < every.std() < 1.1                     # 5760 standard normals (std error 0.013)
