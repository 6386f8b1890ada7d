"""The host side of the device-math tests (tests/device_math_ref.py): the input sets are what they claim to be, the
long-double references are the high-precision side (against 200-bit mpmath), and the ulp measure counts ulps."""
import os
import re

import numpy as np
import pytest

from tests import device_math_ref as ref

LD = ref.LD
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'mjhmc_amd', 'csrc')


def test_long_double_has_a_64_bit_mantissa():
    assert np.finfo(LD).nmant >= 63, 'the references need more than float64'


def test_log_inputs_are_what_u53_returns_and_hold_every_edge():
    u = ref.log_inputs()
    j = u * ref.TWO53
    assert u.dtype == np.float64 and np.all((u > 0) & (u <= 1)) and np.array_equal(j, np.rint(j))
    have = set(u.tolist())
    assert 2.0 ** -53 in have and 1.0 in have and 1.0 - 2.0 ** -53 in have and 4096 / ref.TWO53 in have
    for e in range(1, 54):
        assert 2.0 ** -e in have, e                                          # both ends of every binade ...
        if e < 53:
            assert 2.0 ** -e * (1 - 2.0 ** -(53 - e)) in have, e             # ... and the grid point below it
        m, _ = np.frexp(u[(u >= 2.0 ** -e) & (u < 2.0 ** -(e - 1))])
        if e <= 52:                                                          # both sides of the `low` switch
            assert (m < ref.SQRT_HALF).any() and (m >= ref.SQRT_HALF).any(), e
    m1 = np.frexp(u[(u >= 0.5) & (u < 1)])[0]
    assert ref.SQRT_HALF in m1 and np.nextafter(ref.SQRT_HALF, 0) in m1      # the switch itself, to the last bit
    assert u.size < 100000


def test_angle_inputs_are_in_range_and_hold_every_edge():
    t = ref.angle_inputs()
    assert np.all((t >= 0) & (t <= 2)) and t.size < 300000
    have = set(t.tolist())
    for k in range(17):
        x = k / 8.0
        assert x in have
        assert k == 16 or np.nextafter(x, 3) in have
        assert k == 0 or np.nextafter(x, -1) in have
    n = np.rint(2 * t)
    assert set(n.tolist()) == {0.0, 1.0, 2.0, 3.0, 4.0}
    x = np.abs((t - 0.5 * n) * np.pi)
    for q in range(5):                                                       # both sides of the qx split in every quadrant
        assert ((n == q) & (x < 0.3) & (x > 0.3 - 1e-13)).any() and ((n == q) & (x >= 0.3) & (x < 0.3 + 1e-13)).any(), q
    assert np.all(np.abs(t - 0.5 * n) <= 0.25)


def test_exp_inputs_hold_every_edge():
    h = ref.exp_inputs()
    have = h[~np.isnan(h)]
    assert np.isnan(h).sum() == 1 and np.isinf(h).sum() == 2 and h.size < 120000
    assert have[np.isfinite(have)].min() == -1e308 and have[np.isfinite(have)].max() == 1e308
    for x in ref.EXP_EDGES:
        assert ((have < x) & (have > x - 1e-9 - abs(x) * 1e-13)).sum() >= 64 or x == 0.0
        assert x in have and np.nextafter(x, np.inf) in have and np.nextafter(x, -np.inf) in have
    assert np.signbit(have[have == 0]).any() and not np.signbit(have[have == 0]).all()
    assert (np.abs(np.diff(np.sort(have[(have >= -760) & (have <= 719.9)]))) <= 0.0137 * 1.0001).all()
    # both sides of every threshold the code or its results switch at
    for x in (ref.LN_DBL_MIN, ref.LN_DBL_MAX, -708.0, 709.0, -745.1332, 0.0):
        assert (have < x).any() and (have > x).any()


def test_box_muller_inputs_cross_the_radius_tails_with_the_angle_edges():
    u1, u2 = ref.box_muller_inputs()
    assert u1.shape == u2.shape and u1.size < 500000
    assert np.all((u1 > 0) & (u1 <= 1)) and np.all((u2 > 0) & (u2 <= 1))
    edges = ref.angle_edges()
    for c in ref.BM_U1_CENTRES:
        got = np.unique(2.0 * u2[u1 == c])
        assert np.isin(edges[edges >= 2.0 ** -1022], got).all(), c
    tail = u1[(1 << 16) * -1:]
    assert np.array_equal(tail * ref.TWO53, np.rint(tail * ref.TWO53))


def test_neighbours_walks_the_doubles():
    n = ref.neighbours(1.0, 2)
    assert n.tolist() == [1 - 2.0 ** -52, 1 - 2.0 ** -53, 1.0, 1 + 2.0 ** -52, 1 + 2.0 ** -51]
    z = ref.neighbours(0.0, 2)
    assert z.tolist() == [-1e-323, -5e-324, 0.0, 5e-324, 1e-323]
    assert ref.neighbours(-1.0, 1).tolist() == [-1 - 2.0 ** -52, -1.0, -1 + 2.0 ** -53]
    assert np.all(np.diff(ref.neighbours(-708.0)) > 0) and ref.neighbours(-708.0).size == 129


def test_ulp_measure_on_hand_made_cases():
    one = np.array([1.0, 1.0, 1.0, 1.5, 2.0 ** -1060, 0.0, 5e-324])
    want = np.array([1.0, 1.0 + 2.0 ** -52, 1.0 + 2.0 ** -51, 1.5 - 2.0 ** -51, 2.0 ** -1060 + 3 * 2.0 ** -1074, 2.0 ** -1073, 0.0])
    assert ref.ulp_err(one, want.astype(LD)).tolist() == [0.0, 1.0, 2.0, 2.0, 3.0, 2.0, 1.0]
    # across a binade: the ulp is that of the float64 the reference rounds to
    assert ref.ulp_err(np.array([1.0]), np.array([1.0 - 2.0 ** -53], dtype=LD))[0] == 1.0      # in ulps of [1/2, 1)
    assert ref.ulp_err(np.array([1.0 - 2.0 ** -53]), np.array([1.0], dtype=LD))[0] == 0.5      # in ulps of [1, 2)
    # a long-double reference between two doubles: fractions of an ulp are resolved
    w = LD(1.0) + LD(2.0) ** -54
    assert ref.ulp_err(np.array([1.0, 1.0 + 2.0 ** -52]), np.array([w, w]))[0] == 0.25
    assert ref.ulp_err(np.array([1.0, 1.0 + 2.0 ** -52]), np.array([w, w]))[1] == 0.75
    # non-finite values: equal or infinitely wrong
    big = np.finfo(np.float64).max
    got = np.array([np.inf, big, np.inf, np.nan, 1.0, np.nan, -np.inf, 0.0])
    want = np.array([np.inf, np.inf, big, np.nan, np.nan, 1.0, np.inf, np.inf], dtype=LD)
    assert ref.ulp_err(got, want).tolist() == [0.0, np.inf, np.inf, 0.0, np.inf, np.inf, np.inf, np.inf]
    over = ref.exp_ref(np.array([709.79]))                                    # finite in long double, inf in float64
    assert np.isfinite(over[0]) and ref.ulp_err(np.array([np.inf, big]), np.array([over[0], over[0]])).tolist() == [0.0, np.inf]


def test_long_double_to_float64_lands_in_the_subnormal_range_and_at_inf():
    got = ref.to_f64(ref.exp_ref(np.array([-745.13, -745.2, 709.79, 709.78, -708.4, -1100.0, 1100.0, -np.inf, np.inf])))
    assert got[0] == 5e-324 and got[1] == 0.0 and got[2] == np.inf and np.isfinite(got[3])
    assert 0 < got[4] < 2.0 ** -1022 and got[5] == 0.0 and got[6] == np.inf and got[7] == 0.0 and got[8] == np.inf
    assert np.isnan(ref.to_f64(ref.exp_ref(np.array([np.nan]))))[0]


def _mpf(g, mp):
    """a long double as an mpmath number, exactly: its 64-bit mantissa in two 32-bit pieces (each exact in float64)"""
    m, e = np.frexp(LD(g))
    hi = np.floor(m * LD(2.0 ** 32))
    lo = (m * LD(2.0 ** 32) - hi) * LD(2.0 ** 32)
    assert lo == np.floor(lo) and (hi * LD(2.0 ** 32) + lo) * LD(2.0) ** -64 == m
    return mp.ldexp(mp.mpf(int(float(hi))) * 2 ** 32 + mp.mpf(int(float(lo))), int(e) - 64)


def _rel(got_ld, want_mp, mp):
    """max |got - want| / |want|, the difference taken in mpmath"""
    return max(float(abs(_mpf(g, mp) - w) / abs(w)) for g, w in zip(got_ld, want_mp))


def test_references_agree_with_mpmath_on_the_edges():
    mpmath = pytest.importorskip('mpmath')
    mp = mpmath.mp
    old = mp.prec
    mp.prec = 200
    try:
        bound = 2.0 ** -62
        # log: relative to the result; 1.0 gives exactly 0
        u = ref.log_edges()
        got = ref.neg_log_ref(u)
        assert got[u == 1.0][0] == 0
        keep = u != 1.0
        assert _rel(got[keep], [-mp.log(mp.mpf(float(x))) for x in u[keep]], mp) <= bound
        # exp, in long double and through its conversion to float64 (subnormal, 0, inf)
        h = ref.exp_edges()
        h = h[np.isfinite(h) & (np.abs(h) < 11000)]
        got = ref.exp_ref(h)
        want = [mp.exp(mp.mpf(float(x))) for x in h]
        assert _rel(got, want, mp) <= bound
        g64 = ref.to_f64(got)
        tiny = mp.mpf(2) ** -1074
        dbl_max = mp.mpf(float(np.finfo(np.float64).max))
        for x, g, w in zip(h, g64, want):
            if w >= dbl_max + mp.mpf(2) ** 970:
                assert g == np.inf, x
            elif w < mp.mpf(2) ** -1022:
                assert abs(mp.mpf(float(g)) - w) <= tiny * (0.5 + 2.0 ** -10), x      # nearest subnormal (or 0)
            else:
                assert np.isfinite(g) and abs(mp.mpf(float(g)) - w) <= abs(w) * mp.mpf(2) ** -53 * (1 + 2.0 ** -10), x
        # sin / cos after the exact reduction: absolute, the values are <= 1 (2^-62 of 1)
        t = ref.angle_edges()
        s, c = ref.sincospi_ref(t)
        pi = mp.pi
        ws = [mp.sin(pi * mp.mpf(float(x))) for x in t]
        wc = [mp.cos(pi * mp.mpf(float(x))) for x in t]
        for got_v, want_v in ((s, ws), (c, wc)):
            for g, w, x in zip(got_v, want_v, t):
                d = abs(_mpf(g, mp) - w)
                assert d <= mp.mpf(2) ** -62 * max(abs(w), mp.mpf(2) ** -3), (x, float(d))   # relative above 1/8, absolute below
        for x, es, ec in ((0.0, 0, 1), (0.5, 1, 0), (1.0, 0, -1), (1.5, -1, 0), (2.0, 0, 1)):
            i = int(np.nonzero(t == x)[0][0])
            assert s[i] == es and c[i] == ec
    finally:
        mp.prec = old


def test_the_probe_is_compiled_into_the_test_build_only():
    mk = open(os.path.join(CSRC, 'Makefile')).read()
    for var in ('SRCS', 'ASAN_SRCS', 'HOOKS_SRCS'):
        assert 'device_math_probe.hip' not in re.search(r'^%s\s*=\s*(.*)$' % var, mk, flags=re.M).group(1).split(), var
    assert re.search(r'^HOOKS_ONLY\s*=\s*device_math_probe\.hip\s*$', mk, flags=re.M)
    src = open(os.path.join(CSRC, 'device_math_probe.hip')).read()
    body = [ln for ln in src.splitlines() if ln.strip() and not ln.lstrip().startswith('//')]
    assert body[0] == '#ifdef MJHMC_TEST_HOOKS' and body[-1].startswith('#endif')
    from mjhmc_amd import _lib
    assert 'mjhmc_test_device_math' in _lib.TEST_HOOK_PROTOTYPES and 'mjhmc_test_normal_pairs' in _lib.TEST_HOOK_PROTOTYPES
    assert not any(k.startswith('mjhmc_test_') for k in _lib.PROTOTYPES)
    hdr = open(os.path.join(CSRC, '..', '..', 'include', 'mjhmc_hip.h')).read()
    assert 'mjhmc_test_device_math' not in hdr
    if not os.path.exists(_lib.TEST_HOOKS_PATH):
        import __graft_entry__ as g
        g.build()
    ship = open(_lib.LIB_PATH, 'rb').read()
    test = open(_lib.TEST_HOOKS_PATH, 'rb').read()
    for name in (b'mjhmc_test_device_math', b'mjhmc_test_normal_pairs', b'device_math_kernel', b'normal_pairs_kernel'):
        assert name not in ship and name in test, name
    assert not re.search(rb'mjhmc_test_\w+', ship)
