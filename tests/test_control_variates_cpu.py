"""CPU: what of the device control variates needs no device -- the eight exports in header, bindings and library, the
refusals that come before any handle is touched, the arithmetic of ``ControlVariateExpectations`` on synthetic sums, the
driver's argument checks, and the wiring of csrc/crossmoments.hip into the build."""
import ctypes
import os
import re

import numpy as np
import pytest

from mjhmc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'mjhmc_amd', 'csrc')
H = r'mjhmc_crossmoments\s*\*\s*h'
EXPORTS = {
    'mjhmc_crossmoments_create': (r'mjhmc_sampler\s*\*\s*s\s*,\s*mjhmc_crossmoments\s*\*\*\s*out', 2),
    'mjhmc_crossmoments_create_on': (r'mjhmc_functionals\s*\*\s*f\s*,\s*mjhmc_crossmoments\s*\*\*\s*out', 2),
    'mjhmc_crossmoments_set_shift': (H + r'\s*,\s*const\s+double\s*\*\s*cb', 2),
    'mjhmc_crossmoments_accumulate': (H + r'\s*,\s*int\s+x_slot0\s*,\s*int\s+w_slot0\s*,\s*int\s+n', 4),
    'mjhmc_crossmoments_read': (H + r'\s*,\s*double\s*\*\s*W\s*,\s*double\s*\*\s*Sg\s*,\s*double\s*\*\s*S2g\s*,\s*double\s*\*\s*Sb\s*,'
                                    r'\s*double\s*\*\s*S2b\s*,\s*double\s*\*\s*Cgg\s*,\s*double\s*\*\s*Cgb\s*,\s*int64_t\s*\*\s*n_states', 9),
    'mjhmc_crossmoments_reset': (H, 1),
    'mjhmc_crossmoments_info': (H + r'\s*,\s*int\s*\*\s*ndims\s*,\s*int\s*\*\s*n_values', 3),
    'mjhmc_crossmoments_destroy': (H, 1),
}


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_header_bindings_and_library_agree_on_the_exports(lib):
    from mjhmc_amd import engine
    from mjhmc_amd.samplers.markov_jump_hmc import HMCBase, ControlVariateExpectations  # noqa: F401
    header = open(os.path.join(ROOT, 'include', 'mjhmc_hip.h')).read()
    typedef = r'typedef\s+struct\s+mjhmc_crossmoments\s+mjhmc_crossmoments\s*;'
    assert re.search(typedef, header)
    assert set(n for n in _lib.PROTOTYPES if n.startswith('mjhmc_crossmoments_')) == set(EXPORTS)
    assert set(re.findall(r'\bint\s+(mjhmc_crossmoments_\w+)\s*\(', header)) == set(EXPORTS)
    docs = {}
    for name, (args, nargs) in EXPORTS.items():
        m = re.search(r'/\*((?:(?!\*/).)*)\*/\s*(?:%s\s*)?int\s+%s\s*\(\s*%s\s*\)\s*;' % (typedef, name, args), header, flags=re.S)
        assert m, '%s is declared with a doc comment' % name
        docs[name] = m.group(1)
        restype, argtypes = _lib.PROTOTYPES[name]
        assert restype is ctypes.c_int and len(argtypes) == nargs, name
        assert getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) == nargs
    assert _lib.PROTOTYPES['mjhmc_crossmoments_read'][1][8] == ctypes.POINTER(ctypes.c_int64)
    # every doc comment states the sums it is about
    sums = ('W', 'Sg', 'S2g', 'Sb', 'S2b', 'Cgg', 'Cgb')
    for name in ('mjhmc_crossmoments_create', 'mjhmc_crossmoments_accumulate', 'mjhmc_crossmoments_read', 'mjhmc_crossmoments_reset'):
        for word in sums:
            assert re.search(r'\b%s\b' % word, docs[name]), (name, word)
    for word in ('sum w g_d (b_k - cb_k)', 'sum w g_d g_e', 'MJHMC_ERR_UNSUPPORTED', 'E_p[g] = 0'):
        assert word in docs['mjhmc_crossmoments_create'], word
    for word in ('MJHMC_ERR_NONFINITE', 'mjhmc_crossmoments_reset', 'names the slot'):
        assert word in docs['mjhmc_crossmoments_accumulate'], word
    for name, words in (('mjhmc_crossmoments_create_on', ('Cgb', 'Sb')), ('mjhmc_crossmoments_set_shift', ('Sb', 'S2b', 'Cgb')),
                        ('mjhmc_crossmoments_info', ('Sg', 'Cgb')), ('mjhmc_crossmoments_destroy', ('sums',))):
        for word in words:
            assert word in docs[name], (name, word)
    assert re.search(r'#define\s+MJHMC_ABI_VERSION\s+2\b', header) and lib.mjhmc_abi_version() == 2
    assert callable(engine.DeviceSampler.cross_moments) and callable(engine.DeviceFunctionals.cross_moments)
    for method in ('set_shift', 'accumulate', 'read', 'reset', 'close'):
        assert callable(getattr(engine.DeviceCrossMoments, method)), method
    assert callable(HMCBase.cv_expectations)


def test_null_arguments_are_refused_before_any_handle_is_touched(lib):
    out = ctypes.c_void_p()
    fake = ctypes.c_void_p(1)                     # never dereferenced: the checks come before the handle is touched
    null_err = lambda: b'NULL argument' in lib.mjhmc_last_error()   # noqa: E731
    assert lib.mjhmc_crossmoments_create(None, ctypes.byref(out)) == -1 and null_err()
    assert lib.mjhmc_crossmoments_create(fake, None) == -1 and null_err()
    assert lib.mjhmc_crossmoments_create_on(None, ctypes.byref(out)) == -1 and null_err()
    assert lib.mjhmc_crossmoments_create_on(fake, None) == -1 and null_err()
    assert out.value is None
    assert lib.mjhmc_crossmoments_set_shift(None, None) == -1 and null_err()
    assert lib.mjhmc_crossmoments_accumulate(None, 0, -1, 1) == -1 and null_err()
    assert lib.mjhmc_crossmoments_reset(None) == -1 and null_err()
    d, k = ctypes.c_int(), ctypes.c_int()
    assert lib.mjhmc_crossmoments_info(None, ctypes.byref(d), ctypes.byref(k)) == -1 and null_err()
    assert lib.mjhmc_crossmoments_info(fake, None, ctypes.byref(k)) == -1 and null_err()
    assert lib.mjhmc_crossmoments_info(fake, ctypes.byref(d), None) == -1 and null_err()
    buf = np.zeros(4)
    W, n = ctypes.c_double(), ctypes.c_int64()
    good = [fake, ctypes.byref(W)] + [buf.ctypes.data_as(ctypes.c_void_p)] * 6 + [ctypes.byref(n)]
    for missing in range(9):
        args = list(good)
        args[missing] = None
        assert lib.mjhmc_crossmoments_read(*args) == -1 and null_err(), missing
    assert lib.mjhmc_crossmoments_destroy(None) == 0


def _sums(rs, D, K, M, G=None):
    """synthetic weighted sums of M draws: g (D, M), f (K, M) correlated with g, weights w, shift c"""
    G = rs.randn(D, M) if G is None else G
    F = rs.randn(K, D).dot(G) + 0.5 * rs.randn(K, M) + np.arange(1, K + 1)[:, None]
    w = rs.rand(M) + 0.1
    c = rs.randn(K)
    Fc = F - c[:, None]
    return (w.sum(), (G * w).sum(1), (G * G * w).sum(1), (Fc * w).sum(1), (Fc * Fc * w).sum(1), (G * w).dot(G.T),
            (G * w).dot(Fc.T), M, c), G, F, w


def test_control_variate_arithmetic_on_synthetic_sums():
    from mjhmc_amd.samplers.markov_jump_hmc import ControlVariateExpectations, Expectations
    rs = np.random.RandomState(0)
    D, K, M = 5, 3, 400
    args, G, F, w = _sums(rs, D, K, M)
    r = ControlVariateExpectations(*args)
    W, Sg, S2g, Sb, S2b, Cgg, Cgb, n_states, c = args
    # the formulas, written out independently: a weighted least-squares regression of f on [1, g] by the normal equations
    p = w / w.sum()
    gbar, fbar = G.dot(p), F.dot(p)
    Gc, Fc = G - gbar[:, None], F - fbar[:, None]
    cov_gg, cov_gf = (Gc * p).dot(Gc.T), (Gc * p).dot(Fc.T)
    coef = np.linalg.solve(cov_gg, cov_gf)
    assert r.rank == D and r.coef.shape == (D, K)
    assert np.allclose(r.grad_mean, gbar, rtol=1e-13, atol=1e-15)
    assert np.allclose(r.cov_gg, cov_gg, rtol=0, atol=1e-13) and np.allclose(r.cov_gf, cov_gf, rtol=0, atol=1e-12)
    assert np.allclose(r.coef, coef, rtol=0, atol=1e-11)
    assert np.allclose(r.mean, fbar - coef.T.dot(gbar), rtol=0, atol=1e-11)
    var = (Fc * Fc).dot(p)
    resid = Fc - coef.T.dot(Gc)
    assert np.allclose(r.variance_ratio, (resid * resid).dot(p) / var, rtol=0, atol=1e-11)
    assert np.all(r.variance_ratio > 0) and np.all(r.variance_ratio < 1)
    # plain is the Expectations of f from the same sums, bit for bit
    plain = Expectations(W, Sb, S2b, None, n_states, c)
    assert np.array_equal(r.plain.mean, plain.mean) and np.array_equal(r.plain.var, plain.var) and r.plain.cov is None
    assert np.allclose(r.plain.mean, fbar, rtol=0, atol=1e-12)
    assert np.array_equal(r.mean, r.plain.mean - r.coef.T.dot(r.grad_mean)) or \
        np.allclose(r.mean, r.plain.mean - r.coef.T.dot(r.grad_mean), rtol=0, atol=1e-14)
    assert r.n_states == M and r.total_weight == W and r.W == W
    for name, val in zip(('Sg', 'S2g', 'Sb', 'S2b', 'Cgg', 'Cgb', 'shift'), (Sg, S2g, Sb, S2b, Cgg, Cgb, c)):
        assert getattr(r, name) is val, name
    # f linear in g: the control variates remove all of the variance and return the intercept
    a, Bm = rs.randn(K), rs.randn(K, D)
    Flin = a[:, None] + Bm.dot(G)
    Fs = Flin - c[:, None]
    lin = ControlVariateExpectations(W, Sg, S2g, (Fs * w).sum(1), (Fs * Fs * w).sum(1), Cgg, (G * w).dot(Fs.T), M, c)
    assert np.allclose(lin.mean, a, rtol=0, atol=1e-11) and np.max(np.abs(lin.variance_ratio)) < 1e-11
    assert np.allclose(lin.coef, Bm.T, rtol=0, atol=1e-11)


def test_rank_deficient_gradient_covariance_takes_the_least_squares_branch():
    from mjhmc_amd.samplers.markov_jump_hmc import ControlVariateExpectations
    rs = np.random.RandomState(1)
    D, K, M = 4, 2, 300
    G = rs.randn(D, M)
    G[3] = G[0] - 2.0 * G[1]                       # an exactly dependent control variate: rank 3
    args, G, F, w = _sums(rs, D, K, M, G=G)
    r = ControlVariateExpectations(*args)
    assert r.rank == 3 and r.rank < D
    coef, _, rank, _ = np.linalg.lstsq(r.cov_gg, r.cov_gf, rcond=None)
    assert rank == 3 and np.array_equal(r.coef, coef)
    assert np.all(np.isfinite(r.mean)) and np.all(np.isfinite(r.variance_ratio))
    # the fit is that of the three independent control variates
    keep = [0, 1, 2]
    full = ControlVariateExpectations(args[0], args[1][keep], args[2][keep], args[3], args[4], args[5][np.ix_(keep, keep)],
                                      args[6][keep], M, args[8])
    assert full.rank == 3
    assert np.allclose(r.mean, full.mean, rtol=0, atol=1e-10) and np.allclose(r.variance_ratio, full.variance_ratio, rtol=0, atol=1e-10)


def _bare(nbatch=60, ndims=4, dist=None, comm=None):
    """a sampler without a device: anything that touched it would raise AttributeError, not ValueError"""
    from mjhmc_amd.samplers.markov_jump_hmc import HMCBase
    from mjhmc_amd.misc.distributions import TestGaussian
    s = HMCBase.__new__(HMCBase)
    s._dev, s.ndims, s.nbatch, s._comm = None, ndims, nbatch, comm
    s.distribution = dist if dist is not None else TestGaussian(ndims=ndims, nbatch=nbatch)
    return s


def test_every_value_error_of_the_driver_comes_before_any_device_work():
    from mjhmc_amd.misc.distributions import LambdaDistribution
    from mjhmc_amd.samplers.markov_jump_hmc import Projections
    s = _bare()
    with pytest.raises(ValueError, match='n_iter must be >= 1'):
        s.cv_expectations(0)
    with pytest.raises(ValueError, match='n_iter must be >= 1'):
        s.cv_expectations(-2)
    with pytest.raises(ValueError, match='do not determine a regression'):
        _bare(nbatch=4, ndims=4).cv_expectations(2)            # 8 states, 2 * ndims = 8
    with pytest.raises(ValueError, match='do not determine a regression'):
        _bare(nbatch=3, ndims=4).cv_expectations(2)
    with pytest.raises(ValueError, match='ndims <= 512'):
        _bare(nbatch=4000, ndims=513).cv_expectations(3)
    class TooMany(object):                         # (Projections itself stops at 512 values)
        n_values = 513
    with pytest.raises(ValueError, match='K <= 512'):
        s.cv_expectations(3, of=TooMany())
    with pytest.raises(ValueError, match='shift must have 4 entries'):
        s.cv_expectations(3, shift=np.zeros(3))
    with pytest.raises(ValueError, match='shift must have 2 entries'):
        s.cv_expectations(3, of=Projections(np.ones((2, 4))), shift=np.zeros(4))
    with pytest.raises(ValueError, match='columns'):
        s.cv_expectations(3, of=Projections(np.ones((2, 5))))
    A = np.array([[2.0, 0.5], [0.5, 1.0]])
    d = LambdaDistribution(energy_func=lambda X: 0.5 * np.sum(X * A.dot(X), axis=0).reshape(1, -1),
                           energy_grad_func=lambda X: A.dot(X), init=np.ones((2, 5)), name='dense quadratic')
    assert d.device_energy()[0] == _lib.E_HOST
    with pytest.raises(ValueError, match='opaque Python callables'):
        _bare(nbatch=5, ndims=2, dist=d).cv_expectations(3)
    with pytest.raises(ValueError, match='sharded sampler.*out of scope'):
        _bare(comm=object()).cv_expectations(3)
    # right arguments pass the checks and reach the device (there is none here)
    with pytest.raises(AttributeError):
        s._dwell_weighted = False
        s.cv_expectations(3, shift=np.zeros(4), block=2)


def test_sources_are_wired_into_the_build():
    mk = open(os.path.join(CSRC, 'Makefile')).read()
    srcs = re.search(r'^SRCS\s*=\s*(.*)$', mk, flags=re.M).group(1).split()
    assert 'crossmoments.hip' in srcs
    assert mk.count('crossmoments.hpp') == 3        # a dependency of all three object rules
    for name in ('crossmoments.hip', 'crossmoments.hpp'):
        assert os.path.exists(os.path.join(CSRC, name)), name
    assert '-ffp-contract=off' in mk


def test_the_cross_pass_has_no_float_atomics():
    src = open(os.path.join(CSRC, 'crossmoments.hip')).read()
    code = re.sub(r'//[^\n]*', '', src)
    assert '__builtin_amdgcn_mfma_f64_16x16x4f64' in code and 'xcov_kernel' in code and 'xcov_fold_kernel' in code
    assert 'atomicAdd' not in code and 'fma(' not in code
    assert set(re.findall(r'\batomic\w+', code)) == {'atomicMin'}          # the integer flag of the finiteness check
