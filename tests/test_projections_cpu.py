"""CPU: what of the linear projections needs no device -- the hipRTC compile of a link (mjhmc_projections_check), the
argument refusals of the two new entry points, the bindings, the ``Projections`` description and its principal axes, the
``of=P`` argument checks of the drivers, and the wiring of csrc/projections.hip / .hpp into the build."""
import ctypes
import os
import re

import numpy as np
import pytest

from mjhmc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'mjhmc_amd', 'csrc')
NEW = ('mjhmc_projections_check', 'mjhmc_functionals_create_linear')


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _bare_sampler(ndims):
    """a sampler whose ``_dev`` is None: anything that touched the device would raise AttributeError, not ValueError"""
    from mjhmc_amd.samplers.markov_jump_hmc import HMCBase
    s = HMCBase.__new__(HMCBase)
    s._dev, s.ndims = None, ndims
    return s


# ---------------------------------------------------------------------------------------------------------------------
# 1.  the exports
# ---------------------------------------------------------------------------------------------------------------------
def test_header_bindings_and_library_agree_on_the_two_exports(lib):
    from mjhmc_amd import engine
    from mjhmc_amd.samplers.markov_jump_hmc import HMCBase, Projections
    header = open(os.path.join(ROOT, 'include', 'mjhmc_hip.h')).read()
    for name in NEW:
        assert name in _lib.PROTOTYPES, name
        assert re.search(r'\b%s\s*\(' % name, header), name
        assert getattr(lib, name) is not None
    # the argument counts of the header and of the bindings
    for name in NEW:
        proto = re.search(r'\bint\s+%s\s*\(([^)]*)\)' % name, header).group(1)
        assert len(proto.split(',')) == len(_lib.PROTOTYPES[name][1]), name
    assert re.search(r'#define\s+MJHMC_ABI_VERSION\s+2\b', header) and lib.mjhmc_abi_version() == 2
    assert callable(engine.DeviceFunctionals.linear) and callable(engine.DeviceSampler.projections)
    assert callable(HMCBase.projections) and callable(Projections.principal)


# ---------------------------------------------------------------------------------------------------------------------
# 2.  mjhmc_projections_check
# ---------------------------------------------------------------------------------------------------------------------
def test_links_compile_without_a_device(lib):
    inc = _lib.KERNEL_HEADERS.encode()
    for K in (1, 16, 17, 512):                         # both tiles
        assert lib.mjhmc_projections_check(K, None, inc) == 0, lib.mjhmc_last_error()
    assert lib.mjhmc_projections_check(3, None, None) == 0, 'the identity needs no headers'
    for K, link in ((3, b'u'), (3, b'u * u + p[0]'), (65, b'k == 0 ? u : 1.0 / (1.0 + exp(-u))'), (1, b'u > p[0] ? 1.0 : 0.0')):
        assert lib.mjhmc_projections_check(K, link, inc) == 0, lib.mjhmc_last_error()


def test_a_syntax_error_returns_the_compilers_text(lib):
    inc = _lib.KERNEL_HEADERS.encode()
    assert lib.mjhmc_projections_check(4, b'u * y', inc) == -1
    msg = lib.mjhmc_last_error()
    assert b'link expression does not compile' in msg and b'undeclared' in msg and b"'y'" in msg, msg
    assert lib.mjhmc_projections_check(4, b'u +', inc) == -1 and b'error' in lib.mjhmc_last_error()
    for link in (b'', b'  ', b'u; u'):
        assert lib.mjhmc_projections_check(4, link, inc) == -1 and b'one C expression' in lib.mjhmc_last_error(), link
    assert lib.mjhmc_projections_check(4, b'u', None) == -1 and b'NULL argument' in lib.mjhmc_last_error()


def test_counts_outside_the_range_are_refused_with_a_message(lib):
    inc = _lib.KERNEL_HEADERS.encode()
    for K in (0, 513, -1):
        assert lib.mjhmc_projections_check(K, None, inc) == -1
        assert b'K must be in [1, 512], got %d' % K in lib.mjhmc_last_error()
        assert lib.mjhmc_projections_check(K, b'u', inc) == -1 and b'K must be in [1, 512]' in lib.mjhmc_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# 3.  mjhmc_functionals_create_linear: refusals that come before the handle is touched
# ---------------------------------------------------------------------------------------------------------------------
def test_create_linear_refuses_null_and_fake_handles(lib):
    inc = _lib.KERNEL_HEADERS.encode()
    out = ctypes.c_void_p()
    fake = ctypes.c_void_p(1)                          # never dereferenced: the checks below come before the handle is touched
    A, b, p = np.ones((2, 3)), np.zeros(2), np.ones(2)
    for args in ((None, 2, _lib.ptr(A), _lib.ptr(b), None, None, 0, inc, ctypes.byref(out)),
                 (fake, 2, None, _lib.ptr(b), None, None, 0, inc, ctypes.byref(out)),
                 (fake, 2, _lib.ptr(A), _lib.ptr(b), None, None, 0, inc, None),
                 (fake, 2, _lib.ptr(A), None, b'u', None, 0, None, ctypes.byref(out))):
        assert lib.mjhmc_functionals_create_linear(*args) == -1
        assert b'NULL argument' in lib.mjhmc_last_error()
    assert lib.mjhmc_functionals_create_linear(fake, 2, _lib.ptr(A), None, None, None, 2, inc, ctypes.byref(out)) == -1
    assert b'params is NULL' in lib.mjhmc_last_error()
    for K in (0, 513):
        assert lib.mjhmc_functionals_create_linear(fake, K, _lib.ptr(A), None, None, _lib.ptr(p), 2, inc, ctypes.byref(out)) == -1
        assert b'K must be in [1, 512], got %d' % K in lib.mjhmc_last_error()
    assert out.value is None
    assert lib.mjhmc_abi_version() == 2


# ---------------------------------------------------------------------------------------------------------------------
# 4.  Projections
# ---------------------------------------------------------------------------------------------------------------------
def test_projections_description_validates_before_any_run(lib):
    from mjhmc_amd.samplers.markov_jump_hmc import Projections
    s = _bare_sampler(4)
    rs = np.random.RandomState(0)
    A = rs.randn(3, 4)
    P = s.projections(A, b=[1.0, 2.0, 3.0], link='u * u + p[0]', params=[0.5], names=['a', 'b', 'c'])
    assert isinstance(P, Projections) and P.n_values == 3 and P.names == ['a', 'b', 'c'] and P.link == 'u * u + p[0]'
    assert np.array_equal(P.A, A) and np.array_equal(P.b, [1.0, 2.0, 3.0]) and np.array_equal(P.params, [0.5])
    assert P.A.dtype == P.b.dtype == np.float64 and P.A.flags.c_contiguous
    # one direction, a scalar b, the defaults
    one = s.projections(A[0], b=3.0)
    assert one.n_values == 1 and one.A.shape == (1, 4) and np.array_equal(one.b, [3.0]) and one.names == ['u0'] and one.link is None
    assert s.projections(A).names == ['u0', 'u1', 'u2'] and np.array_equal(s.projections(A).b, np.zeros(3))
    assert np.array_equal(s.projections(A, b=2.0).b, [2.0, 2.0, 2.0])
    # slot_bytes: rows padded to 64, values to an even count, float64
    for K, N in ((1, 1), (3, 65), (64, 200), (65, 64), (512, 1000)):
        P = Projections(np.ones((K, 4)))
        assert P.slot_bytes(N) == (N + 63) // 64 * 64 * ((K + 1) // 2 * 2) * 8, (K, N)
    # shapes
    with pytest.raises(ValueError, match='ndims = 4 columns'):
        s.projections(rs.randn(3, 5))
    with pytest.raises(ValueError, match='ndims = 4 columns'):
        s.projections(rs.randn(5))
    with pytest.raises(ValueError, match=r'\(K, ndims\)'):
        s.projections(rs.randn(2, 3, 4))
    with pytest.raises(ValueError, match='b must be a scalar or have K = 3'):
        s.projections(A, b=np.zeros(4))
    with pytest.raises(ValueError, match='b must be a scalar or have K = 3'):
        s.projections(A, b=np.zeros((3, 1)))
    with pytest.raises(ValueError, match='names'):
        s.projections(A, names=['a'])
    # the range of K
    with pytest.raises(ValueError, match=r'K must be in \[1, 512\], got 513'):
        s.projections(np.ones((513, 4)))
    with pytest.raises(ValueError, match=r'K must be in \[1, 512\], got 0'):
        s.projections(np.ones((0, 4)))
    assert s.projections(np.ones((512, 4))).n_values == 512
    # finiteness
    for bad in (np.nan, np.inf, -np.inf):
        Ab = A.copy()
        Ab[1, 2] = bad
        with pytest.raises(ValueError, match='A must be finite'):
            s.projections(Ab)
        with pytest.raises(ValueError, match='b must be finite'):
            s.projections(A, b=[0.0, bad, 0.0])
        with pytest.raises(ValueError, match='params must be finite'):
            s.projections(A, link='u + p[0]', params=[bad])
    # the link
    with pytest.raises(ValueError, match="undeclared identifier 'q'"):
        s.projections(A, link='u * q')
    for link in ('', '  ', 'u; u', 3):
        with pytest.raises(ValueError, match='one C expression'):
            s.projections(A, link=link)


def test_of_argument_checks_come_before_any_device_work():
    from mjhmc_amd.samplers.markov_jump_hmc import Projections
    s = _bare_sampler(4)
    P = Projections(np.eye(4)[:3])
    assert P.n_values == 3
    with pytest.raises(ValueError, match='n_values = 3'):
        s.expectations(5, of=P, shift=np.zeros(4))         # ndims entries: wrong for K = 3
    with pytest.raises(ValueError, match='n_values = 3'):
        s.diagnostics(8, of=P, shift=np.zeros(4))
    with pytest.raises(ValueError, match='n_values = 3'):
        s.marginals(5, of=P, range=(np.zeros(4), np.ones(4)))
    with pytest.raises(ValueError, match='n_values = 3'):
        s.joint_marginals(5, [(0, 1)], of=P, range=(np.zeros(4), np.ones(4)))
    with pytest.raises(ValueError, match=r'n_values = 3'):
        s.joint_marginals(5, [(0, 3)], of=P)               # a pair outside the K values
    # projections of another width than the sampler's
    Q = Projections(np.ones((2, 5)))
    for call in (lambda: s.expectations(5, of=Q), lambda: s.diagnostics(8, of=Q), lambda: s.marginals(5, of=Q),
                 lambda: s.joint_marginals(5, [(0, 1)], of=Q)):
        with pytest.raises(ValueError, match='5 columns'):
            call()
    # the checks that were there stay in front
    for call in (lambda: s.expectations(0, of=P), lambda: s.diagnostics(5, of=P), lambda: s.marginals(3, bins=0, of=P),
                 lambda: s.marginals(3, span=0.0, of=P)):
        with pytest.raises(ValueError):
            call()
    # a right-sized argument passes the checks and reaches the device (there is none here)
    with pytest.raises(AttributeError):
        s._dwell_weighted = False
        s.expectations(5, of=P, shift=np.zeros(3))


# ---------------------------------------------------------------------------------------------------------------------
# 5.  principal axes
# ---------------------------------------------------------------------------------------------------------------------
def _synthetic_expectations(D, seed, cov=True):
    """an Expectations built by hand from a known mean and covariance (W = 1, sums about a zero shift)"""
    from mjhmc_amd.samplers.markov_jump_hmc import Expectations
    rs = np.random.RandomState(seed)
    Q, _ = np.linalg.qr(rs.randn(D, D))
    spec = 10.0 ** np.linspace(-1.0, 1.0, D)
    C = (Q * spec) @ Q.T
    C = 0.5 * (C + C.T)
    mean = rs.randn(D)
    ex = Expectations(1.0, mean.copy(), np.diag(C) + mean * mean, (C + np.outer(mean, mean)) if cov else None, 1000, np.zeros(D))
    return ex, mean, C, spec[::-1]


def test_principal_axes_of_a_synthetic_covariance():
    from mjhmc_amd.samplers.markov_jump_hmc import Projections
    D = 7
    ex, mean, C, spec = _synthetic_expectations(D, 3)
    assert np.allclose(ex.cov, C, rtol=0, atol=1e-12) and np.allclose(ex.mean, mean)
    P = Projections.principal(ex)
    assert P.n_values == D and P.A.shape == (D, D) and P.link is None and P.names[0] == 'u0'
    assert np.max(np.abs(P.A @ P.A.T - np.eye(D))) <= 1e-12, 'the rows are orthonormal'
    M = P.A @ ex.cov @ P.A.T
    lam = np.diag(M)
    assert np.max(np.abs(M - np.diag(lam))) <= 1e-12 and np.all(np.diff(lam) <= 0), 'diagonal, descending'
    assert np.allclose(lam, spec, rtol=1e-10)
    # the sign rule: the largest-magnitude entry of every row is positive
    big = np.argmax(np.abs(P.A), axis=1)
    assert np.all(P.A[np.arange(D), big] > 0)
    assert np.array_equal(P.b, -P.A.dot(ex.mean))
    # k keeps the widest axes
    P3 = Projections.principal(ex, k=3, names=['p0', 'p1', 'p2'])
    assert P3.n_values == 3 and np.array_equal(P3.A, P.A[:3]) and np.array_equal(P3.b, P.b[:3]) and P3.names == ['p0', 'p1', 'p2']
    # whiten: the measured covariance becomes the identity
    Pw = Projections.principal(ex, whiten=True)
    assert np.max(np.abs(Pw.A @ ex.cov @ Pw.A.T - np.eye(D))) <= 1e-12
    assert np.array_equal(Pw.b, -Pw.A.dot(ex.mean))
    assert np.allclose(Pw.A * np.sqrt(lam)[:, None], P.A, rtol=1e-12, atol=0)


def test_principal_axes_refusals():
    from mjhmc_amd.samplers.markov_jump_hmc import Expectations, Projections
    ex, mean, C, spec = _synthetic_expectations(5, 4, cov=False)
    assert ex.cov is None
    with pytest.raises(ValueError, match='cov=True'):
        Projections.principal(ex)
    ex, mean, C, spec = _synthetic_expectations(5, 4)
    for k in (0, 6):
        with pytest.raises(ValueError, match=r'k must be in \[1, ndims = 5\]'):
            Projections.principal(ex, k=k)
    # a covariance with a zero eigenvalue (a constant coordinate): fine as it is, refused for whitening
    flat = Expectations(1.0, np.zeros(3), np.array([1.0, 2.0, 0.0]), np.diag([1.0, 2.0, 0.0]), 10, np.zeros(3))
    assert Projections.principal(flat).n_values == 3
    assert Projections.principal(flat, k=2, whiten=True).n_values == 2
    with pytest.raises(ValueError, match='positive eigenvalues'):
        Projections.principal(flat, whiten=True)


# ---------------------------------------------------------------------------------------------------------------------
# 6.  the build
# ---------------------------------------------------------------------------------------------------------------------
def test_sources_are_wired_into_the_makefile():
    mk = open(os.path.join(CSRC, 'Makefile')).read()
    for var in ('SRCS', 'ASAN_SRCS', 'HOOKS_SRCS'):
        m = re.search(r'^%s\s*=\s*(.*)$' % var, mk, flags=re.M)
        assert m and 'projections.hip' in m.group(1).split(), var
    assert mk.count('projections.hpp') == 3, 'a dependency of all three object rules'
    for name in ('projections.hip', 'projections.hpp'):
        assert os.path.exists(os.path.join(CSRC, name)), name


def test_the_kernel_header_keeps_contraction_off_and_has_no_float_atomics():
    hpp = open(os.path.join(CSRC, 'projections.hpp')).read()
    assert '-ffp-contract=off' in hpp[:hpp.index('#pragma once')], 'the header comment states the flag the kernel relies on'
    assert '#pragma clang fp contract(off)' in hpp
    code = re.sub(r'//[^\n]*', '', hpp)
    assert 'atomicAdd' not in code and 'fma(' not in code
    assert re.findall(r'atomic\w+', code) == ['atomicMin']
    # what hipRTC compiles includes nothing of the project but functionals.hpp
    assert re.findall(r'#include\s+"([^"]+)"', code) == ['functionals.hpp']
