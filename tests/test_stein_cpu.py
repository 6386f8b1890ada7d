"""CPU: what of the kernel Stein discrepancy needs no device -- the three exports in header, bindings and library, the
refusals that come before any handle is touched, the arithmetic of ``SteinDiscrepancy`` on synthetic sums, the driver's
argument checks, and the wiring of csrc/stein.hip into the build."""
import ctypes
import os
import re

import numpy as np
import pytest

from mjhmc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'mjhmc_amd', 'csrc')
EXPORTS = {
    'mjhmc_stein_create': r'mjhmc_sampler\s*\*\s*s\s*,\s*double\s+c\s*,\s*mjhmc_stein\s*\*\*\s*out',
    'mjhmc_stein_evaluate': r'mjhmc_stein\s*\*\s*k\s*,\s*int\s+x_slot\s*,\s*int\s+w_slot\s*,\s*int64_t\s+n_use\s*,\s*double\s+out\[4\]',
    'mjhmc_stein_destroy': r'mjhmc_stein\s*\*\s*k',
}


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_header_bindings_and_library_agree_on_the_exports(lib):
    from mjhmc_amd import engine
    from mjhmc_amd.samplers.markov_jump_hmc import HMCBase, SteinDiscrepancy  # noqa: F401
    header = open(os.path.join(ROOT, 'include', 'mjhmc_hip.h')).read()
    assert re.search(r'typedef\s+struct\s+mjhmc_stein\s+mjhmc_stein\s*;', header)
    docs = {}
    for name, args in EXPORTS.items():
        m = re.search(r'/\*((?:(?!\*/).)*)\*/\s*(?:typedef\s+struct\s+mjhmc_stein\s+mjhmc_stein\s*;\s*)?int\s+%s\s*\(\s*%s\s*\)\s*;'
                      % (name, args), header, flags=re.S)
        assert m, '%s is declared with a doc comment' % name
        docs[name] = m.group(1)
        restype, argtypes = _lib.PROTOTYPES[name]
        assert restype is ctypes.c_int
        assert getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) == len(argtypes)
    assert len(_lib.PROTOTYPES['mjhmc_stein_create'][1]) == 3 and _lib.PROTOTYPES['mjhmc_stein_create'][1][1] is ctypes.c_double
    assert len(_lib.PROTOTYPES['mjhmc_stein_evaluate'][1]) == 5 and _lib.PROTOTYPES['mjhmc_stein_evaluate'][1][3] is ctypes.c_int64
    # the formula, and the refusals, are in the header
    for word in ('gg*t - t^3*dd + ndims*t^3 - 3*t^5*r2', '(c^2 + |x-y|^2)^(-1/2)', 'MJHMC_ERR_UNSUPPORTED'):
        assert word in docs['mjhmc_stein_create'], word
    for word in ('W2', 'Sd', 'MJHMC_ERR_NONFINITE', 'n_use'):
        assert word in docs['mjhmc_stein_evaluate'], word
    assert re.search(r'#define\s+MJHMC_ABI_VERSION\s+2\b', header) and lib.mjhmc_abi_version() == 2
    assert callable(engine.DeviceSampler.stein) and callable(engine.DeviceStein.evaluate) and callable(engine.DeviceStein.close)
    assert callable(HMCBase.stein_discrepancy)


def test_null_and_bad_c_are_refused_before_any_handle_is_touched(lib):
    out = ctypes.c_void_p()
    fake = ctypes.c_void_p(1)                     # never dereferenced: the checks come before the handle is touched
    four = (ctypes.c_double * 4)()
    assert lib.mjhmc_stein_create(None, 1.0, ctypes.byref(out)) == -1 and b'NULL argument' in lib.mjhmc_last_error()
    assert lib.mjhmc_stein_create(fake, 1.0, None) == -1 and b'NULL argument' in lib.mjhmc_last_error()
    for c in (0.0, -1.0, float('nan'), float('inf'), -float('inf')):
        assert lib.mjhmc_stein_create(fake, c, ctypes.byref(out)) == -1, c
        assert b'c must be finite and > 0' in lib.mjhmc_last_error(), c
    assert out.value is None
    assert lib.mjhmc_stein_evaluate(None, 0, -1, 1, four) == -1 and b'NULL argument' in lib.mjhmc_last_error()
    assert lib.mjhmc_stein_evaluate(fake, 0, -1, 1, None) == -1 and b'NULL argument' in lib.mjhmc_last_error()
    assert lib.mjhmc_stein_destroy(None) == 0


def test_stein_discrepancy_arithmetic_on_synthetic_sums():
    from mjhmc_amd.samplers.markov_jump_hmc import SteinDiscrepancy
    W = np.array([4.0, 3.0, 2.5, 1.0])
    W2 = np.array([4.0, 5.0, 6.25, 1.0])        # [2]: one particle of weight 2.5, [3]: one of weight 1 -> W^2 == W2
    S = np.array([8.0, -0.5, 3.0, 0.75])
    Sd = np.array([2.0, 1.5, 3.0, 0.75])
    r = SteinDiscrepancy([0, 2, 4, 6], W, W2, S, Sd, n_particles=4, c=1.5)
    assert r.iterations.tolist() == [0, 2, 4, 6] and r.n_particles == 4 and r.c == 1.5
    assert np.array_equal(r.v, S / (W * W))
    assert np.array_equal(r.ksd, np.sqrt(np.maximum(S / (W * W), 0.0))) and r.ksd[1] == 0.0
    assert r.u[0] == (8.0 - 2.0) / (16.0 - 4.0) and r.u[1] == (-0.5 - 1.5) / (9.0 - 5.0)
    assert np.isnan(r.u[2]) and np.isnan(r.u[3])
    assert r.mean_u == np.mean([r.u[0], r.u[1]])
    for a in (r.W, r.W2, r.S, r.Sd, r.v, r.u, r.ksd):
        assert isinstance(a, np.ndarray) and a.dtype == np.float64 and a.shape == (4,)
    one = SteinDiscrepancy([0], [2.0], [4.0], [1.0], [1.0], 1, 1.0)
    assert np.isnan(one.u[0]) and np.isnan(one.mean_u) and one.v[0] == 0.25


def _bare(nbatch=6, ndims=4, dist=None, comm=None):
    """a sampler without a device: anything that touched it would raise AttributeError, not ValueError"""
    from mjhmc_amd.samplers.markov_jump_hmc import HMCBase
    from mjhmc_amd.misc.distributions import TestGaussian
    s = HMCBase.__new__(HMCBase)
    s._dev, s.ndims, s.nbatch, s._comm = None, ndims, nbatch, comm
    s.distribution = dist if dist is not None else TestGaussian(ndims=ndims, nbatch=nbatch)
    return s


def test_every_value_error_of_the_driver_comes_before_any_device_work():
    from mjhmc_amd.misc.distributions import LambdaDistribution
    s = _bare()
    for kw in (dict(n_iter=0), dict(n_iter=-3), dict(n_iter=4, every=0), dict(n_iter=4, particles=0), dict(n_iter=4, particles=7),
               dict(n_iter=4, c=0.0), dict(n_iter=4, c=-1.0), dict(n_iter=4, c=float('nan')), dict(n_iter=4, c=float('inf'))):
        with pytest.raises(ValueError):
            s.stein_discrepancy(**kw)
    with pytest.raises(ValueError, match='n_iter must be >= 1'):
        s.stein_discrepancy(0)
    with pytest.raises(ValueError, match='every must be >= 1'):
        s.stein_discrepancy(3, every=0)
    with pytest.raises(ValueError, match=r'particles must be in \[1, nbatch = 6\]'):
        s.stein_discrepancy(3, particles=7)
    with pytest.raises(ValueError, match='c must be finite and > 0'):
        s.stein_discrepancy(3, c=0.0)
    A = np.array([[2.0, 0.5], [0.5, 1.0]])
    d = LambdaDistribution(energy_func=lambda X: 0.5 * np.sum(X * A.dot(X), axis=0).reshape(1, -1),
                           energy_grad_func=lambda X: A.dot(X), init=np.ones((2, 5)), name='dense quadratic')
    assert d.device_energy()[0] == _lib.E_HOST
    with pytest.raises(ValueError, match='opaque Python callables'):
        _bare(nbatch=5, ndims=2, dist=d).stein_discrepancy(3)
    with pytest.raises(ValueError, match='sharded sampler'):
        _bare(comm=object()).stein_discrepancy(3)
    # right arguments pass the checks and reach the device (there is none here)
    with pytest.raises(AttributeError):
        s._dwell_weighted = False
        s.stein_discrepancy(3, every=2, particles=6, c=1.0)


def test_sources_are_wired_into_the_build():
    mk = open(os.path.join(CSRC, 'Makefile')).read()
    for var in ('SRCS', 'ASAN_SRCS'):
        m = re.search(r'^%s\s*=\s*(.*)$' % var, mk, flags=re.M)
        assert m and 'stein.hip' in m.group(1).split(), var
    assert mk.count('stein.hpp') == 3        # a dependency of all three object rules
    for name in ('stein.hip', 'stein.hpp'):
        assert os.path.exists(os.path.join(CSRC, name)), name
    assert 'stein_free_all(s)' in open(os.path.join(CSRC, 'api.hip')).read()


def test_the_kernel_has_no_float_atomics_and_no_contraction():
    hpp = open(os.path.join(CSRC, 'stein.hpp')).read()
    head = hpp[:hpp.index('#pragma once')]
    assert '-ffp-contract=off' in head and 'gg*t - t^3*dd + ndims*t^3 - 3*t^5*r2' in head
    assert '-ffp-contract=off' in open(os.path.join(CSRC, 'Makefile')).read()
    code = re.sub(r'//[^\n]*', '', hpp)
    assert '#pragma clang fp contract(off)' in code
    assert 'atomicAdd' not in code and 'fma(' not in code and 'pow(' not in code and 'exp(' not in code and 'log(' not in code
    assert set(re.findall(r'atomic\w+', code)) == {'atomicOr'}
