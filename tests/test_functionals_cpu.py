"""CPU: what of the device functionals needs no device -- the hipRTC compile of the expressions (mjhmc_functionals_check),
the argument refusals of every new entry point, the bindings, the ``of=`` argument checks of the drivers, and the wiring of
csrc/functionals.hip into the build."""
import ctypes
import os
import re

import numpy as np
import pytest

from mjhmc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'mjhmc_amd', 'csrc')
NEW = ('mjhmc_functionals_check', 'mjhmc_functionals_create', 'mjhmc_functionals_destroy', 'mjhmc_functionals_info',
       'mjhmc_functionals_ring_alloc', 'mjhmc_functionals_evaluate', 'mjhmc_functionals_read', 'mjhmc_estimator_create_on',
       'mjhmc_chainstats_create_on', 'mjhmc_histogram_create_on')


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_expressions_compile_without_a_device(lib):
    inc = _lib.KERNEL_HEADERS.encode()
    # J = 0: the values are constants (stats NULL and stats empty)
    assert lib.mjhmc_functionals_check(10, None, b'1.5; 2.0 * 3.0', inc) == 0, lib.mjhmc_last_error()
    assert lib.mjhmc_functionals_check(10, b'', b'1.5', inc) == 0, lib.mjhmc_last_error()
    # the largest set, on a row wider than one wave of 16-byte chunks
    stats = b';'.join(b'd == %d ? x : 0.0' % j for j in range(8))
    values = b';'.join(b'S[%d] + %d.0' % (k % 8, k) for k in range(16))
    assert lib.mjhmc_functionals_check(130, stats, values, inc) == 0, lib.mjhmc_last_error()
    # parameters
    assert lib.mjhmc_functionals_check(3, b'x * x / (p[0] * p[0])', b'S[0] > p[1] ? 1.0 : 0.0', inc) == 0, lib.mjhmc_last_error()


def test_a_syntax_error_returns_the_compilers_text(lib):
    inc = _lib.KERNEL_HEADERS.encode()
    assert lib.mjhmc_functionals_check(4, b'x * y', b'S[0]', inc) == -1
    msg = lib.mjhmc_last_error()
    assert b'do not compile' in msg and b'undeclared' in msg and b"'y'" in msg, msg
    assert lib.mjhmc_functionals_check(4, b'x', b'S[0] +', inc) == -1
    assert b'error' in lib.mjhmc_last_error()


def test_counts_outside_the_family_are_refused_with_a_message(lib):
    inc = _lib.KERNEL_HEADERS.encode()
    assert lib.mjhmc_functionals_check(4, b';'.join([b'x'] * 9), b'S[0]', inc) == -1
    assert b'at most 8 stats (J = 9)' in lib.mjhmc_last_error()
    for values in (b'', b'  ', None):
        rc = lib.mjhmc_functionals_check(4, b'x', values, inc)
        assert rc == -1 and (b'K must be in [1, 16], got 0' in lib.mjhmc_last_error() or values is None), values
    assert lib.mjhmc_functionals_check(4, b'x', b';'.join([b'S[0]'] * 17), inc) == -1
    assert b'K must be in [1, 16], got 17' in lib.mjhmc_last_error()
    assert lib.mjhmc_functionals_check(0, b'x', b'S[0]', inc) == -1 and b'ndims must be >= 1' in lib.mjhmc_last_error()


def test_every_new_entry_point_refuses_null_and_fake_handles(lib):
    inc = _lib.KERNEL_HEADERS.encode()
    out = ctypes.c_void_p()
    fake = ctypes.c_void_p(1)                     # never dereferenced: the checks below come before the handle is touched
    assert lib.mjhmc_functionals_check(4, b'x', None, inc) == -1 and b'NULL argument' in lib.mjhmc_last_error()
    assert lib.mjhmc_functionals_check(4, b'x', b'S[0]', None) == -1 and b'NULL argument' in lib.mjhmc_last_error()
    for args in ((None, b'x', b'S[0]', None, 0, inc, ctypes.byref(out)), (fake, b'x', None, None, 0, inc, ctypes.byref(out)),
                 (fake, b'x', b'S[0]', None, 0, None, ctypes.byref(out)), (fake, b'x', b'S[0]', None, 0, inc, None)):
        assert lib.mjhmc_functionals_create(*args) == -1
        assert b'NULL argument' in lib.mjhmc_last_error()
    assert lib.mjhmc_functionals_create(fake, b'x', b'S[0]', None, 2, inc, ctypes.byref(out)) == -1
    assert b'params is NULL' in lib.mjhmc_last_error()
    # the counts are checked before the sampler is looked at
    assert lib.mjhmc_functionals_create(fake, b';'.join([b'x'] * 9), b'S[0]', None, 0, inc, ctypes.byref(out)) == -1
    assert b'at most 8 stats' in lib.mjhmc_last_error()
    assert lib.mjhmc_functionals_create(fake, b'x', b';'.join([b'1.0'] * 17), None, 0, inc, ctypes.byref(out)) == -1
    assert b'K must be in [1, 16]' in lib.mjhmc_last_error()
    assert out.value is None
    assert lib.mjhmc_functionals_destroy(None) == 0
    k, b = ctypes.c_int(), ctypes.c_uint64()
    assert lib.mjhmc_functionals_info(None, ctypes.byref(k), ctypes.byref(b)) == -1 and b'NULL argument' in lib.mjhmc_last_error()
    assert lib.mjhmc_functionals_info(fake, None, ctypes.byref(b)) == -1 and b'NULL argument' in lib.mjhmc_last_error()
    assert lib.mjhmc_functionals_ring_alloc(None, 4) == -1 and b'functionals is NULL' in lib.mjhmc_last_error()
    assert lib.mjhmc_functionals_ring_alloc(fake, 0) == -1 and b'n_slots must be >= 1' in lib.mjhmc_last_error()
    assert lib.mjhmc_functionals_evaluate(None, 0, 1, 0) == -1 and b'functionals is NULL' in lib.mjhmc_last_error()
    buf = np.zeros(4)
    assert lib.mjhmc_functionals_read(None, 0, 1, _lib.ptr(buf)) == -1 and b'NULL argument' in lib.mjhmc_last_error()
    assert lib.mjhmc_functionals_read(fake, 0, 1, None) == -1 and b'NULL argument' in lib.mjhmc_last_error()
    assert lib.mjhmc_estimator_create_on(None, 0, ctypes.byref(out)) == -1 and b'NULL argument' in lib.mjhmc_last_error()
    assert lib.mjhmc_estimator_create_on(fake, 0, None) == -1 and b'NULL argument' in lib.mjhmc_last_error()
    assert lib.mjhmc_chainstats_create_on(None, 1, ctypes.byref(out)) == -1 and b'NULL argument' in lib.mjhmc_last_error()
    assert lib.mjhmc_chainstats_create_on(fake, 1, None) == -1 and b'NULL argument' in lib.mjhmc_last_error()
    lo, hi = np.zeros(2), np.ones(2)
    for args in ((None, 16, _lib.ptr(lo), _lib.ptr(hi), 0.5, ctypes.byref(out)), (fake, 16, None, _lib.ptr(hi), 0.5, ctypes.byref(out)),
                 (fake, 16, _lib.ptr(lo), None, 0.5, ctypes.byref(out)), (fake, 16, _lib.ptr(lo), _lib.ptr(hi), 0.5, None)):
        assert lib.mjhmc_histogram_create_on(*args) == -1
        assert b'NULL argument' in lib.mjhmc_last_error()
    assert lib.mjhmc_histogram_create_on(fake, 0, _lib.ptr(lo), _lib.ptr(hi), 0.5, ctypes.byref(out)) == -1
    assert b'n_bins must be in [1, 1024]' in lib.mjhmc_last_error()
    assert lib.mjhmc_histogram_create_on(fake, 16, _lib.ptr(lo), _lib.ptr(hi), 0.3, ctypes.byref(out)) == -1
    assert b'power of two' in lib.mjhmc_last_error()
    assert out.value is None
    assert lib.mjhmc_abi_version() == 2


def test_binding_declares_the_functionals_entry_points():
    from mjhmc_amd import engine
    from mjhmc_amd.samplers.markov_jump_hmc import HMCBase, Functionals  # noqa: F401
    for name in NEW:
        assert name in _lib.PROTOTYPES, name
    header = open(os.path.join(ROOT, 'include', 'mjhmc_hip.h')).read()
    for name in NEW:
        assert re.search(r'\b%s\s*\(' % name, header), name
    assert re.search(r'#define\s+MJHMC_ABI_VERSION\s+2\b', header)
    assert hasattr(engine, 'DeviceFunctionals') and hasattr(engine.DeviceSampler, 'functionals') and hasattr(HMCBase, 'functionals')
    for name in ('ring_alloc', 'evaluate', 'read', 'estimator', 'chain_stats', 'histogram', 'close'):
        assert callable(getattr(engine.DeviceFunctionals, name)), name


def test_functionals_description_validates_before_any_run(lib):
    from mjhmc_amd.samplers.markov_jump_hmc import HMCBase, Functionals
    s = HMCBase.__new__(HMCBase)
    s._dev, s.ndims = None, 4
    F = s.functionals(['S[0] / (p[0] * p[0])', 'S[0] > 1.0 ? 1.0 : 0.0'], stats=['x * x'], params=[1.3], names=['r2', 'tail'])
    assert isinstance(F, Functionals) and F.n_values == 2 and F.names == ['r2', 'tail'] and F.stats == ['x * x']
    assert np.array_equal(F.params, [1.3]) and F.slot_bytes(65) == 128 * 2 * 8
    assert s.functionals('S[0]', stats='x').n_values == 1 and s.functionals('1.0').names == ['g0']
    with pytest.raises(ValueError, match="undeclared identifier 'q'"):
        s.functionals(['S[0] * q'], stats=['x'])
    with pytest.raises(ValueError, match='at most 8 stats'):
        s.functionals(['S[0]'], stats=['x'] * 9)
    with pytest.raises(ValueError, match=r'K must be in \[1, 16\]'):
        s.functionals(['1.0'] * 17)
    with pytest.raises(ValueError):
        s.functionals(['S[0]; S[0]'], stats=['x'])        # one expression per entry
    with pytest.raises(ValueError, match='names'):
        s.functionals(['1.0', '2.0'], names=['a'])


def test_of_argument_checks_come_before_any_device_work():
    """a sampler whose ``_dev`` is None: anything that touched the device would raise AttributeError, not ValueError"""
    from mjhmc_amd.samplers.markov_jump_hmc import HMCBase, Functionals
    s = HMCBase.__new__(HMCBase)
    s._dev, s.ndims = None, 4
    F = Functionals(['S[0]', 'S[0] * S[0]', '1.0'], stats=['x'])
    assert F.n_values == 3
    with pytest.raises(ValueError, match='n_values = 3'):
        s.expectations(5, of=F, shift=np.zeros(4))         # ndims entries: wrong for K = 3
    with pytest.raises(ValueError, match='n_values = 3'):
        s.diagnostics(8, of=F, shift=np.zeros(4))
    with pytest.raises(ValueError, match='n_values = 3'):
        s.marginals(5, of=F, range=(np.zeros(4), np.ones(4)))
    with pytest.raises(ValueError):
        s.marginals(5, of=F, range=(np.zeros(3), np.array([1.0, 0.0, 1.0])))
    # the checks that were there stay in front
    for call in (lambda: s.expectations(0, of=F), lambda: s.diagnostics(5, of=F), lambda: s.marginals(3, bins=0, of=F),
                 lambda: s.marginals(3, span=0.0, of=F)):
        with pytest.raises(ValueError):
            call()
    # a right-sized argument passes the checks and reaches the device (there is none here)
    with pytest.raises(AttributeError):
        s._dwell_weighted = False
        s.expectations(5, of=F, shift=np.zeros(3))


def test_sources_are_wired_into_the_makefile():
    mk = open(os.path.join(CSRC, 'Makefile')).read()
    for var in ('SRCS', 'ASAN_SRCS'):
        m = re.search(r'^%s\s*=\s*(.*)$' % var, mk, flags=re.M)
        assert m and 'functionals.hip' in m.group(1).split(), var
    for header in ('functionals.hpp', 'ring_source.hpp'):
        assert mk.count(header) == 3, header             # a dependency of all three object rules
        assert os.path.exists(os.path.join(CSRC, header))
    assert os.path.exists(os.path.join(CSRC, 'functionals.hip'))


def test_the_kernel_header_keeps_contraction_off_and_has_no_float_atomics():
    hpp = open(os.path.join(CSRC, 'functionals.hpp')).read()
    assert '-ffp-contract=off' in hpp[:hpp.index('#pragma once')], 'the header comment states the flag the kernel relies on'
    rtc = open(os.path.join(CSRC, 'user_expr.hip')).read()
    assert '"-ffp-contract=off"' in rtc
    code = re.sub(r'//[^\n]*', '', hpp)
    assert 'atomicAdd' not in code and 'fma(' not in code and '__shared__' not in code
    assert re.findall(r'atomic\w+', code) == ['atomicOr']
