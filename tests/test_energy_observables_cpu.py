"""CPU: what of the energy observables needs no device -- the new export in header, bindings and library, its argument
refusals, the ``EnergyObservables`` description and the drivers' argument checks with it, the arithmetic of ``Temperature``
on a synthetic ``Diagnostics``, and the wiring of csrc/energy_observables.hip into the build."""
import ctypes
import os
import re

import numpy as np
import pytest

from mjhmc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'mjhmc_amd', 'csrc')
NEW = 'mjhmc_functionals_create_energy'


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_header_bindings_and_library_agree_on_the_export(lib):
    from mjhmc_amd import engine
    from mjhmc_amd.samplers.markov_jump_hmc import HMCBase, EnergyObservables, Temperature  # noqa: F401
    header = open(os.path.join(ROOT, 'include', 'mjhmc_hip.h')).read()
    m = re.search(r'/\*((?:(?!\*/).)*)\*/\s*int\s+%s\s*\(\s*mjhmc_sampler\s*\*\s*s\s*,\s*mjhmc_functionals\s*\*\*\s*out\s*\)\s*;' % NEW,
                  header, flags=re.S)
    assert m, 'the export is declared with a doc comment'
    for word in ('grad_sq', 'virial', 'MJHMC_E_HOST'):
        assert word in m.group(1), word
    assert re.search(r'#define\s+MJHMC_ABI_VERSION\s+2\b', header) and lib.mjhmc_abi_version() == 2
    restype, argtypes = _lib.PROTOTYPES[NEW]
    assert restype is ctypes.c_int and len(argtypes) == 2
    assert getattr(lib, NEW).argtypes is not None and len(getattr(lib, NEW).argtypes) == 2   # resolved and declared by load()
    assert callable(engine.DeviceSampler.energy_observables) and callable(engine.DeviceFunctionals.energy)
    assert callable(HMCBase.energy_observables) and callable(HMCBase.temperature)
    assert not hasattr(engine, 'DeviceEnergyObservables'), 'one handle class: DeviceFunctionals has the alternate constructor'


def test_null_arguments_are_refused_with_a_message(lib):
    out = ctypes.c_void_p()
    fake = ctypes.c_void_p(1)                     # never dereferenced: the NULL check comes before the handle is touched
    assert getattr(lib, NEW)(None, ctypes.byref(out)) == -1 and b'NULL argument' in lib.mjhmc_last_error()
    assert getattr(lib, NEW)(fake, None) == -1 and b'NULL argument' in lib.mjhmc_last_error()
    assert getattr(lib, NEW)(None, None) == -1 and b'NULL argument' in lib.mjhmc_last_error()
    assert out.value is None


def test_description_object():
    from mjhmc_amd.samplers.markov_jump_hmc import HMCBase, EnergyObservables
    from mjhmc_amd.misc.distributions import TestGaussian
    s = HMCBase.__new__(HMCBase)
    s._dev, s.ndims, s.distribution = None, 4, TestGaussian(ndims=4, nbatch=3)
    EO = s.energy_observables()
    assert isinstance(EO, EnergyObservables)
    assert EO.n_values == 3 and EO.names == ['E', 'grad_sq', 'virial']
    for N, Npad in ((1, 64), (64, 64), (65, 128), (200, 256)):
        assert EO.slot_bytes(N) == Npad * 4 * 8


def test_a_host_energy_is_refused_before_anything_runs():
    from mjhmc_amd.samplers.markov_jump_hmc import HMCBase
    from mjhmc_amd.misc.distributions import LambdaDistribution
    A = np.array([[2.0, 0.5], [0.5, 1.0]])
    d = LambdaDistribution(energy_func=lambda X: 0.5 * np.sum(X * A.dot(X), axis=0).reshape(1, -1),
                           energy_grad_func=lambda X: A.dot(X), init=np.ones((2, 5)), name='dense quadratic')
    assert d.device_energy()[0] == _lib.E_HOST
    s = HMCBase.__new__(HMCBase)
    s._dev, s.ndims, s.distribution = None, 2, d          # no device: anything that touched it would raise AttributeError
    with pytest.raises(ValueError, match='opaque Python callables'):
        s.energy_observables()
    with pytest.raises(ValueError, match='opaque Python callables'):
        s.temperature(8)


def test_of_argument_checks_come_before_any_device_work():
    """a sampler whose ``_dev`` is None: anything that touched the device would raise AttributeError, not ValueError"""
    from mjhmc_amd.samplers.markov_jump_hmc import HMCBase, EnergyObservables
    s = HMCBase.__new__(HMCBase)
    s._dev, s.ndims = None, 4
    EO = EnergyObservables()
    with pytest.raises(ValueError, match='n_values = 3'):
        s.expectations(5, of=EO, shift=np.zeros(4))        # ndims entries: wrong for K = 3
    with pytest.raises(ValueError, match='n_values = 3'):
        s.diagnostics(8, of=EO, shift=np.zeros(4))
    with pytest.raises(ValueError, match='n_values = 3'):
        s.marginals(5, of=EO, range=(np.zeros(4), np.ones(4)))
    with pytest.raises(ValueError):
        s.marginals(5, of=EO, range=(np.zeros(3), np.array([1.0, 0.0, 1.0])))
    with pytest.raises(ValueError, match='n_values = 3'):
        s.joint_marginals(5, pairs=[(0, 2)], of=EO, range=(np.zeros(4), np.ones(4)))
    with pytest.raises(ValueError):
        s.joint_marginals(5, pairs=[(0, 3)], of=EO)        # value 3 does not exist
    for call in (lambda: s.expectations(0, of=EO), lambda: s.diagnostics(5, of=EO), lambda: s.marginals(3, bins=0, of=EO)):
        with pytest.raises(ValueError):
            call()
    # a right-sized argument passes the checks and reaches the device (there is none here)
    with pytest.raises(AttributeError):
        s._dwell_weighted = False
        s.expectations(5, of=EO, shift=np.zeros(3))


def test_temperature_arithmetic_on_a_synthetic_diagnostics():
    """Diagnostics from hand-made per-chain sums of K = 3 values (two parts of 5 chains, 40 states each); T, stderr and z
    are the docstring's formulas on its fields, to the last bit"""
    from mjhmc_amd.samplers.markov_jump_hmc import Diagnostics, Temperature
    rs = np.random.RandomState(4)
    ndims, M, n = 17, 5, 40
    shift = np.array([9.0, 30.0, 16.5])
    parts = []
    for h in range(2):
        m = rs.randn(M, 3) * np.array([0.3, 1.0, 0.4]) + np.array([0.1, -0.5, 0.6])     # chain means about the shift
        v = rs.rand(M, 3) * np.array([8.0, 60.0, 30.0]) + 1.0                            # chain variances
        parts.append((M, n, float(M * n), m.sum(axis=0), (m * m).sum(axis=0), v.sum(axis=0)))
    d = Diagnostics(parts, shift, grad_evals=1234)
    t = Temperature(d, ndims)
    assert t.diagnostics is d and t.ndims == 17
    T = d.mean[2] / 17
    stderr = np.sqrt(d.var_plus[2] / d.ess[2]) / 17
    assert t.T == T and t.stderr == stderr and t.z == (T - 1) / stderr
    assert t.mean_energy == d.mean[0] and t.mean_grad_sq == d.mean[1] and t.rhat_energy == d.rhat[0]
    # the same from the raw sums, spelled out: the formulas of the Diagnostics docstring
    Mtot = 10
    cma = sum(p[3] for p in parts)[2] / Mtot
    between = (sum(p[4] for p in parts)[2] - Mtot * cma * cma) / (Mtot - 1)
    var_plus = sum(p[5] for p in parts)[2] / Mtot + between
    ess = Mtot * (var_plus / between)
    assert t.T == (shift[2] + cma) / 17 and t.stderr == np.sqrt(var_plus / ess) / 17
    assert np.isfinite(t.z) and 0.9 < t.T < 1.1 and t.stderr > 0


def test_sources_are_wired_into_all_three_object_lists():
    mk = open(os.path.join(CSRC, 'Makefile')).read()
    for var in ('SRCS', 'ASAN_SRCS', 'HOOKS_SRCS'):
        m = re.search(r'^%s\s*=\s*(.*)$' % var, mk, flags=re.M)
        assert m and 'energy_observables.hip' in m.group(1).split(), var
    assert mk.count('energy_observables.hpp') == 3        # a dependency of all three object rules
    for name in ('energy_observables.hip', 'energy_observables.hpp'):
        assert os.path.exists(os.path.join(CSRC, name)), name


def test_the_kernel_uses_no_lds_and_no_float_atomics():
    hpp = open(os.path.join(CSRC, 'energy_observables.hpp')).read()
    assert '-ffp-contract=off' in hpp[:hpp.index('#pragma once')], 'the header comment states the flag the kernel relies on'
    assert '-ffp-contract=off' in open(os.path.join(CSRC, 'Makefile')).read()
    code = re.sub(r'//[^\n]*', '', hpp)
    assert 'atomicAdd' not in code and 'fma(' not in code and '__shared__' not in code
    assert re.findall(r'atomic\w+', code) == ['atomicOr']
