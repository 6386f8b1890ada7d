"""No GPU needed: the argument checks of the estimator entry points (include/mjhmc_hip.h: mjhmc_estimator_*,
mjhmc_ring_copy), the arithmetic of the result object, and where the new code is wired in."""
import ctypes
import os
import re

import numpy as np
import pytest

from mjhmc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_null_handles_are_refused_with_a_message(lib):
    h = ctypes.c_void_p()
    W, n = ctypes.c_double(), ctypes.c_int64()
    buf = np.zeros(4)
    calls = [
        lambda: lib.mjhmc_estimator_create(None, 0, ctypes.byref(h)),
        lambda: lib.mjhmc_estimator_create(None, 1, None),
        lambda: lib.mjhmc_estimator_set_shift(None, None),
        lambda: lib.mjhmc_estimator_accumulate(None, 0, -1, 1),
        lambda: lib.mjhmc_estimator_read(None, ctypes.byref(W), _lib.ptr(buf), _lib.ptr(buf), None, ctypes.byref(n)),
        lambda: lib.mjhmc_estimator_reset(None),
        lambda: lib.mjhmc_ring_copy(None, 0, 1),
    ]
    for call in calls:
        assert call() == -1
        assert b'NULL' in lib.mjhmc_last_error()
    assert lib.mjhmc_estimator_destroy(None) == 0
    assert lib.mjhmc_abi_version() == 2


def test_test_hook_is_not_in_the_shipped_library(lib):
    assert not hasattr(lib, 'mjhmc_test_ring_write_dwell')
    assert b'mjhmc_test_ring_write_dwell' not in open(_lib.LIB_PATH, 'rb').read()


def test_expectations_object_is_about_the_true_mean_whatever_the_shift():
    from mjhmc_amd.samplers.markov_jump_hmc import Expectations
    rs = np.random.RandomState(0)
    D, M = 4, 500
    x = rs.randn(M, D) * [1, 2, 0.5, 3] + [10, -4, 0, 2]
    w = rs.rand(M) + 0.1
    mean = (w[:, None] * x).sum(0) / w.sum()
    cov = (w[:, None, None] * (x - mean)[:, :, None] * (x - mean)[:, None, :]).sum(0) / w.sum()
    for c in (np.zeros(D), np.array([9.0, -3.0, 1.0, 0.0])):
        xc = x - c
        ex = Expectations(w.sum(), (w[:, None] * xc).sum(0), (w[:, None] * xc * xc).sum(0),
                          np.einsum('m,md,me->de', w, xc, xc), M, c)
        assert np.allclose(ex.mean, mean, rtol=0, atol=1e-12)
        assert np.allclose(ex.cov, cov, rtol=1e-9, atol=1e-9) and np.allclose(ex.var, np.diag(cov), rtol=1e-9, atol=1e-9)
        assert ex.total_weight == w.sum() and ex.n_states == M
    assert Expectations(2.0, np.ones(3), np.ones(3), None, 2, np.zeros(3)).cov is None


def test_host_energy_and_discrete_samplers_share_the_driver():
    from mjhmc_amd.samplers import markov_jump_hmc as M
    assert M.HMCBase._dwell_weighted is False and M.ControlHMC._dwell_weighted is False
    assert M.ContinuousTimeHMC._dwell_weighted is True and M.MarkovJumpHMC._dwell_weighted is True
    from mjhmc_amd.misc import gen_mj_init
    assert 'EMBEDDED' in gen_mj_init.weighted_variance.__doc__


def test_sources_are_wired_in():
    mk = open(os.path.join(ROOT, 'mjhmc_amd', 'csrc', 'Makefile')).read()
    for var in ('SRCS', 'ASAN_SRCS', 'HOOKS_SRCS'):
        line = re.search(r'^%s\s*=(.*)$' % var, mk, flags=re.M).group(1)
        assert 'estimators.hip' in line, var
    src = open(os.path.join(ROOT, 'mjhmc_amd', 'csrc', 'estimators.hip')).read()
    assert 'atomicAdd' not in src                      # fixed-order folds only: bit-identical from run to run
    assert '__builtin_amdgcn_mfma_f64_16x16x4f64' in src
