"""The test build's switches reach the code that reads them: every translation unit of csrc/ that calls test_env() or
mentions MJHMC_TEST_HOOKS is compiled with -DMJHMC_TEST_HOOKS into libmjhmc_hip_test.so (the Makefile's HOOKS_SRCS, or
HOOKS_ONLY for the units of the test build alone).  A unit left out would read every switch as unset, and the A/B
equality tests (test_gpu_fused.py, test_gpu_dense_parity.py) would compare a path with itself and pass."""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'mjhmc_amd', 'csrc')


def makefile_list(var):
    mk = open(os.path.join(CSRC, 'Makefile')).read()
    return re.search(r'^%s\s*=\s*(.*)$' % var, mk, flags=re.M).group(1).split()


def test_every_unit_with_a_hook_is_built_with_the_define():
    hooked = makefile_list('HOOKS_SRCS') + makefile_list('HOOKS_ONLY')
    units = sorted(glob.glob(os.path.join(CSRC, '*.hip')))
    assert units
    with_hooks = [os.path.basename(u) for u in units
                  if re.search(r'test_env\(|MJHMC_TEST_HOOKS', open(u).read())]
    assert 'iterate.hip' in with_hooks and 'api.hip' in with_hooks      # the schedules' switches, the shape switches
    missing = [u for u in with_hooks if u not in hooked]
    assert not missing, missing


def test_every_hooked_unit_is_a_unit_of_the_library():
    srcs = makefile_list('SRCS')
    assert [u for u in makefile_list('HOOKS_SRCS') if u not in srcs] == []
    for u in makefile_list('HOOKS_SRCS') + makefile_list('HOOKS_ONLY'):
        assert os.path.exists(os.path.join(CSRC, u)), u


def test_the_switch_has_internal_linkage():
    """test_env() is defined in a header under the define: with external linkage the linker could hand the empty form of
    a unit built without the define to a unit built with it"""
    hpp = open(os.path.join(CSRC, 'sampler_internal.hpp')).read()
    forms = re.findall(r'^(.*)\btest_env\(const char\*.*\{', hpp, flags=re.M)
    assert len(forms) == 2 and all(f.strip().startswith('static inline') for f in forms), forms
