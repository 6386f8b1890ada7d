"""CPU: the one cached hipRTC compile behind the generated kernels (rtc_compile_cached, csrc/user_expr.hip) -- what each of
its seven callers says when the caller's expression does not compile, and, through the test build's MJHMC_RTC_KEEP hook
(the sources it keeps are what tools/isa_equal.py --rtc compiles), that a source is compiled once per process and
instantiation.  No device: the *_check entry points compile and stop."""
import ctypes
import os
import re

import pytest

from mjhmc_amd import _lib

ERR_INVALID = -1     # include/mjhmc_hip.h
HDR = _lib.KERNEL_HEADERS.encode()

# (entry point, arguments in front of the include directory, the words in front of the compiler's log): `v` is declared nowhere
FAILURES = [
    ('mjhmc_linear_check', (10, 10, b'0.5f*u*v', b'u'), b'the energy expressions do not compile:\n'),
    ('mjhmc_linear_tall_check', (10, 600, b'0.5f*u*v', b'u'), b'the energy expressions do not compile:\n'),
    ('mjhmc_linear_grouped_check', (10, 600, 2, 40, b'0.5f*u*u', b'v'), b'the energy expressions do not compile:\n'),
    ('mjhmc_pointwise_check', (10, 600, b'u;u*v'), b'the value expressions do not compile:\n'),
    ('mjhmc_influence_check', (10, 600, b'u*v'), b'the value expression does not compile:\n'),
    ('mjhmc_functionals_check', (4, b'x*v', b'S[0]'), b'the functional expressions do not compile:\n'),
    ('mjhmc_projections_check', (4, b'u*v'), b'the link expression does not compile:\n'),
]


@pytest.mark.parametrize('entry,args,words', FAILURES, ids=[f[0] for f in FAILURES])
def test_a_compile_failure_begins_with_the_callers_own_words(entry, args, words):
    lib = _lib.load()
    assert getattr(lib, entry)(*args, HDR) == ERR_INVALID
    msg = lib.mjhmc_last_error()
    assert msg.startswith(words), msg[:80]
    assert b'undeclared' in msg and b"'v'" in msg, msg


def kept(directory):
    return sorted(os.listdir(str(directory)))


def test_a_source_is_compiled_and_kept_once_per_instantiation(tmp_path, monkeypatch):
    hooks = _lib.load_test_hooks()
    monkeypatch.setenv('MJHMC_RTC_KEEP', str(tmp_path))
    e, g = b'0.5f*u*u + 0.f*4711.f', b'u'          # (an expression of this test's own: the cache is the process's)
    assert hooks.mjhmc_linear_tall_check(10, 600, e, g, HDR) == 0, hooks.mjhmc_last_error()
    assert hooks.mjhmc_linear_tall_check(10, 600, e, g, HDR) == 0
    assert hooks.mjhmc_linear_tall_check(100, 5000, e, g, HDR) == 0          # the same instantiation: NB = 1
    first = kept(tmp_path)
    assert len(first) == 1 and re.match(r'mjhmc_linear_tall_\d{4}\.hip$', first[0]), first
    assert hooks.mjhmc_linear_tall_check(200, 600, e, g, HDR) == 0           # the same source at NB = 2
    both = kept(tmp_path)
    assert len(both) == 2 and first[0] in both, both
    texts = [open(os.path.join(str(tmp_path), f)).read() for f in both]
    keep = '__attribute__((used)) static void* const mjhmc_keep_0 = (void*)&mjhmc::lin_tall_eval_kernel<%d>;\n'
    assert sorted(t[t.index('__attribute__((used))'):] for t in texts) == [keep % 1, keep % 2]
    assert texts[0][:texts[0].index('__attribute__((used))')] == texts[1][:texts[1].index('__attribute__((used))')]
    # the shipped library has no such switch
    assert _lib.load().mjhmc_linear_tall_check(10, 600, b'0.5f*u*u + 0.f*4712.f', g, HDR) == 0
    assert kept(tmp_path) == both


@pytest.mark.parametrize('D', [128, 129, 256, 257, 512])
def test_the_tall_and_the_grouped_form_pad_alike(D, tmp_path, monkeypatch):
    """one pad of ndims (tall_pad, csrc/linear_energy.hip) behind both: the tall check instantiates its kernel for P / 128
    blocks of columns, and a grouped model of one block has P slots"""
    hooks = _lib.load_test_hooks()
    monkeypatch.setenv('MJHMC_RTC_KEEP', str(tmp_path))
    assert hooks.mjhmc_linear_tall_check(D, 600, b'0.5f*u*u + 0.f*%d.f' % (4800 + D), b'u', HDR) == 0, hooks.mjhmc_last_error()
    name, = kept(tmp_path)
    nb = int(re.search(r'&mjhmc::lin_tall_eval_kernel<(\d)>;', open(os.path.join(str(tmp_path), name)).read()).group(1))
    slots = ctypes.c_int64(0)
    assert hooks.mjhmc_linear_grouped_layout(D, 2, 2, 1, None, ctypes.byref(slots)) == 0, hooks.mjhmc_last_error()
    assert slots.value == 128 * nb == (128 if D <= 128 else 256 if D <= 256 else 512)
