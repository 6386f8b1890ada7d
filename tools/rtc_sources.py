#!/usr/bin/env python3
"""The hipRTC sources of a fixed list of instances, kept as files: what tools/isa_equal.py compile --rtc DIR compiles.

    python tools/rtc_sources.py DIR [--lib libmjhmc_hip_test.so]

Loads the test build of the library with MJHMC_RTC_KEEP=DIR (csrc/user_expr.hip: rtc_keep) and calls the device-free
*_check entry points; every source hipRTC actually compiles lands in DIR under its file name and a running number, each
followed by the lines that force its kernels' instantiation offline.  No GPU needed.  The list is fixed and walked in one
order, so two libraries that generate the same texts leave byte-identical directories.  tools/pointwise_regs.py,
tools/group_pointwise_regs.py and tools/influence_regs.py take their sources through keep() below."""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mjhmc_amd import _lib  # noqa: E402

SOFTPLUS = 'u > 20.f ? u : log1pf(expf(u))'
LOGISTIC_L = '-(q[1] != 0.f ? ((u > 20.f ? u : log1pf(expf(u))) - q[0]*u) : (0.5f*u*u))'
EXPRS = {   # softplus with a q[0] factor, and the quadratic and ProductOfT pairs of tests/test_linear_tall_cpu.py
    'softplus': ('q[0]*(%s)' % SOFTPLUS, 'q[0]/(1.f + expf(-u))'),
    'quadratic': ('0.5f*u*u', 'u'),
    'product_of_t': ('q[0]*logf(1.f + u*u)', '2.f*q[0]*u/(1.f + u*u)'),
}
POINTWISE_SETS = {   # the value sets of the table of DESIGN.md section 3.3m
    'glm logistic (l, fitted)': [LOGISTIC_L, 'q[1] != 0.f ? (1.f/(1.f + expf(-u))) : 0.f'],
    'u, softplus': ['u', SOFTPLUS],
    '4 values': ['u', SOFTPLUS, 'expf(u)', 'q[0]*u*u'],
}
GROUP_POINTWISE_VALUES = ['q[0]*(u - lse)', 'sm']   # the table of DESIGN.md section 3.3o: a row's log-likelihood (per group,
GROUP_POINTWISE_MEMBER = 2                          # log-mean-exp on) and the fitted class probabilities (per member)
GROUP_SIZES = (2, 10, 16)
INFLUENCE_VALUES = {'u': 'u', 'glm logistic l': LOGISTIC_L}   # those of the table of section 3.3n
NB_DIMS = {1: 100, 2: 200, 4: 400}   # ndims that pads to 128 NB
TALL_K = 600                         # more experts than a square model takes: the blocked layout
WIDE_D = 1000                        # more dims than a tall model takes: the wide form (one kernel whatever the sizes)


def load(path=None):
    if not path:
        return _lib.load_test_hooks()
    return _lib._attach(ctypes.CDLL(path), _lib.PROTOTYPES)


def keep(lib, out, entry, *args):
    """calls the *_check entry point with MJHMC_RTC_KEEP=out; returns the files it left (none: the source was compiled before)"""
    os.makedirs(out, exist_ok=True)
    before = set(os.listdir(out))
    os.environ['MJHMC_RTC_KEEP'] = os.path.abspath(out)
    try:
        rc = getattr(lib, entry)(*[a.encode() if isinstance(a, str) else a for a in args], _lib.KERNEL_HEADERS.encode())
    finally:
        del os.environ['MJHMC_RTC_KEEP']
    if rc:
        raise RuntimeError('%s%r: %s' % (entry, args, lib.mjhmc_last_error().decode()))
    return sorted(os.path.join(out, f) for f in set(os.listdir(out)) - before)


def instances():
    for nb, d in NB_DIMS.items():
        yield ('mjhmc_linear_check', d, d) + EXPRS['softplus']
    for nb, d in NB_DIMS.items():
        for e in EXPRS.values():
            yield ('mjhmc_linear_tall_check', d, TALL_K) + e
    for c, e in zip((2, 10, 16), EXPRS.values()):
        for nb, d in NB_DIMS.items():
            yield ('mjhmc_linear_grouped_check', d, 40 * c + TALL_K, c, 40) + e
    for values in POINTWISE_SETS.values():
        for nb, d in NB_DIMS.items():
            yield 'mjhmc_pointwise_check', d, TALL_K, ';'.join(values)
    for c in GROUP_SIZES:
        for nb, d in NB_DIMS.items():
            yield 'mjhmc_pointwise_grouped_check', d, 40 * c + TALL_K, c, 40, ';'.join(GROUP_POINTWISE_VALUES), GROUP_POINTWISE_MEMBER
    for value in INFLUENCE_VALUES.values():
        for nb, d in NB_DIMS.items():
            yield 'mjhmc_influence_check', d, TALL_K, value
    yield 'mjhmc_functionals_check', 100, 'x*x', 'S[0]; sqrt(S[0])'
    yield 'mjhmc_projections_check', 3, 'u > 0.0 ? u : 0.0'
    for e in EXPRS.values():   # (behind everything else: the running numbers of the files above stay what they were)
        yield ('mjhmc_linear_wide_check', WIDE_D, TALL_K) + e


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('out')
    ap.add_argument('--lib', default=None, help='the test build to load (default: this tree\'s libmjhmc_hip_test.so)')
    a = ap.parse_args()
    lib = load(a.lib)
    for inst in instances():
        for f in keep(lib, a.out, *inst):
            print(os.path.basename(f), inst[0], *[x for x in inst[1:] if isinstance(x, int)], flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
