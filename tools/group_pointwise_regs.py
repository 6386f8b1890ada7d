#!/usr/bin/env python
"""Registers, spills and scratch of lin_group_pointwise_kernel<NB> (csrc/dense_lin_group_pointwise.hpp) as hipcc compiles
the source linear_energy.hip generates, at the library's flags, for C in {2, 10, 16} x NB in {1, 2, 4}: the table of
DESIGN.md section 3.3o.  No GPU needed.

    python tools/group_pointwise_regs.py [--values 'expr;expr' --member MASK] [--out DIR]

The default values are one per-group log-mean-exp value and one per-member value (M = 2): q[0]*(u - lse) and sm.  The
source is the library's own text: the test build keeps what it hands to hipRTC (MJHMC_RTC_KEEP, tools/rtc_sources.py)."""
import argparse
import os
import re
import subprocess
import tempfile

import rtc_sources

CSRC = os.path.join(rtc_sources.ROOT, 'mjhmc_amd', 'csrc')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--values', default=';'.join(rtc_sources.GROUP_POINTWISE_VALUES), help="';'-separated value expressions")
    ap.add_argument('--member', type=int, default=rtc_sources.GROUP_POINTWISE_MEMBER, help='bit m: value m is per member')
    ap.add_argument('--out', default=None, help='keep the sources and the assembly here')
    a = ap.parse_args()
    flags = subprocess.check_output(['make', '-s', '-C', CSRC, 'print-flags']).decode().split()
    out = a.out or tempfile.mkdtemp()
    lib = rtc_sources.load()
    print('| C | NB | VGPRs | AGPRs | spilled VGPRs | spilled SGPRs | scratch bytes | LDS bytes |')
    print('|---|---|---|---|---|---|---|---|')
    for c in rtc_sources.GROUP_SIZES:
        for nb, ndims in rtc_sources.NB_DIMS.items():
            src, = rtc_sources.keep(lib, out, 'mjhmc_pointwise_grouped_check', ndims, 40 * c + rtc_sources.TALL_K, c, 40,
                                    a.values, a.member)
            asm = src[:-4] + '.s'
            subprocess.check_call([os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')] + flags +
                                  ['--cuda-device-only', '-S', '-I', CSRC, src, '-o', asm])
            text = open(asm).read()

            def field(key):
                m = re.search(r'^\s*' + re.escape(key) + r':?\s+(\d+)', text, flags=re.M)
                return m.group(1) if m else '?'
            print('| %d | %d | %s | %s | %s | %s | %s | %s |' % (
                c, nb, field('.vgpr_count'), field('.agpr_count'), field('.vgpr_spill_count'), field('.sgpr_spill_count'),
                field('.private_segment_fixed_size'), field('.group_segment_fixed_size')))


if __name__ == '__main__':
    main()
