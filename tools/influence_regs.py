#!/usr/bin/env python
"""Registers, spills and scratch of lin_values_kernel<NB> (csrc/dense_lin_values.hpp) as hipcc compiles the source
linear_energy.hip generates, at the library's flags, for NB = 1, 2, 4: the table of DESIGN.md section 3.3n.  No GPU needed.

    python tools/influence_regs.py [--value 'expr'] [--out DIR]

The source is the library's own text: the test build keeps what it hands to hipRTC (MJHMC_RTC_KEEP, tools/rtc_sources.py)."""
import argparse
import os
import re
import subprocess
import tempfile

import rtc_sources

CSRC = os.path.join(rtc_sources.ROOT, 'mjhmc_amd', 'csrc')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--value', default=None, help='one value expression (default: u and the logistic log-likelihood)')
    ap.add_argument('--out', default=None, help='keep the sources and the assembly here')
    a = ap.parse_args()
    flags = subprocess.check_output(['make', '-s', '-C', CSRC, 'print-flags']).decode().split()
    sets = {'value': a.value} if a.value else rtc_sources.INFLUENCE_VALUES
    out = a.out or tempfile.mkdtemp()
    lib = rtc_sources.load()
    print('| value | NB | VGPRs | AGPRs | spilled VGPRs | spilled SGPRs | scratch bytes | LDS bytes |')
    print('|---|---|---|---|---|---|---|---|')
    for name, value in sets.items():
        for nb, ndims in rtc_sources.NB_DIMS.items():
            src, = rtc_sources.keep(lib, out, 'mjhmc_influence_check', ndims, rtc_sources.TALL_K, value)
            asm = src[:-4] + '.s'
            subprocess.check_call([os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')] + flags +
                                  ['--cuda-device-only', '-S', '-I', CSRC, src, '-o', asm])
            text = open(asm).read()

            def field(key):
                m = re.search(r'^\s*' + re.escape(key) + r':?\s+(\d+)', text, flags=re.M)
                return m.group(1) if m else '?'
            print('| %s | %d | %s | %s | %s | %s | %s | %s |' % (
                name, nb, field('.vgpr_count'), field('.agpr_count'), field('.vgpr_spill_count'), field('.sgpr_spill_count'),
                field('.private_segment_fixed_size'), field('.group_segment_fixed_size')))


if __name__ == '__main__':
    main()
