#!/usr/bin/env python
"""Registers, spills and scratch of lin_values_kernel<NB> (csrc/dense_lin_values.hpp) as hipcc compiles the source
linear_energy.hip generates, at the library's flags, for NB = 1, 2, 4: the table of DESIGN.md section 3.3n.  No GPU needed.

    python tools/influence_regs.py [--value 'expr'] [--out DIR]

The source text below restates linear_values_source() (csrc/linear_energy.hip); keep the two in step."""
import argparse
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'mjhmc_amd', 'csrc')
VALUES = {
    'u': 'u',
    'glm logistic l': '-(q[1] != 0.f ? ((u > 20.f ? u : log1pf(expf(u))) - q[0]*u) : (0.5f*u*u))',
}


def source(value, nb):
    s = '#include "dense_lin_values.hpp"\nnamespace mjhmc {\nstruct LvUserH {\n'
    s += '  static __device__ __forceinline__ float h(float u, int j, const float* __restrict__ p, LinQ q) {\n'
    s += '    (void)u; (void)j; (void)p; (void)q;\n'
    s += '    return (float)(%s);\n  }\n};\n' % value
    s += 'template <int NB>\n__global__ __launch_bounds__(256, 1) void lin_values_kernel(const LvArgs a, const LinTallModel tm, const PotLinear lin) {\n'
    s += '  __shared__ Shared<NB> sh;\n  __shared__ double wts[kP];\n  lin_values_tiles<NB, LvUserH>(a, tm, lin, sh, wts);\n}\n'
    s += 'template __global__ void lin_values_kernel<%d>(const LvArgs, const LinTallModel, const PotLinear);\n' % nb
    s += '}  // namespace mjhmc\n'
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--value', default=None, help='one value expression (default: u and the logistic log-likelihood)')
    ap.add_argument('--out', default=None, help='keep the sources and the assembly here')
    a = ap.parse_args()
    flags = subprocess.check_output(['make', '-s', '-C', CSRC, 'print-flags']).decode().split()
    values = {'value': a.value} if a.value else VALUES
    out = a.out or tempfile.mkdtemp()
    os.makedirs(out, exist_ok=True)
    print('| value | NB | VGPRs | AGPRs | spilled VGPRs | spilled SGPRs | scratch bytes | LDS bytes |')
    print('|---|---|---|---|---|---|---|---|')
    for name, value in values.items():
        for nb in (1, 2, 4):
            tag = re.sub(r'\W+', '_', name) + '_nb%d' % nb
            src = os.path.join(out, tag + '.hip')
            with open(src, 'w') as f:
                f.write(source(value, nb))
            asm = os.path.join(out, tag + '.s')
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
