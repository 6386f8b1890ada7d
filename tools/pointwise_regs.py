#!/usr/bin/env python
"""Registers, spills and scratch of lin_pointwise_kernel<NB> (csrc/dense_lin_pointwise.hpp) as hipcc compiles the source
linear_energy.hip generates, at the library's flags, for NB = 1, 2, 4: the table of DESIGN.md section 3.3m.  No GPU needed.

    python tools/pointwise_regs.py [--values 'expr;expr'] [--out DIR]

The source text below restates linear_pointwise_source() (csrc/linear_energy.hip); keep the two in step."""
import argparse
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'mjhmc_amd', 'csrc')
SOFTPLUS = 'u > 20.f ? u : log1pf(expf(u))'
SETS = {
    'glm logistic (l, fitted)': ['-(q[1] != 0.f ? ((u > 20.f ? u : log1pf(expf(u))) - q[0]*u) : (0.5f*u*u))',
                                 'q[1] != 0.f ? (1.f/(1.f + expf(-u))) : 0.f'],
    'u, softplus': ['u', SOFTPLUS],
    '4 values': ['u', SOFTPLUS, 'expf(u)', 'q[0]*u*u'],
}


def source(values, nb):
    s = '#include "dense_lin_pointwise.hpp"\nnamespace mjhmc {\nstruct PwUserH {\n'
    s += '  static constexpr int kM = %d;\n  template <int MI>\n' % len(values)
    s += '  static __device__ __forceinline__ float h(float u, int j, const float* __restrict__ p, LinQ q) {\n'
    s += '    (void)u; (void)j; (void)p; (void)q;\n'
    for m, v in enumerate(values):
        s += '    %sif constexpr (MI == %d) return (float)(%s);\n' % ('else ' if m else '', m, v)
    s += '    else return 0.f;\n  }\n};\n'
    s += 'template <int NB>\n__global__ __launch_bounds__(256, 1) void lin_pointwise_kernel(const PwArgs a, const LinTallModel tm, const PotLinear lin) {\n'
    s += '  __shared__ Shared<NB> sh;\n  __shared__ double wts[kP];\n  lin_pointwise_items<NB, PwUserH>(a, tm, lin, sh, wts);\n}\n'
    s += 'template __global__ void lin_pointwise_kernel<%d>(const PwArgs, const LinTallModel, const PotLinear);\n' % nb
    s += '}  // namespace mjhmc\n'
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--values', default=None, help="';'-separated value expressions (default: three sets)")
    ap.add_argument('--out', default=None, help='keep the sources and the assembly here')
    a = ap.parse_args()
    flags = subprocess.check_output(['make', '-s', '-C', CSRC, 'print-flags']).decode().split()
    sets = {'values': a.values.split(';')} if a.values else SETS
    out = a.out or tempfile.mkdtemp()
    os.makedirs(out, exist_ok=True)
    print('| values | NB | VGPRs | AGPRs | spilled VGPRs | spilled SGPRs | scratch bytes | LDS bytes |')
    print('|---|---|---|---|---|---|---|---|')
    for name, values in sets.items():
        for nb in (1, 2, 4):
            tag = re.sub(r'\W+', '_', name) + '_nb%d' % nb
            src = os.path.join(out, tag + '.hip')
            with open(src, 'w') as f:
                f.write(source(values, nb))
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
