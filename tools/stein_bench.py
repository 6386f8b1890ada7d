"""Time the kernel Stein discrepancy pass (csrc/stein.hpp) alone, against its arithmetic floor and against a slot evaluation.

For each shape (bench.py WORKLOADS c2: iso Gaussian 512 dims fp64; c4: Neal funnel 32 dims fp64) a sampler of the TEST build
of the library with max(--particles) particles records one ring slot with its own iterations; then, for each entry of
--particles (the prefix n_use of the pass):
  DeviceStein.evaluate -- the slot's evaluation launches, the pair kernel, the finish kernel and the 40-byte read-back --
  and the slot's evaluation launches alone (mjhmc_test_energy_observables_part, part 0: the same sampler_eval_rows call into
  an energy-observables handle's scratch), --inner calls per timed window, host clock around calls that end in a device
  synchronise, median of --reps repetitions after one warm-up.  pair_ms = evaluate_ms - evaluation_ms is the pair and finish
  kernels plus the read-back: a difference of two host timings, not a kernel time (no profiler run here).
The floor is the issue's: n_use^2 / 2 * ndims * 5 float64 vector instructions at the float64 vector peak (78.6 TFLOP/s = 39.3e12
lane-instructions/s, an fma counted as two flops).  The kernel as written issues 8 per (pair, d) -- 2 subtractions, 3 products,
3 sums, no contraction -- and computes diagonal tiles as full squares, so floor / pair_ms <= 5 / 8 by construction.
Writes one JSON line per (shape, particles); with --out also a markdown table.
usage: python tools/stein_bench.py [--only c2,c4] [--particles 8192,32768] [--reps 5] [--inner 2] [--out profiles/r15/stein.md]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from chainstats_bench import timed, repeated                              # noqa: E402
from energy_observables_bench import hooks_device, rounded                # noqa: E402
from mjhmc_amd import engine                                              # noqa: E402

F64_LANE_INSTR_PER_S = 78.6e12 / 2


def floor_seconds(n_use, ndims):
    return n_use * n_use / 2.0 * ndims * 5 / F64_LANE_INSTR_PER_S


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', default='c2,c4')
    ap.add_argument('--particles', default='8192,32768')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--inner', type=int, default=2, help='calls per timed window')
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    parts = [int(p) for p in args.particles.split(',')]
    recs = []
    for key in [k for k in args.only.split(',') if k]:
        ctx, dev, w, N = hooks_device(key, max(parts), 2)
        lib = ctx.lib
        D = w['D']
        c = float(np.sqrt(D))
        st = dev.stein(c)
        eo = dev.energy_observables()
        eo.ring_alloc(1)

        def evaluation():
            engine.check(lib.mjhmc_test_energy_observables_part(eo.handle, 0, 1, 0, 0), lib)
        t_eval = timed(repeated(evaluation, args.inner), args.reps) / args.inner
        for n_use in parts:
            vals = st.evaluate(0, 1, n_use)
            assert st.evaluate(0, 1, n_use) == vals, 'two evaluations differ'
            t_all = timed(repeated(lambda: st.evaluate(0, 1, n_use), args.inner), args.reps) / args.inner
            W, W2, S, Sd = vals
            fl = floor_seconds(n_use, D)
            pair = t_all - t_eval
            rec = dict(workload=key, D=D, N=N, dtype=w['dtype'], n_use=n_use, c=c, reps=args.reps, inner=args.inner,
                       evaluate_ms=1e3 * t_all, evaluation_ms=1e3 * t_eval, pair_ms=1e3 * pair, floor_ms=1e3 * fl,
                       floor_over_pair=fl / pair, pair_over_evaluation=pair / t_eval,
                       pairs_per_s=n_use * (n_use + 1) / 2.0 / pair, v=S / (W * W), u=(S - Sd) / (W * W - W2))
            recs.append(rec)
            print(rounded(rec), flush=True)
        st.close()
        eo.close()
        dev.close()
        del dev
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('# Kernel Stein discrepancy: the pass alone (tools/stein_bench.py)\n\n')
            f.write('One job on one MI355X; host clock around calls that end in a device synchronise, median of %d repetitions of '
                    '%d calls after a warm-up.  `evaluate` = slot evaluation + pair kernel + finish kernel + read-back; '
                    '`evaluation` = the slot evaluation launches alone; `pair` = their difference (not a profiler kernel time).  '
                    'Floor: n_use^2 / 2 x ndims x 5 float64 vector instructions at 39.3e12 lane-instructions/s (78.6 TFLOP/s).  '
                    'The kernel issues 8 per (pair, d) without contraction.\n\n' % (args.reps, args.inner))
            f.write('| shape | ndims | n_use | evaluate ms | evaluation ms | pair ms | floor ms | floor / pair | pair / evaluation |\n')
            f.write('|---|---|---|---|---|---|---|---|---|\n')
            for r in recs:
                f.write('| %s | %d | %d | %.3f | %.3f | %.3f | %.3f | %.3f | %.1f |\n'
                        % (r['workload'], r['D'], r['n_use'], r['evaluate_ms'], r['evaluation_ms'], r['pair_ms'], r['floor_ms'],
                           r['floor_over_pair'], r['pair_over_evaluation']))
            f.write('\n```\n' + '\n'.join(json.dumps(r) for r in recs) + '\n```\n')


if __name__ == '__main__':
    main()
