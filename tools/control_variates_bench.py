"""Time the control-variate pass (csrc/crossmoments.hip) per recorded state against its yardsticks, at the benchmark's sizes.

For each workload (bench.py WORKLOADS; c2: iso Gaussian 512 x 100 000 fp64; c4: Neal funnel 32 x 1 000 000 fp64; c3:
ProductOfT 512 x 100 000 with float32 state -- c3f64, its float64-state form, runs the multi-pass path, which
mjhmc_crossmoments_create refuses) a sampler of the TEST build of the library records --block + 1 ring slots with its own
iterations; then, in the same job, --inner calls per timed window, host clock around calls that end in a device
synchronise, median of --reps repetitions after one warm-up, all per state (slot):
  cv          DeviceCrossMoments.accumulate on the block: weight check, then per slot the evaluation of dE/dX, the finiteness
              check, the moment and covariance passes on the gradient, the moment pass on the state, the cross pass; one
              flag read-back per call
  cov         DeviceEstimator(want_cov=True).accumulate on the same block: what expectations(cov=True) adds to a run
  evaluation  the slot's evaluation launches alone (mjhmc_test_energy_observables_part, part 0: the same sampler_eval_rows)
  copy        a device-to-device slot copy (mjhmc_ring_copy: the slot read and written once)
cv - cov - evaluation is what the cross pass, the second moment pass and the finiteness check cost together: a difference
of host timings, not a kernel time (no profiler run here).
Writes one JSON line per workload; with --out also a markdown table.
usage: python tools/control_variates_bench.py [--only c2,c4,c3] [--block 4] [--reps 5] [--inner 3] [--n N] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from chainstats_bench import timed, repeated, copy_time                   # noqa: E402
from energy_observables_bench import hooks_device, rounded                # noqa: E402
from mjhmc_amd import engine                                              # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', default='c2,c4,c3')
    ap.add_argument('--block', type=int, default=4)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--inner', type=int, default=3, help='calls per timed window')
    ap.add_argument('--n', type=int, default=0, help='particles (default: the workload\'s)')
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    B = args.block
    recs = []
    for key in [k for k in args.only.split(',') if k]:
        ctx, dev, w, N = hooks_device(key, args.n, B + 1)
        lib = ctx.lib
        cm = dev.cross_moments()
        est = dev.estimator(True)
        eo = dev.energy_observables()
        eo.ring_alloc(1)

        def evaluation():
            engine.check(lib.mjhmc_test_energy_observables_part(eo.handle, 0, 1, 0, 0), lib)
            dev.sync()
        cm.accumulate(0, B, w_slot0=1)
        first = cm.read()
        cm.reset()
        cm.accumulate(0, B, w_slot0=1)
        assert all((a == b).all() if hasattr(a, 'all') else a == b for a, b in zip(first, cm.read())), 'two passes differ'
        t_cv = timed(repeated(lambda: cm.accumulate(0, B, w_slot0=1), args.inner), args.reps) / args.inner / B
        t_cov = timed(repeated(lambda: est.accumulate(0, B, w_slot0=1), args.inner), args.reps) / args.inner / B
        t_eval = timed(repeated(evaluation, args.inner), args.reps) / args.inner
        t_copy = copy_time(dev, B, args.reps, args.inner) / B
        rec = dict(workload=key, D=w['D'], N=N, dtype=w['dtype'], block=B, reps=args.reps, inner=args.inner,
                   cv_ms_per_state=1e3 * t_cv, cov_ms_per_state=1e3 * t_cov, evaluation_ms_per_state=1e3 * t_eval,
                   copy_ms_per_slot=1e3 * t_copy, rest_ms_per_state=1e3 * (t_cv - t_cov - t_eval), cv_over_copy=t_cv / t_copy,
                   cv_over_cov=t_cv / t_cov)
        recs.append(rec)
        print(rounded(rec), flush=True)
        for h in (cm, est, eo, dev):
            h.close()
        del dev
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('# Control variates: the pass per recorded state (tools/control_variates_bench.py)\n\n')
            f.write('One job on one MI355X; host clock around calls that end in a device synchronise, median of %d repetitions of '
                    '%d calls on a block of %d slots after a warm-up; every figure is per state (slot).  `cv` = '
                    'DeviceCrossMoments.accumulate (weight check; per slot the evaluation of dE/dX, the finiteness check, moments and '
                    'covariance of the gradient, moments of the state, the cross pass; one read-back per call); `cov` = '
                    'DeviceEstimator(want_cov=True).accumulate on the same block, what expectations(cov=True) adds to a run; '
                    '`evaluation` = the slot\'s evaluation launches alone; `copy` = a device-to-device slot copy; `rest` = cv - cov - '
                    'evaluation, the cross pass with the second moment pass and the finiteness check (a difference of host timings, not '
                    'a kernel time).  c3 is ProductOfT with float32 state: c3f64 runs the multi-pass path, which the handle refuses.\n\n'
                    % (args.reps, args.inner, B))
            f.write('| shape | ndims | particles | state | cv ms | cov ms | evaluation ms | copy ms | rest ms | cv / copy | cv / cov |\n')
            f.write('|---|---|---|---|---|---|---|---|---|---|---|\n')
            for r in recs:
                f.write('| %s | %d | %d | %s | %.3f | %.3f | %.3f | %.3f | %.3f | %.1f | %.2f |\n'
                        % (r['workload'], r['D'], r['N'], r['dtype'], r['cv_ms_per_state'], r['cov_ms_per_state'],
                           r['evaluation_ms_per_state'], r['copy_ms_per_slot'], r['rest_ms_per_state'], r['cv_over_copy'],
                           r['cv_over_cov']))
            f.write('\n```\n' + '\n'.join(json.dumps(r) for r in recs) + '\n```\n')


if __name__ == '__main__':
    main()
