"""Time the per-dimension lag-sum pass (csrc/lagcov.hip) against its yardsticks, per grid point, at the benchmark's sizes.

For each workload (c2: iso Gaussian 512 x 100 000 fp64; c4: Neal funnel 32 x 1 000 000 fp64; bench.py WORKLOADS), after one
recorded run of --slots iterations into the sample ring (a time grid has the ring's slot layout: the pass reads either the
same way):
  the pass            DeviceSampler.ring_lag_cov(0, slots, max_lag) for every max_lag of --lags (31: one band, one read of
                      the slots; 127: four bands), per slot
  a slot copy         mjhmc_ring_copy (read + write) in the same job: the yardstick of the pass.  The pass's byte rate counts
                      one read of the slots for band 0 and two reads of slots [k0, n) for every later band
  the NumPy path      ring_read of --host-slots slots as (ndims, nbatch, n) plus the same sums on the host, per slot: the
                      yardstick of the feature (the download alone is reported too)
Host clock around calls that end in a device synchronise; median of --reps repetitions after one warm-up.  One JSON line per
workload on stdout and a table in --out (default profiles/r12/lagcov.md).
usage: python tools/lagcov_bench.py [--only c2,c4] [--slots 128] [--lags 31,127] [--host-slots 8] [--reps 5] [--n N]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from chainstats_bench import make_sampler, timed, copy_time   # noqa: E402


def host_lag_sums(x, K):
    n = x.shape[2]
    u = x - x.mean(axis=(1, 2))[:, None, None]
    return np.array([np.sum(u[:, :, :n - k] * u[:, :, k:], axis=(1, 2)) for k in range(K + 1)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', default='c2,c4')
    ap.add_argument('--slots', type=int, default=128)
    ap.add_argument('--lags', default='31,127')
    ap.add_argument('--host-slots', type=int, default=8)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--n', type=int, default=0, help='particles (default: the workload\'s)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r12', 'lagcov.md'))
    args = ap.parse_args()
    lags = [int(k) for k in args.lags.split(',')]
    n = args.slots
    recs = []
    for key in args.only.split(','):
        smp, w, N = make_sampler(key, args.n)
        dev = smp._dev
        D = w['D']
        dev.ring_alloc(n + 1)                                   # (the live state ends in slot n: the copies never write it)
        slot_bytes = dev.ring_slot_bytes()
        Npad = (N + 63) // 64 * 64
        state_bytes = slot_bytes - 8 * Npad
        smp._run(n + 1, ring_slot0=0)
        dev.sync()
        rec = dict(workload=key, D=D, N=N, slots=n, reps=args.reps, state_bytes=state_bytes)
        t_copy = copy_time(dev, 8, args.reps, 4) / 8
        smp._run(n + 1, ring_slot0=0)                           # (the copies shifted slots: record the run again)
        dev.sync()
        rec['copy_ms_per_slot'] = 1e3 * t_copy
        rec['copy_GBps_read_plus_write'] = 2 * state_bytes / t_copy / 1e9
        shift = dev.ring_lag_cov(0, n, 0)[1] / (float(N) * n)
        for K in lags:
            K = min(K, n - 1)
            t = timed(lambda: dev.ring_lag_cov(0, n, K, shift=shift), args.reps)
            reads = n + sum(2 * (n - k0) for k0 in range(32, K + 1, 32))
            rec['pass_K%d_ms_per_slot' % K] = 1e3 * t / n
            rec['pass_K%d_GBps' % K] = reads * state_bytes / t / 1e9
            rec['pass_K%d_fraction_of_copy_rate' % K] = rec['pass_K%d_GBps' % K] / rec['copy_GBps_read_plus_write']
            rec['pass_K%d_fp64_TFLOPS' % K] = 2.0 * 32 * ((K + 32) // 32) * n * N * D / t / 1e12
        m = min(args.host_slots, n)
        t0 = time.perf_counter()
        x = dev.ring_read(0, m, stacked=True)
        t1 = time.perf_counter()
        host_lag_sums(x, m - 1)
        t2 = time.perf_counter()
        rec['numpy_slots'], rec['numpy_lags'] = m, m - 1
        rec['numpy_download_ms_per_slot'] = 1e3 * (t1 - t0) / m
        rec['numpy_sums_ms_per_slot'] = 1e3 * (t2 - t1) / m
        del x, smp, dev
        recs.append(rec)
        print(json.dumps({k: (round(v, 5) if isinstance(v, float) else v) for k, v in rec.items()}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('# Per-dimension lag sums (csrc/lagcov.hip): the pass per grid point\n\n')
        f.write('`python tools/lagcov_bench.py --slots %d --lags %s --host-slots %d --reps %d`; medians of %d repetitions.\n\n'
                % (n, args.lags, args.host_slots, args.reps, args.reps))
        for rec in recs:
            f.write('## %s: %d x %d, %d slots of %.1f MB\n\n' % (rec['workload'], rec['D'], rec['N'], n, rec['state_bytes'] / 1e6))
            f.write('| measure | value |\n|---|---|\n')
            for k, v in rec.items():
                if k not in ('workload', 'D', 'N', 'slots', 'reps', 'state_bytes'):
                    f.write('| %s | %s |\n' % (k, ('%.4g' % v) if isinstance(v, float) else v))
            f.write('\n')


if __name__ == '__main__':
    main()
